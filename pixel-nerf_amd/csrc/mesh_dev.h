// What the four mesh units (meshdist, winding, meshclean, meshraster) share.  No floating-point
// arithmetic beyond finite3's subtractions: where a unit's arithmetic rounds is stated by its own
// `#pragma clang fp contract(off)` region.  A kernel takes a helper from here only where it compiles
// to the instructions its own lines gave (tools/asm_equal.py); k_cc_flatten keeps its index test.
#pragma once
#include "pnr_common.h"

namespace pnr {

constexpr int64_t kMaxCount = 0x7fffffff;   // int32 indices

// x - x is 0 for a finite x and NaN for +-inf or NaN
__device__ __forceinline__ bool finite3(float x, float y, float z) {
    const float s = (x - x) + (y - y) + (z - z);
    return s == s;
}

// The vertex indices of face t (vertex k of it: verts + 3 * (size_t)i[k]); false when one lies
// outside [0, nv), a negative index being a large unsigned one: nothing may be read through them.
__device__ __forceinline__ bool face_indices(const int32_t *__restrict__ faces, size_t t, uint32_t nv, uint32_t i[3]) {
    i[0] = (uint32_t)faces[3 * t];
    i[1] = (uint32_t)faces[3 * t + 1];
    i[2] = (uint32_t)faces[3 * t + 2];
    return i[0] < nv && i[1] < nv && i[2] < nv;
}

// The one read-back of a launcher whose kernels check face indices: `bytes` from `src`, whose first
// int32 is the bad-index flag, after everything queued on `st`.  `fn`: the ABI function in the messages.
inline int read_index_flag(void *dst, const void *src, size_t bytes, hipStream_t st, int64_t n_verts, const char *fn,
                           const char *what) {
    if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(PNR_ERR_HIP, "%s: reading the %s failed: %s", fn, what, hipGetErrorString(hipGetLastError()));
    if (*static_cast<const int32_t *>(dst))
        return fail(PNR_ERR_INVALID, "%s: a face index lies outside [0, %lld)", fn, (long long)n_verts);
    return PNR_OK;
}

}  // namespace pnr
