"""Tensor-level wrappers over the C ABI (device tensors in, device tensors out).

Each wrapper validates device / dtype / contiguity, allocates outputs with torch
(the library never allocates), and launches on the current HIP stream.
"""
import ctypes

import torch

from . import _lib, torchops, util
from ._lib import call, ptr
from ._lib import workspace as _workspace


def _typed(t, name, dtype):
    """``t`` where it is a tensor of ``dtype`` on a HIP device; raises otherwise."""
    if not torch.is_tensor(t):
        raise TypeError("%s must be a tensor" % name)
    if t.device.type != "cuda":
        raise ValueError("pnr: %s must be on a HIP device (got %s); the HIP path has no CPU "
                         "fallback" % (name, t.device))
    if t.dtype != dtype:
        raise ValueError("pnr: %s must be %s (got %s)" % (name, str(dtype).replace("torch.", ""), t.dtype))
    return t


def _dev(t, name):
    return _typed(t, name, torch.float32).contiguous()


def _host_floats(values, n):
    """``values`` as a host ``float[n]`` (zero-filled past them), the void pointer the ABI takes."""
    return ctypes.cast((ctypes.c_float * n)(*values), ctypes.c_void_p)


def sample_coarse(rays, n_coarse, u_coarse, lindisp=False):
    """NeRFRenderer.sample_coarse (nerf.py:98-118): (B, 8), (B, Kc) -> z (B, Kc)."""
    rays = _dev(rays, "rays")
    u = _dev(u_coarse, "u_coarse")
    B = rays.shape[0]
    assert u.shape == (B, n_coarse), (u.shape, B, n_coarse)
    z = torch.empty(B, n_coarse, device=rays.device, dtype=torch.float32)
    call("pnr_sample_coarse", rays.device, ptr(rays), B, n_coarse, ptr(u), int(bool(lindisp)), ptr(z))
    return z


def sample_fine(rays, z_coarse, coarse_weights, coarse_depth, n_fine, n_fine_depth, depth_std,
                u_fine, u_fine_jit, n_depth, lindisp=False):
    """sample_fine + sample_fine_depth + cat + sort (nerf.py:120-161, 284-295).
    Returns the sorted fine-pass depths (B, Kc + Kf)."""
    rays = _dev(rays, "rays")
    zc = _dev(z_coarse, "z_coarse")
    w = _dev(coarse_weights, "coarse_weights")
    B, kc = zc.shape
    nf = n_fine - n_fine_depth
    d = _dev(coarse_depth, "coarse_depth") if n_fine_depth > 0 else None
    uf = _dev(u_fine, "u_fine") if nf > 0 else None
    uj = _dev(u_fine_jit, "u_fine_jit") if nf > 0 else None
    nd = _dev(n_depth, "n_depth") if n_fine_depth > 0 else None
    out = torch.empty(B, kc + n_fine, device=rays.device, dtype=torch.float32)
    call("pnr_sample_fine", rays.device, ptr(rays), B, kc, ptr(zc), ptr(w), ptr(d), n_fine, n_fine_depth,
         float(depth_std), ptr(uf), ptr(uj), ptr(nd), int(bool(lindisp)), ptr(out))
    return out


def composite(z, raw, rays, white_bkgd, want_weights=True):
    """Alpha composite (nerf.py:176-249): z (B, K), raw (B, K, 4) -> (weights, rgb, depth)."""
    z = _dev(z, "z")
    raw = _dev(raw, "raw")
    rays = _dev(rays, "rays")
    B, K = z.shape
    assert raw.shape[:2] == (B, K) and raw.shape[-1] == 4, raw.shape
    w, rgb, depth = torchops.load().composite(z, raw, rays, bool(white_bkgd), bool(want_weights))
    return (w if want_weights else None), rgb, depth


def rng_fill(seed, offset, stream, n_rays, width, device="cuda"):
    """The counter-mode draws of one stream (pnr_rng_fill; include/pnr_abi.h pnr_rng):
    (n_rays, width) for rays offset .. offset + n_rays - 1, exactly as the render kernels
    draw them in counter mode.  stream: _lib.RNG_U_COARSE .. RNG_N_DEPTH."""
    out = torch.empty(n_rays, width, device=device, dtype=torch.float32)
    call("pnr_rng_fill", out.device, int(seed), int(offset), int(stream), int(n_rays), int(width), ptr(out))
    return out


def rng_render_streams(seed, offset, n_rays, n_coarse, n_fine, n_fine_depth, device="cuda"):
    """(u_coarse, u_fine, u_fine_jit, n_depth) of a counter-mode render call, materialised."""
    nf = max(n_fine - n_fine_depth, 0)
    return (rng_fill(seed, offset, _lib.RNG_U_COARSE, n_rays, n_coarse, device),
            rng_fill(seed, offset, _lib.RNG_U_FINE, n_rays, nf, device),
            rng_fill(seed, offset, _lib.RNG_U_FINE_JIT, n_rays, nf, device),
            rng_fill(seed, offset, _lib.RNG_N_DEPTH, n_rays, n_fine_depth, device))


def marching_cubes(grid, level, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """Isosurface of a device grid (nx, ny, nz) at ``level`` (include/pnr_abi.h, "Isosurface
    extraction"; csrc/mcubes.hip): ``(verts (V, 3) float32, faces (T, 3) int32)`` on the grid's
    device, an indexed mesh as skimage.measure.marching_cubes / mcubes.marching_cubes return it
    (index units, normals towards lower values).  ``verts * spacing + origin`` is applied when either
    is given.  A level outside the grid's range returns two empty tensors.  One host sync here (the
    two counts size the outputs); pnr_mc_emit then waits for its own kernels."""
    grid = _dev(grid, "grid")
    if grid.dim() != 3:
        raise ValueError("pnr: grid must be (nx, ny, nz) (got %s)" % (tuple(grid.shape),))
    nx, ny, nz = (int(s) for s in grid.shape)
    if min(nx, ny, nz) < 1:
        raise ValueError("pnr: grid has an empty dimension %s" % (tuple(grid.shape),))
    dev = grid.device
    nbytes = _lib.load().pnr_mc_workspace_bytes(nx, ny, nz)
    ws = _workspace(nbytes, torch.uint8, dev, "pnr_mc_workspace_bytes: grid %s not supported (1 .. 1024 per axis)" % (
        tuple(grid.shape),))
    counts = torch.empty(2, device=dev, dtype=torch.int64)
    call("pnr_mc_count", dev, ptr(grid), nx, ny, nz, float(level), ptr(ws), nbytes, ptr(counts))
    n_v, n_t = (int(c) for c in counts.cpu())
    if n_v >= 2 ** 31 or n_t >= 2 ** 31:
        raise _lib.PnrError("marching_cubes: %d vertices / %d faces do not fit int32 indices" % (n_v, n_t))
    verts = torch.empty(n_v, 3, device=dev, dtype=torch.float32)
    faces = torch.empty(n_t, 3, device=dev, dtype=torch.int32)
    call("pnr_mc_emit", dev, ptr(grid), nx, ny, nz, float(level), ptr(ws), nbytes, ptr(verts) if n_v else None, n_v,
         ptr(faces) if n_t else None, n_t)
    if tuple(spacing) != (1.0, 1.0, 1.0) or tuple(origin) != (0.0, 0.0, 0.0):
        verts = verts * verts.new_tensor(spacing) + verts.new_tensor(origin)
    return verts, faces


# edge of the SSIM-map tile one workgroup of pnr_image_metrics scores (PNR_IMAGE_METRICS_TILE,
# include/pnr_abi.h): a (T + 6) x (T + 6) image is exactly one tile
IMAGE_METRICS_TILE = 16


def image_metrics(x, y, data_range=1.0, k1=0.01, k2=0.03):
    """PSNR and mean SSIM per image of two device stacks (include/pnr_abi.h, "Image metrics";
    csrc/metrics.hip): x, y (N, H, W, C) or (H, W, C) float32, channels last -> ``(psnr (N,),
    ssim (N,))`` float64 on their device.  The scores are those of ``evaluate.psnr_np`` /
    ``evaluate.ssim`` (skimage compare_psnr / compare_ssim(multichannel=True) defaults); psnr is
    +inf where the images are equal.  No host sync."""
    for t, name in ((x, "x"), (y, "y")):
        if not torch.is_tensor(t):
            raise TypeError("%s must be a tensor" % name)
    if y.device != x.device:
        raise ValueError("pnr: y is on %s, x on %s" % (y.device, x.device))
    if tuple(y.shape) != tuple(x.shape):
        raise ValueError("pnr: y has shape %s, x %s" % (tuple(y.shape), tuple(x.shape)))
    x = _dev(x, "x")
    y = _dev(y, "y")
    if x.dim() == 3:
        x, y = x[None], y[None]
    if x.dim() != 4:
        raise ValueError("pnr: x must be (N, H, W, C) or (H, W, C) (got %s)" % (tuple(x.shape),))
    n, h, w, c = (int(s) for s in x.shape)
    if not float(data_range) > 0.0:
        raise ValueError("pnr: data_range must be > 0 (got %r)" % (data_range,))
    if min(h, w) < 7:
        raise ValueError("pnr: x is %d x %d, smaller than the 7 x 7 SSIM window" % (h, w))
    if n < 1 or not 1 <= c <= 4:
        raise ValueError("pnr: x must hold at least one image of 1 .. 4 channels (got %s)" % (tuple(x.shape),))
    dev = x.device
    nbytes = _lib.load().pnr_image_metrics_workspace_bytes(n, h, w, c)
    ws = _workspace(nbytes, torch.float64, dev, "pnr_image_metrics_workspace_bytes: shape %s not supported (H, W <= "
                    "8192, fewer than 2^24 tiles)" % (tuple(x.shape),))
    out = torch.empty(n, 2, device=dev, dtype=torch.float64)
    call("pnr_image_metrics", dev, ptr(x), ptr(y), n, h, w, c, float(data_range), float(k1), float(k2), ptr(ws),
         nbytes, ptr(out))
    psnr = 10.0 * torch.log10(float(data_range) ** 2 / out[:, 0])
    return psnr, out[:, 1]


# tile constants of pnr_nearest (PNR_NEAREST_QUERIES / _TILE / _SLICE, include/pnr_abi.h): rows of a
# per workgroup, rows of b in LDS at a time, rows of b per workgroup; more than NEAREST_SLICE rows of
# b take the combine pass.  MESH_SCAN_CHUNK (PNR_MESH_SCAN_CHUNK): faces per chunk and chunks per
# group of pnr_mesh_sample's CDF.
NEAREST_QUERIES = 1024
NEAREST_TILE = 1024
NEAREST_SLICE = 4096
MESH_SCAN_CHUNK = 256


def _cloud(t, name, dtype=torch.float32):
    t = _typed(t, name, dtype)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("pnr: %s must be (N, 3) (got %s)" % (name, tuple(t.shape)))
    return t.contiguous()


def _same_device(**tensors):
    """Raises unless every named tensor (None: left out) is on the device of the first one."""
    (ref_name, ref), *rest = tensors.items()
    for name, t in rest:
        if t is not None and t.device != ref.device:
            raise ValueError("pnr: %s is on %s, %s on %s" % (name, t.device, ref_name, ref.device))


def _mesh(verts, faces, empty_msg):
    """The prologue of every wrapper that takes an indexed mesh: ``(verts, faces, V, T)`` from verts
    (V, 3) float32 and faces (T, 3) int32 on one HIP device, contiguous.  ``empty_msg`` ends the refusal
    of a mesh without vertices or faces ("... has no surface to sample"); None accepts one."""
    verts = _cloud(verts, "verts")
    faces = _cloud(faces, "faces", torch.int32)
    _same_device(verts=verts, faces=faces)
    n_v, n_t = int(verts.shape[0]), int(faces.shape[0])
    if empty_msg is not None and (n_v < 1 or n_t < 1):
        raise ValueError("pnr: an empty mesh (%d vertices, %d faces) %s" % (n_v, n_t, empty_msg))
    return verts, faces, n_v, n_t


def _seed(seed):
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError("pnr: seed must be in 0 .. 2^64 - 1 (got %r)" % (seed,))
    return int(seed)


def mesh_sample(verts, faces, n, seed=0, want_normals=True):
    """``n`` area-weighted samples of the surface of an indexed device mesh (include/pnr_abi.h,
    "Mesh metrics"; csrc/meshdist.hip): verts (V, 3) float32, faces (T, 3) int32 ->
    ``(points (n, 3), normals (n, 3) or None, tri (n,) int32, area)``, area a 0-dim float64 device
    tensor.  Sample s depends on (seed, s) only.  A face index outside [0, V) or a total area of 0
    raises.  One host sync (the library reads its index flag and the total before it samples)."""
    verts, faces, n_v, n_t = _mesh(verts, faces, "has no surface to sample")
    n = int(n)
    if n < 1:
        raise ValueError("pnr: n must be >= 1 (got %d)" % n)
    seed = _seed(seed)
    dev = verts.device
    nbytes = _lib.load().pnr_mesh_sample_workspace_bytes(n_t) if n < 2 ** 31 else 0
    ws = _workspace(nbytes, torch.float64, dev,
                    "pnr_mesh_sample: %d faces / %d samples not supported (below 2^31)" % (n_t, n))
    points = torch.empty(n, 3, device=dev, dtype=torch.float32)
    normals = torch.empty(n, 3, device=dev, dtype=torch.float32) if want_normals else None
    tri = torch.empty(n, device=dev, dtype=torch.int32)
    area = torch.empty((), device=dev, dtype=torch.float64)
    call("pnr_mesh_sample", dev, ptr(verts), n_v, ptr(faces), n_t, n, seed, ptr(ws), nbytes, ptr(points), ptr(normals),
         ptr(tri), ptr(area))
    return points, normals, tri, area


def nearest(a, b):
    """For every row of a (n, 3) the nearest row of b (m, 3), both float32 on one device
    (include/pnr_abi.h, "Mesh metrics"): ``(d2 (n,) float32, idx (n,) int32)``.  d2 is accumulated
    from the coordinate differences; equal distances resolve to the lowest index.  No host sync."""
    a = _cloud(a, "a")
    b = _cloud(b, "b")
    _same_device(a=a, b=b)
    n, m = int(a.shape[0]), int(b.shape[0])
    if n < 1 or m < 1:
        raise ValueError("pnr: a and b must hold at least one point each (got %d, %d)" % (n, m))
    dev = a.device
    nbytes = _lib.load().pnr_nearest_workspace_bytes(n, m)
    ws = _workspace(nbytes, torch.float32, dev, "pnr_nearest_workspace_bytes: %d x %d points not supported (n < 2^31, "
                    "m <= 65535 * %d)" % (n, m, NEAREST_SLICE))
    d2 = torch.empty(n, device=dev, dtype=torch.float32)
    idx = torch.empty(n, device=dev, dtype=torch.int32)
    call("pnr_nearest", dev, ptr(a), n, ptr(b), m, ptr(ws), nbytes, ptr(d2), ptr(idx))
    return d2, idx


MESH_DISTANCE_KEYS = ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "precision", "recall", "fscore",
                      "normals_accuracy", "normals_completeness", "normal_consistency")


def mesh_distance_sums(d2_ab, idx_ab, d2_ba, idx_ba, na, nb, tau):
    """The eight float64 sums of pnr_mesh_distance_reduce as one device tensor (8,)."""
    dev = d2_ab.device
    out = torch.empty(8, device=dev, dtype=torch.float64)
    call("pnr_mesh_distance_reduce", dev, ptr(d2_ab), ptr(idx_ab), int(d2_ab.shape[0]), ptr(d2_ba), ptr(idx_ba),
         int(d2_ba.shape[0]), ptr(na), ptr(nb), float(tau), ptr(out))
    return out


def mesh_distance(pa, na, pb, nb, tau):
    """Scores of a predicted cloud pa (n, 3) against a ground-truth cloud pb (m, 3) as Occupancy
    Networks' eval_pointcloud defines them: a dict of 0-dim float64 device tensors.  accuracy /
    completeness: mean distance pa -> pb / pb -> pa; chamfer_l1 their mean; chamfer_l2 the mean of
    the two directions' mean SQUARED distances;
    precision / recall: the share of pa / pb nearer than ``tau``; fscore = 2PR / (P + R), 0 where
    P + R = 0; normals_* the mean |n . n'| with the nearest neighbour (na, nb: unit normals of the
    two clouds, or both None: the normal terms are then 0).  No host sync."""
    pa = _cloud(pa, "pa")
    pb = _cloud(pb, "pb")
    if (na is None) != (nb is None):
        raise ValueError("pnr: give the normals of both clouds, or of neither")
    if na is not None:
        na = _cloud(na, "na")
        nb = _cloud(nb, "nb")
        if tuple(na.shape) != tuple(pa.shape) or tuple(nb.shape) != tuple(pb.shape):
            raise ValueError("pnr: normals must match their points (got %s for %s, %s for %s)" % (
                tuple(na.shape), tuple(pa.shape), tuple(nb.shape), tuple(pb.shape)))
    _same_device(pa=pa, pb=pb, na=na, nb=nb)
    if not float(tau) >= 0.0:
        raise ValueError("pnr: tau must be >= 0 (got %r)" % (tau,))
    n, m = int(pa.shape[0]), int(pb.shape[0])
    if n < 1 or m < 1:
        raise ValueError("pnr: pa and pb must hold at least one point each (got %d, %d)" % (n, m))
    d2_ab, idx_ab = nearest(pa, pb)
    d2_ba, idx_ba = nearest(pb, pa)
    return scores_from_sums(mesh_distance_sums(d2_ab, idx_ab, d2_ba, idx_ba, na, nb, tau), n, m)


def scores_from_sums(s, n, m):
    """The score dict from the eight sums (a device tensor of 8 float64) and the two counts."""
    acc, acc2, prec, nacc = s[0] / n, s[1] / n, s[2] / n, s[3] / n
    comp, comp2, rec, ncomp = s[4] / m, s[5] / m, s[6] / m, s[7] / m
    pr = prec + rec
    f = torch.where(pr > 0, 2.0 * prec * rec / torch.where(pr > 0, pr, torch.ones_like(pr)), torch.zeros_like(pr))
    return {"accuracy": acc, "completeness": comp, "chamfer_l1": 0.5 * (acc + comp), "chamfer_l2": 0.5 * (acc2 + comp2),
            "precision": prec, "recall": rec, "fscore": f, "normals_accuracy": nacc, "normals_completeness": ncomp,
            "normal_consistency": 0.5 * (nacc + ncomp)}


# tile constants of pnr_winding (PNR_WINDING_QUERIES / _TILE / _SLICE, include/pnr_abi.h): queries per
# workgroup, faces in LDS at a time, faces per workgroup; more than WINDING_SLICE faces take the
# combine pass.
WINDING_QUERIES = 512
WINDING_TILE = 512
WINDING_SLICE = 4096


def winding_number(verts, faces, points):
    """Generalized winding number of an indexed device mesh at every query point (include/pnr_abi.h,
    "Mesh containment"; csrc/winding.hip): verts (V, 3) float32, faces (T, 3) int32, points (n, 3)
    float32 -> ``w (n,) float64``.  1 inside and 0 outside a closed mesh with outward faces (the
    orientation ``marching_cubes`` gives density blobs), a fraction near the holes of an open one.
    The pairs are scored in fp32 and summed in fp64 in a fixed order: ``w[i]`` depends on
    ``points[i]`` and the mesh only.  A face with an index outside [0, V) contributes 0; a
    non-finite query gives NaN.  No host sync."""
    verts, faces, n_v, n_t = _mesh(verts, faces, "contains nothing")
    points = _cloud(points, "points")
    _same_device(verts=verts, points=points)
    n = int(points.shape[0])
    if n < 1:
        raise ValueError("pnr: points must hold at least one point (got %d)" % n)
    dev = verts.device
    nbytes = _lib.load().pnr_winding_workspace_bytes(n, n_t) if n_v < 2 ** 31 else 0
    ws = _workspace(nbytes, torch.float64, dev, "pnr_winding_workspace_bytes: %d points x %d faces not supported "
                    "(n < 2^31, faces <= min(2^31 - 1, 65535 * %d))" % (n, n_t, WINDING_SLICE))
    w = torch.empty(n, device=dev, dtype=torch.float64)
    call("pnr_winding", dev, ptr(verts), n_v, ptr(faces), n_t, ptr(points), n, ptr(ws), nbytes, ptr(w))
    return w


def mesh_contains(verts, faces, points, thresh=0.5):
    """``winding_number(...) > thresh`` as a bool tensor (n,): which points the mesh contains.  A
    non-finite point is outside."""
    return winding_number(verts, faces, points) > thresh


def box_sample(lo, hi, n, seed=0, device="cuda"):
    """``n`` points uniform in the box [lo, hi] (two triples of floats) as a float32 device tensor
    (n, 3): pnr_box_sample (include/pnr_abi.h, "Mesh containment").  Sample s depends on (seed, s)
    only, so the first rows of a longer call equal a shorter one."""
    lo, hi = [float(x) for x in lo], [float(x) for x in hi]
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("pnr: lo and hi must be triples (got %d, %d values)" % (len(lo), len(hi)))
    n = int(n)
    if n < 1:
        raise ValueError("pnr: n must be >= 1 (got %d)" % n)
    seed = _seed(seed)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("pnr: box_sample draws on a HIP device (got %s); the HIP path has no CPU fallback" % (dev,))
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    points = torch.empty(n, 3, device=dev, dtype=torch.float32)
    call("pnr_box_sample", dev, _host_floats(lo, 3), _host_floats(hi, 3), n, seed, ptr(points))
    return points


# constants of pnr_mesh_raster (PNR_RASTER_*, include/pnr_abi.h): (view, face) lanes per workgroup,
# the side of the pixel block a wave tests per step of a large face, the largest pixel bounds one
# lane scans on its own, the most point lights of pnr_mesh_shade
RASTER_BLOCK = 256
RASTER_TILE = 8
RASTER_SMALL_PIXELS = 8
RASTER_MAX_LIGHTS = 8


def _raster_args(verts, faces, poses, width, height, focal, c, want_ws):
    """What mesh_raster and mesh_shade check and refuse alike; the last two entries are mesh_raster's
    workspace (``want_ws``; mesh_shade takes none) and its size."""
    verts, faces, n_v, n_t = _mesh(verts, faces, "renders nothing")
    poses = _typed(poses, "poses", torch.float32)
    if poses.dim() != 3 or poses.shape[1] not in (3, 4) or poses.shape[2] != 4:
        raise ValueError("pnr: poses must be (NV, 4, 4) or (NV, 3, 4) (got %s)" % (tuple(poses.shape),))
    poses = poses.contiguous()
    _same_device(verts=verts, poses=poses)
    nv = int(poses.shape[0])
    if nv < 1:
        raise ValueError("pnr: poses must hold at least one view (got %d)" % nv)
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError("pnr: width and height must be >= 1 (got %d, %d)" % (width, height))
    fx, fy, cx, cy = util._focal_c(width, height, focal, c)
    nbytes = _lib.load().pnr_mesh_raster_workspace_bytes(nv, height, width, n_t) if n_v < 2 ** 31 else 0
    ws = _workspace(nbytes, torch.int64, verts.device if want_ws else None,
                    "pnr_mesh_raster_workspace_bytes: %d views of %d x %d with %d faces not supported (sides "
                    "in 1 .. 8192, NV H W and faces below 2^31)" % (nv, width, height, n_t))
    return verts, faces, poses, nv, n_v, n_t, width, height, fx, fy, cx, cy, ws, nbytes


def mesh_raster(verts, faces, poses, width, height, focal, c=None):
    """Nearest face and depth of an indexed device mesh for every pixel of a batch of cameras
    (include/pnr_abi.h, "Mesh rendering"; csrc/meshraster.hip): verts (V, 3) float32, faces (T, 3)
    int32, poses (NV, 4, 4) or (NV, 3, 4) float32 camera-to-world in the loader's convention ->
    ``(face (NV, H, W) int32, depth (NV, H, W) float32)``.  Pixel [v, j, i] is ray [v, j, i] of
    ``util.gen_rays(poses, width, height, focal, ., ., c)``; ``face`` is -1 and ``depth`` 0 where the
    ray hits nothing, else ``depth`` is the distance along the unit direction (the composite's
    depth).  Both are functions of the inputs alone, bit for bit.  No host sync."""
    verts, faces, poses, nv, n_v, n_t, width, height, fx, fy, cx, cy, ws, nbytes = _raster_args(
        verts, faces, poses, width, height, focal, c, True)
    dev = verts.device
    face = torch.empty(nv, height, width, device=dev, dtype=torch.int32)
    depth = torch.empty(nv, height, width, device=dev, dtype=torch.float32)
    call("pnr_mesh_raster", dev, ptr(verts), n_v, ptr(faces), n_t, ptr(poses), nv, int(poses.shape[1]), width, height,
         fx, fy, cx, cy, ptr(ws), nbytes, ptr(face), ptr(depth))
    return face, depth


class raster_small_pixels(_lib._restored):
    """Context manager: pnr_mesh_raster_set_small(pixels) inside, the previous value restored after.
    It moves the threshold between the lane path and the wave path of ``mesh_raster`` (measurements
    and tests; the outputs do not depend on it)."""
    setter = "pnr_mesh_raster_set_small"

    def __init__(self, pixels):
        self.value = int(pixels)


def mesh_shade(verts, faces, poses, width, height, focal, face, depth, c=None, lights=(), weights=(),
               albedo=(0.8, 0.8, 0.8), ambient=0.2, background=(1.0, 1.0, 1.0), want_normal=False):
    """Flat-shaded colour of ``mesh_raster``'s pixels (include/pnr_abi.h, "Mesh rendering", Shading):
    ``rgb (NV, H, W, 3) float32`` channels-last (the layout ``image_metrics`` takes), and with
    ``want_normal`` the unit face normals turned towards the camera ``(NV, H, W, 3)`` (else None).
    ``lights``: up to RASTER_MAX_LIGHTS world positions (triples), ``weights`` one float each;
    ``albedo`` and ``background`` triples; colours of covered pixels are clamped to [0, 254/255]."""
    verts, faces, poses, nv, n_v, n_t, width, height, fx, fy, cx, cy, _, _ = _raster_args(
        verts, faces, poses, width, height, focal, c, False)
    dev = verts.device
    for t, name, dtype in ((face, "face", torch.int32), (depth, "depth", torch.float32)):
        if tuple(_typed(t, name, dtype).shape) != (nv, height, width):
            raise ValueError("pnr: %s must be %s (got %s)" % (name, (nv, height, width), tuple(t.shape)))
    _same_device(verts=verts, face=face, depth=depth)
    lights = [[float(x) for x in l] for l in lights]
    weights = [float(x) for x in weights]
    if len(lights) != len(weights) or len(lights) > RASTER_MAX_LIGHTS or any(len(l) != 3 for l in lights):
        raise ValueError("pnr: lights must be at most %d triples with one weight each (got %d lights, %d weights)"
                         % (RASTER_MAX_LIGHTS, len(lights), len(weights)))
    albedo, background = [float(x) for x in albedo], [float(x) for x in background]
    if len(albedo) != 3 or len(background) != 3:
        raise ValueError("pnr: albedo and background must be triples")
    n_l = len(lights)
    face, depth = face.contiguous(), depth.contiguous()
    rgb = torch.empty(nv, height, width, 3, device=dev, dtype=torch.float32)
    normal = torch.empty(nv, height, width, 3, device=dev, dtype=torch.float32) if want_normal else None
    call("pnr_mesh_shade", dev, ptr(verts), n_v, ptr(faces), n_t, ptr(poses), nv, int(poses.shape[1]), width, height,
         fx, fy, cx, cy, ptr(face), ptr(depth), _host_floats([x for l in lights for x in l], max(1, 3 * n_l)),
         _host_floats(weights, max(1, n_l)), n_l, _host_floats(albedo, 3), float(ambient), _host_floats(background, 3),
         ptr(rgb), ptr(normal))
    return rgb, normal


# workgroup size of the weld / component kernels (PNR_MESH_CLEAN_BLOCK, include/pnr_abi.h): one
# thread per vertex or face, so sizes around a multiple of it exercise the partial last workgroup
MESH_CLEAN_BLOCK = 256
COMPONENT_STAT_KEYS = ("labels", "vert_id", "face_id", "n_verts", "n_faces", "area", "signed_volume")


def mesh_weld_remap(verts):
    """``remap (V,) int32`` of pnr_mesh_weld (include/pnr_abi.h, "Mesh cleanup"; csrc/meshclean.hip):
    remap[i] is the lowest index whose vertex has the same three coordinates as vertex i (-0.0 equals
    +0.0; a vertex with a NaN coordinate maps to itself).  No host sync."""
    verts = _cloud(verts, "verts")
    n_v = int(verts.shape[0])
    dev = verts.device
    if n_v == 0:
        return torch.empty(0, device=dev, dtype=torch.int32)
    nbytes = _lib.load().pnr_mesh_weld_workspace_bytes(n_v)
    ws = _workspace(nbytes, torch.int32, dev,
                    "pnr_mesh_weld_workspace_bytes: %d vertices not supported (1 .. 2^29)" % n_v)
    remap = torch.empty(n_v, device=dev, dtype=torch.int32)
    call("pnr_mesh_weld", dev, ptr(verts), n_v, ptr(ws), nbytes, ptr(remap))
    return remap


def mesh_weld(verts, faces):
    """Merge equal vertices of a device mesh (an STL soup, say): verts (V, 3) float32, faces (T, 3)
    int32 -> ``(verts' (V', 3), faces' (T, 3) int32, remap (V,) int32)``.  ``remap`` is
    ``mesh_weld_remap``'s, in ORIGINAL indices; verts' are the vertices with remap[i] == i in ascending
    original order and faces' the same T rows re-indexed into them: no face is dropped, degenerate
    ones included, so row t still is record t of the STL.  One host sync (V' sizes the output)."""
    verts, faces, n_v, _ = _mesh(verts, faces, None)   # an empty mesh welds to itself
    remap = mesh_weld_remap(verts)
    keep = remap == torch.arange(n_v, device=verts.device, dtype=torch.int32)
    new_index = torch.cumsum(keep, 0, dtype=torch.int64) - 1
    if faces.numel() and n_v:
        f = faces.long()
        if bool(((f < 0) | (f >= n_v)).any()):
            raise ValueError("pnr: a face index lies outside [0, %d)" % n_v)
        faces = new_index[remap.long()[f]].to(torch.int32)
    elif faces.numel():
        raise ValueError("pnr: faces over an empty vertex set")
    return verts[keep], faces.contiguous(), remap


def mesh_components(verts_or_n, faces, return_launches=False):
    """Connected components of an indexed device mesh (include/pnr_abi.h, "Mesh cleanup"): faces (T, 3)
    int32 over V vertices (``verts_or_n``: the (V, 3) vertex tensor, or V itself) ->
    ``(vert_label (V,) int32, face_label (T,) int32, n_components)``.  Two vertices are connected when
    a face names both; a label is the lowest vertex index of the component, and a vertex no face names
    is a component of its own.  A face index outside [0, V) raises.  ``return_launches`` appends the
    number of kernel launches the library took.  Two host syncs (the library's index flag, and the
    count)."""
    faces = _cloud(faces, "faces", torch.int32)
    n_v = int(verts_or_n.shape[0]) if torch.is_tensor(verts_or_n) else int(verts_or_n)
    if n_v < 0:
        raise ValueError("pnr: the number of vertices must be >= 0 (got %d)" % n_v)
    n_t = int(faces.shape[0])
    dev = faces.device
    if n_v == 0:
        if n_t:
            raise ValueError("pnr: faces over an empty vertex set")
        out = (torch.empty(0, device=dev, dtype=torch.int32), torch.empty(0, device=dev, dtype=torch.int32), 0)
        return out + (0,) if return_launches else out
    nbytes = _lib.load().pnr_mesh_components_workspace_bytes(n_v, n_t)
    ws = _workspace(nbytes, torch.int32, dev, "pnr_mesh_components_workspace_bytes: %d vertices / %d faces not "
                    "supported (below 2^31)" % (n_v, n_t))
    vert_label = torch.empty(n_v, device=dev, dtype=torch.int32)
    face_label = torch.empty(n_t, device=dev, dtype=torch.int32)
    launches = ctypes.c_int32(0)
    call("pnr_mesh_components", dev, ptr(faces) if n_t else None, n_t, n_v, ptr(ws), nbytes, ptr(vert_label),
         ptr(face_label) if n_t else None, ctypes.byref(launches))
    n_c = int((vert_label == torch.arange(n_v, device=dev, dtype=torch.int32)).sum())
    out = (vert_label, face_label, n_c)
    return out + (int(launches.value),) if return_launches else out


def mesh_component_stats(verts, faces, vert_label, face_label):
    """Per-component statistics of a labelled device mesh (``mesh_components``' labels) as a dict of
    device tensors (COMPONENT_STAT_KEYS): ``labels`` (C,) int32 ascending, the dense id c = 0 .. C - 1
    of a component being its label's rank; ``vert_id`` (V,) / ``face_id`` (T,) int64 dense ids;
    ``n_verts`` / ``n_faces`` (C,) int64, exact; ``area`` / ``signed_volume`` (C,) float64
    (pnr_mesh_component_sums: per-face terms in fp64 from the fp32 vertices, summed in a fixed order
    that depends on the component's own faces only, so a component's sums are bit-identical from run
    to run and inside any larger mesh).  The faces are grouped by component with a stable sort; the
    counts are integer bincounts.  One host sync (C)."""
    verts, faces, n_v, n_t = _mesh(verts, faces, None)   # no faces: every component's sums are 0
    dev = verts.device
    for t, name, n in ((vert_label, "vert_label", n_v), (face_label, "face_label", n_t)):
        if not torch.is_tensor(t) or t.dtype != torch.int32 or tuple(t.shape) != (n,) or t.device != dev:
            raise ValueError("pnr: %s must be an int32 tensor of shape (%d,) on %s" % (name, n, dev))
    labels = torch.unique(vert_label)   # sorted ascending
    n_c = int(labels.shape[0])
    vert_id = torch.searchsorted(labels, vert_label)
    face_id = torch.searchsorted(labels, face_label)
    cnt_v = torch.bincount(vert_id, minlength=n_c)
    cnt_f = torch.bincount(face_id, minlength=n_c)
    sums = torch.zeros(n_c, 2, device=dev, dtype=torch.float64)
    if n_t and n_c:
        order = torch.sort(face_id, stable=True).indices.contiguous()
        seg = torch.zeros(n_c + 1, device=dev, dtype=torch.int64)
        seg[1:] = torch.cumsum(cnt_f, 0)
        call("pnr_mesh_component_sums", dev, ptr(verts), n_v, ptr(faces), n_t, ptr(order), ptr(seg), n_c, ptr(sums))
    return {"labels": labels, "vert_id": vert_id, "face_id": face_id, "n_verts": cnt_v, "n_faces": cnt_f,
            "area": sums[:, 0].contiguous(), "signed_volume": sums[:, 1].contiguous()}
