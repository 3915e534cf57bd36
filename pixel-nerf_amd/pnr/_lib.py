"""ctypes binding of libpnr.so (include/pnr_abi.h).

The product path has no fallback: if the HIP library is missing or fails to load,
every call raises.  ``torch`` is imported first so that the HIP runtime torch
ships (soname libamdhip64.so.7) is the one libpnr.so binds to.
"""
import ctypes
import os

import torch  # noqa: F401  (load torch's HIP runtime before libpnr.so)

_HERE = os.path.dirname(os.path.abspath(__file__))
# PNR_LIB_PATH: alternate build (diagnostic ablation builds only)
LIB_PATH = os.environ.get("PNR_LIB_PATH") or os.path.join(_HERE, "libpnr.so")

c_f = ctypes.c_float
c_i32 = ctypes.c_int32
c_i64 = ctypes.c_int64
c_size = ctypes.c_size_t
c_vp = ctypes.c_void_p
PF = ctypes.POINTER(ctypes.c_float)


class Scene(ctypes.Structure):
    _fields_ = [("latent", c_vp), ("cams", c_vp), ("n_obj", c_i32), ("n_views", c_i32),
                ("latent_h", c_i32), ("latent_w", c_i32), ("latent_c", c_i32),
                ("image_w", c_f), ("image_h", c_f)]


class MlpDesc(ctypes.Structure):
    _fields_ = [("d_in", c_i32), ("d_latent", c_i32), ("d_hidden", c_i32), ("d_out", c_i32),
                ("n_blocks", c_i32), ("combine_layer", c_i32), ("pe_n", c_i32),
                ("precision", c_i32)]


class MlpWeights(ctypes.Structure):
    _fields_ = [("desc", MlpDesc), ("lin_in_w", c_vp), ("lin_in_b", c_vp),
                ("lin_z_w", c_vp * 8), ("lin_z_b", c_vp * 8),
                ("fc0_w", c_vp * 8), ("fc0_b", c_vp * 8),
                ("fc1_w", c_vp * 8), ("fc1_b", c_vp * 8),
                ("lin_out_w", c_vp), ("lin_out_b", c_vp),
                ("pe_freqs", c_vp), ("pe_phases", c_vp)]


class Rays(ctypes.Structure):
    _fields_ = [("rays", c_vp), ("n_rays", c_i64), ("rays_per_obj", c_i64)]


class Rng(ctypes.Structure):
    """Injected streams, or counter mode (Philox {seed, offset}) when all four are NULL."""
    _fields_ = [("u_coarse", c_vp), ("u_fine", c_vp), ("u_fine_jit", c_vp), ("n_depth", c_vp),
                ("seed", ctypes.c_uint64), ("offset", ctypes.c_uint64)]


# pnr_rng counter-mode stream ids (PNR_RNG_*)
RNG_U_COARSE, RNG_U_FINE, RNG_U_FINE_JIT, RNG_N_DEPTH = 0, 1, 2, 3
RNG_MESH = 4   # PNR_RNG_MESH: the surface-sampling draws of pnr_mesh_sample (not a pnr_rng_fill stream)
RNG_VOLUME = 5   # PNR_RNG_VOLUME: the box-sample draws of pnr_box_sample (not a pnr_rng_fill stream)
ABI_VERSION = 8


class RenderCfg(ctypes.Structure):
    _fields_ = [("n_coarse", c_i32), ("n_fine", c_i32), ("n_fine_depth", c_i32),
                ("depth_std", c_f), ("white_bkgd", c_i32), ("lindisp", c_i32),
                ("march_mode", c_i32),   # ABI 3: -1 = the pnr_render_set_fused default
                ("ray_order", c_vp)]     # ABI 8: the fused march's processing order (NULL: input order)


class RenderOut(ctypes.Structure):
    _fields_ = [("coarse_rgb", c_vp), ("coarse_depth", c_vp), ("coarse_weights", c_vp),
                ("fine_rgb", c_vp), ("fine_depth", c_vp), ("fine_weights", c_vp),
                ("z_coarse", c_vp), ("z_fine", c_vp)]


# name -> (restype, argtypes); must match include/pnr_abi.h exactly
SIGNATURES = {
    "pnr_abi_version": (c_i32, []),
    "pnr_last_error": (ctypes.c_char_p, []),
    "pnr_mlp_packed_bytes": (c_size, [ctypes.POINTER(MlpDesc)]),
    "pnr_mlp_pack": (c_i32, [ctypes.POINTER(MlpWeights), c_vp, c_size, c_vp]),
    "pnr_point_query_workspace_bytes": (c_size, [ctypes.POINTER(Scene), c_i64]),
    "pnr_point_query": (c_i32, [ctypes.POINTER(Scene), ctypes.POINTER(MlpDesc), c_vp, c_vp, c_vp,
                                c_i64, c_vp, c_vp, c_size, c_vp]),
    "pnr_render_workspace_bytes": (c_size, [ctypes.POINTER(Scene), ctypes.POINTER(RenderCfg), c_i64]),
    "pnr_render_forward": (c_i32, [ctypes.POINTER(Scene), ctypes.POINTER(MlpDesc), c_vp, c_vp,
                                   ctypes.POINTER(Rays), ctypes.POINTER(Rng),
                                   ctypes.POINTER(RenderCfg), ctypes.POINTER(RenderOut), c_vp,
                                   c_size, c_vp]),
    "pnr_render_forward_events": (c_i32, [ctypes.POINTER(Scene), ctypes.POINTER(MlpDesc), c_vp, c_vp,
                                          ctypes.POINTER(Rays), ctypes.POINTER(Rng),
                                          ctypes.POINTER(RenderCfg), ctypes.POINTER(RenderOut),
                                          c_vp, c_size, c_vp, ctypes.POINTER(c_vp)]),
    "pnr_latent_project_bytes": (c_size, [ctypes.POINTER(Scene), ctypes.POINTER(MlpDesc)]),
    "pnr_latent_project": (c_i32, [ctypes.POINTER(Scene), ctypes.POINTER(MlpWeights), c_vp, c_size, c_vp]),
    "pnr_point_query_proj": (c_i32, [ctypes.POINTER(Scene), ctypes.POINTER(MlpDesc), c_vp, c_vp, c_vp, c_vp,
                                     c_i64, c_vp, c_vp, c_size, c_vp]),
    "pnr_render_forward_proj": (c_i32, [ctypes.POINTER(Scene), ctypes.POINTER(MlpDesc), c_vp, c_vp, c_vp, c_vp,
                                        ctypes.POINTER(Rays), ctypes.POINTER(Rng),
                                        ctypes.POINTER(RenderCfg), ctypes.POINTER(RenderOut),
                                        c_vp, c_size, c_vp, ctypes.POINTER(c_vp)]),
    "pnr_render_set_fused": (c_i32, [c_i32]),
    "pnr_mlp_set_lean": (c_i32, [c_i32]),
    "pnr_mlp_last_kernel": (c_i32, []),
    "pnr_sample_coarse": (c_i32, [c_vp, c_i64, c_i32, c_vp, c_i32, c_vp, c_vp]),
    "pnr_sample_fine": (c_i32, [c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_i32, c_i32, c_f, c_vp,
                                c_vp, c_vp, c_i32, c_vp, c_vp]),
    "pnr_composite": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "pnr_rng_fill": (c_i32, [ctypes.c_uint64, ctypes.c_uint64, c_i32, c_i64, c_i32, c_vp, c_vp]),
    "pnr_gen_rays": (c_i32, [c_vp, c_i64, c_i32, c_i32, c_i32, c_f, c_f, c_f, c_f, c_f, c_f, c_vp, c_vp]),
    "pnr_latent_channels_last": (c_i32, [ctypes.POINTER(c_vp), ctypes.POINTER(c_i32), ctypes.POINTER(c_i32),
                                         ctypes.POINTER(c_i32), c_i32, c_i32, c_vp, c_i32, c_i32, c_vp]),
    "pnr_latent_channels_last_nhwc": (c_i32, [ctypes.POINTER(c_vp), ctypes.POINTER(c_i32), ctypes.POINTER(c_i32),
                                              ctypes.POINTER(c_i32), c_i32, c_i32, c_vp, c_i32, c_i32, c_vp]),
    "pnr_fold_batchnorm": (c_i32, [c_vp, c_i32, c_i64, c_vp]),
    "pnr_latent_channels_last_backward": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "pnr_point_save_floats": (c_size, [ctypes.POINTER(MlpDesc), c_i64]),
    "pnr_render_points": (c_i32, [ctypes.POINTER(Scene), ctypes.POINTER(MlpDesc), c_vp,
                                  ctypes.POINTER(Rays), c_vp, c_i32, c_vp, c_vp, c_vp, c_size, c_vp]),
    "pnr_composite_backward": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp,
                                       c_vp, c_vp]),
    "pnr_points_input_backward": (c_i32, [ctypes.POINTER(Scene), ctypes.POINTER(MlpDesc), c_vp,
                                          ctypes.POINTER(Rays), c_vp, c_i32, c_vp, c_vp, c_vp, c_vp,
                                          c_vp]),
    "pnr_points_input_backward_masked": (c_i32, [ctypes.POINTER(Scene), ctypes.POINTER(MlpDesc), c_vp,
                                                 ctypes.POINTER(Rays), c_vp, c_i32, c_vp, c_vp, c_vp, c_vp,
                                                 c_vp, c_vp]),
    "pnr_mlp_packed_t_bytes": (c_size, [ctypes.POINTER(MlpDesc)]),
    "pnr_mlp_pack_t": (c_i32, [ctypes.POINTER(MlpWeights), c_vp, c_vp, c_size, c_vp]),
    "pnr_mlp_backward": (c_i32, [ctypes.POINTER(MlpDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp,
                                 c_vp]),
    "pnr_mlp_backward_workspace_bytes": (c_size, [ctypes.POINTER(MlpDesc), c_i64]),
    "pnr_mlp_backward_bias": (c_i32, [ctypes.POINTER(MlpDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp,
                                      c_vp, c_vp, c_size, c_vp]),
    "pnr_mlp_backward_views": (c_i32, [ctypes.POINTER(MlpDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_vp,
                                       c_vp, c_vp, c_vp, c_size, c_vp]),
    "pnr_weight_grad_workspace_bytes": (c_size, [c_i32, c_i64]),
    "pnr_weight_grad": (c_i32, [ctypes.POINTER(c_vp), ctypes.POINTER(c_vp), ctypes.POINTER(c_vp), c_i32, c_i64,
                                c_vp, c_size, c_vp]),
    "pnr_weight_grad_arith": (c_i32, [ctypes.POINTER(c_vp), ctypes.POINTER(c_vp), ctypes.POINTER(c_vp), c_i32,
                                      c_i64, c_i32, c_vp, c_size, c_vp]),
    # isosurface extraction (csrc/mcubes.hip); pnr_mc_case_table is host-only
    "pnr_mc_workspace_bytes": (c_size, [c_i32, c_i32, c_i32]),
    "pnr_mc_count": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_f, c_vp, c_size, c_vp, c_vp]),
    "pnr_mc_emit": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_f, c_vp, c_size, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "pnr_mc_case_table": (c_i32, [c_vp]),
    # per-image MSE / SSIM (csrc/metrics.hip); out is float64
    "pnr_image_metrics_workspace_bytes": (c_size, [c_i64, c_i32, c_i32, c_i32]),
    "pnr_image_metrics": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_f, c_f, c_f, c_vp, c_size, c_vp, c_vp]),
    # mesh metrics (csrc/meshdist.hip); total_area and out are float64, faces / tri / idx int32
    "pnr_mesh_sample_workspace_bytes": (c_size, [c_i64]),
    "pnr_mesh_sample": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_i64, ctypes.c_uint64, c_vp, c_size, c_vp, c_vp, c_vp,
                                c_vp, c_vp]),
    "pnr_nearest_workspace_bytes": (c_size, [c_i64, c_i64]),
    "pnr_nearest": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_size, c_vp, c_vp, c_vp]),
    "pnr_mesh_distance_reduce": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, ctypes.c_double, c_vp,
                                         c_vp]),
    # mesh containment (csrc/winding.hip); w is float64, lo / hi of pnr_box_sample are host float[3]
    "pnr_winding_workspace_bytes": (c_size, [c_i64, c_i64]),
    "pnr_winding": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_size, c_vp, c_vp]),
    "pnr_box_sample": (c_i32, [c_vp, c_vp, c_i64, ctypes.c_uint64, c_vp, c_vp]),
    # mesh cleanup (csrc/meshclean.hip); labels / remap int32, order / seg_start int64, out float64,
    # launches a host int32
    "pnr_mesh_weld_workspace_bytes": (c_size, [c_i64]),
    "pnr_mesh_weld": (c_i32, [c_vp, c_i64, c_vp, c_size, c_vp, c_vp]),
    "pnr_mesh_components_workspace_bytes": (c_size, [c_i64, c_i64]),
    "pnr_mesh_components": (c_i32, [c_vp, c_i64, c_i64, c_vp, c_size, c_vp, c_vp, ctypes.POINTER(c_i32), c_vp]),
    "pnr_mesh_component_sums": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp]),
    # mesh rendering (csrc/meshraster.hip); face int32, depth / rgb / normal float32; lights, weights,
    # albedo and background of pnr_mesh_shade are host float arrays
    "pnr_mesh_raster_workspace_bytes": (c_size, [c_i64, c_i32, c_i32, c_i64]),
    "pnr_mesh_raster": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_i32, c_i32, c_i32, c_f, c_f, c_f, c_f,
                                c_vp, c_size, c_vp, c_vp, c_vp]),
    "pnr_mesh_raster_set_small": (c_i32, [c_i32]),
    "pnr_mesh_shade": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_i32, c_i32, c_i32, c_f, c_f, c_f, c_f,
                               c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_f, c_vp, c_vp, c_vp, c_vp]),
}

# pnr_weight_grad_arith arithmetics (PNR_WGRAD_*, ABI 4)
WGRAD_ARITH = {"f16x3": 0, "bf16x6": 1}

_lib = None


class PnrError(RuntimeError):
    pass


def load():
    """Load libpnr.so once; raise loudly if it is missing (no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PnrError("libpnr.so not built (%s); run `make -C pixel-nerf_amd` or "
                       "__graft_entry__.build()" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        if os.environ.get("PNR_LIB_PATH") and not hasattr(lib, name):
            continue   # an older diagnostic build (A/B against a previous revision)
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.pnr_abi_version() != ABI_VERSION:
        raise PnrError("libpnr.so ABI version %d, this binding expects %d; rebuild it"
                       % (lib.pnr_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().pnr_last_error().decode(errors="replace")
        raise PnrError("%s failed (status %d): %s" % (what, rc, msg))


def ptr(t):
    """Device pointer of a tensor (or None -> NULL)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


class _restored:
    """Context manager base: the library switch ``setter`` takes ``value`` inside and, after, the
    value it held before (every ``pnr_*_set_*`` returns the previous one)."""
    setter = None

    def __enter__(self):
        self.prev = getattr(load(), self.setter)(self.value)
        return self

    def __exit__(self, *exc):
        getattr(load(), self.setter)(self.prev)
        return False


class fused_march(_restored):
    """Context manager: pnr_render_set_fused(mode) inside, the previous DEFAULT restored after
    (2, the default: fused passes + fine-draw kernel; 1: fine draws in the coarse epilogue too;
    0: the separate sample / composite kernels).  It changes the process default, which only
    calls without their own mode use; ``NeRFRenderer.march_mode`` names the mode per renderer
    (pnr_render_cfg.march_mode, no process state)."""
    setter = "pnr_render_set_fused"

    def __init__(self, mode):
        self.value = int(mode)


# pnr_mlp_last_kernel (PNR_MLP_KERNEL_*)
MLP_KERNEL_NONE, MLP_KERNEL_GENERAL, MLP_KERNEL_LEAN = 0, 1, 2


class lean_mlp(_restored):
    """Context manager: pnr_mlp_set_lean(on) inside, the previous setting restored after.  Off,
    every point-model launch of the process takes the general kernel (bit-identical outputs)."""
    setter = "pnr_mlp_set_lean"

    def __init__(self, on):
        self.value = int(bool(on))


def stream_of(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def call(name, device, *args):
    """The one checked launch: ``name(*args, stream)`` of libpnr.so with ``device`` current and on
    torch's current stream of that device; a non-zero status raises PnrError as ``check`` words it.
    For every entry point that ends in a stream (the size queries, pnr_mlp_last_kernel, the set_*
    switches and pnr_mc_case_table have none: ``load().pnr_x(...)``)."""
    fn = getattr(load(), name)
    with torch.cuda.device(device):
        rc = fn(*args, stream_of(device))
    if rc != 0:
        check(rc, name)


def workspace(nbytes, dtype, dev, refusal):
    """The buffer a ``pnr_*_bytes`` size query sized, as a tensor of ``dtype`` on ``dev`` (``dev``
    None: the check alone, no buffer).  A size of 0 is the library's refusal of the shape:
    PnrError(``refusal``)."""
    if nbytes == 0:
        raise PnrError(refusal)
    return None if dev is None else torch.empty(nbytes // dtype.itemsize, device=dev, dtype=dtype)
