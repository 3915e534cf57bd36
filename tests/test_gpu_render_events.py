"""The ``events`` argument of the fused render (``pnr_render_forward_proj``, reached through
``pnr.torchops.EVENTS_HOOK``) on an MI355X (``-m gpu``).

The render records up to seven HIP events on its stream, around the kernels of the coarse and the
fine pass; ``bench.py`` reads all seven.  Which launches fall between which events depends on
the route the call takes, so every route is rendered once here: 8 rays of one object with one
source view (16 point tiles at most).  After a stream synchronize every consecutive pair of
recorded events must give an elapsed time >= 0, and the outputs must equal those of the same call
made without events.  Nothing is asserted about how long an interval is.
"""
import ctypes

import pytest
import torch

import test_gpu_parity as tgp
from pnr import synth, torchops
from pnr.models import PixelNeRFNet
from pnr.renderer import NeRFRenderer

pytestmark = pytest.mark.gpu
DEV = tgp.DEV
N_RAYS = 8

# (n_coarse, n_fine, n_fine_depth, march_mode, mlp_fine is None, events recorded)
CASES = [
    pytest.param(64, 64, 0, 0, False, 7, id="separate-kernels"),
    pytest.param(64, 64, 16, 2, False, 7, id="fused-coarse-draw-kernel-fused-fine"),
    pytest.param(64, 64, 16, 1, False, 7, id="fine-draws-in-coarse-epilogue"),
    pytest.param(64, 64, 0, 3, False, 7, id="single-launch"),
    pytest.param(64, 32, 0, 2, False, 7, id="fused-coarse-separate-fine"),   # 96 is no tile multiple
    pytest.param(64, 64, 0, 2, True, 7, id="coarse-output-reuse"),
    pytest.param(48, 0, 0, 2, False, 4, id="separate-coarse-no-fine"),
]


class HipEvents:
    """hipEvent_t handles from the HIP runtime torch already loaded (as bench.py makes them)."""

    def __init__(self):
        self.hip = ctypes.CDLL("libamdhip64.so.7")
        self.hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        self.hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p,
                                                 ctypes.c_void_p]
        self.hip.hipEventDestroy.argtypes = [ctypes.c_void_p]

    def create(self, n):
        evs = []
        for _ in range(n):
            e = ctypes.c_void_p()
            assert self.hip.hipEventCreate(ctypes.byref(e)) == 0
            evs.append(e)
        return evs

    def elapsed_ms(self, a, b):
        ms = ctypes.c_float(-1.0)
        return self.hip.hipEventElapsedTime(ctypes.byref(ms), a, b), ms.value

    def destroy(self, evs):
        for e in evs:
            self.hip.hipEventDestroy(e)


@pytest.fixture(scope="module")
def scene():
    return synth.scene_srn(seed=0, n_rays=N_RAYS, pick="hash")


@pytest.fixture(scope="module")
def nets(scene):
    """{mlp_fine is None: encoded net}"""
    out = {}
    for share in (False, True):
        net = PixelNeRFNet(tgp.model_conf())
        net.load_state_dict(synth.pixelnerf_state(1), strict=False)
        if share:
            net.mlp_fine = None
        net = net.to(DEV).eval()
        net.encode_latent(scene["latent"].to(DEV), scene["poses"].to(DEV), scene["focal"].to(DEV), (128, 128))
        out[share] = net
    return out


@pytest.mark.parametrize("kc,kf,kfd,mode,share,n_events", CASES)
def test_render_events_recorded_on_every_route(scene, nets, kc, kf, kfd, mode, share, n_events):
    net = nets[share]
    if mode == 3:   # the single launch needs both projections
        assert net.hip_proj(True) is not None and net.hip_proj(False) is not None
    r = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, depth_std=0.01, white_bkgd=True)
    streams = synth.rng_streams(2, N_RAYS, kc, kf, kfd)   # injected: a render consumes r.streams
    r.return_z = True
    r.march_mode = mode
    rays = scene["rays"][None].to(DEV)
    ev = HipEvents()
    calls = []

    def hook(n_rays, n_coarse, n_fine):
        assert (int(n_rays), int(n_coarse), int(n_fine)) == (N_RAYS, kc, kf)
        evs = ev.create(7)
        calls.append(evs)
        return [int(e.value) for e in evs]

    try:
        r.streams = streams
        with torch.no_grad():
            plain = r(net, rays, want_weights=True)
        assert torchops.EVENTS_HOOK is None
        torchops.EVENTS_HOOK = hook
        r.streams = streams
        try:
            with torch.no_grad():
                timed = r(net, rays, want_weights=True)
        finally:
            torchops.EVENTS_HOOK = None
        torch.cuda.current_stream().synchronize()
        assert len(calls) == 1
        evs = calls[0]
        for i in range(n_events - 1):
            rc, ms = ev.elapsed_ms(evs[i], evs[i + 1])
            assert rc == 0, "hipEventElapsedTime(%d, %d) = %d" % (i, i + 1, rc)
            assert ms >= 0.0, (i, ms)
    finally:
        for evs in calls:
            ev.destroy(evs)
    for p in (("coarse", "fine") if kf > 0 else ("coarse",)):
        for k in ("rgb", "depth", "weights", "z"):
            assert torch.equal(timed[p][k], plain[p][k]), (p, k)
    assert bool(torch.isfinite(timed.coarse.rgb).all())
