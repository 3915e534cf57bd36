"""Host-side checks of the "f16" render mode (PNR_PREC_F16): the ABI constant and pack sizes,
the refusals that need no device, and the CPU emulation (tests/f16_emul.py) that the GPU tests
of the mode take their tolerances from.  No GPU."""
import os
import re

import pytest
import torch

import f16_emul
import fixtures
from oracle import ref_cpu
from pnr import _lib, synth
from pnr.models import PRECISIONS, PixelNeRFNet
from pnr.renderer import NeRFRenderer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pnr_abi.h")


def _conf():
    mlp = dict(type="resnet", n_blocks=5, d_hidden=512, combine_layer=3, combine_type="average")
    return dict(use_encoder=True, use_xyz=True, use_code=True,
                code=dict(num_freqs=6, freq_factor=1.5, include_input=True), use_viewdirs=True,
                use_code_viewdirs=False, mlp_coarse=mlp, mlp_fine=dict(mlp),
                encoder=dict(backbone="resnet34", pretrained=False, num_layers=4))


def test_precision_constant_in_python_and_header():
    assert PRECISIONS["f16"] == 1
    text = open(HEADER).read()
    assert re.search(r"^#define\s+PNR_PREC_F16\s+1\s*$", text, flags=re.M)
    assert re.search(r"^#define\s+PNR_ABI_VERSION\s+8\b", text, flags=re.M)   # additive: no new version


def test_single_part_pack_sizes():
    lib = _lib.load()
    d1 = _lib.MlpDesc(42, 512, 512, 4, 5, 3, 12, 1)
    d3 = _lib.MlpDesc(42, 512, 512, 4, 5, 3, 12, 3)
    s1, s3 = lib.pnr_mlp_packed_bytes(d1), lib.pnr_mlp_packed_bytes(d3)
    assert s1 != 0, lib.pnr_last_error()
    assert s1 < s3
    assert s1 >= 13 * 512 * 512 * 2
    # one fp16 part per 512-wide layer: exactly half of f16x3's layer bytes less
    assert s3 - s1 == 13 * 512 * 512 * 2
    # the backward pack stays f16x3's
    assert lib.pnr_mlp_packed_t_bytes(d3) != 0
    assert lib.pnr_mlp_packed_t_bytes(d1) == 0


def _cpu_net(precision="f16"):
    net = PixelNeRFNet(_conf())
    net.mlp_precision = precision
    return net


def test_refusals_before_any_device_work():
    net = _cpu_net()
    assert any(p.requires_grad for p in net.parameters())
    r = NeRFRenderer(n_coarse=8, n_fine=8)
    rays = torch.zeros(1, 4, 8)
    with torch.enable_grad():
        with pytest.raises(NotImplementedError, match=r'"f16" is inference only; use f16x3'):
            r(net, rays)
    # training-mode sigma noise takes the same graph, with or without grad
    r2 = NeRFRenderer(n_coarse=8, n_fine=8, noise_std=1.0).train()
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match=r'"f16" is inference only; use f16x3'):
            r2(net, rays)
    with pytest.raises(NotImplementedError, match=r'"f16" is inference only; use f16x3'):
        net._forward_points_grad(torch.zeros(1, 4, 3), True, torch.zeros(1, 4, 3))
    from pnr.train import RenderPoints

    class Ctx:
        pass

    with pytest.raises(NotImplementedError, match=r'"f16" is inference only; use f16x3'):
        RenderPoints.forward(Ctx(), net, True, torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(1))
    # only the projected-latent kernels exist in f16
    net.use_latent_proj = False
    with pytest.raises(NotImplementedError, match=r'"f16" is inference only; use f16x3.*use_latent_proj'):
        net._require_hip()
    with pytest.raises(NotImplementedError, match=r'"f16" is inference only; use f16x3.*use_latent_proj'):
        net.hip_mlp(True)
    # an MLP without lin_z layers has no projected latent
    conf = _conf()
    conf["mlp_coarse"] = dict(conf["mlp_coarse"], combine_layer=0)
    conf["mlp_fine"] = dict(conf["mlp_fine"], combine_layer=0)
    flat = PixelNeRFNet(conf)
    flat.mlp_precision = "f16"
    with pytest.raises(NotImplementedError, match=r'"f16" is inference only; use f16x3.*lin_z'):
        flat.hip_mlp(True)
    # the other modes are not touched by the check
    ok = _cpu_net("f16x3")
    ok.use_latent_proj = False
    ok._check_f16()


def _pointquery():
    cfg, arr = fixtures.load("fw_pointquery")
    sd = fixtures.state_dict(cfg)
    scene = ref_cpu.Scene(fixtures.latent_of(cfg), arr["poses"], fixtures.focal_of(arr),
                          cfg["width"], cfg["height"], None)
    return sd, scene, arr["xyz"], torch.zeros_like(arr["xyz"])


def test_scale_exp_matches_the_kernel_rule():
    m = torch.tensor([0.0, 1.0, 0.75, 2.0 ** 14, 3.0, float("inf"), float("nan"), 2.0 ** -100, 2.0 ** 100])
    e = f16_emul.scale_exp(m).tolist()
    # m < 2^frexp_exp, e = 14 - frexp_exp: 1.0 = 0.5 * 2^1 -> 13; 0.75 -> 14; 2^14 -> -1; 3 -> 12
    assert e == [0, 13, 14, -1, 12, 0, 0, 40, -64]
    mid = m[[1, 2, 3, 4]].double()   # unclamped: the scaled maximum lands in [2^13, 2^14)
    assert bool((torch.ldexp(mid, torch.tensor(e)[[1, 2, 3, 4]]) < 2.0 ** 14).all())
    assert bool((torch.ldexp(mid, torch.tensor(e)[[1, 2, 3, 4]]) >= 2.0 ** 13).all())


@pytest.mark.parametrize("coarse", [True, False])
def test_emulation_sanity_on_pointquery(coarse, monkeypatch):
    sd, scene, xyz, vd = _pointquery()
    with torch.no_grad():
        ref = ref_cpu.pixelnerf_forward(sd, scene, xyz, coarse, vd)
        f16_emul.install(monkeypatch)
        emu = ref_cpu.pixelnerf_forward(sd, scene, xyz, coarse, vd)
        monkeypatch.setattr(f16_emul, "ROUND", False)
        exact = ref_cpu.pixelnerf_forward(sd, scene, xyz, coarse, vd)
    d = (emu - ref).abs()
    print("emulation vs oracle, %s: max|d rgb| %.3e mean|d rgb| %.3e max|d sigma| %.3e (sigma up to %.2f)" % (
        "coarse" if coarse else "fine", float(d[..., :3].max()), float(d[..., :3].mean()),
        float(d[..., 3].max()), float(ref[..., 3].max())))
    assert not torch.equal(emu, ref)
    assert float(d[..., :3].max()) < 1.0 / 510.0       # half an 8-bit step
    assert float((exact - ref).abs().max()) <= 1e-6    # the twin without its roundings is the oracle
