"""pnr.ops.image_metrics (csrc/metrics.hip) on the device against pnr.evaluate.ssim / psnr_np on the
host, which tests/test_data_eval.py pins to brute-force window sums.  The device op is never
compared with itself except for run-to-run and batch-versus-alone bit identity.

Tolerance 1e-9 (SSIM absolute, PSNR in dB where finite): both sides are fp64 on identical fp32
inputs and differ in summation order only.  The variance cancellation against C2 = 9e-4 costs at
most ~49 * 1.1e-16 / 9e-4 = 6e-12 relative, the MSE over <= 4e5 terms ~4e-11 relative; 1e-9 leaves
two orders of magnitude over both."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_synth as ms
from pnr import _lib, evaluate, ops

pytestmark = pytest.mark.gpu
TOL = 1e-9
T = ops.IMAGE_METRICS_TILE


def dev():
    return torch.device("cuda", 0)


def images(shape, seed, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    x = (lo + (hi - lo) * rng.random(shape)).astype(np.float32)
    y = np.clip(x + (0.1 * (hi - lo) * rng.normal(size=shape)).astype(np.float32), lo, hi).astype(np.float32)
    return x, y


def yardstick(x, y, **kw):
    """(psnr, ssim) per image on the host."""
    ssim_kw = dict(kw)
    psnr_kw = {k: v for k, v in kw.items() if k == "data_range"}
    return (np.array([evaluate.psnr_np(a, b, **psnr_kw) for a, b in zip(x, y)]),
            np.array([evaluate.ssim(a, b, **ssim_kw) for a, b in zip(x, y)]))


def device_scores(x, y, **kw):
    p, s = ops.image_metrics(torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev()), **kw)
    assert p.dtype == s.dtype == torch.float64 and p.shape == s.shape == (len(x),) and p.device.type == "cuda"
    return p.cpu().numpy(), s.cpu().numpy()


def check(x, y, pick=None, **kw):
    p, s = device_scores(x, y, **kw)
    if pick is not None:
        x, y, p, s = x[pick], y[pick], p[pick], s[pick]
    rp, rs = yardstick(x, y, **kw)
    print("max |d ssim| %.3e  max |d psnr| %.3e dB" % (np.abs(s - rs).max(), np.abs(p - rp)[np.isfinite(rp)].max()
                                                      if np.isfinite(rp).any() else 0.0))
    assert np.array_equal(np.isfinite(p), np.isfinite(rp))
    assert np.abs(s - rs).max() < TOL
    fin = np.isfinite(rp)
    assert np.abs(p[fin] - rp[fin]).max(initial=0.0) < TOL
    return p, s


SHAPES = [
    (1, 7, 7, 1),                    # one window
    (1, 7, 8, 3), (1, 8, 7, 3),      # two windows
    (1, 13, 9, 4),
    (5, 23, 22, 3),
    (3, T + 6, T + 6, 3),            # exactly one tile
    (2, T + 7, T + 6, 3), (2, T + 6, T + 7, 1),   # a one-pixel second tile in each direction
    (1, 2 * T + 9, T + 11, 3),
    (24, 64, 64, 3),                 # the NMR batch
    (1, 128, 128, 3),                # an SRN frame
    (1, 300, 400, 3),                # a DTU frame
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matches_the_host_scores(shape):
    x, y = images(shape, seed=sum(shape))
    check(x, y)


def test_more_workgroups_than_a_16_bit_grid_dimension():
    x, y = images((70000, 7, 7, 1), seed=3)
    check(x, y, pick=slice(5, None, 70000 // 64 + 1))


def test_three_dimensional_input_is_one_image():
    x, y = images((1, 20, 31, 3), seed=5)
    p, s = ops.image_metrics(torch.from_numpy(x[0]).to(dev()), torch.from_numpy(y[0]).to(dev()))
    p4, s4 = ops.image_metrics(torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev()))
    assert p.shape == (1,) and torch.equal(p, p4) and torch.equal(s, s4)


# ---- values -------------------------------------------------------------------------------------
def test_equal_images():
    x, _ = images((2, 40, 33, 3), seed=11)
    p, s = device_scores(x, x.copy())
    assert np.all(np.abs(s - 1.0) < 1e-12) and np.all(p == np.inf)


def test_constant_images_closed_form():
    a, b = float(np.float32(0.3)), float(np.float32(0.55))
    x = np.full((2, 25, 19, 3), a, np.float32)
    y = np.full((2, 25, 19, 3), b, np.float32)
    p, s = check(x, y)
    c1 = 0.01 ** 2
    assert np.all(np.abs(s - (2 * a * b + c1) / (a * a + b * b + c1)) < TOL)   # the C2 factor is C2 / C2
    assert np.all(np.abs(p - 10 * np.log10(1.0 / (a - b) ** 2)) < TOL)


def test_inverted_image_scores_negative():
    x, _ = images((2, 30, 30, 3), seed=13)
    p, s = check(x, (1.0 - x).astype(np.float32))
    assert np.all(s < 0)


def test_data_range_two():
    x, y = images((2, 21, 37, 3), seed=17, lo=-1.0, hi=1.0)
    check(x, y, data_range=2.0)


def test_other_constants():
    x, y = images((2, 21, 37, 3), seed=19)
    p, s = check(x, y, k1=0.02, k2=0.05)
    assert np.abs(s - yardstick(x, y)[1]).max() > 1e-6     # the constants reached the kernel


def test_nan_stays_in_its_row():
    x, y = images((5, 2 * T + 9, T + 11, 3), seed=23)
    p0, s0 = ops.image_metrics(torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev()))
    for which in (0, 1):
        bad = [x.copy(), y.copy()]
        bad[which][2, T + 8, 3, 1] = np.nan
        p, s = ops.image_metrics(torch.from_numpy(bad[0]).to(dev()), torch.from_numpy(bad[1]).to(dev()))
        assert bool(torch.isnan(p[2])) and bool(torch.isnan(s[2]))
        keep = torch.tensor([0, 1, 3, 4], device=dev())
        assert torch.equal(p[keep], p0[keep]) and torch.equal(s[keep], s0[keep])


# ---- determinism and batching -------------------------------------------------------------------
def test_bit_identical_across_calls_and_batching():
    x, y = images((5, 2 * T + 9, T + 11, 3), seed=29)
    xd, yd = torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())
    p, s = ops.image_metrics(xd, yd)
    p2, s2 = ops.image_metrics(xd, yd)
    assert torch.equal(p, p2) and torch.equal(s, s2)
    for i in range(5):
        pi, si = ops.image_metrics(xd[i:i + 1], yd[i:i + 1])
        assert torch.equal(pi, p[i:i + 1]) and torch.equal(si, s[i:i + 1])


# ---- layout and refusals ------------------------------------------------------------------------
def test_non_contiguous_view():
    rng = np.random.default_rng(31)
    xc = torch.from_numpy(rng.random((3, 3, 20, 26), dtype=np.float32)).to(dev())   # (N, C, H, W)
    yc = torch.from_numpy(rng.random((3, 3, 20, 26), dtype=np.float32)).to(dev())
    xv, yv = xc.permute(0, 2, 3, 1), yc.permute(0, 2, 3, 1)
    assert not xv.is_contiguous()
    p, s = ops.image_metrics(xv, yv)
    p2, s2 = ops.image_metrics(xv.contiguous(), yv.contiguous())
    assert torch.equal(p, p2) and torch.equal(s, s2)
    rp, rs = yardstick(xv.cpu().numpy(), yv.cpu().numpy())
    assert np.abs(s.cpu().numpy() - rs).max() < TOL and np.abs(p.cpu().numpy() - rp).max() < TOL


def test_refusals():
    x = torch.zeros(2, 9, 9, 3, device=dev())
    with pytest.raises(ValueError, match="y must be on a HIP device|y is on cpu"):
        ops.image_metrics(x, x.cpu())
    with pytest.raises(ValueError, match="x must be on a HIP device"):
        ops.image_metrics(x.cpu(), x.cpu())
    with pytest.raises(ValueError, match="x must be float32"):
        ops.image_metrics(x.half(), x.half())
    with pytest.raises(ValueError, match="y must be float32"):
        ops.image_metrics(x, x.double())
    with pytest.raises(ValueError, match="y has shape"):
        ops.image_metrics(x, x[:, :8])
    with pytest.raises(ValueError, match="7 x 7 SSIM window"):
        ops.image_metrics(x[:, :6], x[:, :6])
    with pytest.raises(ValueError, match="data_range"):
        ops.image_metrics(x, x, data_range=0.0)


# ---- the C ABI on the device --------------------------------------------------------------------
def test_abi_on_the_device():
    shape = (2, T + 7, T + 6, 3)
    x, y = images(shape, seed=37)
    xd, yd = torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())
    lib = _lib.load()
    n, h, w, c = shape
    need = lib.pnr_image_metrics_workspace_bytes(n, h, w, c)
    assert need >= 16 * n * c * 2
    ws = torch.empty(need // 8, device=dev(), dtype=torch.float64)
    out = torch.full((n * 2 + 1,), -7.0, device=dev(), dtype=torch.float64)
    st = _lib.stream_of(dev())
    args = (_lib.ptr(xd), _lib.ptr(yd), n, h, w, c, 1.0, 0.01, 0.03)
    assert lib.pnr_image_metrics(*args, _lib.ptr(ws), need - 1, _lib.ptr(out), st) == -4
    assert lib.pnr_image_metrics(*args, _lib.ptr(ws), need, ctypes.c_void_p(out.data_ptr() + 4), st) == -1
    assert b"aligned" in lib.pnr_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                       # the refused calls wrote nothing
    assert lib.pnr_image_metrics(*args, _lib.ptr(ws), need, _lib.ptr(out), st) == 0
    p, s = ops.image_metrics(xd, yd)
    got = out[:2 * n].reshape(n, 2)
    assert torch.equal(got[:, 1], s) and torch.equal(10.0 * torch.log10(1.0 / got[:, 0]), p)
    assert float(out[-1]) == -7.0


# ---- callers ------------------------------------------------------------------------------------
class RenderTape:
    """Stands in for the bound renderer inside eval_approx: records the batches it renders, or
    replays recorded ones."""

    def __init__(self, inner, tape, replay):
        self.inner, self.tape, self.replay = inner, tape, replay

    def eval(self):
        return self

    def __call__(self, rays):
        if self.replay:
            return self.tape.pop(0)
        rgb, depth = self.inner(rays)
        self.tape.append((rgb.clone(), depth.clone()))
        return rgb, depth


def test_eval_approx_backends_agree(tmp_path):
    """evaluate.eval_approx on the synthetic SRN directory with the device scores and with the
    host scores, same seed: the per-object lists agree to TOL.

    Two separate runs do not render the same bits (the encoder's convolutions; test_data_eval.py
    holds two runs of one backend to 1e-5 only, and two runs measured here differed by 2.4e-7 dB),
    so the host run scores the very batches the device run rendered: the renderer of the device
    run is taped and replayed.  Everything else of eval_approx (view selection, ground truth,
    layout, the per-batch scoring) runs twice.  The spread between two independent runs is
    printed."""
    from pnr import synth
    from pnr.data import SRNDataset
    from pnr.models import PixelNeRFNet
    from pnr.renderer import NeRFRenderer
    from srn_synth import make_inputs, write_srn_dir

    root = write_srn_dir(str(tmp_path), make_inputs(n_obj=2, n_views=3, size=24, seed=0))
    dset = SRNDataset(root, stage="test", image_size=(24, 24))
    mlp = dict(type="resnet", n_blocks=5, d_hidden=512, combine_layer=3, combine_type="average")
    conf = dict(use_encoder=True, use_xyz=True, use_code=True, code=dict(num_freqs=6, freq_factor=1.5),
                use_viewdirs=True, use_code_viewdirs=False, mlp_coarse=mlp, mlp_fine=mlp,
                encoder=dict(backbone="resnet34", pretrained=False, num_layers=4))
    torch.manual_seed(0)
    net = PixelNeRFNet(conf)
    net.load_state_dict(synth.pixelnerf_state(2), strict=False)
    net = net.to(dev()).eval()
    tape = []

    def run(backend, taped=False, replay=False):
        r = NeRFRenderer(n_coarse=32, n_fine=16, white_bkgd=True).to(dev())
        if taped:
            bind = r.bind_parallel
            r.bind_parallel = lambda *a, **k: RenderTape(bind(*a, **k).eval(), tape, replay)
        return evaluate.eval_approx(net, r, dset, dev(), source=[1], batch_size=2, seed=7, metrics_backend=backend)

    fresh = run("numpy")
    device = run("hip", taped=True)
    assert len(tape) == 1
    host = run("numpy", taped=True, replay=True)
    assert not tape
    print("eval_approx numpy %s %s hip %s %s" % (host["psnr"], host["ssim"], device["psnr"], device["ssim"]))
    print("two independent renders, both scored on the host: max |d psnr| %.3e dB, max |d ssim| %.3e" % (
        np.abs(np.array(fresh["psnr"]) - np.array(host["psnr"])).max(),
        np.abs(np.array(fresh["ssim"]) - np.array(host["ssim"])).max()))
    assert device["objects"] == host["objects"] == 2
    assert np.abs(np.array(device["psnr"]) - np.array(host["psnr"])).max() < TOL
    assert np.abs(np.array(device["ssim"]) - np.array(host["ssim"])).max() < TOL
    assert abs(device["mean_ssim"] - host["mean_ssim"]) < TOL and abs(device["mean_psnr"] - host["mean_psnr"]) < TOL


def clear_of_rounding_boundaries(path):
    """No number of an all_metrics.txt lies within 1e-7 of where its sixth decimal flips."""
    objs = [d for d in sorted(os.listdir(path)) if os.path.isdir(os.path.join(path, d))]
    rows = [ms.read_metrics(os.path.join(path, d, "metrics.txt")) for d in objs]
    groups = [rows] + [[r for d, r in zip(objs, rows) if d.startswith(cat + "_")] for cat in ms.CATS]
    for group in groups:
        for k in ("psnr", "ssim"):
            mean = sum(r[k] for r in group) / len(group)
            if abs((mean * 1e6) % 1.0 - 0.5) <= 0.1:
                return False
    return True


def test_calc_metrics_script_backends_agree(tmp_path):
    """scripts/calc_metrics.py --metrics_backend hip as a user runs it, against the same tree scored
    on the host.  all_metrics.txt prints six decimals, so the two files can only be compared byte
    for byte where no mean sits on a rounding boundary: seed 5 was picked on the host for that
    (seeds 0 .. 4 each have a mean within 1e-7 of one), and the property is asserted below."""
    data, out = ms.write_dvr_tree(str(tmp_path), seed=5)
    for cat in ms.CATS:
        shutil.rmtree(os.path.join(out, cat + "_" + ms.UNLISTED))
    out_hip = str(tmp_path / "out_hip")
    shutil.copytree(out, out_hip)
    argv = ["-D", data, "-F", "dvr", "--multicat"]
    ms.load_script().main(argv + ["-O", out, "--metrics_backend", "numpy"])
    assert clear_of_rounding_boundaries(out)               # of the host scores: a property of the seed
    r = subprocess.run([sys.executable, ms.SCRIPT, *argv, "-O", out_hip, "--metrics_backend", "hip"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "hip backend" in r.stdout
    objs = [d for d in sorted(os.listdir(out)) if os.path.isdir(os.path.join(out, d))]
    assert len(objs) == 4
    for d in objs:
        a, b = (ms.read_metrics(os.path.join(o, d, "metrics.txt")) for o in (out, out_hip))
        assert set(a) == set(b) == {"psnr", "ssim"}
        print(d, a, b)
        assert abs(a["psnr"] - b["psnr"]) < TOL and abs(a["ssim"] - b["ssim"]) < TOL
    with open(os.path.join(out, "all_metrics.txt"), "rb") as f, open(os.path.join(out_hip, "all_metrics.txt"), "rb") as g:
        assert f.read() == g.read()
