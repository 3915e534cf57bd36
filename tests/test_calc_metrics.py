"""scripts/calc_metrics.py on the host (numpy backend) and the host-side refusals of the image
metrics ABI: no GPU needed.

The map step is checked against pnr.evaluate.ssim / psnr_np on the arrays it decodes, the reduce
step against the reference's own eval/calc_metrics.py -R where a reference checkout is present
(copied into a scratch tree at test time with import stubs for the libraries it needs but never
calls under -R; nothing of it is kept)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import textwrap

import pytest

import metrics_synth as ms
from pnr import _lib, evaluate, ops

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "eval", "calc_metrics.py")),
                               reason="reference checkout absent")


# ---- C ABI ------------------------------------------------------------------------------------
def test_image_metrics_abi_refuses_without_touching_a_device():
    lib = _lib.load()
    assert lib.pnr_abi_version() == 8
    wsb = lib.pnr_image_metrics_workspace_bytes
    assert wsb(1, 6, 64, 3) == 0 and wsb(1, 64, 6, 3) == 0          # below the window
    assert wsb(1, 64, 64, 5) == 0 and wsb(1, 64, 64, 0) == 0        # channels
    assert wsb(0, 64, 64, 3) == 0 and wsb(-1, 64, 64, 3) == 0       # images
    assert wsb(1, 64, 8193, 3) == 0 and wsb(1, 8193, 64, 3) == 0    # above the limit
    assert wsb(1, 8192, 8192, 4) > 0 and wsb(1, 7, 7, 1) > 0
    sizes = [wsb(n, 64, 64, 3) for n in (1, 2, 3, 24, 25, 1000, 70000)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    # one (ssim, squared error) pair of float64 per (image, channel, tile)
    t = ops.IMAGE_METRICS_TILE
    tiles = ((64 - 6 + t - 1) // t) ** 2
    assert 16 * 24 * 3 * tiles <= wsb(24, 64, 64, 3) < 16 * 24 * 3 * tiles + 256

    fn = lib.pnr_image_metrics
    buf = (ctypes.c_char * 8192)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)
    ok = (1.0, 0.01, 0.03)
    assert fn(None, p, 1, 7, 7, 1, *ok, p, 4096, p, None) == -1 and b"NULL" in lib.pnr_last_error()
    assert fn(p, None, 1, 7, 7, 1, *ok, p, 4096, p, None) == -1 and b"NULL" in lib.pnr_last_error()
    assert fn(p, p, 1, 7, 7, 1, *ok, p, 4096, None, None) == -1 and b"NULL" in lib.pnr_last_error()
    assert fn(p, p, 1, 8193, 7, 1, *ok, p, 4096, p, None) == -2 and b"8192" in lib.pnr_last_error()
    assert fn(p, p, 1, 7, 8193, 1, *ok, p, 4096, p, None) == -2 and b"8192" in lib.pnr_last_error()
    assert fn(p, p, 1, 6, 7, 1, *ok, p, 4096, p, None) == -1 and b"7 x 7 window" in lib.pnr_last_error()
    assert fn(p, p, 0, 7, 7, 1, *ok, p, 4096, p, None) == -1
    assert fn(p, p, 1, 7, 7, 5, *ok, p, 4096, p, None) == -1
    assert fn(p, p, 1, 7, 7, 1, 0.0, 0.01, 0.03, p, 4096, p, None) == -1 and b"data_range" in lib.pnr_last_error()
    assert fn(p, p, 1, 7, 7, 1, *ok, p, 8, p, None) == -4
    assert fn(p, p, 1, 7, 7, 1, *ok, None, 4096, p, None) == -4
    assert fn(p, p, 1, 7, 7, 1, *ok, p, 4096, ctypes.c_void_p(p.value + 4), None) == -1
    assert b"aligned" in lib.pnr_last_error()
    assert fn(p, p, 1, 7, 7, 1, *ok, ctypes.c_void_p(p.value + 4), 4096, p, None) == -1


def test_tile_constant_matches_the_header():
    with open(os.path.join(ms.REPO, "include", "pnr_abi.h")) as f:
        m = re.search(r"#define PNR_IMAGE_METRICS_TILE (\d+)", f.read())
    assert m and int(m.group(1)) == ops.IMAGE_METRICS_TILE


def test_python_op_refuses_on_the_host():
    import torch

    x = torch.zeros(2, 8, 8, 3)
    with pytest.raises(ValueError, match="x must be on a HIP device"):
        ops.image_metrics(x, x)
    with pytest.raises(ValueError, match="shape"):
        ops.image_metrics(x, x[:1])
    with pytest.raises(ValueError, match="backend"):
        evaluate.image_metrics(x, x, backend="cuda")
    p, s = evaluate.image_metrics(x + 0.25, x + 0.5)      # tensors on the host: the numpy path
    assert len(p) == len(s) == 2 and abs(p[0] - 10 * 1.2041199826559248) < 1e-9


# ---- the map step -------------------------------------------------------------------------------
def expected_text(data_obj, rend, img_dir, name_fmt, view_ids):
    ps = ss = 0.0
    for vid in view_ids:
        pred, gt = ms.decoded(os.path.join(data_obj, img_dir, name_fmt % vid), os.path.join(rend, "%06d.png" % vid))
        assert pred.shape == gt.shape == (16, 16, 3)
        ps += evaluate.psnr_np(pred, gt)
        ss += evaluate.ssim(pred, gt)
    return "psnr {}\nssim {}".format(float(ps / len(view_ids)), float(ss / len(view_ids)))


def dvr_objects(data, out):
    """(category, data object dir, render dir) of the objects the DVR map step must score."""
    return [(cat, os.path.join(data, cat, obj), os.path.join(out, cat + "_" + obj))
            for cat in ms.CATS for obj in ("obja", "objb")]


def metrics_text(rend):
    with open(os.path.join(rend, "metrics.txt")) as f:
        return f.read()


@pytest.fixture(scope="module")
def script():
    return ms.load_script()


@pytest.fixture()
def dvr(tmp_path, script):
    """The DVR tree after a plain multi-category map on the host.  (The reduce, like the
    reference's, wants a metrics.txt in every folder of the output root, and the tree holds one
    rendered object outside the split list: tests that reduce remove it first.)"""
    data, out = ms.write_dvr_tree(str(tmp_path))
    script.run_map(script.parse_args(["-D", data, "-O", out, "-F", "dvr", "--multicat", "--metrics_backend", "numpy"]))
    return data, out


def test_map_scores_each_listed_rendered_object(dvr):
    data, out = dvr
    for cat, obj_dir, rend in dvr_objects(data, out):
        assert metrics_text(rend) == expected_text(obj_dir, rend, "image", "%04d.png", ms.VIEW_IDS)
    for cat in ms.CATS:
        # in the split list but never rendered; rendered but not in the split list
        assert not os.path.exists(os.path.join(out, cat + "_objc"))
        assert not os.path.exists(os.path.join(out, cat + "_" + ms.UNLISTED, "metrics.txt"))


def test_multicat_reduce_lines(dvr):
    data, out = dvr
    for cat in ms.CATS:   # the reduce reads every folder of the output root: drop the unscored one
        shutil.rmtree(os.path.join(out, cat + "_" + ms.UNLISTED))
    script_main = ms.load_script().main
    script_main(["-D", data, "-O", out, "-R", "--multicat"])
    with open(os.path.join(out, "all_metrics.txt")) as f:
        lines = f.read().split("\n")
    assert len(lines) == 4 and lines[2] == "---"
    per_cat = {}
    for cat, _, rend in dvr_objects(data, out):
        per_cat.setdefault(cat, []).append(ms.read_metrics(os.path.join(rend, "metrics.txt")))
    rows = []
    for line, cat in zip(lines[:2], sorted(ms.CATS)):
        rows += per_cat[cat]
        mean = {k: (0.0 + per_cat[cat][0][k] + per_cat[cat][1][k]) / 2 for k in ("psnr", "ssim")}
        label = "{:12s}".format(ms.CATS[cat].split(",")[0])
        assert line == "%s psnr: %.6f ssim: %.6f n_inst: 2" % (label, mean["psnr"], mean["ssim"])
    tot = {k: sum(r[k] for r in rows) / 4 for k in ("psnr", "ssim")}
    assert lines[3] == "%s psnr: %.6f ssim: %.6f" % ("{:12s}".format("total"), tot["psnr"], tot["ssim"])
    assert "lpips" not in "".join(lines)


def test_exclusions_and_overwrite(dvr, tmp_path, script):
    data, out = dvr
    before = {rend: metrics_text(rend) for _, _, rend in dvr_objects(data, out)}
    cat0, cat1 = sorted(ms.CATS)
    viewlist = tmp_path / "src_dvr.txt"
    rows = ["%s %s %d" % (cat, obj, 2 if cat == cat0 else 3) for cat in ms.CATS for obj in ms.LISTED + (ms.UNLISTED,)]
    viewlist.write_text("\n".join(rows) + "\n")
    argv = ["-D", data, "-O", out, "-F", "dvr", "--multicat", "--metrics_backend", "numpy", "-L", str(viewlist),
            "-P", "0"]
    script.run_map(script.parse_args(argv))               # metrics.txt exists: left alone
    assert {rend: metrics_text(rend) for rend in before} == before
    script.run_map(script.parse_args(argv + ["--overwrite"]))
    for cat, obj_dir, rend in dvr_objects(data, out):
        keep = (3, 5) if cat == cat0 else (2, 5)          # -P drops 0, the list drops 2 or 3
        assert metrics_text(rend) == expected_text(obj_dir, rend, "image", "%04d.png", keep)
        assert metrics_text(rend) != before[rend]


def test_reduce_only_leaves_metrics_alone(dvr, script):
    data, out = dvr
    for cat in ms.CATS:
        shutil.rmtree(os.path.join(out, cat + "_" + ms.UNLISTED))
    rends = [rend for _, _, rend in dvr_objects(data, out)]
    with open(os.path.join(rends[0], "metrics.txt"), "w") as f:
        f.write("psnr 10.0\nssim 0.5")
    with open(os.path.join(rends[1], "metrics.txt"), "w") as f:
        f.write("psnr 20.0\nssim 0.25\nlpips 0.125")       # lpips on one object only: not listed
    for rend in rends[2:]:
        with open(os.path.join(rend, "metrics.txt"), "w") as f:
            f.write("psnr 30.0\nssim 1.0")
    stamp = {rend: (metrics_text(rend), os.stat(os.path.join(rend, "metrics.txt")).st_mtime_ns) for rend in rends}
    script.main(["-D", data, "-O", out, "-F", "dvr", "-R", "--overwrite"])
    assert stamp == {rend: (metrics_text(rend), os.stat(os.path.join(rend, "metrics.txt")).st_mtime_ns)
                     for rend in rends}
    with open(os.path.join(out, "all_metrics.txt")) as f:
        assert f.read() == " psnr: 22.500000 ssim: 0.687500"


def test_srn_layout_view_filters_as_a_user_runs_it(tmp_path):
    """The command line itself, SRN layout (RGBA ground truth, no split list), with
    --eval_view_list and --exclude_dtu_bad together: of the ids 0 2 3 5 the list keeps 0 2 3,
    the bad views drop 3."""
    data, out = ms.write_srn_tree(str(tmp_path))
    views = tmp_path / "views.txt"
    views.write_text("0 2 3 7\n")
    r = subprocess.run([sys.executable, ms.SCRIPT, "-D", data, "-O", out, "-F", "srn", "--metrics_backend", "numpy",
                        "--eval_view_list", str(views), "--exclude_dtu_bad"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sum("lpips" in ln for ln in r.stderr.splitlines()) == 1   # said once: LPIPS is not provided
    vals = []
    for obj in ("car0", "car1"):
        rend = os.path.join(out, obj)
        assert metrics_text(rend) == expected_text(os.path.join(data, obj), rend, "rgb", "%06d.png", (0, 2))
        vals.append(ms.read_metrics(os.path.join(rend, "metrics.txt")))
    with open(os.path.join(out, "all_metrics.txt")) as f:
        assert f.read() == " psnr: %.6f ssim: %.6f" % ((0.0 + vals[0]["psnr"] + vals[1]["psnr"]) / 2,
                                                       (0.0 + vals[0]["ssim"] + vals[1]["ssim"]) / 2)


def test_dtu_sort_orders_by_scan_number(tmp_path, script, capsys):
    out = tmp_path / "out"
    for name, v in (("scan9", 1.0), ("scan10", 2.0), ("scan114", 3.0), ("_ignored", 9.0)):
        os.makedirs(out / name)
        (out / name / "metrics.txt").write_text("psnr %r\nssim %r" % (v, v / 4))
    script.main(["-O", str(out), "-F", "srn", "-R", "--dtu_sort"])
    printed = [ln.split()[0] for ln in capsys.readouterr().out.splitlines() if ln.startswith(str(out) + os.sep)]
    assert [os.path.basename(p) for p in printed] == ["scan9", "scan10", "scan114"]
    assert (out / "all_metrics.txt").read_text() == " psnr: 2.000000 ssim: 0.500000"


# ---- reduce parity with the reference ---------------------------------------------------------------
STUBS = {
    "skimage/__init__.py": "",
    "skimage/measure.py": "",
    "lpips.py": "",
    "imageio.py": "",
}


@needs_ref
def test_reduce_matches_the_reference_script(dvr, tmp_path):
    data, out = dvr
    for cat in ms.CATS:
        shutil.rmtree(os.path.join(out, cat + "_" + ms.UNLISTED))
    ref_dir = tmp_path / "ref"
    os.makedirs(ref_dir / "stubs" / "skimage")
    shutil.copyfile(os.path.join(REF, "eval", "calc_metrics.py"), ref_dir / "calc_metrics.py")
    stubs = dict(STUBS)
    try:
        import tqdm  # noqa: F401
    except ImportError:
        stubs["tqdm.py"] = "def tqdm(it, *a, **k):\n    return it\n"
    for name, body in stubs.items():
        (ref_dir / "stubs" / name).write_text(textwrap.dedent(body))
    env = dict(os.environ, PYTHONPATH=str(ref_dir / "stubs"), CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    ours = ms.load_script().main
    for extra in ([], ["--multicat", "--metadata", "metadata.yaml"]):
        ours(["-D", data, "-O", out, "-R"] + extra)
        with open(os.path.join(out, "all_metrics.txt")) as f:
            mine = f.read()
        os.remove(os.path.join(out, "all_metrics.txt"))
        r = subprocess.run([sys.executable, str(ref_dir / "calc_metrics.py"), "-D", data, "-O", out, "-R"] + extra,
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        with open(os.path.join(out, "all_metrics.txt")) as f:
            theirs = f.read()
        assert " lpips: 0.000000" in theirs
        assert mine == theirs.replace(" lpips: 0.000000", "") and "psnr" in mine
