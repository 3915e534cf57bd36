"""Synthetic dataset + render trees for scripts/calc_metrics.py (tests/test_calc_metrics.py and
tests/test_gpu_metrics.py): a two-category DVR-layout dataset with its ``<category>_<object>``
render folders, and a flat SRN-layout dataset.  Rendered PNGs are the ground truth plus seeded
uint8 noise."""
import importlib.util
import json
import os

import numpy as np
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(REPO, "scripts", "calc_metrics.py")
CATS = {"02691156": "airplane,aeroplane,plane", "03001627": "chair"}
VIEW_IDS = (0, 2, 3, 5)          # 3 and 5 are on the hard-coded DTU bad-view list
LISTED = ("obja", "objb", "objc")  # in softras_test.lst; objc has no render folder
UNLISTED = "objd"                # rendered, but not in the split list


def load_script():
    """scripts/calc_metrics.py as a module (its ``main(argv)`` runs in-process)."""
    spec = importlib.util.spec_from_file_location("calc_metrics_script", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _views(rng, size, alpha):
    gt = rng.integers(0, 256, (size, size, 4 if alpha else 3), dtype=np.uint8)
    # smooth half of the image so that the variance term of SSIM is not noise everywhere
    gt[: size // 2, :, :3] = (gt[: size // 2, :1, :3] // 2 + 60)
    noise = rng.integers(-25, 26, (size, size, 3))
    pred = np.clip(gt[..., :3].astype(np.int64) + noise, 0, 255).astype(np.uint8)
    return gt, pred


def write_dvr_tree(root, seed=0, size=16):
    """-> (datadir, render root).  data/<cat>/<obj>/image/<id:04>.png, data/<cat>/softras_test.lst,
    data/metadata.yaml (JSON); out/<cat>_<obj>/<id:06>.png."""
    rng = np.random.default_rng(seed)
    data, out = os.path.join(root, "data"), os.path.join(root, "out")
    os.makedirs(out)
    for cat in CATS:
        for obj in LISTED + (UNLISTED,):
            os.makedirs(os.path.join(data, cat, obj, "image"))
            rend = os.path.join(out, cat + "_" + obj)
            if obj != "objc":
                os.makedirs(rend)
            for vid in VIEW_IDS:
                gt, pred = _views(rng, size, alpha=False)
                Image.fromarray(gt).save(os.path.join(data, cat, obj, "image", "%04d.png" % vid))
                if obj != "objc":
                    Image.fromarray(pred).save(os.path.join(rend, "%06d.png" % vid))
        with open(os.path.join(data, cat, "softras_test.lst"), "w") as f:
            f.write("\n".join(LISTED) + "\n")
    with open(os.path.join(data, "metadata.yaml"), "w") as f:
        json.dump({cat: {"id": cat, "name": name} for cat, name in CATS.items()}, f)
    return data, out


def write_srn_tree(root, seed=1, size=16, objs=("car0", "car1")):
    """-> (datadir, render root).  srn/<obj>/rgb/<id:06>.png (RGBA, as SRN ships them);
    srn_out/<obj>/<id:06>.png."""
    rng = np.random.default_rng(seed)
    data, out = os.path.join(root, "srn"), os.path.join(root, "srn_out")
    for obj in objs:
        os.makedirs(os.path.join(data, obj, "rgb"))
        os.makedirs(os.path.join(out, obj))
        for vid in VIEW_IDS:
            gt, pred = _views(rng, size, alpha=True)
            Image.fromarray(gt).save(os.path.join(data, obj, "rgb", "%06d.png" % vid))
            Image.fromarray(pred).save(os.path.join(out, obj, "%06d.png" % vid))
    return data, out


def decoded(gt_path, pred_path):
    """The two arrays the map step scores for one view."""
    from pnr.data import _imread

    return (_imread(pred_path).astype(np.float32) / 255.0,
            _imread(gt_path).astype(np.float32)[..., :3] / 255.0)


def read_metrics(path):
    with open(path) as f:
        return {k: float(v) for k, v in (line.split() for line in f)}
