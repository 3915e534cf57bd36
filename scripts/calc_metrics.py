#!/usr/bin/env python
"""eval/calc_metrics.py counterpart: per-object PSNR / SSIM of rendered views against the dataset's
ground truth (map), then their means over all objects and, with --multicat, per category (reduce).

  python scripts/calc_metrics.py -D <datadir> -O <eval output> -F dvr --list_name softras_test \
      [--multicat] [-L src_dvr.txt] [-P "0 1"] [--eval_view_list views.txt] [--exclude_dtu_bad] \
      [--overwrite] [-R] [--dtu_sort] [--metrics_backend auto|hip|numpy]

Map: every object directory of the dataset (filtered by <category>/<list_name>.lst for the dvr
format) that has a folder of the same name (``<category>_<object>`` with --multicat) under the
output root pairs ``<object>/<image|rgb>/<id>.{png,jpg}`` with ``<output>/<object>/<id:06>.png``,
drops the excluded view ids, scores all remaining views in ONE ``pnr.evaluate.image_metrics`` call
(on the device with the hip backend) and writes ``metrics.txt`` as ``psnr {}\\nssim {}``.  The
scores are skimage's compare_psnr / compare_ssim(multichannel=True, data_range=1) as pnr.evaluate
restates them.  LPIPS is written as a third line only where the ``lpips`` package imports.

Reduce: every folder of the output root whose name does not start with "_" contributes its
``metrics.txt``; ``all_metrics.txt`` gets one `` {name}: {mean:.6f}`` per metric that every object
carries, preceded with --multicat by one line per category (names from the dataset's metadata file,
JSON) with ``n_inst``.
"""
import argparse
import json
import os
import os.path as osp
import sys
import warnings

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, osp.join(REPO, "pixel-nerf_amd"))

import numpy as np  # noqa: E402

METRIC_NAMES = ["psnr", "ssim", "lpips"]
DTU_BAD_VIEWS = [3, 4, 5, 6, 7, 16, 17, 18, 19, 20, 21, 36, 37, 38, 39]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Calculate PSNR / SSIM for rendered images.")
    ap.add_argument("--datadir", "-D", type=str, default="/home/group/chairs_test",
                    help="Dataset directory, used directly (the directory that holds the objects, or the "
                         "categories with --multicat)")
    ap.add_argument("--output", "-O", type=str, default="eval", help="Root path of the rendered output (eval.py)")
    ap.add_argument("--dataset_format", "-F", type=str, default="dvr", help="Dataset format, nerf | srn | dvr")
    ap.add_argument("--list_name", type=str, default="softras_test", help="Filter list prefix for DVR")
    ap.add_argument("--gpu_id", type=int, default=0, help="GPU id (hip backend, LPIPS)")
    ap.add_argument("--overwrite", action="store_true", help="overwrite existing metrics.txt")
    ap.add_argument("--exclude_dtu_bad", action="store_true", help="exclude the hardcoded DTU bad views")
    ap.add_argument("--multicat", action="store_true",
                    help="Prepend category id to object id. Specify if the model fits multiple categories.")
    ap.add_argument("--viewlist", "-L", type=str, default="",
                    help="Path to a source view list, e.g. src_dvr.txt; excludes each object's source views")
    ap.add_argument("--eval_view_list", type=str, default=None, help="Path to eval view list")
    ap.add_argument("--primary", "-P", type=str, default="", help="List of views to exclude")
    ap.add_argument("--lpips_batch_size", type=int, default=32, help="Batch size for LPIPS")
    ap.add_argument("--reduce_only", "-R", action="store_true", help="skip the map (per-object metrics)")
    ap.add_argument("--metadata", type=str, default="metadata.yaml",
                    help="Dataset metadata under datadir (JSON), for the category names if --multicat")
    ap.add_argument("--dtu_sort", action="store_true", help="Sort using DTU scene order instead of lex")
    ap.add_argument("--metrics_backend", choices=("auto", "hip", "numpy"), default="auto",
                    help="hip = score on the device (pnr.ops.image_metrics), numpy = on the host; auto = hip "
                         "when a HIP device is present, else numpy")
    return ap.parse_args(argv)


def dataset_layout(args):
    """(list file name or "", image folder name or "") of the dataset format."""
    if args.dataset_format == "dvr":
        return args.list_name + ".lst", "image"
    if args.dataset_format == "srn":
        return "", "rgb"
    if args.dataset_format == "nerf":
        warnings.warn("test split not implemented for NeRF synthetic data format")
        return "", ""
    raise NotImplementedError("Not supported data format " + args.dataset_format)


def load_lpips(args):
    """The LPIPS scorer, or None (said once) where the package is missing."""
    try:
        import lpips
    except ImportError:
        print("calc_metrics: the lpips package does not import; metrics.txt gets no lpips line", file=sys.stderr)
        return None
    import torch

    dev = "cuda:%d" % args.gpu_id if torch.cuda.is_available() else "cpu"
    net = lpips.LPIPS(net="vgg").to(device=dev)

    def score(preds, gts):
        p = torch.from_numpy(preds).permute(0, 3, 1, 2) * 2.0 - 1.0
        g = torch.from_numpy(gts).permute(0, 3, 1, 2) * 2.0 - 1.0
        with torch.no_grad():
            vals = [net(pi.to(device=dev), gi.to(device=dev)).reshape(-1)
                    for pi, gi in zip(torch.split(p, args.lpips_batch_size), torch.split(g, args.lpips_batch_size))]
        return torch.cat(vals).mean().item()

    return score


def run_map(args):
    from pnr import evaluate
    from pnr.data import _imread

    list_name, img_dir_name = dataset_layout(args)
    backend = evaluate._resolve_backend(args.metrics_backend, "metrics")
    if backend == "hip":
        import torch

        torch.cuda.set_device(args.gpu_id)
    print("Scoring with the", backend, "backend")

    if args.multicat:
        cats = sorted(os.listdir(args.datadir))
    else:
        cats = ["."]

    def fmt_obj_name(c, x):
        return c + "_" + x if args.multicat else x

    exclude_lut = None
    if len(args.viewlist) > 0:
        print("Excluding views from list", args.viewlist)
        with open(args.viewlist, "r") as f:
            rows = [x.strip().split() for x in f.readlines()]
        exclude_lut = {x[0] + "/" + x[1]: list(map(int, x[2:])) for x in rows if len(x) >= 2}
    base_exclude_views = list(map(int, args.primary.split()))
    if args.exclude_dtu_bad:
        base_exclude_views.extend(DTU_BAD_VIEWS)
    eval_views = None
    if args.eval_view_list is not None:
        with open(args.eval_view_list, "r") as f:
            eval_views = list(map(int, f.readline().split()))
        print("Only using views", eval_views)

    all_objs = []
    print("CATEGORICAL SUMMARY")
    total_objs = 0
    for cat in cats:
        cat_root = osp.join(args.datadir, cat)
        if not osp.isdir(cat_root):
            continue
        objs = sorted(os.listdir(cat_root))
        if len(list_name) > 0:
            with open(osp.join(cat_root, list_name), "r") as f:
                split = set(x.strip() for x in f.readlines())
            objs = [x for x in objs if x in split]
        objs = [(osp.join(cat_root, x), osp.join(args.output, fmt_obj_name(cat, x))) for x in objs]
        objs = [x for x in objs if osp.isdir(x[0])]
        objs_avail = [x for x in objs if osp.exists(x[1])]
        print(cat, "TOTAL", len(objs), "AVAILABLE", len(objs_avail))
        total_objs += len(objs)
        all_objs.extend(objs_avail)
    print(">>> USING", len(all_objs), "OF", total_objs, "OBJECTS")

    lpips_score = load_lpips(args)

    def process_obj(path, rend_path):
        im_root = osp.join(path, img_dir_name) if len(img_dir_name) > 0 else path
        out_path = osp.join(rend_path, "metrics.txt")
        if osp.exists(out_path) and not args.overwrite:
            return
        exclude_views = list(base_exclude_views)
        if exclude_lut is not None:
            exclude_views.extend(exclude_lut[osp.basename(rend_path).replace("_", "/")])
        gts, preds = [], []
        for im_name in sorted(os.listdir(im_root)):
            stem, ext = osp.splitext(im_name)
            if ext != ".jpg" and ext != ".png":
                continue
            im_id = int(stem)
            im_rend_path = osp.join(rend_path, "{:06}.png".format(im_id))
            if not osp.exists(im_rend_path) or im_id in exclude_views:
                continue
            if eval_views is not None and im_id not in eval_views:
                continue
            gt = _imread(osp.join(im_root, im_name)).astype(np.float32)[..., :3] / 255.0
            pred = _imread(im_rend_path).astype(np.float32) / 255.0
            if gt.ndim != 3 or gt.shape != pred.shape:
                raise ValueError("%s is %s but its render %s is %s" % (osp.join(im_root, im_name), gt.shape,
                                                                      im_rend_path, pred.shape))
            gts.append(gt)
            preds.append(pred)
        if not gts:
            print("calc_metrics: no view of %s has a render in %s; no metrics.txt written" % (path, rend_path),
                  file=sys.stderr)
            return
        # one call per image size (an object's views share one in every supported dataset)
        psnrs, ssims = [None] * len(gts), [None] * len(gts)
        for shape in sorted(set(g.shape for g in gts)):
            idx = [i for i, g in enumerate(gts) if g.shape == shape]
            p, s = evaluate.image_metrics(np.stack([preds[i] for i in idx]), np.stack([gts[i] for i in idx]), backend)
            for i, pi, si in zip(idx, p, s):
                psnrs[i], ssims[i] = pi, si
        psnr_avg, ssim_avg = 0.0, 0.0
        for p, s in zip(psnrs, ssims):
            psnr_avg += p
            ssim_avg += s
        out_txt = "psnr {}\nssim {}".format(psnr_avg / len(gts), ssim_avg / len(gts))
        if lpips_score is not None:
            if len(set(g.shape for g in gts)) > 1:
                raise ValueError("LPIPS needs views of one size in " + path)
            out_txt += "\nlpips {}".format(lpips_score(np.stack(preds), np.stack(gts)))
        with open(out_path, "w") as f:
            f.write(out_txt)

    for obj_path, obj_rend_path in all_objs:
        process_obj(obj_path, obj_rend_path)


def read_metrics(path):
    """metrics.txt -> {name: float}, one ``name value`` pair per line."""
    with open(path, "r") as f:
        return {tok[0]: float(tok[1]) for tok in (line.split() for line in f) if len(tok) == 2}


def mean_line(label, rows, names):
    """``label`` followed by `` {name}: {mean:.6f}`` per metric; the mean adds the rows in order
    from 0.0 and divides once."""
    txt = label
    for name in names:
        acc = 0.0
        for row in rows:
            acc += row[name]
        txt += " {}: {:.6f}".format(name, acc / len(rows))
    return txt


def run_reduce(args):
    folders = [x for x in os.listdir(args.output) if x[0] != "_" and osp.isdir(osp.join(args.output, x))]
    if args.dtu_sort:
        folders.sort(key=lambda x: int(x[4:]))   # scan<N>
    else:
        folders.sort()
    print(">>> PROCESSING", len(folders), "OBJECTS")
    if not folders:
        raise SystemExit("calc_metrics: no object folder under " + args.output)
    rows = [read_metrics(osp.join(args.output, x, "metrics.txt")) for x in folders]
    # the metrics every object carries: an absent one (lpips without the package) is not a 0
    names = [n for n in METRIC_NAMES if all(n in row for row in rows)]
    if len(folders) < 100:
        for x, row in zip(folders, rows):
            print(osp.join(args.output, x), *[repr(row[n]) for n in names])

    lines = []
    if args.multicat:
        with open(osp.join(args.datadir, args.metadata), "r") as f:
            meta = json.load(f)
        by_cat = {cat: [] for cat in meta}
        for x, row in zip(folders, rows):
            cat = x.split("_")[0]
            if cat not in by_cat:
                raise KeyError("category %s of %s is not in %s" % (cat, x, args.metadata))
            by_cat[cat].append(row)
        for cat in sorted(by_cat):
            if by_cat[cat]:
                label = "{:12s}".format(meta[cat]["name"].split(",")[0])
                lines.append(mean_line(label, by_cat[cat], names) + " n_inst: {}".format(len(by_cat[cat])))
        lines.append("---")
    lines.append(mean_line("{:12s}".format("total") if args.multicat else "", rows, names))
    text = "\n".join(lines)
    out_path = osp.join(args.output, "all_metrics.txt")
    with open(out_path, "w") as f:
        f.write(text)
    print("WROTE", out_path)
    print(text)


def main(argv=None):
    args = parse_args(argv)
    dataset_layout(args)   # refuse an unknown format before any work
    if not args.reduce_only:
        print(">>> Compute")
        run_map(args)
    print(">>> Reduce")
    run_reduce(args)


if __name__ == "__main__":
    main()
