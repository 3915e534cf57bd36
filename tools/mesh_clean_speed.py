#!/usr/bin/env python
"""Times the mesh cleanup on one MI355X, three ways, on the mesh scripts/eval.py would clean: the
marching-cubes mesh (pnr.ops.marching_cubes) of a 256^3 grid holding two blobs and a few hundred
single-voxel floaters, resident on the device, as its STL soup (three vertices per triangle).

  kernel  pnr.ops.mesh_weld of the soup, mesh_components, mesh_component_stats (csrc/meshclean.hip)
          and the whole pnr.evaluate.clean_mesh(keep="largest", backend="hip")          (HIP events)
  torch   the same steps as torch ops on the same device: torch.unique(dim=0) for the weld,
          min-label rounds (scatter_reduce amin over the faces, then pointer jumping) to a fixed
          point for the labels, bincount and a mask for the selection                    (HIP events)
  host    device -> host copy, np.unique(axis=0), scipy.sparse.csgraph.connected_components, the
          largest component, host -> device copy                                         (host clock)
Medians over --reps runs after --warmup; the kernel and the torch route alternate inside one loop.
The shader clock is read (not set) before and after from the driver's sysfs table.  The file also
records the launches pnr_mesh_components took, the rounds the torch route needed, the bytes each
kernel pass moves at least (its inputs and outputs once), and that the three routes kept the same
faces.

  python tools/mesh_clean_speed.py [--out profiles/meshclean/meshclean_speed.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "pixel-nerf_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pnr import _lib, evaluate, ops  # noqa: E402
from speed_common import _stats, events, floater_grid, shader_clock_mhz  # noqa: E402


def torch_labels(n_verts, faces):
    """Min-label rounds in torch: (vert_label, rounds)."""
    f = faces.long()
    label = torch.arange(n_verts, device=faces.device)
    rounds = 0
    while True:
        rounds += 1
        cur = label[f]
        low = cur.min(1).values
        new = label.clone()
        for k in range(3):
            new.scatter_reduce_(0, cur[:, k], low, "amin")
            new.scatter_reduce_(0, f[:, k], low, "amin")
        while True:
            jump = new[new]
            if torch.equal(jump, new):
                break
            new = jump
        if torch.equal(new, label):
            return label, rounds
        label = new


def torch_route(soup):
    """(kept face mask, rounds): weld with torch.unique, label, keep the component with the most faces."""
    uniq, inv = torch.unique(soup, dim=0, return_inverse=True)
    faces = inv.reshape(-1, 3)
    label, rounds = torch_labels(uniq.shape[0], faces)
    fl = label[faces[:, 0]]
    counts = torch.bincount(fl, minlength=uniq.shape[0])
    return fl == counts.argmax(), rounds


def host_route(soup, dev):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    s = soup.cpu().numpy()
    uniq, inv = np.unique(s, axis=0, return_inverse=True)
    f = inv.reshape(-1, 3)
    rows, cols = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(len(uniq),) * 2)
    _, comp = connected_components(graph, directed=False)
    fl = comp[f[:, 0]]
    keep = fl == np.bincount(fl).argmax()
    kept = s.reshape(-1, 3, 3)[keep].reshape(-1, 3)
    out = torch.from_numpy(kept).to(dev)
    torch.cuda.synchronize(dev)
    return keep, out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--floaters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_clean_speed.py needs a HIP device: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    clock_before = shader_clock_mhz()
    verts, faces = ops.marching_cubes(floater_grid(args.res, dev, args.floaters), 0.0)
    soup = verts[faces.long()].reshape(-1, 3).contiguous()
    soup_faces = torch.arange(soup.shape[0], device=dev, dtype=torch.int32).reshape(-1, 3)
    n_t, n_s = int(faces.shape[0]), int(soup.shape[0])

    wv, wf, _ = ops.mesh_weld(soup, soup_faces)
    vl, fl, n_comp, launches = ops.mesh_components(wv, wf, return_launches=True)
    n_w = int(wv.shape[0])
    print("mesh: %d faces, soup of %d vertices welds to %d, %d components" % (n_t, n_s, n_w, n_comp))

    stages = {"weld": lambda: ops.mesh_weld(soup, soup_faces), "components": lambda: ops.mesh_components(wv, wf),
              "stats": lambda: ops.mesh_component_stats(wv, wf, vl, fl),
              "clean_mesh": lambda: evaluate.clean_mesh(soup, soup_faces, keep="largest", backend="hip")}
    ms = {k: [] for k in list(stages) + ["torch"]}
    for i in range(args.warmup + args.reps):   # alternating, so a drifting clock hits both alike
        for k, fn in stages.items():
            t = events(fn, 0, 1)
            if i >= args.warmup:
                ms[k] += t
        t = events(lambda: torch_route(soup), 0, 1)
        if i >= args.warmup:
            ms["torch"] += t
    host_ms = []
    for i in range(args.warmup + args.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        keep_host, _ = host_route(soup, dev)
        if i >= args.warmup:
            host_ms.append((time.perf_counter() - t0) * 1e3)

    # the three routes keep the same faces
    cv, cf, info = evaluate.clean_mesh(soup, soup_faces, keep="largest", backend="hip")
    keep_torch, rounds = torch_route(soup)
    kept_kernel = cv[cf.long()].reshape(-1, 3)
    kept_torch = soup.reshape(-1, 3, 3)[keep_torch].reshape(-1, 3)
    same = bool(torch.equal(kept_kernel, kept_torch)) and bool(np.array_equal(keep_host, keep_torch.cpu().numpy()))

    table = _lib.load().pnr_mesh_weld_workspace_bytes(n_s)
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = dict(device=torch.cuda.get_device_name(0), shader_clock_mhz=dict(before=clock_before, after=shader_clock_mhz()),
               grid=args.res, floaters=args.floaters, faces=n_t, soup_vertices=n_s, welded_vertices=n_w,
               components=n_comp, info=info, warmup=args.warmup, reps=args.reps, host_threads=torch.get_num_threads(),
               kernel_route=dict(weld_ms=_stats(ms["weld"]), components_ms=_stats(ms["components"]),
                                 stats_ms=_stats(ms["stats"]), clean_mesh_ms=_stats(ms["clean_mesh"]),
                                 components_launches=launches,
                                 note="each stage includes its torch plumbing and host syncs (compaction, counts, "
                                      "the stable sort of the faces); clean_mesh is the whole chain in one call"),
               torch_route=dict(ms=_stats(ms["torch"]), label_rounds=rounds),
               host_route=dict(ms=_stats(host_ms), note="D2H, np.unique(axis=0), scipy connected_components, H2D"),
               min_bytes_per_pass=dict(weld_insert=12 * n_s + table, weld_lookup=12 * n_s + table + 4 * n_s,
                                       components_init=4 * n_w, components_hook=12 * n_t + 4 * n_w,
                                       components_flatten=4 * n_w + 12 * n_t + 4 * n_w + 4 * n_t,
                                       component_sums=8 * n_t + 12 * n_t + 12 * n_w),
               clean_mesh_over_torch=med["clean_mesh"] / med["torch"],
               clean_mesh_over_host=med["clean_mesh"] / statistics.median(host_ms),
               routes_keep_the_same_faces=same)
    print(json.dumps(out, indent=1, sort_keys=True))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
