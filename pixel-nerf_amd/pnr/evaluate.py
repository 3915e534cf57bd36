"""Evaluation: image metrics over a dataset, and the scores of a predicted mesh.

Image metrics.  Counterpart of eval/eval_approx.py:56-153: for every object one
random target view is rendered from the chosen source view(s) through ``render_par`` (bind_parallel,
simple_output) and scored against the ground-truth image with PSNR and SSIM at data_range 1.  The
view selection replays the reference's draws in order on torch's global generator (seeded with
``seed``): per batch ``randint(0, NV, (SB, 1))`` for a random source, then
``randint(0, NV - NS, (SB, 1))`` for the target, shifted past the sources.

``ssim`` restates skimage.measure.compare_ssim(X, Y, multichannel=True, data_range=1) with
its defaults (7 x 7 uniform window, sample covariance, K1 = 0.01, K2 = 0.03, per-channel
mean over the map cropped by 3 pixels); skimage is absent offline, so that restatement is
pinned by the brute-force window sum in tests/test_host.py, not by skimage itself.

Mesh scores: ``mesh_metrics`` (Chamfer, F-score, normal consistency), ``volume_iou``, ``clean_mesh``
(weld, components, floater removal) and ``render_mesh_views`` / ``silhouette_scores``.  Each is a
dispatcher and the assembly of its scores: ``_resolve_backend`` says which backend runs, ``"hip"``
places the inputs with ``_to_device`` and calls pnr.ops, ``"numpy"`` converts them with
``mesh_np._host_mesh`` and calls the host restatements of pnr.mesh_np (re-exported here).
"""
import numpy as np
import torch

from . import util
from .mesh_np import (_RNG_MESH, _RNG_VOLUME, _draws, _host_mesh, _signed_volume_np,  # noqa: F401
                      _weld_apply_np, box_sample_np, component_stats_np, components_np, nearest_np, raycast_np,
                      sample_mesh_np, shade_np, weld_np, winding_np)

__all__ = ["ssim", "psnr_np", "image_metrics", "select_views", "eval_approx", "mesh_metrics", "sample_mesh_np",
           "nearest_np", "MESH_METRIC_NAMES", "volume_iou", "winding_np", "box_sample_np",
           "VOLUME_METRIC_NAMES", "clean_mesh", "weld_np", "components_np", "component_stats_np",
           "CLEAN_INFO_NAMES", "sphere_poses", "raycast_np", "shade_np", "render_mesh_views", "silhouette_scores",
           "SIL_METRIC_NAMES", "ssaa_camera"]


def psnr_np(pred, target, data_range=1.0):
    """skimage compare_psnr: 10 log10(data_range^2 / mse)."""
    mse = float(np.mean((np.asarray(pred, np.float64) - np.asarray(target, np.float64)) ** 2))
    return float("inf") if mse == 0.0 else 10.0 * np.log10(data_range ** 2 / mse)


def ssim(x, y, data_range=1.0, win_size=7, k1=0.01, k2=0.03):
    """Mean SSIM of two (H, W, C) images (skimage compare_ssim, multichannel, defaults)."""
    from scipy.ndimage import uniform_filter

    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    assert x.shape == y.shape and x.ndim == 3
    vals = []
    for ch in range(x.shape[-1]):
        a, b = x[..., ch], y[..., ch]
        n = win_size ** 2
        cov_norm = n / (n - 1.0)
        ux = uniform_filter(a, size=win_size)
        uy = uniform_filter(b, size=win_size)
        uxx = uniform_filter(a * a, size=win_size)
        uyy = uniform_filter(b * b, size=win_size)
        uxy = uniform_filter(a * b, size=win_size)
        vx = cov_norm * (uxx - ux * ux)
        vy = cov_norm * (uyy - uy * uy)
        vxy = cov_norm * (uxy - ux * uy)
        c1 = (k1 * data_range) ** 2
        c2 = (k2 * data_range) ** 2
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        pad = (win_size - 1) // 2
        vals.append(s[pad:-pad, pad:-pad].mean())
    return float(np.mean(vals))


def image_metrics(x, y, backend="numpy"):
    """(psnr list, ssim list) of two (N, H, W, C) stacks in [0, 1] at data_range 1.  ``"numpy"``
    scores image by image on the host with ``psnr_np`` / ``ssim`` (tensors are copied there);
    ``"hip"`` scores the stack on its device (``ops.image_metrics``, float32 tensors or arrays,
    moved to the current HIP device if they are on the host) with one readback."""
    if backend == "numpy":
        if torch.is_tensor(x):
            x = x.detach().cpu().numpy()
        if torch.is_tensor(y):
            y = y.detach().cpu().numpy()
        assert len(x) == len(y), (len(x), len(y))
        return [float(psnr_np(a, b)) for a, b in zip(x, y)], [ssim(a, b) for a, b in zip(x, y)]
    if backend != "hip":
        raise ValueError("metrics backend must be 'numpy' or 'hip' (got %r)" % (backend,))
    from . import ops

    x, y = (t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t, np.float32)) for t in (x, y))
    dev = x.device if x.device.type == "cuda" else (y.device if y.device.type == "cuda" else torch.device("cuda"))
    psnr, ssim_ = ops.image_metrics(x.to(dev), y.to(dev))
    both = torch.stack([psnr, ssim_]).cpu()
    return both[0].tolist(), both[1].tolist()


def select_views(sb, nv, source):
    """(src_view (SB, NS), dest_view (SB, 1)) as eval_approx.py:111-118 draws them."""
    source = torch.as_tensor(source, dtype=torch.long).reshape(-1)
    ns = source.numel()
    if ns == 1 and int(source[0]) == -1:
        src_view = torch.randint(0, nv, (sb, 1))
    else:
        src_view = source.unsqueeze(0).expand(sb, -1)
    dest_view = torch.randint(0, nv - ns, (sb, 1))
    for i in range(ns):
        dest_view += dest_view >= src_view[:, i:i + 1]
    return src_view, dest_view


def eval_approx(net, renderer, dset, device, source=(64,), batch_size=4, seed=1234, coarse=False,
                ray_batch_size=50000, gpu_ids=None, log=None, metrics_backend="numpy"):
    """eval_approx.py:56-153 on an already built net / renderer / dataset.  Returns
    {"psnr": [...], "ssim": [...], "mean_psnr", "mean_ssim", "objects"}.  ``metrics_backend``:
    ``"numpy"`` copies each rendered batch to the host and scores it there, ``"hip"`` scores it on
    the device (``image_metrics``)."""
    if metrics_backend not in ("numpy", "hip"):
        raise ValueError("metrics_backend must be 'numpy' or 'hip' (got %r)" % (metrics_backend,))
    if coarse:
        net.mlp_fine = None
    renderer.eval_batch_size = ray_batch_size
    if renderer.n_coarse < 64:
        renderer.n_coarse = 64
    if coarse:
        renderer.n_coarse = 64
        renderer.n_fine = 128
        renderer.using_fine = True
    render_par = renderer.bind_parallel(net, gpu_ids, simple_output=True).eval()
    loader = torch.utils.data.DataLoader(dset, batch_size=batch_size, shuffle=False, num_workers=0)
    z_near, z_far = dset.z_near, dset.z_far
    torch.random.manual_seed(seed)
    ns = len(torch.as_tensor(source).reshape(-1))
    psnrs, ssims = [], []
    with torch.no_grad():
        for data in loader:
            images = data["images"]          # (SB, NV, 3, H, W) in [-1, 1]
            poses = data["poses"]            # (SB, NV, 4, 4)
            focal = data["focal"][0]
            images_0to1 = images * 0.5 + 0.5
            SB, NV, _, H, W = images.shape
            src_view, dest_view = select_views(SB, NV, source)
            dest_poses = util.batched_index_select_nd(poses, dest_view)
            all_rays = util.gen_rays(dest_poses.reshape(-1, 4, 4), W, H, focal, z_near, z_far).reshape(SB, -1, 8)
            pri_images = util.batched_index_select_nd(images, src_view)
            pri_poses = util.batched_index_select_nd(poses, src_view)
            net.encode(pri_images.to(device=device), pri_poses.to(device=device), focal.to(device=device))
            rgb_fine, _ = render_par(all_rays.to(device=device))
            gt = util.batched_index_select_nd(images_0to1, dest_view).reshape(SB, 3, H, W)
            if metrics_backend == "numpy":
                rgb_fine = rgb_fine.reshape(SB, H, W, 3).cpu().numpy()
                gt = gt.permute(0, 2, 3, 1).contiguous().numpy()
                for sb in range(SB):
                    ssims.append(ssim(rgb_fine[sb], gt[sb]))
                    psnrs.append(psnr_np(rgb_fine[sb], gt[sb]))
            else:   # the render stays on its device, the ground truth goes to it
                gt = gt.to(device=rgb_fine.device, dtype=torch.float32).permute(0, 2, 3, 1)
                p, s = image_metrics(rgb_fine.reshape(SB, H, W, 3).float(), gt, metrics_backend)
                psnrs.extend(p)
                ssims.extend(s)
            if log is not None:
                log("curr psnr %.4f ssim %.4f" % (np.mean(psnrs), np.mean(ssims)))
    assert ns >= 1
    return {"psnr": psnrs, "ssim": ssims, "mean_psnr": float(np.mean(psnrs)) if psnrs else None,
            "mean_ssim": float(np.mean(ssims)) if ssims else None, "objects": len(psnrs)}


# ---- mesh scores: which backend, and where its inputs go ---------------------------------------------
def _resolve_backend(backend, what):
    """``"hip"`` or ``"numpy"`` from the ``backend`` argument of the mesh functions (``what`` names the
    caller's family in the message); ``"auto"`` is hip where a HIP device is present."""
    if backend == "auto":
        backend = "hip" if torch.cuda.is_available() else "numpy"
    if backend not in ("hip", "numpy"):
        raise ValueError("%s backend must be 'auto', 'numpy' or 'hip' (got %r)" % (what, backend))
    return backend


def _to_device(meshes, poses=None):
    """The hip backends' inputs on one device: ``([(verts, faces), ...], poses)`` from ``(verts,
    faces)`` pairs and optional camera poses, tensors or arrays, as contiguous tensors: verts float32
    (V, 3), faces int32 (T, 3), poses float32.  The device is that of the first CUDA tensor among
    them, else the current HIP device."""
    flat = [t for mesh in meshes for t in mesh] + [poses]
    dev = next((t.device for t in flat if torch.is_tensor(t) and t.device.type == "cuda"),
               torch.device("cuda", torch.cuda.current_device()))

    def place(t, dtype):
        t = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
        return t.to(device=dev, dtype=dtype).contiguous()

    placed = [(place(v, torch.float32).reshape(-1, 3), place(f, torch.int32).reshape(-1, 3)) for v, f in meshes]
    return placed, None if poses is None else place(poses, torch.float32)


# ---- mesh reconstruction metrics (Occupancy Networks' eval_pointcloud) -----------------------------
MESH_METRIC_NAMES = ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "precision", "recall", "fscore",
                     "normals_accuracy", "normals_completeness", "normal_consistency")


def _mesh_scores(d2_ab, idx_ab, d2_ba, idx_ba, na, nb, tau):
    """The ten scores from the two fp64 distance fields (numpy)."""
    d_ab, d_ba = np.sqrt(d2_ab), np.sqrt(d2_ba)
    acc, comp = float(d_ab.mean()), float(d_ba.mean())
    prec, rec = float((d_ab < tau).mean()), float((d_ba < tau).mean())
    nacc = float(np.abs((na.astype(np.float64) * nb[idx_ab].astype(np.float64)).sum(-1)).mean())
    ncomp = float(np.abs((nb.astype(np.float64) * na[idx_ba].astype(np.float64)).sum(-1)).mean())
    return {"accuracy": acc, "completeness": comp, "chamfer_l1": 0.5 * (acc + comp),
            "chamfer_l2": 0.5 * (float(d2_ab.mean()) + float(d2_ba.mean())), "precision": prec, "recall": rec,
            "fscore": 2.0 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0, "normals_accuracy": nacc,
            "normals_completeness": ncomp, "normal_consistency": 0.5 * (nacc + ncomp)}


def _empty_mesh_scores():
    inf = float("inf")
    out = dict.fromkeys(MESH_METRIC_NAMES, 0.0)
    out.update(accuracy=inf, completeness=inf, chamfer_l1=inf, chamfer_l2=inf)
    return out


def mesh_metrics(pred, gt, n_samples=100000, tau=0.01, seed=0, backend="auto"):
    """Scores of a predicted mesh against a ground-truth mesh, each a ``(verts (V, 3), faces (T, 3))``
    pair of tensors or arrays: ``n_samples`` area-weighted surface samples of each (the predicted
    mesh drawn with ``seed``, the ground truth with ``seed + 1``), nearest neighbours both ways, and
    the scores of Occupancy Networks' eval_pointcloud as a dict of floats (MESH_METRIC_NAMES):
    accuracy / completeness = mean distance pred -> gt / gt -> pred, chamfer_l1 their mean,
    chamfer_l2 the mean of the two mean SQUARED distances, precision / recall = the share of pred /
    gt samples nearer than ``tau``, fscore = 2PR / (P + R) (0 where P + R = 0), normals_* the mean
    |n . n'| with the nearest neighbour.  ``"hip"`` runs pnr.ops.mesh_sample / nearest /
    mesh_distance on the device the meshes are on (host meshes are moved to the current HIP device)
    with one read-back; ``"numpy"`` restates the sampling rule on the host and searches with scipy's
    cKDTree, or a chunked brute force without scipy; ``"auto"`` is hip where a HIP device is present.
    A predicted mesh without faces is a result, not an error: the four distances are +inf and the
    other scores 0.  An empty ground truth raises."""
    backend = _resolve_backend(backend, "metrics")
    if len(gt[1]) == 0:
        raise ValueError("mesh_metrics: the ground-truth mesh has no faces")
    if len(pred[1]) == 0:
        return _empty_mesh_scores()
    if backend == "numpy":
        pa, na, _, _ = sample_mesh_np(*pred, n_samples, seed)
        pb, nb, _, _ = sample_mesh_np(*gt, n_samples, seed + 1)
        d2_ab, idx_ab = nearest_np(pa, pb)
        d2_ba, idx_ba = nearest_np(pb, pa)
        return _mesh_scores(d2_ab, idx_ab, d2_ba, idx_ba, na, nb, tau)
    from . import ops

    (pred, gt), _ = _to_device((pred, gt))
    pa, na, _, _ = ops.mesh_sample(*pred, n_samples, seed)
    pb, nb, _, _ = ops.mesh_sample(*gt, n_samples, seed + 1)
    scores = ops.mesh_distance(pa, na, pb, nb, tau)
    vals = torch.stack([scores[k] for k in MESH_METRIC_NAMES]).cpu().tolist()
    return dict(zip(MESH_METRIC_NAMES, vals))


# ---- mesh containment and volumetric IoU (Occupancy Networks' third headline score) ----------------
VOLUME_METRIC_NAMES = ("iou", "volume_pred", "volume_gt", "n_points")


def _signed_volume(v, f):
    """Sum of a . (b x c) / 6 over the faces, fp64: a 0-dim tensor on the mesh's device (the host
    counterpart is mesh_np._signed_volume_np)."""
    t = v.double()[f.long()]
    return (t[:, 0] * torch.linalg.cross(t[:, 1], t[:, 2])).sum() / 6.0


def _grown_box(lo, hi, padding):
    """The sampling box from the fp32 bounds: grown on every side by padding x the largest extent, in
    fp32 (both backends run this on the host, so their boxes are the same bits)."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    pad = np.float32(padding) * (hi - lo).max()
    return lo - pad, hi + pad


def volume_iou(pred, gt, n_points=100000, seed=0, padding=0.05, backend="auto"):
    """Volumetric IoU of a predicted mesh against a ground-truth mesh, each a ``(verts (V, 3), faces
    (T, 3))`` pair of tensors or arrays, as Occupancy Networks scores it: ``n_points`` uniform
    points (pnr_box_sample's draws with ``seed``) in the axis-aligned bounds of both meshes' vertices
    grown on every side by ``padding`` x the largest extent, each classified against each mesh by its
    generalized winding number (inside: w > 0.5).  Returns a dict of floats (VOLUME_METRIC_NAMES):
    ``iou`` = |A and B| / |A or B| from the integer counts (0 where the union is empty),
    ``volume_pred`` / ``volume_gt`` = the share of points inside times the box's volume, ``n_points``.
    A mesh whose signed volume (sum of a . (b x c) / 6, fp64) is negative has inward faces: its w is
    negated before the threshold, so an inside-out STL scores as the solid it bounds.  ``"hip"`` runs
    pnr.ops.box_sample / mesh_contains on the device the meshes are on (host meshes are moved to the
    current HIP device) and reads the bounds back once; ``"numpy"`` is the same rule in fp64 on the
    host (``winding_np``); ``"auto"`` is hip where a HIP device is present.  A predicted mesh without
    faces is a result: iou 0 and volume_pred 0 (the box is then the ground truth's).  An empty ground
    truth raises."""
    backend = _resolve_backend(backend, "metrics")
    n_points = int(n_points)
    if n_points < 1:
        raise ValueError("volume_iou: n_points must be >= 1 (got %d)" % n_points)
    if len(gt[1]) == 0:
        raise ValueError("volume_iou: the ground-truth mesh has no faces")
    empty = len(pred[1]) == 0
    if backend == "numpy":
        (pv, pf), (gv, gf) = _host_mesh(*pred), _host_mesh(*gt)
        both = gv if empty else np.concatenate([pv, gv])
        lo, hi = _grown_box(both.min(0), both.max(0), padding)
        pts = box_sample_np(lo, hi, n_points, seed)

        def inside(v, f):   # inward faces: the w of the solid they bound
            w = winding_np(v, f, pts)
            return (-w if _signed_volume_np(v, f) < 0 else w) > 0.5

        in_g = inside(gv, gf)
        in_p = np.zeros(n_points, bool) if empty else inside(pv, pf)
        counts = [int((in_p & in_g).sum()), int((in_p | in_g).sum()), int(in_p.sum()), int(in_g.sum())]
    else:
        from . import ops

        ((pv, pf), (gv, gf)), _ = _to_device((pred, gt))
        dev = gv.device
        if empty:
            both, vol_p = gv, torch.ones((), device=dev, dtype=torch.float64)
        else:
            both, vol_p = torch.cat([pv, gv]), _signed_volume(pv, pf)
        vol_g = _signed_volume(gv, gf)
        # the one read-back before the draws: the fp32 bounds (exact in fp64) and the two signs
        head = torch.cat([both.min(0).values.double(), both.max(0).values.double(), torch.stack([vol_p, vol_g])]).cpu()
        lo, hi = _grown_box(head[0:3].numpy().astype(np.float32), head[3:6].numpy().astype(np.float32), padding)
        pts = ops.box_sample(lo.tolist(), hi.tolist(), n_points, seed, device=dev)

        def inside(v, f, volume):   # inward faces: the w of the solid they bound
            return ops.mesh_contains(v, f, pts, 0.5) if volume >= 0 else (-ops.winding_number(v, f, pts)) > 0.5

        in_g = inside(gv, gf, float(head[7]))
        in_p = torch.zeros(n_points, device=dev, dtype=torch.bool) if empty else inside(pv, pf, float(head[6]))
        counts = torch.stack([(in_p & in_g).sum(), (in_p | in_g).sum(), in_p.sum(), in_g.sum()]).cpu().tolist()
    inter, union, n_p, n_g = (int(c) for c in counts)
    box = float(np.prod(hi.astype(np.float64) - lo.astype(np.float64)))
    return {"iou": inter / union if union else 0.0, "volume_pred": n_p / n_points * box,
            "volume_gt": n_g / n_points * box, "n_points": float(n_points)}


# ---- mesh cleanup: weld, connected components, floater removal -------------------------------------
CLEAN_INFO_NAMES = ("n_components", "n_components_kept", "faces_kept")




def _select_components(n_faces, measure, keep, min_frac):
    """bool (C,): the components that stay.  Only components with faces take part; ``largest`` is the
    first maximum of the measure (the lowest label on a tie), ``min_frac`` keeps measure >= min_frac *
    the largest measure (fp64).  A NaN measure counts as 0.  Both backends run this on the host."""
    has = np.asarray(n_faces) > 0
    if not has.any():
        return has
    m = np.where(has, np.nan_to_num(np.asarray(measure, np.float64), nan=0.0), -np.inf)
    if keep == "largest":
        sel = np.zeros(len(m), bool)
        sel[int(np.argmax(m))] = True
        return sel
    if min_frac is not None:
        return has & (m >= float(min_frac) * m.max())
    return has


def clean_mesh(verts, faces, weld=True, keep="largest", min_frac=None, by="faces", backend="auto"):
    """Drop the floaters of a mesh: ``(verts', faces', info)`` from verts (V, 3), faces (T, 3), tensors
    or arrays.  With ``weld`` equal vertices are merged first (an STL soup has one component per
    triangle until then); the connected components are labelled; ``keep="largest"`` keeps the one
    component with the most faces (``by="faces"``) or the most area (``by="area"``), a tie going to the
    lowest label; ``keep="all"`` with ``min_frac=F`` (0 < F <= 1) keeps every component whose measure is
    >= F times the largest's, and without it every component.  Kept vertices and faces keep their
    relative order, vertices no kept face names are dropped, faces are re-indexed as int32.  ``info``:
    ``n_components`` (components that hold a face), ``n_components_kept``, ``faces_kept``.  ``"hip"``
    runs pnr.ops.mesh_weld / mesh_components / mesh_component_stats on the device the mesh is on (a
    host mesh is moved to the current HIP device) and returns device tensors; it reads the
    per-component measure back once and selects on the host with the code the ``"numpy"`` backend
    uses, which restates the definitions in pure numpy and returns arrays: labels, remaps, kept sets
    and counts are the same on both (``by="area"`` compares fp64 sums whose last bits differ between
    the two, so only an exact tie or threshold hit can choose differently).  ``"auto"`` is hip where a
    HIP device is present."""
    backend = _resolve_backend(backend, "clean_mesh")
    if keep not in ("largest", "all"):
        raise ValueError("clean_mesh: keep must be 'largest' or 'all' (got %r)" % (keep,))
    if by not in ("faces", "area"):
        raise ValueError("clean_mesh: by must be 'faces' or 'area' (got %r)" % (by,))
    if min_frac is not None:
        if keep == "largest":
            raise ValueError("clean_mesh: min_frac goes with keep='all' ('largest' keeps one component)")
        if not 0.0 < float(min_frac) <= 1.0:
            raise ValueError("clean_mesh: min_frac must be in (0, 1] (got %r)" % (min_frac,))
    if backend == "numpy":
        v, f = _host_mesh(verts, faces, np.int32)
        if weld:
            v, f, _ = _weld_apply_np(v, f)
        vl, fl, _ = components_np(len(v), f)
        st = component_stats_np(v, f, vl, fl)
        sel = _select_components(st["n_faces"], st["n_faces"] if by == "faces" else st["area"], keep, min_frac)
        faces_k = f[sel[st["face_id"]]] if len(f) else f
        used = np.zeros(len(v), bool)
        used[faces_k.reshape(-1)] = True
        out_v, out_f = v[used], (np.cumsum(used) - 1)[faces_k].astype(np.int32).reshape(-1, 3)
        n_comp = int((st["n_faces"] > 0).sum())
    else:
        from . import ops

        ((v, f),), _ = _to_device(((verts, faces),))
        dev = v.device
        if weld:
            v, f, _ = ops.mesh_weld(v, f)
        vl, fl, _ = ops.mesh_components(v, f)
        st = ops.mesh_component_stats(v, f, vl, fl)
        # the one read-back of the selection: the exact face counts and the measure, (2, C) fp64
        host = torch.stack([st["n_faces"].double(), st["n_faces"].double() if by == "faces" else st["area"]])
        host = host.cpu().numpy()
        sel = _select_components(host[0], host[1], keep, min_frac)
        n_comp = int((host[0] > 0).sum())
        if f.shape[0]:
            faces_k = f[torch.from_numpy(sel).to(dev)[st["face_id"]]]
        else:
            faces_k = f
        used = torch.zeros(v.shape[0], device=dev, dtype=torch.bool)
        used[faces_k.long().reshape(-1)] = True
        out_v = v[used]
        out_f = (torch.cumsum(used, 0, dtype=torch.int64) - 1)[faces_k.long()].to(torch.int32).reshape(-1, 3)
    return out_v, out_f, {"n_components": n_comp, "n_components_kept": int(sel.sum()),
                          "faces_kept": int(out_f.shape[0])}


# ---- mesh rendering: cameras, the host ray cast, views of a mesh, silhouette scores ----------------
SIL_METRIC_NAMES = ("sil_iou", "sil_depth_l1", "sil_views")
_FILE_FLIP = np.diag([1.0, -1.0, -1.0, 1.0])


def sphere_poses(n_views, radius, hemisphere=True):
    """The cameras of the reference's Blender scripts: points of a golden spiral on the sphere of
    ``radius`` (point i of N: azimuth 2 pi i / golden ratio, polar angle arccos(1 - 2 (i + 0.5) / N)),
    each looking at the origin with the world's z axis up.  ``hemisphere`` takes N = 2 n_views points
    and keeps the upper half (the first n_views), else N = n_views over the whole sphere.  Returns
    ``(poses, file_poses)``, both (n_views, 4, 4) float64 camera-to-world: ``poses`` in the loader's
    convention (x right, y up, looking down -z: what SRNDataset returns and gen_rays takes) and
    ``file_poses`` as the pose files hold them; they differ by the diag(1, -1, -1, 1) the loader
    applies on the right."""
    n_views = int(n_views)
    if n_views < 1:
        raise ValueError("sphere_poses: n_views must be >= 1 (got %d)" % n_views)
    n = 2 * n_views if hemisphere else n_views
    i = np.arange(n, dtype=np.float64)
    theta = 2.0 * np.pi * i / ((1.0 + 5.0 ** 0.5) / 2.0)
    phi = np.arccos(1.0 - 2.0 * (i + 0.5) / n)
    pos = float(radius) * np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], -1)
    pos = pos[:n_views]
    z = pos / np.linalg.norm(pos, axis=1, keepdims=True)          # the camera looks down -z, at the origin
    x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y = np.cross(z, x)
    poses = np.tile(np.eye(4), (n_views, 1, 1))
    poses[:, :3, 0], poses[:, :3, 1], poses[:, :3, 2], poses[:, :3, 3] = x, y, z, pos
    return poses, poses @ _FILE_FLIP


def ssaa_camera(k, fx, fy, cx, cy):
    """(fx, fy, cx, cy) of the k x supersampled image whose k x k blocks are centred on the pixels'
    rays: fx k, fy k, cx k + (k - 1) / 2, cy k + (k - 1) / 2."""
    return fx * k, fy * k, cx * k + (k - 1) / 2.0, cy * k + (k - 1) / 2.0


def _raster(verts, faces, poses, width, height, fx, fy, cx, cy, backend):
    """(face, depth) on `backend`: device tensors from hip, arrays from numpy."""
    if backend == "numpy":
        return raycast_np(verts, faces, poses, width, height, (fx, fy), (cx, cy))
    from . import ops

    return ops.mesh_raster(verts, faces, poses, width, height, (fx, fy), (cx, cy))


def render_mesh_views(verts, faces, poses, width, height, focal, c=None, ssaa=1, backend="auto", **shading):
    """Shaded views of a mesh from a batch of cameras: a dict with ``rgb`` (NV, H, W, 3) float32 in
    [0, 1], ``mask`` (NV, H, W) float32 (the covered share of each pixel) and ``face`` / ``depth`` of
    the raster itself, (NV, k H, k W).  ``ssaa = k`` renders at k times the size with the camera
    ``ssaa_camera`` gives, whose k x k samples are centred on the pixel's ray, and box-averages the
    blocks of ``rgb`` and of the mask in torch.  ``shading``: the keyword arguments of
    ``ops.mesh_shade`` (lights, weights, albedo, ambient, background).  ``"hip"`` runs pnr.ops.mesh_raster
    / mesh_shade on the device the inputs are on (host inputs are moved to the current HIP device) and
    returns device tensors; ``"numpy"`` runs ``raycast_np`` / ``shade_np`` on the host and returns host
    tensors; ``"auto"`` is hip where a HIP device is present."""
    from . import util

    backend = _resolve_backend(backend, "render")
    k = int(ssaa)
    if k < 1:
        raise ValueError("render_mesh_views: ssaa must be >= 1 (got %d)" % k)
    width, height = int(width), int(height)
    fx, fy, cx, cy = ssaa_camera(k, *util._focal_c(width, height, focal, c))
    w, h = width * k, height * k
    if backend == "numpy":
        face, depth = raycast_np(verts, faces, poses, w, h, (fx, fy), (cx, cy))
        rgb, _ = shade_np(verts, faces, poses, w, h, (fx, fy), face, depth, c=(cx, cy), **shading)
        face, depth, rgb = torch.from_numpy(face), torch.from_numpy(depth).float(), torch.from_numpy(rgb).float()
    else:
        from . import ops

        ((verts, faces),), poses = _to_device(((verts, faces),), poses)
        face, depth = ops.mesh_raster(verts, faces, poses, w, h, (fx, fy), (cx, cy))
        rgb, _ = ops.mesh_shade(verts, faces, poses, w, h, (fx, fy), face, depth, c=(cx, cy), **shading)
    mask = (face >= 0).float()
    if k > 1:
        nv = rgb.shape[0]
        rgb = rgb.reshape(nv, height, k, width, k, 3).mean(dim=(2, 4))
        mask = mask.reshape(nv, height, k, width, k).mean(dim=(2, 4))
    return {"rgb": rgb, "mask": mask, "face": face, "depth": depth}


def silhouette_scores(pred, gt, poses, width, height, focal, c=None, backend="auto"):
    """The 2D scores of single-view reconstruction work: a predicted mesh against a ground-truth
    mesh, each a ``(verts, faces)`` pair of tensors or arrays, both seen from ``poses``.  Returns a
    dict of floats (SIL_METRIC_NAMES): ``sil_iou`` = the mean over the views of |A and B| / |A or B|
    of the two silhouettes (a view where both are empty counts 1), ``sil_depth_l1`` = the mean
    |depth_pred - depth_gt| over the pixels of all views that both cover (+inf when there is none),
    ``sil_views`` = the number of views.  A predicted mesh without faces is a result (it covers
    nothing); an empty ground truth raises.  Backends as in ``render_mesh_views``."""
    from . import util

    backend = _resolve_backend(backend, "render")
    (pv, pf), (gv, gf) = pred, gt
    if len(gf) == 0:
        raise ValueError("silhouette_scores: the ground-truth mesh has no faces")
    width, height = int(width), int(height)
    fx, fy, cx, cy = util._focal_c(width, height, focal, c)
    if backend == "hip":
        ((pv, pf), (gv, gf)), poses = _to_device((pred, gt), poses)
    nv = int(poses.shape[0])
    face_g, depth_g = _raster(gv, gf, poses, width, height, fx, fy, cx, cy, backend)
    if len(pf):
        face_p, depth_p = _raster(pv, pf, poses, width, height, fx, fy, cx, cy, backend)
    else:
        face_p, depth_p = face_g * 0 - 1, depth_g * 0
    if backend == "numpy":
        face_p, depth_p, face_g, depth_g = (torch.from_numpy(np.ascontiguousarray(t))
                                            for t in (face_p, depth_p, face_g, depth_g))
    a, b = (face_p >= 0).reshape(nv, -1), (face_g >= 0).reshape(nv, -1)
    inter, union = (a & b).sum(1).double(), (a | b).sum(1).double()
    iou = torch.where(union > 0, inter / union.clamp(min=1.0), torch.ones_like(union)).mean()
    both = (a & b).reshape(depth_p.shape)
    err = ((depth_p.double() - depth_g.double()).abs() * both).sum()
    out = torch.stack([iou, err, inter.sum()]).cpu().tolist()   # the one read-back
    return {"sil_iou": out[0], "sil_depth_l1": out[1] / out[2] if out[2] > 0 else float("inf"),
            "sil_views": float(nv)}
