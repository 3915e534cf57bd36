"""Approximate PSNR / SSIM evaluation over an SRN-layout dataset.

Counterpart of eval/eval_approx.py:56-153: for every object one random target view is
rendered from the chosen source view(s) through ``render_par`` (bind_parallel,
simple_output) and scored against the ground-truth image with PSNR and SSIM at
data_range 1.  The view selection replays the reference's draws in order on torch's global
generator (seeded with ``seed``): per batch ``randint(0, NV, (SB, 1))`` for a random source,
then ``randint(0, NV - NS, (SB, 1))`` for the target, shifted past the sources.

``ssim`` restates skimage.measure.compare_ssim(X, Y, multichannel=True, data_range=1) with
its defaults (7 x 7 uniform window, sample covariance, K1 = 0.01, K2 = 0.03, per-channel
mean over the map cropped by 3 pixels); skimage is absent offline, so that restatement is
pinned by the brute-force window sum in tests/test_host.py, not by skimage itself.
"""
import numpy as np
import torch

from . import util

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


# ---- mesh reconstruction metrics (Occupancy Networks' eval_pointcloud) -----------------------------
MESH_METRIC_NAMES = ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "precision", "recall", "fscore",
                     "normals_accuracy", "normals_completeness", "normal_consistency")
_RNG_MESH = 4   # PNR_RNG_MESH


def _philox_uniform(seed, stream, count):
    """(count,) float32: U[0, 1) of elements e = 0 .. count - 1 of a counter-mode stream
    (include/pnr_abi.h pnr_rng: Philox4x32-10, counter (lo32 e, hi32 e, stream, 0), key = seed,
    (word 0 >> 8) * 2^-24)."""
    mask = np.uint64(0xFFFFFFFF)
    e = np.arange(count, dtype=np.uint64)
    c = [e & mask, e >> np.uint64(32), np.full(count, stream, np.uint64), np.zeros(count, np.uint64)]
    k = [np.uint64(int(seed) & 0xFFFFFFFF), np.uint64((int(seed) >> 32) & 0xFFFFFFFF)]
    for r in range(10):
        if r:
            k = [(k[0] + np.uint64(0x9E3779B9)) & mask, (k[1] + np.uint64(0xBB67AE85)) & mask]
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
    return (c[0] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _mesh_draws(seed, n):
    """(n, 3) float32: draws 0 .. 2 of rays 0 .. n - 1 of the counter-mode stream PNR_RNG_MESH
    (include/pnr_abi.h pnr_rng: Philox4x32-10, counter (lo32 e, hi32 e, stream, 0), e = 3 ray + k,
    key = seed, U[0, 1) = (word 0 >> 8) * 2^-24), what pnr_mesh_sample draws on the device."""
    return _philox_uniform(seed, _RNG_MESH, 3 * n).reshape(n, 3)


def sample_mesh_np(verts, faces, n, seed=0):
    """pnr_mesh_sample's rule on the host: ``(points (n, 3) float32, normals (n, 3) float32, tri (n,)
    int32, total area)``.  Areas in fp64 from the fp32 vertices, their inclusive sum with np.cumsum,
    the first face whose sum exceeds u0 * total, the fold of (u1, u2) at u1 + u2 > 1, the point
    a + u1 (b - a) + u2 (c - a) in fp32.  The device's sum runs in another fixed order, so a sample
    whose target lies within rounding of a face boundary may fall on the neighbouring face there."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    if f.shape[0] == 0 or f.min() < 0 or f.max() >= v.shape[0]:
        raise ValueError("sample_mesh_np: no faces, or a face index outside [0, %d)" % v.shape[0])
    a, b, c = (v[f[:, i]] for i in range(3))
    cr = np.cross(b.astype(np.float64) - a, c.astype(np.float64) - a)
    ln = np.sqrt(cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1] + cr[:, 2] * cr[:, 2])
    cdf = np.cumsum(0.5 * ln)
    total = float(cdf[-1])
    if not (total > 0.0 and np.isfinite(total)):
        raise ValueError("sample_mesh_np: the total area is %r, nothing to sample" % total)
    u = _mesh_draws(seed, n)
    tri = np.minimum(np.searchsorted(cdf, u[:, 0].astype(np.float64) * total, side="right"), len(cdf) - 1)
    u1, u2 = u[:, 1].copy(), u[:, 2].copy()
    fold = (u1 + u2) > np.float32(1.0)
    u1[fold], u2[fold] = np.float32(1.0) - u1[fold], np.float32(1.0) - u2[fold]
    pa, pb, pc = a[tri], b[tri], c[tri]
    points = (pa + u1[:, None] * (pb - pa)) + u2[:, None] * (pc - pa)
    normals = (cr[tri] / ln[tri][:, None]).astype(np.float32)
    return points.astype(np.float32), normals, tri.astype(np.int32), total


def nearest_np(a, b, chunk=2048):
    """(squared distance, index) of the nearest row of b for every row of a, in fp64 on the host:
    scipy's cKDTree where scipy imports, a chunked brute force otherwise."""
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    if cKDTree is not None:
        d, idx = cKDTree(b).query(a)
        return d * d, idx.astype(np.int64)
    d2 = np.empty(len(a))
    idx = np.empty(len(a), np.int64)
    for i in range(0, len(a), chunk):
        dd = ((a[i:i + chunk, None, :] - b[None, :, :]) ** 2).sum(-1)
        idx[i:i + chunk] = dd.argmin(1)
        d2[i:i + chunk] = dd[np.arange(dd.shape[0]), idx[i:i + chunk]]
    return d2, idx


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
    if backend == "auto":
        backend = "hip" if torch.cuda.is_available() else "numpy"
    if backend not in ("hip", "numpy"):
        raise ValueError("metrics backend must be 'auto', 'numpy' or 'hip' (got %r)" % (backend,))
    (pv, pf), (gv, gf) = pred, gt
    if len(gf) == 0:
        raise ValueError("mesh_metrics: the ground-truth mesh has no faces")
    if len(pf) == 0:
        return _empty_mesh_scores()
    if backend == "numpy":
        pv, pf, gv, gf = (t.detach().cpu().numpy() if torch.is_tensor(t) else t for t in (pv, pf, gv, gf))
        pa, na, _, _ = sample_mesh_np(pv, pf, n_samples, seed)
        pb, nb, _, _ = sample_mesh_np(gv, gf, n_samples, seed + 1)
        d2_ab, idx_ab = nearest_np(pa, pb)
        d2_ba, idx_ba = nearest_np(pb, pa)
        return _mesh_scores(d2_ab, idx_ab, d2_ba, idx_ba, na, nb, tau)
    from . import ops

    dev = next((t.device for t in (pv, pf, gv, gf) if torch.is_tensor(t) and t.device.type == "cuda"),
               torch.device("cuda", torch.cuda.current_device()))

    def on_dev(t, dtype):
        t = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
        return t.to(device=dev, dtype=dtype).reshape(-1, 3)

    pa, na, _, _ = ops.mesh_sample(on_dev(pv, torch.float32), on_dev(pf, torch.int32), n_samples, seed)
    pb, nb, _, _ = ops.mesh_sample(on_dev(gv, torch.float32), on_dev(gf, torch.int32), n_samples, seed + 1)
    scores = ops.mesh_distance(pa, na, pb, nb, tau)
    vals = torch.stack([scores[k] for k in MESH_METRIC_NAMES]).cpu().tolist()
    return dict(zip(MESH_METRIC_NAMES, vals))


# ---- mesh containment and volumetric IoU (Occupancy Networks' third headline score) ----------------
VOLUME_METRIC_NAMES = ("iou", "volume_pred", "volume_gt", "n_points")
_RNG_VOLUME = 5   # PNR_RNG_VOLUME


def _volume_draws(seed, n):
    """(n, 3) float32: draws 0 .. 2 of rays 0 .. n - 1 of the counter-mode stream PNR_RNG_VOLUME
    (width 3, offset 0, key = seed), what pnr_box_sample draws on the device."""
    return _philox_uniform(seed, _RNG_VOLUME, 3 * n).reshape(n, 3)


def box_sample_np(lo, hi, n, seed=0):
    """pnr_box_sample's rule on the host: (n, 3) float32, coordinate k = u_k * fl(hi_k - lo_k) + lo_k
    with one rounding.  The product is exact in fp64 and the sum is rounded there before it is
    rounded to fp32, so a coordinate differs from the device's fma by one ulp where the fp64 sum
    lands on an fp32 tie (about 2^-29 of the draws)."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    ext = (hi - lo).astype(np.float64)
    return (_volume_draws(seed, n).astype(np.float64) * ext + lo.astype(np.float64)).astype(np.float32)


def winding_np(verts, faces, points, chunk=None):
    """Generalized winding number on the host, (n,) float64: pnr_winding's formula (include/pnr_abi.h,
    "Mesh containment") in fp64 numpy on the fp32 inputs, ``chunk`` queries at a time (default: about
    2^21 pairs per step).  A face with an index outside [0, V) contributes 0."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    f = f[((f >= 0) & (f < len(v))).all(1)]
    w = np.zeros(len(p))
    if len(f) == 0 or len(p) == 0:
        return w
    tri = [v[f[:, k], c][None, :] for k in range(3) for c in range(3)]   # Ax Ay Az Bx ... Cz, each (1, T)
    if chunk is None:
        chunk = max(1, (1 << 21) // len(f))
    with np.errstate(invalid="ignore"):
        for i in range(0, len(p), chunk):
            q = [p[i:i + chunk, c, None] for c in range(3)]
            ax, ay, az, bx, by, bz, cx, cy, cz = (tri[3 * k + c] - q[c] for k in range(3) for c in range(3))
            la = np.sqrt(ax * ax + ay * ay + az * az)
            lb = np.sqrt(bx * bx + by * by + bz * bz)
            lc = np.sqrt(cx * cx + cy * cy + cz * cz)
            num = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)
            den = (la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la
                   + (cx * ax + cy * ay + cz * az) * lb)
            w[i:i + chunk] = (2.0 * np.arctan2(num, den)).sum(-1) / (4.0 * np.pi)   # arctan2(0, 0) = 0
    return w


def _signed_volume_np(v, f):
    t = np.asarray(v, np.float64)[np.asarray(f, np.int64)]
    return float(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)


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
    if backend == "auto":
        backend = "hip" if torch.cuda.is_available() else "numpy"
    if backend not in ("hip", "numpy"):
        raise ValueError("metrics backend must be 'auto', 'numpy' or 'hip' (got %r)" % (backend,))
    n_points = int(n_points)
    if n_points < 1:
        raise ValueError("volume_iou: n_points must be >= 1 (got %d)" % n_points)
    (pv, pf), (gv, gf) = pred, gt
    if len(gf) == 0:
        raise ValueError("volume_iou: the ground-truth mesh has no faces")
    empty = len(pf) == 0
    if backend == "numpy":
        pv, pf, gv, gf = (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (pv, pf, gv, gf))
        gv = np.ascontiguousarray(gv, np.float32).reshape(-1, 3)
        both = gv if empty else np.concatenate([np.ascontiguousarray(pv, np.float32).reshape(-1, 3), gv])
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

        dev = next((t.device for t in (pv, pf, gv, gf) if torch.is_tensor(t) and t.device.type == "cuda"),
                   torch.device("cuda", torch.cuda.current_device()))

        def on_dev(t, dtype):
            t = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
            return t.to(device=dev, dtype=dtype).reshape(-1, 3)

        def signed_volume(v, f):
            t = v.double()[f.long()]
            return (t[:, 0] * torch.linalg.cross(t[:, 1], t[:, 2])).sum() / 6.0

        gv, gf = on_dev(gv, torch.float32), on_dev(gf, torch.int32)
        if empty:
            both, vol_p = gv, torch.ones((), device=dev, dtype=torch.float64)
        else:
            pv, pf = on_dev(pv, torch.float32), on_dev(pf, torch.int32)
            both, vol_p = torch.cat([pv, gv]), signed_volume(pv, pf)
        vol_g = signed_volume(gv, gf)
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


def weld_np(verts):
    """pnr_mesh_weld's rule on the host (include/pnr_abi.h, "Mesh cleanup"): ``remap (V,) int32``,
    remap[i] = the lowest index whose three coordinates compare equal to vertex i's as floats (-0.0
    equals +0.0); a vertex with a NaN coordinate keeps remap[i] = i.  A lexicographic sort, then the
    minimum index of every run of equal rows."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    remap = np.arange(v.shape[0], dtype=np.int64)
    ok = np.nonzero(~np.isnan(v).any(1))[0]
    if ok.size:
        w = v[ok] + np.float32(0.0)   # -0 + 0 = +0: equal floats sort next to each other either way
        order = np.lexsort((w[:, 2], w[:, 1], w[:, 0]))
        s = w[order]
        start = np.concatenate([[True], (s[1:] != s[:-1]).any(1)])
        first = np.minimum.reduceat(ok[order], np.nonzero(start)[0])
        remap[ok[order]] = first[np.cumsum(start) - 1]
    return remap.astype(np.int32)


def _weld_apply_np(verts, faces):
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError("weld: a face index lies outside [0, %d)" % v.shape[0])
    remap = weld_np(v)
    keep = remap == np.arange(v.shape[0])
    new_index = np.cumsum(keep) - 1
    return v[keep], new_index[remap[f]].astype(np.int32).reshape(-1, 3), remap


def components_np(n_verts, faces):
    """pnr_mesh_components' labels on the host, pure numpy: ``(vert_label (V,) int32, face_label (T,)
    int32, n_components)``.  Two vertices are connected when a face names both; a label is the lowest
    vertex index of the component; a vertex no face names is its own component.  Rounds of "every
    face lowers the labels of its vertices, and of their labels, to the face's minimum", each followed
    by pointer jumping to a fixed point, until nothing changes."""
    n_verts = int(n_verts)
    f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= n_verts):
        raise ValueError("components: a face index lies outside [0, %d)" % n_verts)
    label = np.arange(n_verts, dtype=np.int64)
    while f.size:
        cur = label[f]
        low = cur.min(1)
        new = label.copy()
        for k in range(3):
            np.minimum.at(new, cur[:, k], low)
            np.minimum.at(new, f[:, k], low)
        while True:
            jump = new[new]
            if np.array_equal(jump, new):
                break
            new = jump
        if np.array_equal(new, label):
            break
        label = new
    face_label = label[f[:, 0]] if f.size else np.zeros(0, np.int64)
    return label.astype(np.int32), face_label.astype(np.int32), int((label == np.arange(n_verts)).sum())


def _face_terms_np(verts, faces):
    """(area (T,), volume term (T,)) in fp64 from the fp32 vertices, in the header's operation order."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w = b - a, c - a
    nx, ny, nz = (u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                  u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0])
    area = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    mx, my, mz = (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1], b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2],
                  b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])
    return area, (a[:, 0] * mx + a[:, 1] * my) + a[:, 2] * mz


def component_stats_np(verts, faces, vert_label, face_label):
    """ops.mesh_component_stats on the host: the same dict (numpy arrays).  The integer entries are
    those of the device; area and signed_volume are numpy's fp64 sums of the same per-face terms over
    each component's faces in ascending order (another summation order than the device's)."""
    vert_label, face_label = np.asarray(vert_label, np.int32), np.asarray(face_label, np.int32)
    labels = np.unique(vert_label)
    n_c = len(labels)
    vert_id, face_id = np.searchsorted(labels, vert_label), np.searchsorted(labels, face_label)
    cnt_v = np.bincount(vert_id, minlength=n_c).astype(np.int64)
    cnt_f = np.bincount(face_id, minlength=n_c).astype(np.int64)
    area, vol = np.zeros(n_c), np.zeros(n_c)
    if len(face_id):
        terms_a, terms_v = _face_terms_np(verts, faces)
        order = np.argsort(face_id, kind="stable")
        has = np.nonzero(cnt_f)[0]
        start = (np.cumsum(cnt_f) - cnt_f)[has]
        area[has] = np.add.reduceat(terms_a[order], start)
        vol[has] = np.add.reduceat(terms_v[order], start) / 6.0
    return {"labels": labels, "vert_id": vert_id.astype(np.int64), "face_id": face_id.astype(np.int64),
            "n_verts": cnt_v, "n_faces": cnt_f, "area": area, "signed_volume": vol}


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
    if backend == "auto":
        backend = "hip" if torch.cuda.is_available() else "numpy"
    if backend not in ("hip", "numpy"):
        raise ValueError("clean_mesh backend must be 'auto', 'numpy' or 'hip' (got %r)" % (backend,))
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
        v, f = (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (verts, faces))
        v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(f, np.int32).reshape(-1, 3)
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

        dev = next((t.device for t in (verts, faces) if torch.is_tensor(t) and t.device.type == "cuda"),
                   torch.device("cuda", torch.cuda.current_device()))

        def on_dev(t, dtype):
            t = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
            return t.to(device=dev, dtype=dtype).reshape(-1, 3).contiguous()

        v, f = on_dev(verts, torch.float32), on_dev(faces, torch.int32)
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


def _np_mesh(verts, faces):
    v, f = (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (verts, faces))
    return np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(f, np.int64).reshape(-1, 3)


def _np_poses(poses):
    p = poses.detach().cpu().numpy() if torch.is_tensor(poses) else np.asarray(poses)
    p = np.ascontiguousarray(p, np.float32).astype(np.float64)
    if p.ndim != 3 or p.shape[1] not in (3, 4) or p.shape[2] != 4:
        raise ValueError("poses must be (NV, 4, 4) or (NV, 3, 4) (got %s)" % (p.shape,))
    return p


def _pixel_dirs(width, height, fx, fy, cx, cy):
    """(X, -Y) of every pixel's direction (X, -Y, -1), (H W,) each, from the fp32 camera scalars."""
    fx, fy, cx, cy = (float(np.float32(t)) for t in (fx, fy, cx, cy))
    jj, ii = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    return ((ii - cx) / fx).reshape(-1), (-(jj - cy) / fy).reshape(-1)


def raycast_np(verts, faces, poses, width, height, focal, c=None, chunk=None):
    """pnr_mesh_raster's rule on the host (include/pnr_abi.h, "Mesh rendering"): ``(face (NV, H, W)
    int32, depth (NV, H, W) float64)`` by brute force over all pixels x faces in fp64 on the fp32
    inputs, ``chunk`` pixels at a time (default: about 2^21 pairs per step).  The same homogeneous hit
    rule (no two edge volumes of strictly opposite signs, not edge-on, depth > 0), the smallest
    camera-z depth wins and equal depths go to the lower face; faces with an index outside [0, V),
    a non-finite vertex or zero area, and views with a non-finite pose, contribute nothing."""
    from . import util

    v, f = _np_mesh(verts, faces)
    p = _np_poses(poses)
    width, height = int(width), int(height)
    fx, fy, cx, cy = util._focal_c(width, height, focal, c)
    X, Yn = _pixel_dirs(width, height, fx, fy, cx, cy)
    length = np.sqrt(X * X + Yn * Yn + 1.0)
    nv, hw = p.shape[0], width * height
    face = np.full((nv, hw), -1, np.int32)
    depth = np.zeros((nv, hw))
    ok = ((f >= 0) & (f < len(v))).all(1) if len(v) else np.zeros(len(f), bool)
    ids = np.nonzero(ok)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        tri = v.astype(np.float64)[f[ids]]                               # (T, 3, 3)
        area = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        good = np.isfinite(tri).all((1, 2)) & (area != 0).any(1) & np.isfinite(area).all(1)
    ids, tri = ids[good], tri[good]
    if len(ids) == 0:
        return face.reshape(nv, height, width), depth.reshape(nv, height, width)
    chunk = chunk or max(1, (1 << 21) // len(ids))
    for k in range(nv):
        if not np.isfinite(p[k, :3]).all():
            continue
        try:   # R^-1 (v - o), rows: the device takes the fp32 R for a rotation and uses R^T
            cam = (tri - p[k, :3, 3]) @ np.linalg.inv(p[k, :3, :3]).T
        except np.linalg.LinAlgError:
            continue
        a, b, cc = cam[:, 0], cam[:, 1], cam[:, 2]
        n_ab, n_bc, n_ca = np.cross(a, b), np.cross(b, cc), np.cross(cc, a)
        for i in range(0, hw, chunk):
            x, y = X[i:i + chunk, None], Yn[i:i + chunk, None]
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                e_ab = x * n_ab[:, 0] + y * n_ab[:, 1] - n_ab[:, 2]
                e_bc = x * n_bc[:, 0] + y * n_bc[:, 1] - n_bc[:, 2]
                e_ca = x * n_ca[:, 0] + y * n_ca[:, 1] - n_ca[:, 2]
                pos = (e_ab > 0) | (e_bc > 0) | (e_ca > 0)
                neg = (e_ab < 0) | (e_bc < 0) | (e_ca < 0)
                det = e_ab + e_bc + e_ca
                s = -(e_bc * a[:, 2] + e_ca * b[:, 2] + e_ab * cc[:, 2]) / det
                hit = ~(pos & neg) & (det != 0) & (s > 0) & np.isfinite(s)
            s = np.where(hit, s, np.inf)
            best = s.argmin(1)                                          # the first minimum: the lowest face
            sb = s[np.arange(len(best)), best]
            got = np.isfinite(sb)
            face[k, i:i + chunk] = np.where(got, ids[best], -1)
            depth[k, i:i + chunk] = np.where(got, sb * length[i:i + chunk], 0.0)
    return face.reshape(nv, height, width), depth.reshape(nv, height, width)


def shade_np(verts, faces, poses, width, height, focal, face, depth, c=None, lights=(), weights=(),
             albedo=(0.8, 0.8, 0.8), ambient=0.2, background=(1.0, 1.0, 1.0)):
    """pnr_mesh_shade's formula in fp64 on the host: ``(rgb (NV, H, W, 3), normal (NV, H, W, 3))``
    float64 from the face and depth of a raster (include/pnr_abi.h, "Mesh rendering", Shading)."""
    from . import util

    v, f = _np_mesh(verts, faces)
    p = _np_poses(poses)
    width, height = int(width), int(height)
    fx, fy, cx, cy = util._focal_c(width, height, focal, c)
    X, Yn = _pixel_dirs(width, height, fx, fy, cx, cy)
    u = np.stack([X, Yn, -np.ones_like(X)], -1)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    face = np.asarray(face).reshape(p.shape[0], -1)
    depth = np.asarray(depth, np.float64).reshape(p.shape[0], -1)
    rgb = np.empty(face.shape + (3,))
    normal = np.zeros(face.shape + (3,))
    rgb[:] = np.asarray(background, np.float64)
    for k in range(p.shape[0]):
        m = face[k] >= 0
        if not m.any():
            continue
        tri = v.astype(np.float64)[f[face[k][m]]]
        d = u[m] @ p[k, :3, :3].T
        pt = p[k, :3, 3] + depth[k][m, None] * d
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        n = np.where(((n * d).sum(1) > 0)[:, None], -n, n)
        lum = np.full(len(n), float(ambient))
        for L, w in zip(lights, weights):
            to = np.asarray(L, np.float64) - pt
            with np.errstate(invalid="ignore", divide="ignore"):
                cos = (n * to).sum(1) / np.linalg.norm(to, axis=1)
            lum += float(w) * np.where(cos > 0, cos, 0.0)
        rgb[k][m] = np.clip(np.asarray(albedo, np.float64) * lum[:, None], 0.0, 254.0 / 255.0)
        normal[k][m] = n
    shape = (p.shape[0], height, width, 3)
    return rgb.reshape(shape), normal.reshape(shape)


def _raster_backend(backend):
    if backend == "auto":
        backend = "hip" if torch.cuda.is_available() else "numpy"
    if backend not in ("hip", "numpy"):
        raise ValueError("render backend must be 'auto', 'numpy' or 'hip' (got %r)" % (backend,))
    return backend


def _raster(verts, faces, poses, width, height, fx, fy, cx, cy, backend):
    """(face, depth) on `backend`: device tensors from hip, arrays from numpy."""
    if backend == "numpy":
        return raycast_np(verts, faces, poses, width, height, (fx, fy), (cx, cy))
    from . import ops

    return ops.mesh_raster(verts, faces, poses, width, height, (fx, fy), (cx, cy))


def _to_device(verts, faces, poses):
    dev = next((t.device for t in (verts, faces, poses) if torch.is_tensor(t) and t.device.type == "cuda"),
               torch.device("cuda", torch.cuda.current_device()))

    def on_dev(t, dtype):
        t = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
        return t.to(device=dev, dtype=dtype).contiguous()

    return on_dev(verts, torch.float32).reshape(-1, 3), on_dev(faces, torch.int32).reshape(-1, 3), on_dev(
        poses, torch.float32)


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

    backend = _raster_backend(backend)
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

        verts, faces, poses = _to_device(verts, faces, poses)
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

    backend = _raster_backend(backend)
    (pv, pf), (gv, gf) = pred, gt
    if len(gf) == 0:
        raise ValueError("silhouette_scores: the ground-truth mesh has no faces")
    width, height = int(width), int(height)
    fx, fy, cx, cy = util._focal_c(width, height, focal, c)
    if backend == "hip":
        gv, gf, poses = _to_device(gv, gf, poses)
        if len(pf):
            pv, pf, _ = _to_device(pv, pf, poses)
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
