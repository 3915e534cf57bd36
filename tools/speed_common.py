"""What the mesh speed tools (mesh_speed, mesh_metrics_speed, winding_speed, mesh_clean_speed,
mesh_render_speed) share: device-event timing, the statistics of a list of times, the read-only
shader clock, and the two synthetic density grids their meshes are extracted from."""
import glob
import statistics

import torch


def _stats(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), runs=len(ms))


def shader_clock_mhz():
    """The active level of every card's pp_dpm_sclk table (read only), or None."""
    out = []
    for path in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            with open(path) as f:
                out += [int(ln.split()[1].lower().replace("mhz", "")) for ln in f if ln.strip().endswith("*")]
        except (OSError, ValueError, IndexError):
            pass
    return out or None


def events(fn, warmup, reps):
    """Device-event milliseconds of ``reps`` calls of fn after ``warmup`` untimed ones."""
    ms = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return ms


def blob_grid(res, dev, bump):
    """A res^3 density: a sphere of radius 0.6 with a low-frequency bump of the given amplitude."""
    g = torch.linspace(-1, 1, res, device=dev)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    r = torch.sqrt(x * x + y * y + z * z)
    return (0.6 + bump * torch.sin(5 * x) * torch.cos(4 * y) * torch.sin(3 * z) - r).contiguous()


def floater_grid(res, dev, n_floaters, seed=0):
    """Two blobs (signed distance to two spheres, world units over [-1, 1]^3) and n_floaters single
    voxels set above the level, each at least 0.1 away from the blobs."""
    g = torch.linspace(-1, 1, res, device=dev)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    a = 0.45 - torch.sqrt((x + 0.3) ** 2 + y ** 2 + z ** 2)
    b = 0.25 - torch.sqrt((x - 0.5) ** 2 + (y - 0.3) ** 2 + z ** 2)
    grid = torch.maximum(a, b).contiguous()
    gen = torch.Generator().manual_seed(seed)
    p = torch.randint(2, res - 2, (4 * n_floaters, 3), generator=gen).to(dev)
    far = grid[p[:, 0], p[:, 1], p[:, 2]] < -0.1
    p = p[far][:n_floaters]
    grid[p[:, 0], p[:, 1], p[:, 2]] = 0.5
    return grid
