"""Compat shim: ``util.recon`` (reference src/util/recon.py) on the device extractor.

``marching_cubes`` keeps the reference's grid (util.gen_grid over [c1, c2], 'ij' order), its fake
view directions (towards the origin; the grid point AT the origin gets NaN directions as in the
reference, which the extractor counts as outside), its ``(c2 - c1) / reso`` scaling (not
``reso - 1``: recon.py:74) and its ``+ c1`` offset.  The isosurface comes from
pnr.ops.marching_cubes instead of PyMCubes.  PyMCubes is not installed where this project is
built, so its own triangle winding cannot be pinned here: this shim winds like skimage's default
(normals towards lower sigma), and a caller that depends on PyMCubes' orientation should check it
against that library once."""
import warnings

import numpy as np
import torch

from pnr import ops
from pnr.mesh import save_obj  # noqa: F401
from pnr.util import gen_grid


def marching_cubes(occu_net, c1=[-1, -1, -1], c2=[1, 1, 1], reso=[128, 128, 128], isosurface=50.0, sigma_idx=3,
                   eval_batch_size=100000, coarse=True, device=None):
    """recon.py:12-78: (vertices (V, 3) float64, triangles (T, 3) int32) numpy arrays."""
    if occu_net.use_viewdirs:
        warnings.warn("Running marching cubes with fake view dirs (pointing to origin), output may be invalid")
    with torch.no_grad():
        grid = gen_grid(*zip(c1, c2, reso), ij_indexing=True)
        is_train = occu_net.training
        print("Evaluating sigma @", grid.size(0), "points")
        occu_net.eval()
        if device is None:
            device = next(occu_net.parameters()).device
        grid = grid.to(device=device)
        sigmas = torch.empty(grid.size(0), device=device)
        vd_all = -grid / torch.norm(grid, dim=-1).unsqueeze(-1) if occu_net.use_viewdirs else None
        for i in range(0, grid.size(0), eval_batch_size):
            pnts = grid[i:i + eval_batch_size][None]
            if vd_all is not None:
                out = occu_net(pnts, coarse=coarse, viewdirs=vd_all[i:i + eval_batch_size][None])
            else:
                out = occu_net(pnts, coarse=coarse)
            sigmas[i:i + eval_batch_size] = out[0, :, sigma_idx]
        print("Running marching cubes")
        verts, faces = ops.marching_cubes(sigmas.view(*reso).contiguous(), isosurface)
        vertices = verts.cpu().numpy().astype(np.float64)
        triangles = faces.cpu().numpy()
        c1, c2 = np.array(c1), np.array(c2)
        vertices *= (c2 - c1) / np.array(reso)
    if is_train:
        occu_net.train()
    return vertices + c1, triangles
