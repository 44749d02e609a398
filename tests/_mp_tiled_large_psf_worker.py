"""Worker of the large-PSF tiled GLR test (one process per rank, host group, all ranks on GPU 0):
a TiledGLR over a given cube_faint with a P = TILED_P PSF, without the PCA in front (the tile is
put where the PCA would write it).  Writes the tile's correl / correl_min / profile and how many
rectangles ran ahead of the halo exchange."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from origin_amd import multigpu, synth  # noqa: E402


def field(P):
    """(cube_faint, mask, psf, profiles): 150 x 320 spaxels, areas of 50."""
    Nz, Ny, Nx = 64, 150, 320
    rng = np.random.default_rng(P)
    cube = rng.standard_normal((Nz, Ny, Nx)).astype(np.float32)
    cube[20:30, 70, 160] += 25.0
    cube[40:44, 10, 300] += 30.0
    mask = (rng.random((Nz, Ny, Nx)) < 0.005).astype(np.uint8)
    psf = synth.moffat_psf(Nz, P).astype(np.float64)
    return cube, mask, psf, synth.dico_fwhm(3)


def tiling(world, P, Ny, Nx):
    return multigpu.Tiling(Ny, Nx, world, halo=P // 2 + 1, area_size=50)


def main():
    out = sys.argv[1]
    P = int(os.environ["TILED_P"])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    comm = multigpu.init_comm(rank, world, 0, backend="host")
    cube, mask, psf, prof = field(P)
    Nz, Ny, Nx = cube.shape
    til = tiling(world, P, Ny, Nx)
    t = til.tile(rank)
    sl = (slice(None), slice(t.y0, t.y1), slice(t.x0, t.x1))
    from origin_amd.device import Context
    ctx = Context(0)
    d_mask = ctx.to_device(np.ascontiguousarray(mask[sl]))
    glr = multigpu.TiledGLR(ctx, comm, til, rank, Nz, psf, prof, pcut=1e-8)
    # the tile in the interior of the halo-extended buffer, where a greedy PCA run with
    # into=glr.faint_target() leaves it; run(None, ...) then starts the interior regions ahead of
    # the exchange that fills the halo
    ext, top, left = glr.faint_target()
    shape = cube[sl].shape
    host = np.zeros(glr.eshape, np.float32)
    host[:, top:top + shape[1], left:left + shape[2]] = cube[sl]
    ext.upload(host)
    correl, cmin = ctx.empty(shape, np.float32), ctx.empty(shape, np.float32)
    profile = ctx.empty(shape, np.uint8)
    glr.run(None, d_mask, correl, profile, cmin)
    ctx.sync()
    np.savez(f"{out}.rank{rank}.npz", y0=t.y0, y1=t.y1, x0=t.x0, x1=t.x1,
             correl=correl.to_host(), correl_min=cmin.to_host(), profile=profile.to_host(),
             n_early=len(glr.last_rects[0]), spatial_mfma=int(glr.plan.spatial_on_matrix_cores),
             rows=int(glr.plan.rows_supported()))
    comm.barrier()
    comm.close()


if __name__ == "__main__":
    main()
