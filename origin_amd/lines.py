"""Line estimation of step 8 on the device (reference muse_origin/lib_origin.py:1805-1938,
called by ``ComputeSpectra.run``, steps.py:1082-1096).

For every detection the reference cuts an (Nz, P, P) column out of raw and var and runs
``method_PCA_wgt`` (:1535-1617: two leading singular vectors, two weighted least-squares
deconvolutions against the PSF, a DCT denoising) at each of the ``(2 size_grid + 1)^2`` grid
positions, in a Python loop.  Here all (detection, grid offset) problems of a batch run together
(``origin_lines_estimate``, csrc/lines.hip) on the cubes that stay in HBM; only the winning grid
offset's line, variance, flux, residual and position leave the GPU.

Tables are plain dicts of NumPy columns, as in ``detection.py``.  The WCS columns of the
reference's ``Cat2`` (``ra``, ``dec``, ``lbda``, :1922-1925) and the trimming of the lines into
``Spectrum`` objects (steps.py:1103-1125) need mpdaf and stay with the caller.

Deviations from the reference:

* a window that holds a non-finite raw value, a var that is NaN or <= 0, or a channel whose
  ``sum psf^2 / var`` is 0 is degenerate and takes no part in the grid; a detection left without
  grid offsets, or whose criterion is not finite, gets the fallback row ``(0.0, 1e6, [0], [0],
  y0, x0, z0)`` of :1760-1769.  (The reference hands NaN to ARPACK there.)
* grid offsets outside the field do not compete (the reference leaves 0 / inf in their cells);
* ties between grid offsets go to the first in ``np.where`` order (the reference raises);
* weighted fields (mosaics) are supported for ``size_grid == 0`` only -- ``ComputeSpectra``'s
  default; the reference's own loop overwrites its ``psf`` after the first grid position.
"""
import numpy as np

from . import cubes, kernels

NEW_COLUMNS = ("x", "y", "z", "residual", "flux", "num_line")
CRITERIA = ("flux", "mse")


def check_arguments(weights, size_grid, criteria):
    if criteria not in CRITERIA:
        raise ValueError("Bad criteria: (flux) or (mse)")
    if weights is not None and size_grid > 0:
        raise ValueError("weighted fields are supported for size_grid == 0 only")


def make_cat2(cat, res):
    """The input columns plus x, y, z, residual, flux, num_line in the reference's order
    (:1927-1936: ``ra dec lbda x0 x y0 y z0 z T_GLR profile residual flux num_line``): x, y, z
    behind x0, y0, z0, the other three at the end."""
    n = len(res["flux5"])
    new = dict(x=res["yxz"][:, 1].astype(np.int64), y=res["yxz"][:, 0].astype(np.int64),
               z=res["yxz"][:, 2].astype(np.int64), residual=res["mse5"].astype(np.float64),
               flux=res["flux5"].astype(np.float64), num_line=np.arange(1, n + 1))
    out = {}
    for k, v in cat.items():
        if k in new:
            continue
        out[k] = np.array(v, copy=True)
        if k in ("x0", "y0", "z0"):
            out[k[0]] = new[k[0]]
    for k in ("residual", "flux", "num_line"):
        out[k] = new[k]
    return out


def estimate_lines(ctx, cat, raw, var, psf, weights=None, size_grid=0, criteria='flux',
                   order_dct=30, horiz_psf=1, horiz=5, max_problems=0):
    """``estimation_line`` for the detections of ``cat`` (a dict of NumPy columns with ``x0``,
    ``y0``, ``z0``, as ``detection.threshold_detections`` makes) on the float32 device cubes
    ``raw`` and ``var``.  ``psf``: (Nz, P, P), or one per field with ``weights`` (one (Ny, Nx) map
    per field).  Returns ``(cat2, lin_est, var_est)``: the new table and, per detection, the
    estimated line and its variance as float64 arrays (``[0]`` for a fallback row).
    ``max_problems``: at most that many (detection, grid offset) problems per batch (default:
    sized from the free device memory); results do not depend on it."""
    check_arguments(weights, size_grid, criteria)
    res = kernels.lines_estimate(ctx, raw, var, psf, weights, cat["z0"], cat["y0"], cat["x0"],
                                 size_grid, CRITERIA.index(criteria), order_dct, horiz_psf, horiz,
                                 max_problems)
    fb = res["fallback"] != 0
    lin_est = [np.zeros(1) if f else row for f, row in zip(fb, res["line"])]
    var_est = [np.zeros(1) if f else row for f, row in zip(fb, res["var"])]
    return make_cat2(cat, res), lin_est, var_est


def from_session(orig, cat1, grid_dxy=0):
    """``estimate_lines`` as ``ComputeSpectra.run`` calls it (steps.py:1082-1096: criteria
    'flux', order_dct 30, horiz_psf 1, horiz 5) on what a session holds: the device copies of
    cube_raw and var that step 1 uploaded (uploaded now otherwise), ``orig.PSF`` and
    ``orig.wfields``."""
    ctx = cubes.ctx_of(orig)
    raw, var, _ = cubes.inputs_on_device(orig, ctx)
    return estimate_lines(ctx, cat1, raw, var, orig.PSF, orig.wfields, size_grid=grid_dxy)
