"""Matching of point lists on the device (csrc/match.hip).

``ball_match`` answers "which points of A have a point of B within r, and the other way round"
for two small host tables: what the reference asks of two ``cKDTree`` s and ``query_ball_tree``.
Its two consumers are step 7 (``detection.threshold_detections``: the std detections with no
correl detection near, reference steps.py:983-992) and ``true_purity``, the reference's
validation tool ``compute_true_purity`` (lib_origin.py:2375-2443) on a cube that stays in HBM.
"""
import numpy as np

from . import cubes, kernels

PURITY_COLUMNS = ("thresh", "ndetect", "ntrue", "nfalse", "nmiss", "purity")


def ball_match(ctx, a, b, r, a_val=None, want=None):
    """``a``, ``b``: three columns (x, y, z) each.  Returns a dict: ``a_hit`` (bool, one per point
    of ``a``: some point of ``b`` lies within ``r``), ``b_hit`` (the same seen from ``b``) and,
    with ``a_val`` (one value per point of ``a``, held as float32), ``b_max``: float64, the largest
    ``a_val`` over the points of ``a`` within ``r`` of each point of ``b``, ``-inf`` where there is
    none.  Within ``r`` means ``(dx*dx + dy*dy) + dz*dz <= r*r`` in float64 as NumPy rounds it.
    ``want``: the outputs to compute and return, all of them when None; a caller that needs
    ``a_hit`` alone (step 7) spares the device the flags of ``b`` and a query its cells after the
    first hit."""
    out = kernels.ball_match(ctx, a, b, r, a_val, want)
    return {k: v.astype(np.float64 if k == "b_max" else bool) for k, v in out.items()}


def true_purity(ctx, cube_local_max, ref_xyz, nref, maxdist=4.5, threshmin=4, threshmax=7):
    """The table of ``compute_true_purity`` (reference lib_origin.py:2386-2403) as a dict of
    columns ``thresh, ndetect, ntrue, nfalse, nmiss, purity`` in the reference's row order.

    ``cube_local_max``: anything ``cubes.resident`` takes; ``ref_xyz``: the three columns (x, y,
    z in pixels) of the reference lines; ``nref``: the count the misses are taken from.

    The reference builds a tree over the maxima above each of the thresholds and matches it with
    the tree of the reference lines.  Whether a maximum lies within ``maxdist`` of a line does not
    depend on the threshold, and the sets ``{T > thr}`` are nested, so one ``where_above`` at
    ``threshmin`` and one match give every row: a maximum is a true detection at ``thr`` when it
    is matched and ``T > thr``; a line is found at ``thr`` when the largest T among the maxima
    within ``maxdist`` of it exceeds ``thr``.  ``T`` is compared as float64, as ``where_above``
    does.  ``purity`` is NaN where ``ndetect == 0``."""
    w = cubes.where_above(cubes.resident(ctx, cube_local_max), threshmin)
    T = w["value"]
    m = ball_match(ctx, (w["x"], w["y"], w["z"]), ref_xyz, maxdist, a_val=T)
    thresh = np.arange(threshmin, threshmax, 0.1)
    ndetect = np.array([np.count_nonzero(T > thr) for thr in thresh], dtype=np.int64)
    ntrue = np.array([np.count_nonzero(m["a_hit"] & (T > thr)) for thr in thresh], dtype=np.int64)
    nmiss = np.array([nref - np.count_nonzero(m["b_max"] > thr) for thr in thresh], dtype=np.int64)
    nfalse = ndetect - ntrue
    with np.errstate(divide="ignore", invalid="ignore"):
        purity = 1 - nfalse / ndetect
    return dict(thresh=thresh, ndetect=ndetect, ntrue=ntrue, nfalse=nfalse, nmiss=nmiss,
                purity=purity)
