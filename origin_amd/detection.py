"""Thresholding of step 7 on the device (reference muse_origin/steps.py:935-994).

``Detection.run`` opens with three ``np.where(cube > threshold)`` scans of full host cubes
(:958, :968; ``det_correl_min`` :938) and fancy-indexed gathers at the hits (:962-963, :971).
With the cubes resident in HBM those are ordered stream compactions
(``origin_where_above``): only the detections leave the GPU, in the order ``np.where``
returns them, so everything downstream (``spatiospectral_merging``, the segmentation labels,
the WCS columns -- host code on 10^3..10^5 rows) sees the same table.

The second half (:1010-1036) is here as well: ``merge_detections`` is the reference's
``spatiospectral_merging`` (lib_origin.py:1259-1387) on the device (csrc/merge.hip, DESIGN.md
section 3h), ``make_cat1`` the table work around it, so that ``threshold_detections`` ->
``make_cat1`` -> ``lines.estimate_lines`` runs without leaving the package.

Tables are plain dicts of NumPy columns (astropy is not a dependency of this package);
``astropy.table.Table(cat0)`` gives the reference's ``Cat0`` before ``_format_cat``.
"""
import numpy as np

from . import cubes, kernels, match

CAT0_COLUMNS = ("x0", "y0", "z0", "comp", "STD", "T_GLR", "profile")


def det_correl_min(ctx, cube_local_min, thresh):
    """``Detection.det_correl_min`` (steps.py:935-939): positions above ``thresh`` in
    cube_local_min -> (zm, ym, xm)."""
    w = cubes.where_above(cubes.resident(ctx, cube_local_min), thresh)
    return w["z"], w["y"], w["x"]


def threshold_detections(ctx, cube_local_max, cube_profile, cube_std_local_max,
                         threshold_correl, threshold_std, maxdist_lines=2.5):
    """The first half of ``Detection.run`` (steps.py:956-994) on cubes in any form
    ``cubes.resident`` takes; ``cube_profile`` (uint8) in the form of ``cube_local_max``.

    Returns ``(cat0, cat_correl, cat_std_kept)``: ``cat0`` the raw detection table (correl
    rows, then std rows: the ``vstack`` of :981), ``cat_correl`` its correl rows and
    ``cat_std_kept`` the std rows farther than ``maxdist_lines`` from every correl detection
    (:983-994; in ascending row order) -- the two tables the reference stacks again at :1010.
    The match of :983-992 runs on the device (``match.ball_match``); ``unmatched_std`` is the
    host statement of the same rule.
    """
    c = cubes.where_above(cubes.resident(ctx, cube_local_max), threshold_correl,
                          aux=cubes.resident(ctx, cube_profile, np.uint8))
    s = cubes.where_above(cubes.resident(ctx, cube_std_local_max), threshold_std)
    n, m = c["z"].size, s["z"].size
    cat = dict(x0=c["x"], y0=c["y"], z0=c["z"], comp=np.zeros(n, int), STD=np.full(n, np.nan),
               T_GLR=c["value"], profile=c["aux"])
    cat_std = dict(x0=s["x"], y0=s["y"], z0=s["z"], comp=np.ones(m, int), STD=s["value"],
                   T_GLR=np.full(m, np.nan), profile=np.zeros(m, np.uint8))
    cat0 = {k: np.concatenate([cat[k], cat_std[k]]) for k in CAT0_COLUMNS}
    hit = match.ball_match(ctx, (cat_std["x0"], cat_std["y0"], cat_std["z0"]),
                           (cat["x0"], cat["y0"], cat["z0"]), maxdist_lines,
                           want=("a_hit",))["a_hit"]
    keep = np.flatnonzero(~hit)
    return cat0, cat, {k: v[keep] for k, v in cat_std.items()}


def from_session(orig, threshold=None, threshold_std=None, maxdist_lines=2.5):
    """``threshold_detections`` on the cubes a session holds (device copies left by steps 1 and
    5 when there are any, host cubes uploaded otherwise) with the thresholds of step 6
    (``param['threshold']``, ``param['threshold_std']``) unless given, like steps.py:951-954."""
    ctx = cubes.ctx_of(orig)
    thr = orig.param['threshold'] if threshold is None else threshold
    thr_std = orig.param['threshold_std'] if threshold_std is None else threshold_std
    prof = cubes.session_cube(orig, 'cube_profile', np.uint8)
    if prof.dtype != np.uint8:     # (a device copy somebody made with another element type)
        prof = ctx.to_device(cubes.host_array(prof).astype(np.uint8))
    return threshold_detections(ctx, cubes.session_cube(orig, 'cube_local_max'), prof,
                                cubes.session_cube(orig, 'cube_std_local_max'), thr, thr_std,
                                maxdist_lines)


def unmatched_std(cat, cat_std, maxdist_lines=2.5):
    """Rows of ``cat_std`` with no correl detection within ``maxdist_lines`` voxels
    (steps.py:983-992: two cKDTrees and ``query_ball_tree``), ascending."""
    from scipy.spatial import cKDTree

    n, m = len(cat["z0"]), len(cat_std["z0"])
    if n == 0 or m == 0:
        return np.arange(m)
    kdt_cor = cKDTree(np.array([cat["x0"], cat["y0"], cat["z0"]]).T)
    kdt_std = cKDTree(np.array([cat_std["x0"], cat_std["y0"], cat_std["z0"]]).T)
    hit = np.zeros(m, dtype=bool)
    for lst in kdt_cor.query_ball_tree(kdt_std, maxdist_lines):
        hit[lst] = True
    return np.flatnonzero(~hit)


def merge_detections(ctx, cat, tol_spat=3, tol_spec=5, shape=None):
    """``spatiospectral_merging`` (lib_origin.py:1319-1387) for ``cat``, a dict of columns with
    ``x0``, ``y0``, ``z0`` and ``area``.  Returns the reference's output table as a dict of
    columns: the input columns with ``area`` replaced by the largest label of the row's group,
    then 0-based ``imatch`` (after the spectral stage) and ``imatch2`` (before it), rows sorted
    by ``imatch`` and, inside one ``imatch``, by input row (the reference's unstable sort leaves
    that order open: DESIGN.md section 3h).  ``shape``: (Nz, Ny, Nx) of the cube, from the
    column maxima when None."""
    x, y, z = (np.asarray(cat[k]) for k in ("x0", "y0", "z0"))
    if shape is None:
        shape = tuple(int(v.max()) + 1 if len(v) else 1 for v in (z, y, x))
    res = kernels.merge_detections(ctx, x, y, z, cat["area"], shape, tol_spat, tol_spec)
    order = np.argsort(res["imatch"], kind="stable")
    out = {k: np.asarray(v)[order] for k, v in cat.items() if k not in ("imatch", "imatch2")}
    out["area"] = res["area"][order].astype(np.asarray(cat["area"]).dtype, copy=False)
    out["imatch"] = res["imatch"][order].astype(np.int64)
    out["imatch2"] = res["imatch2"][order].astype(np.int64)
    return out


def purity_estimation(cat, Pval, Pval_comp):
    """``purity_estimation`` (lib_origin.py:1941-1991): the ``purity`` column for a table with
    ``comp``, ``T_GLR`` and ``STD``: linear interpolation (extrapolated, clipped to [0, 1]) of
    ``Pval['Pval_r']`` over ``Pval['Tval_r']`` at T_GLR where ``comp == 0``, of ``Pval_comp`` at
    STD where ``comp == 1``."""
    from scipy.interpolate import interp1d

    comp = np.asarray(cat["comp"])
    purity = np.zeros(len(comp))
    for c, col, tab in ((0, "T_GLR", Pval), (1, "STD", Pval_comp)):
        ksel = comp == c
        if np.count_nonzero(ksel) > 0:
            f = interp1d(np.asarray(tab["Tval_r"]), np.asarray(tab["Pval_r"]), bounds_error=False,
                         fill_value="extrapolate")
            purity[ksel] = f(np.asarray(cat[col], dtype=float)[ksel])
    return np.clip(purity, 0, 1)


def make_cat1(ctx, cat_correl, cat_std_kept, segmap_label, Pval, Pval_comp, tol_spat=3,
              tol_spec=5, wcs=None, wave=None):
    """The second half of ``Detection.run`` (steps.py:1010-1036): ``Cat1`` from the two tables
    ``threshold_detections`` returns.  ``segmap_label``: (Ny, Nx) integer labels (an array, or an
    mpdaf Image).  ``Pval`` / ``Pval_comp``: the purity tables of step 6 (anything indexable by
    ``'Tval_r'`` / ``'Pval_r'``).  ``wcs`` / ``wave`` (mpdaf objects the caller owns) add ``ra``,
    ``dec``, ``lbda`` in front when given.  Columns, in the reference's order: ``ID [ra dec
    lbda] x0 y0 z0 comp STD T_GLR profile seg_label imatch imatch2 purity``; ``imatch`` /
    ``imatch2`` count from 1, ``ID`` runs 1..k in ``imatch`` order, rows are sorted by ``ID`` and
    inside one ``ID`` by input row."""
    cat = {k: np.concatenate([np.asarray(cat_correl[k]), np.asarray(cat_std_kept[k])])
           for k in CAT0_COLUMNS}
    seg = cubes.host_array(segmap_label)
    cat["area"] = seg[cat["y0"], cat["x0"]]
    shape = None
    if len(cat["z0"]):
        shape = (int(cat["z0"].max()) + 1,) + tuple(seg.shape)
    cat = merge_detections(ctx, cat, tol_spat, tol_spec, shape)
    out = {}
    if wcs is not None:
        dec, ra = wcs.pix2sky(np.stack((cat["y0"], cat["x0"])).T).T
        out["ra"], out["dec"] = ra, dec
    if wave is not None:
        out["lbda"] = wave.coord(cat["z0"])
    for k, v in cat.items():
        out["seg_label" if k == "area" else k] = v
    out["imatch"] = out["imatch"] + 1
    out["imatch2"] = out["imatch2"] + 1
    # sequential IDs in imatch order; the rows are sorted by imatch already
    ids = np.unique(out["imatch"], return_inverse=True)[1] + 1
    out = dict(ID=ids.astype(np.int64), **out)
    out["purity"] = purity_estimation(out, Pval, Pval_comp)
    return out


def cat1_from_session(orig, segmap_label=None, tol_spat=3, tol_spec=5, threshold=None,
                      threshold_std=None, maxdist_lines=2.5):
    """``from_session`` and then ``make_cat1`` with ``orig.Pval``, ``orig.Pval_comp``, ``orig.wcs``
    and ``orig.wave``: the ``Cat1`` of ``Detection.run``.  ``segmap_label=None`` uses
    ``orig.segmap_cont`` as it is: the reference's extra ``phot_deblend_sources`` pass over it
    (steps.py:1006) needs photutils and stays with the caller, who passes its result here."""
    _, cat, cat_std = from_session(orig, threshold, threshold_std, maxdist_lines)
    seg = orig.segmap_cont if segmap_label is None else segmap_label
    return make_cat1(cubes.ctx_of(orig), cat, cat_std, seg, orig.Pval, orig.Pval_comp, tol_spat,
                     tol_spec, getattr(orig, "wcs", None), getattr(orig, "wave", None))
