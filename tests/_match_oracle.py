"""Host oracles of the matching tests (test_match_cases.py, test_hip_match.py, test_true_purity.py).

``brute``: the predicate of ``origin_ball_match`` in NumPy float64, in the stated order.
``true_purity_trees``: a restatement of the reference's compute_true_purity table
(lib_origin.py:2383-2403) with ``scipy.spatial.cKDTree``, one tree per threshold.
``true_purity_direct``: the same table by per-threshold brute force, with no tree and no nesting
argument.
"""
import numpy as np

COLUMNS = ("thresh", "ndetect", "ntrue", "nfalse", "nmiss", "purity")


def pairs(a, b, r, chunk=512):
    """Boolean (n, m) matrix of ``(dx*dx + dy*dy) + dz*dz <= r*r`` in float64: NumPy rounds every
    difference, product and sum separately, in this order."""
    ax, ay, az = (np.asarray(c, np.float64) for c in a)
    bx, by, bz = (np.asarray(c, np.float64) for c in b)
    r2 = np.float64(r) * np.float64(r)
    out = np.zeros((ax.size, bx.size), bool)
    for i in range(0, ax.size, chunk):
        s = slice(i, i + chunk)
        dx = ax[s, None] - bx[None, :]
        dy = ay[s, None] - by[None, :]
        dz = az[s, None] - bz[None, :]
        out[s] = (dx * dx + dy * dy) + dz * dz <= r2
    return out


def d2(a, b, chunk=512):
    """The float64 (n, m) matrix of the left-hand side above."""
    ax, ay, az = (np.asarray(c, np.float64) for c in a)
    bx, by, bz = (np.asarray(c, np.float64) for c in b)
    out = np.zeros((ax.size, bx.size))
    for i in range(0, ax.size, chunk):
        s = slice(i, i + chunk)
        dx = ax[s, None] - bx[None, :]
        dy = ay[s, None] - by[None, :]
        dz = az[s, None] - bz[None, :]
        out[s] = (dx * dx + dy * dy) + dz * dz
    return out


def brute(a, b, r, a_val=None):
    """``a_hit`` / ``b_hit`` (bool) and, with ``a_val``, ``b_max`` (float32, -inf where no point of
    ``a`` is within ``r``) from the pair matrix."""
    p = pairs(a, b, r)
    out = dict(a_hit=p.any(axis=1), b_hit=p.any(axis=0))
    if a_val is not None:
        v = np.asarray(a_val, np.float32)
        out["b_max"] = np.where(p, v[:, None], np.float32(-np.inf)).max(axis=0, initial=-np.inf) \
            .astype(np.float32)
    return out


def tree_pairs(a, b, r):
    """The pair matrix as ``cKDTree(A).query_ball_tree(cKDTree(B), r)`` gives it."""
    from scipy.spatial import cKDTree

    A = np.array([np.asarray(c, np.float64) for c in a]).T.reshape(-1, 3)
    B = np.array([np.asarray(c, np.float64) for c in b]).T.reshape(-1, 3)
    out = np.zeros((len(A), len(B)), bool)
    if len(A) == 0 or len(B) == 0:
        return out
    for i, lst in enumerate(cKDTree(A).query_ball_tree(cKDTree(B), r)):
        out[i, lst] = True
    return out


def _table(rows):
    cols = {k: np.array([row[i] for row in rows]) for i, k in enumerate(COLUMNS[:5])}
    for k in COLUMNS[1:5]:
        cols[k] = cols[k].astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        cols["purity"] = 1 - cols["nfalse"] / cols["ndetect"]                  # :2403
    return cols


def true_purity_trees(cube, ref_xyz, nref, maxdist=4.5, threshmin=4, threshmax=7):
    """lib_origin.py:2383-2403 restated: a tree over the reference lines (:2383); the voxels above
    ``threshmin`` with their values (:2386-2388); per threshold of ``arange(threshmin, threshmax,
    0.1)`` (:2390) the voxels with T > thr (:2394), a tree over them (:2396), the non-empty
    neighbour lists of ``query_ball_tree`` (:2397), their number as ntrue (:2398) and ``nref`` less
    the distinct lines in them as nmiss (:2399); nfalse = ndetect - ntrue (:2400).  ``cube``: host
    array whose values are compared as float64."""
    from scipy.spatial import cKDTree

    cube = np.asarray(cube).astype(np.float64)
    ref = np.array([np.asarray(c, np.float64) for c in ref_xyz]).T.reshape(-1, 3)
    kdref = cKDTree(ref) if len(ref) else None
    z, y, x = np.where(cube > threshmin)
    T = cube[z, y, x]
    rows = []
    for thr in np.arange(threshmin, threshmax, 0.1):
        sel = T > thr
        ndetect = int(sel.sum())
        lists = []
        if ndetect and kdref is not None:
            kdt = cKDTree(np.array([x[sel], y[sel], z[sel]], dtype=np.float64).T)
            lists = [lst for lst in kdt.query_ball_tree(kdref, maxdist) if lst]
        ntrue = len(lists)
        found = set()
        for lst in lists:
            found.update(lst)
        rows.append((thr, ndetect, ntrue, ndetect - ntrue, nref - len(found)))
    return _table(rows)


def true_purity_direct(cube, ref_xyz, nref, maxdist=4.5, threshmin=4, threshmax=7):
    """The same table with the brute-force predicate on the voxels above each threshold."""
    cube = np.asarray(cube).astype(np.float64)
    rows = []
    for thr in np.arange(threshmin, threshmax, 0.1):
        z, y, x = np.where(cube > thr)
        p = pairs((x, y, z), ref_xyz, maxdist)
        ntrue = int(p.any(axis=1).sum())
        rows.append((thr, len(z), ntrue, len(z) - ntrue, nref - int(p.any(axis=0).sum())))
    return _table(rows)
