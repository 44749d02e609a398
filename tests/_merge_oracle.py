"""TEST INFRASTRUCTURE ONLY -- never imported by the product (origin_amd/).

The spatio-spectral merging of step 7 (reference lib_origin.py:1259-1387) restated in plain NumPy,
int64 / float64, without recursion and without astropy; tools/gen_merge_golden.py pins it to the
reference's own function (tests/golden/g12_merging.npz).  The float predicates are the
reference's own expressions.

Stage 1: seeds are the unmatched rows in ascending order.  A row m is eligible for seed s when
``not (hypot(xs - xm, ys - ym) > tol_spat * sqrt(2))`` or ``sqrt((zm - zs)**2) < tol_spec``; the
group of s is what near steps (``hypot(dx, dy) < tol_spat``) reach from s through rows that were
unmatched when s started and are eligible for s.  Renumbering: imatch -> rank of the seed, area
-> the group's maximum.  Stage 2, per area label > 0: for every group id cu of the label in
ascending order, with the ids alive at that moment as a snapshot (stop when one is left, skip cu
when it is gone), every other id otg of the snapshot in ascending order joins cu when the
smallest |dz| between their rows -- cu's rows as they are after the joins made so far -- is below
tol_spec.

Also here: the input cases of the fixture and of tests/test_merging.py, and a host union-find
for the components of the near graph.
"""
import numpy as np


def stage1(x, y, z, tol_spat, tol_spec):
    x, y, z = (np.asarray(v, np.int64) for v in (x, y, z))
    n = len(x)
    imatch = np.full(n, -1, np.int64)
    for s in range(n):
        if imatch[s] >= 0:
            continue
        cu_spat = np.hypot(x[s] - x, y[s] - y)
        eligible = ~(cu_spat > tol_spat * np.sqrt(2)) | (np.sqrt((z - z[s]) ** 2) < tol_spec)
        imatch[s] = s
        stack = [s]
        while stack:
            m = stack.pop()
            spatdist = np.hypot(x[m] - x, y[m] - y)
            ind = np.flatnonzero((spatdist < tol_spat) & (imatch < 0) & eligible)
            imatch[ind] = s
            stack.extend(ind.tolist())
    return imatch


def renumber(imatch, area):
    seeds, gid = np.unique(imatch, return_inverse=True)
    gmax = np.full(len(seeds), np.iinfo(np.int64).min)
    np.maximum.at(gmax, gid, np.asarray(area, np.int64))
    return gid.astype(np.int64), gmax[gid]


def stage2(gid, area, z, tol_spec):
    iout = np.array(gid, np.int64)
    z = np.asarray(z, np.int64)
    for label in np.unique(area):
        if label <= 0:
            continue
        ind = np.flatnonzero(area == label)
        zs = {g: z[ind[iout[ind] == g]] for g in np.unique(iout[ind])}
        for cu in sorted(zs):
            snapshot = sorted(zs)
            if len(snapshot) == 1:
                break
            if cu not in zs:
                continue
            for otg in snapshot:
                if otg == cu:
                    continue
                difz = zs[cu][:, None] - zs[otg][None, :]
                if np.sqrt(difz ** 2).min() < tol_spec:
                    zs[cu] = np.concatenate([zs[cu], zs.pop(otg)])
                    iout[ind[iout[ind] == otg]] = cu
    return iout


def merge(x, y, z, area, tol_spat, tol_spec):
    """dict(area, imatch2, imatch) in input row order, int64."""
    n = len(x)
    if n == 0:
        e = np.zeros(0, np.int64)
        return dict(area=e, imatch2=e.copy(), imatch=e.copy())
    gid, amax = renumber(stage1(x, y, z, tol_spat, tol_spec), area)
    return dict(area=amax, imatch2=gid, imatch=stage2(gid, amax, z, tol_spec))


def components(x, y, tol_spat):
    """Lowest row of every row's connected component of the near graph (host union-find)."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    n = len(x)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    cells = {}
    for r in range(n):
        cells.setdefault((int(x[r]), int(y[r])), []).append(r)
    w = int(np.ceil(tol_spat))
    offs = [(dx, dy) for dx in range(-w, w + 1) for dy in range(-w, w + 1)
            if np.hypot(dx, dy) < tol_spat]
    for (cx, cy), rows in cells.items():
        for dx, dy in offs:
            other = cells.get((cx + dx, cy + dy))
            if other:
                a, b = find(rows[0]), find(other[0])
                if a != b:
                    parent[max(a, b)] = min(a, b)
        for r in rows[1:]:
            a, b = find(rows[0]), find(r)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(r) for r in range(n)], np.int64)


def purity(comp, T_GLR, STD, Tval, Pval, Tval_comp, Pval_comp):
    """The reference's purity_estimation (:1941-1991) on plain arrays."""
    from scipy.interpolate import interp1d
    comp = np.asarray(comp)
    out = np.zeros(len(comp))
    for c, val, tv, pv in ((0, T_GLR, Tval, Pval), (1, STD, Tval_comp, Pval_comp)):
        ksel = comp == c
        if np.count_nonzero(ksel) > 0:
            f = interp1d(tv, pv, bounds_error=False, fill_value="extrapolate")
            out[ksel] = f(np.asarray(val, float)[ksel])
    return np.clip(out, 0, 1)


# ------------------------------------------------------------------------------------- the cases
def _case(name, rows, tol_spat=3, tol_spec=5, shape=None):
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    x, y, z, area = rows.T
    if shape is None:
        shape = (int(z.max()) + 1, int(y.max()) + 1, int(x.max()) + 1)
    return dict(name=name, x=x, y=y, z=z, area=area, tol_spat=tol_spat, tol_spec=tol_spec,
                shape=tuple(shape))


def case_one_spaxel():
    """300 rows in one spaxel: z spread over the cube, one group whatever dz is."""
    rng = np.random.default_rng(2)
    z = rng.integers(0, 3681, 300)
    return _case("one_spaxel", np.stack([np.full(300, 5), np.full(300, 7), z, np.zeros(300)], 1),
                 shape=(3681, 12, 12))


def case_thresholds(tol_spat, tol_spec=5):
    """Offsets on the thresholds around seeds.  Every pattern is a seed at (cx, cy), stepping
    stones that are near each other and close to the seed, and probes at chosen seed distances
    with dz = dzmax and dzmax + 1 (dzmax = ceil(tol_spec) - 1)."""
    t = int(np.ceil(tol_spat))
    dzmax = int(np.ceil(tol_spec)) - 1
    rows = []
    cx = 10

    def add(dx, dy, dz, cy):
        rows.append((cx + dx, cy + dy, 100 + dz, 0))
    cy = 10
    # (t, 0) is not near for an integer tol_spat; (t - 1, t - 1) is near when its hypot says so
    for k, (dx, dy) in enumerate([(t, 0), (0, t), (t - 1, t - 1), (t - 1, 0), (t, 1), (1, t)]):
        add(0, 0, 0, cy)
        add(dx, dy, 50, cy)       # dz far: joins only if near and within sqrt(2) tol of the seed
        cy += 3 * t + 8
    # seed distance on and around tol_spat * sqrt(2), reached over stepping stones one king move
    # apart with the seed's z (always eligible)
    for (dx, dy) in [(t, t), (t + 1, 1), (t + 1, 2), (t + 1, t - 1), (t, t + 1), (t + 1, t + 1)]:
        for dz in (dzmax, dzmax + 1, -dzmax, -dzmax - 1, 0):
            add(0, 0, 0, cy)
            px = py = 0
            while max(dx - px, dy - py) > 1:
                px, py = px + (px < dx), py + (py < dy)
                add(px, py, 0, cy)
            add(dx, dy, dz, cy)
            cy += 3 * t + 8
    return _case(f"thresholds_{tol_spat}_{tol_spec}", rows, tol_spat, tol_spec,
                 shape=(200, cy + 8, 40))


def case_chain(n=1500):
    """A serpentine of n rows two pixels apart (lines 8 apart, joined at the turns), z 100 / 101:
    one group as deep as the chain.  Beside every third row two more at z 140 / 141, one behind
    the other: ineligible for the chain's seed beyond its radius, so the first becomes a later
    seed and claims the second, which nothing else can reach.  Row order is shuffled."""
    rng = np.random.default_rng(4)
    per = 30
    path, side = [], []
    line = 0
    while len(path) < n:
        ks = range(per) if line % 2 == 0 else range(per - 1, -1, -1)
        for k in ks:
            path.append((2 * k, 8 * line))
            if k % 3 == 1:
                side.append((2 * k, 8 * line + 2, 140))
                side.append((2 * k, 8 * line + 4, 141))
        xe = path[-1][0]
        path += [(xe, 8 * line + d) for d in (2, 4, 6)]
        line += 1
    path = path[:n]
    ymax = max(p[1] for p in path)
    rows = [(px, py, 100 + i % 2, (i // 400) % 3) for i, (px, py) in enumerate(path)]
    rows += [(px, py, zz, 1) for px, py, zz in side if py <= ymax]
    rows = np.array(rows)
    return _case("chain", rows[rng.permutation(len(rows))], shape=(200, ymax + 1, 2 * per))


def case_two_seeds(swap):
    """Two seeds 6 apart with different z and rows between them that both reach: the lower
    seed row takes them."""
    a, b = (10, 10, 100, 0), (16, 10, 300, 0)
    rows = [b, a] if swap else [a, b]
    rows += [(12, 10, 100, 0), (14, 10, 300, 0), (13, 10, 200, 0), (8, 10, 100, 0),
             (18, 10, 300, 0)]
    return _case("two_seeds_swapped" if swap else "two_seeds", rows, shape=(400, 24, 24))


def case_crowded(n=5000, side=40, seed=6):
    """One component: n rows over a side x side field, a few z clusters, labels in patches."""
    rng = np.random.default_rng(seed)
    x, y = rng.integers(0, side, n), rng.integers(0, side, n)
    centres = rng.integers(20, 3660, 40)
    z = np.clip(centres[rng.integers(0, 40, n)] + rng.integers(-6, 7, n), 0, 3680)
    area = ((x // 10) + 4 * (y // 10)) % 5
    return _case("crowded", np.stack([x, y, z, area], 1), shape=(3681, side, side))


def case_isolated(n=1200):
    """n single detections 4 pixels apart: one component each."""
    rng = np.random.default_rng(7)
    k = np.arange(n)
    rows = np.stack([4 * (k % 40), 4 * (k // 40), rng.integers(0, 3681, n), k % 4], 1)
    return _case("isolated", rows[rng.permutation(n)], shape=(3681, 4 * (n // 40) + 1, 160))


def case_stage2():
    """Groups far apart in space (one row or a few rows each) that only the spectral stage can
    join."""
    rows = []
    sx = [0]

    def group(zs, label, labels=None):
        for i, zz in enumerate(zs):
            rows.append((sx[0] + (i % 2), 5 + (i // 2) % 2, zz, label if labels is None else labels[i]))
        sx[0] += 8
    # area 0 never merges, although the lines coincide
    group([500], 0), group([500], 0), group([501, 502], 0)
    # a group spanning labels 3 and 7 ends in 7, and meets the other group of 7 there
    group([900, 905], None, labels=[3, 7]), group([903], 7), group([2000], 3)
    # the non-transitive walk: a < b < c in label 11; b does not match a (dz 8), c matches a
    # (dz 4) and brings a within 4 of b
    group([1000], 11), group([1008], 11), group([1004], 11)
    # the same with the ids the other way round, label 12: here a absorbs on its own walk
    group([1100], 12), group([1104], 12), group([1108], 12)
    # b joins nothing at a's walk, absorbs at its own: label 13 (a, b, c, d)
    group([1200, 1230], 13), group([1210], 13), group([1214, 1226], 13), group([1206], 13)
    # an area left with one group at the first step
    group([1500], 14), group([1502], 14), group([1900], 15)
    # dz = 0 and dz exactly tol_spec
    group([1600], 16), group([1600], 16), group([1700], 17), group([1705], 17)
    # the last bitmap word is partial (Nz = 3681): channels 3676 .. 3680
    group([3680], 18), group([3676], 18), group([3671], 18), group([3648, 3679], 19), group([3652], 19)
    # word boundaries
    group([31], 20), group([32], 20), group([63, 64], 21), group([68], 21), group([0], 22), group([4], 22)
    # an area with 200 groups on a z ladder with gaps on both sides of tol_spec
    rng = np.random.default_rng(8)
    zz = np.cumsum(rng.integers(3, 9, 200)) + 100
    for i in rng.permutation(200):
        group([int(zz[i])] + ([int(zz[i]) + 1500] if i % 7 == 0 else []), 30)
    return _case("stage2", rows, shape=(3681, 12, sx[0] + 4))


def case_small(n):
    rows = [(3, 4, 10, 2), (4, 4, 30, 5)][:n]
    c = _case(f"n{n}", rows if n else np.zeros((0, 4)), shape=(40, 8, 8))
    return c


def golden_cases():
    return [case_small(2), case_one_spaxel(), case_thresholds(3), case_thresholds(2),
            case_thresholds(4), case_thresholds(3, 5.5), case_chain(), case_two_seeds(False),
            case_two_seeds(True), case_isolated(), case_stage2()]


def random_field(seed):
    """Clustered sources plus background on a random segmap with label 0 present, in the order
    ``vstack([correl, std])`` gives (each half in np.where order: z major)."""
    rng = np.random.default_rng(1000 + seed)
    side = int(rng.integers(40, 121))
    Nz = 400 if seed % 2 == 0 else 3681
    n = int(rng.integers(300, 3001))
    nsrc = int(rng.integers(5, 60))
    cy, cx = rng.integers(0, side, nsrc), rng.integers(0, side, nsrc)
    nlines = rng.integers(1, 4, nsrc)
    cz = rng.integers(0, Nz, (nsrc, 3))
    ncl = int(0.7 * n)
    s = rng.integers(0, nsrc, ncl)
    x = np.clip(cx[s] + np.rint(rng.normal(0, 1.6, ncl)).astype(int), 0, side - 1)
    y = np.clip(cy[s] + np.rint(rng.normal(0, 1.6, ncl)).astype(int), 0, side - 1)
    z = np.clip(cz[s, rng.integers(0, 3, ncl) % nlines[s]] + rng.integers(-3, 4, ncl), 0, Nz - 1)
    nbg = n - ncl
    x = np.concatenate([x, rng.integers(0, side, nbg)])
    y = np.concatenate([y, rng.integers(0, side, nbg)])
    z = np.concatenate([z, rng.integers(0, Nz, nbg)])
    segmap = np.zeros((side, side), np.int64)
    for lab in range(1, int(rng.integers(3, 12))):
        y0, x0 = rng.integers(0, side, 2)
        h, w = rng.integers(4, side // 2, 2)
        segmap[y0:y0 + h, x0:x0 + w] = lab
    p = rng.permutation(n)
    x, y, z = x[p], y[p], z[p]
    half = n * 2 // 3
    order = np.concatenate([np.lexsort((x[:half], y[:half], z[:half])),
                            half + np.lexsort((x[half:], y[half:], z[half:]))])
    x, y, z = x[order], y[order], z[order]
    tol_spat = [3, 3, 2, 4, 2.5][seed % 5]
    tol_spec = [5, 5, 3, 5.5][seed % 4]
    return dict(name=f"random{seed}", x=x, y=y, z=z, area=segmap[y, x], tol_spat=tol_spat,
                tol_spec=tol_spec, shape=(Nz, side, side))
