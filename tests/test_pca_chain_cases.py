"""The inputs of tests/test_hip_pca_chain.py and everything about them that needs no GPU.

Every case is a seeded field (float32 noise of unit variance plus planted spectra with amplitudes
a0 r^j (a0 = 5 but for case F), thresholds half-way between two sorted O2 values) aimed at one branch of the launch arithmetic
of the greedy PCA's per-iteration chain (csrc/pca.hip), as restated in _pca_chain_geometry.py.
Checked here:
  1. the stepwise restatement (_pca_chain_oracle.py) equals cpu_ref.Compute_GreedyPCA_area(...,
     itermax=t, svd="dense") at every checkpoint: mapO2 and nstop equal, F to 1e-12 relative;
  2. at 256 CUs every case reaches the geometry it is aimed at (a condition on the input);
  3. the inputs are decidable: threshold margin >= 1e-6 and background-boundary margin >= 1e-9 at
     every iteration, eigen gap >= 0.02 (case E: 0.004), and the SVD and Gram restatements closer
     than one float32 ulp of max|X|.
No library load.
"""
import functools

import numpy as np
import pytest

import _pca_chain_geometry as geo
import _pca_chain_oracle as orc
from oracle import cpu_ref


RHO = 1e-11    # residual bound of the eigen-solvers (header of test_hip_pca_batches.py)


# ------------------------------------------------------------------------------------ building blocks
def o2(X):
    return np.mean(np.asarray(X, dtype=np.float64) ** 2, axis=0)


def halfway(X, spx, k):
    """Threshold half-way between the k-th and the (k+1)-th largest O2 of the area: k nuisances."""
    s = np.sort(o2(X[:, spx]))[::-1]
    return float(0.5 * (s[k - 1] + s[k]))


def plant(X, where, rng, r, a0=5.0, j0=0):
    """Independent unit-variance spectra with amplitudes a0 r^j (j = j0, j0+1, ...) at `where`."""
    Nz = X.shape[0]
    for j, s in enumerate(where):
        X[:, s] += np.float32(a0 * r ** (j0 + j)) * rng.standard_normal(Nz).astype(np.float32)


def scattered_labels(runs, S, seed, keep=0):
    """Flat label vector: the runs (label, count) in raster order, then a tenth of the positions
    behind the first `keep` swapped at random, so that no area is a rectangle or contiguous."""
    lab = np.concatenate([np.full(c, l) for l, c in runs])
    assert len(lab) == S
    rng = np.random.default_rng(seed)
    pick = keep + rng.choice(S - keep, (S - keep) // 10, replace=False)
    lab[pick] = lab[rng.permutation(pick)]
    return lab


class Case:
    """A field (X: float32 (Nz, S)), its areas and thresholds, and how the device is to run it."""

    def __init__(self, name, X, shape, labels, thr, noise_pop=50, inplace=False, checkpoints=None,
                 gap_min=0.02):
        self.name, self.X, self.shape = name, X, shape
        self.Nz, self.S = X.shape
        assert shape[0] * shape[1] == self.S and X.dtype == np.float32
        self.areamap = np.asarray(labels).reshape(shape)
        self.nb = len(thr)
        self.spx = [np.flatnonzero(np.asarray(labels) == a + 1) for a in range(self.nb)]
        self.sizes = [len(s) for s in self.spx]
        self.thr, self.noise_pop, self.inplace = list(thr), noise_pop, inplace
        self.X64 = X.astype(np.float64)
        self.tests = [o2(self.X64[:, s]) for s in self.spx]
        self._checkpoints, self.gap_min = checkpoints, gap_min

    @functools.cached_property
    def records(self):
        return orc.run(self.X64, self.spx, self.thr, self.noise_pop, "svd")

    @functools.cached_property
    def records_gram(self):
        return orc.run(self.X64, self.spx, self.thr, self.noise_pop, "gram")

    @property
    def last(self):
        return len(self.records) - 1

    @property
    def checkpoints(self):
        if self._checkpoints is None:
            return list(range(self.last + 1))
        return sorted({min(t, self.last) for t in self._checkpoints} | {self.last})

    def works(self, upto=None):
        """Per executed iteration [(area, n, nb)] of the areas with n >= 2 (what the device runs)."""
        out = []
        for r in self.records[:self.last if upto is None else min(upto, self.last)]:
            w = [(a, n, nb) for a, n, nb, _ in r.work()]
            if not w:
                break
            out.append(w)
        return out

    def geometry(self, num_cu, upto=None):
        return geo.run(num_cu, self.Nz, self.S, self.sizes, self.works(upto), self.inplace)

    def n_sequence(self, a):
        return [r.steps[a].n for r in self.records if r.steps[a] is not None]

    def bound(self, t):
        """What test_hip_pca_chain.py allows at checkpoint t beside the half ulp of the last
        rounding: (record, E (S,), untouched (S,) bool).  E[s] = T_s * 2 rho / gamma * ||X[:, s]||_2
        with T_s the vectors removed from s's area so far and gamma the smallest eigen gap of that
        area so far, plus 0.5 sqrt(Nz) ulp32(max_z |X[:, s]|) per flush before the last one;
        untouched: spaxels outside every area or in an area that has not removed a vector."""
        r = orc.at(self.records, t)
        done = self.records[:min(t, self.last)]               # the iterations executed
        _, flushes = self.geometry(256, upto=t)               # (the CU count does not move a flush)
        midrun = sum(not f["final"] for f in flushes)
        E, untouched = np.zeros(self.S), np.ones(self.S, bool)
        for a, spx in enumerate(self.spx):
            gaps = [q.steps[a].gap for q in done
                    if q.steps[a] is not None and q.steps[a].gap is not None]
            assert r.T[a] == len(gaps)
            if not gaps:
                continue
            untouched[spx] = False
            E[spx] = len(gaps) * 2 * RHO / min(gaps) * np.linalg.norm(self.X64[:, spx], axis=0)
            E[spx] += midrun * 0.5 * np.sqrt(self.Nz) * orc.ulp32(
                np.max(np.abs(self.X64[:, spx]), axis=0))
        return r, E, untouched

    def distance(self):
        """max |F_svd - F_gram| over all records, and whether the discrete outputs agree."""
        assert len(self.records) == len(self.records_gram)
        d = 0.0
        for r, g in zip(self.records, self.records_gram):
            assert np.array_equal(r.mapO2, g.mapO2) and r.nstop == g.nstop
            d = max(d, float(np.max(np.abs(r.F - g.F))))
        return d


# ------------------------------------------------------------------------------------ the cases
A_NZ = (3, 16, 17, 33, 250, 257)
A_SEED = {3: 1, 16: 1, 17: 1, 33: 2, 250: 1, 257: 1}
# targets of the S = 300 field at 256 CUs: gather (nzb, gzper, last), deflate (nzs, zper, last),
# flush nxb * nzb and its padding
A_TARGETS = {
    3: ((1, 16, 3), (3, 1, 1), 2, 6),
    16: ((1, 16, 16), (16, 1, 1), 2, 6),
    17: ((2, 16, 1), (17, 1, 1), 2, 6),
    33: ((3, 16, 1), (17, 2, 1), 4, 4),
    250: ((16, 16, 10), (32, 8, 2), 16, 0),
    257: ((9, 32, 1), (29, 9, 5), 18, 6),
}


def case_slices(Nz, S):
    """A: one area of 300 spaxels with 6 sources, in place, in a field of S = 300 (the iterating
    area covers the field: deflate_dot_rows_kernel) or S = 700 (deflate_dot_kernel)."""
    rng = np.random.default_rng(1000 * A_SEED[Nz] + Nz)
    X = rng.standard_normal((Nz, S)).astype(np.float32)
    if S == 300:
        labels = np.ones(S, int)
    else:   # the area scattered over the 700 spaxels
        labels = np.zeros(S, int)
        labels[np.sort(np.random.default_rng(7).choice(S, 300, replace=False))] = 1
    spx = np.flatnonzero(labels == 1)
    plant(X, spx[rng.choice(300, 6, replace=False)], rng, 1.25)
    return Case(f"A-Nz{Nz}-S{S}", X, (S // 25, 25), labels, [halfway(X, spx, 6)], inplace=True)


B_SHAPE = (37, 41)
B_RUNS = ((0, 57), (4, 60), (1, 700), (2, 500), (3, 200))


def field_B(seed=30):
    """The field of B and D: Nz = 33, 37 x 41 = 1517 spaxels.  The 57 spaxels of no area come first
    and the 60 of area 4 (no nuisance) behind them, so the first 64-spaxel wave of
    deflate_dot_rows_kernel holds no iterating spaxel; areas 1-3 (700, 500, 200 spaxels) are
    scattered behind.  Area 1: 3 sources, area 2: 8, area 3: one (exactly one nuisance)."""
    Nz, S = 33, B_SHAPE[0] * B_SHAPE[1]
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((Nz, S)).astype(np.float32)
    labels = scattered_labels(B_RUNS, S, seed + 1, keep=128)
    spx = [np.flatnonzero(labels == a) for a in (1, 2, 3, 4)]
    src1 = rng.choice(spx[0], 3 + 250, replace=False)
    plant(X, src1[:3], rng, 1.25, j0=8)
    # a faint share (0.8) of the strongest source's spectrum in 250 more spaxels of area 1: the
    # vector that removes the source moves their O2 by more than the noise spreads it, so the
    # background set changes by many entries at once
    g = (X[:, src1[2]].astype(np.float64) / np.sqrt(o2(X[:, src1[2]]))).astype(np.float32)
    X[:, src1[3:]] += np.float32(0.8) * g[:, None]
    plant(X, rng.choice(spx[1], 8, replace=False), rng, 1.25)
    plant(X, rng.choice(spx[2], 1, replace=False), rng, 1.25)
    # two spaxels of area 1 with the same spectrum, the third lowest O2 of the area
    order = np.argsort(o2(X[:, spx[0]]))
    X[:, spx[0][order[3]]] = X[:, spx[0][order[2]]]
    thr = [halfway(X, spx[0], 3), halfway(X, spx[1], 8), halfway(X, spx[2], 1),
           1.5 * float(o2(X[:, spx[3]]).max())]
    return X, labels, thr


def case_field():
    X, labels, thr = field_B()
    return Case("B", X, B_SHAPE, labels, thr)


D_POPS = (2, 50, 1e9)


def case_background(noise_pop):
    X, labels, thr = field_B()
    return Case(f"D-{noise_pop:g}", X, B_SHAPE, labels, thr, noise_pop=noise_pop)


C_GROUPS = ((30, 16.0), (50, 8.0), (15, 10.0), (30, 5.0))   # (spaxels, amplitude): removed in this order


def case_widths():
    """C: Nz = 40, one area of 40 x 50 = 2000 spaxels.  Four groups of nuisance spaxels share a
    spectrum each (amplitudes graded by 1 % per spaxel), so that one removed vector drops a whole
    group: n falls 135 -> 105 -> 55 -> 40 -> 10 and then one by one (ten independent sources)."""
    Nz, S = 40, 2000
    rng = np.random.default_rng(41)
    X = rng.standard_normal((Nz, S)).astype(np.float32)
    where = rng.choice(S, sum(c for c, _ in C_GROUPS) + 10, replace=False)
    k = 0
    for count, amp in C_GROUPS:
        g = rng.standard_normal(Nz).astype(np.float32)
        for i in range(count):
            X[:, where[k]] += np.float32(amp * (1 + 0.01 * i)) * g
            k += 1
    plant(X, where[k:][::-1], rng, 1.12)
    spx = np.arange(S)
    return Case("C", X, (40, 50), np.ones(S, int), [halfway(X, spx, len(where))])


def case_cap():
    """E: Nz = 96, S = 600: area 1 (480 spaxels) with 70 sources of amplitudes 5 * 1.02^j runs past
    PCA_CAP = 64 vectors; area 2 (120 spaxels) with 3 sources stops after 3 iterations.  The 70
    spectra are orthogonal to each other (columns of a random orthonormal basis, scaled to unit
    variance): random spectra of 96 channels overlap, each removed vector takes 1 / 96 of every
    other source with it, and all 70 are below the threshold after 48 iterations."""
    Nz, S = 96, 600
    rng = np.random.default_rng(72)
    X = rng.standard_normal((Nz, S)).astype(np.float32)
    labels = scattered_labels(((1, 480), (2, 120)), S, 73)
    spx = [np.flatnonzero(labels == a) for a in (1, 2)]
    Q, _ = np.linalg.qr(rng.standard_normal((Nz, 70)))
    for j, s in enumerate(rng.choice(spx[0], 70, replace=False)):
        X[:, s] += (5 * 1.02 ** j * np.sqrt(Nz) * Q[:, j]).astype(np.float32)
    plant(X, rng.choice(spx[1], 3, replace=False), rng, 1.25)
    thr = [halfway(X, spx[0], 70), halfway(X, spx[1], 3)]
    return Case("E", X, (24, 25), labels, thr, checkpoints=(0, 1, 2, 63, 64, 65, 66),
                gap_min=0.004)


F_SIZES = (1, 2, 1023, 1024, 1025, 12288, 12289)
F_SOURCES = (1, 1, 3, 3, 3, 3, 3)
F_SHAPE = (140, 200)


def case_selection(general):
    """F: Nz = 8, areas of 1, 2, 1023, 1024, 1025 and 12288 spaxels (the resident selection with
    1, 2 and 12 entries per thread); `general` adds one of 12289 (pca_select_kernel for all).  An
    all-zero spaxel (O2 == 0: the filtered-index quirk) in the middle of the 1025-spaxel area."""
    Nz, S = 8, F_SHAPE[0] * F_SHAPE[1]
    rng = np.random.default_rng(61)
    X = rng.standard_normal((Nz, S)).astype(np.float32)
    runs = [(a + 1, c) for a, c in enumerate(F_SIZES)]
    labels = scattered_labels(runs + [(0, S - sum(F_SIZES))], S, 62)
    thr = []
    for a, k in enumerate(F_SOURCES):
        spx = np.flatnonzero(labels == a + 1)
        if a == 4:
            X[:, spx[500]] = 0
        plant(X, rng.choice(np.delete(spx, 500) if a == 4 else spx, k, replace=False), rng, 1.6,
              a0=8.0)
        thr.append(halfway(X, spx, k) if len(spx) > k else 0.5 * float(o2(X[:, spx]).min()))
    if not general:
        labels = np.where(labels == 7, 0, labels)
        thr = thr[:6]
    return Case("F-general" if general else "F-resident", X, F_SHAPE, labels, thr)


CASE_IDS = ([f"A-Nz{Nz}-S{S}" for Nz in A_NZ for S in (300, 700)] + ["B", "C"] +
            [f"D-{p:g}" for p in D_POPS] + ["E", "F-resident", "F-general"])


@functools.lru_cache(maxsize=None)
def case(cid):
    if cid.startswith("A-"):
        nz, s = cid[4:].split("-S")
        return case_slices(int(nz), int(s))
    if cid.startswith("D-"):
        return case_background(float(cid[2:]))
    return {"B": case_field, "C": case_widths, "E": case_cap,
            "F-resident": lambda: case_selection(False),
            "F-general": lambda: case_selection(True)}[cid]()


# ------------------------------------------------------------------------------------ 1. restatement
# (case F's area of one spaxel is a nuisance without any background candidate: cpu_ref takes the
# mean of an empty slice, as the reference does, before it breaks at n == 1)
@pytest.mark.filterwarnings("ignore:Mean of empty slice", "ignore:invalid value encountered")
@pytest.mark.parametrize("cid", CASE_IDS)
def test_restatement_equals_the_oracle_at_every_checkpoint(cid):
    c = case(cid)
    for t in c.checkpoints:
        F, mapO2, nstop = cpu_ref.Compute_GreedyPCA_area(
            c.nb, c.X64.reshape((c.Nz,) + c.shape), c.areamap, c.noise_pop, c.thr, t, c.tests,
            svd="dense")
        r = orc.at(c.records, t)
        assert nstop == r.nstop, (cid, t)
        assert np.array_equal(mapO2.reshape(-1), r.mapO2), (cid, t)
        err = np.max(np.abs(F.reshape(c.Nz, -1) - r.F))
        assert err <= 1e-12 * np.max(np.abs(c.X64)), (cid, t, err)
    assert c.records[-1].nstop == 0


def test_restated_trace_lacks_the_single_nuisance_entry():
    """cpu_ref's trace holds the (1, nb) entry of an area's last iteration; the device's work list
    (areas with n >= 2) does not."""
    c = case("A-Nz33-S300")
    tr = []
    cpu_ref.Compute_GreedyPCA(c.X64, c.tests[0], c.thr[0], 50, 10 ** 6, svd="dense", trace=tr)
    assert tr[-1][0] == 1
    assert [(1, n) for n, _ in tr[:-1]] == orc.device_trace(c.records, 10 ** 6)
    assert [nb for _, nb in tr] == [r.steps[0].nb for r in c.records[:-1]]


# ------------------------------------------------------------------------------------ 3. conditions
@pytest.mark.parametrize("cid", CASE_IDS)
def test_inputs_are_decidable(cid):
    c = case(cid)
    steps = [s for r in c.records for s in r.steps if s is not None]
    assert min(s.thr_margin for s in steps) >= 1e-6
    assert min(s.bg_margin for s in steps) >= 1e-9
    gaps = [s.gap for s in steps if s.gap is not None]
    assert not gaps or min(gaps) >= c.gap_min, min(gaps)
    d = c.distance()
    print(f"{cid}: |F_svd - F_gram| = {d:.2e}, smallest gap "
          f"{min(gaps) if gaps else float('nan'):.4f}, iterations {c.last}")
    assert d < float(orc.ulp32(np.max(np.abs(c.X64))))
    # and the GPU test's bound covers it: the formulation the device follows (Gram) lies inside
    # the bound that the SVD restatement sets
    for t, (r, g) in enumerate(zip(c.records, c.records_gram)):
        E = c.bound(t)[1]
        assert np.all(np.abs(r.F - g.F) <= E[None, :] + 1e-13 * np.max(np.abs(c.X64))), (cid, t)


# ------------------------------------------------------------------------------------ 2. geometry
# What each case is aimed at, as a function of the CU count: asserted here for 256 CUs and by the
# GPU tests for the device at hand.  (The slice counts of the gather and of the deflation depend
# on the CU count; the table of case A is the one for 256.)
def aim_slices(cid, num_cu):
    c = case(cid)
    Nz, S = c.Nz, c.S
    gather, deflate, fblocks, padding = A_TARGETS[Nz]
    its, flushes = c.geometry(num_cu)
    assert len(its) >= min(3, Nz - 1) and len(flushes) == 1
    for g in its:
        if num_cu == 256:
            assert g["gather"] == gather and g["deflate"] == deflate, (S, g)
        assert g["gather"][1] % 16 == 0 and g["deflate"][0] <= min(32, Nz)
        assert g["rows"] == (S == 300)              # 2 * cb >= S: the rows kernel; else the lists kernel
    f = flushes[0]
    # (the area's 300 spaxels make nxb = 2 in both fields)
    assert (f["nxb"], f["nxb"] * f["nzb"], f["padding"]) == (2, fblocks, padding)
    assert f["last_rows"] == (Nz % 32 or 32)        # rows of Us beyond Nz
    assert [g["fbold"][0] for g in its] == [False] + [True] * (len(its) - 1)
    assert [g["svalid"][0] for g in its] == [False] + [True] * (len(its) - 1)
    assert its[0]["uw_empty_slices"] == (geo.UW_SLICES - Nz if Nz < geo.UW_SLICES else
                                         geo.UW_SLICES - geo.cdiv(Nz, geo.cdiv(Nz, 32)))


def aim_field(cid, num_cu):
    c = case(cid)
    assert c.sizes == [700, 500, 200, 60] and c.S - sum(c.sizes) == 57 and c.S % 64
    r0 = c.records[0]
    assert r0.steps[3] is None and c.records[-1].mapO2[c.spx[3]].max() == 0      # no nuisance
    assert r0.steps[2].n == 1 and c.records[1].steps[2] is None                    # exactly one
    assert np.array_equal(np.unique(c.records[-1].mapO2[c.spx[2]]), [0, 1])
    depth = [len(c.n_sequence(a)) for a in range(4)]
    assert 2 <= depth[0] < depth[1]                                                # the largest stops first
    its, flushes = c.geometry(num_cu)
    rows = [g["rows"] for g in its]
    assert rows[0] and not rows[-1] and rows == sorted(rows, reverse=True)
    # a 64-spaxel wave of the rows kernel without an iterating spaxel while that kernel runs
    iterating = np.zeros(c.S, bool)
    for a, _, _ in c.works()[0]:
        iterating[c.spx[a]] = True
    waves = np.add.reduceat(iterating, np.arange(0, c.S, 64))
    assert waves[0] == 0 and np.all(waves[1:] > 0)
    f, = flushes
    assert f["areas"] == [0, 1, 2, 3] and len(set(f["T"])) >= 3 and f["T"][2:] == [0, 0]
    assert len({c.sizes[a] for a in f["areas"]}) == 4


def aim_widths(cid, num_cu):
    c = case(cid)
    n = c.n_sequence(0)
    its, _ = c.geometry(num_cu)
    assert {144, 112, 64, 48, 16} <= {g["ldmax"] for g in its}, n

    def crosses(limit):
        return any(a > limit >= b for a, b in zip(n, n[1:]))
    assert crosses(64) and crosses(48) and crosses(96), n
    assert {g["all_small"] for g in its} == {False, True}
    assert {g["gather_colblocks"] for g in its} >= {1, 2, 3}
    assert {g["eig_launch"] for g in its} == {"plain", "mid", "small"}
    assert all(g["fbold"][0] for g in its[1:]) and not its[0]["fbold"][0]
    drops = [a - b for a, b in zip(n, n[1:])]          # one iteration drops a whole group
    assert sorted(drops, reverse=True)[:4] == sorted((cnt for cnt, _ in C_GROUPS), reverse=True)


def bg_changes(c):
    """(entered, left) of the background set between consecutive iterations, all areas."""
    d = []
    for a in range(c.nb):
        sets = [set(r.steps[a].bg.tolist()) for r in c.records
                if r.steps[a] is not None and r.steps[a].n >= 2]
        d += [(len(q - p), len(p - q)) for p, q in zip(sets, sets[1:])]
    return d


def aim_background(cid, num_cu):
    c = case(cid)
    nbs = [s.nb for r in c.records for s in r.steps if s is not None]
    assert geo.selection(c.sizes)[0]                  # the resident selection keeps dlist
    if c.noise_pop == 2:     # second trip of the 64-lane loops over nb and ndiff
        assert max(nbs) >= 65
        assert any(i + o >= 65 and i > 0 and o > 0 for i, o in bg_changes(c))
    elif c.noise_pop == 1e9:
        assert set(nbs) == {1} and (0, 0) in bg_changes(c)
    else:                    # two spaxels of equal O2 inside a background set, not at its boundary
        s = c.records[0].steps[0]
        pos = {int(sp): i for i, sp in enumerate(c.spx[0])}
        vals = np.sort([c.tests[0][pos[int(sp)]] for sp in s.bg])
        assert np.any(np.diff(vals) == 0) and vals[-1] != vals[-2] and s.bg_margin >= 1e-9


def aim_cap(cid, num_cu):
    c = case(cid)
    assert c.last >= geo.PCA_CAP + 2 and c.records[-1].T[1] == 3
    its, flushes = c.geometry(num_cu)
    assert [g["flushed_before"] for g in its].count(True) == 1 and its[64]["flushed_before"]
    assert its[63]["fbold"] == [True] and its[63]["svalid"] == [True]
    assert its[64]["fbold"] == [False] and its[64]["svalid"] == [False]
    assert its[65]["fbold"] == [True] and its[65]["svalid"] == [True]
    assert [f["final"] for f in flushes] == [False, True]
    assert flushes[0]["T"] == [64, 3] and flushes[1]["areas"] == [0]
    assert set(c.checkpoints) >= {0, 1, 2, 63, 64, 65, 66, c.last}


def aim_selection(cid, num_cu):
    c = case(cid)
    general = cid == "F-general"
    assert c.sizes == list(F_SIZES if general else F_SIZES[:6])
    resident, ept = geo.selection(c.sizes)
    assert resident != general and ept[:6] == [1, 1, 1, 1, 2, 12]
    assert not c.X[:, c.spx[4][500]].any() and c.tests[4][500] == 0
    # the quirk shows: the background columns of that area are not its nb lowest O2 values
    for rec in c.records:
        s = rec.steps[4]
        if s is not None:
            t = np.mean(rec.F[:, c.spx[4]] ** 2, axis=0)
            naive = c.spx[4][np.argsort(np.where(t > 0, t, np.inf))[:s.nb]]
            assert set(naive.tolist()) != set(s.bg.tolist())
    assert c.records[0].steps[0].n == 1 and c.records[0].steps[0].nb == 0
    assert max(len(c.n_sequence(a)) for a in range(c.nb)) >= 3
    assert all(max(c.n_sequence(a)) <= 3 for a in range(c.nb))


AIMS = {"A": aim_slices, "B": aim_field, "C": aim_widths, "D": aim_background, "E": aim_cap,
        "F": aim_selection}


def check_aim(cid, num_cu):
    AIMS[cid[0]](cid, num_cu)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_case_reaches_its_geometry_at_256_cus(cid):
    check_aim(cid, 256)
