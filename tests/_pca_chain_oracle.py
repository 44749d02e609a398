"""Test-side float64 restatement of the greedy PCA, one lock-step iteration at a time.

``cpu_ref.Compute_GreedyPCA`` (lib_origin.py:848-954) runs one area to its end and returns the last
cube only.  Here the same loop -- with the filtered-index quirk of :908-917 (the background columns
are indices into ``test[test > 0]`` used on the unfiltered cube) and the single-nuisance break of
:927 -- advances all areas of a field together, as csrc/pca.hip does, and hands out the state after
every iteration: record t is what ``Compute_GreedyPCA_area(..., itermax=t)`` returns (the cube after
t deflations, mapO2 with the (t+1)-th selection counted, nstop = the areas that selection stopped),
together with the selection made on that cube (the work of iteration t+1) and the margins that say
how far the input is from a decision flipping.

Two formulations of the removed vector: ``form="svd"`` takes u from the dense SVD of x_red (the
reference's call, LAPACK instead of ARPACK as cpu_ref's svd="dense"); ``form="gram"`` takes the
leading eigenvector v of the float64 Gram matrix Xp^T Xp (``eigh``) and u = Xp v / |Xp v|, the
device's formulation.  Their distance bounds what the choice of formulation can move.
"""
import numpy as np


class AreaStep:
    """The selection one area makes on the cube of a record, i.e. the work of the next iteration."""
    __slots__ = ("n", "nb", "T", "nuis", "bg", "gap", "thr_margin", "bg_margin", "u", "b")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


class Record:
    """State after t lock-step iterations.  F (Nz, S) float64; mapO2 (S,), nstop: as with
    itermax = t; steps[a]: AreaStep of area a's next iteration, None once the area has stopped
    (steps[a].n == 0 cannot occur: an area without nuisance stops and gets None)."""

    def __init__(self, t, F, mapO2, nstop, steps, T):
        self.t, self.F, self.mapO2, self.nstop, self.steps, self.T = t, F, mapO2, nstop, steps, T

    def work(self):
        """[(area, n, nb, T)] of the areas the device puts into iteration t+1's work list (n >= 2)."""
        return [(a, s.n, s.nb, s.T) for a, s in enumerate(self.steps) if s is not None and s.n >= 2]


def _select(F_a, test, thr, noise_pop):
    """lib :889 / :908-917 on one area: nuisance columns, background columns (with the quirk), nb and
    the two margins."""
    pypx = np.where(test > thr)[0]                                   # :889 / :949
    test_v = test[test > 0]                                          # :908-909
    nind = np.where(test_v <= thr)[0]
    vals = test_v[nind]
    sortind = np.argsort(vals, kind="stable")
    nb = 1 + int(len(nind) / noise_pop)                              # :914
    bgcols = nind[sortind[:nb]]                                      # :917 (indices of the FILTERED vector)
    s = vals[sortind]
    bg_margin = (s[nb] - s[nb - 1]) / s[nb - 1] if len(s) > nb else np.inf   # (nb >= 1)
    thr_margin = float(np.min(np.abs(test - thr)) / thr)
    return pypx, bgcols, min(nb, len(nind)), thr_margin, float(bg_margin)


def _vector(x_red, form):
    """Leading left singular vector of x_red and the relative gap (l1 - l2) / l1 of x_red^T x_red."""
    if form == "svd":
        U, s, _ = np.linalg.svd(x_red, full_matrices=False)          # :940
        u = U[:, 0]
        l1, l2 = s[0] ** 2, (s[1] ** 2 if len(s) > 1 else 0.0)
    else:
        w, V = np.linalg.eigh(x_red.T @ x_red)
        u = x_red @ V[:, -1]
        u = u / np.linalg.norm(u)
        l1, l2 = w[-1], (max(w[-2], 0.0) if len(w) > 1 else 0.0)
    return u, float((l1 - l2) / l1)


def chain(X, area_spx, thr, noise_pop, form="svd"):
    """Generator over Record t = 0, 1, ... until no area selects a nuisance any more.
    X: (Nz, S) float64 (cube_std, flattened); area_spx: flat spaxel indices per area in C order;
    thr: threshold per area.  The initial test is O2test(X) of each area."""
    X = np.asarray(X, dtype=np.float64)
    Nz, S = X.shape
    na = len(area_spx)
    F = X.copy()                                                     # :892
    faint = [X[:, s].copy() for s in area_spx]
    test = [np.mean(f ** 2, axis=0) for f in faint]
    mapO2 = np.zeros(S)
    active = [len(s) > 0 for s in area_spx]
    T = [0] * na
    t = 0
    while True:
        steps, plans = [None] * na, [None] * na
        map_t, nstop = mapO2.copy(), 0
        for a in range(na):
            if not active[a]:
                continue
            pypx, bgcols, nb, thr_m, bg_m = _select(faint[a], test[a], thr[a], noise_pop)
            if len(pypx) == 0:                                       # :899
                active[a] = False
                continue
            spx = np.asarray(area_spx[a])
            map_t[spx[pypx]] += 1                                    # :901 (before the itermax test)
            nstop += 1                                               # :902-905 with itermax = t
            # :917 (no candidate at all: the reference's mean of an empty slice, NaN)
            b = np.mean(faint[a][:, bgcols], axis=1) if len(bgcols) else np.full(Nz, np.nan)
            x_red = faint[a][:, pypx]                                # :920
            x_red = x_red - np.outer(b, b @ x_red)                   # :923 (a a^T b, no (a^T a)^-1)
            if form == "svd":
                x_red = x_red / np.nansum(b ** 2)                    # :924
            u, gap = (None, None) if len(pypx) == 1 else _vector(x_red, form)
            steps[a] = AreaStep(n=len(pypx), nb=nb, T=T[a], nuis=spx[pypx], bg=spx[bgcols],
                                gap=gap, thr_margin=thr_m, bg_margin=bg_m, u=u, b=b)
            plans[a] = pypx
        yield Record(t, F.copy(), map_t, nstop, steps, list(T))
        if nstop == 0:
            return
        mapO2 = map_t
        for a in range(na):
            s = steps[a]
            if s is None:
                continue
            if s.n == 1:                                             # :927
                active[a] = False
                continue
            faint[a] -= np.outer(s.u, s.u @ faint[a])                # :943
            test[a] = np.mean(faint[a] ** 2, axis=0)                 # :946
            F[:, area_spx[a]] = faint[a]
            T[a] += 1
        t += 1


def run(X, area_spx, thr, noise_pop, form="svd"):
    """All records of ``chain`` as a list: records[t] is the run with itermax = t; the last one is
    the unbounded run (nstop == 0)."""
    return list(chain(X, area_spx, thr, noise_pop, form))


def at(records, t):
    """The record a run with itermax = t ends in."""
    return records[min(t, len(records) - 1)]


def device_trace(records, t):
    """What build_work_list stores in h_trace during a run with itermax = t: per executed iteration
    (areas with n >= 2, the sum of their n).  An iteration whose areas all have n == 1 enqueues
    nothing and ends the device's loop (no area can iterate after it: areas only stop)."""
    out = []
    for r in records[:min(t, len(records) - 1)]:
        w = r.work()
        if not w:
            break
        out.append((len(w), sum(n for _, n, _, _ in w)))
    return out


def ulp32(x):
    """Spacing of float32 at |x| (array or scalar), as float64."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)
