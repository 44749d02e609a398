"""GPU tests of the greedy PCA's batched launches: what origin_pca_run does at every iteration --
one Gram launch over the tile lists of many matrices of different widths, one eigen-solver launch
whose kernel is chosen by the largest matrix while every block picks a solver by its own n --
given to the two unit-test entry points (origin_pca_gram, origin_pca_eig) as such batches, and
fields whose areas iterate out of step through origin_pca_run.

References: NumPy / LAPACK in float64 and oracle/cpu_ref.py.  Tolerances are those of the
single-matrix tests and of the header of test_hip_parity.py:
  Gram        : max|G - X^T X| <= 1e-12 max|X^T X| per matrix
  eigenpair   : |theta - w| <= 1e-12 w, | |v| - 1 | < 1e-12, |A v - w v| <= 1e-11 w,
                1 - |v . v_lapack| <= 1e-10 / max(gap, 1e-12)^2 + 1e-13, v[n:ld] == 0
  cube_faint  : mapO2 and nstop identical, max-abs <= 1e-4, rel-Frobenius <= 2e-6
"""
import numpy as np
import pytest

from _gram_geometry import gram_geometry, num_cu_of
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

# constants of csrc/pca_eig.h / pca_eig.hip / pca.hip that the cases are built around
LANCZOS_M, PW_N, LP_NMAX = 48, 96, 512
PCA_CAP = 64           # removed vectors kept per area before the cube is flushed
SENTINEL = -7.25e250   # fills the buffers a kernel must not write outside its matrices


@pytest.fixture(scope="module")
def hip():
    import origin_amd.lib_origin as lib
    return lib


@pytest.fixture(scope="module")
def ctx():
    from origin_amd.device import default_context
    return default_context(0)


def ld_of(n):
    return (n + 15) // 16 * 16


# ------------------------------------------------------------------------------- Gram batches
def gram_batch(widths, Nz, seed, slack=304):
    """Inputs of origin_pca_gram for matrices of n columns each (ld = n rounded up to 16): the
    concatenated [Nz][ld] blocks with columns n..ld zero (as the driver's gather leaves them) and
    uneven column scales (a transposed tile shows), xp_off, g_off = running sum of ld^2 with
    `slack` doubles in front of, between and behind the matrices, and the upper-triangle 32 x 32
    tile list over all matrices."""
    rng = np.random.default_rng(seed)
    X, xp_off, g_off, ti, tj, ta = [], [], [], [], [], []
    xp, g = 0, slack
    for a, n in enumerate(widths):
        ld = ld_of(n)
        x = np.zeros((Nz, ld))
        x[:, :n] = rng.standard_normal((Nz, n)) * (1 + (np.arange(n) * 7 + a) % 23)[None, :]
        X.append(x)
        xp_off.append(xp)
        g_off.append(g)
        xp += Nz * ld
        g += ld * ld + slack
        iu, ju = np.triu_indices((ld + 31) // 32)
        ti.append(iu), tj.append(ju), ta.append(np.full(len(iu), a))
    return dict(Nz=Nz, widths=list(widths), X=X, ld=[ld_of(n) for n in widths],
                xp_off=np.array(xp_off, np.int64), g_off=np.array(g_off, np.int64), g_total=g,
                tiles=np.stack([np.concatenate(ti), np.concatenate(tj),
                                np.concatenate(ta)]).astype(np.int32))


def run_gram(ctx, b, order=None):
    """One origin_pca_gram call over the whole batch; returns the host copy of d_G (sentinel
    filled before the call)."""
    from origin_amd import _capi
    tiles = b["tiles"] if order is None else b["tiles"][:, order]
    dX = ctx.to_device(np.concatenate([x.ravel() for x in b["X"]]))
    d_xo, d_go = ctx.to_device(b["xp_off"]), ctx.to_device(b["g_off"])
    d_ld = ctx.to_device(np.array(b["ld"], np.int64))
    d_t = [ctx.to_device(np.ascontiguousarray(t)) for t in tiles]
    G = ctx.to_device(np.full(b["g_total"], SENTINEL))
    _capi.call("origin_pca_gram", ctx.handle, dX.p, d_xo.p, d_ld.p, b["Nz"], tiles.shape[1],
               d_t[0].p, d_t[1].p, d_t[2].p, b["g_total"], G.p, d_go.p)
    return G.to_host()


def check_gram(b, got):
    """Every G_a against X_a^T X_a; exact symmetry; pad rows / columns exactly zero; the slack
    around the matrices still holds the sentinel."""
    untouched = np.ones(b["g_total"], bool)
    for a, (n, ld, x, off) in enumerate(zip(b["widths"], b["ld"], b["X"], b["g_off"])):
        G = got[off:off + ld * ld].reshape(ld, ld)
        untouched[off:off + ld * ld] = False
        ref = x.T @ x
        err, scale = np.max(np.abs(G - ref)), np.max(np.abs(ref))
        assert err <= 1e-12 * scale, (a, n, err / scale)
        assert np.array_equal(G, G.T), (a, n)
        assert np.all(G[n:, :] == 0) and np.all(G[:, n:] == 0), (a, n)
    assert np.all(got[untouched] == SENTINEL)


MIXED_WIDTHS = (1, 15, 16, 17, 33, 77, 130)
KSPLIT_WIDTHS = (5, 40, 70)
# 1153 = 18 * 64 + 1: ksplit = 18 slabs of 68 channels, the last one starts at 1156 >= Nz
KSPLIT_NZ = (3, 31, 63, 64, 127, 128, 130, 257, 1153)


def test_gram_batch_of_mixed_widths(ctx):
    """gram_kernel / gram_reduce_kernel over one tile list of seven matrices, ld = 16, 32, 48, 80
    and 144: tiles that are clamped to half their width (ld no multiple of 32), per-matrix
    xp_off / g_off / ld looked up through tile_a.  Nz = 517: eight K-split slabs of 68 channels
    (two 32-channel trips and one that ends after 4) on the 256-CU device, the last one short."""
    b = gram_batch(MIXED_WIDTHS, 517, seed=21)
    assert sorted(set(b["ld"])) == [16, 32, 48, 80, 144]
    check_gram(b, run_gram(ctx, b))


def test_gram_ksplit_geometries_include_an_empty_slab():
    """The Nz of test_gram_batch_ksplit_geometry on the 256-CU device, from gram_launch's formula:
    ksplit 1 (Nz < 64 and Nz < 128), 2 and 4 with a slab depth that is no multiple of 32 and a short
    last slab, and 18 slabs of which the last is empty (z0 >= Nz)."""
    ntiles = gram_batch(KSPLIT_WIDTHS, 3, seed=0)["tiles"].shape[1]
    geo = {Nz: gram_geometry(256, ntiles, Nz) for Nz in KSPLIT_NZ}
    assert [geo[Nz][0] for Nz in KSPLIT_NZ] == [1, 1, 1, 1, 1, 2, 2, 4, 18]
    assert any((ks - 1) * zper >= Nz for Nz, (ks, zper) in geo.items())          # an empty slab
    assert any(zper % 32 and ks > 1 for ks, zper in geo.values())                # ends mid-trip
    assert any(0 < Nz - (ks - 1) * zper < zper for Nz, (ks, zper) in geo.items() if ks > 1)


@pytest.mark.parametrize("Nz", KSPLIT_NZ)
def test_gram_batch_ksplit_geometry(ctx, Nz):
    """gram_launch's ksplit (from num_cu, ntiles and Nz / 64) and gram_kernel's slab depth (rounded
    to 4, walked 32 channels per trip) on a batch of three matrices: Nz below one trip, below 64
    (ksplit = 1), slabs that end in mid-trip, a short last slab and (Nz = 1153) an empty one."""
    b = gram_batch(KSPLIT_WIDTHS, Nz, seed=30 + Nz)
    check_gram(b, run_gram(ctx, b))


def test_gram_batch_with_more_tiles_than_slots(ctx):
    """gram_launch with ntiles >= 8 * num_cu: ksplit falls to 1 although Nz / 64 = 3 would allow
    three slabs (matrices of n = 200, 28 tiles each, as many as it takes on this device)."""
    num_cu = num_cu_of(ctx)
    nmat = (8 * num_cu + 27) // 28
    b = gram_batch((200,) * nmat, 192, seed=40)
    assert b["tiles"].shape[1] >= 8 * num_cu
    assert gram_geometry(num_cu, b["tiles"].shape[1], 192)[0] == 1
    check_gram(b, run_gram(ctx, b))


def test_gram_batch_is_independent_of_the_tile_order(ctx):
    """gram_kernel / gram_reduce_kernel with the tile list shuffled, tile_a not grouped by matrix:
    bit for bit the unshuffled result (the slabs are summed in fixed order), slack included."""
    b = gram_batch(MIXED_WIDTHS, 517, seed=21)
    order = np.random.default_rng(5).permutation(b["tiles"].shape[1])
    assert np.any(np.diff(b["tiles"][2][order]) < 0)          # not grouped by matrix
    want = run_gram(ctx, b)
    got = run_gram(ctx, b, order)
    check_gram(b, got)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------- eigen-solver batches
def psd_matrix(n, kind, seed):
    """Symmetric PSD matrix with the spectra of test_lanczos_leading_eigenvector: a wide gap, two
    close leading values, a flat spectrum, rank 2; `zero` is the all-zero matrix."""
    if kind == "zero":
        return np.zeros((n, n))
    rng = np.random.default_rng(seed)
    Qm, _ = np.linalg.qr(rng.standard_normal((n, n)))
    if kind == "gap":
        lam = np.concatenate([[1000.0], rng.uniform(0.1, 10, n - 1)])
    elif kind == "close":
        lam = np.concatenate([[1.0, 0.999], rng.uniform(0.0, 0.9, n - 2)])
    elif kind == "lowrank":
        lam = np.concatenate([[1000.0, 3.0], np.zeros(n - 2)])
    else:
        lam = 1.0 + 0.05 * rng.random(n)
    assert len(lam) == n
    A = (Qm * np.sort(lam)[::-1]) @ Qm.T
    return 0.5 * (A + A.T)


_matrices = {}


def matrix(n, kind):
    key = (n, kind)
    if key not in _matrices:
        A = psd_matrix(n, kind, 100 + n)   # (the single-matrix test's seeds)
        _matrices[key] = (A,) + tuple(np.linalg.eigh(A))
    return _matrices[key]


def run_eig(ctx, specs, lead=176, slack=208, vslack=16):
    """One origin_pca_eig call over the matrices (n, kind) of `specs`, packed into one d_G at
    g_off = `lead` + running sum of (ld^2 + `slack`), q_off = running sum of qrows * ld, v_off =
    running sum of (ld + `vslack`); d_v is sentinel filled.  Returns [(v[ld], info[3])] per matrix
    after checking that nothing but the vectors was written to d_v."""
    from origin_amd import _capi
    rows = _capi.load().origin_pca_eig_qrows()
    ns = [n for n, _ in specs]
    lds = [ld_of(n) for n in ns]
    g_off = lead + np.concatenate([[0], np.cumsum([ld * ld + slack for ld in lds])])
    q_off = np.concatenate([[0], np.cumsum([rows * ld for ld in lds])])
    v_off = vslack + np.concatenate([[0], np.cumsum([ld + vslack for ld in lds])])
    G = np.full(g_off[-1], np.nan)     # whatever a solver reads outside its matrix poisons it
    for (n, kind), ld, off in zip(specs, lds, g_off):
        g = np.zeros((ld, ld))
        g[:n, :n] = matrix(n, kind)[0]
        G[off:off + ld * ld] = g.ravel()
    as_dev = lambda x: ctx.to_device(np.asarray(x, np.int64))
    dG, d_go, d_ld, d_n = ctx.to_device(G), as_dev(g_off[:-1]), as_dev(lds), as_dev(ns)
    d_qo, d_vo = as_dev(q_off[:-1]), as_dev(v_off[:-1])
    v = ctx.to_device(np.full(v_off[-1], SENTINEL))
    info = ctx.to_device(np.full(3 * len(specs), SENTINEL))
    _capi.call("origin_pca_eig", ctx.handle, dG.p, d_go.p, d_ld.p, d_n.p, len(specs),
               int(q_off[-1]), d_qo.p, v.p, d_vo.p, info.p)
    hv, hinfo = v.to_host(), info.to_host().reshape(-1, 3)
    out, untouched = [], np.ones(len(hv), bool)
    for ld, off, i3 in zip(lds, v_off, hinfo):
        out.append((hv[off:off + ld].copy(), i3))
        untouched[off:off + ld] = False
    assert np.all(hv[untouched] == SENTINEL)
    return out


def check_pair(spec, v, info):
    """What test_lanczos_leading_eigenvector checks, for one matrix of a batch."""
    n, kind = spec
    A, w, V = matrix(n, kind)
    theta, resid, restarts = info
    assert np.all(np.isfinite(v)) and np.all(np.isfinite(info)), spec
    assert np.all(v[n:] == 0), spec
    got = v[:n]
    assert abs(np.linalg.norm(got) - 1) < 1e-12, spec
    if kind == "zero":   # tridiag_top_lean's convention for T == 0: eigenvalue 0, a unit vector
        assert theta == 0.0, spec
        return
    assert abs(theta - w[-1]) <= 1e-12 * w[-1], (spec, theta, w[-1])
    r = np.linalg.norm(A @ got - w[-1] * got)
    assert r <= 1e-11 * w[-1], (spec, r, resid, restarts)
    gap = (w[-1] - w[-2]) / w[-1] if n > 1 else 1.0
    assert 1 - abs(got @ V[:, -1]) <= 1e-10 / max(gap, 1e-12) ** 2 + 1e-13, spec


_alone = {}


def solved_alone(ctx, spec):
    if spec not in _alone:
        _alone[spec] = run_eig(ctx, [spec])[0]
        check_pair(spec, *_alone[spec])
    return _alone[spec]


def check_batch(ctx, specs):
    """Every matrix of the batch against LAPACK, and against the same matrix solved in a call of
    its own (a different launch-level kernel for most: compared with the tolerances, not bit for
    bit -- eig_mid_power sums its trace over NW waves, 16 or 8 by the calling kernel)."""
    res = run_eig(ctx, specs)
    for spec, (v, info) in zip(specs, res):
        check_pair(spec, v, info)
        n, kind = spec
        if kind == "zero":
            continue
        va, ia = solved_alone(ctx, spec)
        w = matrix(n, kind)[1]
        gap = (w[-1] - w[-2]) / w[-1] if n > 1 else 1.0
        assert abs(info[0] - ia[0]) <= 1e-12 * w[-1], spec
        assert 1 - abs(v[:n] @ va[:n]) <= 1e-10 / max(gap, 1e-12) ** 2 + 1e-13, spec
    return res


SMALL_BATCH = [(1, "flat"), (2, "gap"), (16, "close"), (17, "lowrank"), (33, "gap"), (48, "close")]
MID_BATCH = [(1, "gap"), (20, "lowrank"), (48, "close"), (49, "gap"), (64, "close"), (96, "flat")]
PLAIN_BATCH = [(1, "flat"), (20, "close"), (48, "gap"), (49, "lowrank"), (96, "close"), (97, "gap"),
               (208, "flat"), (209, "close"), (256, "lowrank"), (257, "gap"), (300, "close")]
ROUND2_BATCH = [(513, "gap"), (1, "flat"), (20, "lowrank"), (49, "close"), (96, "gap"),
                (130, "close")]


def test_eig_batch_small_launch(ctx):
    """ldmax <= LANCZOS_M: eig_power_kernel with dynamic LDS = SmallWork only; every block in
    eig_small_power<16> with one, two and three tile rows."""
    assert max(ld_of(n) for n, _ in SMALL_BATCH) <= LANCZOS_M
    check_batch(ctx, SMALL_BATCH)


def test_eig_batch_mid_launch(ctx):
    """LANCZOS_M < ldmax <= PW_N: eig_power_kernel with dynamic LDS = PW_BYTES; blocks with
    n <= LANCZOS_M overlay SmallWork on it (eig_small_power<16>), the others run
    eig_mid_power<16>."""
    assert LANCZOS_M < max(ld_of(n) for n, _ in MID_BATCH) <= PW_N
    check_batch(ctx, MID_BATCH)


@pytest.mark.parametrize("reverse", [False, True])
def test_eig_batch_plain_launch(ctx, reverse):
    """PW_N < ldmax <= LP_NMAX: lanczos_plain_kernel, 512 threads; per block eig_small_power<8>
    (n <= LANCZOS_M), eig_mid_power<8> (n <= PW_N), lanczos_plain<1> with the matrix resident
    (n <= 208) or partly streamed (n <= 256) and lanczos_plain<2> above, all on one PlainLds-sized
    dynamic LDS block.  Reversed: block index and LDS reuse pair differently."""
    assert PW_N < max(ld_of(n) for n, _ in PLAIN_BATCH) <= LP_NMAX
    check_batch(ctx, PLAIN_BATCH[::-1] if reverse else PLAIN_BATCH)


def test_eig_batch_round2_launch(ctx):
    """ldmax > LP_NMAX: lanczos_kernel (basis in the global scratch at q_off, dynamic LDS =
    PW_BYTES): the 513-column matrix and a 130-column one in the restarted Lanczos with the basis
    at their own q_off, the small ones in eig_small_power<16> / eig_mid_power<16> next to them."""
    assert max(ld_of(n) for n, _ in ROUND2_BATCH) > LP_NMAX
    check_batch(ctx, ROUND2_BATCH)


def test_eig_batch_same_matrix_at_both_ends(ctx):
    """lanczos_plain_kernel over eight matrices, the first and the last the same (n = 150, two
    close leading values): same code, same data, only g_off / q_off / v_off and the block index
    differ -- vector and (theta, residual, restarts) equal bit for bit."""
    specs = [(150, "close"), (20, "gap"), (64, "close"), (97, "lowrank"), (209, "gap"),
             (48, "flat"), (300, "close"), (150, "close")]
    res = check_batch(ctx, specs)
    assert np.array_equal(res[0][0], res[-1][0])
    assert np.array_equal(res[0][1], res[-1][1])


@pytest.mark.parametrize("launch", ["plain", "round2"])
def test_eig_batch_with_all_zero_matrices(ctx, launch):
    """An all-zero matrix in every per-matrix branch next to ordinary ones: eig_small_power and
    eig_mid_power (trace 0: first unit vector), lanczos_plain (breakdown at the first step,
    tridiag_top_lean's T == 0) in lanczos_plain_kernel; the two power solvers and the restarted
    Lanczos (the same T == 0 branch) in lanczos_kernel.  Every loop of the three solvers is
    bounded whatever the data (fixed squaring count of 64, restart caps of 60 / 8, mmax steps), so
    the case can only fail, not hang.  Zero matrices come back finite with theta == 0 and a unit
    vector; their neighbours meet the usual tolerances."""
    if launch == "plain":
        specs = [(150, "gap"), (20, "zero"), (64, "zero"), (150, "zero"), (300, "zero"),
                 (48, "close"), (97, "lowrank"), (300, "close")]
    else:
        specs = [(513, "gap"), (130, "zero"), (20, "zero"), (64, "zero"), (49, "close"),
                 (96, "lowrank")]
    check_batch(ctx, specs)


# ------------------------------------------------------------------------------- areas out of step
def irregular_areamap(Ny, Nx, sizes, seed):
    """Labels 1..len(sizes) with exactly sizes[a] spaxels each: runs in raster order below a first
    row of label 0 (they end in mid-row), then a tenth of the spaxels swapped at random, so that
    no area is a rectangle or contiguous.  What is left over is label 0."""
    rng = np.random.default_rng(seed)
    lab = np.zeros(Ny * Nx, int)
    run = np.concatenate([np.full(s, a + 1) for a, s in enumerate(sizes)])
    assert Nx + len(run) <= Ny * Nx
    lab[Nx:Nx + len(run)] = run
    pick = Nx + rng.choice(len(run), len(run) // 10, replace=False)
    lab[pick] = lab[rng.permutation(pick)]
    amap = lab.reshape(Ny, Nx)
    assert np.all(amap[0] == 0)
    assert [int((amap == a + 1).sum()) for a in range(len(sizes))] == list(sizes)
    return amap


def plant(cube, areamap, area, count, rng, shared=None, avoid=()):
    """`count` strong spaxels in `area`, amplitudes graded 6.0 + 0.05 j as in
    test_pca_more_iterations_than_vector_slots: independent spectra, or all of them the spectrum
    `shared`, so that a single removed vector clears them all.  `avoid`: flat indices to leave."""
    Nz = cube.shape[0]
    flat = cube.reshape(Nz, -1)
    spx = np.setdiff1d(np.nonzero(areamap.reshape(-1) == area)[0], avoid)
    for j, s in enumerate(rng.choice(spx, count, replace=False)):
        src = rng.standard_normal(Nz).astype(np.float32) if shared is None else shared
        flat[:, s] += np.float32(6.0 + 0.05 * j) * src


def thresholds_for(cube, areamap, counts):
    """Per area: O2 of cube_std and the threshold half-way between the counts[a]-th and the next
    largest O2 value: exactly counts[a] nuisance spaxels at the first iteration."""
    tests, thr = [], []
    for a, k in enumerate(counts):
        t = cpu_ref.O2test(cube[:, areamap == a + 1])
        s = np.sort(t)[::-1]
        tests.append(t)
        thr.append(float(0.5 * (s[k - 1] + s[k])))
    return tests, thr


class OutOfStepCase:
    """A field, its thresholds, and the float64 oracle's run of it (cube_faint, mapO2, nstop)."""

    def __init__(self, cube, areamap, counts, itermax=300):
        self.cube = cube.astype(np.float32).astype(float)    # what the device holds, exactly
        self.areamap, self.nb, self.itermax = areamap, len(counts), itermax
        self.tests, self.thr = thresholds_for(self.cube, areamap, counts)
        self.ref = cpu_ref.Compute_GreedyPCA_area(self.nb, self.cube, areamap, 50, self.thr,
                                                  itermax, self.tests, svd="dense")

    def trace(self):
        """Per area, the nuisance count of every iteration."""
        out = []
        for a in range(self.nb):
            tr = []
            cpu_ref.Compute_GreedyPCA(self.cube[:, self.areamap == a + 1], self.tests[a],
                                      self.thr[a], 50, self.itermax, svd="dense", trace=tr)
            out.append([n for n, _ in tr])
        return out

    def first_counts(self):
        return [int((t > thr).sum()) for t, thr in zip(self.tests, self.thr)]

    def depth(self):
        """Per area, the iterations it took (the largest mapO2 value)."""
        return [int(self.ref[1][self.areamap == a + 1].max()) for a in range(self.nb)]

    def assert_decidable(self):
        """A condition on the inputs, not a tolerance on the kernels: at the start and at the end
        of the oracle's run no O2 value lies within relative 1e-5 of its area's threshold, and no
        two O2 values of an area tie (the background selection sorts them)."""
        for a in range(self.nb):
            sel = self.areamap == a + 1
            assert len(np.unique(self.tests[a])) == len(self.tests[a]), a
            for o2 in (self.tests[a], cpu_ref.O2test(self.ref[0][:, sel])):
                assert np.min(np.abs(o2 / self.thr[a] - 1)) > 1e-5, a

    def check(self, hip):
        """The project's criteria for cube_faint (header of test_hip_parity.py)."""
        faint, mapO2, nstop = hip.Compute_GreedyPCA_area(self.nb, self.cube, self.areamap, 50,
                                                         self.thr, self.itermax, self.tests)
        ref = self.ref
        assert nstop == ref[2]
        assert np.array_equal(mapO2, ref[1])
        assert np.max(np.abs(faint - ref[0])) <= 1e-4
        assert np.linalg.norm(faint - ref[0]) <= 2e-6 * np.linalg.norm(ref[0])
        out = self.areamap == 0
        assert out.any() and np.array_equal(faint[:, out], self.cube[:, out])


def mixed_sizes_case():
    """Nz = 128, five areas of 40 to 1600 spaxels on an irregular label map with 4 to 260 planted
    strong spaxels; thresholds that make 6, 60, 130, 230 and 300 spaxels nuisances at first."""
    rng = np.random.default_rng(61)
    Nz, Ny, Nx = 128, 50, 64
    sizes, planted = (40, 150, 400, 900, 1600), (4, 30, 70, 150, 260)
    areamap = irregular_areamap(Ny, Nx, sizes, seed=62)
    cube = rng.standard_normal((Nz, Ny, Nx)).astype(np.float32)
    for a, k in enumerate(planted):
        plant(cube, areamap, a + 1, k, rng)
    return OutOfStepCase(cube, areamap, (6, 60, 130, 230, 300))


def all_small_case(twin):
    """Nz = 200, four areas of 120 to 330 spaxels with at most 47 nuisance spaxels at first; in
    the twin the last area starts at 60."""
    rng = np.random.default_rng(71)
    Nz, Ny, Nx = 200, 31, 32
    sizes = (120, 200, 260, 330)
    areamap = irregular_areamap(Ny, Nx, sizes, seed=72)
    cube = rng.standard_normal((Nz, Ny, Nx)).astype(np.float32)
    for a, k in enumerate((3, 10, 20)):
        plant(cube, areamap, a + 1, k, rng)
    if not twin:
        plant(cube, areamap, 4, 35, rng)
        return OutOfStepCase(cube, areamap, (5, 14, 30, 47))
    # the twin's last area: two groups of spaxels that share a spectrum each -- the first removed
    # vectors clear a group at a time, and the count falls below 48 while three areas still iterate
    plant(cube, areamap, 4, 24, rng)
    for _ in range(2):
        plant(cube, areamap, 4, 16, rng, shared=rng.standard_normal(Nz).astype(np.float32))
    return OutOfStepCase(cube, areamap, (5, 14, 30, 60))


def uneven_depth_case():
    """The `deep` field of test_pca_into_a_box_of_a_larger_cube (one area that needs more than 64
    iterations) with six more rows: a second area with two nuisance spaxels that one removed
    vector clears.  (The reference projects on the background mean b without normalising it,
    (1 - b b^T) x, which stretches x along b by 1 - |b|^2, about -60 here: the first vector an
    area removes is close to b.  The two spaxels therefore carry b's direction itself.)"""
    rng = np.random.default_rng(78)
    Nz, Ny, Nx = 240, 20, 25
    cube = rng.standard_normal((Nz, Ny, Nx)).astype(np.float32)
    flat = cube.reshape(Nz, -1)
    for j in range(80):
        flat[:, 5 * j + 3] += (6.0 + 0.05 * j) * rng.standard_normal(Nz).astype(np.float32)
    rng2 = np.random.default_rng(79)
    early = rng2.standard_normal((Nz, 6 * Nx)).astype(np.float32)
    cube = np.concatenate([cube, early.reshape(Nz, 6, Nx)], axis=1)
    areamap = np.ones((Ny + 6, Nx), int)
    areamap[0, :] = 0
    areamap[Ny:, :] = 2
    # b of the early area's first iteration: the mean of its 1 + int(148 / 50) = 3 lowest-O2 spaxels
    lowest = np.argsort(cpu_ref.O2test(early.astype(float)))[:3]
    b = early[:, lowest].astype(float).mean(axis=1)
    shared = (b / np.linalg.norm(b) * np.sqrt(Nz)).astype(np.float32)
    plant(cube, areamap, 2, 2, rng2, shared=shared, avoid=Ny * Nx + lowest)
    # (79 of the 475 O2 values lie above the 83.5th percentile that test takes as threshold)
    return OutOfStepCase(cube, areamap, (79, 2))


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            made[name] = dict(mixed=mixed_sizes_case, small=lambda: all_small_case(False),
                              twin=lambda: all_small_case(True), uneven=uneven_depth_case)[name]()
        return made[name]
    return get


def solver_class(n):
    return int(np.searchsorted([LANCZOS_M, PW_N, 208, 256], n, side="left"))


def test_pca_areas_of_mixed_batch_sizes(hip, cases):
    """origin_pca_run with five areas of 40 to 1600 spaxels whose first-iteration nuisance counts
    (6, 60, 130, 230, 300) fall one in each per-matrix solver class -- eig_small_power
    (<= LANCZOS_M), eig_mid_power (<= PW_N), lanczos_plain<1> resident (<= 208) and streamed
    (<= 256), lanczos_plain<2> -- inside one lanczos_plain_kernel launch, and that finish at
    different iterations: the work list shrinks area by area, the launch-level kernel changes as
    the largest area shrinks and leaves, and the three deepest areas cross the PCA_CAP flush."""
    c = cases("mixed")
    assert c.first_counts() == [6, 60, 130, 230, 300]
    assert [solver_class(n) for n in c.first_counts()] == [0, 1, 2, 3, 4]
    depth = c.depth()
    assert len(set(depth)) == len(depth), depth       # the areas drop out one by one
    assert max(depth) > PCA_CAP
    c.assert_decidable()
    c.check(hip)


@pytest.mark.parametrize("twin", [False, True])
def test_pca_all_small_switch(hip, cases, twin):
    """The all_small path of enqueue_chain (w.ldmax <= LANCZOS_M: gram_reduce_kernel skipped,
    eig_power_kernel sums the K-split slabs itself) at Nz = 200, ksplit = 3: four areas that
    never have more than 48 nuisance spaxels, so every iteration takes it; and (twin) one area
    that starts at 60 and falls to 48 or below after a few iterations, so the run starts on the
    reduced-Gram path (eig_power_kernel on G) and changes to the slab path while three
    areas still iterate."""
    c = cases("twin" if twin else "small")
    ntiles = sum(len(np.triu_indices((ld_of(n) + 31) // 32)[0]) for n in c.first_counts())
    assert gram_geometry(256, ntiles, 200)[0] == 3    # the fused slab sum is live
    trace = c.trace()
    # per iteration: does the largest nuisance count among the areas that still iterate (it picks
    # the path of that iteration) fit the small solver
    its = max(len(t) for t in trace)
    small = [max(t[k] for t in trace if len(t) > k) <= LANCZOS_M for k in range(its)]
    if twin:
        assert c.first_counts() == [5, 14, 30, 60]
        k = small.index(True)
        assert 2 <= k <= 8 and all(small[k:]) and not any(small[:k]), small
        assert sum(len(t) > k + 2 for t in trace) >= 3          # not alone when it switches
        assert all(max(t) <= LANCZOS_M for t in trace[:3])
    else:
        assert c.first_counts() == [5, 14, 30, 47]
        assert its > 30 and all(small)
    c.assert_decidable()
    c.check(hip)


def test_pca_uneven_depth_across_a_flush(hip, cases):
    """origin_pca_run's mid-run flush (F = X - U C once an area holds PCA_CAP = 64 vectors) with
    an area that finished after its first iteration next to the one that forces the flush: the
    early area's columns are written by a flush it takes no further part in."""
    c = cases("uneven")
    depth = c.depth()
    assert depth[1] == 1 and depth[0] > PCA_CAP, depth
    assert c.first_counts()[1] == 2
    c.assert_decidable()
    c.check(hip)
