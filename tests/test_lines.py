"""Line estimation (origin_amd/lines.py, csrc/lines.hip) against tests/_line_oracle.py, the NumPy
float64 restatement of the reference's estimation_line that tools/gen_line_golden.py pins to the
reference itself (tests/golden/g11_lines.npz).

Tolerances.  The fixture records, per case, the distance between the reference (ARPACK) and the
restatement (LAPACK): the spread between two correct float64 solvers on this problem.
  CPU: restatement vs fixture, continuous outputs to 100 x that distance, y / x / z equal.
  GPU: |d| <= TOL max|oracle| over a detection's array for line, var, flux, residual, with
       TOL = 1000 x the largest recorded distance (the device adds a squared condition number
       through the Gram form and another summation order), never above 1e-9; y / x / z equal.
Inputs are float32-representable and the oracle gets the same rounded values.  Every field has a
continuum source under each detection; before discrete outputs are compared the oracle's own
decision margins are asserted (singular values separated 3x, peakdet neighbour differences and
grid criterion gaps above 1e-6 relative).
"""
import os

import numpy as np
import pytest

import _line_oracle as oracle
from _gram_geometry import gram_geometry, num_cu_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_lines.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def golden_case(g, i):
    k = f"c{i}_"
    weights = [w.astype(float) for w in g[k + "weights"]] if k + "weights" in g.files else None
    psf = g[k + "psf"].astype(float)
    sg, mse, order, hp, hz = (int(v) for v in g[k + "params"])
    return dict(raw=g[k + "raw"].astype(float), var=g[k + "var"].astype(float),
                psf=list(psf) if weights is not None else psf, weights=weights,
                det=tuple(int(v) for v in g[k + "det"]), size_grid=sg,
                criteria="mse" if mse else "flux", order_dct=None if order < 0 else order,
                horiz_psf=hp, horiz=hz, line=g[k + "line"], lvar=g[k + "lvar"],
                scalars=g[k + "scalars"], yxz=g[k + "yxz"], dist=g[k + "dist"])


def device_tol(g):
    dist = max(float(g[f"c{i}_dist"].max()) for i in range(int(g["ncases"])))
    assert dist > 0
    return min(1000 * dist, 1e-9)


# ------------------------------------------------------------------------------------ not gpu
def test_restatement_against_the_reference_fixture(golden):
    """tests/_line_oracle.py on the fixture's inputs against the outputs the reference's own
    GridAnalysis gave: line, var, flux, residual to 100 x the recorded ARPACK / LAPACK distance,
    positions equal.  The cases: size_grid 0 and 1, a source one pixel off, z0 = 3 and Nz - 2,
    order_dct None / 10 / 30, two weighted fields, criteria 'mse' at x0 = 0."""
    n = int(golden["ncases"])
    assert n >= 5
    for i in range(n):
        c = golden_case(golden, i)
        z0, y0, x0 = c["det"]
        flux, mse, line, lvar, y, x, z, fb = oracle.grid_analysis(
            c["raw"], c["var"], c["psf"], c["weights"], y0, x0, z0, c["size_grid"], c["criteria"],
            c["order_dct"], c["horiz_psf"], c["horiz"])
        assert not fb and (y, x, z) == tuple(c["yxz"]), i
        tl, tv = 100 * c["dist"]
        assert np.max(np.abs(line - c["line"])) <= tl * np.max(np.abs(c["line"])), i
        assert np.max(np.abs(lvar - c["lvar"])) <= tv * np.max(np.abs(c["lvar"])), i
        assert abs(flux - c["scalars"][0]) <= tl * max(abs(c["scalars"][0]),
                                                       np.max(np.abs(c["line"]))), i
        assert abs(mse - c["scalars"][1]) <= tl * abs(c["scalars"][1]), i


def fake_result(n, Nz):
    return dict(line=np.arange(n * Nz, dtype=float).reshape(n, Nz), var=np.ones((n, Nz)),
                flux5=np.arange(n) + 0.5, mse5=np.arange(n) + 0.25,
                yxz=np.arange(3 * n, dtype=np.int32).reshape(n, 3),
                fallback=np.array([0, 1, 0][:n], np.int32), nbatch=1)


def test_cat2_columns_and_dtypes_from_a_stubbed_kernel(monkeypatch):
    """estimate_lines around a stubbed kernels.lines_estimate: the input columns plus x, y, z
    behind x0, y0, z0 and residual, flux, num_line at the end (reference :1927-1936), integer
    positions, float64 flux / residual, num_line from 1; fallback rows give ``[0]`` arrays."""
    from origin_amd import kernels, lines
    seen = {}

    def stub(ctx, raw, var, psf, weights, z0, y0, x0, *args):
        seen["args"] = args
        return fake_result(len(z0), 7)
    monkeypatch.setattr(kernels, "lines_estimate", stub)
    cat = dict(ra=np.zeros(3), dec=np.zeros(3), lbda=np.zeros(3), x0=np.array([4, 5, 6]),
               y0=np.array([1, 2, 3]), z0=np.array([9, 8, 7]), T_GLR=np.ones(3),
               profile=np.zeros(3, np.uint8))
    cat2, lin, var = lines.estimate_lines(None, cat, None, None, None, criteria="mse",
                                          order_dct=None)
    assert list(cat2) == ["ra", "dec", "lbda", "x0", "x", "y0", "y", "z0", "z", "T_GLR", "profile",
                          "residual", "flux", "num_line"]
    assert seen["args"] == (0, 1, None, 1, 5, 0)
    for k in ("x", "y", "z", "num_line"):
        assert cat2[k].dtype.kind == "i", k
    assert cat2["flux"].dtype == np.float64 and cat2["residual"].dtype == np.float64
    assert np.array_equal(cat2["y"], [0, 3, 6]) and np.array_equal(cat2["x"], [1, 4, 7])
    assert np.array_equal(cat2["z"], [2, 5, 8]) and np.array_equal(cat2["num_line"], [1, 2, 3])
    assert np.array_equal(cat2["flux"], [0.5, 1.5, 2.5])
    assert np.array_equal(cat2["residual"], [0.25, 1.25, 2.25])
    assert cat2["profile"].dtype == np.uint8 and cat2["x0"] is not cat["x0"]
    assert [a.shape for a in lin] == [(7,), (1,), (7,)] and lin[1][0] == 0 and var[1][0] == 0
    assert lin[0].dtype == np.float64 and np.array_equal(lin[2], np.arange(14, 21))
    # detection.py's table has no WCS columns
    cat = dict(x0=np.array([4]), y0=np.array([1]), z0=np.array([9]), comp=np.zeros(1, int))
    assert list(lines.estimate_lines(None, cat, None, None, None)[0]) == [
        "x0", "x", "y0", "y", "z0", "z", "comp", "residual", "flux", "num_line"]


def test_bad_arguments_raise_before_any_device_work():
    from origin_amd import lib_origin, lines
    cat = dict(x0=np.array([1]), y0=np.array([1]), z0=np.array([1]))
    w = [np.ones((4, 4))] * 2
    with pytest.raises(ValueError, match="size_grid"):
        lines.estimate_lines(None, cat, None, None, [None, None], weights=w, size_grid=1)
    with pytest.raises(ValueError, match="criteria"):
        lines.estimate_lines(None, cat, None, None, None, criteria="snr")
    with pytest.raises(ValueError, match="size_grid"):
        lib_origin.estimation_line(cat, None, None, [None, None], w, None, None, size_grid=1)
    with pytest.raises(ValueError, match="criteria"):
        lib_origin.estimation_line(cat, None, None, None, None, None, None, criteria="snr")
    with pytest.raises(ValueError, match="criteria"):
        oracle.grid_analysis(None, None, None, None, 0, 0, 0, 0, "snr", 30, 1, 5)
    assert "estimation_line" in lib_origin.__all__


# ------------------------------------------------------------------------------------ gpu
@pytest.fixture(scope="module")
def ctx():
    from origin_amd.device import default_context
    return default_context(0)


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def gaussian_psf(Nz, P, fwhm0=2.6, fwhm1=2.0):
    yy, xx = np.mgrid[:P, :P] - P // 2
    out = np.empty((Nz, P, P))
    for z in range(Nz):
        s = (fwhm0 + (fwhm1 - fwhm0) * z / (Nz - 1)) / 2.355
        g = np.exp(-(yy ** 2 + xx ** 2) / (2 * s * s))
        out[z] = g / g.sum()
    return f32(out)


class Field:
    """Noise with a continuum source and an emission line under each detection (``shift``: the
    line's offset from the catalogue position), float32-representable, and its float64 oracle."""

    def __init__(self, Nz, Ny, Nx, P, dets, seed, shifts=None, weights=None, psf2=None,
                 line_amp=300):
        rng = np.random.default_rng(seed)
        self.shape, self.P = (Nz, Ny, Nx), P
        self.psf = gaussian_psf(Nz, P)
        var = f32(rng.uniform(0.8, 1.3, (Nz, Ny, Nx)))
        raw = rng.standard_normal((Nz, Ny, Nx)) * np.sqrt(var)
        h, zz = P // 2, np.arange(Nz)
        for i, (z0, y0, x0) in enumerate(dets):
            dy, dx = shifts[i] if shifts else (0, 0)
            # (one continuum shape for all: where windows overlap the matrix stays near rank one)
            cont = (300 + 20 * i) * (1 + 0.4 * np.sin(zz / 9.0))
            line = (line_amp + 30 * i) * np.exp(-0.5 * ((zz - z0) / 1.6) ** 2)
            for spec, cy, cx in ((cont, y0, x0), (line, y0 + dy, x0 + dx)):
                ys, xs = np.arange(cy - h, cy + h + 1), np.arange(cx - h, cx + h + 1)
                oky, okx = (ys >= 0) & (ys < Ny), (xs >= 0) & (xs < Nx)
                raw[np.ix_(zz, ys[oky], xs[okx])] += (spec[:, None, None]
                                                      * self.psf[:, oky][:, :, okx])
        self.raw, self.var = f32(raw), var
        self.dets = np.array(dets)
        self.weights = weights
        self.psfs = self.psf if weights is None else [self.psf, psf2]
        self.cat = dict(x0=self.dets[:, 2], y0=self.dets[:, 1], z0=self.dets[:, 0])

    def device(self, ctx):
        return ctx.to_device(self.raw, np.float32), ctx.to_device(self.var, np.float32)

    def oracle(self, info=None, **kw):
        return oracle.estimate_lines(self.raw, self.var, self.psfs, self.weights, self.dets[:, 0],
                                     self.dets[:, 1], self.dets[:, 2], info=info, **kw)


def assert_margins(info, grid=False):
    """Conditions on the inputs, not tolerances on the kernels."""
    assert max(info["sv_ratio"]) <= 1 / 3, max(info["sv_ratio"])
    assert min(info["peak_margin"]) > 1e-6
    if grid:
        assert min(info["crit_gap"]) > 1e-6


def compare(got, ref, tol, label=""):
    """got: (cat2, lin_est, var_est) of estimate_lines; ref: the oracle's dict.  Returns the
    largest relative differences (line, var, flux, residual)."""
    cat2, lin, var = got
    worst = np.zeros(4)
    for k in ("y", "x", "z"):
        assert np.array_equal(cat2[k], ref[k]), (label, k, cat2[k], ref[k])
    for i in range(len(ref["flux"])):
        assert lin[i].shape == ref["line"][i].shape, (label, i)
        sl = np.max(np.abs(ref["line"][i])) or 1.0
        sv = np.max(np.abs(ref["var"][i])) or 1.0
        d = [np.max(np.abs(lin[i] - ref["line"][i])) / sl,
             np.max(np.abs(var[i] - ref["var"][i])) / sv,
             abs(cat2["flux"][i] - ref["flux"][i]) / (abs(ref["flux"][i]) or 1.0),
             abs(cat2["residual"][i] - ref["residual"][i]) / (abs(ref["residual"][i]) or 1.0)]
        worst = np.maximum(worst, d)
    print(f"lines {label}: max rel diff line {worst[0]:.2e} var {worst[1]:.2e} "
          f"flux {worst[2]:.2e} residual {worst[3]:.2e} (tol {tol:.1e})")
    assert np.all(worst <= tol), (label, worst, tol)
    return worst


def scattered(rng, n, Nz, Ny, Nx, zlo=8):
    """n detections, the first ones on the field's edges and corner."""
    dets = [(int(rng.integers(zlo, Nz - zlo)), int(rng.integers(0, Ny)), int(rng.integers(0, Nx)))
            for _ in range(n)]
    dets[0] = (dets[0][0], 0, Nx // 2)
    dets[1] = (dets[1][0], Ny - 1, Nx - 1)
    dets[2] = (dets[2][0], Ny // 2, 0)
    return dets


@pytest.mark.gpu
@pytest.mark.parametrize("P", [5, 7, 9])
def test_gather_against_numpy(ctx, P):
    """origin_lines_gather: ds = raw / sqrt(var) minus its row mean over the P^2 window, windows
    clipped at each of the four edges and at two corners, Nx % 4 != 0, Nz = 67 (a last block of
    three rows), ld = 32, 64, 96 with zero slack columns; row means to 1e-14 relative (the data is
    positive: the mean does not cancel), elements to 1e-14 of the row's largest |ds|."""
    from origin_amd import kernels
    Nz, Ny, Nx = 67, 13, 14
    rng = np.random.default_rng(40 + P)
    raw = f32(5 + rng.random((Nz, Ny, Nx)))
    var = f32(rng.uniform(0.5, 2.0, (Nz, Ny, Nx)))
    psf = gaussian_psf(Nz, P)
    centres = [(6, 7), (0, 6), (Ny - 1, 6), (6, 0), (6, Nx - 1), (0, 0), (Ny - 1, Nx - 1)]
    A, mean, flag = kernels.lines_gather(ctx, ctx.to_device(raw, np.float32),
                                         ctx.to_device(var, np.float32), psf, None, centres)
    ld = (P * P + 15) // 16 * 16
    assert A.shape == (len(centres), Nz, ld) and ld == {5: 32, 7: 64, 9: 96}[P]
    assert not flag.any()
    for i, (cy, cx) in enumerate(centres):
        d, inside = oracle.window(raw, cy, cx, P, 0.0)
        v, _ = oracle.window(var, cy, cx, P, np.inf)
        assert (not inside.all()) == (i > 0)
        ds = (d / np.sqrt(v)).reshape(Nz, -1)
        m = ds.mean(axis=1)
        assert np.max(np.abs(mean[i] - m) / np.abs(m)) <= 1e-14, (i, P)
        want = ds - m[:, None]
        assert np.max(np.abs(A[i][:, :P * P] - want) / np.max(np.abs(ds), axis=1)[:, None]) <= 1e-14
        assert np.all(A[i][:, P * P:] == 0)


ESTIMATOR_CASES = {(67, 5): (20, 22), (131, 13): (26, 27), (96, 25): (40, 42), (517, 9): (20, 22)}


@pytest.mark.gpu
@pytest.mark.parametrize("Nz,P", list(ESTIMATOR_CASES))
def test_estimator_against_the_oracle_in_one_and_two_batches(ctx, golden, Nz, P):
    """The whole estimator on 12 detections: Gram widths 32, 176, 640 and 96 (four per-matrix
    solver classes of origin_pca_eig; Nz = 96 < P^2 = 625 is a rank-deficient Gram), windows
    clipped at edges and a corner; then the same detections in two batches (max_problems = 6):
    bit for bit the one-batch result."""
    from origin_amd import lines
    Ny, Nx = ESTIMATOR_CASES[(Nz, P)]
    dets = scattered(np.random.default_rng(Nz + P), 12, Nz, Ny, Nx)
    f = Field(Nz, Ny, Nx, P, dets, seed=100 + Nz)
    info = {}
    ref = f.oracle(info)
    assert_margins(info)
    assert not ref["fallback"].any()
    raw, var = f.device(ctx)
    from origin_amd import kernels
    one = kernels.lines_estimate(ctx, raw, var, f.psf, None, *f.dets.T)
    two = kernels.lines_estimate(ctx, raw, var, f.psf, None, *f.dets.T, max_problems=6)
    assert (one["nbatch"], two["nbatch"]) == (1, 2)
    for k in ("line", "var", "flux5", "mse5", "yxz", "fallback"):
        assert np.array_equal(one[k], two[k]), k
    compare(lines.estimate_lines(ctx, f.cat, raw, var, f.psf), ref, device_tol(golden),
            f"Nz={Nz} P={P}")


@pytest.mark.gpu
def test_gram_groups_do_not_change_a_result(ctx):
    """The (517, 9) shape at size_grid = 1: 97 problems of 6 Gram tiles each in one batch, more
    than the largest Gram group that keeps a single problem's K-split (48 on a 256-CU device: three
    groups; restated here from the launch rule for the device at hand), against one detection, and
    so one group, per batch (max_problems = 9).  Bit for bit the same."""
    from origin_amd import kernels
    Nz, Ny, Nx, P = 517, 20, 22, 9
    f = Field(Nz, Ny, Nx, P, scattered(np.random.default_rng(12), 12, Nz, Ny, Nx), seed=617)
    nprob = int(kernels.lines_problem_counts(f.dets[:, 1], f.dets[:, 2], 1, Ny, Nx).sum())
    num_cu, tiles = num_cu_of(ctx), 6    # ld = 96: the upper triangle of 3 x 3 tiles
    ks1 = gram_geometry(num_cu, tiles, Nz)[0]
    gmax = 1
    while gmax < 1024 and gram_geometry(num_cu, (gmax + 1) * tiles, Nz)[0] == ks1:
        gmax += 1
    assert nprob > gmax, (nprob, gmax)
    raw, var = f.device(ctx)
    one = kernels.lines_estimate(ctx, raw, var, f.psf, None, *f.dets.T, size_grid=1)
    assert one["nbatch"] == 1
    many = kernels.lines_estimate(ctx, raw, var, f.psf, None, *f.dets.T, size_grid=1,
                                  max_problems=9)
    assert many["nbatch"] == 12
    for k in ("line", "var", "flux5", "mse5", "yxz", "fallback"):
        assert np.array_equal(one[k], many[k]), k


@pytest.fixture(scope="module")
def grid_field():
    """Nz = 67, P = 5: a detection at x0 = 0, one whose line sits one pixel off in y, one off in
    x and y, and an ordinary one."""
    dets = [(30, 7, 0), (25, 6, 6), (40, 10, 12), (33, 3, 9)]
    shifts = [(0, 0), (1, 0), (-1, 1), (0, 0)]
    return Field(67, 14, 17, 5, dets, seed=7, shifts=shifts, line_amp=100)


@pytest.mark.gpu
@pytest.mark.parametrize("size_grid", [0, 1])
def test_size_grid(ctx, golden, grid_field, size_grid):
    """size_grid 0 and 1: grid offsets outside the field (x0 = 0) are skipped, and with the grid
    the (y, x) of the two shifted sources move onto them."""
    from origin_amd import lines
    f = grid_field
    info = {}
    ref = f.oracle(info, size_grid=size_grid)
    assert_margins(info, grid=size_grid > 0)
    if size_grid:
        assert (ref["y"][2], ref["x"][2]) == (9, 13) != (f.dets[2][1], f.dets[2][2])
    else:
        assert np.array_equal(ref["y"], f.dets[:, 1]) and np.array_equal(ref["x"], f.dets[:, 2])
    raw, var = f.device(ctx)
    compare(lines.estimate_lines(ctx, f.cat, raw, var, f.psf, size_grid=size_grid), ref,
            device_tol(golden), f"size_grid={size_grid}")


@pytest.mark.gpu
def test_ends_of_the_spectral_axis(ctx, golden):
    """z0 = 3 and z0 = Nz - 2: the clipped peakdet window, maxz = z0 - 5 + z_est with the
    reference's arithmetic (z0 < 5) and the slice(maxz - 5, maxz + 6) whose negative start counts
    from the end (an empty range: flux criterion 0); the selection entry point on the oracle's
    own deconvolutions gives the same rows."""
    from origin_amd import kernels, lines
    Nz = 67
    f = Field(Nz, 12, 13, 5, [(3, 5, 6), (Nz - 2, 6, 4), (30, 8, 8)], seed=9)
    info = {}
    ref = f.oracle(info)
    assert_margins(info)
    assert ref["z"][0] < 5 and ref["z"][1] >= Nz - 6
    raw, var = f.device(ctx)
    compare(lines.estimate_lines(ctx, f.cat, raw, var, f.psf), ref, device_tol(golden), "ends")
    sel = kernels.lines_select(ctx, raw, f.psf, None, *f.dets.T, np.array(ref["line"]),
                               np.array(ref["var"]), np.zeros(3, np.int32))
    assert np.array_equal(sel["yxz"], np.stack([ref["y"], ref["x"], ref["z"]], axis=1))
    assert np.array_equal(sel["line"], np.array(ref["line"])) and not sel["fallback"].any()
    assert np.max(np.abs(sel["flux5"] - ref["flux"]) / np.abs(ref["flux"])) <= 1e-14
    assert np.max(np.abs(sel["mse5"] - ref["residual"]) / np.abs(ref["residual"])) <= 1e-13


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(criteria="mse", size_grid=1), dict(order_dct=None),
                                dict(order_dct=10, horiz_psf=2, horiz=3)],
                         ids=["mse", "no_dct", "dct10"])
def test_criteria_and_dct_order(ctx, golden, grid_field, kw):
    from origin_amd import lines
    f = grid_field
    info = {}
    ref = f.oracle(info, **kw)
    assert_margins(info, grid="size_grid" in kw)
    assert not ref["fallback"].any()
    raw, var = f.device(ctx)
    compare(lines.estimate_lines(ctx, f.cat, raw, var, f.psf, **kw), ref, device_tol(golden),
            str(kw))


@pytest.mark.gpu
def test_two_weighted_fields(ctx, golden):
    """A mosaic of two weighted fields at size_grid = 0; the second field covers only x >= 8, so
    it does not cover the first detection's window."""
    from origin_amd import lines
    Nz, Ny, Nx, P = 67, 12, 18, 5
    w0 = f32(np.linspace(0.3, 0.9, Nx)[None, :] * np.ones((Ny, 1)))
    w1 = f32(1 - w0)
    w1[:, :8] = 0
    dets = [(30, 6, 3), (25, 5, 11), (40, 9, 14)]
    f = Field(Nz, Ny, Nx, P, dets, seed=12, weights=[w0, w1], psf2=gaussian_psf(Nz, P, 3.0, 2.4))
    assert oracle.window(w1[None], 6, 3, P, 0.0)[0].sum() == 0
    info = {}
    ref = f.oracle(info)
    assert_margins(info)
    raw, var = f.device(ctx)
    compare(lines.estimate_lines(ctx, f.cat, raw, var, f.psfs, weights=f.weights), ref,
            device_tol(golden), "weighted")


@pytest.mark.gpu
def test_fallback_rows(ctx, golden):
    """A detection in a fully masked region (data 0, var inf) and one with a var == 0 voxel in its
    window come back as the fallback row (0.0, 1e6, [0], [0], y0, x0, z0); the detections around
    them are what they are without the damage (bit for bit: nothing is shared between problems)."""
    from origin_amd import lines
    Nz, Ny, Nx, P = 67, 14, 24, 5
    dets = [(30, 6, 3), (25, 7, 10), (40, 5, 16), (35, 9, 21), (20, 11, 3)]
    f = Field(Nz, Ny, Nx, P, dets, seed=15)
    raw, var = f.device(ctx)
    clean = lines.estimate_lines(ctx, f.cat, raw, var, f.psf)
    f.raw[:, 4:11, 7:14] = 0
    f.var[:, 4:11, 7:14] = np.inf         # detection 1: masked
    f.var[11, 6, 17] = 0                  # detection 2: a var == 0 voxel in its window
    ref = f.oracle()
    assert list(ref["fallback"]) == [False, True, True, False, False]
    raw, var = f.device(ctx)
    got = lines.estimate_lines(ctx, f.cat, raw, var, f.psf)
    compare(got, ref, device_tol(golden), "fallback")
    cat2, lin, lvar = got
    for i in (1, 2):
        assert (cat2["flux"][i], cat2["residual"][i]) == (0.0, 1e6)
        assert (cat2["z"][i], cat2["y"][i], cat2["x"][i]) == dets[i]
        assert np.array_equal(lin[i], [0]) and np.array_equal(lvar[i], [0])
    for i in (0, 3, 4):
        assert np.array_equal(lin[i], clean[1][i]) and np.array_equal(lvar[i], clean[2][i])
        assert cat2["flux"][i] == clean[0]["flux"][i]


@pytest.mark.gpu
def test_function_seam_equals_estimate_lines(ctx, grid_field):
    """lib_origin.estimation_line (host arrays in, the reference's positional signature) gives
    what lines.estimate_lines gives on the device cubes."""
    from origin_amd import lib_origin, lines
    f = grid_field
    raw, var = f.device(ctx)
    want = lines.estimate_lines(ctx, f.cat, raw, var, f.psf, size_grid=1)
    cat2, lin, lvar = lib_origin.estimation_line(f.cat, f.raw, f.var, f.psf, None, None, None)
    assert list(cat2) == list(want[0])
    for k in cat2:
        assert np.array_equal(cat2[k], want[0][k]), k
    assert all(np.array_equal(a, b) for a, b in zip(lin, want[1]))
    assert all(np.array_equal(a, b) for a, b in zip(lvar, want[2]))


@pytest.mark.gpu
def test_from_session_after_steps_1_to_7(ctx):
    """lines.from_session on the detections of step 7 of a small session: the cubes step 1 left
    on the device, the session's PSF; the rows equal estimate_lines on fresh uploads."""
    from origin_amd import synth
    from origin_amd import detection, lines
    from origin_amd.steps import SimpleOrig
    f, raw, var, mask = synth.small_case(Nz=160, Ny=48, Nx=52, seed=3, psf_size=9, nprof=3,
                                         area_size=24)
    orig = SimpleOrig(raw, var, mask, f.PSF.astype(float), f.profiles, ctx=ctx)
    orig.step01_preprocessing()
    orig.step02_areas.set_areamap(f.areamap)
    orig.step03_compute_PCA_threshold()
    orig.step04_compute_greedy_PCA()
    orig.step05_compute_TGLR()
    lmax = orig.cube_local_max._data
    smax = orig.cube_std_local_max._data
    t_cor = float(np.sort(lmax[lmax > 0])[-12])
    t_std = float(np.sort(smax[smax > 0])[-12])
    _, cat, _ = detection.from_session(orig, threshold=t_cor, threshold_std=t_std)
    n = len(cat["z0"])
    assert 5 <= n <= 20
    cat2, lin, lvar = lines.from_session(orig, cat)
    assert list(cat2)[:6] == ["x0", "x", "y0", "y", "z0", "z"] and len(lin) == len(lvar) == n
    assert np.array_equal(cat2["num_line"], np.arange(1, n + 1))
    assert np.array_equal(cat2["x"], cat["x0"]) and np.array_equal(cat2["y"], cat["y0"])
    want = lines.estimate_lines(ctx, cat, ctx.to_device(np.asarray(raw), np.float32),
                                ctx.to_device(np.asarray(var), np.float32), f.PSF.astype(float))
    for k in cat2:
        assert np.array_equal(cat2[k], want[0][k], equal_nan=cat2[k].dtype.kind == "f"), k
    assert all(np.array_equal(a, b) for a, b in zip(lin, want[1]))
    assert all(a.shape in ((160,), (1,)) and np.all(np.isfinite(a)) for a in lin)
