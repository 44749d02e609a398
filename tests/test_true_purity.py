"""GPU: ``lib_origin.compute_true_purity`` against the restated reference (one cKDTree per
threshold, tests/_match_oracle.py) for a local-maximum cube in four forms, the reference table as
a mapping and as a FITS file, the wave axis as an object and as header cards; and step 7's std
match on the device against the host ``unmatched_std``.  Every comparison is exact."""
import numpy as np
import pytest

import _match_oracle as oracle
from _cube_forms import as_sparse

pytestmark = pytest.mark.gpu

SHAPE = (40, 23, 17)
CARDS = dict(CRVAL3=4750.0, CRPIX3=1.0, CD3_3=1.25, CTYPE3="AWAV", CUNIT3="Angstrom")
FORMS = ("host", "device", "sparse", "lazy")


class Wave:
    """An object with mpdaf's ``WaveCoord.pixel``: the linear axis of CARDS."""

    def pixel(self, lbda):
        return (np.asarray(lbda, dtype=np.float64) - 4750.0) / 1.25 + 1.0 - 1.0


@pytest.fixture(scope="module")
def ctx():
    from origin_amd.device import default_context
    return default_context(0)


@pytest.fixture(scope="module")
def cube():
    """About 2 % non-zero voxels in [3.5, 7.5]; values equal to float32(thr) and its two float32
    neighbours for several thresholds of the grid; 30 maxima around the line at (8, 11, 20.5)."""
    rng = np.random.default_rng(11)
    c = np.zeros(SHAPE, np.float32)
    at = rng.random(SHAPE) < 0.02
    c[at] = rng.uniform(3.5, 7.5, int(at.sum())).astype(np.float32)
    z, y, x = (rng.integers(lo, hi, 60) for lo, hi in ((17, 25), (8, 15), (5, 12)))
    for zz, yy, xx in list(dict.fromkeys(zip(z, y, x)))[:30]:
        c[zz, yy, xx] = np.float32(rng.uniform(3.8, 7.4))
    grid = np.arange(4, 7, 0.1)
    spots = np.flatnonzero(c.reshape(-1) == 0)[::97]
    k = 0
    for thr in grid[[0, 1, 3, 7, 12, 20, 29]]:
        t32 = np.float32(thr)
        for v in (t32, np.nextafter(t32, np.float32(np.inf)), np.nextafter(t32, np.float32(-np.inf))):
            c.reshape(-1)[spots[k]] = v
            k += 1
    c.setflags(write=False)
    return c


@pytest.fixture(scope="module")
def refcat():
    """25 rows, 18 of them lines (TYPE 6): some outside the field, some with nothing near, two
    that share the cluster's detections."""
    rng = np.random.default_rng(12)
    q = np.concatenate([[8.0, 9.5, -3.0, 30.0, 5.25, 16.75, 2.0, 12.5], rng.uniform(-2, 18, 17)])
    p = np.concatenate([[11.0, 11.5, 4.0, 11.0, -2.5, 22.0, 2.0, 40.0], rng.uniform(-2, 24, 17)])
    zz = np.concatenate([[20.5, 21.25, 10.0, 20.0, 7.75, 44.0, -1.5, 3.0],
                         np.round(rng.uniform(-3, 43, 17) * 4) / 4])
    typ = np.full(25, 6, np.int64)
    typ[[6, 9, 12, 15, 18, 21, 24]] = [1, 2, 3, 0, 5, 7, 1]
    cat = dict(ID=np.arange(25, dtype=np.int64), TYPE=typ, Q=q, P=p, LOBS=4750.0 + 1.25 * zz)
    assert np.count_nonzero(typ == 6) == 18
    assert np.array_equal(Wave().pixel(cat["LOBS"]), zz)
    return cat


def _form(ctx, cube, form):
    from origin_amd.cubes import LazyCube
    if form == "host":
        return cube
    if form == "device":
        return ctx.to_device(cube)
    if form == "sparse":
        return as_sparse(ctx, cube)
    return LazyCube(dev=as_sparse(ctx, cube))


def _expected(cube, refcat, maxdist, threshmin, threshmax):
    six = refcat["TYPE"] == 6
    ref = (refcat["Q"][six], refcat["P"][six], Wave().pixel(refcat["LOBS"][six]))
    return oracle.true_purity_trees(cube, ref, 25, maxdist, threshmin, threshmax)


def _assert_same_table(got, ref):
    assert list(got) == list(oracle.COLUMNS)
    for k in oracle.COLUMNS:
        assert got[k].dtype == ref[k].dtype, k
        assert np.array_equal(got[k], ref[k], equal_nan=True), k


def test_the_fixture_is_what_it_claims(cube, refcat):
    nz = cube[cube != 0]
    assert 0.015 < nz.size / cube.size < 0.03 and nz.min() >= 3.5 and nz.max() <= 7.5
    ref = _expected(cube, refcat, 4.5, 4, 7)
    assert ref["ntrue"][0] >= 30 and ref["nfalse"].min() > 0
    assert ref["nmiss"].min() >= 7 and ref["nmiss"].min() < 25 and ref["nmiss"].max() > ref["nmiss"].min()
    grid = np.arange(4, 7, 0.1)
    assert sum(bool((cube == np.float32(t)).any()) for t in grid) >= 7


@pytest.mark.parametrize("form", FORMS)
def test_table_equals_the_restated_reference(ctx, cube, refcat, form, tmp_path):
    from origin_amd import fitsio, lib_origin
    path = fitsio.write_table(str(tmp_path / "refcat.fits"), refcat)
    ref = _expected(cube, refcat, 4.5, 4, 7)
    for cat in (refcat, path):
        for wave in (Wave(), CARDS):
            got = lib_origin.compute_true_purity(_form(ctx, cube, form), cat, wave=wave)
            _assert_same_table(got, ref)
    assert not np.isnan(got["purity"]).any()
    # nref counts every row of the catalogue, not only the 18 lines
    assert got["nmiss"].min() >= 25 - 18


@pytest.mark.parametrize("form", FORMS)
def test_other_radius_and_thresholds_above_the_maximum(ctx, cube, refcat, form):
    from origin_amd import lib_origin
    ref = _expected(cube, refcat, 2.5, 3.75, 8.2)
    got = lib_origin.compute_true_purity(_form(ctx, cube, form), refcat, 2.5, 3.75, 8.2, wave=CARDS)
    _assert_same_table(got, ref)
    assert np.array_equal(np.isnan(got["purity"]), got["ndetect"] == 0)
    assert np.isnan(got["purity"]).any() and not np.isnan(got["purity"]).all()


def test_wave_of_the_cube(ctx, cube, refcat):
    from origin_amd import lib_origin
    from origin_amd.cubes import LazyCube
    ref = _expected(cube, refcat, 4.5, 4, 7)
    with_wave = LazyCube(dev=ctx.to_device(cube))
    with_wave.wave = Wave()
    _assert_same_table(lib_origin.compute_true_purity(with_wave, refcat), ref)
    with_cards = LazyCube(dev=ctx.to_device(cube))
    with_cards.wave = CARDS
    _assert_same_table(lib_origin.compute_true_purity(with_cards, refcat), ref)
    # the argument goes first
    with_wave.wave = object()
    _assert_same_table(lib_origin.compute_true_purity(with_wave, refcat, wave=CARDS), ref)


def test_no_reference_lines_and_no_detections(ctx, cube, refcat):
    from origin_amd import match
    none = (np.zeros(0), np.zeros(0), np.zeros(0))
    got = match.true_purity(ctx, cube, none, 25)
    _assert_same_table(got, oracle.true_purity_trees(cube, none, 25))
    assert not got["ntrue"].any() and (got["nmiss"] == 25).all()
    six = refcat["TYPE"] == 6
    ref = (refcat["Q"][six], refcat["P"][six], Wave().pixel(refcat["LOBS"][six]))
    empty = np.zeros(SHAPE, np.float32)
    got = match.true_purity(ctx, empty, ref, 25)
    _assert_same_table(got, oracle.true_purity_trees(empty, ref, 25))
    assert np.isnan(got["purity"]).all()


# ------------------------------------------------------------------------------ step 7
def _step7_cubes():
    """Correl maxima, std maxima at d2 = 6 (matched at 2.5) and d2 = 8 (kept) from them, next to a
    correl maximum at distance 0 and 1, one far from everything; values 5 / 9 so that thresholds of
    4 and 8 take all of a cube and 20 takes none."""
    lmax = np.zeros(SHAPE, np.float32)
    lstd = np.zeros(SHAPE, np.float32)
    prof = np.zeros(SHAPE, np.uint8)
    correl = [(10, 5, 4), (10, 15, 4), (25, 5, 10), (25, 15, 10), (33, 20, 14), (5, 20, 2)]
    for i, (z, y, x) in enumerate(correl):
        lmax[z, y, x] = 5 + i / 4
        prof[z, y, x] = i + 1
    std = [(10 + 1, 5 + 1, 4 + 2),      # d2 = 6 from correl 0
           (10, 15 + 2, 4 + 2),         # d2 = 8 from correl 1
           (25 - 2, 5 - 1, 10 + 1),     # d2 = 6
           (25 + 2, 15, 10 - 2),        # d2 = 8
           (33, 20, 14),                # d2 = 0
           (5, 20 + 1, 2),              # d2 = 1
           (38, 1, 15)]                 # far from everything
    for i, (z, y, x) in enumerate(std):
        lstd[z, y, x] = 9 + i / 8
    return lmax, prof, lstd


class _TreeSpy:
    def __init__(self, real):
        self.real, self.made = real, 0

    def __call__(self, *a, **k):
        self.made += 1
        return self.real(*a, **k)


@pytest.mark.parametrize("thr, thr_std, nkept", [(4.0, 8.0, 3), (20.0, 8.0, 7), (4.0, 20.0, 0),
                                                  (20.0, 20.0, 0)])
def test_step7_keeps_the_rows_unmatched_std_keeps(ctx, monkeypatch, thr, thr_std, nkept):
    import scipy.spatial
    from origin_amd import detection
    lmax, prof, lstd = _step7_cubes()
    spy = _TreeSpy(scipy.spatial.cKDTree)
    monkeypatch.setattr(scipy.spatial, "cKDTree", spy)
    cat0, cat, kept = detection.threshold_detections(ctx, lmax, prof, lstd, thr, thr_std, 2.5)
    assert spy.made == 0, "threshold_detections still builds a cKDTree"
    n = len(cat["z0"])
    cat_std = {k: v[n:] for k, v in cat0.items()}
    assert (cat_std["comp"] == 1).all() and (cat["comp"] == 0).all()
    keep = detection.unmatched_std(cat, cat_std, 2.5)
    assert (spy.made > 0) == (n > 0 and len(cat_std["z0"]) > 0)      # the spy sees the host form
    assert len(keep) == nkept
    assert list(kept) == list(cat_std)
    for k, v in cat_std.items():
        assert kept[k].dtype == v.dtype, k
        assert kept[k].tobytes() == v[keep].tobytes(), k
    if nkept == 3:
        assert sorted(zip(kept["z0"], kept["y0"], kept["x0"])) == [(10, 17, 6), (27, 15, 8), (38, 1, 15)]
