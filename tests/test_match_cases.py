"""CPU: the point lists of tests/_match_cases.py are what they claim, ``cKDTree`` agrees with the
float64 predicate on every one of them (the condition they were chosen under: the device is
compared with the predicate, the reference uses the trees), the two oracles of the true-purity
table agree, and the seam has the new function with its refusals.  Nothing here touches a device."""
import numpy as np
import pytest

import _match_cases as mc
import _match_oracle as oracle

CASES = list(mc.cases())


@pytest.mark.parametrize("name", CASES)
def test_tree_equals_the_predicate_pair_for_pair(name):
    a, b, _ = mc.cases()[name]
    for r in mc.RADII:
        assert np.array_equal(oracle.tree_pairs(a, b, r), oracle.pairs(a, b, r)), (name, r)


def test_sizes_family_has_every_size():
    sizes = {int(c[0][0].size) for c in mc.family("A_").values()} | \
        {int(c[1][0].size) for c in mc.family("A_").values()}
    assert {0, 1, 63, 64, 65, 257, 4099} <= sizes
    a, b, _ = mc.cases()["A_coincident_1x1x1"]
    assert all(not c.any() for c in a + b)


def test_ties_family_has_exact_ties():
    a, b, _ = mc.cases()["B_ties"]
    assert all(np.array_equal(c * 4, np.round(c * 4)) for c in b)       # the quarter grid
    d2 = oracle.d2(a, b)
    for v in (0.0, 6.0, 6.25, 8.0, 20.25):
        assert (d2 == v).any(), v
    # decided by the tie: a B point whose only partners within 2.5 (4.5) sit exactly at it
    for r in (2.5, 4.5):
        only_ties = ((d2 <= r * r).any(axis=0)) & ~((d2 < r * r).any(axis=0))
        assert only_ties.any(), r


def test_bbox_family_leaves_the_range_of_a():
    a, b, _ = mc.cases()["C_bbox_outside"]
    Nz, Ny, Nx = mc.FIELD
    corners = {(x, y, z) for x in (0, Nx - 1) for y in (0, Ny - 1) for z in (0, Nz - 1)}
    assert corners <= set(zip(*a))
    out = np.maximum(a[0].min() - b[0], b[0] - a[0].max())              # how far outside in x
    hit = oracle.pairs(a, b, 4.5).any(axis=0)
    assert (hit & (out > 0) & (out <= 4.5)).any() and ((out > 4.5) & ~hit).any()
    assert (b[0] < 0).any() and (b[1] < 0).any() and (b[2] < 0).any()
    a, b, _ = mc.cases()["C_bbox_negative"]
    assert all(c.max() < 0 for c in a)


@pytest.mark.parametrize("r", mc.SHELL_RADII)
def test_shell_family_decides_at_the_last_bits(r):
    a, b, _ = mc.cases()[f"D_shell_{r}"]
    d2 = oracle.d2(a, b)
    r2 = r * r
    near = np.abs(d2 - r2) <= 4 * np.spacing(r2)
    assert np.count_nonzero(near) >= 100
    assert (near & (d2 <= r2)).any() and (near & (d2 > r2)).any()


def test_load_family_fills_a_cell_and_a_column():
    _, b, _ = mc.cases()["E_load_one_cell"]
    cell = np.floor(np.array(b)).astype(int)
    assert np.unique(cell, axis=1, return_counts=True)[1].max() > 256
    a, b, _ = mc.cases()["E_load_column_3681"]
    assert len(set(zip(b[0], b[1]))) == 1 and b[0].size == 600
    assert b[2].max() - b[2].min() > 3000 and a[2].max() == 3680
    assert np.unique(b[2]).size < b[2].size                             # duplicates inside B
    a, b, _ = mc.cases()["E_load_duplicates"]
    assert np.unique(np.array(a), axis=1).shape[1] < a[0].size
    assert np.unique(np.array(b), axis=1).shape[1] < b[0].size


def test_bmax_family():
    a, b, v = mc.cases()["F_bmax"]
    p = oracle.pairs(a, b, 1.0)
    near = [v[p[:, j]] for j in range(b[0].size)]
    assert len(near[0]) >= 3 and np.unique(near[0]).size == len(near[0]) and near[0].min() < 0
    assert len(near[1]) >= 2 and np.unique(near[1]).size == 1
    assert len(near[2]) >= 2 and near[2].max() < 0
    assert len(near[3]) == 0
    ref = oracle.brute(a, b, 1.0, v)["b_max"]
    assert ref.dtype == np.float32 and ref[3] == -np.inf and ref[0] == np.float32(7.25)
    for _, _, val in mc.cases().values():
        assert val.dtype == np.float32 and not (val == 0).any() and np.isfinite(val).all()


# ------------------------------------------------------------------------------ the table
def _small_cube(seed=3):
    rng = np.random.default_rng(seed)
    cube = np.zeros((12, 9, 7), np.float32)
    at = rng.random(cube.shape) < 0.08
    cube[at] = rng.uniform(3.5, 7.5, int(at.sum())).astype(np.float32)
    ref = (rng.uniform(-2, 8, 9), rng.uniform(-2, 10, 9), rng.uniform(-2, 13, 9))
    return cube, ref


def test_restated_reference_equals_the_direct_computation():
    cube, ref = _small_cube()
    for maxdist, tmax in ((4.5, 7), (1.0, 7), (2.5, 8.2)):
        t = oracle.true_purity_trees(cube, ref, 14, maxdist, 4, tmax)
        d = oracle.true_purity_direct(cube, ref, 14, maxdist, 4, tmax)
        assert list(t) == list(oracle.COLUMNS)
        for k in oracle.COLUMNS:
            assert np.array_equal(t[k], d[k], equal_nan=True), k
        assert np.array_equal(np.isnan(t["purity"]), t["ndetect"] == 0)
    assert np.isnan(t["purity"]).any() and t["ntrue"].max() > 0 and t["nmiss"].min() < 14


# ------------------------------------------------------------------------------ the seam
def test_seam_has_the_function_and_the_entry():
    from origin_amd import _capi, lib_origin
    assert callable(lib_origin.compute_true_purity)
    assert "origin_ball_match" in _capi.SIGNATURES


class _NoDevice:
    """A cube that fails the test if anything tries to make it resident."""

    shape = (4, 3, 2)

    def __getattr__(self, name):
        if name in ("wave", "wave_header"):
            raise AttributeError(name)
        raise AssertionError(f"the cube was touched ({name}) before the arguments were refused")


def test_seam_refuses_before_any_device_call(monkeypatch):
    from origin_amd import lib_origin

    def no_ctx(*a, **k):
        raise AssertionError("a context was asked for")

    monkeypatch.setattr(lib_origin, "_ctx", no_ctx)
    cat = dict(TYPE=np.array([6, 1]), Q=np.array([1.0, 2.0]), P=np.array([1.0, 2.0]),
               LOBS=np.array([5000.0, 5100.0]))
    cards = dict(CRVAL3=4750.0, CRPIX3=1.0, CD3_3=1.25)
    with pytest.raises(ValueError, match="LOBS"):
        lib_origin.compute_true_purity(_NoDevice(), {k: v for k, v in cat.items() if k != "LOBS"},
                                       wave=cards)
    with pytest.raises(ValueError, match="wave"):
        lib_origin.compute_true_purity(_NoDevice(), cat)
    # no figure is drawn: ImportError without matplotlib, NotImplementedError with it
    with pytest.raises((ImportError, NotImplementedError)):
        lib_origin.compute_true_purity(_NoDevice(), cat, wave=cards, plot=True)
    with pytest.raises(ValueError, match="CRPIX3"):
        lib_origin.compute_true_purity(_NoDevice(), cat, wave=dict(CRVAL3=4750.0, CD3_3=1.25))
