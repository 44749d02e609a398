"""GPU: ``origin_ball_match`` (csrc/match.hip) against the float64 predicate in NumPy on every point
list of tests/_match_cases.py at every radius.  All comparisons are exact: flags and float32
values bit for bit; there is no tolerance."""
import numpy as np
import pytest

import _match_cases as mc
import _match_oracle as oracle

pytestmark = pytest.mark.gpu

CASES = list(mc.cases())
SUBSET_CASES = ("A_sizes_63_65", "B_ties", "C_bbox_outside", "E_load_one_cell", "F_bmax")


@pytest.fixture(scope="module")
def ctx():
    from origin_amd.device import default_context
    return default_context(0)


def _same_bits(got, ref):
    return got.dtype == ref.dtype and got.shape == ref.shape and got.tobytes() == ref.tobytes()


@pytest.mark.parametrize("r", mc.RADII)
@pytest.mark.parametrize("name", CASES)
def test_device_equals_the_predicate(ctx, name, r):
    from origin_amd import kernels
    a, b, val = mc.cases()[name]
    ref = oracle.brute(a, b, r, val)
    got = kernels.ball_match(ctx, a, b, r, val)
    assert sorted(got) == ["a_hit", "b_hit", "b_max"]
    assert np.array_equal(got["a_hit"], ref["a_hit"].astype(np.uint8))
    assert np.array_equal(got["b_hit"], ref["b_hit"].astype(np.uint8))
    assert _same_bits(got["b_max"], ref["b_max"])
    assert np.array_equal(got["b_max"] == -np.inf, ~ref["b_hit"])
    # a_hit alone: a query stops at its first partner
    alone = kernels.ball_match(ctx, a, b, r, want=("a_hit",))
    assert list(alone) == ["a_hit"] and _same_bits(alone["a_hit"], got["a_hit"])


@pytest.mark.parametrize("name", SUBSET_CASES)
def test_output_subsets(ctx, name):
    from origin_amd import kernels
    a, b, val = mc.cases()[name]
    for r in (1.0, 2.5):
        ref = oracle.brute(a, b, r, val)
        only_a = kernels.ball_match(ctx, a, b, r, want=("a_hit",))
        only_b = kernels.ball_match(ctx, a, b, r, want=("b_hit",))
        no_val = kernels.ball_match(ctx, a, b, r)
        only_max = kernels.ball_match(ctx, a, b, r, val, want=("b_max",))
        assert list(only_a) == ["a_hit"] and list(only_b) == ["b_hit"]
        assert sorted(no_val) == ["a_hit", "b_hit"] and list(only_max) == ["b_max"]
        for got in (only_a, no_val):
            assert np.array_equal(got["a_hit"], ref["a_hit"].astype(np.uint8))
        for got in (only_b, no_val):
            assert np.array_equal(got["b_hit"], ref["b_hit"].astype(np.uint8))
        assert _same_bits(only_max["b_max"], ref["b_max"])


def test_the_package_level_call_returns_bool_and_float64(ctx):
    from origin_amd import match
    a, b, val = mc.cases()["F_bmax"]
    ref = oracle.brute(a, b, 1.0, val)
    got = match.ball_match(ctx, a, b, 1.0, a_val=val)
    assert got["a_hit"].dtype == bool and got["b_hit"].dtype == bool
    assert got["b_max"].dtype == np.float64
    assert np.array_equal(got["a_hit"], ref["a_hit"]) and np.array_equal(got["b_hit"], ref["b_hit"])
    assert np.array_equal(got["b_max"], ref["b_max"].astype(np.float64))
    assert sorted(match.ball_match(ctx, a, b, 1.0)) == ["a_hit", "b_hit"]


def test_refusals(ctx):
    from origin_amd import kernels
    from origin_amd._capi import OriginHipError
    a, b, val = mc.cases()["F_bmax"]
    bad = (a[0].copy(), a[1], a[2])
    bad[0][3] = np.nan
    inf_b = (b[0], b[1].copy(), b[2])
    inf_b[1][0] = np.inf
    nan_val = val.copy()
    nan_val[2] = np.nan
    for args, kw in (((bad, b, 1.0), {}), ((a, inf_b, 1.0), {}), ((a, b, -1.0), {}),
                     ((a, b, 1.0, nan_val), {}),
                     ((a, b, np.nan), {}), ((a, b, np.inf), {}),
                     ((a, b, 1.0), dict(want=("a_hit", "b_max")))):
        with pytest.raises(OriginHipError) as e:
            kernels.ball_match(ctx, *args, **kw)
        assert e.value.code == -1 and "ORIGIN_E_ARG" in str(e.value)
    # the context is as usable as before
    ref = oracle.brute(a, b, 1.0, val)
    assert np.array_equal(kernels.ball_match(ctx, a, b, 1.0)["a_hit"], ref["a_hit"].astype(np.uint8))


@pytest.mark.parametrize("name", ("B_ties", "E_load_one_cell", "E_load_column_3681", "D_shell_2.5"))
def test_a_permutation_of_b_permutes_its_outputs_only(ctx, name):
    """Slot order inside a cell comes from atomics; it must not show."""
    from origin_amd import kernels
    a, b, val = mc.cases()[name]
    perm = np.random.default_rng(5).permutation(b[0].size)
    for r in (2.5, 4.5):
        one = kernels.ball_match(ctx, a, b, r, val)
        two = kernels.ball_match(ctx, a, tuple(c[perm] for c in b), r, val)
        assert np.array_equal(two["a_hit"], one["a_hit"])
        assert np.array_equal(two["b_hit"], one["b_hit"][perm])
        assert _same_bits(two["b_max"], one["b_max"][perm])
        again = kernels.ball_match(ctx, a, b, r, val)
        assert all(_same_bits(again[k], one[k]) for k in one)
