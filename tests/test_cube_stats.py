"""Moments and standard deviation of a device cube (csrc/stats.hip, kernels.cube_moments /
cube_std, session.TiledCube.moments / std): the two ``np.std`` calls of the reference's
``add_tglr_stat`` (lib_origin.py:2127-2129) as reductions on the device.

Reference: float64 NumPy sums of the same float32 values, ``np.std(a.astype(np.float64))``.
Tolerance (derived, not measured; both sides are float64): 1e-12 relative on ``std`` and on each
sum relative to the sum of the absolute values of its terms.  The device's longest serial chain
at the largest shape here is a few thousand terms per accumulator, so its worst case is about
10^3 * 2^-53 ~ 1e-13 and the tree stages add less; NumPy's pairwise sums are below that.  The
mean's error enters M2 only squared.  Every test prints its figures before it asserts.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-12
BIG_YX = (129, 131)
MEDIUM = (17, 33, 35)      # 20 blocks, S odd, voxel count not a multiple of 4


@pytest.fixture(scope="module")
def ctx():
    from origin_amd.device import default_context
    return default_context(0)


def reference(a, shift=0.0, keep=None):
    """(n, s1, s2, sum |x - shift|) in float64 over the kept spaxels of the float32 cube a."""
    d = a.astype(np.float64).reshape(a.shape[0], -1)
    if keep is not None:
        d = d[:, np.asarray(keep).reshape(-1) != 0]
    d = d - shift
    return float(d.size), float(np.sum(d)), float(np.sum(d * d)), float(np.sum(np.abs(d)))


def check_moments(ctx, dev, a, shift=0.0, keep=None, tag=""):
    from origin_amd import kernels
    k = None if keep is None else ctx.to_device(np.ascontiguousarray(keep, np.uint8).reshape(-1))
    n, s1, s2 = kernels.cube_moments(ctx, dev, shift, k)
    rn, r1, r2, rabs = reference(a, shift, keep)
    e1 = abs(s1 - r1) / rabs if rabs else abs(s1 - r1)
    e2 = abs(s2 - r2) / r2 if r2 else abs(s2 - r2)
    print(f"cube_moments {tag} shape {a.shape} shift {shift:g}: n {n:.0f} "
          f"err(s1)/sum|t| {e1:.3e} err(s2)/sum|t| {e2:.3e}")
    assert n == rn
    assert e1 <= RTOL and e2 <= RTOL
    return n, s1, s2


def check_std(ctx, dev, a, keep=None, tag=""):
    from origin_amd import kernels
    k = None if keep is None else ctx.to_device(np.ascontiguousarray(keep, np.uint8).reshape(-1))
    got = kernels.cube_std(ctx, dev, k)
    d = a.astype(np.float64).reshape(a.shape[0], -1)
    if keep is not None:
        d = d[:, np.asarray(keep).reshape(-1) != 0]
    want = float(np.std(d))
    err = abs(got - want) / want if want else abs(got - want)
    print(f"cube_std {tag} shape {a.shape}: got {got!r} want {want!r} rel err {err:.3e}")
    assert err <= RTOL
    return got


@pytest.fixture(scope="module")
def big(ctx):
    """A cube of more than three sweeps of the launch grid (and not a multiple of one), from the
    launch constants; host array and device copy shared by the tests below, never modified."""
    from origin_amd import kernels
    sweep = kernels.cube_moments_sweep(1 << 40)          # the grid at its cap
    assert sweep == 1024 * kernels.MOMENTS_LANES * kernels.MOMENTS_VEC
    s = BIG_YX[0] * BIG_YX[1]
    nz = int(np.ceil(3.2 * sweep / s))
    n = nz * s
    assert n >= 3 * sweep and n % sweep != 0 and n % 4 != 0 and s % 2 == 1
    assert kernels.cube_moments_sweep(n) == sweep
    rng = np.random.default_rng(5)
    a = rng.normal(0.2, 3.0, (nz,) + BIG_YX).astype(np.float32)
    return a, ctx.to_device(a)


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 7), MEDIUM])
def test_moments_and_std_small_shapes(ctx, shape):
    rng = np.random.default_rng(sum(shape))
    a = rng.normal(-0.5, 2.0, shape).astype(np.float32)
    dev = ctx.to_device(a)
    n, s1, _ = check_moments(ctx, dev, a, 0.0, tag="small")
    check_moments(ctx, dev, a, s1 / n, tag="small")
    check_moments(ctx, dev, a, 0.37, tag="small")
    check_std(ctx, dev, a, tag="small")


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_misaligned_view(ctx, offset):
    """A cube that starts 4, 8 or 12 bytes behind a 16-byte boundary: head voxels are read as
    scalars, the vectors start at the boundary."""
    shape = (5, 7, 9)
    n = int(np.prod(shape))
    rng = np.random.default_rng(offset)
    buf = rng.normal(1.0, 2.0, n + 8).astype(np.float32)
    buf[:offset] = np.nan                     # what lies before and behind the view is not read
    buf[offset + n:] = np.nan
    whole = ctx.to_device(buf)
    assert whole.ptr % 16 == 0
    dev = whole.view(offset, shape)
    a = buf[offset:offset + n].reshape(shape)
    check_moments(ctx, dev, a, 0.25, tag=f"offset {offset}")
    keep = (np.arange(63) % 3 != 0).astype(np.uint8)
    check_moments(ctx, dev, a, 0.25, keep, tag=f"offset {offset} keep")
    check_std(ctx, dev, a, tag=f"offset {offset}")


def test_more_than_three_sweeps_of_the_grid(ctx, big):
    a, dev = big
    n, s1, _ = check_moments(ctx, dev, a, 0.0, tag="big")
    check_moments(ctx, dev, a, s1 / n, tag="big")
    check_std(ctx, dev, a, tag="big")


def test_keep_over_several_sweeps(ctx, big):
    """The spaxel index is carried along the grid stride: checked where a lane makes several
    steps, with S odd."""
    a, dev = big
    yy, xx = np.indices(BIG_YX)
    keep = ((yy + xx) % 2).astype(np.uint8)
    check_moments(ctx, dev, a, 0.1, keep, tag="big checkerboard")
    check_std(ctx, dev, a, keep, tag="big checkerboard")


def test_mean_far_from_zero(ctx):
    """mean 1000, sigma 1: the two-pass form keeps its digits where sum x^2 - (sum x)^2 / n,
    taken in float64 from the same sums, has lost about six of them."""
    rng = np.random.default_rng(11)
    a = rng.normal(1000.0, 1.0, (31, 33, 35)).astype(np.float32)
    dev = ctx.to_device(a)
    check_moments(ctx, dev, a, 0.0, tag="mean 1000")
    got = check_std(ctx, dev, a, tag="mean 1000")
    assert 0.9 < got < 1.1


@pytest.mark.parametrize("shape", [(3, 5, 7), MEDIUM])
def test_keep_maps(ctx, shape):
    from origin_amd import kernels
    rng = np.random.default_rng(3)
    a = rng.normal(0.0, 1.0, shape).astype(np.float32)
    dev = ctx.to_device(a)
    yy, xx = np.indices(shape[1:])
    checker = ((yy + xx) % 2 == 0).astype(np.uint8)
    one = np.zeros(shape[1:], np.uint8)
    one[shape[1] - 1, shape[2] - 2] = 3           # any non-zero byte keeps
    none = np.zeros(shape[1:], np.uint8)
    for tag, keep in (("checkerboard", checker), ("one spaxel", one)):
        check_moments(ctx, dev, a, 0.2, keep, tag=tag)
        check_std(ctx, dev, a, keep, tag=tag)
    k = ctx.to_device(none.reshape(-1))
    assert kernels.cube_moments(ctx, dev, 0.2, k) == (0.0, 0.0, 0.0)
    assert np.isnan(kernels.cube_std(ctx, dev, k))


def test_nan_propagates_like_numpy(ctx):
    from origin_amd import kernels
    rng = np.random.default_rng(4)
    a = rng.normal(0.0, 1.0, MEDIUM).astype(np.float32)
    a[7, 11, 13] = np.nan
    dev = ctx.to_device(a)
    n, s1, s2 = kernels.cube_moments(ctx, dev, 0.0)
    assert n == a.size and np.isnan(s1) and np.isnan(s2)
    assert np.isnan(kernels.cube_std(ctx, dev)) and np.isnan(np.std(a.astype(np.float64)))
    # in an excluded spaxel it is not part of the sums
    keep = np.ones(MEDIUM[1:], np.uint8)
    keep[11, 13] = 0
    check_moments(ctx, dev, a, 0.0, keep, tag="NaN excluded")
    check_std(ctx, dev, a, keep, tag="NaN excluded")


def test_two_calls_are_bit_identical(ctx, big):
    from origin_amd import kernels
    a, dev = big
    keep = ctx.to_device((np.arange(BIG_YX[0] * BIG_YX[1]) % 3 != 0).astype(np.uint8))
    for k in (None, keep):
        first = kernels.cube_moments(ctx, dev, 0.2, k)
        again = kernels.cube_moments(ctx, dev, 0.2, k)
        assert np.array(first).tobytes() == np.array(again).tobytes()
    assert np.float64(kernels.cube_std(ctx, dev)).tobytes() == \
        np.float64(kernels.cube_std(ctx, dev)).tobytes()


def test_arguments_are_checked(ctx):
    from origin_amd import kernels
    with pytest.raises(TypeError):
        kernels.cube_moments(ctx, ctx.zeros((2, 2, 2), np.float64))
    with pytest.raises(ValueError):
        kernels.cube_moments(ctx, ctx.zeros((2, 2, 2), np.float32),
                             keep=ctx.zeros((3,), np.uint8))


def test_tiled_cube_std_on_two_contexts_of_one_card():
    """``TiledCube.std()`` over two contexts on one card: each rank reduces the spaxels it owns
    (an irregular border, windows that overlap, arrays larger than their windows and NaN outside
    them), the host adds the triples; equal to the one-context ``cube_std`` of the gathered cube.
    The other three reductions of the same cube, with and without a keep map, against NumPy."""
    from _cube_forms import tiled
    from origin_amd import catalog, kernels
    from origin_amd.session import DeviceGroup
    rng = np.random.default_rng(8)
    shape = (9, 10, 13)
    field = rng.normal(5.0, 2.0, shape).astype(np.float32)
    g = DeviceGroup([0, 0])
    try:
        cube = tiled(g, field)
        assert np.array_equal(cube.to_host(), field)
        ctx = g.ctxs[0]
        want = kernels.cube_std(ctx, cube.gathered(ctx))
        got = cube.std()
        ref = float(np.std(field.astype(np.float64)))
        print(f"TiledCube.std {got!r} one context {want!r} numpy {ref!r} "
              f"rel err {abs(got - want) / want:.3e} / {abs(got - ref) / ref:.3e}")
        assert abs(got - want) <= RTOL * want and abs(got - ref) <= RTOL * ref
        assert catalog.cube_std(ctx, cube) == got
        n, s1, s2 = cube.moments(0.5)
        rn, r1, r2, rabs = reference(field, 0.5)
        assert n == rn and abs(s1 - r1) <= RTOL * rabs and abs(s2 - r2) <= RTOL * r2
        f64 = field.astype(np.float64)
        yy, xx = np.indices(shape[1:])
        keep = (yy + 2 * xx) % 3 != 0
        thr = [5.0, 0.0, 7.5, -0.2, 1e9]
        for kp in (None, keep):
            kept = f64 if kp is None else f64 * kp
            assert np.array_equal(cube.zmax_map(kp), kept.max(axis=0))
            sel = f64 if kp is None else f64[:, kp]
            counts = [np.count_nonzero(sel > t) for t in thr]
            assert np.array_equal(cube.count_above(thr, kp), counts)
        aux = (np.arange(field.size) % 251).astype(np.uint8).reshape(shape)
        w = cube.where_above(9.0, aux=tiled(g, aux, outside=0))
        z, y, x = np.where(f64 > 9.0)
        assert z.size > 10
        for k, want in (("z", z), ("y", y), ("x", x), ("value", f64[z, y, x]),
                        ("aux", aux[z, y, x])):
            assert np.array_equal(w[k], want), k
    finally:
        g.close()
