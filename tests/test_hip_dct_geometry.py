"""GPU: section A of the C ABI (csrc/dct.hip: fit, continuum, channel sums, standardisation, the
continuum pass of its own, O2) against float64 NumPy at every launch geometry of the kernels.

Reference: ``cpu_ref.dct_fit_columns`` / ``cpu_ref.standardize_columns``, the vectorised float64
restatement of ``cpu_ref.dct_residual`` / ``cpu_ref.preprocessing`` that
``tests/test_host_logic.py::test_column_references_equal_the_per_spaxel_oracle`` pins to the
per-spaxel oracle and to the golden vectors.  The fit is independent per spaxel, so on the large
fields the reference runs on a SAMPLE of spaxels: the first and the last 64-spaxel group, the
lanes either side of 64-spaxel boundaries, every spaxel with a masked voxel, every group that holds
such a spaxel where the test is about the mask flag, and about 1000 random ones.  Fields of up to
4096 spaxels are checked whole.  Only in the cases at S = 512 x 513 is a share of the cube left
unchecked (about 99 % of the spaxels of the fit; the channel sums there are over the whole cube).

Shapes.  The moments kernel splits a group of 64 spaxels over ZS waves and the spectral axis over
nzc chunks of mirror pairs; both depend on S, Nz, the order and the CU count.  The shapes below are
sized for the MI355X's 256 CUs (num_cu * 16 = 4096 waves; ZS is capped at 4 for orders 6..12 by
the 64 KiB cross-wave area), and ``_geometry`` restates the host's choice only to aim masked
voxels at a given wave or chunk -- the geometry itself is never asserted, and on another chip the
same checks hold for whatever geometry that chip takes.

Tolerances.
  benign inputs (var in [1, 2], and the two-level variance of the mask-flag test):
    continuum, cube_std, cont_dct, images, o2: |d| <= 1e-5 * max(1, |x|)    
    coefficients: |d| <= 1e-5 * max |raw| of the column
    zsum: |d| <= 1e-6 * sum |raw| of the channel;  zcnt: exact
  hard inputs (sky-line variance, continuum 1e4 x noise): derived at run time from the reference
    alone.  Run A uses the exact float64 1 / var and 1 / sqrt(var); run B moves each of them by
    one float32 ulp in a random direction (the kernels take them from v_rcp_f32 / v_rsq_f32, 1 ulp
    each, on float32 variance).  Per output, tol = 4 * max(|A - B| / max(1, |A|)) + 2^-23 and
    the assertion is |device - A| <= tol * max(1, |A|); the 4 covers summation order, the 2^-23
    the float32 storage.  The test prints, per output, the reference sensitivity, the bound and
    the device error (run with -s).  Reference sensitivities (they do not depend on the device),
    coef / cont / cube_std / cont_dct / ima_std / ima_dct / o2:
      (530, 6, 11):   4.5e-8  8.8e-12  1.2e-7  2.3e-7  1.1e-7  1.2e-8  5.5e-8
      (21, 512, 513): 2.6e-7  3.6e-11  3.0e-7  2.3e-7  6.8e-7  7.2e-8  2.1e-7
"""
import numpy as np
import pytest

from oracle import cpu_ref

pytestmark = pytest.mark.gpu

BIG = (21, 512, 513)          # ZS = 1, S % 4 == 0 (512 x 513 = 64 x 4104: whole groups)
BIG_RAGGED = (21, 511, 515)   # ZS = 1, 4112 groups, S % 64 == 61, S % 4 == 1


@pytest.fixture(scope="module")
def hip():
    import origin_amd.lib_origin as lib
    return lib


@pytest.fixture(scope="module")
def ctx():
    from origin_amd.device import default_context
    return default_context(0)


# --------------------------------------------------------------------------------- helpers
def _cdiv(a, b):
    return -(-a // b)


def _geometry(Nz, S, order, num_cu=256):
    """(ZS, zchunk, nzc) as fit_plan (csrc/dct.hip) picks them on a chip of ``num_cu`` CUs: wave w of
    chunk c owns the mirror pairs p = c * zchunk + w + i * ZS, pair p = channels p and Nz - 1 - p."""
    waves = _cdiv(S, 64)
    ZS = 1
    while ZS < 8 and waves * ZS < num_cu * 16:
        ZS *= 2
    nacc = 3 * order + 2
    while ZS > 1 and (ZS - 1) * (nacc + 1) * 64 * 8 > 64 * 1024:
        ZS //= 2
    nzc = _cdiv(10 * num_cu * 16, waves * ZS)
    nzc = max(1, min(nzc, 16, Nz // 256))
    npair = max(1, Nz // 2)
    zchunk = _cdiv(_cdiv(npair, nzc), 8 * ZS) * 8 * ZS
    return ZS, zchunk, _cdiv(npair, zchunk)


def _scaled(got, ref):
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    assert got.shape == ref.shape
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    assert not np.isnan(err).any(), "NaN against a finite reference"
    return float(err.max()) if err.size else 0.0


def _assert_scaled(got, ref, tol, what):
    err = _scaled(got, ref)
    assert err <= tol, f"{what}: max scaled error {err:.3e} > {tol:.3e}"


def _benign(shape, seed, nmask=300, full_spaxel=True, full_channel=False):
    """(Nz, S) float32 raw / var and bool mask as ORIGIN.init leaves them (raw = 0, var = inf where
    masked): a ramp + noise, var in [1, 2], sparse masked voxels, a fully masked spaxel."""
    Nz, S = shape[0], shape[1] * shape[2]
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((Nz, S), dtype=np.float32) * 3 + 50
    raw += (10 * np.linspace(0, 1, Nz, dtype=np.float32))[:, None]
    var = 1 + rng.random((Nz, S), dtype=np.float32)
    mask = np.zeros((Nz, S), bool)
    n = min(nmask, 1 + Nz * S // 500)
    mask[rng.integers(0, Nz, n), rng.integers(0, S, n)] = True
    if full_spaxel and S > 2:
        mask[:, S // 2] = True
    if full_channel:
        mask[Nz // 3] = True
    raw[mask], var[mask] = 0, np.inf
    return raw, var, mask


def _sample(S, masked, rng, nrand=1000, groups=()):
    """Indices of the spaxels to check: all of a small field; of a large one both end groups, the
    lanes either side of a few 64-spaxel boundaries, every masked spaxel, whole ``groups`` and
    ``nrand`` random spaxels."""
    if S <= 4096:
        return np.arange(S)
    ng = _cdiv(S, 64)
    parts = [np.arange(64), np.arange((ng - 1) * 64, S), np.flatnonzero(masked),
             rng.integers(0, S, nrand)]
    for g in rng.integers(1, ng - 1, 6):
        parts.append(np.array([64 * g - 1, 64 * g, 64 * g + 63, 64 * g + 64]))
    for g in groups:
        parts.append(np.arange(64 * g, min(S, 64 * g + 64)))
    return np.unique(np.concatenate(parts))


def _upload(ctx, shape, raw, var, mask):
    return (ctx.to_device(raw.reshape(shape), np.float32), ctx.to_device(var.reshape(shape), np.float32),
            ctx.to_device(mask.reshape(shape).view(np.uint8)))


def _cos_table(Nz, order):
    return np.cos(((np.arange(Nz) + 0.5) * (np.pi / Nz))[:, None] * np.arange(order + 1))


def _check_fit(ctx, shape, order, approx, raw, var, mask, idx, dev=None, sums=True):
    """dct_fit and dct_fit_sums against the reference on the spaxels ``idx``: coefficients, the
    continuum kernel on the device's own coefficients (against NumPy's evaluation of the SAME
    coefficients, so that a failure names the kernel), the continuum against the reference, and
    the channel sums of the folded form against NumPy.  Returns the device's (coef, zsum, zcnt)."""
    from origin_amd import kernels
    Nz, S = raw.shape
    d_raw, d_var, d_mask = dev if dev is not None else _upload(ctx, shape, raw, var, mask)
    r64 = raw[:, idx].astype(np.float64)
    cont_ref, coef_ref = cpu_ref.dct_fit_columns(r64, var[:, idx].astype(np.float64), mask[:, idx],
                                                 order, approx)
    ctol = 1e-5 * np.abs(r64).max(axis=0)
    ctab = _cos_table(Nz, order)
    out = None
    for form in ("fit", "fit_sums"):
        if form == "fit":
            coef = kernels.dct_fit(ctx, d_raw, d_var, d_mask, order, approx)
        else:
            out = kernels.dct_fit_sums(ctx, d_raw, d_var, d_mask, order, approx)
            coef = out[0]
        c = coef.to_host().reshape(order + 1, S)[:, idx]
        assert np.isfinite(c).all(), f"{form}: non-finite coefficients"
        bad = np.abs(c - coef_ref) > ctol
        assert not bad.any(), (
            f"{form}: coefficients of spaxels {idx[bad.any(axis=0)][:8]} off by up to "
            f"{np.abs(c - coef_ref).max():.3e}")
        cont = kernels.dct_continuum(ctx, coef, Nz).to_host().reshape(Nz, S)
        _assert_scaled(cont[:, idx], ctab @ c, 1e-5, f"{form}: continuum kernel on its own input")
        _assert_scaled(cont[:, idx], cont_ref, 1e-5, f"{form}: continuum")
        if form == "fit_sums" and sums:
            _check_sums(out[1], out[2], raw, mask, cont, "fit_sums")
    return out


def _check_sums(zsum, zcnt, raw, mask, cont, what):
    """zsum / zcnt against NumPy: sum over the unmasked spaxels of raw - cont (the device's own
    float32 continuum, whole cube), within 1e-6 of sum |raw|; counts exact."""
    ref = np.where(mask, 0.0, raw.astype(np.float64) - cont).sum(axis=1)
    scale = np.abs(raw).sum(axis=1, dtype=np.float64) + 1.0
    err = np.max(np.abs(zsum.to_host() - ref) / scale)
    assert err <= 1e-6, f"{what}: zsum off by {err:.3e} of sum|raw|"
    assert np.array_equal(zcnt.to_host(), (~mask).sum(axis=1).astype(float)), f"{what}: zcnt"


# ------------------------------------------------------------- 2. the fit at every geometry
FIT_CASES = [
    # ZS = 8 (fewer than 1024 waves, order <= 5); order 5: the largest LDS use with the fold
    ((45, 7, 19), 3, False), ((45, 7, 19), 3, True), ((64, 9, 33), 5, False),
    # ZS = 4 by the LDS cap
    ((37, 5, 13), 10, False), ((29, 6, 11), 12, False),
    # ZS = 4 by wave count, ZS = 2, ZS = 1 (512 x 513 is a whole number of 64-spaxel groups: the
    # ragged last group at ZS = 1 is 511 x 515's)
    ((21, 250, 281), 3, False), ((21, 400, 401), 10, False),
    (BIG, 10, False), (BIG, 10, True), ((22, 512, 513), 4, False), (BIG_RAGGED, 10, False),
    # several chunks: whole trips; odd Nz (middle channel on the last chunk's first wave); a
    # partial last trip
    ((512, 5, 13), 10, False), ((513, 5, 13), 10, False), ((513, 5, 13), 10, True),
    ((513, 9, 70), 3, False), ((530, 6, 11), 10, False),
    # minimal Nz
    ((2, 3, 5), 1, False), ((3, 4, 4), 2, False), ((13, 3, 5), 12, False), ((13, 3, 5), 12, True),
]


@pytest.mark.parametrize("shape,order,approx", FIT_CASES)
def test_fit_matches_float64_reference(ctx, shape, order, approx):
    """origin_dct_fit, origin_dct_fit_sums and origin_dct_continuum against the float64 reference
    (module docstring: sample, tolerances), masked and clean spaxels, at one launch geometry."""
    raw, var, mask = _benign(shape, seed=shape[0] * 1000 + shape[2] + order)
    rng = np.random.default_rng(7)
    idx = _sample(raw.shape[1], mask.any(axis=0), rng)
    _check_fit(ctx, shape, order, approx, raw, var, mask, idx)


def test_fit_one_wave_per_group_and_several_chunks(ctx):
    """ZS = 1 with nzc >= 2: (512, 512, 513), order 10.  The cube is a 64-spaxel random block
    repeated along the field plus an offset per spaxel (cheap to make on the host); masked voxels
    sit in the first and in a later chunk.  The continuum kernel runs on the sampled coefficients
    only, as a (1, n) field, and the channel sums are not compared (both are covered at
    (21, 512, 513)); about 99.5 % of the spaxels are not checked."""
    from origin_amd import kernels
    shape, order = (512, 512, 513), 10
    Nz, S = shape[0], shape[1] * shape[2]
    rng = np.random.default_rng(11)
    ng = _cdiv(S, 64)
    block = rng.standard_normal((Nz, 64), dtype=np.float32) * 3
    block += (10 * np.linspace(0, 1, Nz, dtype=np.float32))[:, None]
    raw = np.ascontiguousarray(np.tile(block, (1, ng))[:, :S])
    raw += (40 + 20 * rng.random(S, dtype=np.float32))[None, :]
    var = np.ascontiguousarray(np.tile(1 + rng.random((Nz, 64), dtype=np.float32), (1, ng))[:, :S])
    mask = np.zeros((Nz, S), bool)
    _, zchunk, nzc = _geometry(Nz, S, order)
    for z, s in ((0, 0), (Nz - 1, S - 1), (zchunk + 3, 64 * 7 + 5), (Nz - 1 - (zchunk + 9), 64 * 1000),
                 (Nz // 2 - 1, 64 * 2000 + 63), (Nz // 2, 64 * 3000 + 1), (17, S - 64)):
        mask[z, s] = True
    mask[:, 64 * 1234 + 9] = True
    zz, ss = np.nonzero(mask)
    raw[zz, ss], var[zz, ss] = 0, np.inf
    masked = mask.any(axis=0)
    idx = _sample(S, masked, rng, groups=np.flatnonzero(masked) // 64)
    dev = _upload(ctx, shape, raw, var, mask)
    r64 = raw[:, idx].astype(np.float64)
    cont_ref, coef_ref = cpu_ref.dct_fit_columns(r64, var[:, idx].astype(np.float64), mask[:, idx],
                                                 order)
    ctol = 1e-5 * np.abs(r64).max(axis=0)
    for form in ("fit", "fit_sums"):
        fn = kernels.dct_fit if form == "fit" else kernels.dct_fit_sums
        res = fn(ctx, *dev, order, False)
        coef = res if form == "fit" else res[0]
        c = np.ascontiguousarray(coef.to_host().reshape(order + 1, S)[:, idx])
        bad = np.abs(c - coef_ref) > ctol
        assert not bad.any(), f"{form}: coefficients of spaxels {idx[bad.any(axis=0)][:8]}"
        if form == "fit_sums":
            assert np.array_equal(res[2].to_host(), (~mask).sum(axis=1).astype(float))
        del res, coef
    d_c = ctx.to_device(c.reshape(order + 1, 1, len(idx)), np.float64)
    cont = kernels.dct_continuum(ctx, d_c, Nz).to_host().reshape(Nz, len(idx))
    _assert_scaled(cont, cont_ref, 1e-5, "continuum")


# ------------------------------------------------------ 2b. every order reaches its own kernels
ORDERS_SHAPE = (13, 3, 5)


@pytest.fixture(scope="module")
def small_cube(ctx):
    raw, var, mask = _benign(ORDERS_SHAPE, seed=14)  # (a masked voxel outside the masked spaxel)
    return raw, var, mask, _upload(ctx, ORDERS_SHAPE, raw, var, mask)


def _check_order(ctx, small_cube, order):
    """dct_fit_sums, dct_continuum and the five outputs of dct_standardize at ``order`` on the whole
    (13, 3, 5) field against the float64 reference, benign tolerances of the module docstring."""
    from origin_amd import kernels
    raw, var, mask, dev = small_cube
    Nz, S = raw.shape
    r64, v64 = raw.astype(np.float64), var.astype(np.float64)
    cont_ref, coef_ref = cpu_ref.dct_fit_columns(r64, v64, mask, order)
    assert coef_ref.shape == (order + 1, S)
    coef, zsum, zcnt = kernels.dct_fit_sums(ctx, *dev, order)
    c = coef.to_host().reshape(order + 1, S)
    assert np.all(np.abs(c - coef_ref) <= 1e-5 * np.abs(r64).max(axis=0)), (
        f"order {order}: coefficients off by up to {np.abs(c - coef_ref).max():.3e}")
    cont = kernels.dct_continuum(ctx, coef, Nz).to_host().reshape(Nz, S)
    _assert_scaled(cont, cont_ref, 1e-5, f"order {order}: continuum")
    _check_sums(zsum, zcnt, raw, mask, cont, f"order {order}: fit_sums")
    std = kernels.dct_standardize(ctx, *dev, coef, zsum, zcnt)
    with np.errstate(invalid="ignore", divide="ignore"):
        zmean = zsum.to_host() / zcnt.to_host()
    ref = cpu_ref.standardize_columns(r64, v64, mask, cont_ref, zmean)
    for k in STD_KEYS:
        _assert_scaled(std[k].to_host().reshape(ref[k].shape), ref[k], 1e-5, f"order {order}: {k}")


@pytest.mark.parametrize("order", range(1, 13))
def test_every_order_runs_its_own_instantiation(ctx, small_cube, order):
    """The run-time order selects the kernels' ORDER template parameter (with_order, csrc/dct.hip).
    The coefficient array has order + 1 rows, so a dispatch that lands on a neighbouring
    instantiation gives another continuum, not a rounding difference."""
    _check_order(ctx, small_cube, order)


def test_unsupported_orders_raise_and_a_valid_call_still_works(ctx, small_cube):
    """Order 0, order 13 and order 12 on 12 channels are refused by origin_dct_fit,
    origin_dct_continuum and origin_dct_standardize; the next valid call gives the right answer."""
    from origin_amd import _capi, kernels
    Ny, Nx = ORDERS_SHAPE[1:]
    for order, Nz in ((0, 13), (13, 13), (12, 12)):
        raw, var = ctx.zeros((Nz, Ny, Nx), np.float32), ctx.zeros((Nz, Ny, Nx), np.float32)
        mask = ctx.zeros((Nz, Ny, Nx), np.uint8)
        coef = ctx.zeros((order + 1, Ny, Nx), np.float64)
        zsum, zcnt = ctx.zeros((Nz,), np.float64), ctx.zeros((Nz,), np.float64)
        for call in (lambda: kernels.dct_fit(ctx, raw, var, mask, order),
                     lambda: kernels.dct_continuum(ctx, coef, Nz),
                     lambda: kernels.dct_standardize(ctx, raw, var, mask, coef, zsum, zcnt)):
            with pytest.raises(_capi.OriginHipError) as e:
                call()
            assert e.value.code == -1 and "order" in str(e.value), (order, Nz)
    _check_order(ctx, small_cube, 10)


# ------------------------------------------------------------------ 3. mask-flag placement
@pytest.mark.parametrize("shape,order", [((530, 6, 11), 10), ((513, 5, 13), 10), (BIG_RAGGED, 10)])
def test_single_masked_voxel_selects_the_plain_fit(ctx, shape, order):
    """One masked voxel in an otherwise clean spaxel, at every place the any-mask flag is taken
    from: channel 0, channel Nz - 1, the middle channel of an odd Nz, a channel of a wave other
    than 0 and one of a chunk other than 0 (where the geometry has them: ZS > 1 with two chunks
    at (530, 6, 11), odd Nz with two chunks at (513, 5, 13), ZS = 1 at (21, 511, 515)), the last
    live lane of the last group (S % 64 != 0), lane 0 of group 0.  The variance of every spaxel
    is 100 times larger in the second half of the spectrum, so that the weighted and the plain fit
    differ far beyond the tolerance (asserted on the reference): the masked spaxel must match the
    plain fit, its unmasked neighbours of the same group the weighted one."""
    Nz, S = shape[0], shape[1] * shape[2]
    assert S % 64 != 0
    rng = np.random.default_rng(Nz + S)
    var = 1 + rng.random((Nz, S), dtype=np.float32)
    var[Nz // 2:] *= 100
    raw = rng.standard_normal((Nz, S), dtype=np.float32) * 3 * np.sqrt(var) + 50
    raw += (10 * np.linspace(0, 1, Nz, dtype=np.float32))[:, None]
    ZS, zchunk, nzc = _geometry(Nz, S, order)
    ng = _cdiv(S, 64)
    chans = {"first": 0, "last": Nz - 1, "near the middle": Nz // 2 - 1}
    if Nz & 1:
        chans["middle"] = Nz // 2
    if ZS > 1:
        chans["front, last wave"] = ZS - 1
        chans["back, wave 1"] = Nz - 2
    if nzc > 1:
        chans["front, chunk 1"] = zchunk + (1 if ZS > 1 else 0)
        chans["back, last chunk"] = Nz - 1 - ((nzc - 1) * zchunk + ZS - 1)
    # spaxels: spread over the lanes of group 0, of a middle group and of the last group
    free = [s for s in (5, 17, 38, 62, 63, 64 * (ng // 2) + 31, 64 * (ng // 2) + 1, 64 * (ng - 1),
                        64 * (ng // 2) + 63, 64 * (ng // 2) + 12, 1, 33, 2) if 0 < s < S - 1]
    free = list(dict.fromkeys(free))
    assert len(free) >= len(chans)
    mask = np.zeros((Nz, S), bool)
    for (name, z), s in zip(chans.items(), free):
        mask[z, s] = True
    mask[1 % Nz, 0] = True                      # lane 0 of group 0
    mask[Nz - 2, S - 1] = True                  # the last live lane of the last group
    raw[mask], var[mask] = 0, np.inf
    masked = np.flatnonzero(mask.any(axis=0))
    assert len(masked) == len(chans) + 2 and np.all(mask[:, masked].sum(axis=0) == 1)
    # premise: on the masked spaxels the two fits differ by >= 100 x the tolerance
    r64, v64 = raw[:, masked].astype(np.float64), var[:, masked].astype(np.float64)
    plain, _ = cpu_ref.dct_fit_columns(r64, v64, mask[:, masked], order)
    weighted, _ = cpu_ref.dct_fit_columns(r64, v64, np.zeros_like(mask[:, masked]), order)
    gap = np.max(np.abs(plain - weighted) / np.maximum(1.0, np.abs(plain)), axis=0)
    assert gap.min() >= 100 * 1e-5, f"fits differ by only {gap.min():.2e}"
    idx = _sample(S, mask.any(axis=0), rng, groups=np.unique(masked // 64))
    _check_fit(ctx, shape, order, False, raw, var, mask, idx)


# -------------------------------------------- 4. standardisation, continuum pass, O2
STD_CASES = [((2, 3, 5), 1), ((13, 3, 5), 10), ((37, 5, 13), 10), ((96, 10, 13), 10),
             ((129, 17, 15), 10), ((130, 1, 257), 10), ((131, 257, 1), 10), ((40, 4, 16), 10),
             (BIG, 10)]
STD_KEYS = ("cube_std", "cont_dct", "ima_std", "ima_dct", "o2")


@pytest.mark.parametrize("shape,order", STD_CASES)
def test_standardize_all_outputs_and_call_forms(ctx, shape, order):
    """origin_dct_resid_sums (both code paths: S % 4 == 0 and not), origin_dct_standardize's five
    outputs against the reference given the device's zsum / zcnt, its NULL-able outputs, and
    origin_dct_cont_std / _async against it bit for bit.  Sparse masked voxels, a fully masked
    spaxel and a fully masked channel (whose mean does not exist: every voxel of it is masked,
    cube_std is 0 there)."""
    from origin_amd import kernels
    Nz, S = shape[0], shape[1] * shape[2]
    raw, var, mask = _benign(shape, seed=Nz + 31 * S, full_channel=True)
    rng = np.random.default_rng(S)
    few = np.flatnonzero(mask.sum(axis=0) > 1)      # masked beyond the fully masked channel
    idx = _sample(S, np.isin(np.arange(S), few), rng)
    dev = _upload(ctx, shape, raw, var, mask)
    coef, zsum, zcnt = _check_fit(ctx, shape, order, False, raw, var, mask, idx, dev=dev)
    cont = kernels.dct_continuum(ctx, coef, Nz).to_host().reshape(Nz, S)
    s1, n1 = kernels.dct_resid_sums(ctx, dev[0], dev[2], coef)
    _check_sums(s1, n1, raw, mask, cont, "resid_sums")

    # all five outputs, every optional pointer given
    full = kernels.dct_standardize(ctx, *dev, coef, zsum, zcnt)
    got = {k: full[k].to_host() for k in STD_KEYS}
    with np.errstate(invalid="ignore", divide="ignore"):
        zmean = zsum.to_host() / zcnt.to_host()
    r64, v64 = raw[:, idx].astype(np.float64), var[:, idx].astype(np.float64)
    cont_ref, _ = cpu_ref.dct_fit_columns(r64, v64, mask[:, idx], order)
    ref = cpu_ref.standardize_columns(r64, v64, mask[:, idx], cont_ref, zmean)
    for k in STD_KEYS:
        g = got[k].reshape(-1, S)[:, idx].reshape(ref[k].shape)
        _assert_scaled(g, ref[k], 1e-5, k)
    assert np.all(got["cube_std"].reshape(Nz, S)[mask] == 0)
    # cont_dct NULL; only o2 given: what is present is the same bits
    no_cont = kernels.dct_standardize(ctx, *dev, coef, zsum, zcnt, want_cont=False)
    assert no_cont["cont_dct"] is None and no_cont["ima_dct"] is None
    only_o2 = kernels.dct_standardize(ctx, *dev, coef, zsum, zcnt, want_cont=False,
                                      want_images=False, o2=ctx.empty(shape[1:], np.float64))
    assert only_o2["ima_std"] is None and only_o2["ima_dct"] is None
    for form, keys in ((no_cont, ("cube_std", "ima_std", "o2")), (only_o2, ("cube_std", "o2"))):
        for k in keys:
            assert np.array_equal(form[k].to_host(), got[k], equal_nan=True), k
    # the continuum pass of its own, on the main and on the auxiliary stream
    for aux in (False, True):
        for want_image in (True, False):
            o = kernels.dct_cont_std(ctx, dev[1], coef, want_image=want_image, aux=aux)
            if aux:
                ctx.aux_join()
            ctx.sync()
            assert np.array_equal(o["cont_dct"].to_host(), got["cont_dct"], equal_nan=True)
            if want_image:
                assert np.array_equal(o["ima_dct"].to_host(), got["ima_dct"], equal_nan=True)
            else:
                assert o["ima_dct"] is None


def test_cosine_table_is_replaced_only_after_the_auxiliary_pass(ctx):
    """Two cubes in a session: an auxiliary-stream continuum pass at (Nz, order), then the fit of a
    cube of another Nz, then one of another order -- each replaces the cached cosine table the
    auxiliary pass reads -- and only then the auxiliary pass's output is read.  All three must
    match the reference."""
    from origin_amd import kernels
    shape, order = (131, 60, 257), 10
    Nz, S = shape[0], shape[1] * shape[2]
    raw, var, mask = _benign(shape, seed=5)
    rng = np.random.default_rng(6)
    idx = _sample(S, mask.any(axis=0), rng)
    dev = _upload(ctx, shape, raw, var, mask)
    coef = kernels.dct_fit(ctx, *dev, order)
    others = []
    for shp, o in (((45, 7, 19), order), ((45, 7, 19), 3)):
        r, v, m = _benign(shp, seed=shp[0] + o)
        others.append((shp, o, r, v, m, _upload(ctx, shp, r, v, m)))
    ctx.sync()
    pas = kernels.dct_cont_std(ctx, dev[1], coef, aux=True)
    fits = [kernels.dct_fit(ctx, *d, o) for (_, o, _, _, _, d) in others]
    ctx.aux_join()
    ctx.sync()
    r64, v64 = raw[:, idx].astype(np.float64), var[:, idx].astype(np.float64)
    cont_ref, _ = cpu_ref.dct_fit_columns(r64, v64, mask[:, idx], order)
    ref = cpu_ref.standardize_columns(r64, v64, mask[:, idx], cont_ref, np.zeros(Nz))
    _assert_scaled(pas["cont_dct"].to_host().reshape(Nz, S)[:, idx], ref["cont_dct"], 1e-5, "cont_dct")
    _assert_scaled(pas["ima_dct"].to_host().reshape(S)[idx], ref["ima_dct"], 1e-5, "ima_dct")
    for (shp, o, r, v, m, _), c in zip(others, fits):
        _, coef_ref = cpu_ref.dct_fit_columns(r.astype(np.float64), v.astype(np.float64), m, o)
        got = c.to_host().reshape(o + 1, -1)
        assert np.all(np.abs(got - coef_ref) <= 1e-5 * np.abs(r).max(axis=0)), (shp, o)


@pytest.mark.parametrize("Nz", [1, 2, 63, 64, 65])
def test_o2_ragged_shapes(hip, Nz):
    rng = np.random.default_rng(Nz)
    for S in (1, 255, 256, 257):
        x = (rng.standard_normal((Nz, S)) * 10.0 ** rng.integers(-3, 4, (1, S))).astype(np.float32)
        got = hip.O2test(x)
        assert got.shape == (S,) and got.dtype == np.float64
        np.testing.assert_allclose(got, np.mean(x.astype(float) ** 2, 0), rtol=1e-12)


# --------------------------------------------------------------------------- 5. hard inputs
def _hard(shape, seed):
    """Sky-line variance (5 % of the channels carry 1e3..1e4 times the variance), an overall scale
    per spaxel in [0.1, 10], noise of that variance on a continuum 1e4 times the noise; sparse
    masked voxels and a fully masked spaxel."""
    Nz, S = shape[0], shape[1] * shape[2]
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-1, 1, S)
    lines = np.ones(Nz)
    nl = max(1, round(0.05 * Nz))
    lines[rng.choice(Nz, nl, replace=False)] = 10.0 ** rng.uniform(3, 4, nl)
    var = ((1 + rng.random((Nz, S))) * scale[None, :] * lines[:, None]).astype(np.float32)
    z = (np.arange(Nz) + 0.5) / Nz
    cont = 1e4 * np.sqrt(scale)[None, :] * (1 + 0.2 * np.cos(np.pi * z) + 0.05 * np.cos(3 * np.pi * z))[:, None]
    raw = (cont + rng.standard_normal((Nz, S)) * np.sqrt(var)).astype(np.float32)
    mask = np.zeros((Nz, S), bool)
    n = min(300, 1 + Nz * S // 500)
    mask[rng.integers(0, Nz, n), rng.integers(0, S, n)] = True
    mask[:, S // 2] = True
    raw[mask], var[mask] = 0, np.inf
    return raw, var, mask


def _one_f32_ulp(x, rng):
    """x (float64) moved by one ulp of its float32 value, up or down at random."""
    with np.errstate(invalid="ignore"):
        ulp = np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
    return np.where(np.isfinite(ulp), x + ulp * rng.choice([-1.0, 1.0], x.shape), x)


@pytest.mark.parametrize("shape,order", [((530, 6, 11), 10), (BIG, 10)])
def test_hard_inputs_within_the_references_own_sensitivity(ctx, shape, order):
    """Fit, continuum and standardisation on sky-line variance and a continuum 1e4 times the noise
    (the cancellation in ((double) r - cont) - mean), ZS > 1 and ZS = 1 (sampled).  The bound per
    output is derived here from the reference alone (module docstring); every output is finite
    and cube_std is exactly 0 on masked voxels."""
    from origin_amd import kernels
    Nz, S = shape[0], shape[1] * shape[2]
    raw, var, mask = _hard(shape, seed=Nz + S)
    rng = np.random.default_rng(S + 1)
    idx = _sample(S, mask.any(axis=0), rng)
    dev = _upload(ctx, shape, raw, var, mask)
    coef, zsum, zcnt = kernels.dct_fit_sums(ctx, *dev, order)
    cont = kernels.dct_continuum(ctx, coef, Nz)
    std = kernels.dct_standardize(ctx, *dev, coef, zsum, zcnt)
    got = {k: std[k].to_host().reshape(-1, S) for k in STD_KEYS}
    got["coef"] = coef.to_host().reshape(order + 1, S)
    got["cont"] = cont.to_host().reshape(Nz, S)
    zs, zc = zsum.to_host(), zcnt.to_host()
    assert np.all(zc == (~mask).sum(axis=1)) and np.all(zc > 0)
    for k, g in got.items():
        assert np.isfinite(g).all(), f"{k}: not finite"
    assert np.isfinite(zs).all()
    assert np.all(got["cube_std"][mask] == 0)
    _check_sums(zsum, zcnt, raw, mask, got["cont"], "fit_sums")
    # reference A (exact weights) and B (each weight one float32 ulp away)
    r64, v64, m = raw[:, idx].astype(np.float64), var[:, idx].astype(np.float64), mask[:, idx]
    zmean = zs / zc
    w, rs = 1.0 / v64, 1.0 / np.sqrt(v64)
    runs = []
    for wi, ri in ((w, rs), (_one_f32_ulp(w, rng), _one_f32_ulp(rs, rng))):
        c, y = cpu_ref.dct_fit_columns(r64, v64, m, order, weights=wi)
        o = cpu_ref.standardize_columns(r64, v64, m, c, zmean, inv_std=ri)
        o.update(coef=y, cont=c)
        runs.append(o)
    A, B = runs
    failed = []
    for k in ("coef", "cont") + STD_KEYS:
        sens = _scaled(B[k], A[k])
        tol = 4 * sens + 2.0 ** -23
        err = _scaled(got[k][:, idx].reshape(A[k].shape), A[k])
        print(f"hard {shape} {k:9s} reference sensitivity {sens:.3e}  bound {tol:.3e}  "
              f"device error {err:.3e}")
        if not err <= tol:
            failed.append(f"{k}: {err:.3e} > {tol:.3e}")
    assert not failed, "; ".join(failed)
