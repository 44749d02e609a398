"""The fp32 FMA kernels of the GLR (csrc/glr_fp32.hip) against the float64 oracle, at every
spectral form, window template and z chunking, and the spatial stage's z-march.

These kernels run for plans made with precision="f32", dictionaries of more than 26 profiles,
half widths above 32, fields smaller than the PSF, PSF sizes the matrix cores do not take, weighted
plans the matrix-core norm forms do not serve, and the norm cube of every weighted plan.  Every
GPU test here first asserts, through ``GLRPlan.paths()`` and tests/_glr_fp32_geometry.py, the
kernel form, the window template and the chunk counts it was written for (conditions on the
inputs, for the device at hand), then compares.

Inputs.  Cube: float32-representable standard normal noise with one +40 spike (on the first
channel of the second z chunk).  PSF: ``synth.moffat_psf`` times 1 + 0.3 * random, renormalised
per channel (asymmetric in x and y).  Mask: 3 % random voxels, row y = 0 at every channel, one
whole interior spaxel.  Dictionaries: ``build_dictionary`` (every tap >= 0.1 of the largest, so a
dropped or shifted edge tap shows at the tolerance), used with pcut=None, pmeansub=False.
Weighted fields: two float32-representable weight maps, PSFs of different FWHM, the second field
zero for x < 8, both zero on the 4 x 4 corner at the high end of y and x -- the spaxels whose
whole PSF window lies there have den <= 0 and T exactly 0, profile 0 (reference
lib_origin.py:1057).

Oracle: ``cpu_ref.Correlation_GLR_test_direct`` on the float64 copies (the spatial cases, 5 M
voxels each: the FFT form ``cpu_ref.Correlation_GLR_test``; with a PSF wider than 7 no spaxel is
uncovered, so its den is nowhere rounding noise); mask glue and maps as ``cpu_ref.compute_TGLR``
has them (correl[mask] = 0, profile[mask] = 0, maxmap = max_z correl, minmap = min_z correl_min).
The per-profile T_k come from one oracle run per profile.

Criteria (header of tests/test_hip_parity.py):
  correl, correl_min: max |d| <= 1e-4
  maxmap, minmap:     max |d| <= 1e-4, over all spaxels and again over the border spaxels alone
  profile:            mismatching voxels <= 1e-4 of all; at each of them the oracle's T of the
                      device's choice is within 2e-4 of the oracle's maximum (two values that are
                      each within 1e-4 cannot be told apart beyond that; this implies that the
                      oracle's two largest T_k differ by at most 2e-4 there)
  exact:              correl == 0 and profile == 0 on the mask, correl_min unmasked there;
                      correl, correl_min and profile exactly 0 on the uncovered spaxels
Input condition for the profile cap (CPU test): the share of voxels whose oracle top-two gap is
below 1e-5 is at most 1e-4 (the uncovered spaxels, where every T_k is exactly 0 and the first
profile wins by rule, are checked exactly instead and do not count).
"""
import functools

import numpy as np
import pytest

import _glr_fp32_geometry as geo
from oracle import cpu_ref
from origin_amd import synth

gpu = pytest.mark.gpu

P_SPEC = 7
TOL = 1e-4

# id: (half widths, Nz, lwt, LWMAX of spectral_kernel (0: generic), (nzc, zchunk, last), border slices)
FAMILIES = {
    "t8": ((0, 1, 3, 8, 5), 301, 8, 8, (4, 76, 73), 8),
    "t16": ((2, 9, 16, 12), 301, 16, 16, (2, 152, 149), 4),
    "t24": ((17, 24, 4, 20), 421, 24, 32, (2, 212, 209), 4),
    "t29": ((25, 29, 10), 501, 29, 32, (2, 252, 249), 4),
    "t32": ((30, 32, 31, 6), 541, 32, 32, (2, 272, 269), 4),
    "gen": ((40, 33, 5), 681, 0, 0, (2, 344, 337), None),
}
# field: (Ny, Nx, weighted, form of the families t*, form of gen)
FIELDS = {
    "even": (26, 30, False, "packed", None),
    "odd": (27, 31, False, "fp32", "generic"),
    "weighted": (26, 30, True, "fp32", "generic"),
}
SPECTRAL_CASES = [(f, fld) for f in FAMILIES for fld in FIELDS
                  if not (f == "gen" and fld == "even")]
K27 = ("k27", "even")
K27_LWS = tuple(1 + i % 9 for i in range(27))
K27_NZ = 160

# (P, Ny, Nx, weighted, kernel): the spatial stage with one one-tap profile
SPATIAL_CASES = [
    (7, 70, 70, False, "spatial4x4<7, false, false>"),
    (9, 70, 70, False, "spatial4x4<9, false, false>"),
    (25, 70, 70, False, "spatial4x4<25, false, false>"),
    (9, 70, 72, False, "spatial4x4<9, true, false>"),
    (25, 70, 72, False, "spatial4x4<25, true, false>"),
    (9, 70, 72, True, "spatial4x4<9, true, true> + spatial_kernel(A = NULL)"),
    (11, 70, 70, False, "spatial_kernel"),
]


def _seed(*key):
    return sum((i + 1) * sum(map(ord, str(k))) for i, k in enumerate(key))


# ------------------------------------------------------------------------------ inputs
def make_psf(Nz, P, rng, fwhm0=3.6, fwhm1=3.0):
    psf = synth.moffat_psf(Nz, P, fwhm0=fwhm0, fwhm1=fwhm1).astype(np.float64)
    psf *= 1.0 + 0.3 * rng.random(psf.shape)
    return psf / psf.sum(axis=(1, 2), keepdims=True)


def make_weights(Ny, Nx):
    w0 = (0.2 + 0.6 * np.linspace(0, 1, Ny)[:, None] * np.ones((1, Nx))).astype(np.float32)
    w1 = (1.0 - w0).astype(np.float32)
    w1[:, :8] = 0.0
    w0[-4:, -4:] = 0.0
    w1[-4:, -4:] = 0.0
    return [w0.astype(np.float64), w1.astype(np.float64)]


def uncovered_spaxels(weights, P):
    """Spaxels whose whole PSF window (clipped by the field) has zero weight in every field."""
    Ny, Nx = weights[0].shape
    c = P // 2
    cov = np.zeros((Ny + 2 * c, Nx + 2 * c))
    cov[c:c + Ny, c:c + Nx] = sum(weights) > 0
    tot = np.zeros((Ny, Nx))
    for dy in range(P):
        for dx in range(P):
            tot += cov[dy:dy + Ny, dx:dx + Nx]
    return tot == 0


def border_spaxels(Ny, Nx, P):
    c = P // 2
    b = np.ones((Ny, Nx), bool)
    b[c:Ny - c, c:Nx - c] = False
    return b


def make_inputs(Nz, Ny, Nx, P, weighted, spike_z, seed):
    rng = np.random.default_rng(seed)
    cube = rng.standard_normal((Nz, Ny, Nx), dtype=np.float32)
    spike = (spike_z, Ny // 2, Nx // 2 + 1)
    cube[spike] += np.float32(40.0)
    mask = rng.random((Nz, Ny, Nx)) < 0.03
    mask[:, 0, :] = True
    mask[:, Ny // 3, Nx // 3] = True
    mask[spike] = False
    if weighted:
        psf = [make_psf(Nz, P, rng), make_psf(Nz, P, rng, fwhm0=2.7, fwhm1=3.4)]
        weights = make_weights(Ny, Nx)
        uncovered = uncovered_spaxels(weights, P)     # (none for P > 7: the corner is 4 x 4)
        assert uncovered.any() == (P <= 7) and not uncovered[0].any()
    else:
        psf, weights, uncovered = make_psf(Nz, P, rng), None, np.zeros((Ny, Nx), bool)
    return dict(shape=(Nz, Ny, Nx), P=P, cube=cube, mask=mask, psf=psf, weights=weights,
                uncovered=uncovered, border=border_spaxels(Ny, Nx, P))


def spectral_inputs(family, field):
    if (family, field) == K27:
        lws, Nz = K27_LWS, K27_NZ
    else:
        lws, Nz = FAMILIES[family][:2]
    Ny, Nx, weighted = FIELDS[field][:3]
    zchunk = geo.spectral_chunks(256, Ny * Nx, Nz, max(lws))[1]
    inp = make_inputs(Nz, Ny, Nx, P_SPEC, weighted, zchunk, _seed(family, field))
    inp["profiles"] = geo.build_dictionary(lws, _seed(family))
    return inp


def oracle(inp, fft=False):
    """correl (mask glue applied), profile, correl_min, maps, and the per-profile T_k."""
    cube = inp["cube"].astype(np.float64)
    run = cpu_ref.Correlation_GLR_test if fft else cpu_ref.Correlation_GLR_test_direct
    kw = dict(pcut=None, pmeansub=False)
    profs = inp["profiles"]
    correl, profile, cmin = run(cube, inp["psf"], inp["weights"], profs, **kw)
    if len(profs) == 1:
        Tk = correl[None].copy()
    else:
        Tk = np.stack([run(cube, inp["psf"], inp["weights"], [p], **kw)[0] for p in profs])
    correl[inp["mask"]] = 0          # compute_TGLR (steps.py:781)
    profile[inp["mask"]] = 0         # (steps.py:788)
    return dict(correl=correl, profile=profile, correl_min=cmin, maxmap=correl.max(axis=0),
                minmap=cmin.min(axis=0), Tk=Tk)


@functools.lru_cache(maxsize=None)
def spectral_case(family, field):
    """Inputs and oracle of a spectral case: computed once, shared by the CPU condition test and
    the GPU test, never modified."""
    inp = spectral_inputs(family, field)
    return inp, oracle(inp)


def close_gap_share(inp, ref, gap):
    """Share of voxels (uncovered spaxels aside) whose oracle top-two gap is below ``gap``."""
    top2 = np.sort(ref["Tk"], axis=0)[-2:]
    d = (top2[1] - top2[0])[:, ~inp["uncovered"]]
    return float(np.mean(d < gap))


# ------------------------------------------------------------------------------ CPU tests
def test_geometry_of_the_cases_on_256_cus():
    """The helper's restatement gives, for the families and fields above on 256 CUs, the chunking
    each case was designed for; on fields this small the Nz cap binds, whatever the CU count."""
    nb = geo.nborder_of(26, 30, P_SPEC)
    assert nb == 300
    for fam, (lws, Nz, lwt, tmpl, chunks, slices) in FAMILIES.items():
        lwmax = max(lws)
        assert geo.lwt_of(lwmax) == lwt and geo.lwmax_template(lwmax) == tmpl, fam
        for Ny, Nx in ((26, 30), (27, 31)):
            for cu in (256, 64, 304):
                assert geo.spectral_chunks(cu, Ny * Nx, Nz, lwmax) == chunks, (fam, Ny, Nx, cu)
        assert chunks[0] >= 2 and chunks[2] % geo.SPEC_ZC != 0 and chunks[1] % geo.SPEC_ZC == 0
        if slices is not None:
            assert geo.border_slices(256, nb, Nz, lwmax)[0] == slices, fam
    assert geo.spectral_chunks(256, 26 * 30, K27_NZ, max(K27_LWS)) == (2, 80, 80)
    assert geo.border_slices(256, nb, K27_NZ, max(K27_LWS))[0] == 4
    # 390 packed lanes: a second block of spectral3_kernel that is partly dead
    assert 26 * 30 // 2 > 256 and 26 * 30 // 2 % 256 != 0
    assert geo.spatial_nz(256, 70, 70) == geo.spatial_nz(256, 70, 72) == 1031
    assert geo.spatial_march(256, 1031, 70, 70) == (2, 516, 1)
    # a cube of one chunk, as every fp32 run of the other test files has it
    assert geo.spectral_chunks(256, 27 * 31, 90, 29) == (1, 92, 90)
    # half widths: 0, 1, the template limits and values inside each range
    lws = {lw for f in FAMILIES.values() for lw in f[0]}
    assert {0, 1, 8, 16, 24, 29, 32} <= lws
    for lo, hi in ((1, 8), (8, 16), (16, 24), (24, 29), (29, 32), (32, 64)):
        assert any(lo < lw < hi for lw in lws), (lo, hi)


def test_dictionary_taps_are_all_visible():
    """Every tap of every profile is at least 0.1 of the profile's largest, and the profiles have
    exactly the lengths asked for."""
    for fam, lws in [(f, v[0]) for f, v in FAMILIES.items()] + [("k27", K27_LWS)]:
        profs = geo.build_dictionary(lws, _seed(fam))
        assert [len(p) for p in profs] == [2 * lw + 1 for lw in lws]
        r = geo.tap_ratio(profs)
        print(f"{fam}: smallest tap ratio {r:.3f}")
        assert r >= 0.1, (fam, r)
        for p in profs:
            if len(p) > 1:
                assert not np.array_equal(p, p[::-1])     # asymmetric
        prep = cpu_ref.prepare_profiles(profs, None, False)
        assert [len(p) for p in prep] == [len(p) for p in profs]    # untrimmed


@pytest.mark.parametrize("family,field", SPECTRAL_CASES + [K27])
def test_oracle_gap_condition(family, field):
    """Input condition of the profile cap: near ties of the oracle's two best profiles are rarer
    than the mismatches the cap allows."""
    inp, ref = spectral_case(family, field)
    share = close_gap_share(inp, ref, 1e-5)
    print(f"{family}/{field}: share of voxels with top-two gap < 1e-5: {share:.2e}, "
          f"< 1e-6: {close_gap_share(inp, ref, 1e-6):.2e}")
    assert share <= 1e-4
    # the oracle's own profile is the first maximum of its per-profile runs
    k = np.argmax(ref["Tk"], axis=0)
    assert np.array_equal(np.where(inp["mask"], 0, k), ref["profile"])


def test_paths_is_bound():
    from origin_amd import _capi, kernels
    assert "origin_glr_plan_paths" in _capi.SIGNATURES
    assert len(_capi.SIGNATURES["origin_glr_plan_paths"]) == 6
    assert kernels.GLRPlan.SPECTRAL_FORMS == ("table", "normw", "norm_mfma", "packed", "fp32",
                                              "generic")
    assert callable(kernels.GLRPlan.paths)


# ------------------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def ctx():
    from origin_amd.device import default_context
    return default_context(0)


def run_plan(ctx, inp, precision):
    from origin_amd import kernels
    return kernels.GLRPlan(ctx, inp["shape"], inp["psf"], inp["weights"], inp["profiles"], None,
                           False, precision=precision)       # pcut=None, pmeansub=False


def run_and_fetch(ctx, plan, inp):
    out = plan.run(ctx.to_device(inp["cube"], np.float32),
                   mask=ctx.to_device(inp["mask"].astype(np.uint8)), want_maps=True)
    ctx.sync()
    return {k: out[k].to_host() for k in ("correl", "profile", "correl_min", "maxmap", "minmap")}


def compare(tag, got, inp, ref):
    mask, border, unc = inp["mask"], inp["border"], inp["uncovered"]
    err = {k: np.abs(got[k].astype(np.float64) - ref[k])
           for k in ("correl", "correl_min", "maxmap", "minmap")}
    for k in err:
        assert np.isfinite(got[k]).all(), (tag, k)
    miss = got["profile"] != ref["profile"]
    share = float(np.mean(miss))
    # the oracle's T of the device's choice against the oracle's maximum, at the mismatches
    top = ref["Tk"].max(axis=0)
    assert got["profile"].max() < len(ref["Tk"]), tag
    chosen = np.take_along_axis(ref["Tk"], got["profile"][None].astype(np.intp), axis=0)[0]
    worst_pick = float((top - chosen)[miss].max()) if miss.any() else 0.0
    print(f"{tag}: max|d| correl {err['correl'].max():.2e} correl_min {err['correl_min'].max():.2e} "
          f"maxmap {err['maxmap'].max():.2e} (border {err['maxmap'][border].max():.2e}) "
          f"minmap {err['minmap'].max():.2e} (border {err['minmap'][border].max():.2e}) "
          f"profile mismatches {share:.2e}, worst pick {worst_pick:.2e}")
    # exact
    assert np.all(got["correl"][mask] == 0), tag
    assert np.all(got["profile"][mask] == 0), tag
    assert np.any(got["correl_min"][mask] != 0), tag          # correl_min is not masked
    if unc.any():
        for k in ("correl", "correl_min", "profile"):
            assert np.all(got[k][:, unc] == 0), (tag, k)
    # to tolerance
    for k in ("correl", "correl_min", "maxmap", "minmap"):
        assert err[k].max() <= TOL, (tag, k, float(err[k].max()))
    for k in ("maxmap", "minmap"):
        assert err[k][border].max() <= TOL, (tag, k, "border")
    assert share <= 1e-4, (tag, share)
    assert worst_pick <= 2e-4, (tag, worst_pick)


@gpu
@pytest.mark.parametrize("family,field", SPECTRAL_CASES)
def test_spectral_forms_and_chunks(ctx, family, field):
    """Every spectral kernel of glr_fp32.hip at two or more z chunks with a short last chunk:
    even field -> packed (spectral3_kernel<lwt>, border pass spectral_kernel<LWMAX, false> on the
    list in several slices, list_maps_*), odd field -> spectral_kernel<LWMAX, false> /
    spectral_generic_kernel<false>, weighted fields -> spectral_kernel<LWMAX, true> /
    spectral_generic_kernel<true> (norm cube from spatial_kernel with A = NULL)."""
    lws, Nz, lwt, tmpl, chunks, slices = FAMILIES[family]
    Ny, Nx, weighted, form_t, form_gen = FIELDS[field]
    form = form_gen if family == "gen" else form_t
    inp, ref = spectral_case(family, field)
    plan = run_plan(ctx, inp, "f32")
    paths = plan.paths()
    num_cu = geo.num_cu_of(ctx)
    assert plan.precision == "f32" and not paths["spatial_mfma"]
    assert paths["spectral"] == form, paths
    assert paths["lwt"] == lwt and paths["lwmax"] == max(lws), paths
    assert geo.lwmax_template(paths["lwmax"]) == tmpl
    nzc, zchunk, last = geo.spectral_chunks(num_cu, Ny * Nx, Nz, paths["lwmax"])
    assert nzc >= 2 and last % geo.SPEC_ZC != 0, (nzc, zchunk, last)
    assert (nzc, zchunk, last) == chunks
    if form == "packed":
        assert paths["nborder"] == geo.nborder_of(Ny, Nx, P_SPEC) == 300
        assert geo.border_slices(num_cu, paths["nborder"], Nz, paths["lwmax"])[0] >= 2
    else:
        assert paths["nborder"] == (0 if weighted else geo.nborder_of(Ny, Nx, P_SPEC))
    got = run_and_fetch(ctx, plan, inp)
    plan.close()
    compare(f"{family}/{field}", got, inp, ref)


@gpu
def test_more_than_26_profiles_take_the_packed_kernel_by_themselves(ctx):
    """K = 27 (half widths cycling 1 .. 9) with no precision given: the plan reports "f32" and the
    packed form; the same dictionary cut to 26 profiles does not."""
    inp, ref = spectral_case(*K27)
    Nz, Ny, Nx = inp["shape"]
    plan = run_plan(ctx, inp, None)
    paths = plan.paths()
    assert plan.K == 27 and plan.precision == "f32"
    assert paths["spectral"] == "packed" and paths["lwt"] == 16 and paths["lwmax"] == 9, paths
    assert not paths["spatial_mfma"]
    num_cu = geo.num_cu_of(ctx)
    assert geo.spectral_chunks(num_cu, Ny * Nx, Nz, 9)[0] >= 2
    assert geo.border_slices(num_cu, paths["nborder"], Nz, 9)[0] >= 2
    cut = dict(inp, profiles=inp["profiles"][:26])
    plan26 = run_plan(ctx, cut, None)
    assert plan26.precision != "f32" and plan26.paths()["spectral"] != "packed"
    plan26.close()
    got = run_and_fetch(ctx, plan, inp)
    plan.close()
    compare("k27", got, inp, ref)


@gpu
@pytest.mark.parametrize("P,Ny,Nx,weighted,kernel", SPATIAL_CASES,
                         ids=[f"P{c[0]}-{c[1]}x{c[2]}{'-weighted' if c[3] else ''}"
                              for c in SPATIAL_CASES])
def test_spatial_stage_z_march(ctx, P, Ny, Nx, weighted, kernel):
    """glr_fp32_spatial with one one-tap profile [1.0] (T = cube_fsf / sqrt(norm): the spectral
    stage adds nothing): spatial4x4_kernel marching zper >= 2 planes per block with a last z block
    shorter than zper -- Nx = 70 is no multiple of 4 (non-VEC), 70 x 72 with P = 9 / 25 is VEC,
    with two weighted fields HAS_B accumulating over fields and the norm cube from spatial_kernel
    with A = NULL -- and the generic spatial_kernel (P = 11)."""
    num_cu = geo.num_cu_of(ctx)
    Nz = geo.spatial_nz(num_cu, Ny, Nx)
    zper, blocks, last = geo.spatial_march(num_cu, Nz, Ny, Nx)
    assert zper >= 2 and last < zper and blocks >= 2, (Nz, zper, blocks, last)
    vec = Nx % 4 == 0 and (P // 2) % 4 == 0
    assert vec == ("<%d, true" % P in kernel)
    inp = make_inputs(Nz, Ny, Nx, P, weighted, Nz // 2, _seed("spatial", P, Ny, Nx, weighted))
    inp["profiles"] = [np.array([1.0])]
    plan = run_plan(ctx, inp, "f32")
    paths = plan.paths()
    assert plan.precision == "f32" and not paths["spatial_mfma"], paths
    assert paths["spectral"] == ("fp32" if weighted else "packed"), paths
    assert paths["lwt"] == 8 and paths["lwmax"] == 0, paths
    got = run_and_fetch(ctx, plan, inp)
    plan.close()
    ref = oracle(inp, fft=True)
    compare(kernel, got, inp, ref)
