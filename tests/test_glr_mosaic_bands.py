"""GPU: the GLR of a mosaic of weighted fields (several PSFs, one weight map each) in row bands and
rectangles -- origin_glr_plan_prepare, then origin_glr_run_rows / _rect / _finish on the two
spectral forms of a plan with a norm cube: NORMW (the FOLD form of the table kernel on the norm cube,
the two-product kernel for the 32 channels at either end) and the two-product kernel everywhere
(ORIGIN_GLR_NO_FOLD=1), on spaxel ranges and rectangles.  Then what is built on bands: the GLR in
the shadow of the greedy PCA's tail (pipeline.greedy_pca_then_glr) and the regions of a tile ahead
of its halo exchange (multigpu.TiledGLR behind SimpleOrig(devices=[0, 0])).

The fields are those of tests/test_hip_parity.py's weighted tests: Moffat PSFs that vary smoothly
with the channel (eps of the FOLD form passes), linear weight ramps normalised to sum 1, one corner
that one field does not cover and one that no field covers, a sparse random mask."""
import numpy as np
import pytest

from oracle import cpu_ref
from origin_amd import synth

pytestmark = pytest.mark.gpu

OUTPUTS = ("correl", "correl_min", "profile", "maxmap", "minmap")


@pytest.fixture(scope="module")
def ctx():
    from origin_amd.device import default_context
    return default_context(0)


def mosaic(Nz, Ny, Nx, nf, P=9):
    """PSFs and weight maps of ``nf`` fields over an (Ny, Nx) field."""
    x = np.linspace(0, 1, Nx)[None, :] * np.ones((Ny, 1))
    y = np.linspace(0, 1, Ny)[:, None] * np.ones((1, Nx))
    raww = [0.3 + x, 1.1 - x, 0.2 + y][:nf]
    tot = sum(raww)
    psfs = [synth.moffat_psf(3681, P, fwhm0=3.6 - 0.3 * f, fwhm1=3.0 + 0.2 * f)[:Nz].astype(np.float64)
            for f in range(nf)]
    ws = [(raww[f] / tot).astype(np.float32).astype(np.float64) for f in range(nf)]
    ws[0][:5, :7] = 0.0                       # a corner one field does not cover
    for w in ws:
        w[-9:, -10:] = 0.0                    # a corner NO field covers: norm = 0 -> T = 0
    return psfs, ws


def set_form(monkeypatch, form):
    if form == "norm_mfma":
        monkeypatch.setenv("ORIGIN_GLR_NO_FOLD", "1")
    else:
        monkeypatch.delenv("ORIGIN_GLR_NO_FOLD", raising=False)


def outputs(ctx, shape):
    correl, cmin = ctx.empty(shape, np.float32), ctx.empty(shape, np.float32)
    prof_i = ctx.empty(shape, np.uint8)
    for a in (correl, cmin, prof_i):
        a.fill_bytes(0x7f)
    return correl, cmin, prof_i


def host(out):
    return {k: out[k].to_host() for k in OUTPUTS}


@pytest.mark.parametrize("form,precision,nprof,nf", [("normw", "f16x2", 20, 2),
                                                     ("normw", "bf16", 20, 2),
                                                     ("norm_mfma", "f16x2", 20, 2),   # two passes
                                                     ("norm_mfma", "f16x2", 3, 3)])   # one pass
def test_weighted_row_bands_write_what_the_whole_run_writes(ctx, monkeypatch, form, precision,
                                                            nprof, nf):
    """A weighted plan's run split into four row bands (shuffled, one on the side stream) is bit
    for bit ``plan.run``: the bands' waves hold the spaxels the whole run's waves hold, their z
    chunks and partial-map rows are the whole field's, both passes of a dictionary of more than
    13 profiles cover the band.  A height that is no multiple of 64, a width that is no multiple
    of 32, three fields in the last case.  Before ``prepare()`` a band of a weighted plan raises
    (the norm cube and its eps are not a band's to make)."""
    from origin_amd import kernels
    rng = np.random.default_rng(5)
    Nz, Ny, Nx = 330, 230, 77
    cube = rng.standard_normal((Nz, Ny, Nx)).astype(np.float32)
    cube[150:190] *= 21.0
    mask = (rng.random((Nz, Ny, Nx)) < 0.01).astype(np.uint8)
    psfs, ws = mosaic(Nz, Ny, Nx, nf)
    set_form(monkeypatch, form)
    plan = kernels.GLRPlan(ctx, cube.shape, psfs, ws, synth.dico_fwhm(nprof), 1e-8, True,
                           precision=precision)
    assert plan.precision == precision
    d_cube, d_mask = ctx.to_device(cube), ctx.to_device(mask)
    correl, cmin, prof_i = outputs(ctx, cube.shape)
    assert not plan.rows_supported()
    with pytest.raises(Exception, match="origin_glr_plan_prepare"):
        plan.run_rows(d_cube, d_mask, correl, prof_i, cmin, 0, 64, first=True)
    plan.prepare()
    plan.prepare()                                                  # (idempotent)
    assert plan.paths()["spectral"] == form and plan.paths()["spatial_mfma"]
    assert plan.rows_supported()
    plan.run_rows(d_cube, d_mask, correl, prof_i, cmin, 128, 192, first=True)
    plan.run_rows(d_cube, d_mask, correl, prof_i, cmin, 0, 64, side=True)
    plan.run_rows(d_cube, d_mask, correl, prof_i, cmin, 192, Ny)
    plan.run_rows(d_cube, d_mask, correl, prof_i, cmin, 64, 128)
    maxmap, minmap = plan.run_finish()
    ctx.sync()
    got = host(dict(correl=correl, correl_min=cmin, profile=prof_i, maxmap=maxmap, minmap=minmap))
    want = host(plan.run(d_cube, mask=d_mask, want_maps=True))
    for k in OUTPUTS:
        assert np.array_equal(got[k], want[k]), k
    with pytest.raises(Exception):
        plan.run_rows(d_cube, d_mask, correl, prof_i, cmin, 32, 128)   # not a multiple of 64
    plan.close()


@pytest.fixture(scope="module")
def rect_field():
    """The field of the rectangle test and its float64 reference (made once for both forms)."""
    rng = np.random.default_rng(8)
    Nz, Ny, Nx = 330, 150, 170
    cube = rng.standard_normal((Nz, Ny, Nx)).astype(np.float32)
    cube[150:190] *= 19.0
    mask = (rng.random((Nz, Ny, Nx)) < 0.01).astype(np.uint8)
    psfs, ws = mosaic(Nz, Ny, Nx, 2)
    prof = synth.dico_fwhm(14)      # (more than 13: the two-product form in two merged passes)
    ref = cpu_ref.Correlation_GLR_test(cube.astype(np.float64), psfs, ws, prof, nthreads=1,
                                       pcut=1e-8, pmeansub=True)
    return cube, mask, psfs, ws, prof, ref


@pytest.mark.parametrize("form", ["normw", "norm_mfma"])
def test_weighted_rectangles_agree_with_the_whole_run(ctx, monkeypatch, rect_field, form):
    """The field in four rectangles of 64 x 64 regions (one on the side stream), what a tile does
    around its halo exchange.  The rectangle of whole rows is bit for bit the whole run's; in the
    others a wave of the spectral stage holds 32 columns of one row (other tile scales), so they
    and the whole run are each held to the float64 oracle at the bound of
    test_glr_weighted_fields_fold_form_on_the_norm_cube -- (eps + 3e-6) times the running maximum
    over 193 channels of max |T_ref|, eps = 0 for the two-product form -- and differ from each
    other by at most twice that."""
    from scipy.ndimage import maximum_filter1d
    from origin_amd import kernels
    cube, mask, psfs, ws, prof, ref = rect_field
    Nz, Ny, Nx = cube.shape
    set_form(monkeypatch, form)
    plan = kernels.GLRPlan(ctx, cube.shape, psfs, ws, prof, 1e-8, True, precision="f16x2")
    plan.prepare()
    assert plan.paths()["spectral"] == form and plan.rows_supported()
    eps = plan.fold_eps()[0] if form == "normw" else 0.0
    assert 0.0 <= eps <= 2e-6
    d_cube, d_mask = ctx.to_device(cube), ctx.to_device(mask)
    want = host(plan.run(d_cube, mask=d_mask, want_maps=True))
    correl, cmin, prof_i = outputs(ctx, cube.shape)
    plan.run_rect(d_cube, d_mask, correl, prof_i, cmin, 64, Ny, 64, Nx, first=True, side=True)
    plan.run_rect(d_cube, d_mask, correl, prof_i, cmin, 0, 64, 0, Nx)          # all columns
    plan.run_rect(d_cube, d_mask, correl, prof_i, cmin, 64, 128, 0, 64)
    plan.run_rect(d_cube, d_mask, correl, prof_i, cmin, 128, Ny, 0, 64)
    maxmap, minmap = plan.run_finish()
    ctx.sync()
    got = host(dict(correl=correl, correl_min=cmin, profile=prof_i, maxmap=maxmap, minmap=minmap))
    plan.close()
    for k in ("correl", "correl_min", "profile"):
        assert np.array_equal(got[k][:, :64], want[k][:, :64]), k     # the band of whole rows
    local = maximum_filter1d(np.abs(ref[0]).max(axis=(1, 2)), size=193, mode="nearest")
    tol = ((eps + 3e-6) * local)[:, None, None]
    m = mask.astype(bool)
    refs = dict(correl=np.where(m, 0.0, ref[0]), correl_min=ref[2])   # (correl[mask] = 0)
    for k, r in refs.items():
        for name, o in (("rectangles", got), ("whole", want)):
            err = np.abs(o[k] - r)
            print(form, k, name, "max err / bound", float(np.max(err / tol)))
            assert np.all(err <= tol), (k, name)
        assert np.all(np.abs(got[k] - want[k]) <= 2 * tol), k
    for k, r in (("maxmap", refs["correl"].max(axis=0)), ("minmap", ref[2].min(axis=0))):
        for o in (got, want):
            assert np.all(np.abs(o[k] - r) <= tol.max()), k
    sel = np.ones((Ny, Nx), bool)
    sel[-9:, -10:] = False       # (no field reaches: every T is 0, the oracle's index is FFT noise)
    refp = np.where(m, 0, ref[1])
    for o in (got, want):
        assert np.mean(o["profile"][:, sel] != refp[:, sel]) <= 1e-4
        assert np.all(o["correl"][:, -5:, -6:] == 0.0)                # the uncovered corner
    assert np.max(np.abs(got["maxmap"] - got["correl"].max(axis=0))) == 0.0
    assert np.max(np.abs(got["minmap"] - got["correl_min"].min(axis=0))) == 0.0


def test_weighted_glr_in_the_shadow_of_the_pca_tail(ctx, monkeypatch):
    """pipeline.greedy_pca_then_glr with a two-field plan: it prepares the plan, the hook fires
    while one straggler area iterates, the early bands run on the side stream -- and cube_faint,
    mapO2, nstop, the GLR's outputs and the local maxima are bit for bit those of greedy_pca
    followed by plan.run."""
    from origin_amd import kernels, pipeline
    rng = np.random.default_rng(11)
    Nz, Ny, Nx = 150, 300, 128
    cube = rng.standard_normal((Nz, Ny, Nx)).astype(np.float32)
    areamap = np.zeros((Ny, Nx), int)
    for i in range(3):
        for j in range(2):
            areamap[100 * i:100 * (i + 1), 64 * j:64 * (j + 1)] = 2 * i + j + 1
    nb = 6
    flat = cube.reshape(Nz, -1)
    # a few bright spectra per area; many more, of comparable strength, in area 4 (rows 100-199)
    for a in range(nb):
        idx = np.flatnonzero(areamap.reshape(-1) == a + 1)
        for j in range(40 if a == 3 else 3):
            flat[:, idx[17 * j + 5]] += (7.0 + 0.11 * j) * rng.standard_normal(Nz).astype(np.float32)
    X = cube.astype(float)
    tests = [cpu_ref.O2test(X[:, areamap == a + 1]) for a in range(nb)]
    thr = [float(np.percentile(t, 99.0)) for t in tests]
    mask = (rng.random((Nz, Ny, Nx)) < 0.005).astype(np.uint8)
    psfs, ws = mosaic(Nz, Ny, Nx, 2)
    monkeypatch.delenv("ORIGIN_GLR_NO_FOLD", raising=False)
    plan = kernels.GLRPlan(ctx, cube.shape, psfs, ws, synth.dico_fwhm(20), 1e-8, True,
                           precision="f16x2")
    d, d_mask = ctx.to_device(cube), ctx.to_device(mask)
    F0, map0, nstop0, _ = pipeline.greedy_pca(ctx, d, areamap, nb, thr, tests, 50, 100)
    out0 = plan.run(F0, mask=d_mask, want_maps=True)
    assert plan.paths()["spectral"] == "normw"
    want = host(out0)
    want_lm = [a.to_host() for a in kernels.local_max(ctx, out0["correl"], out0["correl_min"],
                                                      d_mask, 3)]
    # a plan of its own for the chain: greedy_pca_then_glr is what prepares it
    chain = kernels.GLRPlan(ctx, cube.shape, psfs, ws, synth.dico_fwhm(20), 1e-8, True,
                            precision="f16x2")
    assert not chain.rows_supported()
    correl, cmin, prof_i = outputs(ctx, cube.shape)
    faint = ctx.empty(cube.shape, np.float32)
    faint.fill_bytes(0x7f)
    lmax, lmin = ctx.empty(cube.shape, np.float32), ctx.empty(cube.shape, np.float32)
    F1, map1, nstop1, _, out1 = pipeline.greedy_pca_then_glr(
        ctx, chain, d, areamap, nb, thr, tests, d_mask, correl, prof_i, cmin, faint,
        max_active=1, local_max=(lmax, lmin))
    ctx.sync()
    assert chain.paths()["spectral"] == "normw" and chain.rows_supported()
    early, late = out1["bands"]
    assert early and late, (early, late)                         # the hook did fire
    assert nstop0 == nstop1 and np.array_equal(map0, map1)
    assert np.array_equal(F1.to_host(), F0.to_host())
    for k in OUTPUTS:
        assert np.array_equal(out1[k].to_host(), want[k]), k
    assert np.array_equal(out1["local_max"].to_host(), want_lm[0])
    assert np.array_equal(out1["local_min"].to_host(), want_lm[1])
    plan.close()
    chain.close()


def test_tiled_mosaic_runs_regions_ahead_of_the_halo_exchange(monkeypatch):
    """``SimpleOrig(..., wfields=[w0, w1], devices=[0, 0])`` through steps 1-5 on a 2 x 2 grid of
    areas: each rank's TiledGLR prepares its weighted plan, so the 64 x 64 regions of its extended
    box that read no foreign spaxel run ahead of the halo exchange (``last_rects[0]``).  Against
    the same chain on one context: mapO2 identical, the GLR cubes and maps within 1e-4 (DESIGN
    section 6b's bound for two contexts)."""
    from origin_amd.steps import SimpleOrig
    monkeypatch.delenv("ORIGIN_GLR_NO_FOLD", raising=False)
    monkeypatch.delenv("ORIGIN_TILED_INTERIOR_FIRST", raising=False)
    Nz, Ny, Nx = 100, 256, 192
    f = synth.SyntheticField(Nz, Ny, Nx, seed=6, psf_size=9, nprof=3, blob_density=1 / 200,
                             emitter_density=1 / 900, area_size=50)
    raw, var, mask = f.arrays()
    mask[10:14, 3, 7] = True
    mask[:, 125, 141] = True
    raw[mask] = 0
    var[mask] = np.inf
    areamap = np.zeros((Ny, Nx), int)
    for i in range(2):
        for j in range(2):
            areamap[128 * i:128 * (i + 1), 96 * j:96 * (j + 1)] = 2 * i + j + 1
    psfs, ws = mosaic(Nz, Ny, Nx, 2)

    def chain(orig):
        orig.step01_preprocessing()
        orig.step02_areas.set_areamap(areamap)
        orig.step03_compute_PCA_threshold()
        orig.step04_compute_greedy_PCA()
        orig.step05_compute_TGLR()
        return orig
    one = chain(SimpleOrig(raw, var, mask, psfs, f.profiles, wfields=ws))
    two = chain(SimpleOrig(raw, var, mask, psfs, f.profiles, wfields=ws, devices=[0, 0]))
    sess = two._hip_session
    assert sess.world == 2
    for st in sess.rk:
        glr = st["glr"]
        assert glr.plan.paths()["spectral"] == "normw" and glr.plan.rows_supported()
        assert len(glr.last_rects[0]) > 0, glr.last_rects
    assert np.array_equal(np.asarray(two.mapO2), np.asarray(one.mapO2))
    for name in ("cube_correl", "cube_correl_min"):
        assert np.max(np.abs(getattr(two, name)._data - getattr(one, name)._data)) <= 1e-4, name
    assert np.max(np.abs(np.asarray(two.maxmap) - np.asarray(one.maxmap))) <= 1e-4
    sess.close()
