"""GLR with PSF sizes 27 to 41 (the FSF cube of ORIGIN is (Nz, PSF_size, PSF_size), origin.py:161):
the matrix-core spatial stage (csrc/glr_spatial_mfma.hip, three k-steps per window row) and the
scheduling built on it -- row bands, rectangles, the GLR in the greedy PCA's tail, interior
regions of tiles ahead of the halo exchange.  Oracle: oracle.cpu_ref.Correlation_GLR_test in
float64.  The last test is host only: the MFMA count model."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from oracle import cpu_ref
from origin_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the sizes above 25 whose spatial stage runs on the matrix cores (kernels.SPATIAL_MFMA_SIZES)
LARGE = (27, 29, 31, 33, 35, 37, 39, 41)
MID, TOP = 31, max(LARGE)


@pytest.fixture(scope="module")
def ctx():
    from origin_amd.device import default_context
    return default_context(0)


def _ragged_cases():
    cases = []
    for P in LARGE:
        cases.append(((30, 70, 67), P))            # Nx % 4 != 0, Ny % 64 != 0, two region columns
        cases.append(((28, 66, 42), P))            # narrower than one region
        if (P // 2) % 4 == 0:
            cases.append(((26, 130, 132), P))      # float4 tile loads and stores
    cases.append(((24, 20, 60), MID))              # a field smaller than the PSF: fp32
    cases.append(((24, 50, 30), TOP))
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("shape,P", _ragged_cases())
def test_large_psf_spatial_stage_on_matrix_cores(ctx, shape, P):
    """Every large P on ragged fields: against the float64 oracle and against the fp32 plan; a
    field smaller than the PSF keeps the fp32 kernels."""
    from origin_amd import kernels
    rng = np.random.default_rng(P + shape[2])
    Nz, Ny, Nx = shape
    cube = rng.standard_normal(shape).astype(np.float32)
    cube[Nz // 2, Ny // 2, Nx // 3] += 40.0
    psf = synth.moffat_psf(Nz, P).astype(np.float64)
    psf *= 1.0 + 0.3 * rng.random(psf.shape)          # asymmetric in x and y
    psf /= psf.sum(axis=(1, 2), keepdims=True)
    prof = synth.dico_fwhm(3)
    ref = cpu_ref.Correlation_GLR_test(cube.astype(np.float64), psf, None, prof, nthreads=1,
                                       pcut=1e-8, pmeansub=True)
    small = min(Ny, Nx) < P
    d = ctx.to_device(cube)
    got = {}
    for prec in ("f16x2", "f32"):
        plan = kernels.GLRPlan(ctx, shape, psf, None, prof, 1e-8, True, precision=prec)
        assert plan.precision == ("f32" if small else prec)
        assert plan.spatial_on_matrix_cores == (plan.precision == "f16x2")
        out = plan.run(d, mask=None, want_maps=False)
        got[prec] = out["correl"].to_host()
        assert np.max(np.abs(got[prec] - ref[0])) <= 1e-4
        assert np.max(np.abs(out["correl_min"].to_host() - ref[2])) <= 1e-4
        assert np.mean(out["profile"].to_host() != ref[1]) <= 1e-4
        plan.close()
    assert np.max(np.abs(got["f16x2"] - got["f32"])) <= 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("P", [MID, TOP])
def test_large_psf_bf16_meets_the_bf16_tolerance(ctx, P):
    """precision="bf16" at a large P: the tolerances of the bf16 GLR."""
    from origin_amd import kernels
    rng = np.random.default_rng(12 + P)
    Nz, Ny, Nx = 300, 50, 70
    cube = rng.standard_normal((Nz, Ny, Nx)).astype(np.float32)
    cube[150, 25, 30] += 30.0
    psf = synth.moffat_psf(Nz, P).astype(np.float64)
    prof = synth.dico_fwhm(20)
    ref = cpu_ref.Correlation_GLR_test(cube.astype(np.float64), psf, None, prof, nthreads=1,
                                       pcut=1e-8, pmeansub=True)
    plan = kernels.GLRPlan(ctx, cube.shape, psf, None, prof, 1e-8, True, precision="bf16")
    assert plan.precision == "bf16" and plan.spatial_on_matrix_cores
    out = plan.run(ctx.to_device(cube), mask=None, want_maps=True)
    T, Tmin, arg = out["correl"].to_host(), out["correl_min"].to_host(), out["profile"].to_host()
    d = T - ref[0]
    assert np.max(np.abs(d)) <= 5e-2 and np.sqrt(np.mean(d * d)) <= 5e-3
    assert np.max(np.abs(Tmin - ref[2])) <= 5e-2
    assert (arg != ref[1]).mean() <= 0.02
    assert np.max(np.abs(out["maxmap"].to_host() - ref[0].max(axis=0))) <= 5e-2
    plan.close()


@pytest.mark.gpu
def test_large_psf_weighted_fields_on_matrix_cores(ctx):
    """A mosaic of two weighted fields at P = 31, one corner covered by one field only and one by
    none: against the oracle and against the fp32 plan."""
    from origin_amd import kernels
    P = MID
    rng = np.random.default_rng(31)
    Nz, Ny, Nx = 48, 70, 133
    cube = rng.standard_normal((Nz, Ny, Nx)).astype(np.float32)
    cube[Nz // 2, Ny // 2, Nx // 3] += 40.0
    x = np.linspace(0, 1, Nx)[None, :] * np.ones((Ny, 1))
    raww = [0.2 + x, 1.2 - x]
    tot = sum(raww)
    psfs, ws = [], []
    for f in range(2):
        p = synth.moffat_psf(Nz, P, fwhm0=3.6 - 0.4 * f, fwhm1=3.0 + 0.2 * f).astype(np.float64)
        p *= 1.0 + 0.2 * rng.random(p.shape)
        p /= p.sum(axis=(1, 2), keepdims=True)
        psfs.append(p)
        ws.append((raww[f] / tot).astype(np.float32).astype(np.float64))
    ws[0][:5, :7] = 0.0
    ws[1][-4:, -6:] = 0.0
    ws[0][-4:, -6:] = 0.0
    prof = synth.dico_fwhm(3)
    ref = cpu_ref.Correlation_GLR_test(cube.astype(np.float64), psfs, ws, prof, nthreads=1,
                                       pcut=1e-8, pmeansub=True)
    d = ctx.to_device(cube)
    got = {}
    for prec in ("f16x2", "f32"):
        plan = kernels.GLRPlan(ctx, cube.shape, psfs, ws, prof, 1e-8, True, precision=prec)
        assert plan.precision == prec
        assert plan.spatial_on_matrix_cores == (prec == "f16x2")
        out = plan.run(d, mask=None, want_maps=True)
        got[prec] = out["correl"].to_host()
        assert np.max(np.abs(got[prec] - ref[0])) <= 1e-4
        assert np.max(np.abs(out["correl_min"].to_host() - ref[2])) <= 1e-4
        assert np.mean(out["profile"].to_host() != ref[1]) <= 1e-4
        assert np.max(np.abs(out["maxmap"].to_host() - ref[0].max(axis=0))) <= 1e-4
        plan.close()
    assert np.max(np.abs(got["f16x2"] - got["f32"])) <= 1e-4


def _outputs(ctx, shape):
    correl, cmin = ctx.empty(shape, np.float32), ctx.empty(shape, np.float32)
    prof_i = ctx.empty(shape, np.uint8)
    for a in (correl, cmin, prof_i):
        a.fill_bytes(0x7f)
    return correl, cmin, prof_i


@pytest.mark.gpu
@pytest.mark.parametrize("P", [MID, TOP])
def test_large_psf_row_bands_write_what_the_whole_run_writes(ctx, P):
    """Row bands of a large-P plan (shuffled, one on the side stream): bit for bit plan.run."""
    from origin_amd import kernels
    rng = np.random.default_rng(P)
    Nz, Ny, Nx = 120, 230, 77
    cube = rng.standard_normal((Nz, Ny, Nx)).astype(np.float32)
    cube[40:90] *= 21.0
    mask = (rng.random((Nz, Ny, Nx)) < 0.01).astype(np.uint8)
    psf = synth.moffat_psf(3681, P)[:Nz].astype(np.float64)
    plan = kernels.GLRPlan(ctx, cube.shape, psf, None, synth.dico_fwhm(20), 1e-8, True,
                           precision="f16x2")
    assert plan.rows_supported()
    d_cube, d_mask = ctx.to_device(cube), ctx.to_device(mask)
    whole = plan.run(d_cube, mask=d_mask, want_maps=True)
    want = {k: whole[k].to_host() for k in ("correl", "correl_min", "profile", "maxmap", "minmap")}
    correl, cmin, prof_i = _outputs(ctx, cube.shape)
    plan.run_rows(d_cube, d_mask, correl, prof_i, cmin, 128, 192, first=True)
    plan.run_rows(d_cube, d_mask, correl, prof_i, cmin, 0, 64, side=True)
    plan.run_rows(d_cube, d_mask, correl, prof_i, cmin, 192, Ny)
    plan.run_rows(d_cube, d_mask, correl, prof_i, cmin, 64, 128)
    maxmap, minmap = plan.run_finish()
    ctx.sync()
    got = dict(correl=correl.to_host(), correl_min=cmin.to_host(), profile=prof_i.to_host(),
               maxmap=maxmap.to_host(), minmap=minmap.to_host())
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    plan.close()


@pytest.mark.gpu
def test_large_psf_rectangles_agree_with_the_whole_run(ctx):
    """run_rect at P = 31: a rectangle of whole rows bit for bit, the others to rounding."""
    from origin_amd import kernels
    rng = np.random.default_rng(8)
    Nz, Ny, Nx = 120, 150, 170
    cube = rng.standard_normal((Nz, Ny, Nx)).astype(np.float32)
    cube[30:70] *= 19.0
    mask = (rng.random((Nz, Ny, Nx)) < 0.01).astype(np.uint8)
    psf = synth.moffat_psf(3681, MID)[:Nz].astype(np.float64)
    plan = kernels.GLRPlan(ctx, cube.shape, psf, None, synth.dico_fwhm(20), 1e-8, True,
                           precision="f16x2")
    d_cube, d_mask = ctx.to_device(cube), ctx.to_device(mask)
    whole = plan.run(d_cube, mask=d_mask, want_maps=True)
    want = {k: whole[k].to_host() for k in ("correl", "correl_min", "profile", "maxmap", "minmap")}
    correl, cmin, prof_i = _outputs(ctx, cube.shape)
    plan.run_rect(d_cube, d_mask, correl, prof_i, cmin, 64, Ny, 64, Nx, first=True, side=True)
    plan.run_rect(d_cube, d_mask, correl, prof_i, cmin, 0, 64, 0, Nx)
    plan.run_rect(d_cube, d_mask, correl, prof_i, cmin, 64, 128, 0, 64)
    plan.run_rect(d_cube, d_mask, correl, prof_i, cmin, 128, Ny, 0, 64)
    maxmap, minmap = plan.run_finish()
    ctx.sync()
    got = dict(correl=correl.to_host(), correl_min=cmin.to_host(), profile=prof_i.to_host(),
               maxmap=maxmap.to_host(), minmap=minmap.to_host())
    for k in ("correl", "correl_min", "profile"):
        assert np.array_equal(got[k][:, :64], want[k][:, :64]), k
    scale = np.abs(want["correl"]).max()
    for k in ("correl", "correl_min", "maxmap", "minmap"):
        assert np.max(np.abs(got[k] - want[k])) <= 3e-6 * scale, k
    assert np.mean(got["profile"] != want["profile"]) <= 1e-4
    assert np.max(np.abs(got["maxmap"] - got["correl"].max(axis=0))) == 0.0
    plan.close()


@pytest.mark.gpu
def test_large_psf_glr_in_the_pca_tail(ctx):
    """pipeline.greedy_pca_then_glr with a P = 31 plan: one area of six iterates long after the
    others, the bands that read none of its rows (halo 15) run in the PCA's shadow; every output
    is bit for bit that of greedy_pca followed by plan.run."""
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
    for a in range(nb):
        idx = np.flatnonzero(areamap.reshape(-1) == a + 1)
        for j in range(40 if a == 3 else 3):
            flat[:, idx[17 * j + 5]] += (7.0 + 0.11 * j) * rng.standard_normal(Nz).astype(np.float32)
    X = cube.astype(float)
    tests = [cpu_ref.O2test(X[:, areamap == a + 1]) for a in range(nb)]
    thr = [float(np.percentile(t, 99.0)) for t in tests]
    mask = (rng.random((Nz, Ny, Nx)) < 0.005).astype(np.uint8)
    psf = synth.moffat_psf(3681, MID)[:Nz].astype(np.float64)
    plan = kernels.GLRPlan(ctx, cube.shape, psf, None, synth.dico_fwhm(20), 1e-8, True,
                           precision="f16x2")
    assert plan.rows_supported()
    d, d_mask = ctx.to_device(cube), ctx.to_device(mask)
    F0, map0, nstop0, _ = pipeline.greedy_pca(ctx, d, areamap, nb, thr, tests, 50, 100)
    out0 = plan.run(F0, mask=d_mask, want_maps=True)
    want = {k: out0[k].to_host() for k in ("correl", "correl_min", "profile", "maxmap", "minmap")}
    correl, cmin, prof_i = _outputs(ctx, cube.shape)
    faint = ctx.empty(cube.shape, np.float32)
    faint.fill_bytes(0x7f)
    F1, map1, nstop1, _, out1 = pipeline.greedy_pca_then_glr(
        ctx, plan, d, areamap, nb, thr, tests, d_mask, correl, prof_i, cmin, faint, max_active=1)
    ctx.sync()
    assert nstop0 == nstop1 and np.array_equal(map0, map1)
    assert np.array_equal(F1.to_host(), F0.to_host())
    for k in want:
        assert np.array_equal(out1[k].to_host(), want[k]), k
    early, late = out1["bands"]
    assert early and late, (early, late)
    plan.close()


@pytest.mark.gpu
def test_large_psf_tiled_interior_regions_ahead_of_the_halo_exchange(ctx, tmp_path):
    """Two ranks on one card (host group) at P = 31: TiledGLR runs the tiles' interior rectangles
    ahead of the halo exchange; the stitched tiles match the one-context run."""
    from _mp_tiled_large_psf_worker import field
    from origin_amd import kernels
    P, world = MID, 2
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2",
                   TILED_P=str(P))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests",
                                                                    "_mp_tiled_large_psf_worker.py"),
                                       str(tmp_path / "t")], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    logs = [p.communicate(timeout=600)[0].decode()[-3000:] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    tiles = [np.load(str(tmp_path / f"t.rank{r}.npz")) for r in range(world)]
    assert all(int(t["spatial_mfma"]) and int(t["rows"]) for t in tiles)
    assert sum(int(t["n_early"]) for t in tiles) > 0
    cube, mask, psf, prof = field(P)
    plan = kernels.GLRPlan(ctx, cube.shape, psf, None, prof, 1e-8, True)
    out = plan.run(ctx.to_device(cube), mask=ctx.to_device(mask), want_maps=False)
    one = {k: out[k].to_host() for k in ("correl", "correl_min")}
    plan.close()
    for k in ("correl", "correl_min"):
        full = np.zeros(cube.shape, np.float32)
        for t in tiles:
            full[:, int(t["y0"]):int(t["y1"]), int(t["x0"]):int(t["x1"])] = t[k]
        assert np.max(np.abs(full - one[k])) <= 1e-4, k


# ---------------------------------------------------------------------- host only
def _count_model(P, terms=3, Nz=3681, N=600, K=20, n_narrow=10, num_cu=256):
    from origin_amd import _capi
    a, b = C.c_long(), C.c_long()
    _capi.call("origin_glr_mfma_count_model", num_cu, terms, K, n_narrow, Nz, N, N, P,
               C.byref(a), C.byref(b))
    return a.value


def test_large_psf_mfma_count_model():
    """The spatial stage's MFMA count at 3681 x 600 x 600 (100 regions of 64 x 64, four waves per
    region and channel): (P + 3) x 3 k-steps for the large sizes, 0 above 41, and the P <= 25
    values unchanged."""
    from origin_amd import kernels
    base = 100 * 3681 * 4
    for P in LARGE:
        assert P in kernels.SPATIAL_MFMA_SIZES
        for terms in (1, 3):
            assert _count_model(P, terms) == base * (P + 3) * 3 * terms > 0
    assert {P: (P + 3) * 3 for P in (27, 31, 35, 41)} == {27: 90, 31: 102, 35: 114, 41: 132}
    for P in (43, 45, 26, 3):
        assert _count_model(P) == 0
    # (4 + P - 1) x ceil((8 + P - 1) / 16) k-steps, f16 split: the values before the large sizes
    old = {5: 35337600, 7: 44172000, 9: 53006400, 11: 123681600, 13: 141350400, 15: 159019200,
           17: 176688000, 19: 194356800, 21: 212025600, 23: 229694400, 25: 247363200}
    assert {P: _count_model(P) for P in old} == old
