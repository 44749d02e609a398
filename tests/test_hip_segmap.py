"""GPU: the segmentation kernels (csrc/segmap.hip) against SciPy -- ``np.array_equal`` everywhere,
there is no tolerance in this file except the one of the host threshold fit (rtol 1e-10, the
tolerance tests/test_host_logic.py has for ``compute_thresh_gaussfit`` against the reference).

* the labeller against ``scipy.ndimage.label`` for every pattern x shape of tests/_segmap_cases.py
  (shapes derived from ``origin_label_tile``);
* every mask stage against tests/_segmap_oracle.py for every mask pattern and ``fwhm_fsf``;
* ``merged_labels`` against ``ndi.label((a > 0) | (b > 0))``;
* the reference's golden labels (tests/golden/g14_segmap.npz);
* steps 1-6 through ``SimpleOrig``: every segmentation call of the steps, recorded, against the
  oracle on the recorded inputs."""
import os

import numpy as np
import pytest
from scipy import ndimage as ndi

import _segmap_cases as cases
import _segmap_oracle as oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g14_segmap.npz")
SHAPE_NAMES = ("one_pixel", "one_row", "one_column", "one_tile", "below_a_tile", "many_tiles",
               "two_scan_passes")


@pytest.fixture(scope="module")
def ctx():
    from origin_amd.device import default_context
    return default_context(0)


@pytest.fixture(scope="module")
def geometry():
    from origin_amd import kernels
    return kernels.label_tile() + (kernels.label_scan_span(),)


@pytest.mark.parametrize("pattern", list(cases.LABEL_PATTERNS))
@pytest.mark.parametrize("shape_name", SHAPE_NAMES)
def test_labels_are_scipys(ctx, geometry, shape_name, pattern):
    from origin_amd import segmap
    Ny, Nx = cases.label_shapes(*geometry)[shape_name]
    mask = cases.LABEL_PATTERNS[pattern](Ny, Nx)
    want, nwant = ndi.label(mask)
    got, ngot = segmap.label_mask(ctx, mask)
    assert got.dtype == np.int32 and got.shape == (Ny, Nx)
    assert ngot == nwant
    assert np.array_equal(got, want)
    again, nagain = segmap.label_mask(ctx, mask)            # the same from run to run
    assert nagain == ngot and np.array_equal(again, got)


@pytest.mark.parametrize("pattern", list(cases.MASK_PATTERNS))
@pytest.mark.parametrize("shape_name", ["a", "b"])
def test_mask_stages_are_scipys(ctx, geometry, shape_name, pattern):
    from origin_amd import segmap
    Ny, Nx = cases.mask_shapes(*geometry[:2])[shape_name]
    data = cases.MASK_PATTERNS[pattern](Ny, Nx)
    for fwhm in cases.FWHM_FSF:
        want = oracle.mask_stages(data, cases.GAMMA, fwhm)
        got = segmap.mask_stages(ctx, data, cases.GAMMA, fwhm)
        for stage, (g, w) in enumerate(zip(got, want), 1):
            assert np.array_equal(g, w), f"fwhm_fsf {fwhm}, stage {stage}: " \
                                         f"{np.count_nonzero(g != w)} pixels differ"
        labels, n = segmap.labels_at(ctx, data, cases.GAMMA, fwhm)
        wl, wn = oracle.labels_at(data, cases.GAMMA, fwhm)
        assert n == wn and np.array_equal(labels, wl), f"fwhm_fsf {fwhm}: labels"
        if fwhm == 1:
            assert not got[3].any()                        # f = 0: the empty mask


def test_disc_offsets_are_the_strict_ones(ctx):
    """One pixel through the disc of f = 5 (fwhm_fsf 10 and 11): the 3-4-5 offsets are out.  The
    pixel sits in a plus (which erosion and dilation leave alone) at a corner of the image too."""
    from origin_amd import segmap
    data = np.zeros((40, 45))
    for cy, cx in ((20, 22), (1, 1), (38, 43)):
        data[cy, cx - 1:cx + 2] = data[cy - 1:cy + 2, cx] = 2.0
    for fwhm in (10, 11, 25):
        want = oracle.mask_stages(data, 1.0, fwhm)[3]
        got = segmap.mask_stages(ctx, data, 1.0, fwhm)[3]
        assert np.array_equal(got, want), fwhm
    got = segmap.mask_stages(ctx, data, 1.0, 10)[3]
    assert got[20, 22 + 5] and not got[20, 22 + 6]           # the plus's arm + 4, not + 5
    assert got[20 + 3, 22 + 1 + 3] and not got[20 + 4, 22 + 1 + 3]


@pytest.mark.parametrize("shape_name", ["many_tiles", "one_row", "one_pixel"])
def test_merged_labels(ctx, geometry, shape_name):
    from origin_amd import segmap
    Ny, Nx = cases.label_shapes(*geometry)[shape_name]
    a = ndi.label(cases.LABEL_PATTERNS["random_0.3"](Ny, Nx))[0]
    b = ndi.label(cases.LABEL_PATTERNS["rings"](Ny, Nx))[0]
    z = np.zeros((Ny, Nx), np.int32)
    for x, y in ((a, b), (b, a), (a, z), (z, z), (a.astype(np.int64), b.astype(np.float64))):
        want = ndi.label((x > 0) | (y > 0))[0]
        got = segmap.merged_labels(ctx, x, y)
        assert got.dtype == np.int32 and np.array_equal(got, want)


def test_golden_labels(ctx):
    import origin_amd.lib_origin as lib
    from origin_amd import segmap
    with np.load(GOLDEN) as g:
        for n in "abc":
            data, gamma, want = g[n + "_data"], float(g[n + "_gamma"]), g[n + "_labels"]
            pfa, fwhm = float(g[n + "_pfa"]), int(g[n + "_fwhm_fsf"])
            got, ngot = segmap.labels_at(ctx, data, gamma, fwhm)
            assert ngot == want.max() and np.array_equal(got, want), n
            gam2, lab2 = lib.compute_segmap_gauss(data, pfa, fwhm_fsf=fwhm)
            np.testing.assert_allclose(gam2, gamma, rtol=1e-10)
            assert lab2.dtype == np.int32 and np.array_equal(lab2, want), n


@pytest.fixture(scope="module")
def session():
    """Steps 1-6 on the small synthetic field, every segmentation call recorded."""
    from origin_amd import segmap, synth
    from origin_amd.steps import SimpleOrig
    calls = []
    real = segmap.segmap_gauss, segmap.merged_labels

    def rec_gauss(ctx, data, pfa, fwhm_fsf=0, bins='fd'):
        out = real[0](ctx, data, pfa, fwhm_fsf, bins=bins)
        calls.append(("gauss", np.array(data), pfa, fwhm_fsf, out))
        return out

    def rec_merged(ctx, a, b):
        out = real[1](ctx, a, b)
        calls.append(("merged", np.array(a), np.array(b), out))
        return out

    f, raw, var, mask = synth.small_case(Nz=160, Ny=48, Nx=52, seed=3, psf_size=9, nprof=3,
                                         area_size=24)
    orig = SimpleOrig(raw, var, mask, f.PSF.astype(float), f.profiles)
    segmap.segmap_gauss, segmap.merged_labels = rec_gauss, rec_merged
    try:
        orig.step01_preprocessing()
        orig.step02_areas.set_areamap(f.areamap)
        orig.step03_compute_PCA_threshold()
        orig.step04_compute_greedy_PCA()
        orig.step05_compute_TGLR()
        orig.step06_compute_purity_threshold()
    finally:
        segmap.segmap_gauss, segmap.merged_labels = real
    return orig, calls


def test_steps_call_the_device_path(session):
    orig, calls = session
    assert [c[0] for c in calls] == ["gauss", "gauss", "merged", "gauss", "merged"]
    mean_fwhm = int(np.ceil(np.mean(orig.FWHM_PSF)))
    assert [c[3] for c in calls if c[0] == "gauss"] == [mean_fwhm, mean_fwhm, 0]
    assert [c[2] for c in calls if c[0] == "gauss"] == [0.01, 0.01, 1e-5]
    for c in calls:
        if c[0] == "gauss":
            _, data, pfa, fwhm, (gamma, labels) = c
            assert data.dtype == np.float64 and labels.dtype == np.int32
            assert np.array_equal(labels, oracle.labels_at(data, gamma, fwhm)[0])
            # (the fit is host code either way: the oracle's whole function gives the same gamma)
            assert oracle.compute_segmap_gauss(data, pfa, fwhm)[0] == gamma
        else:
            _, a, b, labels = c
            assert np.array_equal(labels, oracle.merged_labels(a, b))
    assert np.array_equal(np.asarray(orig.segmap_cont), calls[0][4][1])
    assert np.array_equal(np.asarray(orig.segmap_merged), calls[2][3])
    assert np.array_equal(np.asarray(orig.segmap_purity), calls[4][3])
    assert np.array_equal(calls[2][1], calls[0][4][1]) and np.array_equal(calls[2][2], calls[1][4][1])
    assert np.array_equal(calls[4][1], calls[3][4][1])
    assert np.asarray(orig.segmap_merged).max() >= 1          # not vacuous


def test_segmap_purity_from_the_stored_maps(session):
    orig, _ = session
    gamma, res = oracle.compute_segmap_gauss(np.asarray(orig.maxmap, dtype=np.float64), 1e-5, 0)
    want = oracle.merged_labels(res, np.asarray(orig.segmap_merged))
    assert np.array_equal(np.asarray(orig.segmap_purity), want)
