"""CPU: the segmentation kernels' interface is declared, exported and bound; the patterns and
shapes of tests/_segmap_cases.py are what they claim; tests/_segmap_oracle.py reproduces the
reference's golden labels (tests/golden/g14_segmap.npz, tools/gen_segmap_golden.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import ndimage as ndi

import _segmap_cases as cases
import _segmap_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g14_segmap.npz")
ENTRIES = ("origin_segmap_mask", "origin_segmap_union", "origin_segmap_label", "origin_label_tile",
           "origin_label_scan_span")


@pytest.fixture(scope="module")
def geometry():
    from origin_amd import build, kernels
    build.build()
    return kernels.label_tile() + (kernels.label_scan_span(),)


def test_entry_points_are_declared_exported_and_bound():
    from origin_amd import build, _capi, kernels, lib_origin, segmap, steps
    build.build()
    header = open(os.path.join(ROOT, "include", "origin_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(os.path.join(ROOT, "origin_amd", "liborigin_hip.so"))
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _capi.SIGNATURES, f"{name} is not bound"
    for name in ("segmap_mask", "segmap_union", "segmap_label", "label_tile", "label_scan_span"):
        assert callable(getattr(kernels, name))
    for name in ("segmap_gauss", "merged_labels"):
        assert callable(getattr(segmap, name))
    assert "compute_segmap_gauss" in lib_origin.__all__
    # the SciPy restatement has left the product
    assert not hasattr(steps, "compute_segmap_gauss") and not hasattr(steps, "fftconvolve")


def test_tile_query_and_shape_classes(geometry):
    tw, th, span = geometry
    assert tw >= 2 and th >= 2 and span >= tw * th
    shapes = cases.label_shapes(tw, th, span)
    assert shapes["one_pixel"] == (1, 1)
    ny, nx = shapes["one_row"]
    assert ny == 1 and tw < nx <= 2 * tw                    # two tiles side by side, one seam
    ny, nx = shapes["one_column"]
    assert nx == 1 and th < ny <= 2 * th
    assert shapes["one_tile"] == (th, tw)
    ny, nx = shapes["below_a_tile"]
    assert ny < th and nx < tw
    ny, nx = shapes["many_tiles"]                           # several tiles, ragged last ones
    assert ny > 2 * th and ny % th and nx > 2 * tw and nx % tw
    ny, nx = shapes["two_scan_passes"]
    assert ny * nx > span
    assert all(ny <= 300 and nx <= 300 for ny, nx in shapes.values())
    (ay, ax), (by, bx) = cases.mask_shapes(tw, th).values()  # one each side of a tile's edge
    assert ay == th - 1 and by == th + 1 and ax == tw + 1 and bx > 2 * tw and bx % tw


@pytest.mark.parametrize("shape_name", ["one_pixel", "one_row", "one_column", "one_tile",
                                        "below_a_tile", "many_tiles", "two_scan_passes"])
def test_label_patterns_are_what_they_claim(geometry, shape_name):
    Ny, Nx = cases.label_shapes(*geometry)[shape_name]
    count = {k: ndi.label(f(Ny, Nx))[1] for k, f in cases.LABEL_PATTERNS.items()}
    for k, f in cases.LABEL_PATTERNS.items():
        m = f(Ny, Nx)
        assert m.shape == (Ny, Nx) and m.dtype == bool, k
        assert np.array_equal(m, f(Ny, Nx)), f"{k} is not reproducible"
    assert count["zeros"] == 0 and count["ones"] == 1
    assert count["serpentine"] == 1 and count["comb"] == 1 and count["spiral"] == 1
    assert count["checkerboard"] == (Ny * Nx + 1) // 2
    assert count["rows"] == (Ny + 1) // 2 and count["columns"] == (Nx + 1) // 2
    assert count["rings"] == cases.rings_count(Ny, Nx)
    if Ny * Nx > 500:
        dens = [cases.LABEL_PATTERNS[k](Ny, Nx).mean() for k in
                ("random_0.3", "random_0.5", "random_0.593", "random_0.8")]
        assert np.allclose(dens, (0.3, 0.5, 0.593, 0.8), atol=0.05)
        # the serpentine passes through every row, the comb's teeth meet in the last row only
        assert cases.LABEL_PATTERNS["serpentine"](Ny, Nx).any(axis=1).all()
        assert ndi.label(cases.LABEL_PATTERNS["comb"](Ny, Nx)[:-1])[1] == (Nx + 1) // 2


def test_mask_patterns_are_what_they_claim(geometry):
    tw, th, _ = geometry
    for Ny, Nx in cases.mask_shapes(tw, th).values():
        st = {k: oracle.mask_stages(f(Ny, Nx), cases.GAMMA) for k, f in cases.MASK_PATTERNS.items()}
        m0, m1, m2, _ = st["borders"]
        # a blob on every border and corner survives there (outside counts as 1 for the erosion)
        for edge in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
            assert m2[edge].any()
        assert m2[0, 0] and m2[0, -1] and m2[-1, 0] and m2[-1, -1]
        assert m0[0, 8:12].all() and not m2[0, 8:12].any()       # the thin strips do not
        m0, m1, m2, _ = st["specks"]
        assert m0[5, 5] and m0[9, 9:11].all() and m0[14:16, 20].all() and m0[-1, -1]
        assert m1.sum() == 1 and m1[19, 5] and m2.sum() == 5     # only the square's centre stays
        m0, m1, m2, _ = st["cross"]
        assert m0.sum() == 25 and m1.sum() == 5 and np.array_equal(m2, m0)
        d = cases.MASK_PATTERNS["nonfinite"](Ny, Nx)
        m0 = st["nonfinite"][0]
        assert not m0[np.isnan(d)].any() and not m0[d == -np.inf].any() and m0[d == np.inf].all()
        assert np.isnan(d).sum() >= 3 and (d == -np.inf).sum() >= 3
        d = cases.MASK_PATTERNS["equal_gamma"](Ny, Nx)
        m0 = st["equal_gamma"][0]
        assert (d == cases.GAMMA).sum() == 2 and not m0[d == cases.GAMMA].any()
        assert m0[20, 8] and not m0[22, 11]
        d = cases.MASK_PATTERNS["everything"](Ny, Nx)
        assert np.isnan(d).any() and (d == -np.inf).any() and (d == cases.GAMMA).any()
    # f of the disc: 0 (empty), 1 (identity), 2 (3 x 3 square), 5 (without the 3-4-5 offsets)
    m = np.zeros((21, 21), bool)
    m[10, 10] = True
    disc = lambda fw: fftconvolve_disc(m, fw)
    assert not disc(1).any() and np.array_equal(disc(2), m) and np.array_equal(disc(3), m)
    assert disc(4).sum() == 9 and disc(4)[9:12, 9:12].all()
    assert np.array_equal(disc(10), disc(11)) and disc(10)[10, 14] and disc(10)[13, 13]
    assert not disc(10)[13, 14] and not disc(10)[14, 13] and not disc(10)[10, 15]


def fftconvolve_disc(mask, fwhm_fsf):
    """The disc stage of the oracle alone (a mask that erosion and dilation would change)."""
    from scipy.signal import fftconvolve
    f = int(fwhm_fsf) // 2
    disc = np.hypot(*list(np.mgrid[:2 * f + 1, :2 * f + 1] - f)) < f
    return fftconvolve(mask, disc, mode='same') > 1e-9


def test_oracle_is_pinned_to_the_reference():
    with np.load(GOLDEN) as g:
        names = sorted(k[:-5] for k in g.files if k.endswith("_data"))
        assert len(names) == 3
        assert sorted(int(g[n + "_fwhm_fsf"]) for n in names) == [0, 3, 4]
        assert sorted(float(g[n + "_pfa"]) for n in names) == [1e-5, 0.01, 0.01]
        for n in names:
            data, gamma, want = g[n + "_data"], float(g[n + "_gamma"]), g[n + "_labels"]
            assert data.shape[0] <= 96 and data.shape[1] <= 128 and want.dtype == np.int32
            assert want.max() >= 5 and np.min(np.abs(data - gamma)) > 1e-6 * abs(gamma)
            for edge in (want[0], want[-1], want[:, 0], want[:, -1]):
                assert edge.any()
            got, ngot = oracle.labels_at(data, gamma, int(g[n + "_fwhm_fsf"]))
            assert ngot == want.max() and np.array_equal(got, want)
            # and the whole function with the product's host fit
            gam2, lab2 = oracle.compute_segmap_gauss(data, float(g[n + "_pfa"]),
                                                     int(g[n + "_fwhm_fsf"]))
            np.testing.assert_allclose(gam2, gamma, rtol=1e-10)
            assert np.array_equal(lab2, want)
