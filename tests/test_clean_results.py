"""Step 9 (origin_amd/catalog.py) and the Step classes of steps 7-9 (origin_amd/steps.py).

CPU: ``catalog.merge_similar_lines`` / ``unique_sources`` / ``add_tglr_stat`` against the
reference's own outputs in tests/golden/g13_clean.npz (tools/gen_clean_golden.py: every case at
``z_pix_threshold`` 5 and 3).  Integer, bool and string columns equal; float columns within 1e-13
relative (sums of at most a few hundred float64 terms on both sides), NaN where the reference has
NaN.  The reference leaves the order of rows with equal ``(ID, z)`` open, so both sides are
ordered by ``(ID, z, num_line)`` first; the package's own order, ``(ID, z, input row)``, is
asserted separately.  Then the documented deviations, the table file format and the Step seam.

GPU: the chain ``step07_detection`` -> ``step08_compute_spectra`` -> ``step09_clean_results`` on
a small session, its dump / load, and the function seam of ``lib_origin.add_tglr_stat``.
"""
import os
from collections import OrderedDict

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FRTOL = 1e-13
REFERENCE_FIRST_NINE = [
    ("Preprocessing", "preprocessing"), ("CreateAreas", "areas"),
    ("ComputePCAThreshold", "compute_PCA_threshold"), ("ComputeGreedyPCA", "compute_greedy_PCA"),
    ("ComputeTGLR", "compute_TGLR"), ("ComputePurityThreshold", "compute_purity_threshold"),
    ("Detection", "detection"), ("ComputeSpectra", "compute_spectra"),
    ("CleanResults", "clean_results")]


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "g13_clean.npz"))
    return {k: z[k] for k in z.files}


def _names(a):
    return [s.decode() for s in a]


def case_ids():
    z = np.load(os.path.join(GOLDEN, "g13_clean.npz"))
    return [(i, int(t)) for i in range(len(z["names"])) for t in z["thresholds"]]


def same_column(got, want, name):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, name
    if want.dtype.kind == "S":
        assert got.dtype.kind == "U" and [s for s in got] == _names(want), name
    elif want.dtype.kind == "b":
        assert got.dtype == bool and np.array_equal(got, want), name
    elif want.dtype.kind == "i":
        assert got.dtype.kind in "iu" and np.array_equal(got, want), name
    else:
        assert got.dtype == np.float64, name
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        ok = ~np.isnan(want)
        assert np.all(np.abs(got[ok] - want[ok]) <= FRTOL * np.abs(want[ok])), name


# ------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("case,thr", case_ids())
def test_catalog_matches_the_reference(golden, case, thr):
    from origin_amd import catalog
    cat2 = OrderedDict((k, golden[f"c{case}_in_{k}"]) for k in _names(golden["input_columns"]))
    before = {k: v.copy() for k, v in cat2.items()}
    lines = catalog.merge_similar_lines(cat2, z_pix_threshold=thr)
    src = catalog.unique_sources(lines)
    src = catalog.add_tglr_stat(src, lines, np.std(golden["cube_correl"]),
                                np.std(golden["cube_std"]))
    assert all(np.array_equal(cat2[k], before[k], equal_nan=True) for k in before)  # input intact
    # the package's own row order: (ID, z, input row); num_line is the input row + 1
    n = len(lines["ID"])
    assert np.array_equal(np.lexsort((lines["num_line"], lines["z"], lines["ID"])), np.arange(n))
    pre = f"c{case}_t{thr}_"
    assert list(lines) == _names(golden[pre + "lines_columns"])
    assert list(src) == _names(golden[pre + "src_columns"])
    ref_order = np.lexsort((golden[pre + "lines_num_line"], golden[pre + "lines_z"],
                            golden[pre + "lines_ID"]))
    for k in lines:
        same_column(lines[k], golden[pre + "lines_" + k][ref_order], f"lines.{k}")
    assert np.all(np.diff(src["ID"]) > 0)
    for k in src:
        same_column(src[k], golden[pre + "src_" + k], f"sources.{k}")


def test_fixture_holds_the_cases_the_tables_must_survive(golden):
    """The fixture is what it says: a merged pair and a split pair at the threshold, a chain that
    percolates, NaN maxima for a source mixing comp 0 and 1, rows with equal (ID, z)."""
    names = _names(golden["names"])
    i = names.index("pair_gap_below_and_at_threshold")
    ids, merged = golden[f"c{i}_t5_lines_ID"], golden[f"c{i}_t5_lines_merged_in"]
    assert np.sum(merged[ids == 3] != -9999) == 1 and np.all(merged[ids == 5] == -9999)
    i = names.index("percolating_chain")
    assert np.all(golden[f"c{i}_t5_lines_line_merged_flag"])
    assert not np.any(golden[f"c{i}_t3_lines_line_merged_flag"])
    i = names.index("mixed_comp_source")
    row = list(golden[f"c{i}_t5_src_ID"]).index(17)
    assert np.isnan(golden[f"c{i}_t5_src_T_GLR"][row]) and np.isnan(golden[f"c{i}_t5_src_STD"][row])
    i = names.index("equal_z")
    z = golden[f"c{i}_in_z"][golden[f"c{i}_in_ID"] == 20]
    assert len(z) == 2 and z[0] == z[1]
    i = names.index("five_unmerged_lines")
    assert golden[f"c{i}_t5_src_waves"][0].decode().count(",") == 2
    i = names.index("random_300")
    assert len(golden[f"c{i}_in_ID"]) == 300 and len(np.unique(golden[f"c{i}_in_ID"])) == 60


def hand_table(ids, z, flux, with_wcs=False):
    n = len(ids)
    cat = OrderedDict(ID=np.array(ids, np.int64), x=np.arange(n, dtype=np.int64) * 2,
                      y=np.arange(n, dtype=np.int64) * 3 + 1, z=np.array(z, np.int64),
                      comp=np.zeros(n, np.int64), STD=np.full(n, np.nan),
                      T_GLR=np.linspace(5.0, 9.0, n), seg_label=np.array(ids, np.int64) % 3,
                      purity=np.linspace(0.6, 1.0, n), flux=np.array(flux, float),
                      num_line=np.arange(1, n + 1))
    if with_wcs:
        cat["ra"], cat["dec"] = np.linspace(1, 2, n), np.linspace(-2, -1, n)
        cat["lbda"] = 4800.0 + 1.25 * cat["z"]
    return cat


def test_deviation_1_equal_id_and_z_keep_the_input_order():
    from origin_amd import catalog
    cat = hand_table([4, 4, 4, 2], [50, 50, 50, 9], [1.0, 3.0, 2.0, 5.0])
    lines = catalog.merge_similar_lines(cat)
    assert lines["num_line"].tolist() == [4, 1, 2, 3]
    assert lines["merged_in"].tolist() == [-9999, 2, -9999, 2]
    assert lines["line_merged_flag"].tolist() == [False, True, True, True]


def test_deviation_2_zero_flux_sum_takes_the_unweighted_mean():
    from origin_amd import catalog
    cat = hand_table([1, 2, 2], [10, 20, 200], [0.0, 2.0, -2.0])     # a fallback row; a sum of 0
    src = catalog.unique_sources(catalog.merge_similar_lines(cat))
    assert src["ID"].tolist() == [1, 2] and src["n_lines"].tolist() == [1, 2]
    assert src["x"].tolist() == [0.0, 3.0] and src["y"].tolist() == [1.0, 5.5]


def test_deviation_3_empty_cat2_gives_empty_tables():
    from origin_amd import catalog
    cat = hand_table([], [], [], with_wcs=True)
    lines = catalog.merge_similar_lines(cat)
    src = catalog.add_tglr_stat(catalog.unique_sources(lines), lines, 2.0, 3.0)
    assert list(lines)[-4:] == ["line_merged_flag", "merged_in", "nsigTGLR", "nsigSTD"]
    assert list(src) == ["ID", "ra", "dec", "x", "y", "n_lines", "seg_label", "comp",
                         "line_merged_flag", "waves", "flux", "STD", "nsigSTD", "T_GLR",
                         "nsigTGLR", "purity"]
    assert all(len(v) == 0 for v in lines.values()) and all(len(v) == 0 for v in src.values())
    assert lines["line_merged_flag"].dtype == bool and lines["merged_in"].dtype == np.int64


def test_deviation_4_without_wcs_columns_the_derived_ones_are_left_out():
    from origin_amd import catalog
    cat = hand_table([1, 1, 3], [10, 12, 20], [1.0, 3.0, 2.0])
    lines = catalog.merge_similar_lines(cat)
    src = catalog.add_tglr_stat(catalog.unique_sources(lines), lines, 2.0, 4.0)
    assert list(src) == ["ID", "x", "y", "n_lines", "seg_label", "comp", "line_merged_flag",
                         "flux", "STD", "nsigSTD", "T_GLR", "nsigTGLR", "purity"]
    assert src["x"].tolist() == [(0 * 1.0 + 2 * 3.0) / 4.0, 4.0]
    assert np.array_equal(lines["nsigTGLR"], lines["T_GLR"] / 2.0)
    assert np.all(np.isnan(lines["nsigSTD"])) and np.all(np.isnan(src["STD"]))
    assert src["T_GLR"].tolist() == [7.0, 9.0] and src["n_lines"].tolist() == [1, 1]
    with_wcs = hand_table([1, 1, 3], [10, 12, 20], [1.0, 3.0, 2.0], with_wcs=True)
    src = catalog.unique_sources(catalog.merge_similar_lines(with_wcs))
    assert src["waves"].tolist() == ["4815", "4825"]


def test_table_files_learn_bool_and_string_columns_and_header_cards(tmp_path):
    from origin_amd import fitsio
    cols = OrderedDict(ID=np.array([3, 1, 2]), x=np.array([0.5, np.nan, -2.0]),
                       line_merged_flag=np.array([True, False, True]),
                       waves=np.array(["4815,5003,6120", "", "7001"]),
                       raw=np.array([b"ab", b"c", b""]))
    p = fitsio.write_table(str(tmp_path / "t.fits"), cols,
                           header={"CAT3_TS": "2024-05-06T07:08:09.123456", "NCASE": 3})
    assert os.path.getsize(p) % 2880 == 0
    meta = {}
    back = fitsio.read_table(p, header=meta)
    assert list(back) == list(cols)
    assert back["ID"].dtype == np.int64 and np.array_equal(back["ID"], cols["ID"])
    assert np.array_equal(back["x"], cols["x"], equal_nan=True)
    assert back["line_merged_flag"].dtype == bool
    assert np.array_equal(back["line_merged_flag"], cols["line_merged_flag"])
    assert back["waves"].dtype.kind == "U" and back["waves"].tolist() == cols["waves"].tolist()
    assert back["raw"].tolist() == ["ab", "c", ""]
    assert meta["CAT3_TS"] == "2024-05-06T07:08:09.123456" and meta["NCASE"] == 3
    assert not any(k.startswith(("TTYPE", "TFORM", "NAXIS")) for k in meta)
    hdr = [h for h, _, _ in fitsio.scan(p)][1]
    assert hdr["TFORM3"] == "L" and hdr["TFORM4"] == "14A" and hdr["NAXIS1"] == 8 + 8 + 1 + 14 + 2
    assert list(fitsio.read_table(p)) == list(cols)            # header= is optional
    with pytest.raises(ValueError):
        fitsio.write_table(str(tmp_path / "u.fits"), cols, header={"NAXIS2": 5})
    empty = OrderedDict(ID=np.zeros(0, np.int64), waves=np.zeros(0, "U1"), f=np.zeros(0, bool))
    back = fitsio.read_table(fitsio.write_table(str(tmp_path / "e.fits"), empty))
    assert [len(v) for v in back.values()] == [0, 0, 0] and back["f"].dtype == bool


def test_golden_table_file_reads_as_before():
    from oracle import fits_ref
    from origin_amd import fitsio
    path = os.path.join(GOLDEN, "g9_table.fits")
    ours, ref = fitsio.read_table(path), fits_ref.read_table(path)
    arrays = np.load(os.path.join(GOLDEN, "g9_arrays.npz"))
    assert list(ours) == ["Tval_r", "Pval_r", "Det_m", "Det_M"]
    for k in ours:
        assert ours[k].dtype == arrays["table_" + k].dtype
        assert np.array_equal(ours[k], ref[k]) and np.array_equal(ours[k], arrays["table_" + k])
    for name in os.listdir(GOLDEN):
        if name.startswith("g9_") and name.endswith(".fits"):
            assert len(fitsio.scan(os.path.join(GOLDEN, name))) == 2, name


def test_spectra_file_round_trip(tmp_path):
    from origin_amd import steps
    spectra = OrderedDict([(7, (np.arange(5.0), np.ones(5), 12)), (2, (np.zeros(3), np.ones(3), 0))])
    p = str(tmp_path / "spectra.npz")
    steps.write_spectra(p, spectra)
    back = steps.read_spectra(p)
    assert list(back) == [7, 2] and back[7][2] == 12 and back[2][2] == 0
    assert all(np.array_equal(back[k][i], spectra[k][i]) for k in spectra for i in (0, 1))


def _dummy_session():
    """A session that never touches the device: enough for the Step machinery."""
    from origin_amd.steps import SimpleOrig
    cube = np.zeros((4, 3, 5))
    return SimpleOrig(cube, cube + 1, None, None, None, ctx=object())


def test_steps_are_the_first_nine_of_the_reference():
    from origin_amd import steps
    assert [(c.__name__, c.name) for c in steps.STEPS] == REFERENCE_FIRST_NINE
    # steps 7-9 of a session are made at their first use (method, output or steps[name]), in
    # STEPS order whatever the order of use; a session that stops at step 6 lists the six
    orig = _dummy_session()
    assert [s.name for s in orig.steps.values()] == [n for _, n in REFERENCE_FIRST_NINE[:6]]
    assert "detection" not in orig.param
    assert orig.step09_clean_results.method_name == "step09_clean_results"
    assert orig.Cat1 is None and orig.steps["compute_spectra"].idx == 8
    assert [s.method_name for s in orig.steps.values()][6:] == [
        "step07_detection", "step08_compute_spectra", "step09_clean_results"]
    assert orig.param["detection"]["stepidx"] == 7
    with pytest.raises(KeyError):
        orig.steps["create_masks"]
    with pytest.raises(AttributeError):
        orig.step10_create_masks
    assert orig.step07_detection.require is None
    assert orig.step08_compute_spectra.require == ("detection",)
    assert orig.step09_clean_results.require == ("compute_spectra",)
    assert [n for n, _ in steps.Detection._dataobjs] == ["Cat0", "Cat1", "segmap_label"]
    assert steps.ComputeSpectra._dataobjs == [("Cat2", "table"), ("spectra", "spectra")]
    assert steps.CleanResults._dataobjs == [("Cat3_lines", "table"), ("Cat3_sources", "table")]
    assert (steps.Detection.desc, steps.ComputeSpectra.desc, steps.CleanResults.desc) == (
        "Thresholding and spatio-spectral merging", "Lines estimation", "Results cleaning")
    import inspect
    sig = {c: [(k, p.default) for k, p in inspect.signature(c.run).parameters.items()][2:]
           for c in steps.STEPS[6:]}
    assert sig[steps.Detection] == [("threshold", None), ("threshold_std", None), ("tol_spat", 3),
                                    ("tol_spec", 5), ("maxdist_lines", 2.5), ("segmap", None)]
    assert sig[steps.ComputeSpectra] == [("grid_dxy", 0), ("spectrum_size_fwhm", 6)]
    assert sig[steps.CleanResults] == [("merge_lines_z_threshold", 5)]


def test_require_blocks_step09_before_step08():
    from origin_amd.steps import Status
    orig = _dummy_session()
    with pytest.raises(RuntimeError, match="^step 08 must be run before$"):
        orig.step09_clean_results()
    assert orig.steps["clean_results"].status is Status.NOTRUN
    with pytest.raises(RuntimeError, match="^step 07 must be run before$"):
        orig.step08_compute_spectra()
    assert orig.param["clean_results"]["params"] == {"merge_lines_z_threshold": 5}


def test_session_threshold_properties_and_shape():
    orig = _dummy_session()
    assert orig.shape == (4, 3, 5)
    assert orig.threshold_correl is None and orig.threshold_std is None
    orig.threshold_correl, orig.threshold_std = 7.5, 3.25
    assert orig.param["threshold"] == 7.5 and orig.param["threshold_std"] == 3.25
    assert orig.FWHM_profiles is None


# ------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ctx():
    from origin_amd.device import default_context
    return default_context(0)


def tables_equal(a, b, rtol_cols=()):
    assert list(a) == list(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, k
        if k in rtol_cols:
            assert np.array_equal(np.isnan(x), np.isnan(y)), k
            ok = ~np.isnan(y)
            assert np.all(np.abs(x[ok] - y[ok]) <= 1e-12 * np.abs(y[ok])), k
        elif x.dtype.kind in "US":
            assert x.tolist() == y.tolist(), k
        else:
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), k


@pytest.fixture(scope="module")
def chain(ctx):
    """Steps 1-9 on the small session of test_lines.py::test_from_session_after_steps_1_to_7."""
    from origin_amd import synth
    from origin_amd.steps import SimpleOrig
    f, raw, var, mask = synth.small_case(Nz=160, Ny=48, Nx=52, seed=3, psf_size=9, nprof=3,
                                         area_size=24)
    fwhm = [2.0, 4.1, 7.0]

    def session():
        return SimpleOrig(raw, var, mask, f.PSF.astype(float), f.profiles, ctx=ctx,
                          FWHM_profiles=fwhm)
    orig = session()
    orig.step01_preprocessing()
    orig.step02_areas.set_areamap(f.areamap)
    orig.step03_compute_PCA_threshold()
    orig.step04_compute_greedy_PCA()
    orig.step05_compute_TGLR()
    orig.step06_compute_purity_threshold(purity=0.8)
    # the purity curve of so small a cube may be degenerate: curves by hand for step 7
    t = np.linspace(0.0, 50.0, 11)
    orig.steps["compute_purity_threshold"].Pval = dict(Tval_r=t, Pval_r=np.clip(t / 20, 0, 1))
    orig.steps["compute_purity_threshold"].Pval_comp = dict(Tval_r=t, Pval_r=np.clip(t / 10, 0, 1))
    lmax = orig.cube_local_max._data
    smax = orig.cube_std_local_max._data
    t_cor = float(np.sort(lmax[lmax > 0])[-12])
    t_std = float(np.sort(smax[smax > 0])[-12])
    orig.step07_detection(threshold=t_cor, threshold_std=t_std)
    orig.step08_compute_spectra()
    orig.step09_clean_results()
    return dict(orig=orig, session=session, t_cor=t_cor, t_std=t_std, fwhm=fwhm, raw=raw)


@pytest.mark.gpu
def test_step_chain_7_to_9(chain):
    from origin_amd import catalog, detection, lines
    from origin_amd.steps import Status
    orig = chain["orig"]
    assert len(orig.steps) == 9 and all(s.status is Status.RUN for s in orig.steps.values())
    assert orig.param["threshold"] == chain["t_cor"] == orig.threshold_correl
    assert orig.param["threshold_std"] == chain["t_std"] == orig.threshold_std
    assert orig.param["detection"]["params"]["tol_spec"] == 5
    cat0 = detection.from_session(orig)[0]
    tables_equal(orig.Cat0, cat0)
    cat1 = detection.cat1_from_session(orig)
    assert 5 <= len(cat1["ID"]) <= 40
    tables_equal(orig.Cat1, cat1)
    assert np.array_equal(orig.segmap_label, np.asarray(orig.segmap_cont))
    cat2, lin, lvar = lines.from_session(orig, cat1)
    tables_equal(orig.Cat2, cat2)
    # spectra: z +- ceil(FWHM * 6 / 2) clipped to the cube, fallback rows left out
    radius = np.ceil(np.array(chain["fwhm"]) * 6 / 2).astype(int)
    Nz = chain["raw"].shape[0]
    kept = [i for i in range(len(lin)) if len(lin[i]) > 1]
    assert list(orig.spectra) == [int(cat2["num_line"][i]) for i in kept] and kept
    for i in kept:
        data, var, z_min = orig.spectra[int(cat2["num_line"][i])]
        z, r = int(cat2["z"][i]), int(radius[cat2["profile"][i]])
        lo, hi = max(z - r, 0), min(z + r, Nz - 1)
        assert z_min == lo and len(data) == len(var) == hi - lo + 1
        assert np.array_equal(data, lin[i][lo:hi + 1]) and np.array_equal(var, lvar[i][lo:hi + 1])
    # step 9 = catalog.clean_results fed with np.std of the host cubes
    lines3 = catalog.merge_similar_lines(cat2)
    src3 = catalog.add_tglr_stat(catalog.unique_sources(lines3), lines3,
                                 np.std(orig.cube_correl._data), np.std(orig.cube_std._data))
    nsig = ("nsigTGLR", "nsigSTD")
    tables_equal(orig.Cat3_lines, lines3, nsig)
    tables_equal(orig.Cat3_sources, src3, nsig)
    assert len(src3["ID"]) == len(np.unique(cat2["ID"])) >= 2
    assert orig.Cat3_lines.meta["CAT3_TS"] == orig.Cat3_sources.meta["CAT3_TS"]
    assert orig.Cat3_lines.meta["CAT3_TS"][:2] == "20"
    zm = orig.steps["detection"].det_correl_min(chain["t_cor"])
    want = np.where(orig.cube_local_min._data > chain["t_cor"])
    assert all(np.array_equal(a, b) for a, b in zip(zm, want))


@pytest.mark.gpu
def test_segmap_override_is_shape_checked(chain):
    orig = chain["orig"]
    with pytest.raises(ValueError, match="segmap does not have the same shape"):
        orig.steps["detection"].run(orig, segmap=np.zeros((5, 5), int))


@pytest.mark.gpu
def test_dump_and_load_into_a_fresh_session(chain, tmp_path):
    from origin_amd.steps import Status
    orig = chain["orig"]
    want = {n: OrderedDict(getattr(orig, n)) for n in ("Cat0", "Cat1", "Cat2", "Cat3_lines",
                                                       "Cat3_sources")}
    ts = orig.Cat3_lines.meta["CAT3_TS"]
    spectra = OrderedDict(orig.spectra)
    seg = np.array(orig.segmap_label)
    out = str(tmp_path)
    last = list(orig.steps.values())[6:]
    for step in last:
        step.dump(out)
        assert step.status is Status.DUMPED
    assert os.path.isfile(f"{out}/Cat3_sources.fits") and os.path.isfile(f"{out}/spectra.npz")
    fresh = chain["session"]()
    for name in ("detection", "compute_spectra", "clean_results"):
        fresh.steps[name].status = Status.DUMPED
        fresh.steps[name].load(out)
    for n, tab in want.items():
        tables_equal(getattr(fresh, n), tab)
    assert fresh.Cat3_lines.meta["CAT3_TS"] == ts == fresh.Cat3_sources.meta["CAT3_TS"]
    assert fresh.Cat3_lines["line_merged_flag"].dtype == bool
    assert list(fresh.spectra) == list(spectra)
    for k, (data, var, z_min) in spectra.items():
        got = fresh.spectra[k]
        assert np.array_equal(got[0], data) and np.array_equal(got[1], var) and got[2] == z_min
    assert np.array_equal(np.asarray(fresh.segmap_label._data), seg)
    # (the shared session reads its own outputs back from the same files from here on)
    tables_equal(orig.Cat3_sources, want["Cat3_sources"])


@pytest.mark.gpu
def test_lib_origin_add_tglr_stat_takes_host_and_device_cubes(ctx, golden):
    import origin_amd.lib_origin as hip
    from origin_amd.steps import LazyCube
    i = _names(golden["names"]).index("random_300")
    cat2 = OrderedDict((k, golden[f"c{i}_in_{k}"]) for k in _names(golden["input_columns"]))
    correl, std = golden["cube_correl"], golden["cube_std"]
    d_correl, d_std = ctx.to_device(correl, np.float32), ctx.to_device(std, np.float32)
    out = []
    for a, b in ((correl, std), (d_correl, d_std), (LazyCube(d_correl), LazyCube(host=std))):
        lines = hip.merge_similar_lines(cat2, z_pix_threshold=5)
        src = hip.add_tglr_stat(hip.unique_sources(lines), lines, a, b)
        out.append((lines, src))
    for lines, src in out[1:]:
        tables_equal(lines, out[0][0])
        tables_equal(src, out[0][1])
    # against the reference's tables: its cubes are float64, ours their float32 roundings e, and
    # |std(a + e) - std(a)| <= rms(e) <= max |e|
    pre = f"c{i}_t5_"
    got = out[0][1]
    for k, cube in (("nsigTGLR", correl), ("nsigSTD", std)):
        tol = np.max(np.abs(cube.astype(np.float32) - cube)) / np.std(cube) + 1e-12
        want = golden[pre + "src_" + k]
        ok = ~np.isnan(want)
        assert np.array_equal(np.isnan(got[k]), ~ok)
        assert np.all(np.abs(got[k][ok] - want[ok]) <= tol * np.abs(want[ok])), k
