"""Spatio-spectral merging of step 7 (origin_amd/detection.py, csrc/merge.hip) against
tests/_merge_oracle.py, the NumPy restatement that tools/gen_merge_golden.py pins to the
reference's own spatiospectral_merging / purity_estimation (tests/golden/g12_merging.npz).

Every comparison of the merging is exact integer equality: there is no tolerance.  The fixture
holds, in input row order: two rows; 300 rows in one spaxel; offsets on the near / far / dz
thresholds for tol_spat 3, 2, 4 and tol_spec 5.5; a chain of 1500 rows with later seeds beside it;
two seeds that reach the same rows, in both row orders; 1200 isolated detections; the stage-2
patterns (area 0, a group over two labels, the non-transitive walk, dz = 0, the last bitmap word,
200 groups in one label); one component of 5000 rows in a 40 x 40 field (the reference needs 3.4 s
for it).  n = 0 and n = 1 are checked against the oracle only.
"""
import os

import numpy as np
import pytest

import _merge_oracle as oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_merging.npz")
OUT = ("area", "imatch2", "imatch")
NAMES = ["n2", "one_spaxel", "thresholds_3_5", "thresholds_2_5", "thresholds_4_5",
         "thresholds_3_5.5", "chain", "two_seeds", "two_seeds_swapped", "isolated", "stage2",
         "crowded"]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def golden_case(g, i):
    k = f"c{i}_"
    tol_spat, tol_spec = (float(v) for v in g[k + "tol"])
    return dict(x=g[k + "x"], y=g[k + "y"], z=g[k + "z"], area=g[k + "area"], tol_spat=tol_spat,
                tol_spec=tol_spec, shape=tuple(int(v) for v in g[k + "shape"]),
                out={o: g[k + "out_" + o] for o in OUT})


@pytest.fixture(scope="module")
def random_refs():
    """The oracle on the random fields, computed once per seed."""
    cache = {}

    def get(seed):
        if seed not in cache:
            c = oracle.random_field(seed)
            cache[seed] = (c, oracle.merge(c["x"], c["y"], c["z"], c["area"], c["tol_spat"],
                                           c["tol_spec"]))
        return cache[seed]
    return get


# ------------------------------------------------------------------------------------ not gpu
def test_fixture_holds_every_case(golden):
    assert list(golden["names"]) == NAMES
    assert os.path.getsize(GOLDEN) < 300 * 1024


@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_restatement_equals_the_reference_fixture(golden, i):
    c = golden_case(golden, i)
    got = oracle.merge(c["x"], c["y"], c["z"], c["area"], c["tol_spat"], c["tol_spec"])
    for o in OUT:
        assert np.array_equal(got[o], c["out"][o]), o


def test_fixture_decides_the_designed_cases(golden):
    """What the cases were built to show, read off the reference's own answers."""
    c = golden_case(golden, NAMES.index("one_spaxel"))
    assert len(np.unique(c["out"]["imatch"])) == 1
    c = golden_case(golden, NAMES.index("chain"))
    assert np.bincount(c["out"]["imatch2"]).max() > 1024          # deeper than any workgroup
    assert len(np.unique(c["out"]["imatch2"])) > 400              # and the later seeds beside it
    a = golden_case(golden, NAMES.index("two_seeds"))["out"]["imatch2"]
    b = golden_case(golden, NAMES.index("two_seeds_swapped"))["out"]["imatch2"]
    assert np.bincount(a).tolist() == np.bincount(b).tolist() == [5, 2]
    assert a[0] == 0 and a[1] == 1 and b[0] == 0 and b[1] == 1   # the lower seed row wins
    c = golden_case(golden, NAMES.index("isolated"))
    assert np.array_equal(c["out"]["imatch2"], np.arange(1200))
    c = golden_case(golden, NAMES.index("stage2"))
    zero = c["out"]["area"] == 0
    assert np.array_equal(c["out"]["imatch"][zero], c["out"]["imatch2"][zero])
    assert not np.array_equal(c["out"]["imatch"], c["out"]["imatch2"])
    c = golden_case(golden, NAMES.index("crowded"))
    assert len(c["x"]) == 5000 and len(np.unique(oracle.components(c["x"], c["y"], 3))) == 1


def test_oracle_on_empty_and_single_tables():
    for n in (0, 1):
        c = oracle.case_small(n)
        got = oracle.merge(c["x"], c["y"], c["z"], c["area"], 3, 5)
        for o in OUT:
            assert got[o].shape == (n,)
        if n:
            assert got["imatch"][0] == 0 and got["area"][0] == 2


def test_purity_equals_the_reference_fixture(golden):
    from origin_amd import detection, lib_origin
    p = {k[7:]: golden[k] for k in golden.files if k.startswith("purity_")}
    ref = p["out"]
    assert np.isnan(ref).sum() == 2 and ref[~np.isnan(ref)].min() == 0 and np.nanmax(ref) == 1
    cat = dict(comp=p["comp"], T_GLR=p["T_GLR"], STD=p["STD"])
    tabs = (dict(Tval_r=p["Tval"], Pval_r=p["Pval"]),
            dict(Tval_r=p["Tval_comp"], Pval_r=p["Pval_comp"]))
    for got in (oracle.purity(p["comp"], p["T_GLR"], p["STD"], p["Tval"], p["Pval"],
                              p["Tval_comp"], p["Pval_comp"]),
                detection.purity_estimation(cat, *tabs),
                lib_origin.purity_estimation(cat, *tabs)["purity"]):
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.nanmax(np.abs(got - ref)) <= 1e-15


@pytest.mark.parametrize("tol_spat", [2, 3, 4, 2.5])
def test_predicate_tables_are_numpy_hypot(tol_spat):
    from origin_amd import kernels
    near, far = kernels.merge_predicate_tables(tol_spat)
    R = near.shape[0]
    assert near.shape == far.shape == (R, R) and near.dtype == far.dtype == np.uint8
    assert R == int(np.ceil(tol_spat * np.sqrt(2))) + 2
    for a in range(R + 6):
        for b in range(R + 6):
            n = bool(np.hypot(a, b) < tol_spat)
            f = bool(np.hypot(a, b) > tol_spat * np.sqrt(2))
            if a < R and b < R:
                assert near[a, b] == n and far[a, b] == f, (a, b)
            else:                                       # beyond the tables: not near, far
                assert not n and f, (a, b)
    t = int(tol_spat)
    if t == tol_spat:                                   # the tie on the diagonal is NumPy's answer
        assert far[t, t] == (np.hypot(t, t) > t * np.sqrt(2))


def fake_cat(c, rng):
    n = len(c["x"])
    comp = (rng.random(n) < 0.3).astype(int)
    return dict(x0=c["x"], y0=c["y"], z0=c["z"], comp=comp,
                STD=np.where(comp == 1, rng.uniform(0, 8, n), np.nan),
                T_GLR=np.where(comp == 0, rng.uniform(3, 13, n), np.nan),
                profile=rng.integers(0, 5, n).astype(np.uint8))


PVAL = dict(Tval_r=np.linspace(4, 12, 9), Pval_r=np.linspace(0.2, 1.0, 9))
PVAL_COMP = dict(Tval_r=np.linspace(1, 7, 7), Pval_r=np.linspace(0.0, 0.9, 7))


def check_cat1(cat1, cat, seg, ref):
    """``cat1`` against the input table ``cat`` (correl rows then std rows), the segmap and the
    oracle's answer for those rows."""
    n = len(cat["x0"])
    assert list(cat1) == ["ID", "x0", "y0", "z0", "comp", "STD", "T_GLR", "profile", "seg_label",
                          "imatch", "imatch2", "purity"]
    assert all(len(v) == n for v in cat1.values())
    # the input row of every output row: the (random, unique) test value identifies it
    key = lambda t: np.where(np.asarray(t["comp"]) == 0, t["T_GLR"], t["STD"])
    rows = {float(k): i for i, k in enumerate(key(cat))}
    assert len(rows) == n
    src = np.array([rows[float(k)] for k in key(cat1)])
    for col in ("x0", "y0", "z0", "comp"):
        assert np.array_equal(cat1[col], np.asarray(cat[col])[src])
    assert np.array_equal(np.sort(src), np.arange(n))
    ids = cat1["ID"]
    k = ids.max()
    assert np.array_equal(np.unique(ids), np.arange(1, k + 1))
    assert np.all(np.diff(ids) >= 0)
    assert np.all(np.diff(src)[np.diff(ids) == 0] > 0)            # input order inside one ID
    assert np.array_equal(cat1["imatch"], ref["imatch"][src] + 1)
    assert np.array_equal(cat1["imatch2"], ref["imatch2"][src] + 1)
    assert np.array_equal(ids, np.unique(cat1["imatch"], return_inverse=True)[1] + 1)
    assert np.array_equal(cat1["seg_label"], ref["area"][src])
    for g in np.unique(cat1["imatch2"]):
        m = cat1["imatch2"] == g
        assert np.all(cat1["seg_label"][m] == seg[cat1["y0"][m], cat1["x0"][m]].max())
    assert np.all((cat1["purity"] >= 0) & (cat1["purity"] <= 1))
    for col in ("STD", "T_GLR", "profile"):
        assert np.array_equal(cat1[col], np.asarray(cat[col])[src], equal_nan=True)


def test_cat1_columns_from_a_stubbed_kernel(monkeypatch, random_refs):
    """make_cat1 around a stubbed kernels.merge_detections (the oracle): columns in the
    reference's order, IDs, row order, seg_label, purity; ra / dec / lbda in front when a wcs
    and a wave axis are given."""
    from origin_amd import detection, kernels
    c, ref = random_refs(3)
    seg = np.zeros(c["shape"][1:], np.int64)
    seg[c["y"], c["x"]] = c["area"]
    seen = {}

    def stub(ctx, x0, y0, z0, area, shape, tol_spat, tol_spec):
        seen["args"] = (shape, tol_spat, tol_spec)
        assert np.array_equal(area, c["area"])
        r = oracle.merge(x0, y0, z0, area, tol_spat, tol_spec)
        return dict(comp=oracle.components(x0, y0, tol_spat), **r)
    monkeypatch.setattr(kernels, "merge_detections", stub)
    cat = fake_cat(c, np.random.default_rng(5))
    half = len(c["x"]) * 2 // 3
    cat_a = {k: v[:half] for k, v in cat.items()}
    cat_b = {k: v[half:] for k, v in cat.items()}
    cat1 = detection.make_cat1(None, cat_a, cat_b, seg, PVAL, PVAL_COMP, c["tol_spat"],
                               c["tol_spec"])
    assert seen["args"] == ((int(c["z"].max()) + 1,) + seg.shape, c["tol_spat"], c["tol_spec"])
    check_cat1(cat1, cat, seg, ref)

    class Wcs:
        def pix2sky(self, yx):
            return np.stack([yx[:, 0] * 2.0, yx[:, 1] * 3.0], 1)

    class Wave:
        def coord(self, z):
            return 4750 + 1.25 * np.asarray(z)
    cat1w = detection.make_cat1(None, cat_a, cat_b, seg, PVAL, PVAL_COMP, c["tol_spat"],
                                c["tol_spec"], wcs=Wcs(), wave=Wave())
    assert list(cat1w)[:5] == ["ID", "ra", "dec", "lbda", "x0"] and list(cat1w)[-1] == "purity"
    assert np.array_equal(cat1w["ra"], 3.0 * cat1w["x0"])
    assert np.array_equal(cat1w["dec"], 2.0 * cat1w["y0"])
    assert np.array_equal(cat1w["lbda"], 4750 + 1.25 * cat1w["z0"])


def test_reference_signatures_are_there():
    import inspect
    from origin_amd import lib_origin
    assert list(inspect.signature(lib_origin.spatiospectral_merging).parameters) == [
        "tbl", "tol_spat", "tol_spec"]
    assert list(inspect.signature(lib_origin.purity_estimation).parameters) == [
        "cat", "Pval", "Pval_comp"]


# ---------------------------------------------------------------------------------------- gpu
@pytest.fixture(scope="module")
def ctx():
    from origin_amd.device import default_context
    return default_context(0)


def device_merge(ctx, c):
    from origin_amd import kernels
    return kernels.merge_detections(ctx, c["x"], c["y"], c["z"], c["area"], c["shape"],
                                    c["tol_spat"], c["tol_spec"])


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_device_equals_the_reference_fixture(ctx, golden, i):
    c = golden_case(golden, i)
    got = device_merge(ctx, c)
    assert np.array_equal(got["comp"], oracle.components(c["x"], c["y"], c["tol_spat"]))
    for o in OUT:
        assert got[o].dtype == np.int32 and np.array_equal(got[o], c["out"][o]), o


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1])
def test_device_on_empty_and_single_tables(ctx, n):
    c = oracle.case_small(n)
    got = device_merge(ctx, c)
    ref = oracle.merge(c["x"], c["y"], c["z"], c["area"], 3, 5)
    assert got["comp"].shape == (n,) and np.all(got["comp"] == 0)
    for o in OUT:
        assert got[o].shape == (n,) and np.array_equal(got[o], ref[o])


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(20))
def test_device_equals_the_restatement_on_random_fields(ctx, random_refs, seed):
    c, ref = random_refs(seed)
    assert len(c["x"]) <= 3000 and (c["area"] == 0).any() and (c["area"] > 0).any()
    got = device_merge(ctx, c)
    assert np.array_equal(got["comp"], oracle.components(c["x"], c["y"], c["tol_spat"]))
    for o in OUT:
        assert np.array_equal(got[o], ref[o]), o


@pytest.mark.gpu
def test_two_calls_give_identical_tables(ctx, golden):
    for name in ("crowded", "chain", "stage2"):
        c = golden_case(golden, NAMES.index(name))
        a, b = device_merge(ctx, c), device_merge(ctx, c)
        for k in a:
            assert np.array_equal(a[k], b[k]), (name, k)


@pytest.mark.gpu
def test_arguments_outside_the_cube_are_refused(ctx):
    from origin_amd import _capi
    c = oracle.case_small(2)
    with pytest.raises(_capi.OriginHipError):
        device_merge(ctx, dict(c, shape=(40, 8, 4)))              # x0 = 4 is outside Nx = 4
    with pytest.raises(ValueError):
        device_merge(ctx, dict(c, tol_spat=0))


@pytest.mark.gpu
def test_cat1_properties_on_the_device(ctx, random_refs):
    from origin_amd import detection, lib_origin
    c, ref = random_refs(4)
    seg = np.zeros(c["shape"][1:], np.int64)
    seg[c["y"], c["x"]] = c["area"]
    cat = fake_cat(c, np.random.default_rng(6))
    half = len(c["x"]) * 2 // 3
    cat1 = detection.make_cat1(ctx, {k: v[:half] for k, v in cat.items()},
                               {k: v[half:] for k, v in cat.items()}, seg, PVAL, PVAL_COMP,
                               c["tol_spat"], c["tol_spec"])
    check_cat1(cat1, cat, seg, ref)
    # the function seam: the reference's table, rows by imatch and then by input row
    tbl = lib_origin.spatiospectral_merging(dict(x0=c["x"], y0=c["y"], z0=c["z"], area=c["area"]),
                                            c["tol_spat"], c["tol_spec"])
    assert list(tbl) == ["x0", "y0", "z0", "area", "imatch", "imatch2"]
    order = np.argsort(ref["imatch"], kind="stable")
    assert np.array_equal(tbl["imatch"], ref["imatch"][order])
    assert np.array_equal(tbl["imatch2"], ref["imatch2"][order])
    assert np.array_equal(tbl["area"], ref["area"][order])
    assert np.array_equal(tbl["z0"], c["z"][order])


@pytest.mark.gpu
def test_cubes_to_cat2_without_leaving_the_package(ctx):
    """threshold_detections -> make_cat1 -> lines.estimate_lines on a 60 x 24 x 24 cube: three
    sources with two lines each on a continuum, a segmap with two labels."""
    from origin_amd import detection, lines
    Nz, Ny, Nx, P = 60, 24, 24, 5
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[:P, :P] - P // 2
    psf = np.exp(-(yy ** 2 + xx ** 2) / 2.0)
    psf = np.broadcast_to(psf / psf.sum(), (Nz, P, P)).astype(np.float32).astype(np.float64)
    raw = rng.standard_normal((Nz, Ny, Nx)).astype(np.float32)
    var = np.ones((Nz, Ny, Nx), np.float32)
    local_max = np.zeros((Nz, Ny, Nx), np.float32)
    std_max = np.zeros((Nz, Ny, Nx), np.float32)
    profile = rng.integers(0, 4, (Nz, Ny, Nx)).astype(np.uint8)
    seg = np.zeros((Ny, Nx), np.int64)
    zz = np.arange(Nz)
    for lab, (y0, x0, z1, z2) in enumerate([(6, 6, 12, 40), (6, 16, 20, 23), (16, 10, 30, 50)]):
        spec = 200.0 + 300 * np.exp(-0.5 * ((zz - z1) / 1.5) ** 2) \
            + 300 * np.exp(-0.5 * ((zz - z2) / 1.5) ** 2)
        raw[:, y0 - 2:y0 + 3, x0 - 2:x0 + 3] += (spec[:, None, None] * psf).astype(np.float32)
        for z0, dy, dx in ((z1, 0, 0), (z1 + 1, 1, 0), (z2, 0, 1)):
            local_max[z0, y0 + dy, x0 + dx] = 9 + dy + dx
        std_max[z2 + 4, y0 - 1, x0 - 1] = 7                      # kept: farther than 2.5 voxels
        std_max[z1, y0, x0 + 1] = 7                              # dropped: next to a correl row
        if lab < 2:
            seg[y0 - 3:y0 + 4, x0 - 3:x0 + 4] = lab + 1
    local_max[5, 20, 20] = 8                                     # a lone detection on label 0
    d = ctx.to_device
    cat0, cat, cat_std = detection.threshold_detections(ctx, d(local_max), d(profile), d(std_max),
                                                        5.0, 5.0)
    assert len(cat["z0"]) == 10 and len(cat_std["z0"]) == 3 and len(cat0["z0"]) == 16
    cat1 = detection.make_cat1(ctx, cat, cat_std, seg, PVAL, PVAL_COMP)
    assert len(cat1["ID"]) == 13 and cat1["ID"].max() == 4
    assert sorted(np.bincount(cat1["ID"])[1:]) == [1, 4, 4, 4]
    # label 2's two lines are 3 channels apart and its std row 4 more: one source either way
    for i in np.unique(cat1["ID"]):
        assert len(np.unique(cat1["seg_label"][cat1["ID"] == i])) == 1
    cat2, lin, lvar = lines.estimate_lines(ctx, cat1, d(raw), d(var), psf)
    assert list(cat2)[:4] == ["ID", "x0", "x", "y0"] and list(cat2)[-3:] == ["residual", "flux",
                                                                              "num_line"]
    assert np.array_equal(cat2["ID"], cat1["ID"]) and len(lin) == 13
    assert np.array_equal(cat2["num_line"], np.arange(1, 14))
    assert np.all(np.isfinite(cat2["flux"])) and all(a.shape == (Nz,) for a in lin)
    assert np.array_equal(cat2["x"], cat2["x0"]) and np.array_equal(cat2["y"], cat2["y0"])


@pytest.mark.gpu
def test_cat1_from_session_after_steps_1_to_6(ctx):
    """cat1_from_session on a small session run through step 6: its thresholds, purity tables
    and segmap_cont; equal to make_cat1 on what from_session returns, and accepted by
    lines.from_session."""
    from origin_amd import detection, lines, synth
    from origin_amd.steps import SimpleOrig
    f, raw, var, mask = synth.small_case(Nz=160, Ny=48, Nx=52, seed=3, psf_size=9, nprof=3,
                                         area_size=24)
    orig = SimpleOrig(raw, var, mask, f.PSF.astype(float), f.profiles, ctx=ctx)
    orig.step01_preprocessing()
    orig.step02_areas.set_areamap(f.areamap)
    orig.step03_compute_PCA_threshold()
    orig.step04_compute_greedy_PCA()
    orig.step05_compute_TGLR()
    orig.step06_compute_purity_threshold(purity=0.8)
    cat1 = detection.cat1_from_session(orig)
    _, cat, cat_std = detection.from_session(orig)
    n = len(cat["z0"]) + len(cat_std["z0"])
    assert n > 0 and len(cat1["ID"]) == n
    seg = np.asarray(orig.segmap_cont)
    want = detection.make_cat1(ctx, cat, cat_std, seg, orig.Pval, orig.Pval_comp)
    assert list(cat1) == list(want) and list(cat1)[0] == "ID" and list(cat1)[-1] == "purity"
    for k in cat1:
        assert np.array_equal(cat1[k], want[k], equal_nan=cat1[k].dtype.kind == "f"), k
    assert np.array_equal(cat1["seg_label"] >= seg[cat1["y0"], cat1["x0"]], np.ones(n, bool))
    assert np.array_equal(np.unique(cat1["ID"]), np.arange(1, cat1["ID"].max() + 1))
    cat2, lin, _ = lines.from_session(orig, cat1)
    assert np.array_equal(cat2["ID"], cat1["ID"]) and len(lin) == n
