"""One field in every form a cube takes between the steps (origin_amd/cubes.py), through the
consumers of steps 6, 7 and 9 and ``Step.dump``: the five reductions, ``Compute_threshold_purity``,
``threshold_detections`` / ``det_correl_min``, ``cube_std`` / ``add_tglr_stat`` and ``write_image``.

Expectations are NumPy's on the host field (the float32 values widened to float64, as the
reference holds its cubes), never another form's output.  All of it is index work, comparisons and
copies of float32 values, so everything is compared exactly; the one exception is ``std``, whose
sums run in another order on a tiled cube: bit-equal to ``kernels.cube_std`` of the dense device
cube for the forms on one context, within ``test_cube_stats.RTOL`` (derived there) of NumPy's for
the tiled ones.
"""
import numpy as np
import pytest

from _cube_forms import as_sparse, tiled
from test_cube_stats import RTOL

pytestmark = pytest.mark.gpu

SHAPE = (9, 10, 12)
SINGLE = ("host_f64", "device", "sparse", "lazy_device", "lazy_sparse", "lazy_host", "fits")
TILED = ("tiled_dense", "tiled_sparse")
THRESHOLDS = [0.05, 0.0, 0.3, -0.2, 1e9]


def sparse_field(seed, scale):
    """float32, about one voxel in ten non-zero, both signs, values repeated and values equal to
    the thresholds used below (strict >), so that zeros, negative thresholds and ties matter."""
    rng = np.random.default_rng(seed)
    a = (np.round(rng.normal(0.0, 1.0, SHAPE), 1) * scale).astype(np.float32)
    a[rng.random(SHAPE) >= 0.1] = 0.0
    a += 0.0                                                     # (no -0.0: a list form drops it)
    flat = a.reshape(-1)
    flat[rng.choice(flat.size, 8, replace=False)] = np.array(
        [0.2, 0.3, 0.05, -0.2, -1.0, 0.5, 0.5, 2.5], np.float32) * scale
    return a


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The two fields (local maxima / minima), the aux cube and the keep map on the host, and all
    of them in the nine forms; made once, never modified."""
    from origin_amd import fitsio
    from origin_amd.session import DeviceGroup
    from origin_amd.steps import LazyCube
    g = DeviceGroup([0, 0])
    ctx = g.ctxs[0]
    tmp = tmp_path_factory.mktemp("forms")
    fields = dict(lmax=sparse_field(21, 1.0), lmin=sparse_field(22, 0.5))
    aux = (np.arange(fields["lmax"].size) % 251).astype(np.uint8).reshape(SHAPE)
    yy, xx = np.indices(SHAPE[1:])
    keep = (yy + 2 * xx) % 3 != 0                                # a third of the spaxels dropped
    d_aux = ctx.to_device(aux)
    forms = {}
    for name, a in fields.items():
        f64 = a.astype(np.float64)
        path = fitsio.write_image(str(tmp / f"{name}.fits"), f64, ctx=ctx)
        forms[name] = dict(
            host_f64=f64, device=ctx.to_device(a), sparse=as_sparse(ctx, a),
            tiled_dense=tiled(g, a), tiled_sparse=tiled(g, a, part=as_sparse),
            lazy_device=LazyCube(dev=ctx.to_device(a)), lazy_sparse=LazyCube(dev=as_sparse(ctx, a)),
            lazy_host=LazyCube(host=f64), fits=fitsio.FitsCube(path))
    auxes = {k: d_aux for k in SINGLE}
    auxes.update({k: tiled(g, aux, outside=0) for k in TILED})
    yield dict(ctx=ctx, fields={k: v.astype(np.float64) for k, v in fields.items()}, aux=aux,
               keep=keep, forms=forms, auxes=auxes, tmp=tmp)
    g.close()


@pytest.mark.parametrize("form", SINGLE + TILED)
def test_reductions_of_every_form(world, form):
    from origin_amd import cubes, kernels
    ctx, f64, keep = world["ctx"], world["fields"]["lmax"], world["keep"]
    cube = cubes.resident(ctx, world["forms"]["lmax"][form])
    aux = cubes.resident(ctx, world["auxes"][form], np.uint8)
    for kp in (None, keep):
        want = f64.max(axis=0) if kp is None else np.where(kp, f64.max(axis=0), 0.0)
        assert np.array_equal(cubes.zmax_map(cube, kp), want)
        sel = f64 if kp is None else f64[:, kp]
        counts = [np.count_nonzero(sel > t) for t in THRESHOLDS]
        assert np.array_equal(cubes.count_above(cube, THRESHOLDS, kp), counts)
    for t in (0.2, 0.0, -1.0):
        w = cubes.where_above(cube, t, aux=aux)
        z, y, x = np.where(f64 > t)                              # C order
        assert 0 < z.size < f64.size
        for k, want in (("z", z), ("y", y), ("x", x), ("value", f64[z, y, x]),
                        ("aux", world["aux"][z, y, x])):
            assert np.array_equal(w[k], want), (t, k)
    got = cubes.std(cube)
    ref = float(np.std(f64))
    print(f"std {form}: {got!r} numpy {ref!r} rel err {abs(got - ref) / ref:.3e}")
    if form in SINGLE:
        one = kernels.cube_std(ctx, world["forms"]["lmax"]["device"])
        assert np.float64(got).tobytes() == np.float64(one).tobytes()
    assert abs(got - ref) <= RTOL * ref


def purity_reference(purity, lmax, lmin, keep, threshlist):
    """Compute_threshold_purity (reference lib_origin.py:1425-1470) in NumPy."""
    L1, L0 = keep.size, int(np.count_nonzero(keep))
    kmin = lmin[:, keep]
    if threshlist is None:
        map_max = lmax.max(axis=0)
        threshmax = min(kmin.max(axis=0).max(), map_max.max())
        threshlist = np.linspace(np.median(map_max) * 1.1, threshmax, 50)
    threshlist = np.asarray(threshlist, dtype=np.float64)
    n1 = np.array([np.count_nonzero(lmax > t) for t in threshlist])
    n0 = np.array([np.count_nonzero(kmin > t) for t in threshlist]) * (L1 / L0)
    with np.errstate(divide="ignore", invalid="ignore"):
        est = 1 - n0 / n1
    order = np.argsort(threshlist, kind="stable")
    res = dict(Tval_r=threshlist[order], Pval_r=est[order], Det_m=n0.astype(int)[order],
               Det_M=n1[order])
    thr = np.inf if est[-1] < purity else np.interp(purity, res["Pval_r"], res["Tval_r"])
    return float(thr), res


@pytest.mark.parametrize("threshlist", [None, THRESHOLDS[:4] + [0.7, 1.2]], ids=["auto", "list"])
@pytest.mark.parametrize("form", SINGLE + TILED)
def test_purity_table_of_every_form(world, form, threshlist):
    import origin_amd.lib_origin as hip
    keep = world["keep"]
    segmap = (~keep).astype(int)                                 # background = kept spaxels
    want_thr, want = purity_reference(0.4, world["fields"]["lmax"], world["fields"]["lmin"], keep,
                                      threshlist)
    with np.errstate(all="ignore"):
        thr, res = hip.Compute_threshold_purity(0.4, world["forms"]["lmax"][form],
                                                world["forms"]["lmin"][form], segmap,
                                                threshlist=threshlist)
    assert np.isfinite(want_thr) and thr == want_thr
    for c in ("Tval_r", "Pval_r", "Det_m", "Det_M"):
        assert np.array_equal(np.asarray(res[c], float), np.asarray(want[c], float),
                              equal_nan=True), c


@pytest.mark.parametrize("form", SINGLE + TILED)
def test_detections_of_every_form(world, form):
    from origin_amd import detection
    ctx, lmax, smax = world["ctx"], world["fields"]["lmax"], world["fields"]["lmin"]
    forms = world["forms"]
    cat0, cat, _ = detection.threshold_detections(ctx, forms["lmax"][form], world["auxes"][form],
                                                  forms["lmin"][form], 0.2, 0.1)
    z, y, x = np.where(lmax > 0.2)
    zs = np.where(smax > 0.1)[0]
    assert z.size and zs.size and len(cat0["z0"]) == z.size + zs.size
    for k, want in (("z0", z), ("y0", y), ("x0", x), ("T_GLR", lmax[z, y, x]),
                    ("profile", world["aux"][z, y, x])):
        assert np.array_equal(cat[k], want), k
    got = detection.det_correl_min(ctx, forms["lmin"][form], -1.0)
    for a, b in zip(got, np.where(smax > -1.0)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("form", SINGLE + TILED)
def test_cube_std_and_tglr_stat_of_every_form(world, form):
    import origin_amd.lib_origin as hip
    from origin_amd import catalog
    ctx, forms = world["ctx"], world["forms"]
    refs = [float(np.std(world["fields"][k])) for k in ("lmax", "lmin")]
    got = [catalog.cube_std(ctx, forms[k][form]) for k in ("lmax", "lmin")]
    for g_, r in zip(got, refs):
        assert abs(g_ - r) <= RTOL * r
    lines = dict(ID=np.array([1, 1, 2]), T_GLR=np.array([3.0, 4.0, 5.0]),
                 STD=np.array([1.0, 2.0, 3.0]), flux=np.ones(3), purity=np.ones(3))
    hip.add_tglr_stat(dict(ID=np.array([1, 2])), lines, forms["lmax"][form], forms["lmin"][form])
    assert np.array_equal(lines["nsigTGLR"], lines["T_GLR"] / got[0])
    assert np.array_equal(lines["nsigSTD"], lines["STD"] / got[1])


@pytest.mark.parametrize("form", SINGLE + TILED)
def test_write_image_of_every_form(world, form):
    from origin_amd import fitsio
    path = fitsio.write_image(str(world["tmp"] / f"out_{form}.fits"), world["forms"]["lmax"][form],
                              ctx=world["ctx"])
    assert np.array_equal(fitsio.FitsCube(path)._data, world["fields"]["lmax"])
