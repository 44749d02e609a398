"""Function seam (tier B1): the hot functions of the reference's
``muse_origin/lib_origin.py`` with identical names, signatures and return tuples, running
on the MI355X through liborigin_hip.so.

``muse_origin.steps`` resolves these names through its module globals (steps.py:19-41), so

    import muse_origin.steps, origin_amd.lib_origin as hip
    for name in hip.__all__:
        setattr(muse_origin.steps, name, getattr(hip, name))

swaps the implementation without touching the reference.  Inputs and
outputs are host ``ndarray`` s (float64 out, as the reference produces); internally the
cubes are float32 in HBM.  There is no CPU fallback: without the library or a GPU every
function raises.
"""
import logging

import numpy as np

from . import catalog, cubes, detection, fitsio, kernels, lines, match, segmap, sparse
from .catalog import _columns
from .device import default_context
from .pca import GreedyPCA
from .thresholds import compute_thresh_gaussfit

__all__ = (
    'compute_segmap_gauss',
    'dct_residual',
    'O2test',
    'Compute_PCA_threshold',
    'Compute_GreedyPCA',
    'Compute_GreedyPCA_area',
    'Correlation_GLR_test',
    'compute_local_max',
    'compute_thresh_gaussfit',
    'Compute_threshold_purity',
    'estimation_line',
)


def _ctx():
    return default_context(0)


def _mask_on_device(ctx, mask, shape):
    return ctx.to_device(np.broadcast_to(cubes.host_mask(mask, shape), shape), np.uint8)


def compute_segmap_gauss(data, pfa, fwhm_fsf=0, bins='fd'):
    """gamma, labels (reference lib_origin.py:243-280): the threshold of the Gaussian fit on the
    host, mask, erosion, dilation, disc and labels on the device (``origin_amd.segmap``)."""
    return segmap.segmap_gauss(_ctx(), data, pfa, fwhm_fsf, bins=bins)


def dct_residual(w_raw, order, var, approx, mask):
    """Continuum estimated from the DCT decomposition (reference lib_origin.py:150-240;
    despite its name the reference returns the continuum, steps.py:431-434)."""
    ctx = _ctx()
    shape = w_raw.shape
    raw = ctx.to_device(w_raw, np.float32)
    dvar = ctx.to_device(np.broadcast_to(var, shape), np.float32)
    dmask = _mask_on_device(ctx, mask, shape)
    coef = kernels.dct_fit(ctx, raw, dvar, dmask, order, approx)
    cont = kernels.dct_continuum(ctx, coef, shape[0])
    return cont.to_host_f64()


def O2test(arr):
    """mean(arr**2, axis=0) (reference lib_origin.py:957-974)."""
    ctx = _ctx()
    arr = np.asarray(arr)
    d = ctx.to_device(arr, np.float32)
    return kernels.o2test(ctx, d).to_host().reshape(arr.shape[1:])


def Compute_PCA_threshold(faint, pfa):
    """test, histO2, frecO2, thresO2, mea, std (reference lib_origin.py:824-845)."""
    test = O2test(faint)
    histO2, frecO2, thresO2, mea, std = compute_thresh_gaussfit(test, pfa)
    return test, histO2, frecO2, thresO2, mea, std


def Compute_GreedyPCA(cube_in, test, thresO2, Noise_population, itermax):
    """faint, mapO2, nstop for one area given as (Nz, S) (reference lib_origin.py:848-954)."""
    ctx = _ctx()
    cube_in = np.asarray(cube_in)
    Nz, S = cube_in.shape
    F = ctx.to_device(cube_in.reshape(Nz, 1, S), np.float32)
    spx = np.arange(S, dtype=np.int32)
    mapO2, nstop = GreedyPCA(ctx).run(F, [spx], [np.asarray(test, dtype=np.float64)],
                                      [float(thresO2)], Noise_population, itermax)
    return F.to_host_f64().reshape(Nz, S), mapO2[0], nstop


def Compute_GreedyPCA_area(NbArea, cube_std, areamap, Noise_population, threshold_test,
                           itermax, testO2):
    """cube_faint, mapO2, nstop over all areas (reference lib_origin.py:769-821)."""
    ctx = _ctx()
    cube_std = np.asarray(cube_std)
    Nz, Ny, Nx = cube_std.shape
    F = ctx.to_device(cube_std, np.float32)
    flat = np.asarray(areamap).reshape(-1)
    area_spx = [np.nonzero(flat == i)[0].astype(np.int32) for i in range(1, NbArea + 1)]
    thr = [float(threshold_test[i]) for i in range(NbArea)]
    maps, nstop = GreedyPCA(ctx).run(F, area_spx, [np.asarray(t) for t in testO2], thr,
                                     Noise_population, itermax)
    mapO2 = np.zeros(Ny * Nx)
    for spx, m in zip(area_spx, maps):
        mapO2[spx] = m
    return F.to_host_f64(), mapO2.reshape(Ny, Nx), nstop


def Correlation_GLR_test(cube, fsf, weights, profiles, nthreads=1, pcut=None, pmeansub=True):
    """correl, profile (uint8), correl_min (reference lib_origin.py:1070-1217).
    ``nthreads`` is accepted for signature compatibility and ignored."""
    ctx = _ctx()
    cube = np.asarray(cube)
    plan = kernels.GLRPlan(ctx, cube.shape, fsf, weights, profiles, pcut, pmeansub)
    try:
        d = ctx.to_device(cube, np.float32)
        out = plan.run(d, mask=None, want_maps=False)
        correl = out["correl"].to_host_f64()
        profile = out["profile"].to_host()
        correl_min = out["correl_min"].to_host_f64()
    finally:
        plan.close()
    return correl, profile, correl_min


def compute_local_max(correl, correl_min, mask, size=3):
    """local maxima of correl and of -correl_min (reference lib_origin.py:1220-1256)."""
    ctx = _ctx()
    if not np.isscalar(size):
        if len(set(size)) != 1:
            raise ValueError("only cubic windows are supported")
        size = size[0]
    correl = np.asarray(correl)
    dc = ctx.to_device(correl, np.float32)
    dm = dc if correl_min is correl else ctx.to_device(correl_min, np.float32)
    dmask = _mask_on_device(ctx, mask, correl.shape)
    # (sparse pass where it exists: only the maxima cross PCIe, the zeros are made on the host)
    lmax, lmin = sparse.local_max(ctx, dc, dm, dmask, size)
    return lmax.to_host_f64(), lmin.to_host_f64()


class PurityTable(dict):
    """Columns Tval_r, Pval_r, Det_m, Det_M of the purity curve, sorted by Tval_r (what the
    reference returns as an astropy Table, lib_origin.py:1455-1461).  ``as_table()`` builds the
    astropy Table when astropy is installed."""

    colnames = ('Tval_r', 'Pval_r', 'Det_m', 'Det_M')

    def as_table(self):
        from astropy.table import Table
        res = Table([self[c] for c in self.colnames], names=self.colnames)
        res['Tval_r'].format = '.2f'
        res['Pval_r'].format = '.2f'
        return res


def Compute_threshold_purity(purity, cube_local_max, cube_local_min, segmap=None,
                             threshlist=None):
    """Threshold for a given purity (reference lib_origin.py:1391-1479).  The cubes may come in
    any form ``cubes.resident`` takes (host arrays are uploaded as float32; no PCIe traffic for
    what is in HBM already); only per-spaxel maxima and the counts per threshold leave the GPU.
    Returns (threshold, PurityTable)."""
    ctx = _ctx()
    logger = logging.getLogger(__name__)
    lmax, lmin = cubes.resident(ctx, cube_local_max), cubes.resident(ctx, cube_local_min)
    L1 = int(np.prod(lmin.shape[1:]))                                          # :1425
    keep = None
    if segmap is not None:                                                     # :1428-1435
        keep = np.asarray(segmap) == 0
        L0 = int(np.count_nonzero(keep))
        logger.info('using only background pixels (%.1f%%)', L0 / L1 * 100)
    else:
        L0 = L1
    if threshlist is None:                                                     # :1437-1442
        map_max = cubes.zmax_map(lmax)
        threshmax = min(cubes.zmax_map(lmin, keep).max(), map_max.max())
        threshmin = np.median(map_max) * 1.1
        threshlist = np.linspace(threshmin, threshmax, 50)
    threshlist = np.asarray(threshlist, dtype=np.float64)
    n1 = cubes.count_above(lmax, threshlist)                                   # :1444-1450
    n0 = cubes.count_above(lmin, threshlist, keep) * (L1 / L0)                 # :1452
    with np.errstate(divide='ignore', invalid='ignore'):
        est_purity = 1 - n0 / n1                                               # :1454
    order = np.argsort(threshlist, kind='stable')                              # res.sort('Tval_r')
    res = PurityTable(Tval_r=threshlist[order], Pval_r=est_purity[order],
                      Det_m=n0.astype(int)[order], Det_M=n1[order])
    if est_purity[-1] < purity:                                                # :1464-1468
        logger.warning('Maximum computed purity %.2f is below %.2f', est_purity[-1], purity)
        threshold = np.inf
    else:
        threshold = np.interp(purity, res['Pval_r'], res['Tval_r'])            # :1470
        detect = np.interp(threshold, res['Tval_r'], res['Det_M'])
        logger.info('Interpolated Threshold %.2f Detection %d for Purity %.2f', threshold,
                    detect, purity)
    try:  # the reference returns an astropy Table (what Step.dump writes, steps.py:321-322)
        return float(threshold), res.as_table()
    except ImportError:
        return float(threshold), res


def estimation_line(Cat1, raw, var, psf, wght, wcs, wave, size_grid=1, criteria='flux',
                    order_dct=30, horiz_psf=1, horiz=5):
    """Cat2, lin_est, var_est (reference lib_origin.py:1805-1938) through ``lines.estimate_lines``.
    ``Cat1``: any table-like with ``x0``, ``y0``, ``z0`` columns (an astropy Table, a dict of
    columns); ``Cat2`` is a dict of NumPy columns in the reference's column order.  ``wcs`` /
    ``wave`` are used only if not None: ``ra``, ``dec`` and ``lbda`` are then set from the new
    positions (:1922-1925).  Deviations from the reference: see ``origin_amd.lines``."""
    lines.check_arguments(wght, size_grid, criteria)
    ctx = _ctx()
    cat = _columns(Cat1)
    raw, var = cubes.host_array(raw), cubes.host_array(var)
    d_raw = ctx.to_device(raw, np.float32)
    d_var = ctx.to_device(np.broadcast_to(var, raw.shape), np.float32)
    cat2, lin_est, var_est = lines.estimate_lines(ctx, cat, d_raw, d_var, psf, wght, size_grid,
                                                  criteria, order_dct, horiz_psf, horiz)
    if wcs is not None:
        dec, ra = wcs.pix2sky(np.stack((cat2['y'], cat2['x'])).T).T
        cat2['ra'], cat2['dec'] = ra, dec
    if wave is not None:
        cat2['lbda'] = wave.coord(cat2['z'])
    return cat2, lin_est, var_est


# The two functions below keep the reference's signatures but return dicts of NumPy columns, as
# estimation_line does.  They are not in __all__: Detection.run goes on with astropy Table
# methods on what spatiospectral_merging returns, so swapping them into muse_origin.steps
# would break it; detection.make_cat1 is the device version of that whole block.
def spatiospectral_merging(tbl, tol_spat, tol_spec):
    """The reference's table (lib_origin.py:1319-1387: the input columns, ``area`` replaced,
    ``imatch``, ``imatch2``, rows sorted by ``imatch``) through ``detection.merge_detections``.
    ``tbl``: any table-like with ``x0``, ``y0``, ``z0``, ``area`` (an astropy Table, a dict of
    columns).  Rows of one ``imatch`` come in input order."""
    return detection.merge_detections(_ctx(), _columns(tbl), tol_spat, tol_spec)


def purity_estimation(cat, Pval, Pval_comp):
    """``cat`` (``comp``, ``T_GLR``, ``STD``) as a dict of columns with the ``purity`` column of
    the reference (lib_origin.py:1941-1991) added.  Host arithmetic (scipy ``interp1d``)."""
    out = _columns(cat)
    out['purity'] = detection.purity_estimation(out, Pval, Pval_comp)
    return out


# Step 9 (CleanResults.run, steps.py:1149-1160).  Like the two above these return dicts of NumPy
# columns and are not in __all__: the reference's run body goes on with ``table.meta`` and
# astropy methods.  ``origin_amd.catalog`` documents the deviations.
def merge_similar_lines(table, *, z_pix_threshold=5):
    """The reference's table (lib_origin.py:2140-2222: the input rows sorted by ``(ID, z)`` with
    ``line_merged_flag`` and ``merged_in`` added) through ``catalog.merge_similar_lines``."""
    return catalog.merge_similar_lines(_columns(table), z_pix_threshold=z_pix_threshold)


def unique_sources(table):
    """One row per ``ID`` (lib_origin.py:1994-2091) through ``catalog.unique_sources``."""
    return catalog.unique_sources(_columns(table))


def add_tglr_stat(src_table, lines_table, correl, std):
    """``add_tglr_stat`` (lib_origin.py:2094-2137): ``lines_table`` gains ``nsigTGLR`` and
    ``nsigSTD`` in place, the returned source table the per-``ID`` maxima.  ``correl`` / ``std``
    may come in any form ``cubes.resident`` takes (host arrays are uploaded as float32): their
    standard deviations are reductions on the device (``cubes.std``), only the two scalars come
    back."""
    ctx = _ctx()
    return catalog.add_tglr_stat(_columns(src_table), lines_table,
                                 catalog.cube_std(ctx, correl), catalog.cube_std(ctx, std))


# compute_true_purity: the reference's validation tool (it is called by hand, not by a step), so
# it is not in __all__ either.  DESIGN.md section 3l.
class _LinearWave:
    """The linear spectral axis of a DATA header's cards: ``pixel`` as mpdaf's
    ``WaveCoord.pixel`` gives it (0-based, not rounded)."""

    def __init__(self, cards):
        step = cards.get('CD3_3', cards.get('CDELT3'))
        missing = [k for k, v in (('CRVAL3', cards.get('CRVAL3')), ('CRPIX3', cards.get('CRPIX3')),
                                  ('CD3_3 or CDELT3', step)) if v is None]
        if missing:
            raise ValueError('the wave header lacks ' + ', '.join(missing))
        self.crval, self.crpix = float(cards['CRVAL3']), float(cards['CRPIX3'])
        self.step = float(step)

    def pixel(self, lbda):
        return (np.asarray(lbda, dtype=np.float64) - self.crval) / self.step + self.crpix - 1.0


def _wave_axis(wave, cube):
    for w in (wave, getattr(cube, 'wave', None)):
        if w is None:
            continue
        return w if hasattr(w, 'pixel') else _LinearWave(w)
    raise ValueError('no wave axis: give wave= (an object with .pixel(), or the CRVAL3 / CRPIX3 / '
                     'CD3_3 cards of a session: wave=orig.wave_header), or a cube with a .wave')


def compute_true_purity(cube_local_max, refcat, maxdist=4.5, threshmin=4, threshmax=7, plot=False,
                        Pval=None, wave=None):
    """True purity and completeness of a run against a catalogue of known lines (reference
    lib_origin.py:2375-2443) through ``match.true_purity``: a dict of columns ``thresh, ndetect,
    ntrue, nfalse, nmiss, purity``.

    ``cube_local_max``: any form ``cubes.resident`` takes.  ``refcat``: the path of a FITS table
    (read with ``fitsio.read_table``, not ``Table.read``) or a mapping of columns with ``TYPE``,
    ``LOBS``, ``Q``, ``P``.  The lines are the rows with ``TYPE == 6``; the misses are counted
    from ``nref = len(refcat)``, ALL rows -- a quirk of the reference (:2384, :2399) that is kept.
    The z of a line is ``wave.pixel(LOBS)`` with ``wave`` the argument, else
    ``cube_local_max.wave``; either is an object with ``.pixel()`` or the cards of a linear axis
    (``CRVAL3``, ``CRPIX3``, ``CD3_3`` or ``CDELT3``: a session's ``orig.wave_header``, which the
    caller passes as ``wave``).  ``ValueError`` names what is missing, before anything runs on
    the device.  The reference's figure is not drawn: ``plot=True`` needs matplotlib as there
    (``ImportError`` without it) and then raises ``NotImplementedError``, before anything runs;
    the returned columns are what the figure shows.  ``Pval`` is accepted and not used."""
    if plot:
        import matplotlib  # noqa: F401
        raise NotImplementedError('compute_true_purity draws no figure: plot the returned columns')
    ref = _columns(fitsio.read_table(refcat) if isinstance(refcat, (str, bytes)) or
                   hasattr(refcat, '__fspath__') else refcat)
    missing = [k for k in ('TYPE', 'LOBS', 'Q', 'P') if k not in ref]
    if missing:
        raise ValueError('refcat lacks the column(s) ' + ', '.join(missing))
    axis = _wave_axis(wave, cube_local_max)
    lines6 = ref['TYPE'] == 6                                                   # :2381
    zref = np.asarray(axis.pixel(ref['LOBS'][lines6]), dtype=np.float64)        # :2382
    nref = len(ref['TYPE'])                                                     # :2384
    tbl = match.true_purity(_ctx(), cube_local_max, (ref['Q'][lines6], ref['P'][lines6], zref),
                            nref, maxdist, threshmin, threshmax)
    return tbl
