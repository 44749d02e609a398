"""Step seam (tier B2): the four hot steps of the reference's
``muse_origin/steps.py`` -- ``Preprocessing`` (:355), ``ComputePCAThreshold`` (:572),
``ComputeGreedyPCA`` (:634), ``ComputeTGLR`` (:707) -- with the same ``name``, ``desc``,
``require``, ``DataObj`` labels and ``run`` keyword names/defaults, running on the GPU.

Two ways to use them:

* ``register()``: when ``muse_origin`` is importable, subclasses of the reference's own
  step classes (only ``run`` overridden) are swapped into ``muse_origin.steps.STEPS``
  before ``ORIGIN(...)`` is constructed (origin.py:193 reads that list).
* stand-alone: ``SimpleOrig`` carries exactly the attributes the four ``run`` bodies read
   and the minimal ``Step`` machinery below (status, ``require`` check,
  parameter recording, runtime) mirrors reference steps.py:101-352 so tests and the
  benchmark drive the same code without mpdaf.

Steps 7-9 -- ``Detection`` (:895), ``ComputeSpectra`` (:1048), ``CleanResults`` (:1121) -- are here
as stand-alone classes over ``detection.py``, ``lines.py`` and ``catalog.py``; ``register()``
leaves the reference's own classes of those steps alone (they work on astropy tables and mpdaf
objects: INTEGRATION.md).

Cubes produced by one step stay in HBM for the next one (``LazyCube``); a host float64
copy is only made when somebody reads ``._data``.
"""
import inspect
import logging
import os
import time
from collections import OrderedDict
from datetime import datetime
from enum import Enum

import numpy as np

from . import catalog, cubes, detection, fitsio, kernels, lines, pipeline, segmap, sparse
from .cubes import LazyCube, session_cube                         # noqa: F401 (LazyCube: re-export)
from .cubes import cache as _cache, ctx_of as _ctx_of, inputs_on_device as _inputs_on_device
from .device import default_context
from .lib_origin import Compute_threshold_purity

__all__ = ('Preprocessing', 'CreateAreas', 'ComputePCAThreshold', 'ComputeGreedyPCA', 'ComputeTGLR',
           'ComputePurityThreshold', 'Detection', 'ComputeSpectra', 'CleanResults', 'Catalog',
           'Status', 'Step', 'DataObj', 'SimpleOrig', 'STEPS', 'register', 'unregister')


# ----------------------------------------------------------------------------- framework
# Stand-alone harness for sessions without muse_origin/mpdaf.  It honours the same contract as
# the reference's Step machinery (steps.py:112-299) -- the persisted keys of ``param[name]``
# ('stepidx', 'params', 'status', 'runtime', 'execution_date'), the ``stepNN_<name>`` method
# names, the ``require`` check and its error text, FAILED on exceptions -- but is built
# differently: descriptors name themselves (``__set_name__``), classes collect their outputs
# along the MRO in ``__init_subclass__`` (so a mixin + base combination keeps them, which the
# reference's metaclass does not: see register()), and reload goes through a reader table.
class Status(Enum):
    """Values are what the reference persists in the session's yaml (steps.py:112-118)."""
    NOTRUN = 'not run yet'
    RUN = 'run'
    DUMPED = 'dumped outputs'
    FAILED = 'failed'


_DONE = (Status.RUN, Status.DUMPED)

class Catalog(OrderedDict):
    """A table as a dict of NumPy columns that carries header cards in ``meta`` (``CAT3_TS`` of
    the step-9 tables, reference lib_origin.py:2220, :2089), written to and read from the table
    extension's header by ``Step.dump`` / ``Step.load``."""

    def __init__(self, columns=(), meta=None):
        super().__init__(columns)
        self.meta = OrderedDict(meta or {})


def _read_catalog(path):
    meta = OrderedDict()
    return Catalog(fitsio.read_table(path, header=meta), meta)


def write_spectra(path, spectra):
    """The ``spectra`` of step 8 (``OrderedDict num_line -> (data, var, z_min)``) as one ``.npz``:
    ``num_line`` and ``z_min`` (int64, one entry per spectrum, in the dict's order) and, per
    spectrum, ``data_<num_line>`` and ``var_<num_line>`` (float64)."""
    doc = dict(num_line=np.array(list(spectra), dtype=np.int64),
               z_min=np.array([v[2] for v in spectra.values()], dtype=np.int64))
    for k, (data, var, _) in spectra.items():
        doc[f'data_{int(k)}'] = np.asarray(data, dtype=np.float64)
        doc[f'var_{int(k)}'] = np.asarray(var, dtype=np.float64)
    with open(path, 'wb') as f:
        np.savez(f, **doc)


def read_spectra(path):
    with np.load(path) as doc:
        return OrderedDict((int(k), (doc[f'data_{int(k)}'], doc[f'var_{int(k)}'], int(z)))
                           for k, z in zip(doc['num_line'], doc['z_min']))


_READERS = {
    'cube': lambda path: fitsio.FitsCube(path),
    'image': lambda path: fitsio.FitsCube(path),
    'table': _read_catalog,
    'array': lambda path: np.loadtxt(path, ndmin=1),
    'spectra': read_spectra,
}
_EXTENSIONS = {'array': 'txt', 'spectra': 'npz'}     # every other kind: 'fits'


class DataObj:
    """A named output of a step.  Holds the value, or -- once the step has been dumped -- the
    path of its file, in which case the first read brings it back through ``_READERS`` (cubes
    and images as ``fitsio.FitsCube``, decoded by the GPU when used).  A path whose file is
    gone reads as None, an output never produced too (reference behaviour, steps.py:121-163)."""

    def __init__(self, kind):
        self.kind = kind
        self.label = None

    def __set_name__(self, owner, name):
        self.label = name

    def __get__(self, obj, owner=None):
        if obj is None:
            return None
        slot = vars(obj)
        val = slot.get(self.label)
        if not isinstance(val, str):
            return val
        if not os.path.isfile(val):
            return None
        slot[self.label] = val = _READERS[self.kind](val)
        return val

    def __set__(self, obj, val):
        vars(obj)[self.label] = val


def _outputs_of(cls):
    """(label, kind) of every DataObj visible on ``cls``, base classes first."""
    seen = OrderedDict()
    for klass in reversed(cls.__mro__):
        for label, attr in vars(klass).items():
            if isinstance(attr, DataObj):
                seen[label] = attr.kind
    return list(seen.items())


class Step:
    """One processing step of a session: ``step(**kw)`` records the keyword values, refuses to
    run before the steps named in ``require``, runs, and leaves status / runtime / date in
    ``orig.param[name]``."""

    name = None
    desc = None
    require = None
    on_demand = False     # True: a SimpleOrig makes the step at its first use, not at construction
    _dataobjs = []

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        cls._dataobjs = _outputs_of(cls)

    def __init__(self, orig, idx, param):
        self.logger = logging.getLogger(__name__)
        self.orig, self.idx = orig, idx
        self.method_name = f'step{idx:02d}_{self.name}'
        # a reloaded session brings its own record: keep what is there
        self.meta = param.setdefault(self.name, {})
        self.meta.setdefault('stepidx', idx)
        self.param = self.meta.setdefault('params', {})

    def __repr__(self):
        return f'Step {self.idx:02d}: <{type(self).__name__}(status: {self.status.name})>'

    def _loginfo(self, *args):
        self.logger.info(*args)

    def _logdebug(self, *args):
        self.logger.debug(*args)

    def _logwarning(self, *args):
        self.logger.warning(*args)

    status = property(lambda self: self.meta.get('status', Status.NOTRUN),
                      lambda self, val: self.meta.__setitem__('status', val))

    def _record_keywords(self, kwargs):
        for key, par in inspect.signature(self.run).parameters.items():
            if key != 'orig':
                self.param[key] = kwargs.get(key, par.default)

    def _check_required(self):
        for other in (self.orig.steps[r] for r in self.require or ()):
            if other.status not in _DONE:
                raise RuntimeError(f'step {other.idx:02d} must be run before')

    def __call__(self, *args, **kwargs):
        start = time.time()
        self._loginfo('Step %02d - %s', self.idx, self.desc)
        self._record_keywords(kwargs)
        self._check_required()
        self.status = Status.FAILED          # stays if run() raises
        self.run(self.orig, *args, **kwargs)
        self.status = Status.RUN
        self.meta['runtime'] = time.time() - start
        self.meta['execution_date'] = datetime.now().isoformat()
        self._loginfo('%02d Done - %.2f sec.', self.idx, self.meta['runtime'])

    # without mpdaf the outputs stay LazyCube / ndarray
    def store_cube(self, name, data, **kwargs):
        setattr(self, name, data)

    def store_image(self, name, data, **kwargs):
        setattr(self, name, data)

    def dump(self, outpath):
        """Save the outputs of a step that has been run and replace them by the paths of
        their files (reference steps.py:301-340): ``<outpath>/<name>.fits`` for cubes, images
        and tables (``meta`` of a ``Catalog`` as header cards), ``<name>.txt`` for arrays,
        ``<name>.npz`` for the spectra of step 8 (``write_spectra``).  Cubes go from HBM to the file through the
        device-side FITS encoder (fitsio.write_image), float64 on disk unless the reference
        itself holds another type (``convert_float32=False``, steps.py:319)."""
        if self.status is not Status.RUN:
            return
        ctx = getattr(self.orig, 'hip_ctx', None)
        for name, kind in self._dataobjs:
            obj = getattr(self, name)
            if obj is None:
                continue
            outf = f'{outpath}/{name}.{_EXTENSIONS.get(kind, "fits")}'
            self.logger.debug('   - %s [%s]', name, kind)
            if kind in ('cube', 'image'):
                fitsio.write_image(outf, obj, ctx=ctx, header=self._wcs_cards(kind))
            elif kind == 'table':
                if hasattr(obj, 'write'):  # astropy Table
                    obj.write(outf, overwrite=True)
                else:
                    fitsio.write_table(outf, catalog._columns(obj),
                                       header=getattr(obj, 'meta', None))
            elif kind == 'array':
                np.savetxt(outf, obj)
            elif kind == 'spectra':
                write_spectra(outf, obj)
            # the attribute becomes the path of its file: the data (and its copy in HBM) is
            # released and comes back from the file when the attribute is read again
            setattr(self, name, outf)
            _cache(self.orig).pop(name, None)
        self.status = Status.DUMPED

    def load(self, outpath):
        """Point the outputs of a dumped step at their files; they are read when accessed
        (reference steps.py:342-352)."""
        if self.status is not Status.DUMPED:
            return
        for name, kind in self._dataobjs:
            setattr(self, name, f'{outpath}/{name}.{_EXTENSIONS.get(kind, "fits")}')

    def _wcs_cards(self, kind):
        """World-coordinate cards of the session (``orig.wcs_header`` / ``orig.wave_header``:
        plain mappings of FITS keywords when given), as mpdaf adds to the DATA extension."""
        cards = OrderedDict()
        cards.update(getattr(self.orig, 'wcs_header', None) or {})
        if kind == 'cube':
            cards.update(getattr(self.orig, 'wave_header', None) or {})
        return cards


# ----------------------------------------------------------------------------- helpers
# Devices of the sessions that do not say themselves (``register(devices=[...])`` sets it for
# the reference's ORIGIN objects, which know nothing of GPUs); None = one context on device 0.
_DEFAULT_DEVICES = None


def _session_of(orig):
    """The ``session.TiledSession`` of a session that runs on several devices (``orig.hip_devices``
    -- ``SimpleOrig(..., devices=[...])`` -- or ``register(devices=[...])``), made on first use;
    None for the usual one-context session.  One process, one context and one thread per entry;
    the same ordinal twice means two contexts on that card (strips through the host)."""
    sess = orig.__dict__.get('_hip_session')
    if sess is not None:
        return sess
    devices = orig.__dict__.get('hip_devices', None) or _DEFAULT_DEVICES
    if devices is None or len(devices) < 2:
        return None
    from .session import DeviceGroup, TiledSession
    sess = TiledSession(DeviceGroup(devices, orig.__dict__.get('hip_backend')))
    orig.__dict__['_hip_session'] = sess
    return sess


# ----------------------------------------------------------------------------- run bodies
class _HipStepMixin:
    """Store cubes so that they stay in HBM between steps (``cubes.session_cube`` fetches them).
    Under the stand-alone ``Step`` the DataObj holds a ``LazyCube``; under the reference's
    ``Step`` (register()) ``store_cube`` builds an mpdaf Cube from a host array as usual."""

    def _put_cube(self, orig, name, dev, dtype=np.float64):
        _cache(orig)[name] = dev
        if isinstance(self, Step):
            self.store_cube(name, LazyCube(dev, dtype=dtype))
        else:
            self.store_cube(name, dev.to_host_f64() if dtype == np.float64
                            else dev.to_host().astype(dtype, copy=False))


class _PreprocessingRun(_HipStepMixin):
    name = 'preprocessing'
    desc = 'Preprocessing'

    def run(self, orig, dct_order=10, dct_approx=False, pfasegcont=0.01, pfasegres=0.01,
            local_max_size=3, bins='fd'):
        sess = _session_of(orig)
        self._loginfo('DCT computation')
        if sess is not None:   # several devices: row bands, one all-reduce, a one-spaxel halo
            out = sess.preprocess(orig.cube_raw, orig.var, orig.mask, dct_order, dct_approx,
                                  local_max_size)
            Nz = out['cube_std'].shape[0]
            lmax, lmin = out['cube_std_local_max'], out['cube_std_local_min']
            ima_std, ima_dct, o2, cont_o2 = (out['ima_std'], out['ima_dct'].astype(np.float32),
                                             out['o2'], out['cont_o2'])
        else:
            ctx = _ctx_of(orig)
            raw, var, mask = _inputs_on_device(orig, ctx)
            Nz = raw.shape[0]
            out = pipeline.preprocess(ctx, raw, var, mask, dct_order, dct_approx,
                                      allreduce=getattr(orig, 'allreduce', None))
            ima_std = out['ima_std'].to_host().astype(np.float64)
            lmax, lmin = sparse.local_max(ctx, out['cube_std'], out['cube_std'], mask,
                                          local_max_size)
            ima_dct, o2 = out['ima_dct'].to_host(), out['o2_host']
            # sum_z cont_dct^2 is a per-spaxel reduction of the device cube
            cont_o2 = kernels.o2test(ctx, out['cont_dct']).to_host()
        self._loginfo('Std signal saved in self.cube_std and self.ima_std')
        self._put_cube(orig, 'cube_std', out['cube_std'])
        self.store_image('ima_std', ima_std)

        self._loginfo('Compute local maximum of std cube values')
        self._put_cube(orig, 'cube_std_local_max', lmax)
        self._put_cube(orig, 'cube_std_local_min', lmin)

        self._loginfo('DCT continuum saved in self.cont_dct and self.ima_dct')
        self._put_cube(orig, 'cont_dct', out['cont_dct'], np.float32)
        self.store_image('ima_dct', ima_dct)
        _cache(orig)['o2_std'] = o2

        mean_fwhm = int(np.ceil(np.mean(orig.FWHM_PSF)))
        self._loginfo('Segmentation based on the continuum')
        # (mask, morphology and labels on the device, the several-device sessions included: the
        # maps are whole images on the host here; the log10 stays NumPy's)
        sctx = _ctx_of(orig)
        map1 = np.log10(cont_o2 * Nz)
        thresh, map_cont = segmap.segmap_gauss(sctx, map1, pfasegcont, mean_fwhm, bins=bins)
        self.store_image('segmap_cont', map_cont)
        self._loginfo('Segmentation based on the residual')
        thresh, map_res = segmap.segmap_gauss(sctx, o2, pfasegres, mean_fwhm, bins=bins)
        self._loginfo('Merging both maps')
        self.store_image('segmap_merged', segmap.merged_labels(sctx, map_cont, map_res))


class _CreateAreasRun:
    """CreateAreas.run (reference steps.py:492-569): host geometry, origin_amd/areas.py."""
    name = 'areas'
    desc = 'Areas creation'
    _Status = Status     # register() points this at the reference's own enum

    def run(self, orig, pfa=0.2, minsize=100, maxsize=None):
        from .areas import create_areamap
        mask = _data(orig.mask).astype(bool, copy=False)
        nexp = int(np.sum(mask.shape[0] - mask.sum(axis=0) > 0))
        nsub = np.maximum(1, int(np.sqrt(nexp / (minsize ** 2))))
        if nsub > 1:
            self._loginfo('First segmentation of %d^2 square', nsub)
        areamap, nbAreas = create_areamap(mask, _data(orig.segmap_merged), pfa, minsize, maxsize)
        orig.param['nbareas'] = nbAreas
        self.store_image('areamap', areamap)
        self._loginfo('Save the map of areas in self.areamap')
        self._loginfo('%d areas generated', nbAreas)

    def set_areamap(self, areamap):
        """Use an area map made elsewhere (a regular grid in the benchmarks, a map loaded from a
        previous session) instead of running the step: same outputs and status as ``run``."""
        areamap = _data(areamap).astype(int)
        labels = np.unique(areamap)
        self.orig.param['nbareas'] = len(labels) - (1 if 0 in labels else 0)
        self.store_image('areamap', areamap)
        self.status = self._Status.RUN


class _ComputePCAThresholdRun(_HipStepMixin):
    name = 'compute_PCA_threshold'
    desc = 'PCA threshold computation'
    require = ('preprocessing', 'areas')

    def run(self, orig, pfa_test=0.01):
        o2 = _cache(orig).get('o2_std')
        if o2 is None:  # session reloaded: recompute the O2 map from cube_std
            ctx = _ctx_of(orig)
            o2 = kernels.o2test(ctx, cubes.dense(ctx, session_cube(orig, 'cube_std'))).to_host()
        areamap = _data(orig.areamap)
        res = pipeline.pca_threshold(o2, areamap, orig.nbAreas, pfa_test)
        for i in range(orig.nbAreas):
            self._loginfo('Area %d, estimation mean/std/threshold: %f/%f/%f', i + 1,
                          res['meaO2'][i], res['stdO2'][i], res['thresO2'][i])
        orig.testO2, orig.histO2, orig.binO2 = res['testO2'], res['histO2'], res['binO2']
        self.thresO2, self.meaO2, self.stdO2 = res['thresO2'], res['meaO2'], res['stdO2']


class _ComputeGreedyPCARun(_HipStepMixin):
    name = 'compute_greedy_PCA'
    desc = 'Greedy PCA computation'
    require = ('preprocessing', 'areas', 'compute_PCA_threshold')

    def run(self, orig, Noise_population=50, itermax=100, threshold_list=None):
        ctx = _ctx_of(orig) if _session_of(orig) is None else None
        thr = orig.thresO2 if threshold_list is None else threshold_list
        orig.param['threshold_list'] = thr
        self._loginfo('   - List of threshold = %s', ' '.join("%.2f" % x for x in thr))
        self._loginfo('Compute greedy PCA on each zone')
        areamap = _data(orig.areamap)
        sess = _session_of(orig)
        if sess is not None:   # several devices: whole areas per rank (session.TiledSession)
            std = _cache(orig).get('cube_std')
            if std is None:
                std = orig.cube_std
            faint, mapO2, nstop = sess.greedy_pca(
                std, areamap, orig.nbAreas, thr, orig.testO2, _glr_halo(orig), Noise_population,
                itermax)
        else:
            faint, mapO2, nstop, drv = pipeline.greedy_pca(
                ctx, cubes.dense(ctx, session_cube(orig, 'cube_std')), areamap, orig.nbAreas, thr,
                orig.testO2, Noise_population, itermax)
        if nstop > 0:
            self._logwarning('The iterations have been reached the limit of %d in %d cases',
                             itermax, nstop)
        self._put_cube(orig, 'cube_faint', faint)
        self.store_image('mapO2', mapO2)


class _ComputeTGLRRun(_HipStepMixin):
    name = 'compute_TGLR'
    desc = 'GLR test'
    require = ('compute_greedy_PCA',)

    def run(self, orig, size=3, ncpu=1, pcut=1e-8, pmeansub=True):
        sess = _session_of(orig)
        self._loginfo('Correlation')
        if sess is not None:   # several devices: halo exchange + GLR per box of areas
            faint = _cache(orig).get('cube_faint')
            if faint is None:
                faint = orig.cube_faint
            if getattr(sess, 'host_mask', None) is None:
                sess.host_mask = cubes.host_mask(orig.mask, faint.shape)
            out = sess.tglr(faint, _data(orig.areamap), orig.PSF, orig.wfields, orig.profiles,
                            size, pcut, pmeansub)
            maxmap, minmap = out['maxmap'], out['minmap']
        else:
            ctx = _ctx_of(orig)
            _, _, mask = _inputs_on_device(orig, ctx)
            faint = cubes.dense(ctx, session_cube(orig, 'cube_faint'))
            plan = kernels.GLRPlan(ctx, faint.shape, orig.PSF, orig.wfields, orig.profiles, pcut,
                                   pmeansub)
            try:
                out = pipeline.tglr(ctx, plan, faint, mask, size)
                ctx.sync()
            finally:
                plan.close()
            maxmap, minmap = out['maxmap'].to_host(), out['minmap'].to_host()
        self._put_cube(orig, 'cube_correl', out['correl'])
        self._put_cube(orig, 'cube_correl_min', out['correl_min'])
        self._put_cube(orig, 'cube_profile', out['profile'], np.uint8)
        self.store_image('maxmap', maxmap.astype(np.float64))
        self.store_image('minmap', minmap.astype(np.float64))
        self._put_cube(orig, 'cube_local_max', out['local_max'])
        self._put_cube(orig, 'cube_local_min', out['local_min'])


class _ComputePurityThresholdRun(_HipStepMixin):
    """ComputePurityThreshold.run (reference steps.py:848-890): the purity curves come from
    reductions of the local-maximum cubes that are still in HBM."""
    name = 'compute_purity_threshold'
    desc = 'Compute Purity threshold'
    require = ('compute_TGLR',)

    def run(self, orig, purity=0.9, purity_std=None, threshlist=None, pfasegfinal=1e-5,
            bins='fd'):
        if purity_std is None:
            purity_std = purity
        orig.param.update(dict(purity=purity, purity_std=purity_std))
        # another segmap on the maxmap, merged with segmap_merged          (steps.py:862-867)
        sctx = _ctx_of(orig)
        thresh, map_res = segmap.segmap_gauss(sctx, _data(orig.maxmap), pfasegfinal, 0, bins=bins)
        segmap_purity = segmap.merged_labels(sctx, map_res, _data(orig.segmap_merged))
        self.store_image('segmap_purity', segmap_purity)

        self._loginfo('Estimation of threshold with purity = %.2f', purity)
        threshold, pval = Compute_threshold_purity(
            purity, session_cube(orig, 'cube_local_max'), session_cube(orig, 'cube_local_min'),
            segmap_purity, threshlist=threshlist)
        self.Pval = pval
        orig.param['threshold'] = threshold
        self._loginfo('Threshold: %.2f ', threshold)

        self._loginfo('Estimation of threshold std with purity = %.2f', purity_std)
        threshold_std, pval = Compute_threshold_purity(
            purity_std, session_cube(orig, 'cube_std_local_max'),
            session_cube(orig, 'cube_std_local_min'), threshlist=threshlist)
        self.Pval_comp = pval
        orig.param['threshold_std'] = threshold_std
        self._loginfo('Threshold: %.2f ', threshold_std)


class _DetectionRun(_HipStepMixin):
    """Detection.run (reference steps.py:941-1045) through ``origin_amd.detection``: the three
    ``np.where`` scans are stream compactions of the cubes in HBM, the spatio-spectral merging
    runs on the device (csrc/merge.hip).  ``segmap=None`` uses ``segmap_cont`` as it is: the
    reference's extra ``phot_deblend_sources`` pass over it (:1006) needs photutils and stays
    with the caller, who hands its result in as ``segmap``."""
    name = 'detection'
    desc = 'Thresholding and spatio-spectral merging'

    def det_correl_min(self, thresh=None):
        """3D positions of detections in correl_min (steps.py:935-939)."""
        orig = self.orig
        thresh = thresh or orig.param['threshold']
        return detection.det_correl_min(_ctx_of(orig), session_cube(orig, 'cube_local_min'), thresh)

    def run(self, orig, threshold=None, threshold_std=None, tol_spat=3, tol_spec=5,
            maxdist_lines=2.5, segmap=None):
        if threshold is not None:
            orig.threshold_correl = threshold
        if threshold_std is not None:
            orig.threshold_std = threshold_std
        self._loginfo('Thresholding correl (>%.2f) and std (>%.2f)', orig.threshold_correl,
                      orig.threshold_std)
        cat0, cat, cat_std = detection.from_session(orig, maxdist_lines=maxdist_lines)
        self._loginfo('%d detected lines', len(cat['z0']))
        self._loginfo('%d detected lines', len(cat0['z0']) - len(cat['z0']))
        self.Cat0 = cat0
        self._loginfo('kept %d lines from std after filtering', len(cat_std['z0']))

        if segmap is not None:
            self.logger.info('Overriding segmap_cont with the given one')
            seg = _data(segmap)
            if seg.shape != tuple(orig.shape[1:]):
                raise ValueError('segmap does not have the same shape as the processed cube')
        else:
            self.logger.info('Using segmap_cont as it is: the deblending step is the caller\'s '
                             '(pass its result as segmap)')
            seg = _data(orig.segmap_cont)
        self.store_image('segmap_label', seg)

        self.logger.info('Spatio-spectral merging...')
        self._loginfo('Purity estimation')
        cat1 = detection.make_cat1(_ctx_of(orig), cat, cat_std, seg, orig.Pval, orig.Pval_comp,
                                   tol_spat, tol_spec, getattr(orig, 'wcs', None),
                                   getattr(orig, 'wave', None))
        comp = cat1['comp'] == 1
        ns = len(set(cat1['ID']))
        ds = len(set(cat1['ID'][comp]) - set(cat1['ID']))
        self.Cat1 = cat1
        msg = 'Save the catalog in self.Cat1 (%d [+%s] sources, %d [+%d] lines)'
        self._loginfo(msg, ns, ds, len(comp), int(np.count_nonzero(comp)))


class _ComputeSpectraRun(_HipStepMixin):
    """ComputeSpectra.run (reference steps.py:1082-1118) through ``origin_amd.lines``.
    ``spectra`` is an ``OrderedDict num_line -> (data, var, z_min)``: the estimated line and its
    variance on the channels ``z_min .. z_min + len(data) - 1``, that is ``z - r .. z + r`` clipped
    to the cube with ``r = ceil(FWHM_profiles[profile] * spectrum_size_fwhm / 2)`` (:1104-1116;
    the reference wraps the same window in an mpdaf ``Spectrum``).  Without
    ``orig.FWHM_profiles`` the lines are kept whole (``z_min`` 0).  Fallback rows
    (``len(data) == 1``) have no spectrum, as at :1112."""
    name = 'compute_spectra'
    desc = 'Lines estimation'
    require = ('detection',)

    def run(self, orig, grid_dxy=0, spectrum_size_fwhm=6):
        cat2, line_est, line_var = lines.from_session(orig, orig.Cat1, grid_dxy)
        self.Cat2 = cat2
        self._loginfo('Save the updated catalog in self.Cat2 (%d lines)', len(cat2['z']))

        fwhm = getattr(orig, 'FWHM_profiles', None)
        radius = None
        if fwhm is not None:   # radius for spectrum trimming
            radius = np.ceil(np.array(fwhm) * spectrum_size_fwhm / 2).astype(int)
        spectra = OrderedDict()
        for profile, z, num_line, data, vari in zip(cat2['profile'], cat2['z'], cat2['num_line'],
                                                    line_est, line_var):
            if len(data) <= 1:
                continue
            z_min, z_max = 0, len(data)
            if radius is not None:
                z_min = max(int(z) - int(radius[profile]), 0)
                z_max = min(int(z) + int(radius[profile]) + 1, len(data))
            spectra[int(num_line)] = (data[z_min:z_max], vari[z_min:z_max], z_min)
        self.spectra = spectra
        self._loginfo('Save estimated spectrum of each line in self.spectra')


class _CleanResultsRun(_HipStepMixin):
    """CleanResults.run (reference steps.py:1149-1171) through ``origin_amd.catalog``: the table
    work on the host, the two cube standard deviations of ``add_tglr_stat`` as reductions of the
    cubes in HBM (csrc/stats.hip)."""
    name = 'clean_results'
    desc = 'Results cleaning'
    require = ('compute_spectra',)

    def run(self, orig, merge_lines_z_threshold=5):
        lines_, src, ts = catalog.from_session(
            orig, merge_lines_z_threshold=merge_lines_z_threshold)
        self.Cat3_lines = Catalog(lines_, {'CAT3_TS': ts})
        self.Cat3_sources = Catalog(src, {'CAT3_TS': ts})
        self._loginfo('Save the unique source catalog in self.Cat3_sources (%d sources)',
                      len(src['ID']))
        self._loginfo('Save the cleaned lines in self.Cat3_lines (%d lines)', len(lines_['ID']))
        nb_line_merged = int(np.sum(lines_['merged_in'] != catalog.NOT_MERGED))
        if nb_line_merged:
            self._loginfo('%d lines were merged in nearby lines', nb_line_merged)


# ndarray of an image attribute (mpdaf Image under the reference, ndarray here)
_data = cubes.host_array


def _glr_halo(orig, size=3):
    """Spaxels the GLR of step 5 and its local maxima read beyond a rank's own: half the PSF's
    side (PSF_size, origin.py:161) plus half the maximum filter's (steps.py:756 ``size=3``)."""
    psf = orig.PSF[0] if isinstance(orig.PSF, (list, tuple)) else orig.PSF
    return int(np.asarray(psf).shape[-1]) // 2 + int(size) // 2


# ----------------------------------------------------------------------------- stand-alone
class Preprocessing(_PreprocessingRun, Step):
    cube_std = DataObj('cube')
    cont_dct = DataObj('cube')
    ima_std = DataObj('image')
    ima_dct = DataObj('image')
    segmap_cont = DataObj('image')
    segmap_merged = DataObj('image')
    cube_std_local_min = DataObj('cube')
    cube_std_local_max = DataObj('cube')


class CreateAreas(_CreateAreasRun, Step):
    areamap = DataObj('image')



class ComputePCAThreshold(_ComputePCAThresholdRun, Step):
    thresO2 = DataObj('array')
    meaO2 = DataObj('array')
    stdO2 = DataObj('array')


class ComputeGreedyPCA(_ComputeGreedyPCARun, Step):
    cube_faint = DataObj('cube')
    mapO2 = DataObj('image')


class ComputeTGLR(_ComputeTGLRRun, Step):
    cube_correl = DataObj('cube')
    cube_correl_min = DataObj('cube')
    cube_profile = DataObj('cube')
    cube_local_min = DataObj('cube')
    cube_local_max = DataObj('cube')
    maxmap = DataObj('image')
    minmap = DataObj('image')


class ComputePurityThreshold(_ComputePurityThresholdRun, Step):
    __doc__ = _ComputePurityThresholdRun.__doc__
    Pval = DataObj('table')
    Pval_comp = DataObj('table')
    segmap_purity = DataObj('image')


class Detection(_DetectionRun, Step):
    __doc__ = _DetectionRun.__doc__
    on_demand = True
    Cat0 = DataObj('table')
    Cat1 = DataObj('table')
    segmap_label = DataObj('image')


class ComputeSpectra(_ComputeSpectraRun, Step):
    __doc__ = _ComputeSpectraRun.__doc__
    on_demand = True
    Cat2 = DataObj('table')
    spectra = DataObj('spectra')


class CleanResults(_CleanResultsRun, Step):
    __doc__ = _CleanResultsRun.__doc__
    on_demand = True
    Cat3_lines = DataObj('table')
    Cat3_sources = DataObj('table')


# (steps 10 and 11 of the reference -- CreateMasks, SaveSources -- are not here: DESIGN.md 7)
STEPS = [Preprocessing, CreateAreas, ComputePCAThreshold, ComputeGreedyPCA, ComputeTGLR,
         ComputePurityThreshold, Detection, ComputeSpectra, CleanResults]


class _SessionSteps(OrderedDict):
    """The steps of a session by name, in ``STEPS`` order; looking up an ``on_demand`` step that
    has not been used yet makes it."""

    def __init__(self, make):
        super().__init__()
        self._make = make

    def __missing__(self, name):
        return self._make(name)


class SimpleOrig:
    """Stand-in for the ``ORIGIN`` session object carrying exactly what the four hot ``run``
    bodies read: cube_raw, var, mask, FWHM_PSF, PSF, wfields, profiles,
    nbAreas, areamap, param, testO2, thresO2, cube_std, cube_faint.  Steps are bound as
    ``stepNN_name`` callables like origin.py:193-208 does.  Steps 1-6 are made with the session;
    steps 7-9 (``Step.on_demand``) when their method, one of their outputs or ``steps[name]`` is
    first used, so a session that stops at step 6 lists, dumps and records in ``param`` what it
    always did."""

    def __init__(self, cube_raw, var, mask, PSF, profiles, FWHM_PSF=3.3, wfields=None,
                 param=None, ctx=None, devices=None, backend=None, FWHM_profiles=None):
        """``FWHM_profiles``: FWHM of every profile of the dictionary in channels (origin.py:168),
        the window of the spectra step 8 keeps; None keeps the lines whole.
        ``devices``: None (one context, ``ctx`` or device 0) or a list of device ordinals --
        the hot steps then run tiled over them in this one process (origin_amd/session.py); the
        same ordinal twice = two contexts on one card.  ``backend``: "rccl" / "host" for the
        cubes that travel between them (default: RCCL when the ordinals differ)."""
        self.hip_devices = list(devices) if devices is not None else None
        self.hip_backend = backend
        self.cube_raw, self.var, self.mask = cube_raw, var, mask
        self.PSF, self.wfields, self.profiles = PSF, wfields, profiles
        self.FWHM_PSF = FWHM_PSF
        self.FWHM_profiles = FWHM_profiles
        self.param = param or {}
        self.wave = self.wcs = None
        self.testO2 = self.histO2 = self.binO2 = None
        self.hip_ctx = ctx or default_context(0 if not devices else int(devices[0]))
        self.steps = _SessionSteps(self._make_step)
        self._dataobjs = {}
        self._on_demand = {}       # name -> (idx, class) of the steps not made yet
        for i, cls in enumerate(STEPS, start=1):
            if cls.on_demand:
                self._on_demand[cls.name] = (i, cls)
            else:
                self._bind(i, cls)

    @classmethod
    def from_cube(cls, cube, profiles, PSF, FWHM_PSF, LBDA_FWHM_PSF=None, wfields=None,
                  FWHM_profiles=None, ctx=None, devices=None, backend=None, param=None, dq=False):
        """Step 0 of the reference (``ORIGIN.__init__``, origin.py:210-244): a session from the
        path of a MUSE cube file.  The file's bytes go to HBM and one kernel leaves cube_raw, var
        and mask there (``fitsio.read_cube``); ``cube_raw`` / ``var`` / ``mask`` of the session
        are ``LazyCube``s over them (float64 / float64 / bool on demand, as the reference holds
        them), ``ima_white`` the masked mean over z, ``wcs_header`` / ``wave_header`` the world
        coordinates of the DATA header, which ``Step.dump`` writes back.  ``dq=True`` also masks
        the voxels a DQ extension flags (element != 0); by default the extension is ignored with
        a warning.

        ``profiles``: the path of a dictionary (``fitsio.read_profiles``: fills ``FWHM_profiles``
        too) or a list of arrays.  ``PSF``: a ``(Nz, P, P)`` array or the path of its file, or a
        list of either with ``wfields`` (paths or ``(Ny, Nx)`` arrays), one per field of a mosaic;
        checked as origin.py:619-628.  ``FWHM_PSF``: in pixels, one per field.  Building the FSF
        from the ``FSF*`` keywords of the cube's header (``PSF=None`` in the reference) is
        mpdaf's ``FSFModel`` and is not here.  ``param['cubename']``, ``['profiles']`` and
        ``['PSF']`` record the paths.  With two or more ``devices`` every rank of the tiled
        session reads the rows of its own band of step 1 from the file into its own context
        (``TiledSession.open_cube``): the ``LazyCube``s then lie over ``TiledCube``s, step 1 runs
        on the bands where they are, and the whole field is gathered only when somebody reads
        ``._data`` or a later single-device step asks for it."""
        info = fitsio.open_cube(cube, dq=dq)
        if PSF is None:
            raise ValueError(
                "PSF=None: building the FSF from the FSF* keywords of the cube header is mpdaf's "
                "FSFModel and is not part of origin_amd; give the PSF cube(s) and FWHM_PSF")
        Nz, Ny, Nx = info.shape
        param = dict(param or {})
        param['cubename'] = cube
        param['profiles'] = profiles if isinstance(profiles, str) else None
        if isinstance(profiles, str):
            profiles, fwhm = fitsio.read_profiles(profiles)
            FWHM_profiles = fwhm if FWHM_profiles is None else FWHM_profiles
        elif len({np.asarray(p).shape[0] for p in profiles}) != 1:
            raise ValueError("The profiles must have the same size")

        def host(a):
            return fitsio.read_host_image(a) if isinstance(a, str) else np.asarray(a)

        def check_psf(psf):
            if psf.ndim != 3 or psf.shape[1] != psf.shape[2]:
                raise ValueError("PSF must be a square image.")
            if not psf.shape[1] % 2:
                raise ValueError("The spatial size of the PSF must be odd.")
            if psf.shape[0] != Nz:
                raise ValueError("PSF and data cube have not the same dimensions along the "
                                 "spectral axis.")
            return psf

        if isinstance(PSF, (list, tuple)):
            if wfields is None or len(wfields) != len(PSF):
                raise ValueError("a list of PSFs needs one weight map (wfields) per field")
            param['PSF'] = list(PSF) if all(isinstance(p, str) for p in PSF) else None
            PSF = [check_psf(host(p)) for p in PSF]
            wfields = [host(w) for w in wfields]
            for w in wfields:
                if w.shape != (Ny, Nx):
                    raise ValueError(f"weight map {w.shape} for a field of {(Ny, Nx)}")
            FWHM_PSF = list(np.atleast_1d(FWHM_PSF))
        else:
            param['PSF'] = PSF if isinstance(PSF, str) else None
            PSF, wfields = check_psf(host(PSF)), None
            FWHM_PSF = float(np.mean(FWHM_PSF))
        ctx = ctx or default_context(0 if not devices else int(devices[0]))
        orig = cls(None, None, None, PSF, profiles, FWHM_PSF=FWHM_PSF, wfields=wfields,
                   param=param, ctx=ctx, devices=devices, backend=backend,
                   FWHM_profiles=FWHM_profiles)
        sess = _session_of(orig)
        if sess is not None:               # every rank reads the rows of its band of step 1
            raw, var, mask, ima_white = sess.open_cube(info, dq=dq)
            wcs, wave = info.wcs_header, info.wave_header
        else:
            raw, var, mask, ima_white, wcs, wave = fitsio.read_cube(cube, ctx, dq=dq)
            # where _inputs_on_device looks for them
            _cache(orig).update(raw=raw, var=var, mask=mask)
        orig.cube_raw, orig.var, orig.mask = LazyCube(raw), LazyCube(var), LazyCube(mask, dtype=bool)
        orig.LBDA_FWHM_PSF = LBDA_FWHM_PSF
        orig.ima_white, orig.wcs_header, orig.wave_header = ima_white, wcs, wave
        return orig

    def _bind(self, idx, cls):
        step = cls(self, idx, self.param)
        self.steps[step.name] = step
        for name in sorted(self.steps, key=lambda n: self.steps[n].idx):   # keep the STEPS order
            self.steps.move_to_end(name)
        self.__dict__[step.method_name] = step
        for name, _ in step._dataobjs:
            self._dataobjs[name] = step
        return step

    def _make_step(self, name):
        """An ``on_demand`` step at its first use (KeyError for a name that is no step)."""
        idx, cls = self.__dict__.get('_on_demand', {}).pop(name)
        return self._bind(idx, cls)

    def __getattr__(self, name):
        # the method or an output of a step that has not been made yet makes it
        for sname, (idx, cls) in list(self.__dict__.get('_on_demand', {}).items()):
            if name == f'step{idx:02d}_{sname}' or any(name == n for n, _ in cls._dataobjs):
                self._make_step(sname)
                return getattr(self, name)
        d = self.__dict__.get('_dataobjs', {})
        if name in d:
            return getattr(d[name], name)
        raise AttributeError(f"unknown attribute {name}")

    @property
    def nbAreas(self):
        return self.param.get('nbareas')

    @property
    def shape(self):
        """(Nz, Ny, Nx) of the processed cube."""
        if hasattr(self.cube_raw, 'shape'):      # (no host copy for a shape: a LazyCube has one)
            return tuple(self.cube_raw.shape)
        return tuple(_data(self.cube_raw).shape)

    # the thresholds of step 6, overridden by step 7's keywords (origin.py:496-513)
    @property
    def threshold_correl(self):
        """Estimated threshold used to detect lines on local maxima of max correl."""
        return self.param.get('threshold')

    @threshold_correl.setter
    def threshold_correl(self, value):
        self.param['threshold'] = value

    @property
    def threshold_std(self):
        """Estimated threshold used to detect complementary lines on local maxima of std cube."""
        return self.param.get('threshold_std')

    @threshold_std.setter
    def threshold_std(self, value):
        self.param['threshold_std'] = value


# ----------------------------------------------------------------------------- register
def register(devices=None):
    """Swap GPU versions of the six steps built here into ``muse_origin.steps.STEPS``.  Call
    before constructing ``ORIGIN`` (origin.py:193 reads the list then).  Returns the list of
    replaced class names.  ``devices``: list of device ordinals the sessions made afterwards
    spread their hot steps over (one process, one context per entry: origin_amd/session.py);
    None = one context on device 0.

    Each replacement is ``class <Name>(<run mixin>, <reference class>)`` made with the
    reference's own metaclass.  That metaclass rebuilds ``_dataobjs`` from the attributes of
    the class body alone (steps.py:176-185), which is empty here -- the DataObj descriptors
    are inherited -- so the list is copied over from the reference class afterwards;
    ``ORIGIN.__init__`` (origin.py:206-207), ``Step.dump`` and ``Step.load`` all walk it."""
    import muse_origin.steps as ref  # noqa: raises ImportError when the reference is absent

    global _DEFAULT_DEVICES
    _DEFAULT_DEVICES = list(devices) if devices is not None else None
    replaced = []
    for mixin, refname in ((_PreprocessingRun, 'Preprocessing'),
                           (_CreateAreasRun, 'CreateAreas'),
                           (_ComputePCAThresholdRun, 'ComputePCAThreshold'),
                           (_ComputeGreedyPCARun, 'ComputeGreedyPCA'),
                           (_ComputeTGLRRun, 'ComputeTGLR'),
                           (_ComputePurityThresholdRun, 'ComputePurityThreshold')):
        base = getattr(ref, refname)
        if getattr(base, '_origin_amd_base', None) is not None:   # already registered
            replaced.append(refname)
            continue
        new = type(base)(refname, (mixin, base), {'__doc__': base.__doc__,
                                                  '__module__': base.__module__})
        new._dataobjs = list(base._dataobjs)
        new._Status = ref.Status
        new._origin_amd_base = base
        ref.STEPS[ref.STEPS.index(base)] = new
        setattr(ref, refname, new)
        replaced.append(refname)
    return replaced


def unregister():
    """Put the reference's own classes back (tests; A/B runs of one session)."""
    import muse_origin.steps as ref
    for i, cls in enumerate(list(ref.STEPS)):
        base = getattr(cls, '_origin_amd_base', None)
        if base is not None:
            ref.STEPS[i] = base
            setattr(ref, base.__name__, base)
