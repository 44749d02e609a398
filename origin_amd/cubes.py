"""The forms a cube takes between the steps, and the one place that tells them apart (DESIGN.md
section 3e′).

Steps 1 and 5 leave their cubes in HBM as a ``DeviceArray``, a ``sparse.SparseCube`` (the
local-maximum cubes as lists) or a ``session.TiledCube`` (pieces on several contexts, dense or
sparse); a DataObj may also hold a ``LazyCube``, a ``fitsio.FitsCube``, a host array or an mpdaf
object with ``._data``.  ``resident`` is the single ladder over them; the five reductions that
steps 6, 7 and 9 make of a resident cube -- ``zmax_map``, ``count_above``, ``where_above``,
``moments``, ``std`` -- have one dispatch each: a ``DeviceArray`` goes to ``kernels.*``, a
``CubeForm`` answers itself.  A new form subclasses ``CubeForm``, brings the first four and
``gathered``, and is resident by that; one that has to be resolved first (a file, a lazy copy)
adds its rung to ``resident``.
"""
import numpy as np

from . import fitsio, kernels
from .device import DeviceArray, default_context


# ------------------------------------------------------------------------------- forms
class CubeForm:
    """Base of the device-resident forms other than a plain ``DeviceArray``.  A subclass has
    ``shape``, ``dtype``, ``to_host()``, ``gathered(ctx)`` (one dense DeviceArray on ``ctx``) and
    ``zmax_map`` / ``count_above`` / ``where_above`` / ``moments`` with the signatures of the
    functions below, less their first argument."""

    def std(self):
        return std(self)


class LazyCube:
    """What a DataObj holds when mpdaf is absent: a device array plus an on-demand host
    copy with the dtype the reference would have produced.  ``._data`` / ``.data`` mirror
    the mpdaf attribute the ``run`` bodies read (e.g. steps.py:617, :688, :771)."""

    def __init__(self, dev=None, host=None, dtype=np.float64):
        self.dev, self._host, self._dtype = dev, host, dtype

    @property
    def _data(self):
        if self._host is None:
            self._host = (self.dev.to_host_f64() if self._dtype == np.float64
                          else self.dev.to_host().astype(self._dtype, copy=False))
        return self._host

    data = _data

    @property
    def shape(self):
        return self.dev.shape if self.dev is not None else self._host.shape

    def device(self, ctx, dtype=np.float32):
        if self.dev is None:
            self.dev = ctx.to_device(self._host, dtype)
        return self.dev


def host_array(value):
    """Host ndarray of anything cube- or image-like: a resident form is read back, an mpdaf
    object (or a ``LazyCube`` / ``FitsCube``) gives its ``._data``."""
    if isinstance(value, (DeviceArray, CubeForm)):
        return value.to_host()
    return np.asarray(getattr(value, "_data", value))


def host_mask(mask, shape):
    """The mask on the host as it is held (bool or uint8); zeros of ``shape`` for ``None`` /
    ``np.ma.nomask``."""
    if mask is None or mask is np.ma.nomask:
        return np.zeros(shape, np.uint8)
    return host_array(mask)


def resident(ctx, value, dtype=np.float32):
    """``value`` in the device-resident form it already has (DeviceArray, SparseCube, TiledCube);
    a ``LazyCube`` / ``FitsCube`` is resolved, host data (ndarray, mpdaf object) uploaded as
    ``dtype``."""
    if isinstance(value, (LazyCube, fitsio.FitsCube)):
        value = value.device(ctx, dtype)
    if isinstance(value, (DeviceArray, CubeForm)):
        return value
    return ctx.to_device(host_array(value), dtype)


def dense(ctx, value, dtype=np.float32):
    """``resident`` as one DeviceArray on ``ctx``: the lists of a SparseCube scattered, the pieces
    of a TiledCube gathered."""
    cube = resident(ctx, value, dtype)
    return cube if isinstance(cube, DeviceArray) else cube.gathered(ctx)


def keep_map(ctx, keep, n_spaxels):
    """The map of the spaxels to keep as the kernels take it: None, or a flat uint8 DeviceArray
    with one entry per spaxel, from a host bool / uint8 map of any shape or a DeviceArray."""
    if keep is None:
        return None
    if not isinstance(keep, DeviceArray):
        keep = ctx.to_device(np.ascontiguousarray(keep, dtype=np.uint8).reshape(-1))
    if keep.dtype != np.uint8 or keep.size != n_spaxels:
        raise ValueError("keep must be a uint8 map with one entry per spaxel")
    return keep


# ------------------------------------------------------------------------------- reductions
def _keep_of(cube, keep):
    return keep_map(cube.ctx, keep, cube.size // cube.shape[0])


def zmax_map(cube, keep=None):
    """max over z per spaxel -> host float64 (Ny, Nx); spaxels with keep == 0 give 0."""
    if isinstance(cube, DeviceArray):
        return kernels.zmax_map(cube.ctx, cube, _keep_of(cube, keep))
    return cube.zmax_map(keep)


def count_above(cube, thresholds, keep=None):
    """counts[t] = #{kept voxels > thresholds[t]} (int64, host)."""
    if isinstance(cube, DeviceArray):
        return kernels.count_above(cube.ctx, cube, thresholds, _keep_of(cube, keep))
    return cube.count_above(thresholds, keep)


def where_above(cube, threshold, aux=None):
    """``np.where(cube > threshold)`` in NumPy's order with the values there (and those of the
    uint8 cube ``aux``, resident in the same form): ``kernels.where_above``'s dict."""
    if isinstance(cube, DeviceArray):
        return kernels.where_above(cube.ctx, cube, threshold, aux=aux)
    return cube.where_above(threshold, aux=aux)


def moments(cube, shift=0.0, keep=None):
    """``(n, sum(x - shift), sum((x - shift)**2))`` over the kept voxels (kernels.cube_moments)."""
    if isinstance(cube, DeviceArray):
        return kernels.cube_moments(cube.ctx, cube, shift, _keep_of(cube, keep))
    return cube.moments(shift, keep)


def std(cube):
    """``np.std`` of the cube in NumPy's own two-pass form (``kernels.two_pass_std``): the global
    mean of the first pass is the shift of the second, on every part of a tiled cube."""
    return kernels.two_pass_std(lambda shift: moments(cube, shift))


# ------------------------------------------------------------------------------- sessions
# What a session object (``steps.SimpleOrig``, the reference's ORIGIN under register()) keeps for
# the GPU: ``hip_ctx`` and the cubes left in HBM, ``_hip_cache``.
def ctx_of(orig):
    ctx = getattr(orig, 'hip_ctx', None)
    if ctx is None:
        ctx = default_context(0)
        try:
            orig.hip_ctx = ctx
        except Exception:
            pass
    return ctx


def cache(orig):
    c = orig.__dict__.get('_hip_cache')
    if c is None:
        c = orig.__dict__['_hip_cache'] = {}
    return c


def inputs_on_device(orig, ctx):
    """cube_raw / var / mask uploaded once per session (origin.py:262-274)."""
    c = cache(orig)
    if 'raw' not in c:
        c['raw'] = dense(ctx, orig.cube_raw)
        c['var'] = dense(ctx, orig.var)
        # (a bool mask goes up as it is: one byte of 0 / 1 per voxel, no host-side copy)
        c['mask'] = dense(ctx, host_mask(orig.mask, c['raw'].shape), np.uint8)
    return c['raw'], c['var'], c['mask']


def session_cube(orig, name, dtype=np.float32):
    """The resident form of the session's cube ``name``: what a step left in HBM when it is still
    there, the DataObj's value (uploaded, or decoded from its file) otherwise."""
    cube = cache(orig).get(name)
    if cube is not None:
        return cube
    return resident(ctx_of(orig), getattr(orig, name), dtype)
