"""Device-level stage functions: thin, typed wrappers over the C ABI working on
``DeviceArray`` s.  Everything here is asynchronous on the context's stream unless it
returns host values."""
import ctypes as C

import numpy as np

from . import _capi
from .device import DeviceArray

NULL = C.c_void_p(0)


def _p(a):
    return NULL if a is None else a.p


# ------------------------------------------------------------------------- DCT / O2
def dct_fit(ctx, raw, var, mask, order=10, approx=False, coef=None):
    Nz, Ny, Nx = raw.shape
    if coef is None:
        coef = ctx.empty((order + 1, Ny, Nx), np.float64)
    _capi.call("origin_dct_fit", ctx.handle, raw.p, var.p, mask.p, Nz, Ny, Nx, int(order),
               int(bool(approx)), coef.p)
    return coef


def dct_fit_sums(ctx, raw, var, mask, order=10, approx=False, coef=None, zsum=None, zcnt=None):
    """``dct_fit`` and ``dct_resid_sums`` in one call: the per-channel sums of raw over the
    unmasked spaxels are taken inside the moments pass, which reads raw and mask anyway (the
    5 B/voxel plane pass becomes a mask-only visit of the spaxel groups that have masked voxels).
    Returns (coef, zsum, zcnt)."""
    Nz, Ny, Nx = raw.shape
    if coef is None:
        coef = ctx.empty((order + 1, Ny, Nx), np.float64)
    zsum = ctx.empty((Nz,), np.float64) if zsum is None else zsum
    zcnt = ctx.empty((Nz,), np.float64) if zcnt is None else zcnt
    _capi.call("origin_dct_fit_sums", ctx.handle, raw.p, var.p, mask.p, Nz, Ny, Nx, int(order),
               int(bool(approx)), coef.p, zsum.p, zcnt.p)
    return coef, zsum, zcnt


def dct_continuum(ctx, coef, Nz, out=None):
    na, Ny, Nx = coef.shape
    if out is None:
        out = ctx.empty((Nz, Ny, Nx), np.float32)
    _capi.call("origin_dct_continuum", ctx.handle, coef.p, Nz, Ny, Nx, na - 1, out.p)
    return out


def dct_resid_sums(ctx, raw, mask, coef, zsum=None, zcnt=None):
    Nz, Ny, Nx = raw.shape
    zsum = ctx.empty((Nz,), np.float64) if zsum is None else zsum
    zcnt = ctx.empty((Nz,), np.float64) if zcnt is None else zcnt
    _capi.call("origin_dct_resid_sums", ctx.handle, raw.p, mask.p, coef.p, Nz, Ny, Nx,
               coef.shape[0] - 1, zsum.p, zcnt.p)
    return zsum, zcnt


def dct_standardize(ctx, raw, var, mask, coef, zsum, zcnt, cube_std=None, cont_dct=None,
                    want_cont=True, want_images=True, o2=None, ima_std=None):
    Nz, Ny, Nx = raw.shape
    cube_std = ctx.empty((Nz, Ny, Nx), np.float32) if cube_std is None else cube_std
    if cont_dct is None and want_cont:
        cont_dct = ctx.empty((Nz, Ny, Nx), np.float32)
    if ima_std is None and want_images:
        ima_std = ctx.empty((Ny, Nx), np.float32)
    ima_dct = ctx.empty((Ny, Nx), np.float32) if (want_images and cont_dct is not None) else None
    if o2 is None and want_images:
        o2 = ctx.empty((Ny, Nx), np.float64)
    _capi.call("origin_dct_standardize", ctx.handle, raw.p, var.p, mask.p, coef.p, zsum.p,
               zcnt.p, Nz, Ny, Nx, coef.shape[0] - 1, cube_std.p, _p(cont_dct), _p(ima_std),
               _p(ima_dct), _p(o2))
    return dict(cube_std=cube_std, cont_dct=cont_dct, ima_std=ima_std, ima_dct=ima_dct, o2=o2)


def dct_cont_std(ctx, var, coef, cont_dct=None, want_image=True, ima_dct=None, aux=False):
    """cont_dct = continuum / sqrt(var) and its mean image, as a pass of its own (what
    ``dct_standardize(want_cont=False)`` leaves out).  Give ``cont_dct`` / ``ima_dct`` buffers to
    keep the call free of allocations (an allocation can wait for the device).  ``aux``: on the
    context's low-priority auxiliary stream -- ``ctx.aux_join()`` or ``ctx.sync()`` before the
    outputs are read or ``var`` / ``coef`` rewritten."""
    Nz, Ny, Nx = var.shape
    cont_dct = ctx.empty((Nz, Ny, Nx), np.float32) if cont_dct is None else cont_dct
    if ima_dct is None and want_image:
        ima_dct = ctx.empty((Ny, Nx), np.float32)
    _capi.call("origin_dct_cont_std_async" if aux else "origin_dct_cont_std", ctx.handle, var.p,
               coef.p, Nz, Ny, Nx, coef.shape[0] - 1, cont_dct.p, _p(ima_dct))
    return dict(cont_dct=cont_dct, ima_dct=ima_dct)


def o2test(ctx, cube, out=None):
    Nz = cube.shape[0]
    S = cube.size // Nz
    out = ctx.empty(cube.shape[1:], np.float64) if out is None else out
    _capi.call("origin_o2", ctx.handle, cube.p, Nz, S, out.p)
    return out


# ------------------------------------------------------------------------- GLR
def prepare_profiles(profiles, pcut=None, pmeansub=True):
    """Trim / normalise / mean-subtract the dictionary exactly as the reference does
    (lib_origin.py:1155-1165), in float64 on the host (K small vectors)."""
    out = []
    for prof in profiles:
        prof = np.array(prof, dtype=np.float64)
        if pcut is not None:
            lpeak = prof.argmax()
            lw = np.max(np.abs(np.where(prof >= pcut)[0][[0, -1]] - lpeak))
            prof = prof[lpeak - lw: lpeak + lw + 1]
        prof /= np.linalg.norm(prof)
        if pmeansub:
            prof -= prof.mean()
        out.append(prof)
    return out


# PSF sizes whose spatial stage runs on the matrix cores (mirrors origin_spatial_mfma_ok,
# csrc/glr_spatial_mfma.hip): every odd size from 5 to 25 and the large ones measured faster
# there than on the fp32 kernels
SPATIAL_MFMA_SIZES = frozenset(range(5, 26, 2)) | frozenset(range(27, 42, 2))


class GLRPlan:
    """Device-side constants of a GLR run: zero-mean PSFs, weights, prepared profiles and
    normalisation tables (include/origin_hip.h: origin_glr_plan)."""

    PRECISIONS = ("f32", "f16x2", "bf16")   # origin_glr_plan_set_precision codes 0, 1, 2

    def __init__(self, ctx, shape, fsf, weights, profiles, pcut=None, pmeansub=True,
                 precision=None):
        """``precision``: None = library default ("f16x2" where eligible), "f16x2" = both GLR stages
        on the matrix cores with a two-term f16 split (fp32 accumulation, fp32-class results),
        "bf16" = spectral stage with ONE bf16 MFMA per product (BASELINE config 4: SURVEY 8c
        bf16 tolerances), "f32" = fp32 FMA kernels.  ``self.precision`` tells what the plan will
        run (plans with weight maps or very wide profiles only have "f32")."""
        Nz, Ny, Nx = (int(s) for s in shape)
        self.ctx, self.shape = ctx, (Nz, Ny, Nx)
        if weights is None:  # one FSF                         (lib_origin.py:1112-1114)
            fsf_list, w = [fsf], None
        else:
            fsf_list, w = list(fsf), [np.asarray(x, dtype=np.float64) for x in weights]
            if len(fsf_list) != len(w):
                raise ValueError("need one weight map per FSF")
        psf = np.ascontiguousarray(np.stack([np.asarray(f, dtype=np.float64) for f in fsf_list]))
        if psf.ndim != 4 or psf.shape[1] != Nz or psf.shape[2] != psf.shape[3]:
            raise ValueError(f"FSF must be (Nz, P, P) per field, got {psf.shape[1:]}")
        self.P = psf.shape[2]
        wptr = NULL
        if w is not None:
            warr = np.ascontiguousarray(np.stack(w))
            if warr.shape != (len(fsf_list), Ny, Nx):
                raise ValueError("weight maps must be (Ny, Nx)")
            wptr = warr.ctypes.data_as(C.c_void_p)
        prof = prepare_profiles(profiles, pcut, pmeansub)
        self.K = len(prof)
        self.tap_lengths = [len(p) for p in prof]
        off = np.zeros(self.K + 1, dtype=np.int32)
        off[1:] = np.cumsum(self.tap_lengths)
        taps = np.ascontiguousarray(np.concatenate(prof))
        self._h = C.c_void_p()
        _capi.call("origin_glr_plan_create", ctx.handle, Nz, Ny, Nx, len(fsf_list), self.P,
                   psf.ctypes.data_as(C.c_void_p), wptr, self.K,
                   taps.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                   C.byref(self._h))
        n = C.c_size_t()
        _capi.call("origin_glr_work_elems", self._h, C.byref(n))
        self.work_elems = n.value
        _capi.call("origin_glr_plan_bytes", self._h, C.byref(n))
        self.nbytes = n.value
        self._work = None
        if precision is not None:
            if precision not in self.PRECISIONS:
                raise ValueError("precision must be None, 'f32', 'f16x2' or 'bf16'")
            _capi.call("origin_glr_plan_set_precision", self._h, self.PRECISIONS.index(precision))
        got = C.c_int()
        _capi.call("origin_glr_plan_get_precision", self._h, C.byref(got))
        self.precision = self.PRECISIONS[got.value]
        # mirrors origin_spatial_mfma_ok (csrc/glr_spatial_mfma.hip): which spatial kernel runs
        # (weighted mosaics included: per-field accumulation on the matrix cores; their spectral
        # stage convolves the norm cube next to the data and stays in fp32)
        self.spatial_on_matrix_cores = self.precision != "f32" and self.P in SPATIAL_MFMA_SIZES
        # (a weighted plan's spectral stage -- second Toeplitz product for the denominator,
        # csrc/glr_spectral_norm_mfma.hip -- exists for the f16 split only)
        self.spectral_on_matrix_cores = self.precision != "f32" and (
            w is None or (self.precision == "f16x2" and len(self.tap_lengths) <= 26
                          and max(self.tap_lengths) <= 65))

    # -- the same run in row bands (include/origin_hip.h origin_glr_run_rows) ---------------
    def prepare(self):
        """What a plan with weight maps owes before its spectral form is known, now instead of
        inside its first ``run``: the norm cube, then eps of the FOLD form measured on it
        (include/origin_hip.h origin_glr_plan_prepare).  On the main stream, which it
        synchronises: call it ahead of the step, never from a PCA tail hook.  Idempotent; nothing
        to do for a plan without weight maps.  Returns self."""
        _capi.call("origin_glr_plan_prepare", self.ctx.handle, self._h)
        return self

    def rows_supported(self):
        """Whether the plan runs in row bands and rectangles: both stages on the matrix cores (a
        PSF size of SPATIAL_MFMA_SIZES, half widths <= 32, K <= 26) -- one field without weight
        maps, or a mosaic of weighted fields once ``prepare()`` has made its norm cube and
        measured eps (the FOLD form on the norm cube, or the two-product kernel at "f16x2").  A
        weighted plan answers False before ``prepare()``, at "f32", and at "bf16" when its eps
        test fails."""
        ok = C.c_int()
        _capi.call("origin_glr_rows_supported", self._h, C.byref(ok))
        return bool(ok.value)

    def run_rows(self, cube, mask, correl, profile, correl_min, y0, y1, first=False, side=False):
        """The rows [y0, y1) of a run (y0 a multiple of 64, y1 one or Ny): spatial stage (reads
        cube rows [y0 - P//2, y1 + P//2)), spectral stage, partial maps.  ``first``: the first band
        of a run; ``side``: enqueue on the context's side stream (all CUs but a reserve), behind
        what the main stream holds now.  A plan with weight maps accumulates its fields into the
        band and reads its norm cube: ``prepare()`` first (the band raises otherwise)."""
        assert cube.shape == self.shape and cube.dtype == np.float32
        _capi.call("origin_glr_run_rows", self.ctx.handle, self._h, cube.p, _p(mask),
                   self.workspace().p, correl.p, profile.p, correl_min.p, int(y0), int(y1),
                   (1 if first else 0) | (2 if side else 0))

    def run_rect(self, cube, mask, correl, profile, correl_min, y0, y1, x0, x1, first=False,
                 side=False):
        """Rows [y0, y1) x columns [x0, x1) of a run (each a multiple of 64 or the field's end);
        see ``run_rows`` (weighted plans included).  With a proper column range the results agree
        with ``run`` to rounding (the spectral stage's waves hold 32 columns of one row), not bit
        for bit."""
        assert cube.shape == self.shape and cube.dtype == np.float32
        _capi.call("origin_glr_run_rect", self.ctx.handle, self._h, cube.p, _p(mask),
                   self.workspace().p, correl.p, profile.p, correl_min.p, int(y0), int(y1), int(x0),
                   int(x1), (1 if first else 0) | (2 if side else 0))

    def run_finish(self, want_maps=True):
        """Ends a run in row bands: the main stream waits for the side bands; returns
        (maxmap, minmap) or (None, None)."""
        Nz, Ny, Nx = self.shape
        maxmap = self.ctx.empty((Ny, Nx), np.float32) if want_maps else None
        minmap = self.ctx.empty((Ny, Nx), np.float32) if want_maps else None
        _capi.call("origin_glr_run_finish", self.ctx.handle, self._h, self.workspace().p,
                   _p(maxmap), _p(minmap))
        return maxmap, minmap

    def mfma_count(self):
        """(spatial, spectral): matrix-core instructions (32768 flop each) one run issues per
        stage -- rocprofv3's SQ_INSTS_MFMA per launch; 0 for a stage on the fp32 kernels."""
        a, b = C.c_long(), C.c_long()
        _capi.call("origin_glr_plan_mfma_count", self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def fold_eps(self):
        """(eps, active): FOLD of the matrix-core spectral stage -- the plan's measured
        max |1/(a_k sqrt(den_k)) / s - 1| away from the cube's ends and whether the stage uses it
        (eps <= 2e-6, include/origin_hip.h origin_glr_plan_fold_eps)."""
        e, a = C.c_float(), C.c_int()
        _capi.call("origin_glr_plan_fold_eps", self._h, C.byref(e), C.byref(a))
        return e.value, bool(a.value)

    SPECTRAL_FORMS = ("table", "normw", "norm_mfma", "packed", "fp32", "generic")

    def paths(self):
        """Which kernels the next run takes (include/origin_hip.h origin_glr_plan_paths): a dict of
        ``spatial_mfma`` (bool), ``spectral`` (one of SPECTRAL_FORMS: the first three run on the
        matrix cores, the others are the fp32 FMA kernels of csrc/glr_fp32.hip), ``lwt`` (window
        half width of the packed form), ``lwmax`` (largest profile half width) and ``nborder``
        (spaxels of the packed form's border pass)."""
        v = [C.c_int() for _ in range(5)]
        _capi.call("origin_glr_plan_paths", self._h, *(C.byref(x) for x in v))
        return dict(spatial_mfma=bool(v[0].value), spectral=self.SPECTRAL_FORMS[v[1].value],
                    lwt=v[2].value, lwmax=v[3].value, nborder=v[4].value)

    def close(self):
        if self._h is not None and self._h.value:
            # (a plan outliving its context -- interpreter exit closes contexts first -- is not
            # destroyed through the dangling context pointer it holds: the process is ending)
            if self.ctx.handle.value:
                _capi.load().origin_glr_plan_destroy(self._h)
            self._h = C.c_void_p()
        self._work = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def workspace(self):
        if self._work is None:
            self._work = self.ctx.empty((self.work_elems,), np.float32)
        return self._work

    def run(self, cube, mask=None, correl=None, profile=None, correl_min=None, want_maps=True):
        ctx = self.ctx
        Nz, Ny, Nx = self.shape
        assert cube.shape == self.shape and cube.dtype == np.float32
        correl = ctx.empty(self.shape, np.float32) if correl is None else correl
        correl_min = ctx.empty(self.shape, np.float32) if correl_min is None else correl_min
        profile = ctx.empty(self.shape, np.uint8) if profile is None else profile
        maxmap = ctx.empty((Ny, Nx), np.float32) if want_maps else None
        minmap = ctx.empty((Ny, Nx), np.float32) if want_maps else None
        _capi.call("origin_glr_run", ctx.handle, self._h, cube.p, _p(mask), self.workspace().p,
                   correl.p, profile.p, correl_min.p, _p(maxmap), _p(minmap))
        return dict(correl=correl, profile=profile, correl_min=correl_min, maxmap=maxmap,
                    minmap=minmap)


def local_max(ctx, correl, correl_min, mask, size=3, out_max=None, out_min=None):
    Nz, Ny, Nx = correl.shape
    out_max = ctx.empty(correl.shape, np.float32) if out_max is None else out_max
    out_min = ctx.empty(correl.shape, np.float32) if out_min is None else out_min
    _capi.call("origin_local_max", ctx.handle, correl.p, correl_min.p, _p(mask), Nz, Ny, Nx,
               int(size), out_max.p, out_min.p)
    return out_max, out_min


def zmax_map(ctx, cube, keep=None):
    """Per-spaxel maximum over z of a float32 device cube -> host float64 (Ny, Nx);
    ``keep`` (uint8 DeviceArray [Ny*Nx], 0 = excluded) zeroes spaxels first."""
    Nz, Ny, Nx = cube.shape
    m = ctx.empty((Ny, Nx), np.float32)
    _capi.call("origin_zmax_map", ctx.handle, cube.p, _p(keep), Nz, Ny * Nx, m.p)
    return m.to_host().astype(np.float64)


def where_above(ctx, cube, threshold, aux=None, cap=1 << 20):
    """``z, y, x = np.where(cube > threshold)`` on a float32 device cube, in NumPy's order, with
    the values there (and those of the uint8 device cube ``aux``): Detection.run's thresholding
    (steps.py:956-974).  Only the detections cross PCIe.  Returns a dict of host arrays
    ``z, y, x`` (int64), ``value`` (float64) and, with ``aux``, ``aux`` (uint8)."""
    Nz, Ny, Nx = cube.shape
    if cube.dtype != np.float32:
        raise TypeError("where_above needs a float32 device cube")
    if aux is not None and (aux.dtype != np.uint8 or aux.shape != cube.shape):
        raise ValueError("aux must be a uint8 device cube of the same shape")
    count = C.c_long(0)
    cap = max(int(cap), 1)
    while True:
        idx = ctx.empty((3, cap), np.int32)
        val = ctx.empty((cap,), np.float32)
        ax = ctx.empty((cap,), np.uint8) if aux is not None else None
        _capi.call("origin_where_above", ctx.handle, cube.p, _p(aux), Nz, Ny, Nx,
                   float(threshold), cap, idx.view(0, (cap,)).p, idx.view(cap, (cap,)).p,
                   idx.view(2 * cap, (cap,)).p, val.p, _p(ax), C.byref(count))
        n = count.value
        if n <= cap:
            break
        cap = n   # more detections than expected: once more with room for all of them
    def head(a, off, dtype):   # the first n entries only
        if n == 0:
            return np.empty(0, dtype=dtype)
        return a.view(off, (n,)).to_host().astype(dtype)

    out = dict(z=head(idx, 0, np.int64), y=head(idx, cap, np.int64),
               x=head(idx, 2 * cap, np.int64), value=head(val, 0, np.float64))
    if aux is not None:
        out["aux"] = head(ax, 0, np.uint8)
    return out


def count_above(ctx, cube, thresholds, keep=None):
    """counts[t] = #{voxels of cube (x keep) with value > thresholds[t]} (int64, host)."""
    Nz, Ny, Nx = cube.shape
    thr = np.ascontiguousarray(thresholds, dtype=np.float64)
    out = np.zeros(thr.size, dtype=np.int64)
    _capi.call("origin_count_above", ctx.handle, cube.p, _p(keep), Nz, Ny * Nx, thr.size,
               thr.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


# ------------------------------------------------------------------------- cube statistics
MOMENTS_LANES = 256   # lanes per block and voxels per load of origin_cube_moments (csrc/stats.hip)
MOMENTS_VEC = 4


def cube_moments_sweep(n_voxels):
    """Voxels one sweep of ``origin_cube_moments``'s grid covers for a cube of ``n_voxels``."""
    return (_capi.load().origin_cube_moments_blocks(int(n_voxels)) * MOMENTS_LANES * MOMENTS_VEC)


def cube_moments(ctx, cube, shift=0.0, keep=None):
    """``(n, sum(x - shift), sum((x - shift)**2))`` as host floats over the voxels of a float32
    device cube whose spaxel is kept (``keep``: uint8 DeviceArray [Ny*Nx], 0 = excluded, or
    None): float64 arithmetic in a fixed order, one streaming read, three scalars out."""
    if cube.dtype != np.float32:
        raise TypeError("cube_moments needs a float32 device cube")
    Nz = cube.shape[0]
    S = cube.size // Nz
    if keep is not None and (keep.dtype != np.uint8 or keep.size != S):
        raise ValueError("keep must be a uint8 device array with one entry per spaxel")
    out = np.zeros(3, dtype=np.float64)
    _capi.call("origin_cube_moments", ctx.handle, cube.p, _p(keep), Nz, S, float(shift),
               out.ctypes.data_as(C.c_void_p))
    return float(out[0]), float(out[1]), float(out[2])


def std_from_moments(n, m2):
    """sqrt(M2 / n) (ddof 0); NaN for n == 0, as ``np.std`` of an empty array."""
    return float(np.sqrt(m2 / n)) if n > 0 else float("nan")


def two_pass_std(moments):
    """``np.std`` in NumPy's own two-pass form (lib_origin.py:2127-2129) over ``moments(shift)
    -> (n, s1, s2)``: the first pass gives the mean, the second the sum of squared deviations
    from it.  Not ``sum x^2 - (sum x)^2 / n``: that loses the digits a cube with a mean far from
    0 needs."""
    n, s1, _ = moments(0.0)
    if n == 0:
        return float("nan")
    return std_from_moments(n, moments(s1 / n)[2])


def cube_std(ctx, cube, keep=None):
    """``np.std(cube)`` of a float32 device cube (over the kept spaxels): ``two_pass_std``."""
    return two_pass_std(lambda shift: cube_moments(ctx, cube, shift, keep))


# ------------------------------------------------------------------------- line estimation
def _lines_tables(raw, psf, weights):
    """(nfields, P, psf float64 [nf][Nz][P][P], weights float64 [nf][Ny][Nx] or None)."""
    Nz, Ny, Nx = raw.shape
    if weights is None:
        psf = np.asarray(psf, dtype=np.float64)[None]
        w = None
    else:
        psf = np.stack([np.asarray(p, dtype=np.float64) for p in psf])
        w = np.ascontiguousarray(np.stack([np.asarray(x, dtype=np.float64) for x in weights]))
        if w.shape != (psf.shape[0], Ny, Nx):
            raise ValueError("need one (Ny, Nx) weight map per PSF")
    psf = np.ascontiguousarray(psf)
    if psf.ndim != 4 or psf.shape[1] != Nz or psf.shape[2] != psf.shape[3]:
        raise ValueError(f"PSF must be (Nz, P, P) per field, got {psf.shape[1:]}")
    return psf.shape[0], psf.shape[2], psf, w


def _hp(a):
    return NULL if a is None else a.ctypes.data_as(C.c_void_p)


def lines_problem_counts(y0, x0, size_grid, Ny, Nx):
    """Grid offsets inside the field per detection (lib_origin.py:1703-1706)."""
    g = int(size_grid)
    y0, x0 = np.asarray(y0, np.int64), np.asarray(x0, np.int64)
    ny = np.minimum(y0 + g, Ny - 1) - np.maximum(y0 - g, 0) + 1
    nx = np.minimum(x0 + g, Nx - 1) - np.maximum(x0 - g, 0) + 1
    return ny * nx


def _lines_outputs(ndet, Nz):
    return dict(line=np.zeros((ndet, Nz)), var=np.zeros((ndet, Nz)), flux5=np.zeros(ndet),
                mse5=np.zeros(ndet), yxz=np.zeros((ndet, 3), np.int32),
                fallback=np.zeros(ndet, np.int32))


def _det_rows(z0, y0, x0):
    return np.ascontiguousarray(np.stack([np.asarray(z0), np.asarray(y0), np.asarray(x0)], axis=1),
                                dtype=np.int32)


def lines_estimate(ctx, raw, var, psf, weights, z0, y0, x0, size_grid=0, criteria=0, order_dct=30,
                   horiz_psf=1, horiz=5, max_problems=0):
    """``origin_lines_estimate`` on float32 device cubes: the line estimation of every detection
    (reference lib_origin.py:1805-1938).  Returns host arrays: ``line`` / ``var`` float64
    (ndet, Nz), ``flux5``, ``mse5``, ``yxz`` int32 (ndet, 3), ``fallback`` (ndet) and
    ``nbatch``.  ``criteria``: 0 flux, 1 mse; ``order_dct`` None = PCA LS only."""
    Nz, Ny, Nx = raw.shape
    if raw.dtype != np.float32 or var.dtype != np.float32 or var.shape != raw.shape:
        raise TypeError("lines_estimate needs float32 device cubes of one shape")
    nf, P, hpsf, hw = _lines_tables(raw, psf, weights)
    det = _det_rows(z0, y0, x0)
    out = _lines_outputs(len(det), Nz)
    nbatch = C.c_int(0)
    if len(det):
        _capi.call("origin_lines_estimate", ctx.handle, raw.p, var.p, Nz, Ny, Nx, nf, P, _hp(hpsf),
                   _hp(hw), len(det), _hp(det), int(size_grid), int(criteria),
                   -1 if order_dct is None else int(order_dct), int(horiz_psf), int(horiz),
                   int(max_problems), _hp(out["line"]), _hp(out["var"]), _hp(out["flux5"]),
                   _hp(out["mse5"]), _hp(out["yxz"]), _hp(out["fallback"]), C.byref(nbatch))
    out["nbatch"] = nbatch.value
    return out


def lines_gather(ctx, raw, var, psf, weights, centres):
    """``origin_lines_gather`` (unit-test entry point): the standardised, centred work matrices
    of the windows centred at ``centres`` ((y, x) rows) -> (A (n, Nz, ld), means (n, Nz),
    flags (n)) as host arrays."""
    Nz, Ny, Nx = raw.shape
    nf, P, hpsf, hw = _lines_tables(raw, psf, weights)
    cen = np.ascontiguousarray(centres, dtype=np.int32).reshape(-1, 2)
    n, ld = len(cen), (P * P + 15) // 16 * 16
    A = ctx.empty((n, Nz, ld), np.float64)
    mean = ctx.empty((n, Nz), np.float64)
    flag = ctx.empty((n,), np.int32)
    _capi.call("origin_lines_gather", ctx.handle, raw.p, var.p, Nz, Ny, Nx, nf, P, _hp(hpsf),
               _hp(hw), n, _hp(cen), A.p, mean.p, flag.p)
    return A.to_host(), mean.to_host(), flag.to_host()


def lines_select(ctx, raw, psf, weights, z0, y0, x0, deconv, varest, flags, size_grid=0,
                 criteria=0, horiz_psf=1, horiz=5):
    """``origin_lines_select`` (unit-test entry point): the grid analysis on given per-problem
    deconvolutions (rows: per detection its grid offsets inside the field, dy major)."""
    Nz, Ny, Nx = raw.shape
    nf, P, hpsf, hw = _lines_tables(raw, psf, weights)
    det = _det_rows(z0, y0, x0)
    nprob = int(lines_problem_counts(y0, x0, size_grid, Ny, Nx).sum())
    dec = np.ascontiguousarray(deconv, dtype=np.float64)
    ve = np.ascontiguousarray(varest, dtype=np.float64)
    fl = np.ascontiguousarray(flags, dtype=np.int32)
    if dec.shape != (nprob, Nz) or ve.shape != (nprob, Nz) or fl.shape != (nprob,):
        raise ValueError(f"need {nprob} problems of {Nz} channels")
    out = _lines_outputs(len(det), Nz)
    _capi.call("origin_lines_select", ctx.handle, raw.p, Nz, Ny, Nx, nf, P, _hp(hpsf), _hp(hw),
               len(det), _hp(det), int(size_grid), int(criteria), int(horiz_psf), int(horiz),
               _hp(dec), _hp(ve), _hp(fl), _hp(out["line"]), _hp(out["var"]), _hp(out["flux5"]),
               _hp(out["mse5"]), _hp(out["yxz"]), _hp(out["fallback"]))
    return out


# ------------------------------------------------------------------------- spatio-spectral merging
def merge_predicate_tables(tol_spat):
    """The two float predicates of ``itersrc`` (reference lib_origin.py:1300, :1306) over integer
    offsets, evaluated by NumPy exactly as the reference writes them: ``near[a, b] =
    np.hypot(a, b) < tol_spat`` and ``far[a, b] = np.hypot(a, b) > tol_spat * np.sqrt(2)`` for
    ``0 <= a, b <= ceil(tol_spat * sqrt(2)) + 1``.  Beyond the tables nothing is near and
    everything is far.  (``np.hypot(3, 3)`` and ``3 * np.sqrt(2)`` differ in the last bit: the
    device never evaluates either.)"""
    R = int(np.ceil(tol_spat * np.sqrt(2))) + 2
    a = np.arange(R)
    d = np.hypot(a[:, None], a[None, :])
    near = (d < tol_spat).astype(np.uint8)
    far = (d > tol_spat * np.sqrt(2)).astype(np.uint8)
    return np.ascontiguousarray(near), np.ascontiguousarray(far)


def merge_detections(ctx, x0, y0, z0, area, shape, tol_spat, tol_spec):
    """``origin_merge_detections``: ``spatiospectral_merging`` (reference lib_origin.py:1319-1387)
    for detections given as host columns in table order; ``shape`` = (Nz, Ny, Nx) of the cube.
    Returns int32 host arrays in input row order: ``comp`` (lowest row of the row's connected
    component of the near graph), ``area`` (the group's largest label), ``imatch2`` and
    ``imatch`` (0-based group id before / after the spectral stage)."""
    x, y, z, a = (np.ascontiguousarray(v, dtype=np.int32) for v in (x0, y0, z0, area))
    n = len(x)
    if not (len(y) == len(z) == len(a) == n):
        raise ValueError("x0, y0, z0 and area must have one length")
    if not tol_spat > 0:
        raise ValueError("tol_spat must be positive")
    Nz, Ny, Nx = (int(v) for v in shape)
    near, far = merge_predicate_tables(tol_spat)
    out = {k: np.zeros(n, np.int32) for k in ("comp", "area", "imatch2", "imatch")}
    _capi.call("origin_merge_detections", ctx.handle, n, _hp(x), _hp(y), _hp(z), _hp(a), Ny, Nx,
               Nz, near.shape[0], _hp(near), _hp(far), int(np.ceil(tol_spec)) - 1, _hp(out["comp"]),
               _hp(out["area"]), _hp(out["imatch2"]), _hp(out["imatch"]))
    return out


# ------------------------------------------------------------------------- segmentation maps
def label_tile():
    """(TW, TH): the tile one workgroup of ``origin_segmap_label`` builds the components of."""
    tw, th = C.c_int(), C.c_int()
    _capi.call("origin_label_tile", C.byref(tw), C.byref(th))
    return tw.value, th.value


def label_scan_span():
    """Pixels whose root flags the labeller's one scan workgroup counts in a single pass."""
    return _capi.load().origin_label_scan_span()


def segmap_mask(ctx, data, gamma, f=-1, stage=4, out=None):
    """``origin_segmap_mask``: the mask of ``compute_segmap_gauss`` (reference lib_origin.py:268-278)
    of a float64 device map (Ny, Nx) -> uint8 DeviceArray.  ``f``: ``int(fwhm_fsf) // 2``, negative
    = no disc; ``stage`` < 4 stops after the threshold (1), the erosion (2), the dilation (3)."""
    if data.dtype != np.float64 or len(data.shape) != 2:
        raise TypeError("segmap_mask needs a float64 device image")
    Ny, Nx = data.shape
    out = ctx.empty((Ny, Nx), np.uint8) if out is None else out
    _capi.call("origin_segmap_mask", ctx.handle, data.p, Ny, Nx, float(gamma), int(f), int(stage),
               out.p)
    return out


def segmap_union(ctx, a, b, out=None):
    """``(a > 0) | (b > 0)`` of two int32 device label maps -> uint8 DeviceArray."""
    if a.dtype != np.int32 or b.dtype != np.int32 or a.shape != b.shape:
        raise TypeError("segmap_union needs two int32 device maps of one shape")
    out = ctx.empty(a.shape, np.uint8) if out is None else out
    _capi.call("origin_segmap_union", ctx.handle, a.p, b.p, a.size, out.p)
    return out


def segmap_label(ctx, mask, out=None):
    """``scipy.ndimage.label(mask)`` (4-connected) of a uint8 device mask (Ny, Nx) ->
    (int32 DeviceArray of labels, n)."""
    if mask.dtype != np.uint8 or len(mask.shape) != 2:
        raise TypeError("segmap_label needs a uint8 device image")
    Ny, Nx = mask.shape
    out = ctx.empty((Ny, Nx), np.int32) if out is None else out
    n = C.c_int(0)
    _capi.call("origin_segmap_label", ctx.handle, mask.p, Ny, Nx, out.p, C.byref(n))
    return out, n.value


# ------------------------------------------------------------------------- matching of point lists
def ball_match(ctx, a, b, r, a_val=None, want=None):
    """``origin_ball_match``: points of ``a`` / ``b`` (three host columns x, y, z each) with a point
    of the other list within ``r``, under the float64 predicate ``(dx*dx + dy*dy) + dz*dz <= r*r``
    as NumPy rounds it (include/origin_hip.h).  Returns a dict with the outputs named in ``want``:
    ``a_hit`` / ``b_hit`` (uint8, 0 / 1) and ``b_max`` (float32: the largest ``a_val`` within ``r``
    of each point of ``b``, ``-inf`` where there is none).  ``want=None``: all that can be had,
    ``b_max`` only with ``a_val``; the library refuses ``b_max`` asked for without it."""
    A = [np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in a]
    B = [np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in b]
    if len(A) != 3 or len(B) != 3:
        raise ValueError("a and b must have three columns (x, y, z) each")
    n, m = A[0].size, B[0].size
    if any(c.size != n for c in A) or any(c.size != m for c in B):
        raise ValueError("the three columns of a list must have one length")
    val = None
    if a_val is not None:
        val = np.ascontiguousarray(a_val, dtype=np.float32).reshape(-1)
        if val.size != n:
            raise ValueError("a_val must have one entry per point of a")
    if want is None:
        want = ("a_hit", "b_hit") + (("b_max",) if val is not None else ())
    out = {}
    if "a_hit" in want:
        out["a_hit"] = np.zeros(n, np.uint8)
    if "b_hit" in want:
        out["b_hit"] = np.zeros(m, np.uint8)
    if "b_max" in want:
        out["b_max"] = np.zeros(m, np.float32)
    _capi.call("origin_ball_match", ctx.handle, n, _hp(A[0]), _hp(A[1]), _hp(A[2]), _hp(val), m,
               _hp(B[0]), _hp(B[1]), _hp(B[2]), float(r), _hp(out.get("a_hit")),
               _hp(out.get("b_hit")), _hp(out.get("b_max")))
    return out
