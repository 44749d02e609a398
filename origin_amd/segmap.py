"""Segmentation maps of steps 1 and 6 on the device: the reference's
``compute_segmap_gauss`` (lib_origin.py:243-280) behind its threshold fit, and the label of the
union of two label maps (steps.py:487, :869).  The threshold fit is host code by design
(``thresholds.compute_thresh_gaussfit``, ~1e5 numbers); mask, morphology, disc and labels are
kernels of ``csrc/segmap.hip``, bit-identical to SciPy's.  Label maps come back as host int32
arrays: what ``store_image`` and ``areas.create_areamap`` take."""
import numpy as np

from . import kernels
from .thresholds import compute_thresh_gaussfit


def disc_radius(fwhm_fsf):
    """``f`` of the disc (lib_origin.py:273-276): ``int(fwhm_fsf) // 2``, -1 where the reference
    skips the disc (``fwhm_fsf <= 0``)."""
    return int(fwhm_fsf) // 2 if fwhm_fsf > 0 else -1


def mask_stages(ctx, data, gamma, fwhm_fsf=0):
    """The masks after the threshold, the erosion, the dilation and the disc (the last one is what
    gets labelled) as host bool arrays: the unit tests' view of ``origin_segmap_mask``."""
    d = ctx.to_device(np.ascontiguousarray(data, dtype=np.float64))
    f = disc_radius(fwhm_fsf)
    return [kernels.segmap_mask(ctx, d, gamma, f, stage).to_host().astype(bool)
            for stage in (1, 2, 3, 4)]


def labels_at(ctx, data, gamma, fwhm_fsf=0):
    """``compute_segmap_gauss`` behind the fit: (labels int32 (Ny, Nx) on the host, n)."""
    d = ctx.to_device(np.ascontiguousarray(data, dtype=np.float64))
    mask = kernels.segmap_mask(ctx, d, gamma, disc_radius(fwhm_fsf))
    labels, n = kernels.segmap_label(ctx, mask)
    return labels.to_host(), n


def label_mask(ctx, mask):
    """``scipy.ndimage.label(mask)`` of a host 2-D mask: (labels int32, n)."""
    m = ctx.to_device(np.ascontiguousarray(np.asarray(mask) != 0), np.uint8)
    labels, n = kernels.segmap_label(ctx, m)
    return labels.to_host(), n


def segmap_gauss(ctx, data, pfa, fwhm_fsf=0, bins='fd'):
    """``compute_segmap_gauss(data, pfa, fwhm_fsf, bins)`` -> (gamma, labels)."""
    data = np.asarray(data)
    histO2, frecO2, gamma, mea, std = compute_thresh_gaussfit(data, pfa, bins=bins)
    return gamma, labels_at(ctx, data, gamma, fwhm_fsf)[0]


def _as_labels(a):
    a = np.asarray(a)
    if a.dtype.kind not in 'iu' or a.dtype.itemsize > 4:
        a = a > 0           # (a label map reloaded from a file may be float64)
    return np.ascontiguousarray(a, dtype=np.int32)


def merged_labels(ctx, a, b):
    """``ndi.label((a > 0) | (b > 0))[0]`` of two label maps of one shape."""
    a, b = _as_labels(a), _as_labels(b)
    if a.shape != b.shape or a.ndim != 2:
        raise ValueError("merged_labels needs two 2-D maps of one shape")
    mask = kernels.segmap_union(ctx, ctx.to_device(a), ctx.to_device(b))
    labels, n = kernels.segmap_label(ctx, mask)
    return labels.to_host()
