"""SciPy restatement of the reference's ``compute_segmap_gauss`` (lib_origin.py:243-280), stage by
stage: the host code the steps ran before the masks and labels moved to the device
(csrc/segmap.hip).  ``gamma`` is an argument so that the kernels are tested apart from the
threshold fit; tests/test_segmap_cases.py pins this file to the reference's golden labels."""
import numpy as np
from scipy import ndimage as ndi
from scipy.signal import fftconvolve


def mask_stages(data, gamma, fwhm_fsf=0):
    """[data > gamma, eroded, dilated, widened by the disc]: the last one is what is labelled."""
    m0 = np.asarray(data) > gamma
    m1 = ndi.binary_erosion(m0, border_value=1, iterations=1)
    m2 = ndi.binary_dilation(m1, iterations=1)
    m3 = m2
    if fwhm_fsf > 0:
        fwhm_pix = int(fwhm_fsf) // 2
        size = fwhm_pix * 2 + 1
        disc = np.hypot(*list(np.mgrid[:size, :size] - fwhm_pix)) < fwhm_pix
        m3 = fftconvolve(m2, disc, mode='same') > 1e-9
    return [m0, m1, m2, m3]


def labels_at(data, gamma, fwhm_fsf=0):
    """(labels, n) of the reference behind its fit."""
    return ndi.label(mask_stages(data, gamma, fwhm_fsf)[3])


def merged_labels(a, b):
    return ndi.label((np.asarray(a) > 0) | (np.asarray(b) > 0))[0]


def compute_segmap_gauss(data, pfa, fwhm_fsf=0, bins='fd'):
    """The whole function, with the product's host threshold fit: (gamma, labels)."""
    from origin_amd.thresholds import compute_thresh_gaussfit
    histO2, frecO2, gamma, mea, std = compute_thresh_gaussfit(data, pfa, bins=bins)
    return gamma, labels_at(data, gamma, fwhm_fsf)[0]
