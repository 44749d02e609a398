"""Test-side restatement of the launch geometry of the fp32 GLR kernels (csrc/glr_fp32.hip:
spectral_zchunks / glr_fp32_spectral, launch_border_pass, glr_fp32_spatial) and the dictionary
builder of tests/test_hip_glr_fp32.py.  The geometry is restated to AIM inputs at a launch shape
(more than one z chunk, a short last chunk, a z-march of more than one plane); the tests assert
it as a condition on their inputs, for the device at hand."""
import numpy as np

from _gram_geometry import num_cu_of  # noqa: F401  (re-exported: one parser of the device name)

SPEC_ZC = 4          # channels per step of spectral3_kernel
LWT = (8, 16, 24, 29, 32)   # window half widths of spectral3_kernel (plan: build_half_taps_and_rows)


def _cdiv(a, b):
    return -(-a // b)


def lwt_of(lwmax):
    """Template half width of the packed form's tap rows; 0: no rows (half widths above 32)."""
    for t in LWT:
        if lwmax <= t:
            return t
    return 0


def lwmax_template(lwmax):
    """LWMAX of spectral_kernel<LWMAX, .> (forms fp32 and the border pass); 0: generic loops."""
    return 8 if lwmax <= 8 else 16 if lwmax <= 16 else 32 if lwmax <= 32 else 0


def spectral_chunks(num_cu, S, Nz, lwmax):
    """(nzc, zchunk, last): z chunks of the spectral stage (grid.y), channels per chunk and the
    channels of the last one, as glr_fp32_spectral picks them."""
    lw = max(lwmax, 1)
    blocks = _cdiv(S, 256)
    want = _cdiv(num_cu * 8, blocks)
    want = max(1, min(want, max(1, Nz // (8 * lw + 8))))
    nzc = min(64, want)
    zchunk = _cdiv(_cdiv(Nz, nzc), SPEC_ZC) * SPEC_ZC
    nzc = _cdiv(Nz, zchunk)
    return nzc, zchunk, Nz - (nzc - 1) * zchunk


def nborder_of(Ny, Nx, P):
    """Spaxels within P // 2 of the field's border (plan: build_border_tables); Ny, Nx >= P."""
    c = P // 2
    return Ny * Nx - (Ny - 2 * c) * (Nx - 2 * c)


def border_slices(num_cu, nborder, Nz, lwmax):
    """(slices, zcb): z slices of launch_border_pass (grid.y) and channels per slice."""
    bb = _cdiv(nborder, 256)
    nzb = _cdiv(num_cu * 12, bb)
    nzb = max(1, min(nzb, Nz // (4 * max(lwmax, 1) + 4)))
    zcb = _cdiv(Nz, nzb)
    return _cdiv(Nz, zcb), zcb


def spatial_march(num_cu, Nz, Ny, Nx):
    """(zper, blocks, last): planes a block of spatial4x4_kernel marches, z blocks (grid.z) and the
    planes of the last one, as glr_fp32_spatial picks them."""
    tiles = _cdiv(Nx, 64) * _cdiv(Ny, 64)
    nzb = max(1, min(_cdiv(num_cu * 16, tiles), Nz))
    zper = _cdiv(Nz, nzb)
    blocks = _cdiv(Nz, zper)
    return zper, blocks, Nz - (blocks - 1) * zper


def spatial_nz(num_cu, Ny, Nx):
    """The smallest odd Nz >= 7 more than the z blocks the chip asks for: zper = 2 and a last
    block of one plane (256 CUs, 70 x 70: 1031)."""
    tiles = _cdiv(Nx, 64) * _cdiv(Ny, 64)
    nz = _cdiv(num_cu * 16, tiles) + 7
    return nz | 1


def build_dictionary(lws, seed):
    """Profiles of length exactly 2 * lw + 1 for the half widths ``lws``: a broad envelope whose
    peak sits off the centre (at 1.3 lw) times 0.6 + 0.8 * random, so that every tap -- the
    outermost ones included -- is at least 0.1 of the profile's largest and no profile is
    symmetric.  Meant for pcut=None, pmeansub=False: the device gets them untrimmed."""
    rng = np.random.default_rng(seed)
    out = []
    for lw in lws:
        L = 2 * lw + 1
        j = np.arange(L, dtype=np.float64)
        env = np.exp(-0.5 * ((j - 1.3 * lw) / (1.2 * lw + 1.0)) ** 2)
        out.append(env * (0.6 + 0.8 * rng.random(L)))
    return out


def tap_ratio(profiles):
    """Smallest tap over largest tap, the least over the profiles."""
    return min(float(p.min() / p.max()) for p in profiles)
