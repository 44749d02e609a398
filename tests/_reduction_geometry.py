"""Test-side restatement of the launch geometry of the small kernels between the GLR and the
catalogue: origin_zmax_map / origin_count_above (csrc/purity.hip), the sparse local-maximum pass
and its consumers (csrc/localmax.hip: lm_geometry, origin_local_max_sparse_plan,
origin_sparse_count_above) and the column moves (csrc/columns.hip).  The geometry is restated to
AIM inputs at a launch shape (more than one z chunk, a short last chunk, a sweep that ends in mid
plane, one segment above its capacity); tests/test_hip_reduction_shapes.py asserts it as a
condition on its inputs, for the device at hand."""
import numpy as np

from _gram_geometry import num_cu_of  # noqa: F401  (re-exported: one parser of the device name)

LMS_R, LMS_NC = 4, 2     # rows and samples per lane of local_max3s_kernel
LANES = 62               # producing lanes of a wave (lanes 0 and 63 only hand samples on)


def _cdiv(a, b):
    return -(-a // b)


def zmax_chunks(num_cu, Nz, S):
    """(nzc, zchunk, last): z chunks of zmax_map_kernel (grid.y, the rows of the partial-maxima
    buffer zmax_final_kernel reduces), channels per chunk and the channels of the last one."""
    n0 = max(1, min(_cdiv(num_cu * 8 * 256, S), min(64, Nz)))
    zchunk = _cdiv(Nz, n0)
    nzc = _cdiv(Nz, zchunk)
    return nzc, zchunk, Nz - (nzc - 1) * zchunk


def count_sweep(num_cu):
    """Voxels one trip of count_above_kernel's grid-stride loop covers."""
    return num_cu * 16 * 256


def sparse_plan(num_cu, shape):
    """dict(bx, nzc, zp, nseg, seg_cap) of the sparse pass for a cube shape with Nx % 4 == 0."""
    Nz, Ny, Nx = shape
    bx = _cdiv(_cdiv(Ny, LMS_R) * (Nx // LMS_NC), 4 * LANES)
    nzc = max(1, min(_cdiv(num_cu * 16, bx), _cdiv(Nz, 32)))
    zp = _cdiv(Nz, nzc)
    nzc = _cdiv(Nz, zp)
    per_wave = zp * LANES * LMS_NC * LMS_R
    seg_cap = max(256, _cdiv(per_wave // 8, 64) * 64)
    return dict(bx=bx, nzc=nzc, zp=zp, nseg=4 * bx * nzc, seg_cap=seg_cap)


def sparse_segment_of(num_cu, shape):
    """int64 (Nz, Ny, Nx): the segment every voxel's entry goes to.  Lanes walk the flattened
    index t = grp * (Nx // 2) + x2; wave t // 62 owns rows 4 grp .. 4 grp + 3 and columns 2 x2,
    2 x2 + 1; segment = (z chunk * bx + block) * 4 + wave in block."""
    Nz, Ny, Nx = shape
    g = sparse_plan(num_cu, shape)
    z, y, x = np.indices(shape)
    wave = ((y // LMS_R) * (Nx // LMS_NC) + x // LMS_NC) // LANES      # = block * 4 + wave in block
    return (z // g["zp"]) * (4 * g["bx"]) + wave


def sparse_segment_counts(num_cu, cube):
    """Non-zero voxels of a host cube per segment of the sparse pass (int64 [nseg])."""
    seg = sparse_segment_of(num_cu, cube.shape)
    return np.bincount(seg[cube != 0], minlength=sparse_plan(num_cu, cube.shape)["nseg"])


def sparse_count_blocks(num_cu, nseg):
    """Blocks of sparse_count_above_kernel; each walks the segments blockIdx.x, + blocks, ..."""
    return min(nseg, num_cu * 16)


def column_chunks(num_cu, Nz, n):
    """(nzb, zper, last): z chunks of columns_kernel (grid.y), channels per chunk and of the last."""
    bx = _cdiv(n, 256)
    nzb = max(1, min(_cdiv(num_cu * 16, bx), min(Nz, 65535)))
    zper = _cdiv(Nz, nzb)
    nzb = _cdiv(Nz, zper)
    return nzb, zper, Nz - (nzb - 1) * zper


def overflow_case():
    """Section D's input: one segment of the sparse pass above its capacity between healthy
    neighbours ((64, 16, 64), a 32 x 4 x 64 plateau of 2.0 in correl), no mask."""
    rng = np.random.default_rng(5)
    shape = (64, 16, 64)
    a = (0.3 * rng.standard_normal(shape)).astype(np.float32)
    b = (0.3 * rng.standard_normal(shape)).astype(np.float32)
    a[:32, :4, :] = 2.0
    return a, b
