"""The input conditions of tests/test_hip_reduction_shapes.py that can be checked without a GPU:
the restated launch geometry (tests/_reduction_geometry.py) puts the named shapes where the GPU
tests aim them.  No library load."""
import numpy as np
import pytest

import _reduction_geometry as rg
from oracle import cpu_ref


@pytest.mark.parametrize("num_cu", [64, 256, 304])
def test_overflow_case_has_one_segment_above_capacity(num_cu):
    """(64, 16, 64) with a 32 x 4 x 64 plateau: one spaxel block, two z chunks of 32 channels,
    capacity 1984; exactly one of the 16 segments is above it, one wave per chunk is empty, and
    the footprints partition the cube (the counts add up to the non-zero voxels)."""
    a, b = rg.overflow_case()
    g = rg.sparse_plan(num_cu, a.shape)
    assert g == dict(bx=1, nzc=2, zp=32, nseg=8, seg_cap=1984)
    rmax, rmin = cpu_ref.compute_local_max(a.astype(float), b.astype(float),
                                           np.zeros(a.shape, bool), 3)
    cmax, cmin = rg.sparse_segment_counts(num_cu, rmax), rg.sparse_segment_counts(num_cu, rmin)
    assert cmax.size == cmin.size == 8
    assert cmax.sum() == np.count_nonzero(rmax) and cmin.sum() == np.count_nonzero(rmin)
    both = np.concatenate([cmax, cmin])
    assert np.count_nonzero(both > g["seg_cap"]) == 1 and cmax[0] > g["seg_cap"]
    assert cmax[3] == cmax[7] == cmin[3] == cmin[7] == 0        # the fourth wave has no lane
    assert np.all(np.delete(both, [3, 7, 11, 15]) > 0)          # the others hold entries


def test_segments_partition_ragged_shapes():
    """Every voxel belongs to one segment below nseg, and a wave's footprint is 62 lane positions
    of 4 rows x 2 columns: at most zp * 62 * 8 voxels."""
    for shape in [(1, 8, 8), (2, 5, 12), (5, 4, 4), (33, 9, 64), (70, 31, 100)]:
        g = rg.sparse_plan(256, shape)
        seg = rg.sparse_segment_of(256, shape)
        n = np.bincount(seg.reshape(-1), minlength=g["nseg"])
        assert n.size == g["nseg"] and n.sum() == np.prod(shape)
        assert n.max() <= g["zp"] * 62 * 8


def test_zmax_chunkings_at_256_cus():
    """The chunkings section A of the GPU tests names, on a 256-CU device."""
    assert rg.zmax_chunks(256, 1, 1) == (1, 1, 1)
    assert rg.zmax_chunks(256, 5, 7) == (5, 1, 1)
    assert rg.zmax_chunks(256, 63, 15) == (63, 1, 1)
    assert rg.zmax_chunks(256, 65, 16 * 17) == (33, 2, 1)
    assert rg.zmax_chunks(256, 131, 257) == (44, 3, 2)
    assert rg.zmax_chunks(256, 200, 9 * 29) == (50, 4, 4)
    n = 725
    assert n * n >= 256 * 2048 > (n - 1) * (n - 1)
    assert rg.zmax_chunks(256, 3, n * n) == (1, 3, 3)


def test_count_and_column_geometry_at_256_cus():
    total = 7 * 613 * 613
    sweep = rg.count_sweep(256)
    assert total // sweep >= 2 and total % sweep != 0 and (613 * 613) % 2 == 1
    assert rg.sparse_count_blocks(256, 256 * 16 + 5) == 256 * 16
    assert rg.column_chunks(256, 37, 257) == (37, 1, 1)
    assert rg.column_chunks(256, 256 * 8 + 1, 257) == (1025, 2, 1)
    assert rg.column_chunks(256, 3, (256 * 16 + 1) * 256) == (1, 3, 3)
