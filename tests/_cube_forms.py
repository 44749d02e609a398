"""Cube forms built by hand, for the tests of their consumers (test_sparse.py, test_cube_stats.py,
test_cube_forms.py, test_hip_reduction_shapes.py): a ``SparseCube`` from a host cube (``as_sparse``:
full segments; ``as_lists``: any counts, stale slots poisoned) and a ``TiledCube`` over two contexts."""
import numpy as np

# Two windows of a field at least 10 x 12 that overlap in x; ``owner`` cuts it along an irregular
# border inside the overlap.
WINDOWS = [(0, 10, 0, 9), (0, 10, 5, None)]


def as_sparse(ctx, dense):
    """A SparseCube holding exactly the non-zero voxels of a host cube (one segment per 64
    entries): the consumers' side of the format, independent of the pass that fills it."""
    from origin_amd import sparse
    idx = np.flatnonzero(dense.reshape(-1)).astype(np.int64)
    val = dense.reshape(-1)[idx]
    cap = 64
    nseg = max(1, -(-len(idx) // cap))

    class B:
        pass
    b = B()
    b.ctx, b.shape, b.nseg, b.seg_cap = ctx, dense.shape, nseg, cap
    pi = np.zeros(nseg * cap, np.int64)
    pv = np.zeros(nseg * cap, np.float32)
    pi[:len(idx)], pv[:len(idx)] = idx, val
    cnt = np.zeros(2 * nseg, np.int32)
    full, rest = divmod(len(idx), cap)
    cnt[:full] = cap
    if rest:
        cnt[full] = rest
    b.idx, b.val = [ctx.to_device(pi), None], [ctx.to_device(pv), None]
    b.counts = ctx.to_device(cnt)
    return sparse.SparseCube(b, 0)


POISON = np.float32(1e30)


def as_lists(ctx, dense, seg_cap, counts, poison=True, seed=0):
    """A SparseCube holding exactly the non-zero voxels of a host cube in ``len(counts)`` segments
    of ``seg_cap`` slots, ``counts[s]`` entries in segment s (they add up to the non-zero voxels;
    0 and ``seg_cap`` are allowed).  The entries are dealt to the segments in shuffled order.
    ``poison``: every slot behind a segment's count holds a random index INSIDE the cube and the
    value 1e30, so a consumer that read past ``min(counts, seg_cap)`` would show it in its result
    without touching memory outside the arrays."""
    from origin_amd import sparse
    counts = np.asarray(counts, np.int32)
    idx = np.flatnonzero(dense.reshape(-1)).astype(np.int64)
    assert counts.ndim == 1 and counts.size >= 1 and counts.sum() == idx.size
    assert counts.min() >= 0 and counts.max() <= seg_cap
    rng = np.random.default_rng(seed)
    idx = idx[rng.permutation(idx.size)]
    nseg = counts.size
    pi = np.zeros(nseg * seg_cap, np.int64)
    pv = np.zeros(nseg * seg_cap, np.float32)
    if poison:
        pi[:] = rng.integers(0, dense.size, pi.size)
        pv[:] = POISON
    first = np.cumsum(counts) - counts                       # rank of a segment's first entry
    seg = np.repeat(np.arange(nseg), counts)
    slot = seg * seg_cap + (np.arange(idx.size) - first[seg])
    pi[slot], pv[slot] = idx, dense.reshape(-1)[idx]

    class B:
        pass
    b = B()
    b.ctx, b.shape, b.nseg, b.seg_cap = ctx, dense.shape, nseg, int(seg_cap)
    b.idx, b.val = [ctx.to_device(pi), None], [ctx.to_device(pv), None]
    # (the second half belongs to the pass's other cube: full segments nobody may read as cube 0's)
    b.counts = ctx.to_device(np.concatenate([counts, np.full(nseg, seg_cap, np.int32)]))
    return sparse.SparseCube(b, 0)


def tiled(group, field, outside=np.nan, part=lambda ctx, arr: ctx.to_device(arr)):
    """``field`` (Nz, 10, >= 10) as a TiledCube over the two contexts of ``group``: windows that
    overlap, an irregular ownership border, arrays larger than their windows with ``outside``
    around them.  ``part(ctx, host array)`` makes a part: a DeviceArray, or lists (``as_sparse``)."""
    from origin_amd.session import TiledCube
    shape = field.shape
    yy, xx = np.indices(shape[1:])
    owner = (xx + 2 * (yy % 2) >= 7).astype(int)
    parts = []
    for r, (y0, y1, x0, x1) in enumerate(WINDOWS):
        x1 = shape[2] if x1 is None else x1
        by, bx = 1 + r, 2 - r
        arr = np.full((shape[0], (y1 - y0) + 3, (x1 - x0) + 4), outside, field.dtype)
        arr[:, by:by + y1 - y0, bx:bx + x1 - x0] = field[:, y0:y1, x0:x1]
        owned = owner[y0:y1, x0:x1] == r
        assert not owned.all() and owned.any()
        parts.append((part(group.ctxs[r], arr), (by, bx), (y0, y1, x0, x1), owned))
    return TiledCube(group, shape, field.dtype, parts)
