"""Cube forms built by hand, for the tests of their consumers (test_sparse.py, test_cube_stats.py,
test_cube_forms.py): a ``SparseCube`` from a host cube and a ``TiledCube`` over two contexts."""
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
