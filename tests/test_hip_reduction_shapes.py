"""The small kernels between the GLR and the catalogue against NumPy at the shapes where their
launch geometry changes: origin_zmax_map / origin_count_above (csrc/purity.hip), the consumers of
the sparse form on hand-made lists and the sparse pass without a mask (csrc/localmax.hip), and the
column moves (csrc/columns.hip).

Every expectation is NumPy's on the host float32 cube widened to float64, or the oracle's
``compute_local_max``; never another device kernel's output.  Everything here is index work,
comparisons and copies of float32 values: ``np.array_equal`` throughout, no tolerance.  The launch
arithmetic is restated in tests/_reduction_geometry.py; every test asserts the geometry it aims at
as a condition on its input, for the device at hand."""
import numpy as np
import pytest

import _reduction_geometry as rg
from _cube_forms import as_lists
from oracle import cpu_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from origin_amd.device import default_context
    return default_context(0)


@pytest.fixture(scope="module")
def ncu(ctx):
    return rg.num_cu_of(ctx)


def keep_maps(S):
    """None, a pattern that drops a third of the spaxels, all ones, all zeros."""
    return [None, (np.arange(S) % 3 != 0).astype(np.uint8), np.ones(S, np.uint8),
            np.zeros(S, np.uint8)]


def zmax_ref(cube, keep):
    m = cube.astype(np.float64).max(axis=0)
    return m if keep is None else np.where(keep.reshape(m.shape) != 0, m, 0.0)


def kept_sorted(cube, keep):
    """The kept voxels widened to float64 and sorted; NaN voxels (above nothing) left out."""
    v = cube.astype(np.float64).reshape(cube.shape[0], -1)
    if keep is not None:
        v = v[:, keep != 0]
    return np.sort(v[~np.isnan(v)])


def count_ref(v, thr):
    """#{values of the sorted v > thr[t]}: np.searchsorted(side="right")."""
    return (v.size - np.searchsorted(v, np.asarray(thr, np.float64), side="right")).astype(np.int64)


def threshold_lists(cube, seed):
    """The list families of section B: a single value; 50 from linspace; 256; 257; 1024 shuffled
    with duplicates; one wholly above the cube's maximum.  The long ones hold float32 values of
    the cube widened (the comparison is a strict >), negative values and both infinities."""
    rng = np.random.default_rng(seed)
    fin = cube[np.isfinite(cube)].astype(np.float64)
    lo, hi = float(fin.min()), float(fin.max())
    own = np.unique(fin)

    def mixed(n):
        t = np.concatenate([rng.choice(own, n // 2), rng.uniform(lo - 1.0, hi + 1.0, n - n // 2 - 4),
                            [-np.inf, np.inf, -abs(lo) - 0.5, 0.0]])
        assert t.size == n
        return rng.permutation(t)
    t1024 = mixed(1024)
    t1024[rng.choice(1024, 200, replace=False)] = rng.choice(t1024, 200)     # duplicates
    return {"one": np.array([own[own.size // 2]]), "lin50": np.linspace(lo, hi, 50),
            "n256": mixed(256), "n257": mixed(257), "n1024": rng.permutation(t1024),
            "above": hi + np.array([2.0, 1.0, np.inf, 1e-3, 1.5])}


# ----------------------------------------------------------------------------- A. zmax_map
ZMAX_SHAPES = [(1, 1, 1), (5, 1, 7), (63, 3, 5), (65, 16, 17), (131, 1, 257), (200, 9, 29), "wide"]
# (zchunk, channels of the last chunk) each shape is aimed at
ZMAX_CHUNKS = {(1, 1, 1): (1, 1), (5, 1, 7): (1, 1), (63, 3, 5): (1, 1), (65, 16, 17): (2, 1),
               (131, 1, 257): (3, 2), (200, 9, 29): (4, 4)}


@pytest.mark.parametrize("shape", ZMAX_SHAPES, ids=str)
def test_zmax_map_at_every_chunking(ctx, ncu, shape):
    """kernels.zmax_map against np.where(keep, cube.max(0), 0): one channel per chunk, last chunks
    of one and of two channels, a spaxel count that is no multiple of 256 (one lane in the second
    block), the single-chunk path.  Most columns are negative throughout (the partial maxima and
    the final pass start from -inf, not 0); a dozen columns carry their maximum at z = 0, at
    z = Nz - 1 and at the first and last channel of an interior chunk."""
    from origin_amd import kernels
    if shape == "wide":
        n = int(np.ceil(np.sqrt(ncu * 2048)))
        shape = (3, n, n)
        assert n * n >= ncu * 2048
        want = (3, 3)
    else:
        want = ZMAX_CHUNKS[shape]
    Nz, Ny, Nx = shape
    S = Ny * Nx
    nzc, zchunk, last = rg.zmax_chunks(ncu, Nz, S)
    assert (zchunk, last) == want and nzc == -(-Nz // zchunk)
    rng = np.random.default_rng(Nz + S)
    cube = rng.normal(-3.0, 1.0, (Nz, S)).astype(np.float32)
    c = nzc // 2                                          # an interior chunk (or the only one)
    spots = [0, Nz - 1, c * zchunk, min(Nz, (c + 1) * zchunk) - 1]
    cols = np.unique(np.linspace(0, S - 1, 12).astype(int))
    for j, s in enumerate(cols):
        cube[spots[j % 4], s] = 4.0 + j
    plain = np.delete(cube.max(0), cols)                  # the columns without a planted maximum
    assert plain.size == 0 or np.mean(plain < 0) > 0.5
    cube = cube.reshape(shape)
    d = ctx.to_device(cube)
    for keep in keep_maps(S):
        got = kernels.zmax_map(ctx, d, None if keep is None else ctx.to_device(keep))
        assert got.dtype == np.float64 and got.shape == (Ny, Nx)
        assert np.array_equal(got, zmax_ref(cube, keep))


# ----------------------------------------------------------------------------- B. count_above
def count_cube(shape, kind, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(shape).astype(np.float32)
    if kind == "full":                                    # no zeros
        v[v == 0] = 0.5
        return v
    v[rng.random(shape) < 0.9] = 0.0                      # like a local-maximum cube
    if kind == "nonfinite":
        flat = v.reshape(-1)
        flat[[1, 17, 40]] = np.inf
        flat[[3, 50]] = -np.inf
        flat[[5, 6, 77]] = np.nan
    return v


@pytest.mark.parametrize("kind", ["lm", "full"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 7), (7, 613, 613)], ids=str)
def test_count_above_sweeps_and_threshold_lists(ctx, ncu, shape, kind):
    """kernels.count_above against the sorted values: a grid-stride loop of more than two sweeps
    with a ragged last one, ``i % S`` wrapping in mid sweep (S odd), threshold lists of one and of
    more than one 256-lane load, thresholds equal to cube values, with and without a keep map."""
    from origin_amd import kernels
    Nz, Ny, Nx = shape
    S, total = Ny * Nx, Nz * Ny * Nx
    if total > 1000:
        sweep = rg.count_sweep(ncu)
        assert total > 2 * sweep and total % sweep != 0 and S % 2 == 1 and sweep % S != 0
    cube = count_cube(shape, kind, 11)
    if kind == "lm" and total > 100:
        assert 0.85 < np.mean(cube == 0) < 0.95 and cube.min() < 0 < cube.max()
    d = ctx.to_device(cube)
    lists = threshold_lists(cube, 12)
    assert sorted(len(t) for t in lists.values()) == [1, 5, 50, 256, 257, 1024]
    assert lists["above"].min() > cube.max()
    for keep in keep_maps(S)[:2]:
        kd = None if keep is None else ctx.to_device(keep)
        ref = kept_sorted(cube, keep)
        for name, thr in lists.items():
            got = kernels.count_above(ctx, d, thr, kd)
            assert got.dtype == np.int64
            assert np.array_equal(got, count_ref(ref, thr)), (name, keep is None)
        assert not kernels.count_above(ctx, d, lists["above"], kd).any()


def test_count_above_nonfinite_voxels_and_bad_lists(ctx):
    """+inf, -inf and NaN voxels: NaN is above no threshold, -inf not above -inf, +inf above every
    finite one (NumPy's answers).  1025 thresholds and a NaN threshold are refused."""
    from origin_amd import kernels
    from origin_amd._capi import OriginHipError
    cube = count_cube((3, 5, 7), "nonfinite", 13)
    assert np.isnan(cube).sum() == 3 and np.isinf(cube).sum() == 5
    d = ctx.to_device(cube)
    for keep in keep_maps(35)[:2]:
        kd = None if keep is None else ctx.to_device(keep)
        ref = kept_sorted(cube, keep)
        for name, thr in threshold_lists(cube, 14).items():
            assert np.array_equal(kernels.count_above(ctx, d, thr, kd), count_ref(ref, thr)), name
    assert np.array_equal(kernels.count_above(ctx, d, [-np.inf, np.inf, 1e38]), [100, 0, 3])
    with pytest.raises(OriginHipError):
        kernels.count_above(ctx, d, np.linspace(0, 1, 1025))
    with pytest.raises(OriginHipError):
        kernels.count_above(ctx, d, [0.1, np.nan, 0.3])


# ----------------------------------------------------------------------------- C. lists by hand
SEG_CAP = 8


def segment_counts(nseg, total, rng):
    """Entries per segment with 0, 1, SEG_CAP - 1 and SEG_CAP among them.  nseg >= 10: the first
    four and the last five segments are fixed, ``total`` entries in all, the rest dealt in lots of
    1, 3, SEG_CAP - 1 and SEG_CAP to shuffled segments in between (most stay empty)."""
    cap = SEG_CAP
    if nseg == 1:
        return np.array([cap - 1])
    if nseg == 3:
        return np.array([cap, 0, 1])
    counts = np.zeros(nseg, np.int64)
    counts[:4], counts[-5:] = [0, 1, cap - 1, cap], [cap, 0, 1, cap - 1, cap]
    left = total - counts.sum()
    assert left >= 0
    for s in 4 + rng.permutation(nseg - 9):
        if left == 0:
            break
        counts[s] = min(left, rng.choice([1, 3, cap - 1, cap]))
        left -= counts[s]
    assert left == 0
    return counts


def lists_field(shape, seed, density=0.1):
    """One voxel in ten non-zero, both signs, values on a grid of 0.1 (repeated values)."""
    rng = np.random.default_rng(seed)
    v = np.round(rng.normal(0.0, 2.0, shape), 1).astype(np.float32)
    v[v == 0] = np.float32(0.2)
    v[rng.random(shape) >= density] = 0.0
    return v


def thinned(field, n, rng):
    """``field`` with all but n of its non-zero voxels set to zero."""
    idx = rng.permutation(np.flatnonzero(field.reshape(-1)))
    out = field.copy()
    out.reshape(-1)[idx[n:]] = 0.0
    return out


@pytest.fixture(scope="module", params=["one", "three", "two_steps"])
def lists(request, ctx, ncu):
    """(host field (40, 24, 28), its SparseCube, counts): 1, 3 and num_cu * 16 + 5 segments of
    8 slots.  One and three segments hold 7 and 9 entries (the field is thinned to them); the
    last is the full field, more segments than origin_sparse_count_above launches blocks."""
    rng = np.random.default_rng(21)
    field = lists_field((40, 24, 28), 20)
    nseg = {"one": 1, "three": 3, "two_steps": ncu * 16 + 5}[request.param]
    counts = segment_counts(nseg, np.count_nonzero(field), rng)
    if nseg < 10:
        field = thinned(field, counts.sum(), rng)
    else:
        assert 0.08 < np.mean(field != 0) < 0.12
        blocks = rg.sparse_count_blocks(ncu, nseg)
        assert blocks < nseg <= 2 * blocks and counts[blocks:].sum() > 0   # a second trip, not empty
        assert {0, 1, SEG_CAP - 1, SEG_CAP} <= set(counts.tolist())
        assert np.unique(field).size < np.count_nonzero(field) // 4        # repeated values
    assert field.min() < 0 < field.max()
    return field, as_lists(ctx, field, SEG_CAP, counts), counts


def test_lists_read_back(lists):
    """nnz, entries(), dense() and to_host() of hand-made lists: empty and full segments, stale
    entries (1e30 at indices inside the cube) behind every count."""
    field, sp, counts = lists
    assert sp.bufs.nseg == counts.size and sp.nnz == np.count_nonzero(field) == counts.sum()
    idx, val = sp.entries()
    assert idx.dtype == np.int64 and val.dtype == np.float32
    assert np.array_equal(idx, np.flatnonzero(field.reshape(-1)))
    assert np.array_equal(val, field.reshape(-1)[idx])
    assert np.array_equal(sp.dense().to_host(), field)
    assert np.array_equal(sp.to_host(), field)
    got64 = sp.to_host_f64()
    assert got64.dtype == np.float64 and np.array_equal(got64, field.astype(np.float64))


def test_lists_count_above(lists):
    """SparseCube.count_above against the sorted values of the dense host cube: negative
    thresholds add the zeros; the segment loop takes two trips when there are more segments than
    blocks."""
    field, sp, _ = lists
    tl = threshold_lists(field, 22)
    assert any((t < 0).any() for t in tl.values())
    for keep in keep_maps(24 * 28)[:2]:
        ref = kept_sorted(field, keep)
        for name, thr in tl.items():
            assert np.array_equal(sp.count_above(thr, keep), count_ref(ref, thr)), name


def test_lists_zmax_map(lists):
    field, sp, _ = lists
    for keep in keep_maps(24 * 28):
        assert np.array_equal(sp.zmax_map(keep), zmax_ref(field, keep))


def test_lists_where_above(ctx, lists):
    """np.where's order, the values and the gathered aux bytes; cap = 7 forces the second call."""
    field, sp, _ = lists
    auxh = (np.arange(field.size) % 251).astype(np.uint8).reshape(field.shape)
    aux = ctx.to_device(auxh)
    f64 = field.astype(np.float64)
    for t in (0.2, 0.0, 5.0):
        z, y, x = np.where(f64 > t)
        w = sp.where_above(t, aux=aux, cap=7)
        assert np.array_equal(w["z"], z) and np.array_equal(w["y"], y) and np.array_equal(w["x"], x)
        assert np.array_equal(w["value"], f64[z, y, x]) and np.array_equal(w["aux"], auxh[z, y, x])
    assert np.count_nonzero(f64 > 0.2) > 7 or np.count_nonzero(field) < 10


@pytest.mark.parametrize("case", ["one_channel", "negative_plateau"])
def test_lists_zmax_map_of_columns_without_a_zero(ctx, case):
    """A column of a local-maximum cube need not hold a zero: with Nz == 1 a negative 3 x 3
    maximum is the whole column, and a plateau of a negative constant fills its columns.  The map
    is NumPy's: the negative maximum where a kept column has no zero, 0 where keep == 0.

    Before the fix of sparse_zmax_kernel (positive entries only, over a zeroed map) both cases
    failed here: the map held 0 in all 22 (one_channel) / 4 (negative_plateau) columns whose
    NumPy maximum is negative."""
    rng = np.random.default_rng(31)
    if case == "one_channel":
        field = lists_field((1, 8, 12), 30, density=0.5)
        assert (field < 0).sum() > 10 and (field > 0).sum() > 10 and (field == 0).sum() > 10
    else:
        field = lists_field((6, 8, 8), 32)
        field[:, 3:5, 4:6] = -1.5
        field[2, 0, 0], field[:, 7, 7] = -0.7, [0.3, -2.0, 1.1, -0.1, 0.4, -0.6]
    counts = segment_counts(np.count_nonzero(field) // 3 + 10, np.count_nonzero(field), rng)
    sp = as_lists(ctx, field, SEG_CAP, counts)
    assert np.array_equal(sp.to_host(), field)
    S = field.shape[1] * field.shape[2]
    for keep in keep_maps(S):
        want = zmax_ref(field, keep)
        if keep is None or keep.all():
            assert (want < 0).sum() >= 4
        got = sp.zmax_map(keep)
        print(case, "keep", None if keep is None else int(keep.sum()), "columns with a negative "
              "maximum:", int((want < 0).sum()), "of them 0 on the device:",
              int(((want < 0) & (got == 0)).sum()))
        assert np.array_equal(got, want)


# ----------------------------------------------------------------------------- D. the sparse pass
def smoothed(shape, seed):
    """Smoothed noise, like a GLR output: neighbouring voxels correlated."""
    from scipy import ndimage as ndi
    rng = np.random.default_rng(seed)
    a = ndi.uniform_filter(rng.standard_normal(shape).astype(np.float32), 3).astype(np.float32)
    b = ndi.uniform_filter(rng.standard_normal(shape).astype(np.float32), 3).astype(np.float32)
    return a, b


def oracle_local_max(a, b):
    return cpu_ref.compute_local_max(a.astype(float), b.astype(float), np.zeros(a.shape, bool), 3)


@pytest.mark.parametrize("shape", [(1, 8, 8), (2, 5, 12), (5, 4, 4), (33, 9, 64), (70, 31, 100)],
                         ids=str)
def test_sparse_pass_without_a_mask(ctx, ncu, shape):
    """local_max3s_kernel<false>: lists -> host and device dense cubes equal the oracle's
    compute_local_max with an all-false mask; the plan is the restated one."""
    from origin_amd import sparse
    a, b = smoothed(shape, sum(shape))
    g = rg.sparse_plan(ncu, shape)
    assert sparse.plan(ctx, shape) == (g["nseg"], g["seg_cap"])
    refs = oracle_local_max(a, b)
    assert all(np.count_nonzero(r) > 0 for r in refs)
    cubes = sparse.local_max_sparse(ctx, ctx.to_device(a), ctx.to_device(b), None)
    for sp, ref in zip(cubes, refs):
        assert np.array_equal(sp.counts(), rg.sparse_segment_counts(ncu, ref))
        assert np.array_equal(sp.to_host(), ref)
        assert np.array_equal(sp.dense().to_host(), ref)
        idx, val = sp.entries()
        assert np.all(np.diff(idx) > 0) and idx.size == np.count_nonzero(ref)
        assert np.array_equal(val, ref.reshape(-1)[idx])


def test_sparse_pass_one_segment_overflows(ctx, ncu):
    """One segment above its capacity between healthy neighbours (``slot < seg_cap``): the
    overflow is counted and not stored, the neighbours' counts and entries are untouched, waves
    without a lane write 0; the overflowing cube raises, the other one is whole, and
    ``sparse.local_max`` falls back to the dense pass."""
    from origin_amd import sparse
    from origin_amd.device import DeviceArray
    a, b = rg.overflow_case()
    g = rg.sparse_plan(ncu, a.shape)
    rmax, rmin = oracle_local_max(a, b)
    want = np.concatenate([rg.sparse_segment_counts(ncu, rmax), rg.sparse_segment_counts(ncu, rmin)])
    assert want.size == 16 and np.count_nonzero(want > g["seg_cap"]) == 1          # (i)
    assert want[0] > g["seg_cap"] and np.count_nonzero(want == 0) == 4
    da, db = ctx.to_device(a), ctx.to_device(b)
    bufs = sparse.SparseBuffers(ctx, a.shape)
    assert (bufs.nseg, bufs.seg_cap) == (g["nseg"], g["seg_cap"])
    bufs.counts.fill_bytes(0x55)
    sparse.local_max_sparse(ctx, da, db, None, bufs)
    assert np.array_equal(bufs.counts.to_host(), want)                             # (ii)
    with pytest.raises(sparse.SparseOverflow):                                     # (iii)
        sparse.SparseCube(bufs, 0).counts()
    smin = sparse.SparseCube(bufs, 1)                                              # (iv)
    assert np.array_equal(smin.dense().to_host(), rmin) and np.array_equal(smin.to_host(), rmin)
    fa, fb = sparse.local_max(ctx, da, db, None)                                   # (v)
    assert isinstance(fa, DeviceArray) and isinstance(fb, DeviceArray)
    assert np.array_equal(fa.to_host(), rmax) and np.array_equal(fb.to_host(), rmin)


# ----------------------------------------------------------------------------- E. column moves
def move(ctx, name, cube, Nz, S, idx, n, elem, packed):
    from origin_amd import _capi
    _capi.call(name, ctx.handle, cube.p, Nz, S, idx.p, n, elem, packed.p)


def column_cases(ncu):
    big = (ncu * 16 + 1) * 256
    return ([(1, 5, 1, True)]
            + [(37, 300, n, srt) for n in (1, 255, 256, 257) for srt in (True, False)]
            + [(-(-ncu * 16 // 2) + 1, 300, 257, False), (3, big + 3, big, False)])


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_gather_scatter_columns(ctx, ncu, dtype):
    """origin_gather_columns / origin_scatter_columns against NumPy indexing at their own z-chunk
    geometry: one channel per chunk, two with a last chunk of one, a single chunk of three; list
    lengths around a block of 256; sorted and permuted unique indices."""
    elem = np.dtype(dtype).itemsize
    rng = np.random.default_rng(41)
    sentinel = dtype(251)
    for Nz, S, n, srt in column_cases(ncu):
        nzb, zper, last = rg.column_chunks(ncu, Nz, n)
        if Nz == 37:
            assert (zper, last) == (1, 1)
        elif S == 300:
            assert (zper, last) == (2, 1) and nzb == ncu * 4 + 1
        elif Nz == 3:
            assert (nzb, zper) == (1, 3) and -(-n // 256) > ncu * 16
        cube = (rng.standard_normal((Nz, S)) * 50).astype(dtype) if elem == 4 else \
            rng.integers(0, 250, (Nz, S)).astype(dtype)
        idx = rng.permutation(S)[:n].astype(np.int32)
        idx = np.sort(idx) if srt else idx
        assert srt or n < 2 or np.any(np.diff(idx) < 0)
        d_idx = ctx.to_device(idx)
        packed = ctx.to_device(np.full((Nz, n), sentinel, dtype))
        move(ctx, "origin_gather_columns", ctx.to_device(cube), Nz, S, d_idx, n, elem, packed)
        hp = packed.to_host()
        assert np.array_equal(hp, cube[:, idx]), (Nz, S, n, srt)
        target = ctx.to_device(np.full((Nz, S), sentinel, dtype))
        move(ctx, "origin_scatter_columns", target, Nz, S, d_idx, n, elem, packed)
        want = np.full((Nz, S), sentinel, dtype)
        want[:, idx] = hp
        assert np.array_equal(target.to_host(), want), (Nz, S, n, srt)
        again = ctx.to_device(np.full((Nz, n), sentinel, dtype))
        move(ctx, "origin_gather_columns", target, Nz, S, d_idx, n, elem, again)
        assert np.array_equal(again.to_host(), hp), (Nz, S, n, srt)


def test_column_moves_of_nothing_and_bad_element_size(ctx):
    """n == 0 and Nz == 0 leave both buffers as they are; an element size of 2 is refused."""
    from origin_amd._capi import OriginHipError
    cube_h = np.arange(37 * 300, dtype=np.float32).reshape(37, 300)
    packed_h = np.full((37, 5), -77.0, np.float32)
    cube, packed = ctx.to_device(cube_h), ctx.to_device(packed_h)
    idx = ctx.to_device(np.array([4, 0, 299, 7, 150], np.int32))
    for name in ("origin_gather_columns", "origin_scatter_columns"):
        move(ctx, name, cube, 37, 300, idx, 0, 4, packed)
        move(ctx, name, cube, 0, 300, idx, 5, 4, packed)
        assert np.array_equal(cube.to_host(), cube_h) and np.array_equal(packed.to_host(), packed_h)
        with pytest.raises(OriginHipError):
            move(ctx, name, cube, 37, 300, idx, 5, 2, packed)
    assert np.array_equal(cube.to_host(), cube_h) and np.array_equal(packed.to_host(), packed_h)
