"""GPU: the band reader ``origin_cube_read_rows`` and the DQ unit of the step-0 kernel
(csrc/ingest.hip) against NumPy, bit for bit.

A band ``[y0, y1)`` has to be the ``[:, y0:y1]`` slice of what the whole field gives
(tests/test_hip_cube_ingest.py: ``expected``), sums with the sign of a zero sum and counts
included, whatever the chunking; the whole field through the band reader has to be
``origin_cube_read``.  With a DQ unit the rule is ``m = ~isfinite(d) | ~isfinite(s) | (dq != 0)``
and everything after ``m`` is unchanged.  Outputs are pre-filled with 0x5a and compared through
their integer views.  (7, 9) planes give bands whose spaxel count is no multiple of 4 (the scalar
form), (24, 28) and (33, 64) the 16-byte form; (33, 64) bands span several blocks."""
import numpy as np
import pytest

from origin_amd import _capi, fitsio, multigpu
from origin_amd.device import default_context
from test_hip_cube_ingest import LONG_HEADER, PAIRS, Outputs, assert_same, expected, make_case

pytestmark = pytest.mark.gpu

PLANES = [(7, 9), (24, 28), (33, 64)]
NZS = [1, 7, 45]
CASES = [(shape, pair) for shape in PLANES for pair in PAIRS]


def bands_of(Ny, Nx):
    """The bands of the issue: whole field, first row, last row, rows 2-4, and the cuts of
    ``OwnerTiling.row_bands`` for 2 and 3 ranks."""
    out = [(0, Ny), (0, 1), (Ny - 1, Ny), (2, 5)]
    for world in (2, 3):
        p = multigpu.OwnerTiling.row_bands(Ny, Nx, world, 1)
        out += [(p.tile(r).y0, p.tile(r).y1) for r in range(world)]
    return sorted(set(out))


def chunkings(Nz):
    return [0, 1, 3, Nz + 5]


def band_of(want, y0, y1):
    return tuple(np.ascontiguousarray(a[..., y0:y1, :]) for a in want)


def rows_route(ctx, info, y0, y1, ppc, off_dq=None, bitpix_dq=0, **shift):
    Nz, Ny, Nx = info.shape
    out = Outputs(ctx, (Nz, y1 - y0, Nx))
    with open(info.path, "rb", buffering=0) as f:
        _capi.call("origin_cube_read_rows", ctx.handle, f.fileno(),
                   info.off_data + shift.get("data", 0), info.bitpix_data,
                   info.off_stat + shift.get("stat", 0), info.bitpix_stat,
                   -1 if off_dq is None else off_dq + shift.get("dq", 0), bitpix_dq, Nz, Ny, Nx,
                   y0, y1, ppc, out.raw.p, out.var.p, out.mask.p, out.wsum.p, out.wcnt.p)
    return out.host()


def whole_route(ctx, info, ppc):
    out = Outputs(ctx, info.shape)
    with open(info.path, "rb", buffering=0) as f:
        _capi.call("origin_cube_read", ctx.handle, f.fileno(), info.off_data, info.bitpix_data,
                   info.off_stat, info.bitpix_stat, out.Nz, out.S, ppc, out.raw.p, out.var.p,
                   out.mask.p, out.wsum.p, out.wcnt.p)
    return out.host()


@pytest.fixture(scope="module")
def ctx():
    return default_context(0)


# ------------------------------------------------------------------------------- bands
@pytest.mark.parametrize("shape,pair", CASES, ids=lambda v: "x".join(str(i) for i in v))
def test_band_is_the_slice_of_the_field(ctx, tmp_path, shape, pair):
    Ny, Nx = shape
    for k, Nz in enumerate(NZS):
        data, stat = make_case(Nz, Ny, Nx, *pair)
        want = expected(data, stat)
        odd = (k + PLANES.index(shape) + PAIRS.index(pair)) % 2
        path = fitsio.write_cube(str(tmp_path / f"c{Nz}.fits"), data, stat, bitpix=pair,
                                 primary_header=LONG_HEADER if odd else None, stat_first=bool(odd))
        info = fitsio.open_cube(path)
        assert (info.off_stat < info.off_data) == bool(odd)
        for ppc in chunkings(Nz):
            for y0, y1 in bands_of(Ny, Nx):
                what = f"Nz={Nz} rows=[{y0},{y1}) planes_per_chunk={ppc}"
                got = rows_route(ctx, info, y0, y1, ppc)
                assert_same(got, band_of(want, y0, y1), what)
                if (y0, y1) == (0, Ny):
                    assert_same(got, whole_route(ctx, info, ppc), "origin_cube_read, " + what)


def test_bands_cover_both_forms():
    """The band list does reach the scalar form, the 16-byte form, uneven cuts and more than one
    64-lane block of four-voxel groups."""
    assert any((y1 - y0) * 9 % 4 for y0, y1 in bands_of(7, 9))
    assert all((y1 - y0) * 28 % 4 == 0 for y0, y1 in bands_of(24, 28))
    assert len({y1 - y0 for y0, y1 in bands_of(7, 9)[1:]} & {2, 3}) == 2     # 7 rows over 2 and 3 ranks
    assert 33 * 64 // 4 > 64 * 2
    assert (0, 11) in bands_of(33, 64) and (17, 33) in bands_of(33, 64)


def test_read_cube_rows(ctx, tmp_path):
    """``fitsio.read_cube(rows=...)``: the band's arrays and the band's white image."""
    data, stat = make_case(7, 24, 28, -64, -32)
    raw, var, m, wsum, cnt = band_of(expected(data, stat), 5, 13)
    path = fitsio.write_cube(str(tmp_path / "w.fits"), data, stat, bitpix=(-64, -32),
                             header={"CRVAL1": 53.0, "CRVAL3": 4750.0})
    d_raw, d_var, d_mask, white, wcs, wave = fitsio.read_cube(path, ctx, planes_per_chunk=2,
                                                              rows=(5, 13))
    assert d_raw.shape == d_var.shape == d_mask.shape == (7, 8, 28) and white.shape == (8, 28)
    assert_same((d_raw.to_host(), d_var.to_host(), d_mask.to_host()), (raw, var, m), "rows")
    assert (cnt == 0).any() and np.array_equal(np.isnan(white), cnt == 0)
    assert np.array_equal(white[cnt > 0], wsum[cnt > 0] / cnt[cnt > 0])
    assert dict(wcs) == {"CRVAL1": 53.0} and dict(wave) == {"CRVAL3": 4750.0}
    with pytest.raises(ValueError, match="rows"):
        fitsio.read_cube(path, ctx, rows=(5, 25))


def test_bad_rows_are_refused(ctx, tmp_path):
    data, stat = make_case(2, 7, 9, -32, -32)
    info = fitsio.open_cube(fitsio.write_cube(str(tmp_path / "r.fits"), data, stat))
    out = Outputs(ctx, info.shape)
    for y0, y1 in ((-1, 3), (3, 3), (4, 2), (0, 8)):
        with open(info.path, "rb", buffering=0) as f, pytest.raises(_capi.OriginHipError) as e:
            _capi.call("origin_cube_read_rows", ctx.handle, f.fileno(), info.off_data, -32,
                       info.off_stat, -32, -1, 0, 2, 7, 9, y0, y1, 0, out.raw.p, out.var.p,
                       out.mask.p, out.wsum.p, out.wcnt.p)
        assert e.value.code == -1, (y0, y1)


def test_short_file_is_an_error(ctx, tmp_path):
    """Offsets shifted beyond the end of the file: ORIGIN_E_STATE, not a hang -- at the first
    chunk and, with one plane per chunk, after chunks are already in flight."""
    data, stat = make_case(7, 7, 9, -32, -32)
    dq = np.zeros(data.shape, int)
    path = fitsio.write_cube(str(tmp_path / "s.fits"), data, stat, dq=dq)
    info = fitsio.open_cube(path, dq=True)
    for shift, ppc in ((dict(stat=8 * 2880), 2), (dict(dq=2880 - 7 * 7 * 9 * 4 + 200), 1), (dict(dq=2880), 0)):
        with pytest.raises(_capi.OriginHipError) as e:
            rows_route(ctx, info, 2, 5, ppc, info.off_dq, 32, **shift)
        assert e.value.code == -5, shift
    # the same call without a shift is fine
    assert_same(rows_route(ctx, info, 2, 5, 1, info.off_dq, 32),
                band_of(expected(data, stat), 2, 5), "unshifted")


# ------------------------------------------------------------------------------- DQ
DQ_TYPE = {8: np.uint8, 16: np.int16, 32: np.int32}
# values whose low byte / low half-word is zero: a test on part of the element would miss them
DQ_FLAGS = {8: [1, 0x80, 0xff], 16: [1, 0x100, -0x8000, 0x7f00],
            32: [1, 0x100, 0x10000, -2 ** 31, 0x01000000, 0x00ff0000]}


def dq_case(Nz, Ny, Nx, bq, pair, seed=0):
    """(data, stat, dq, where): the contract's values plus flags scattered over voxels, one
    flagged voxel with finite DATA and STAT, one flagged NaN voxel, one spaxel flagged at every
    z (all of them finite there)."""
    data, stat = make_case(Nz, Ny, Nx, *pair, seed=seed)
    rng = np.random.default_rng(100 + seed + bq)
    dq = np.zeros((Nz, Ny, Nx), DQ_TYPE[bq])
    flags = DQ_FLAGS[bq]
    at = rng.permutation(dq.size)[:4 * len(flags)]
    dq.reshape(-1)[at] = np.resize(np.array(flags, np.int64), at.size).astype(DQ_TYPE[bq])
    finite = (Nz - 1, 1, 2)
    data[finite], stat[finite], dq[finite] = 1.5, 0.25, flags[-1]
    both = (0, Ny - 1, 1)
    data[both], dq[both] = np.nan, flags[1]
    column = (slice(None), 1, Nx - 2)
    data[column], stat[column] = 2.0, 1.0
    dq[column] = np.resize(np.array(flags, np.int64), Nz).astype(DQ_TYPE[bq])
    return data, stat, dq, dict(finite=finite, both=both, column=column[1:])


def expected_dq(data, stat, dq):
    with np.errstate(over="ignore"):
        d, s = data.astype(np.float32), stat.astype(np.float32)
    m = ~np.isfinite(d) | ~np.isfinite(s) | (dq != 0)
    raw = np.where(m, np.float32(0), d)
    var = np.where(m, np.float32(np.inf), s)
    wsum = np.add.reduce(raw.astype(np.float64), axis=0)
    return raw, var, m.astype(np.uint8), wsum, (~m).sum(0).astype(np.int32)


def bytes_route(ctx, data, stat, dq, pair, bq, y0, y1, ppc, pad=0):
    """The band's planes uploaded as file bytes and ingested ``ppc`` at a time by
    ``origin_cube_ingest_planes_dq``; ``pad``: DQ bytes start that far into their allocation."""
    bd, bs = pair
    Nz, _, Nx = data.shape
    out = Outputs(ctx, (Nz, y1 - y0, Nx))
    S = out.S

    def be(a, fmt):
        return np.ascontiguousarray(a[:, y0:y1], fmt).view(np.uint8).reshape(Nz, -1)
    db, sb = be(data, ">f4" if bd == -32 else ">f8"), be(stat, ">f4" if bs == -32 else ">f8")
    qb = None if dq is None else be(dq, {8: "u1", 16: ">i2", 32: ">i4"}[bq])
    out.wsum.fill_bytes(0)
    out.wcnt.fill_bytes(0)
    keep = []
    for z0 in range(0, Nz, ppc):
        z1 = min(Nz, z0 + ppc)
        d, s = ctx.to_device(db[z0:z1]), ctx.to_device(sb[z0:z1])
        keep += [d, s]
        if qb is None:
            qp, bits = None, 0
        else:
            q = ctx.to_device(np.concatenate([np.zeros(pad, np.uint8), qb[z0:z1].ravel()]))
            keep.append(q)
            qp, bits = q.view(pad, (q.size - pad,)).p, bq
        _capi.call("origin_cube_ingest_planes_dq", ctx.handle, d.p, bd, s.p, bs, qp, bits,
                   z1 - z0, S, out.raw.view(z0 * S, (S,)).p, out.var.view(z0 * S, (S,)).p,
                   out.mask.view(z0 * S, (S,)).p, out.wsum.p, out.wcnt.p)
    ctx.sync()
    return out.host()


@pytest.mark.parametrize("bq", [8, 16, 32])
@pytest.mark.parametrize("shape", [(7, 9), (24, 28)], ids=lambda s: "%dx%d" % s)
def test_dq_masks_every_non_zero_element(ctx, tmp_path, shape, bq):
    Ny, Nx = shape
    for k, pair in enumerate(PAIRS):
        Nz = (7, 45)[k % 2]
        data, stat, dq, at = dq_case(Nz, Ny, Nx, bq, pair)
        want = expected_dq(data, stat, dq)
        plain = expected(data, stat)
        raw, var, m, wsum, cnt = want
        # the flagged finite voxel: 0 / inf / 1, not counted; the flagged column: nothing counted
        f = at["finite"]
        assert plain[2][f] == 0 and (raw[f], var[f], m[f]) == (0, np.inf, 1)
        assert cnt[f[1:]] <= plain[4][f[1:]] - 1
        assert m[at["both"]] == 1 and plain[2][at["both"]] == 1
        assert plain[4][at["column"]] == Nz and cnt[at["column"]] == 0
        assert wsum[at["column"]] == 0 and not np.signbit(wsum[at["column"]])
        path = fitsio.write_cube(str(tmp_path / f"q{k}.fits"), data, stat, bitpix=pair, dq=dq,
                                 dq_bitpix=bq, primary_header=LONG_HEADER if k % 2 else None,
                                 stat_first=bool(k % 2))
        info = fitsio.open_cube(path, dq=True)
        assert info.bitpix_dq == bq
        for y0, y1 in ((0, Ny), (2, 5), (Ny - 1, Ny)):
            for ppc in (0, 3):
                what = f"{pair} rows=[{y0},{y1}) planes_per_chunk={ppc}"
                got = rows_route(ctx, info, y0, y1, ppc, info.off_dq, bq)
                assert_same(got, band_of(want, y0, y1), "file " + what)
                if ppc:
                    assert_same(bytes_route(ctx, data, stat, dq, pair, bq, y0, y1, ppc),
                                band_of(want, y0, y1), "bytes " + what)
        # the white image: NaN where the DQ unit left nothing
        white = fitsio.read_cube(path, ctx, dq=True)[3]
        assert np.isnan(white[at["column"]]) and np.array_equal(np.isnan(white), cnt == 0)
        # and with the default the unit is ignored
        assert_same(rows_route(ctx, fitsio.open_cube(path), 0, Ny, 0), plain, "dq ignored " + str(pair))


@pytest.mark.parametrize("bq", [8, 16, 32])
def test_all_zero_dq_is_no_dq(ctx, tmp_path, bq):
    for shape in ((7, 9), (24, 28)):
        data, stat = make_case(7, *shape, -32, -64)
        dq = np.zeros(data.shape, DQ_TYPE[bq])
        path = fitsio.write_cube(str(tmp_path / "z.fits"), data, stat, bitpix=(-32, -64), dq=dq,
                                 dq_bitpix=bq)
        info = fitsio.open_cube(path, dq=True)
        for y0, y1 in ((0, shape[0]), (2, 5)):
            without = rows_route(ctx, info, y0, y1, 3)
            assert_same(rows_route(ctx, info, y0, y1, 3, info.off_dq, bq), without, f"file {shape}")
            assert_same(bytes_route(ctx, data, stat, dq, (-32, -64), bq, y0, y1, 3), without,
                        f"bytes {shape}")
            assert_same(bytes_route(ctx, data, stat, None, (-32, -64), 0, y0, y1, 3), without,
                        f"bytes, NULL DQ {shape}")


@pytest.mark.parametrize("bq", [8, 16, 32])
def test_dq_base_short_of_the_vector_alignment(ctx, bq):
    """DQ bytes aligned to their element but not to four of them: the scalar form runs and gives
    the same; a base that is not even element-aligned is refused (ORIGIN_E_ARG)."""
    data, stat, dq, _ = dq_case(7, 24, 28, bq, (-32, -32))
    want = expected_dq(data, stat, dq)
    assert_same(bytes_route(ctx, data, stat, dq, (-32, -32), bq, 0, 24, 3, pad=bq // 8), want,
                "element-aligned")
    if bq > 8:
        with pytest.raises(_capi.OriginHipError) as e:
            bytes_route(ctx, data, stat, dq, (-32, -32), bq, 0, 24, 3, pad=1)
        assert e.value.code == -1


def test_dq_arguments(ctx):
    """A DQ pointer needs BITPIX 8 / 16 / 32, no DQ pointer needs 0: ORIGIN_E_ARG otherwise."""
    buf = ctx.to_device(np.zeros(1024, np.uint8))
    out = Outputs(ctx, (1, 2, 4))
    for q, bits in ((buf.p, 0), (buf.p, 64), (buf.p, -32), (None, 16)):
        with pytest.raises(_capi.OriginHipError) as e:
            _capi.call("origin_cube_ingest_planes_dq", ctx.handle, buf.p, -32, buf.p, -32, q, bits,
                       1, 8, out.raw.p, out.var.p, out.mask.p, out.wsum.p, out.wcnt.p)
        assert e.value.code == -1, bits
