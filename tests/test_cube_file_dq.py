"""CPU: ``fitsio.open_cube(path, dq=True)`` -- the DQ extension of a cube file taken in, or
refused with its reason, before any device call (``no_library`` makes a call an error); and
``dq=False`` on the same files, which returns what it always did."""
import logging
import os

import numpy as np
import pytest

from origin_amd import _capi, fitsio

SHAPE = (5, 3, 4)
N = int(np.prod(SHAPE))


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a library call was made")
    monkeypatch.setattr(_capi, "call", refuse)
    monkeypatch.setattr(_capi, "load", refuse)


def cube(seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(SHAPE), rng.random(SHAPE) + 0.5


def hdu(name, shape, bitpix, extra=None):
    n = int(np.prod(shape)) * abs(bitpix) // 8
    return (fitsio.header_bytes(fitsio._image_cards(shape, bitpix, False, name, extra))
            + b"\0" * (n + -n % fitsio.BLOCK))


def write_hdus(path, *hdus, cut=0):
    with open(path, "wb") as f:
        f.write(fitsio.header_bytes(fitsio._image_cards((), 8, True)))
        for h in hdus:
            f.write(h)
    if cut:
        os.truncate(path, os.path.getsize(path) - cut)
    return str(path)


def padded(nbytes):
    return nbytes + -nbytes % fitsio.BLOCK


@pytest.mark.parametrize("bitpix", [8, 16, 32])
def test_dq_offset_and_bitpix(tmp_path, bitpix, caplog):
    data, stat = cube()
    dq = np.zeros(SHAPE, int)
    dq[1, 2, 3] = 64
    path = fitsio.write_cube(str(tmp_path / "c.fits"), data, stat, dq=dq, dq_bitpix=bitpix)
    with caplog.at_level(logging.WARNING, logger="origin_amd.fitsio"):
        info = fitsio.open_cube(path, dq=True)
    assert not caplog.records                       # the extension is used: nothing to warn of
    assert info.bitpix_dq == bitpix
    # primary header, then per unit one header block and the padded data unit: DATA, STAT, DQ
    assert info.off_data == 2 * fitsio.BLOCK
    assert info.off_stat == info.off_data + padded(N * 4) + fitsio.BLOCK
    assert info.off_dq == info.off_stat + padded(N * 4) + fitsio.BLOCK
    assert os.path.getsize(path) == info.off_dq + padded(N * bitpix // 8)
    # the bytes there are the flags, big-endian
    dt = np.dtype({8: "u1", 16: ">i2", 32: ">i4"}[bitpix])
    got = np.frombuffer(open(path, "rb").read(), dt, N, info.off_dq).reshape(SHAPE)
    assert np.array_equal(got, dq)
    # the fields are appended: the first nine are where they were
    assert info._fields[:9] == ("path", "shape", "off_data", "bitpix_data", "off_stat",
                                "bitpix_stat", "wcs_header", "wave_header", "primary_header")
    assert info._fields[9:] == ("off_dq", "bitpix_dq")


def test_default_ignores_dq_as_before(tmp_path, caplog):
    data, stat = cube()
    plain = fitsio.open_cube(fitsio.write_cube(str(tmp_path / "a.fits"), data, stat))
    path = fitsio.write_cube(str(tmp_path / "b.fits"), data, stat, dq=np.ones(SHAPE, int))
    with caplog.at_level(logging.WARNING, logger="origin_amd.fitsio"):
        info = fitsio.open_cube(path)
        again = fitsio.open_cube(path, dq=False)
    assert len([r for r in caplog.records if "DQ" in r.getMessage() and "ignored" in r.getMessage()]) == 2
    assert info == again and info.off_dq is None and info.bitpix_dq is None
    assert info[1:6] == plain[1:6] and info.primary_header == plain.primary_header
    # write_cube's default DQ unit is BITPIX 32, as before
    assert fitsio.open_cube(path, dq=True).bitpix_dq == 32


def test_no_dq_extension(tmp_path, caplog):
    data, stat = cube()
    path = fitsio.write_cube(str(tmp_path / "a.fits"), data, stat)
    with caplog.at_level(logging.WARNING, logger="origin_amd.fitsio"):
        info = fitsio.open_cube(path, dq=True)
    assert info.off_dq is None and info.bitpix_dq is None and not caplog.records
    assert info == fitsio.open_cube(path)


BAD_DQ = {
    "shape": (dict(shape=(5, 3, 5)), ["(5, 3, 4)", "(5, 3, 5)", "DQ"]),
    "image": (dict(shape=(3, 4)), ["(5, 3, 4)", "(3, 4)", "DQ"]),
    "bitpix64": (dict(bitpix=64), ["DQ", "BITPIX = 64"]),
    "bitpix-32": (dict(bitpix=-32), ["DQ", "BITPIX = -32"]),
    "bscale": (dict(extra={"BSCALE": 2.0}), ["DQ", "BSCALE"]),
    "bzero": (dict(extra={"BZERO": 32768.0}, bitpix=16), ["DQ", "BZERO"]),
    "truncated": (dict(cut=-(N * 4) % fitsio.BLOCK + 1), ["DQ", "truncated", "1 bytes"]),
}


@pytest.mark.parametrize("case", sorted(BAD_DQ))
def test_refusals(tmp_path, case, caplog):
    kw, words = BAD_DQ[case]
    path = write_hdus(tmp_path / "bad.fits", hdu("DATA", SHAPE, -32), hdu("STAT", SHAPE, -32),
                      hdu("DQ", kw.get("shape", SHAPE), kw.get("bitpix", 32), kw.get("extra")),
                      cut=kw.get("cut", 0))
    with pytest.raises(ValueError) as e:
        fitsio.open_cube(path, dq=True)
    assert path in str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    # the same file with the default: the DQ unit is not looked at, only warned of
    with caplog.at_level(logging.WARNING, logger="origin_amd.fitsio"):
        info = fitsio.open_cube(path)
    assert info.shape == SHAPE and info.off_dq is None
    assert [r for r in caplog.records if "DQ" in r.getMessage()]


def test_write_cube_refuses_other_dq_bitpix(tmp_path):
    data, stat = cube()
    with pytest.raises(ValueError, match="BITPIX"):
        fitsio.write_cube(str(tmp_path / "x.fits"), data, stat, dq=np.zeros(SHAPE, int),
                          dq_bitpix=64)
