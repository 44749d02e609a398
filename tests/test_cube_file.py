"""CPU: the host side of step 0 (origin_amd/fitsio.py: write_cube, open_cube, read_profiles).
Headers and refusals only -- every check of open_cube happens before any device call, so the
library is never loaded here (``no_library`` makes a call an error)."""
import logging
import os

import numpy as np
import pytest

from origin_amd import _capi, fitsio, synth

HERE = os.path.dirname(os.path.abspath(__file__))
DICO = os.path.join(HERE, "golden", "Dico_3FWHM.fits")
SHAPE = (5, 3, 4)
WCS = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CRPIX1": 2.5, "CRPIX2": 1.5,
       "CRVAL1": 53.16, "CRVAL2": -27.78, "CD1_1": -5.5e-5, "CD1_2": 0.0, "CD2_1": 0.0,
       "CD2_2": 5.5e-5, "CUNIT1": "deg", "CUNIT2": "deg"}
WAVE = {"CTYPE3": "AWAV", "CUNIT3": "Angstrom", "CRPIX3": 1.0, "CRVAL3": 4750.0, "CD3_3": 1.25,
        "CD1_3": 0.0, "CD2_3": 0.0, "CD3_1": 0.0, "CD3_2": 0.0}


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a library call was made")
    monkeypatch.setattr(_capi, "call", refuse)
    monkeypatch.setattr(_capi, "load", refuse)


def cube(shape=SHAPE, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape), rng.random(shape) + 0.5


def hdu(name, shape, bitpix, extra=None, xtension=True):
    n = int(np.prod(shape)) * abs(bitpix) // 8
    return (fitsio.header_bytes(fitsio._image_cards(shape, bitpix, not xtension, name, extra))
            + b"\0" * (n + -n % fitsio.BLOCK))


def write_hdus(path, *hdus):
    with open(path, "wb") as f:
        f.write(fitsio.header_bytes(fitsio._image_cards((), 8, True)))
        for h in hdus:
            f.write(h)
    return str(path)


@pytest.mark.parametrize("bitpix", [(-32, -32), (-32, -64), (-64, -32), (-64, -64)])
@pytest.mark.parametrize("stat_first", [False, True])
def test_round_trip_layout(tmp_path, bitpix, stat_first):
    data, stat = cube()
    path = fitsio.write_cube(str(tmp_path / "c.fits"), data, stat, header={**WCS, **WAVE},
                             bitpix=bitpix, stat_first=stat_first)
    info = fitsio.open_cube(path)
    assert info.shape == SHAPE
    assert (info.bitpix_data, info.bitpix_stat) == bitpix
    n = int(np.prod(SHAPE))
    first, second = (bitpix[1], bitpix[0]) if stat_first else bitpix
    off1 = 2 * fitsio.BLOCK                      # primary header + first extension header
    nb1 = n * abs(first) // 8
    off2 = off1 + nb1 + -nb1 % fitsio.BLOCK + fitsio.BLOCK
    assert (info.off_stat, info.off_data) == (off1, off2) if stat_first \
        else (info.off_data, info.off_stat) == (off1, off2)
    assert os.path.getsize(path) % fitsio.BLOCK == 0
    # the bytes at the offsets are the arrays, big-endian
    raw = open(path, "rb").read()
    for off, bp, arr in ((info.off_data, bitpix[0], data), (info.off_stat, bitpix[1], stat)):
        dt = np.dtype(">f4" if bp == -32 else ">f8")
        got = np.frombuffer(raw, dt, n, off).reshape(SHAPE)
        assert np.array_equal(got, arr.astype(dt))
    assert dict(info.wcs_header) == WCS
    assert dict(info.wave_header) == WAVE


def test_long_primary_header_and_dq(tmp_path, caplog):
    data, stat = cube()
    extra = {f"HIERK{i:02d}": float(i) for i in range(80)}      # 80 cards: three header blocks
    plain = fitsio.open_cube(fitsio.write_cube(str(tmp_path / "a.fits"), data, stat, header=WCS))
    with caplog.at_level(logging.WARNING, logger="origin_amd.fitsio"):
        assert not caplog.records
        info = fitsio.open_cube(fitsio.write_cube(
            str(tmp_path / "b.fits"), data, stat, header=WCS, primary_header=extra,
            dq=np.ones(SHAPE, int)))
    assert [r for r in caplog.records if "DQ" in r.getMessage()]
    assert info.primary_header["HIERK79"] == 79.0
    shift = 2 * fitsio.BLOCK
    assert (info.off_data, info.off_stat) == (plain.off_data + shift, plain.off_stat + shift)
    assert info[1:6] == (plain.shape, info.off_data, plain.bitpix_data, info.off_stat,
                         plain.bitpix_stat)
    assert info.wcs_header == plain.wcs_header and not info.wave_header


def refused(tmp_path, *hdus, cut=0):
    path = write_hdus(tmp_path / "bad.fits", *hdus)
    if cut:
        os.truncate(path, os.path.getsize(path) - cut)
    with pytest.raises(ValueError) as e:
        fitsio.open_cube(path)
    assert path in str(e.value)
    return str(e.value)


def test_refuses_missing_stat(tmp_path):
    assert "STAT" in refused(tmp_path, hdu("DATA", SHAPE, -32))


def test_refuses_different_shapes(tmp_path):
    msg = refused(tmp_path, hdu("DATA", SHAPE, -32), hdu("STAT", (5, 3, 5), -32))
    assert "(5, 3, 4)" in msg and "(5, 3, 5)" in msg


def test_refuses_images(tmp_path):
    assert "NAXIS" in refused(tmp_path, hdu("DATA", (3, 4), -32), hdu("STAT", (3, 4), -32))


def test_refuses_integer_data(tmp_path):
    assert "BITPIX" in refused(tmp_path, hdu("DATA", SHAPE, 16), hdu("STAT", SHAPE, -32))


def test_refuses_scaled_data(tmp_path):
    assert "BSCALE" in refused(tmp_path, hdu("DATA", SHAPE, -32, {"BSCALE": 2.0}),
                               hdu("STAT", SHAPE, -32))


def test_refuses_truncated_data_unit(tmp_path):
    # the file ends one byte before the end of the last data unit (the padding is gone too)
    n = int(np.prod(SHAPE)) * 4
    msg = refused(tmp_path, hdu("DATA", SHAPE, -32), hdu("STAT", SHAPE, -32),
                  cut=-n % fitsio.BLOCK + 1)
    assert "truncated" in msg and "1 bytes" in msg


def test_read_profiles_of_the_reference_dictionary():
    profiles, fwhm = fitsio.read_profiles(DICO)
    assert fwhm == [2.0, 6.736842105263158, 12.0]
    assert [(p.dtype, p.shape) for p in profiles] == [(np.float64, (201,))] * 3
    for got, want in zip(profiles, synth.dico_fwhm(3)):
        assert np.abs(got - want).max() <= 2.0 ** -52


def test_read_profiles_refuses_unequal_lengths(tmp_path):
    path = write_hdus(tmp_path / "dico.fits", hdu("PROF00", (201,), -64, {"FWHM": 2.0}),
                      hdu("PROF01", (199,), -64, {"FWHM": 3.0}))
    with pytest.raises(ValueError, match="same size"):
        fitsio.read_profiles(path)
