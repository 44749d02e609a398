"""FITS files of the step outputs: what ``Step.dump`` / ``Step.load``
exchange with the disk (reference muse_origin/steps.py:301-352, lazy reload :131-160).

The reference writes every cube / image through mpdaf (``obj.write(outf,
convert_float32=False)``, steps.py:319): a header-only primary HDU followed by an IMAGE
extension named ``DATA`` holding the array (float64 unless the array is float32 / integer),
and reads it back with ``Cube(path)`` / ``Image(path)``, which take the ``DATA`` extension.
mpdaf is not part of the reference tree (nor of this image), so that layout is restated from
the FITS standard and mpdaf's documented behaviour and pinned against ``astropy.io.fits``
(the library mpdaf itself writes through): tests/golden/g9_*.fits were written by astropy,
and files written here are read back by astropy where it is installed.

Headers are host work (a few 80-character cards).  The data unit -- the array widened to
the file type and byte-swapped to big-endian -- is produced and consumed on the GPU
(csrc/fits.hip: ``origin_fits_write_data`` / ``origin_fits_read_data`` stream it to / from
the file descriptor in 64 MiB chunks through pinned buffers, conversion, PCIe copy and file
I/O overlapping), so a cube in HBM reaches the file without a host-side conversion pass.  No CPU fallback: without the
library these functions raise.
"""
import ctypes as C
import logging
import os
import re
from collections import OrderedDict, namedtuple

import numpy as np

from . import _capi, cubes     # (cubes imports this module too: only names used at call time)
from .device import DeviceArray, default_context

BLOCK = 2880
CARD = 80

_TYPE_CODE = {np.dtype(np.float32): 0, np.dtype(np.uint8): 1, np.dtype(np.int32): 2,
              np.dtype(np.float64): 3}
_BITPIX_OF = {np.dtype(np.float64): -64, np.dtype(np.float32): -32, np.dtype(np.uint8): 8,
              np.dtype(np.int16): 16, np.dtype(np.int32): 32, np.dtype(np.int64): 64,
              np.dtype(bool): 8}
_DTYPE_OF = {-64: np.dtype(np.float64), -32: np.dtype(np.float32), 8: np.dtype(np.uint8),
             16: np.dtype(np.int16), 32: np.dtype(np.int32), 64: np.dtype(np.int64)}
# element type a data unit decodes to on the device when the caller wants "what the file holds"
_NATIVE_DEV = {-64: np.dtype(np.float64), -32: np.dtype(np.float32), 8: np.dtype(np.uint8),
               16: np.dtype(np.int32), 32: np.dtype(np.int32), 64: np.dtype(np.int32)}


# ------------------------------------------------------------------------------- headers
def _format_value(value):
    if isinstance(value, (bool, np.bool_)):
        return "%20s" % ("T" if value else "F")
    if isinstance(value, (int, np.integer)):
        return "%20d" % int(value)
    if isinstance(value, (float, np.floating)):
        v = float(value)
        if not np.isfinite(v):
            raise ValueError("FITS header values must be finite")
        s = "%.16G" % v
        if "E" in s:
            m, e = s.split("E")
            if "." not in m:
                m += ".0"
            # the value field of a fixed-format card is 20 characters: drop trailing digits of
            # the significand (as astropy.io.fits does) rather than widen the field
            e = "E%+03d" % int(e)
            s = m[:max(20 - len(e), 3)] + e
        else:
            if "." not in s:
                s += ".0"
            s = s[:20]
        return "%20s" % s
    if isinstance(value, str):
        s = value.replace("'", "''")
        if len(s) > 68:
            raise ValueError("string values longer than 68 characters are not supported")
        return "'%-8s'" % s
    raise TypeError(f"unsupported header value {value!r}")


def card(key, value=None, comment=None):
    """One 80-character header card (FITS standard 4.0, fixed format)."""
    key = key.upper()
    if len(key) > 8 or not all(c.isalnum() or c in "-_" for c in key):
        raise ValueError(f"bad FITS keyword {key!r}")
    if key in ("COMMENT", "HISTORY", "") or value is None:
        text = "%-8s%s" % (key, (" " + str(comment)) if comment else "")
        return text[:CARD].ljust(CARD)
    text = "%-8s= %s" % (key, _format_value(value))
    if comment:
        text += " / " + comment
    return text[:CARD].ljust(CARD)


def header_bytes(cards):
    """Cards + END, padded with blanks to a multiple of 2880 bytes."""
    text = "".join(cards) + "END".ljust(CARD)
    text += " " * (-len(text) % BLOCK)
    return text.encode("ascii")


def _parse_value(field):
    s = field.strip()
    if not s:
        return None
    if s[0] == "'":
        out, i = [], 1
        while i < len(s):
            if s[i] == "'":
                if i + 1 < len(s) and s[i + 1] == "'":
                    out.append("'")
                    i += 2
                    continue
                break
            out.append(s[i])
            i += 1
        return "".join(out).rstrip()
    s = s.split("/")[0].strip()
    if s == "T":
        return True
    if s == "F":
        return False
    try:
        return int(s)
    except ValueError:
        return float(s.replace("D", "E"))


def parse_header(buf, offset=0):
    """(OrderedDict keyword -> value, offset of the byte after the header's last block)."""
    hdr = OrderedDict()
    pos = offset
    while True:
        block = bytes(buf[pos:pos + BLOCK])
        if len(block) < BLOCK:
            raise ValueError("truncated FITS header")
        pos += BLOCK
        for i in range(0, BLOCK, CARD):
            c = block[i:i + CARD].decode("ascii")
            key = c[:8].strip()
            if key == "END":
                return hdr, pos
            if c[8:10] == "= ":
                hdr[key] = _parse_value(c[10:])


def data_bytes(hdr):
    """Size of the data unit a header announces (without the padding)."""
    naxis = hdr.get("NAXIS", 0)
    if naxis == 0:
        return 0
    n = 1
    for i in range(1, naxis + 1):
        n *= hdr[f"NAXIS{i}"]
    return (abs(hdr["BITPIX"]) // 8) * hdr.get("GCOUNT", 1) * (hdr.get("PCOUNT", 0) + n)


def scan(path):
    """[(header, data offset, data bytes)] for every HDU of a file (headers only are read)."""
    out = []
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        pos = 0
        while pos < size:
            f.seek(pos)
            buf = f.read(BLOCK)
            # headers longer than one block: keep reading until END
            while True:
                try:
                    hdr, end = parse_header(buf)
                    break
                except ValueError:
                    more = f.read(BLOCK)
                    if not more:
                        raise
                    buf += more
            nb = data_bytes(hdr)
            out.append((hdr, pos + end, nb))
            pos += end + nb + (-nb % BLOCK)
    return out


# ------------------------------------------------------------------------------- writing
def _device_source(ctx, data):
    """(DeviceArray, host dtype the reference would hold) for anything a DataObj may hold."""
    lazy = isinstance(data, cubes.LazyCube) and data.dev is not None
    if lazy or isinstance(data, (DeviceArray, cubes.CubeForm)):
        dev = cubes.dense(ctx, data)
        return dev, np.dtype(data._dtype) if lazy else dev.dtype
    host = cubes.host_array(data)
    ref_dtype = host.dtype
    if host.dtype == bool:
        host = host.astype(np.uint8)
    elif host.dtype in (np.dtype(np.int64), np.dtype(np.int16)):
        if host.size and (host.max() > np.iinfo(np.int32).max or host.min() < np.iinfo(np.int32).min):
            raise ValueError("integer images beyond int32 are not supported")
        host = host.astype(np.int32)
    elif host.dtype not in _TYPE_CODE:
        host = host.astype(np.float64)
        ref_dtype = host.dtype
    return ctx.to_device(host), np.dtype(ref_dtype)


def _image_cards(shape, bitpix, primary, name=None, extra=None):
    cards = [card("SIMPLE", True, "conforms to FITS standard") if primary
             else card("XTENSION", "IMAGE", "Image extension"),
             card("BITPIX", bitpix, "array data type"),
             card("NAXIS", len(shape), "number of array dimensions")]
    for i, n in enumerate(reversed(shape)):
        cards.append(card(f"NAXIS{i + 1}", int(n)))
    if primary:
        cards.append(card("EXTEND", True))
    else:
        cards += [card("PCOUNT", 0, "number of parameters"), card("GCOUNT", 1, "number of groups")]
        if name:
            cards.append(card("EXTNAME", name, "extension name"))
    reserved = {"SIMPLE", "XTENSION", "BITPIX", "NAXIS", "EXTEND", "PCOUNT", "GCOUNT", "EXTNAME",
                "END"}
    for k, v in (extra or {}).items():
        if k.upper() in reserved or k.upper().startswith("NAXIS"):
            continue
        cards.append(card(k, *(v if isinstance(v, tuple) else (v,))))
    return cards


def _write_data_unit(f, ctx, dev, bitpix):
    """Append the data unit of a device array to the (unbuffered) open file, padded to a block.
    Conversion, PCIe copy and write() overlap inside the library (origin_fits_write_data)."""
    n = dev.size
    _capi.call("origin_fits_write_data", ctx.handle, dev.p, _TYPE_CODE[dev.dtype], n, bitpix,
               f.fileno())
    f.write(b"\0" * (-(n * (abs(bitpix) // 8)) % BLOCK))


def write_image(path, data, name="DATA", header=None, bitpix=None, ctx=None,
                primary_header=None):
    """Write one array as ``<primary, no data> + <IMAGE extension `name`>`` -- the layout of
    mpdaf's ``DataArray.write`` for an object without variance or mask, which is what
    ``Step.store_cube`` / ``store_image`` create (steps.py:284-299, mask=nomask).

    ``data``: any form ``cubes.dense`` takes (host data is uploaded).  ``bitpix``
    defaults to the FITS type of the dtype the reference would hold (float64 -> -64 as with
    ``convert_float32=False``)."""
    ctx = ctx or default_context(0)
    dev, ref_dtype = _device_source(ctx, data)
    if bitpix is None:
        bitpix = _BITPIX_OF.get(ref_dtype, -64)
    if dev.dtype not in _TYPE_CODE:
        raise TypeError(f"no device codec for {dev.dtype}")
    tmp = path + ".part"
    with open(tmp, "wb", buffering=0) as f:
        f.write(header_bytes(_image_cards((), 8, True, extra=primary_header)))
        f.write(header_bytes(_image_cards(dev.shape, bitpix, False, name, header)))
        if dev.size:
            _write_data_unit(f, ctx, dev, bitpix)
    os.replace(tmp, path)
    return path


# ------------------------------------------------------------------------------- reading
def find_hdu(path, ext="DATA"):
    """(header, data offset, data bytes) of the extension called ``ext`` (or number ``ext``);
    like mpdaf, falls back to the first HDU with data when no ``DATA`` extension exists."""
    hdus = scan(path)
    if isinstance(ext, int):
        return hdus[ext]
    for h in hdus:
        if str(h[0].get("EXTNAME", "")).upper() == ext.upper():
            return h
    for h in hdus:
        if h[2] and h[0].get("XTENSION", "IMAGE") == "IMAGE":
            return h
    raise KeyError(f"no image data in {path}")


def read_image(path, ext="DATA", dtype=None, ctx=None):
    """(DeviceArray, header) of an image HDU, decoded on the device.  ``dtype``: element type
    of the device array (float32 for the compute kernels); None keeps what the file holds
    (BITPIX -64 -> float64, -32 -> float32, 8 -> uint8, 16/32/64 -> int32)."""
    ctx = ctx or default_context(0)
    hdr, off, nb = find_hdu(path, ext)
    bitpix = hdr["BITPIX"]
    if hdr.get("BSCALE", 1) != 1 or hdr.get("BZERO", 0) != 0:
        raise ValueError("scaled images (BSCALE / BZERO) are not supported")
    shape = tuple(hdr[f"NAXIS{i}"] for i in range(hdr["NAXIS"], 0, -1))
    dtype = np.dtype(dtype) if dtype is not None else _NATIVE_DEV[bitpix]
    if dtype not in _TYPE_CODE:
        raise TypeError(f"no device codec for {dtype}")
    out = DeviceArray(ctx, shape, dtype)
    n, width = out.size, abs(bitpix) // 8
    if os.path.getsize(path) < off + nb:
        raise ValueError(f"{path}: truncated data unit")
    if n * width != nb:
        raise ValueError(f"{path}: header announces {nb} bytes for {n} elements")
    if n:
        with open(path, "rb", buffering=0) as f:
            f.seek(off)
            _capi.call("origin_fits_read_data", ctx.handle, f.fileno(), bitpix, n,
                       _TYPE_CODE[dtype], out.p)
    return out, hdr


class FitsCube:
    """A dumped cube / image reloaded on demand (what ``DataObj.__get__`` of the reference
    turns a path into, steps.py:141-146): ``._data`` is the host array with the file's dtype,
    ``.device(ctx)`` the float32 (or given) device array, both decoded from the file by the
    GPU and cached."""

    def __init__(self, path, ext="DATA"):
        self.path, self.ext = path, ext
        self._host = None
        self._dev = {}
        hdr, _, _ = find_hdu(path, ext)
        self.header = hdr
        self.shape = tuple(hdr[f"NAXIS{i}"] for i in range(hdr["NAXIS"], 0, -1))
        self._dtype = _DTYPE_OF[hdr["BITPIX"]]

    @property
    def _data(self):
        if self._host is None:
            dev, _ = read_image(self.path, self.ext, None)
            self._host = dev.to_host().astype(self._dtype, copy=False)
            dev.free()
        return self._host

    data = _data

    def device(self, ctx, dtype=np.float32):
        key = np.dtype(dtype)
        if key not in self._dev:
            self._dev[key] = read_image(self.path, self.ext, key, ctx)[0]
        return self._dev[key]


# ------------------------------------------------------------------------------- step 0
# The session's way in (reference origin.py:210-244): a MUSE cube file -- primary HDU, then IMAGE
# extensions DATA and STAT (mpdaf's Cube layout) -- becomes cube_raw / var / mask in HBM and the
# white image, through origin_cube_read (csrc/ingest.hip).  Headers are host work; the voxels
# never exist on the host.
_SPATIAL_CARD = re.compile(r"^(C(TYPE|UNIT|RPIX|RVAL|DELT|ROTA)[12]|(CD|PC)[12]_[12]|RADESYS|EQUINOX|"
                           r"LONPOLE|LATPOLE)$")
_SPECTRAL_CARD = re.compile(r"^(C(TYPE|UNIT|RPIX|RVAL|DELT)3|(CD|PC)(3_[123]|[12]_3))$")

CubeFile = namedtuple("CubeFile", "path shape off_data bitpix_data off_stat bitpix_stat "
                                  "wcs_header wave_header primary_header off_dq bitpix_dq",
                      defaults=(None, None))


def open_cube(path, dq=False):
    """The layout of a cube file, checked before any device call: a ``CubeFile`` with the shape
    ``(Nz, Ny, Nx)``, the byte offsets and BITPIX of the DATA and STAT data units, the spatial
    (``wcs_header``) and spectral (``wave_header``) world-coordinate cards of the DATA header as
    plain mappings -- what ``Step.dump`` writes back -- and the primary header.

    DATA and STAT are found by EXTNAME, in either order; both must be 3-D IMAGE extensions of the
    same shape, BITPIX -32 or -64, without BSCALE / BZERO, and wholly in the file: anything else
    is a ``ValueError`` naming the file and the reason.  By default a DQ extension is *ignored*,
    with a warning: mpdaf would mask the voxels it flags, here the mask is the non-finite voxels of
    DATA and STAT alone (what a MUSE pipeline cube carries: its DQ is folded into NaNs).

    ``dq=True`` takes the DQ extension in: ``off_dq`` / ``bitpix_dq`` of the result are its byte
    offset and BITPIX (both ``None`` when the file has none), and the readers mask the voxels
    whose DQ element is not zero.  It must be an IMAGE extension of DATA's shape, BITPIX 8, 16 or
    32, without BSCALE / BZERO, and wholly in the file; anything else is refused in the same way."""
    try:
        hdus = scan(path)
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None
    found = {}
    for h in hdus[1:]:
        name = str(h[0].get("EXTNAME", "")).strip().upper()
        if h[0].get("XTENSION") == "IMAGE" and name in ("DATA", "STAT", "DQ") and name not in found:
            found[name] = h
    for name in ("DATA", "STAT"):
        if name not in found:
            raise ValueError(f"{path}: no {name} image extension")
    if "DQ" in found and not dq:
        logging.getLogger(__name__).warning(
            "%s: the DQ extension is ignored (only non-finite DATA / STAT voxels are masked)", path)
    size = os.path.getsize(path)
    shapes = {}
    for name in ("DATA", "STAT"):
        hdr, off, nb = found[name]
        if hdr.get("NAXIS") != 3:
            raise ValueError(f"{path}: {name} has NAXIS = {hdr.get('NAXIS')}, a cube has 3")
        if hdr["BITPIX"] not in (-32, -64):
            raise ValueError(f"{path}: {name} has BITPIX = {hdr['BITPIX']}, only -32 and -64 are read")
        if hdr.get("BSCALE", 1) != 1 or hdr.get("BZERO", 0) != 0:
            raise ValueError(f"{path}: {name} is scaled (BSCALE / BZERO), which is not supported")
        if size < off + nb:
            raise ValueError(f"{path}: the {name} data unit is truncated "
                             f"({off + nb - size} bytes missing)")
        shapes[name] = tuple(int(hdr[f"NAXIS{i}"]) for i in (3, 2, 1))
    if shapes["DATA"] != shapes["STAT"]:
        raise ValueError(f"{path}: DATA is {shapes['DATA']} but STAT is {shapes['STAT']}")
    if 0 in shapes["DATA"]:
        raise ValueError(f"{path}: empty cube {shapes['DATA']}")
    off_dq = bitpix_dq = None
    if dq and "DQ" in found:
        hdr, off_dq, nb = found["DQ"]
        bitpix_dq = hdr["BITPIX"]
        shape = tuple(int(hdr[f"NAXIS{i}"]) for i in range(hdr.get("NAXIS", 0), 0, -1))
        if shape != shapes["DATA"]:
            raise ValueError(f"{path}: DATA is {shapes['DATA']} but DQ is {shape}")
        if bitpix_dq not in (8, 16, 32):
            raise ValueError(f"{path}: DQ has BITPIX = {bitpix_dq}, only 8, 16 and 32 are read")
        if hdr.get("BSCALE", 1) != 1 or hdr.get("BZERO", 0) != 0:
            raise ValueError(f"{path}: DQ is scaled (BSCALE / BZERO), which is not supported")
        if size < off_dq + nb:
            raise ValueError(f"{path}: the DQ data unit is truncated "
                             f"({off_dq + nb - size} bytes missing)")
    hdr = found["DATA"][0]
    wcs = OrderedDict((k, v) for k, v in hdr.items() if _SPATIAL_CARD.match(k))
    wave = OrderedDict((k, v) for k, v in hdr.items() if _SPECTRAL_CARD.match(k))
    return CubeFile(path, shapes["DATA"], found["DATA"][1], hdr["BITPIX"], found["STAT"][1],
                    found["STAT"][0]["BITPIX"], wcs, wave, hdus[0][0], off_dq, bitpix_dq)


def read_rows(info, ctx, rows, planes_per_chunk=0):
    """Rows ``[y0, y1)`` of the cube file ``info`` (an ``open_cube`` result) on ``ctx``: the
    band-shaped device arrays ``raw``, ``var``, ``mask`` and the host ``(sum, count)`` of the
    band's white image (``origin_cube_read_rows``).  A DQ unit that ``info`` carries is applied."""
    Nz, Ny, Nx = info.shape
    y0, y1 = (int(v) for v in rows)
    if not 0 <= y0 < y1 <= Ny:
        raise ValueError(f"{info.path}: rows [{y0}, {y1}) of a cube with {Ny} rows")
    shape = (Nz, y1 - y0, Nx)
    raw, var = DeviceArray(ctx, shape, np.float32), DeviceArray(ctx, shape, np.float32)
    mask = DeviceArray(ctx, shape, np.uint8)
    wsum, wcnt = DeviceArray(ctx, shape[1:], np.float64), DeviceArray(ctx, shape[1:], np.int32)
    no_dq = info.off_dq is None
    with open(info.path, "rb", buffering=0) as f:
        _capi.call("origin_cube_read_rows", ctx.handle, f.fileno(), info.off_data, info.bitpix_data,
                   info.off_stat, info.bitpix_stat, -1 if no_dq else info.off_dq,
                   0 if no_dq else info.bitpix_dq, Nz, Ny, Nx, y0, y1, int(planes_per_chunk),
                   raw.p, var.p, mask.p, wsum.p, wcnt.p)
    sums = wsum.to_host(), wcnt.to_host()
    wsum.free()
    wcnt.free()
    return raw, var, mask, sums


def read_cube(path, ctx=None, planes_per_chunk=0, rows=None, dq=False):
    """``(raw, var, mask, ima_white, wcs_header, wave_header)`` of a cube file: the float32 /
    float32 / uint8 device arrays as ``ORIGIN.init`` leaves cube_raw, var and mask (0 / inf / 1 at
    the voxels where DATA or STAT is not finite as float32, origin.py:262-274), the white image
    on the host (float64 mean over the unmasked voxels of each spaxel, NaN where there is none;
    origin.py:240) and the two card mappings of ``open_cube``.  The file bytes go to HBM as they
    are, in chunks of ``planes_per_chunk`` planes (0: 64 MiB), and one kernel does the rest.

    ``rows=(y0, y1)``: only those rows of every plane are read; the arrays and the white image
    are the band's, ``(Nz, y1 - y0, Nx)`` and ``(y1 - y0, Nx)``.  ``dq=True``: the voxels a DQ
    extension flags (element != 0) are masked too (``open_cube``)."""
    info = open_cube(path, dq=dq)
    ctx = ctx or default_context(0)
    Nz, Ny, Nx = info.shape
    if rows is not None or info.off_dq is not None:
        raw, var, mask, (wsum, wcnt) = read_rows(info, ctx, rows or (0, Ny), planes_per_chunk)
        return raw, var, mask, white_image(wsum, wcnt), info.wcs_header, info.wave_header
    S = Ny * Nx
    raw, var = DeviceArray(ctx, info.shape, np.float32), DeviceArray(ctx, info.shape, np.float32)
    mask = DeviceArray(ctx, info.shape, np.uint8)
    wsum, wcnt = DeviceArray(ctx, (Ny, Nx), np.float64), DeviceArray(ctx, (Ny, Nx), np.int32)
    with open(path, "rb", buffering=0) as f:
        _capi.call("origin_cube_read", ctx.handle, f.fileno(), info.off_data, info.bitpix_data,
                   info.off_stat, info.bitpix_stat, Nz, S, int(planes_per_chunk), raw.p, var.p,
                   mask.p, wsum.p, wcnt.p)
    ima_white = white_image(wsum.to_host(), wcnt.to_host())
    wsum.free()
    wcnt.free()
    return raw, var, mask, ima_white, info.wcs_header, info.wave_header


def white_image(wsum, wcnt):
    """sum / count, NaN where the count is 0 (the masked mean of origin.py:240)."""
    out = np.full(wsum.shape, np.nan)
    np.divide(wsum, wcnt, out=out, where=wcnt > 0)
    return out


def read_profiles(path):
    """``(profiles, FWHM_profiles)`` of a dictionary of spectral profiles: the 1-D array of every
    HDU after the primary as float64, and its ``FWHM`` card (reference origin.py:515-533).  Host
    work: a few kilobytes."""
    profiles, fwhm = [], []
    with open(path, "rb") as f:
        for hdr, off, nb in scan(path)[1:]:
            if hdr.get("BITPIX") not in _DTYPE_OF or not nb:
                raise ValueError(f"{path}: extension {hdr.get('EXTNAME')!r} holds no profile")
            if "FWHM" not in hdr:
                raise ValueError(f"{path}: extension {hdr.get('EXTNAME')!r} has no FWHM card")
            f.seek(off)
            p = np.frombuffer(f.read(nb), dtype=_DTYPE_OF[hdr["BITPIX"]].newbyteorder(">"))
            profiles.append(p.astype(np.float64) * hdr.get("BSCALE", 1) + hdr.get("BZERO", 0))
            fwhm.append(hdr["FWHM"])
    if not profiles:
        raise ValueError(f"{path}: no profile")
    if len({p.shape[0] for p in profiles}) != 1:
        raise ValueError("The profiles must have the same size")
    return profiles, fwhm


def read_host_image(path, ext=None):
    """Host array of an image HDU with the file's own type, read with NumPy alone (the PSF cubes
    and weight maps of a session: ``fits.getdata``, origin.py:619, :641-643).  ``ext=None``: the
    first HDU that holds data."""
    hdus = scan(path)
    if ext is None:
        hdu = next((h for h in hdus if h[2] and h[0].get("XTENSION", "IMAGE") == "IMAGE"), None)
        if hdu is None:
            raise ValueError(f"{path}: no image data")
    else:
        hdu = find_hdu(path, ext)
    hdr, off, nb = hdu
    shape = tuple(hdr[f"NAXIS{i}"] for i in range(hdr["NAXIS"], 0, -1))
    with open(path, "rb") as f:
        f.seek(off)
        buf = f.read(nb)
    if len(buf) < nb:
        raise ValueError(f"{path}: truncated data unit")
    dt = _DTYPE_OF[hdr["BITPIX"]]
    arr = np.frombuffer(buf, dtype=dt.newbyteorder(">")).astype(dt).reshape(shape)
    if hdr.get("BSCALE", 1) != 1 or hdr.get("BZERO", 0) != 0:
        arr = arr * hdr.get("BSCALE", 1) + hdr.get("BZERO", 0)
    return arr


def write_cube(path, data, stat, header=None, bitpix=-32, primary_header=None, stat_first=False,
               dq=None, dq_bitpix=32):
    """Write host arrays as a cube file -- ``<primary, no data> + DATA + STAT`` image extensions,
    mpdaf's layout -- with NumPy alone: for the synthetic fields, the tests and the timing tool.
    ``bitpix``: -32 / -64, or a pair (DATA, STAT).  ``header``: further cards of both extensions
    (the world coordinates); ``primary_header``: of the primary HDU.  ``stat_first`` swaps the two
    extensions; ``dq``: an integer cube written as a third extension DQ (BITPIX ``dq_bitpix``:
    8, 16 or 32)."""
    bd, bs = bitpix if isinstance(bitpix, (tuple, list)) else (bitpix, bitpix)
    units = [("DATA", np.asarray(data), bd), ("STAT", np.asarray(stat), bs)]
    if stat_first:
        units.reverse()
    if dq is not None:
        units.append(("DQ", np.asarray(dq), dq_bitpix))
    tmp = path + ".part"
    with open(tmp, "wb") as f:
        f.write(header_bytes(_image_cards((), 8, True, extra=primary_header)))
        for name, arr, bp in units:
            if bp not in ((8, 16, 32) if name == "DQ" else (-32, -64)):
                raise ValueError(f"BITPIX {bp} is not written")
            f.write(header_bytes(_image_cards(arr.shape, bp, False, name,
                                              header if name != "DQ" else None)))
            raw = np.ascontiguousarray(arr, dtype=_DTYPE_OF[bp].newbyteorder(">"))
            f.write(raw.tobytes())
            f.write(b"\0" * (-raw.nbytes % BLOCK))
    os.replace(tmp, path)
    return path


# ------------------------------------------------------------------------------- tables
_TABLE_STRUCTURE = ("XTENSION", "BITPIX", "NAXIS", "NAXIS1", "NAXIS2", "PCOUNT", "GCOUNT", "TFIELDS")


def write_table(path, columns, header=None):
    """Binary-table extension with float64 ('D'), int64 ('K'), bool ('L': one byte, ``T`` /
    ``F``) and fixed-width string ('wA': ASCII, blank padded) columns from a mapping name -> 1-D
    array (the purity tables of step 6, steps.py:853-854, the catalogues of steps 7-9: a few
    dozen to a few thousand rows, host work).  ``header``: a mapping of further cards of the
    extension (``CAT3_TS`` of the step-9 tables).  Layout as astropy's
    ``Table.write(format='fits')``: empty primary + BINTABLE."""
    names = list(columns)
    cols = [np.asarray(columns[k]) for k in names]
    nrows = len(cols[0]) if cols else 0
    fields = []
    for i, c in enumerate(cols):
        if c.ndim != 1 or len(c) != nrows:
            raise ValueError("table columns must be 1-D and of equal length")
        if c.dtype == bool:
            cols[i] = np.where(c, b"T", b"F").astype("S1")
            fields.append(("S1", "L"))
        elif c.dtype.kind in "US":
            cols[i] = c = np.char.encode(c, "ascii") if c.dtype.kind == "U" else c
            w = max(c.dtype.itemsize, 1)
            cols[i] = np.array([s.ljust(w) for s in c.tolist()], dtype=f"S{w}")
            fields.append((f"S{w}", f"{w}A"))
        else:
            fields.append((">i8", "K") if np.issubdtype(c.dtype, np.integer) else (">f8", "D"))
    rec = np.zeros(nrows, dtype=[(n, f[0]) for n, f in zip(names, fields)])
    for n, c in zip(names, cols):
        rec[n] = c
    cards = [card("XTENSION", "BINTABLE", "binary table extension"), card("BITPIX", 8),
             card("NAXIS", 2), card("NAXIS1", rec.dtype.itemsize), card("NAXIS2", nrows),
             card("PCOUNT", 0), card("GCOUNT", 1), card("TFIELDS", len(names))]
    for i, (n, f) in enumerate(zip(names, fields)):
        cards += [card(f"TTYPE{i + 1}", n), card(f"TFORM{i + 1}", f[1])]
    for k, v in (header or {}).items():
        if k.upper() in _TABLE_STRUCTURE or k.upper().startswith(("TTYPE", "TFORM")):
            raise ValueError(f"{k} is a structural keyword of the table")
        cards.append(card(k, v))
    raw = rec.tobytes()
    tmp = path + ".part"
    with open(tmp, "wb") as f:
        f.write(header_bytes(_image_cards((), 8, True)))
        f.write(header_bytes(cards))
        f.write(raw + b"\0" * (-len(raw) % BLOCK))
    os.replace(tmp, path)
    return path


def read_table(path, header=None):
    """OrderedDict name -> array of the first BINTABLE extension: 'D', 'K', 'J', 'E' columns as
    native numbers, 'L' as bool, 'wA' as ``str`` without the padding.  ``header``: a mapping that
    receives the extension's cards other than those describing the table's structure."""
    for hdr, off, nb in scan(path):
        if hdr.get("XTENSION") == "BINTABLE":
            break
    else:
        raise KeyError(f"no binary table in {path}")
    form = {"D": ">f8", "K": ">i8", "J": ">i4", "E": ">f4", "L": "S1"}
    dt, kind = [], {}
    for i in range(1, hdr["TFIELDS"] + 1):
        name, tform = str(hdr[f"TTYPE{i}"]), str(hdr[f"TFORM{i}"]).strip()
        if tform.endswith("A") and (tform[:-1].isdigit() or tform == "A"):
            dt.append((name, "S%d" % int(tform[:-1] or 1)))
            kind[name] = "A"
            continue
        tform = tform.lstrip("1")
        if tform not in form:
            raise ValueError(f"unsupported column format {hdr[f'TFORM{i}']!r}")
        dt.append((name, form[tform]))
        kind[name] = tform
    with open(path, "rb") as f:
        f.seek(off)
        rec = np.frombuffer(f.read(hdr["NAXIS1"] * hdr["NAXIS2"]), dtype=dt)
    if header is not None:
        for k, v in hdr.items():
            if k not in _TABLE_STRUCTURE and not k.startswith(("TTYPE", "TFORM")):
                header[k] = v

    def column(n):
        if kind[n] == "L":
            return rec[n] == b"T"
        if kind[n] == "A":
            return np.char.rstrip(np.char.decode(rec[n], "ascii"))
        return rec[n].astype(rec[n].dtype.newbyteorder("="))
    return OrderedDict((n, column(n)) for n, _ in dt)
