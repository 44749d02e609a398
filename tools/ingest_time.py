"""Timing of step 0: a cube file to cube_raw / var / mask in HBM, on the same
synthetic file, alternating routes, after one warm-up round.  Each time is the host clock around
work that ends in ``ctx.sync()``.

One device (default), three routes:

  read_cube    ``fitsio.read_cube``: file bytes to HBM, one fused kernel (mask, fill, white image)
  read_image   what the package offered before for the same bytes: ``fitsio.read_image`` of DATA
               and of STAT -- two float32 device arrays, no mask, no fill, no white image
  to_device    the array route: ``ctx.to_device`` of host arrays as ``ORIGIN.init`` leaves them
               (float64 raw, float64 var, bool mask), nothing read from a file

    python tools/ingest_time.py [N] [dir] [repeats]   # cube 3681 x N x N, default 300, /dev/shm, 5

Prints one JSON line (profiles/ingest_300.json).

Several devices (``--devices 0,0``), two routes through the session interface alone --
``SimpleOrig.from_cube(path, ..., devices=[...])`` and ``step01_preprocessing`` -- so that this
file also runs against a checkout that has no band reader yet:

  from_cube         the session opened from the file
  from_cube_step1   the same, then step 1

The host clock is taken around each, in alternating rounds after a warm-up; afterwards each route
runs once more in a fresh child process that reports its peak resident set (``ru_maxrss``; on
Linux that figure also carries the high-water mark of the starting process up to the ``exec``,
so it is an upper bound of the route's own).

    python tools/ingest_time.py --devices 0,0 [N] [dir] [repeats]

Prints one JSON line (the two halves of profiles/ingest_tiled_300.json)."""
import argparse
import gc
import json
import os
import resource
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from origin_amd import fitsio, synth  # noqa: E402
from origin_amd.device import default_context  # noqa: E402

NZ = int(os.environ.get("INGEST_NZ", 3681))


def write_file(N, out):
    """The synthetic cube file; returns (path, data, stat)."""
    rng = np.random.default_rng(0)
    reps = NZ // 64 + 1
    data = np.concatenate([rng.standard_normal((64, N, N)).astype(np.float32)] * reps)[:NZ]
    stat = np.concatenate([(1 + 0.2 * rng.random((64, N, N))).astype(np.float32)] * reps)[:NZ]
    masked = np.zeros((N, N), bool)
    masked[:2], masked[-2:], masked[:, :2], masked[:, -2:] = True, True, True, True
    data[:, masked] = np.nan                       # NaN at the masked voxels, as a pipeline cube
    stat[:, masked] = np.nan
    data[rng.integers(0, NZ, 1000), rng.integers(2, N - 2, 1000), rng.integers(2, N - 2, 1000)] = np.nan
    path = fitsio.write_cube(os.path.join(out, "origin_ingest_time.fits"), data, stat, bitpix=-32)
    return path, data, stat


def summary(t):
    t = np.array(t)
    return {"min_s": round(float(t.min()), 4), "median_s": round(float(np.median(t)), 4),
            "max_s": round(float(t.max()), 4)}


# ------------------------------------------------------------------------------- one device
def one_device(N, out, repeats):
    ctx = default_context(0)
    path, data, stat = write_file(N, out)
    file_bytes = 2 * data.size * 4
    # the array route's inputs (origin.py:262-274)
    m = ~np.isfinite(data) | ~np.isfinite(stat)
    raw64 = np.where(m, 0, data).astype(np.float64)
    var64 = np.where(m, np.inf, stat).astype(np.float64)
    del data, stat

    def read_cube():
        for a in fitsio.read_cube(path, ctx)[:3]:
            a.free()

    def read_image():
        for ext in ("DATA", "STAT"):
            fitsio.read_image(path, ext, np.float32, ctx)[0].free()

    def to_device():
        for a in (ctx.to_device(raw64, np.float32), ctx.to_device(var64, np.float32),
                  ctx.to_device(m, np.uint8)):
            a.free()

    routes = [("read_cube", read_cube, file_bytes), ("read_image", read_image, file_bytes),
              ("to_device", to_device, raw64.nbytes + var64.nbytes + m.nbytes)]
    times = {name: [] for name, _, _ in routes}
    for it in range(repeats + 1):              # round 0 warms up (file cache, pinned pools, clocks)
        for name, fn, _ in routes:
            ctx.sync()
            t = time.perf_counter()
            fn()
            ctx.sync()
            if it:
                times[name].append(time.perf_counter() - t)
    os.remove(path)
    doc = {"device": ctx.name, "shape": [NZ, N, N], "bitpix": [-32, -32], "repeats": repeats,
           "file_dir": out, "routes": {}}
    for name, _, nbytes in routes:
        med = float(np.median(times[name]))
        doc["routes"][name] = dict(summary(times[name]), host_bytes=int(nbytes),
                                   GB_per_s_median=round(nbytes / med / 1e9, 2))
    print(json.dumps(doc))


# ------------------------------------------------------------------------------- several devices
TILED_ROUTES = ("from_cube", "from_cube_step1")


def tiled_route(route, path, devices):
    """One run of a route; the seconds it took.  The session is closed and its cubes released
    before the next one starts."""
    from origin_amd.steps import SimpleOrig
    psf, profiles = synth.moffat_psf(NZ, 9).astype(float), synth.dico_fwhm(3)
    gc.collect()
    t = time.perf_counter()
    orig = SimpleOrig.from_cube(path, profiles, psf, FWHM_PSF=3.3, devices=devices)
    if route == "from_cube_step1":
        orig.step01_preprocessing()          # (returns with its images on the host: all work done)
    dt = time.perf_counter() - t
    sess = orig.__dict__.get("_hip_session")
    if sess is not None:
        sess.close()
    return dt


def tiled(N, out, repeats, devices):
    path = write_file(N, out)[0]
    gc.collect()
    try:
        times = {name: [] for name in TILED_ROUTES}
        for it in range(repeats + 1):
            for name in TILED_ROUTES:
                dt = tiled_route(name, path, devices)
                if it:
                    times[name].append(dt)
        rss = {}
        for name in TILED_ROUTES:              # a fresh process per route: its own peak
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--devices",
                                ",".join(map(str, devices)), "--child", name, "--file", path],
                               stdout=subprocess.PIPE, check=True, timeout=900)
            rss[name] = json.loads(r.stdout.decode().strip().splitlines()[-1])["maxrss_MB"]
    finally:
        os.remove(path)
    doc = {"device": default_context(devices[0]).name, "devices": devices, "shape": [NZ, N, N],
           "bitpix": [-32, -32], "repeats": repeats, "file_dir": out,
           "file_bytes": 2 * NZ * N * N * 4, "routes": {}}
    for name in TILED_ROUTES:
        doc["routes"][name] = dict(summary(times[name]), child_maxrss_MB=rss[name])
    print(json.dumps(doc))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("N", nargs="?", type=int, default=300)
    ap.add_argument("dir", nargs="?", default="/dev/shm")
    ap.add_argument("repeats", nargs="?", type=int, default=5)
    ap.add_argument("--devices", help="device ordinals of a tiled session, e.g. 0,0")
    ap.add_argument("--child", choices=TILED_ROUTES, help=argparse.SUPPRESS)
    ap.add_argument("--file", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.devices is None:
        return one_device(a.N, a.dir, a.repeats)
    devices = [int(d) for d in a.devices.split(",")]
    if a.child:
        tiled_route(a.child, a.file, devices)
        print(json.dumps({"maxrss_MB": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024, 1)}))
        return None
    return tiled(a.N, a.dir, a.repeats, devices)


if __name__ == "__main__":
    main()
