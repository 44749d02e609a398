"""Timing of step 0: a cube file to cube_raw / var / mask in HBM, three routes on
the same synthetic file, alternating, after one warm-up round.  Each time is the host clock
around work that ends in ``ctx.sync()``.

  read_cube    ``fitsio.read_cube``: file bytes to HBM, one fused kernel (mask, fill, white image)
  read_image   what the package offered before for the same bytes: ``fitsio.read_image`` of DATA
               and of STAT -- two float32 device arrays, no mask, no fill, no white image
  to_device    the array route: ``ctx.to_device`` of host arrays as ``ORIGIN.init`` leaves them
               (float64 raw, float64 var, bool mask), nothing read from a file

    python tools/ingest_time.py [N] [dir] [repeats]   # cube 3681 x N x N, default 300, /dev/shm, 5

Prints one JSON line (profiles/ingest_300.json)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from origin_amd import fitsio  # noqa: E402
from origin_amd.device import default_context  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 300
out = sys.argv[2] if len(sys.argv) > 2 else "/dev/shm"
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
NZ = int(os.environ.get("INGEST_NZ", 3681))
ctx = default_context(0)
shape = (NZ, N, N)
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
for it in range(repeats + 1):                  # round 0 warms up (file cache, pinned pools, clocks)
    for name, fn, _ in routes:
        ctx.sync()
        t = time.perf_counter()
        fn()
        ctx.sync()
        if it:
            times[name].append(time.perf_counter() - t)
os.remove(path)
doc = {"device": ctx.name, "shape": list(shape), "bitpix": [-32, -32], "repeats": repeats,
       "file_dir": out, "routes": {}}
for name, _, nbytes in routes:
    t = np.array(times[name])
    doc["routes"][name] = {"min_s": round(float(t.min()), 4), "median_s": round(float(np.median(t)), 4),
                           "max_s": round(float(t.max()), 4), "host_bytes": int(nbytes),
                           "GB_per_s_median": round(nbytes / float(np.median(t)) / 1e9, 2)}
print(json.dumps(doc))
