"""Time the cube standard deviation of step 9 (kernels.cube_std, csrc/stats.hip) at survey size.

    python tools/stats_time.py [--shape 3681 600 600] [--repeat 5] [--out profiles/stats_time.json]

Measured, on one cube of normal deviates made on the device side of the upload:

* ``cube_std``: HIP events on the context's stream around the whole call (two passes of
  ``origin_cube_moments``, each ending in a 24-byte copy to the host), best and median of
  ``--repeat``; one pass alone the same way; the achieved rate against the algorithmic bytes
  (2 passes x 4 bytes per voxel), next to the 6.29 TB/s float4-copy figure SURVEY.md cites;
* the host path it replaces: ``to_host_f64`` (D2H and widening to float64) and ``np.std`` of the
  result, wall time, once (``--no-host`` leaves it out: it needs 8 bytes per voxel of host memory
  and as much again inside ``np.std``).

Needs a GPU; prints one JSON document and writes it to ``--out``.  No time here is a pass / fail
condition.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_TBS = 6.29      # float4 copy, SURVEY.md


def timed(ctx, fn, repeat):
    ms = []
    for _ in range(repeat):
        ctx.timer_start(0)
        out = fn()
        ctx.timer_stop(0)
        ctx.sync()
        ms.append(ctx.timer_ms(0))
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[3681, 600, 600])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stats_time.json"))
    args = ap.parse_args()

    from origin_amd import kernels
    from origin_amd.device import default_context

    ctx = default_context(0)
    Nz, Ny, Nx = args.shape
    n = Nz * Ny * Nx
    rng = np.random.default_rng(1)
    plane = Ny * Nx
    cube = ctx.empty((Nz, Ny, Nx), np.float32)
    step = max(1, (1 << 26) // plane)            # upload in slabs of about 256 MB
    for z0 in range(0, Nz, step):
        z1 = min(Nz, z0 + step)
        slab = rng.standard_normal((z1 - z0, Ny, Nx), dtype=np.float32)
        cube.view(z0 * plane, slab.shape).upload(slab * np.float32(2.5) + np.float32(0.3))
    ctx.sync()
    kernels.cube_std(ctx, cube)                                 # code objects, scratch
    std, ms_std = timed(ctx, lambda: kernels.cube_std(ctx, cube), args.repeat)
    _, ms_one = timed(ctx, lambda: kernels.cube_moments(ctx, cube, 0.3), args.repeat)
    keep = ctx.to_device((np.arange(plane) % 2).astype(np.uint8))
    _, ms_keep = timed(ctx, lambda: kernels.cube_moments(ctx, cube, 0.3, keep), args.repeat)
    doc = dict(device=ctx.name, shape=[Nz, Ny, Nx], voxels=n, std=std,
               blocks=kernels.cube_moments_sweep(n) // (kernels.MOMENTS_LANES * kernels.MOMENTS_VEC),
               cube_std_ms=dict(best=min(ms_std), median=float(np.median(ms_std)), all=ms_std),
               one_pass_ms=dict(best=min(ms_one), median=float(np.median(ms_one))),
               one_pass_keep_ms=dict(best=min(ms_keep), median=float(np.median(ms_keep))),
               algorithmic_bytes=2 * 4 * n,
               cube_std_TBs=2 * 4 * n / (min(ms_std) * 1e-3) / 1e12,
               one_pass_TBs=4 * n / (min(ms_one) * 1e-3) / 1e12,
               one_pass_keep_TBs=4 * n / (min(ms_keep) * 1e-3) / 1e12,
               copy_TBs_survey=COPY_TBS)
    _save(doc, args.out)
    if not args.no_host:
        t0 = time.perf_counter()
        host = cube.to_host_f64()
        t1 = time.perf_counter()
        ref = float(np.std(host))
        t2 = time.perf_counter()
        doc["host_path"] = dict(to_host_f64_s=t1 - t0, np_std_s=t2 - t1, total_s=t2 - t0, std=ref,
                                rel_diff=abs(std - ref) / ref)
        doc["speedup_over_host_path"] = (t2 - t0) / (min(ms_std) * 1e-3)
    print(_save(doc, args.out))


def _save(doc, out):
    text = json.dumps(doc, indent=1)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")
    return text


if __name__ == "__main__":
    main()
