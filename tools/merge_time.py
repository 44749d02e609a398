"""Time the spatio-spectral merging (origin_amd/detection.py, csrc/merge.hip) at survey size.

    python tools/merge_time.py [--rows 10000 100000] [--shape 3681 600 600] [--out FILE]

Cases, per row count: a *sparse* field (sources of a few detections each spread over the whole
field: many small components of the near graph) and a *crowded* one (the same number of rows
inside a square small enough to be a single component).  Recorded per case: wall time of
``detection.merge_detections`` (table in, sorted table out, host bookkeeping included; best of
``--repeat``), the components / groups found, and the event profiler's per-kernel-class split from
a second, untimed call at level 1.  Next to it, for scale only, the reference's own recursive
function as it was timed on a CPU-only machine at smaller n (crowded 120 x 120 fields, tol_spat 3,
tol_spec 5; it needs a raised recursion limit there).  Needs a GPU; prints one JSON document and
writes it to ``--out``.  No time here is a pass / fail condition.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REFERENCE_CPU = dict(
    note="reference spatiospectral_merging, measured on a CPU-only machine at smaller n "
         "(synthetic crowded fields, 120 x 120 spaxels, tol_spat 3, tol_spec 5)",
    rows=[1771, 7614, 23443], seconds=[0.65, 6.0, 48.0],
    groups_before_after=[[292, 260], [488, 266], [489, 171]])


def sparse_field(n, shape, seed):
    """Sources of 1..8 detections (two lines, a pixel or two of scatter) all over the field."""
    Nz, Ny, Nx = shape
    rng = np.random.default_rng(seed)
    nsrc = max(n // 4, 1)
    s = rng.integers(0, nsrc, n)
    cy, cx = rng.integers(2, Ny - 2, nsrc), rng.integers(2, Nx - 2, nsrc)
    cz = rng.integers(0, Nz, (nsrc, 2))
    x = np.clip(cx[s] + rng.integers(-1, 2, n), 0, Nx - 1)
    y = np.clip(cy[s] + rng.integers(-1, 2, n), 0, Ny - 1)
    z = np.clip(cz[s, rng.integers(0, 2, n)] + rng.integers(-2, 3, n), 0, Nz - 1)
    return x, y, z


def crowded_field(n, shape, seed):
    """n rows in a square with two rows per spaxel on average: one component."""
    Nz, Ny, Nx = shape
    rng = np.random.default_rng(seed)
    side = min(int(np.sqrt(n / 2)) + 1, Ny, Nx)
    x, y = rng.integers(0, side, n), rng.integers(0, side, n)
    centres = rng.integers(0, Nz, 400)
    z = np.clip(centres[rng.integers(0, 400, n)] + rng.integers(-6, 7, n), 0, Nz - 1)
    return x, y, z


def table(x, y, z, shape):
    """Rows in np.where order (z major), labels in 50 x 50 patches with label 0 present."""
    order = np.lexsort((x, y, z))
    x, y, z = x[order], y[order], z[order]
    area = ((x // 50) + (shape[2] // 50 + 1) * (y // 50)) % 7
    return dict(x0=x, y0=y, z0=z, area=area)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--shape", type=int, nargs=3, default=[3681, 600, 600])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from origin_amd import detection
    from origin_amd.device import default_context

    ctx = default_context(0)
    shape = tuple(args.shape)
    doc = dict(device=ctx.name, shape=shape, tol_spat=3, tol_spec=5, cases={},
               reference_cpu=REFERENCE_CPU)
    warm = table(*sparse_field(64, shape, 0), shape)
    detection.merge_detections(ctx, warm, shape=shape)          # code objects, allocator
    for n in args.rows:
        for name, make in (("sparse", sparse_field), ("crowded", crowded_field)):
            cat = table(*make(n, shape, seed=n % 1000 + len(name)), shape)
            best = None
            for _ in range(args.repeat):
                t0 = time.perf_counter()
                out = detection.merge_detections(ctx, cat, shape=shape)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            ctx.prof_enable(1)
            ctx.prof_reset()
            from origin_amd import kernels
            res = kernels.merge_detections(ctx, cat["x0"], cat["y0"], cat["z0"], cat["area"],
                                           shape, 3, 5)
            prof = ctx.prof_report()
            ctx.prof_enable(0)
            doc["cases"][f"{name}_{n}"] = dict(
                rows=n, wall_ms=best * 1e3, components=int(len(np.unique(res["comp"]))),
                largest_component=int(np.bincount(res["comp"]).max()),
                groups_before=int(out["imatch2"].max()) + 1,
                groups_after=int(len(np.unique(out["imatch"]))),
                kernel_ms={k: round(v[0], 3) for k, v in sorted(prof.items())
                           if k.startswith("merge_")},
                kernel_scopes={k: v[1] for k, v in sorted(prof.items())
                               if k.startswith("merge_")})
            _save(doc, args.out)   # (what is measured so far survives a later step)
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
