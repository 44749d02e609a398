"""Time the line estimation (origin_amd/lines.py) at survey size on the GPU.

    python tools/lines_time.py [--ndet 1000] [--shape 3681 600 600] [--psf 25] [--out FILE]

Case: ``ndet`` synthetic detections (a continuum source and a line under each) on a noise field
of the bench size, ``size_grid`` 0 and 1.  Recorded per grid size: HIP-event time of the
``origin_lines_estimate`` call (host copies of its small tables and results included), the event
profiler's per-kernel-class split from a second, untimed call at level 2, and the bytes and
float64 operations one problem needs, computed from the shapes.  Baseline: the float64 NumPy
restatement (tests/_line_oracle.py) on the same host for ``--nhost`` of those detections at
size_grid 0, wall clock.  Needs a GPU; prints one JSON document and writes it to ``--out``.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def gaussian_psf(Nz, P, fwhm0=3.6, fwhm1=3.0):
    yy, xx = np.mgrid[:P, :P] - P // 2
    s = ((fwhm0 + (fwhm1 - fwhm0) * np.arange(Nz) / (Nz - 1)) / 2.355)[:, None, None]
    g = np.exp(-(yy ** 2 + xx ** 2)[None] / (2 * s * s))
    return (g / g.sum(axis=(1, 2), keepdims=True)).astype(np.float32).astype(np.float64)


def make_field(shape, P, ndet, seed):
    Nz, Ny, Nx = shape
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal(shape, dtype=np.float32)
    var = rng.uniform(0.8, 1.3, shape).astype(np.float32)
    raw *= np.sqrt(var)
    psf = gaussian_psf(Nz, P)
    h, zz = P // 2, np.arange(Nz)
    dets = np.stack([rng.integers(10, Nz - 10, ndet), rng.integers(h, Ny - h, ndet),
                     rng.integers(h, Nx - h, ndet)], axis=1)
    cont = 300 * (1 + 0.4 * np.sin(zz / 90.0))
    for z0, y0, x0 in dets:
        spec = cont + 300 * np.exp(-0.5 * ((zz - z0) / 1.6) ** 2)
        raw[:, y0 - h:y0 + h + 1, x0 - h:x0 + h + 1] += (spec[:, None, None] * psf).astype(np.float32)
    return raw, var, psf, dets


def per_problem_model(Nz, P):
    """Bytes and float64 operations one problem needs at least, from the shapes: the work matrix
    is written twice and read by two Gram products, two A v products and one A^T u; the raw / var
    windows (float32) are read by the two gathers, the second projection and the two
    least-squares passes; a Gram product is Nz ld^2 multiply-adds on its upper triangle's tiles."""
    ld = (P * P + 15) // 16 * 16
    A = Nz * ld * 8
    window = Nz * P * P * 8
    nt = (ld + 31) // 32
    gram_flop = 2 * (nt * (nt + 1) // 2) * 32 * 32 * Nz * 2
    return dict(ld=ld, work_matrix_bytes=A, bytes=7 * A + 5 * window, gram_flop=gram_flop)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndet", type=int, default=1000)
    ap.add_argument("--shape", type=int, nargs=3, default=[3681, 600, 600])
    ap.add_argument("--psf", type=int, default=25)
    ap.add_argument("--nhost", type=int, default=10)
    ap.add_argument("--grids", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from origin_amd import kernels
    from origin_amd.device import default_context
    import _line_oracle as oracle

    ctx = default_context(0)
    shape = tuple(args.shape)
    raw, var, psf, dets = make_field(shape, args.psf, args.ndet, seed=5)
    d_raw, d_var = ctx.to_device(raw), ctx.to_device(var)
    doc = dict(device=ctx.name, shape=shape, psf=args.psf, ndet=args.ndet,
               per_problem=per_problem_model(shape[0], args.psf), grids={})
    # warm-up: code objects, the allocator's blocks
    kernels.lines_estimate(ctx, d_raw, d_var, psf, None, *dets[:8].T)
    for g in args.grids:
        ctx.timer_start(0)
        res = kernels.lines_estimate(ctx, d_raw, d_var, psf, None, *dets.T, size_grid=g)
        ctx.timer_stop(0)
        ms = ctx.timer_ms(0)
        ctx.prof_enable(2)
        ctx.prof_reset()
        kernels.lines_estimate(ctx, d_raw, d_var, psf, None, *dets.T, size_grid=g)
        prof = ctx.prof_report()
        ctx.prof_enable(0)
        nprob = int(kernels.lines_problem_counts(dets[:, 1], dets[:, 2], g, shape[1],
                                                 shape[2]).sum())
        doc["grids"][str(g)] = dict(
            call_ms=ms, problems=nprob, batches=res["nbatch"], ms_per_detection=ms / args.ndet,
            fallback_rows=int(res["fallback"].sum()),
            kernel_ms={k: round(v[0], 3) for k, v in sorted(prof.items())},
            kernel_launches={k: v[1] for k, v in sorted(prof.items())})
        _save(doc, args.out)   # (what is measured so far survives a later step)
    # host baseline: the float64 restatement, this host's BLAS threads
    sub = dets[:args.nhost]
    t0 = time.perf_counter()
    ref = [oracle.grid_analysis(_Window(raw), _Window(var), psf, None, int(y), int(x), int(z), 0,
                                "flux", 30, 1, 5) for z, y, x in sub]
    host_s = (time.perf_counter() - t0) / max(len(sub), 1)
    got = kernels.lines_estimate(ctx, d_raw, d_var, psf, None, *sub.T)
    diff = max(float(np.max(np.abs(got["line"][i] - r[2])) / np.max(np.abs(r[2])))
               for i, r in enumerate(ref))
    doc["host_baseline"] = dict(detections=len(sub), seconds_per_detection=host_s,
                                threads=os.environ.get("OMP_NUM_THREADS"),
                                max_rel_line_diff_device_vs_host=diff)
    if "0" in doc["grids"]:
        doc["speedup_per_detection_grid0"] = host_s * 1e3 / doc["grids"]["0"]["ms_per_detection"]
    print(_save(doc, args.out))


def _save(doc, out):
    text = json.dumps(doc, indent=1)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")
    return text


class _Window:
    """A float32 cube that the oracle's ``window`` can cut float64 windows from without a
    float64 copy of the whole cube."""

    def __init__(self, cube):
        self.cube, self.shape = cube, cube.shape

    def __getitem__(self, idx):
        return np.asarray(self.cube[idx], dtype=np.float64)


if __name__ == "__main__":
    main()
