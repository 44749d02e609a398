"""GLR time against the PSF size: one JSON line per (P, precision) with the wall time of a
whole run, the spatial and spectral stage times of the context's event profiler, and the MFMA
count of plan.mfma_count().

    python tools/glr_psf_time.py [--p 25,27,31,35,41] [--prec f32,f16x2,bf16] [--nz 3681]
                                 [--n 600] [--reps 5]

The cube is standard normal noise (the GLR's cost does not depend on the data), the PSF the
Moffat cube of synth.moffat_psf at the given size, the dictionary the bench's 20 profiles."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from origin_amd import kernels, synth  # noqa: E402
from origin_amd.device import default_context  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", default="25,27,31,35,41")
    ap.add_argument("--prec", default="f32,f16x2,bf16")
    ap.add_argument("--nz", type=int, default=3681)
    ap.add_argument("--n", type=int, default=600)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = default_context(0)
    Nz, N = a.nz, a.n
    shape = (Nz, N, N)
    rng = np.random.default_rng(0)
    cube = ctx.empty(shape, np.float32)
    for z0 in range(0, Nz, 64):
        m = min(64, Nz - z0)
        cube.view(z0 * N * N, (m, N, N)).upload(rng.standard_normal((m, N, N), dtype=np.float32))
    correl, cmin = ctx.empty(shape, np.float32), ctx.empty(shape, np.float32)
    prof_i = ctx.empty(shape, np.uint8)
    dico = synth.dico_fwhm(20)
    for P in [int(v) for v in a.p.split(",")]:
        psf = synth.moffat_psf(Nz, P).astype(np.float64)
        for prec in a.prec.split(","):
            plan = kernels.GLRPlan(ctx, shape, psf, None, dico, 1e-8, True, precision=prec)

            def run():
                plan.run(cube, mask=None, correl=correl, profile=prof_i, correl_min=cmin,
                         want_maps=False)

            run()
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                run()
            ctx.sync()
            wall = 1e3 * (time.perf_counter() - t0) / a.reps
            ctx.prof_reset()
            ctx.prof_enable(True)
            for _ in range(a.reps):
                run()
            ctx.sync()
            rep = ctx.prof_report()
            ctx.prof_enable(False)
            stage = {k: round(v[0] / a.reps, 3) for k, v in rep.items()}
            n_sp, n_sc = plan.mfma_count()
            print(json.dumps(dict(P=P, precision=prec, plan_precision=plan.precision,
                                  spatial_on_matrix_cores=plan.spatial_on_matrix_cores,
                                  rows_supported=plan.rows_supported(), shape=list(shape),
                                  total_ms=round(wall, 3), stages_ms=stage,
                                  mfma_spatial=n_sp, mfma_spectral=n_sc)), flush=True)
            plan.close()


if __name__ == "__main__":
    main()
