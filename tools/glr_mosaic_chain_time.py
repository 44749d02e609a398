"""What the PCA-tail chain buys a mosaic of weighted fields (measurement for DESIGN 3 / 8).

The bench field (3681 x N x N, synthetic), preprocessed once; a GLR plan of TWO weighted fields
over it.  Timed per step, wall clock around a device sync, median of `reps`:
  sequential : pipeline.greedy_pca, then plan.run           (what a mosaic ran before bands)
  chained    : pipeline.greedy_pca_then_glr, default early_budget / max_active
python tools/glr_mosaic_chain_time.py [size] [nz] [reps]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from origin_amd import kernels, pipeline, synth  # noqa: E402
from origin_amd.device import default_context  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 600
    nz = int(sys.argv[2]) if len(sys.argv) > 2 else 3681
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    ctx = default_context(0)
    f = synth.SyntheticField(nz, n, n)
    raw, var, mask = f.arrays()
    print("field made", flush=True)
    d_mask = ctx.to_device(mask.astype(np.uint8))
    pre = pipeline.preprocess(ctx, ctx.to_device(raw), ctx.to_device(var), d_mask, want_cont=False)
    del raw, var
    thr = pipeline.pca_threshold(pre["o2_host"], f.areamap, f.nbAreas, 0.01)
    spx = pipeline.area_lists(f.areamap, f.nbAreas)
    P = f.PSF.shape[1]
    x = np.linspace(0, 1, n)[None, :] * np.ones((n, 1))
    ws = [0.2 + 0.6 * x, 0.8 - 0.6 * x]
    psfs = [f.PSF.astype(np.float64),
            synth.moffat_psf(nz, P, fwhm0=3.2, fwhm1=2.8).astype(np.float64)]
    plan = kernels.GLRPlan(ctx, (nz, n, n), psfs, ws, f.profiles, 1e-8, True)
    try:
        measure(ctx, plan, f, pre, thr, spx, d_mask, (nz, n, n), reps)
    finally:     # (an error must not leave the plan's device memory to the interpreter's teardown)
        ctx.sync()
        plan.close()


def measure(ctx, plan, f, pre, thr, spx, d_mask, shape, reps):
    nz, n, _ = shape
    plan.prepare()
    print("plan prepared", flush=True)
    faint = ctx.empty(shape, np.float32)
    correl, cmin = ctx.empty(shape, np.float32), ctx.empty(shape, np.float32)
    prof_i = ctx.empty(shape, np.uint8)
    state = {"drv": None, "bands": None}

    def sequential():
        _, _, _, state["drv"] = pipeline.greedy_pca(
            ctx, pre["cube_std"], f.areamap, f.nbAreas, thr["thresO2"], thr["testO2"], 50, 100,
            spx=spx, driver=state["drv"], o2_dev=pre["o2"], out=faint)
        plan.run(faint, mask=d_mask, correl=correl, profile=prof_i, correl_min=cmin)

    def chained():
        _, _, _, state["drv"], out = pipeline.greedy_pca_then_glr(
            ctx, plan, pre["cube_std"], f.areamap, f.nbAreas, thr["thresO2"], thr["testO2"], d_mask,
            correl, prof_i, cmin, faint, spx=spx, driver=state["drv"], o2_dev=pre["o2"])
        state["bands"] = out["bands"]

    def timed(fn):
        fn()
        ctx.sync()
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            ctx.sync()
            ts.append(1e3 * (time.perf_counter() - t))
        return float(np.median(ts)), float(min(ts)), float(max(ts))
    res = {}
    for rnd in range(2):       # (A B A B: drift of the device shows as a difference between rounds)
        for name, fn in (("sequential", sequential), ("chained", chained)):
            res.setdefault(name, []).append(timed(fn))
            print(name, "round", rnd, res[name][-1], flush=True)
    early, late = state["bands"]
    print(f"{ctx.name}: two weighted fields {nz} x {n} x {n}, P = {plan.P}, K = {plan.K}, "
          f"precision {plan.precision}, spectral {plan.paths()['spectral']}, rows "
          f"{plan.rows_supported()}, eps {plan.fold_eps()[0]:.2e}")
    for name, rs in res.items():
        print(f"  {name:10s}: " + " | ".join(f"median {m:.1f} ms (min {a:.1f}, max {b:.1f})"
                                            for m, a, b in rs))
    print(f"  bands: early {early}, late {late}", flush=True)


if __name__ == "__main__":
    main()
