"""Time one segmentation (mask, erosion, dilation, disc, labels) on the host and on the device.

    python tools/segmap_time.py [--sizes 300 600] [--fwhm 4] [--repeat 30] [--out FILE]

Per size, on a seeded synthetic map (positive noise plus 60 Gaussian blobs) with the threshold of
the host fit: wall time of ``tests/_segmap_oracle.labels_at`` (the SciPy code the steps ran before
csrc/segmap.hip) and of ``origin_amd.segmap.labels_at`` (upload of the float64 map, kernels,
download of the int32 labels) in the same process, the two alternating; the same for the label of
the union of two label maps; and the kernels alone from the event profiler in a separate loop.
Median and min / max over ``--repeat`` calls after 5 warm-up calls.  The labels of the two paths
are compared before anything is timed.  Needs a GPU; prints one JSON document and writes it to
``--out``.  No time here is a pass / fail condition.
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


def synthetic_map(N, seed=7, nblobs=60):
    rng = np.random.default_rng(seed)
    data = (rng.standard_normal((40, N, N)) ** 2).mean(axis=0)
    yy, xx = np.mgrid[:N, :N]
    for _ in range(nblobs):
        cy, cx = rng.integers(0, N, 2)
        sig, amp = rng.uniform(1.5, 4.0), rng.uniform(2.0, 6.0)
        data += amp * np.exp(-0.5 * ((yy - cy) ** 2 + (xx - cx) ** 2) / sig ** 2)
    return data


def stats(ms):
    ms = np.asarray(ms) * 1e3
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(ms.min()), 4),
                max_ms=round(float(ms.max()), 4), n=len(ms))


def alternate(fa, fb, repeat, warm=5):
    ta, tb = [], []
    for i in range(warm + repeat):
        for f, t in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            f()
            if i >= warm:
                t.append(time.perf_counter() - t0)
    return stats(ta), stats(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[300, 600])
    ap.add_argument("--fwhm", type=int, default=4)
    ap.add_argument("--pfa", type=float, default=0.01)
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segmap_600.json"))
    args = ap.parse_args()

    import _segmap_oracle as oracle
    from origin_amd import segmap
    from origin_amd.device import default_context
    from origin_amd.thresholds import compute_thresh_gaussfit
    ctx = default_context(0)
    doc = dict(device=ctx.name, fwhm_fsf=args.fwhm, pfa=args.pfa, repeat=args.repeat, sizes={})
    for N in args.sizes:
        data = synthetic_map(N)
        gamma = compute_thresh_gaussfit(data, args.pfa)[2]
        want, nwant = oracle.labels_at(data, gamma, args.fwhm)
        got, ngot = segmap.labels_at(ctx, data, gamma, args.fwhm)
        same = bool(ngot == nwant and np.array_equal(got, want))
        other = oracle.labels_at(synthetic_map(N, seed=8), gamma, 0)[0]
        same_merged = bool(np.array_equal(segmap.merged_labels(ctx, want, other),
                                          oracle.merged_labels(want, other)))
        host, dev = alternate(lambda: oracle.labels_at(data, gamma, args.fwhm),
                              lambda: segmap.labels_at(ctx, data, gamma, args.fwhm), args.repeat)
        host_m, dev_m = alternate(lambda: oracle.merged_labels(want, other),
                                  lambda: segmap.merged_labels(ctx, want, other), args.repeat)
        ctx.prof_enable(1)
        ctx.prof_reset()
        for _ in range(args.repeat):
            segmap.labels_at(ctx, data, gamma, args.fwhm)
        kern = {k: round(v[0] / args.repeat, 4) for k, v in ctx.prof_report().items()
                if k.startswith("segmap")}
        ctx.prof_enable(0)
        doc["sizes"][str(N)] = dict(
            labels=int(nwant), identical=same, merged_identical=same_merged,
            segmap_host=host, segmap_device=dev, merged_host=host_m, merged_device=dev_m,
            kernels_ms_per_call=kern, kernels_ms_total=round(sum(kern.values()), 4))
    text = json.dumps(doc, indent=1)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
