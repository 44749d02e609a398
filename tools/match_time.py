"""Time the matching of point lists (origin_amd/match.py, csrc/match.hip) next to the host
cKDTree form of the same inputs, on one MI355X.

    python tools/match_time.py [--size 200] [--nz 3681] [--repeat 3] [--out profiles/match_time.json]

The field is the benchmark's synthetic one (``synth.SyntheticField`` with bench.py's densities) at
``--size`` spaxels a side; steps 1-6 of a session give the local-maximum cubes and the two
thresholds.  Two consumers are timed, each against SciPy on the same machine and the same inputs:

* ``true_purity``: ``match.true_purity`` on the session's ``cube_local_max`` with the injected
  emitters as reference lines (``threshmin`` 4, ``threshmax`` 7, ``maxdist`` 4.5), split into the
  compaction (``cubes.where_above``) and the match.  The host baseline is the reference's loop
  (lib_origin.py:2390-2400: 30 thresholds, a cKDTree over the candidates above each, matched with
  the tree of the lines).  It STARTS FROM THE CANDIDATE LIST the device compaction delivered, not
  from a dense float64 host cube: the reference's ``np.where`` over 10.6 GB at 3681 x 600 x 600,
  and the copy of the cube to the host, are not in it.
* step 7's std match: ``match.ball_match`` on the std and correl detections above the session's
  thresholds against ``detection.unmatched_std`` (two cKDTrees, steps.py:983-992).

Each time is the best of ``--repeat`` wall times, host conversions and copies included; the event
profiler's split of the two kernel classes comes from one more, untimed call.  Both pairs of
results are compared for equality and the outcome recorded.  Needs a GPU; prints one JSON
document and writes it to ``--out``.  No time here is a pass / fail condition.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best_of(repeat, fn):
    best, out = None, None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best * 1e3, out


def host_true_purity(w, ref_xyz, nref, maxdist, threshmin, threshmax):
    """lib_origin.py:2383-2403 from the candidate list ``w`` (x, y, z, value)."""
    from scipy.spatial import cKDTree
    kdref = cKDTree(np.array(ref_xyz, dtype=np.float64).T)
    T = w["value"]
    rows = []
    for thr in np.arange(threshmin, threshmax, 0.1):
        sel = T > thr
        ndetect = int(sel.sum())
        lists = []
        if ndetect:
            kdt = cKDTree(np.array([w["x"][sel], w["y"][sel], w["z"][sel]]).T)
            lists = [lst for lst in kdt.query_ball_tree(kdref, maxdist) if lst]
        found = set()
        for lst in lists:
            found.update(lst)
        rows.append((thr, ndetect, len(lists), ndetect - len(lists), nref - len(found)))
    return {k: np.array([r[i] for r in rows]) for i, k in
            enumerate(("thresh", "ndetect", "ntrue", "nfalse", "nmiss"))}


def kernel_split(ctx, fn):
    ctx.prof_enable(1)
    ctx.prof_reset()
    fn()
    prof = ctx.prof_report()
    ctx.prof_enable(0)
    return {k: round(v[0], 3) for k, v in sorted(prof.items()) if k.startswith("match_")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=200)
    ap.add_argument("--nz", type=int, default=3681)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from origin_amd import cubes, detection, match, synth
    from origin_amd.device import default_context
    from origin_amd.steps import SimpleOrig

    ctx = default_context(0)
    n = args.size
    t0 = time.perf_counter()
    f = synth.SyntheticField(args.nz, n, n, None, 25, 20, 0, 1.0 / 400, 1.0 / 900, 100)
    raw, var, mask = f.arrays()
    t_gen = time.perf_counter() - t0
    orig = SimpleOrig(raw, var, mask, f.PSF.astype(np.float64), f.profiles, ctx=ctx)
    orig.step01_preprocessing()
    orig.step02_areas.set_areamap(f.areamap)
    orig.step03_compute_PCA_threshold()
    orig.step04_compute_greedy_PCA()
    orig.step05_compute_TGLR()
    orig.step06_compute_purity_threshold()
    t_steps = time.perf_counter() - t0 - t_gen
    lmax = cubes.session_cube(orig, "cube_local_max")
    smax = cubes.session_cube(orig, "cube_std_local_max")
    doc = dict(device=ctx.name, shape=[args.nz, n, n], field_seconds=round(t_gen, 1),
               steps_1_to_6_seconds=round(t_steps, 1), repeat=args.repeat,
               host_baseline="scipy.spatial.cKDTree on this machine; the true-purity loop starts "
                             "from the candidate list of the device compaction, not from a dense "
                             "float64 host cube")

    # ---- true purity against the injected emitters
    ref = (f.em_x.astype(np.float64), f.em_y.astype(np.float64), f.em_z.astype(np.float64))
    nref = len(f.em_x)
    maxdist, tmin, tmax = 4.5, 4, 7
    match.true_purity(ctx, lmax, ref, nref, maxdist, tmin, tmax)       # code objects, allocator
    ms_where, w = best_of(args.repeat, lambda: cubes.where_above(lmax, tmin))
    cand = (w["x"], w["y"], w["z"])
    ms_match, _ = best_of(args.repeat, lambda: match.ball_match(ctx, cand, ref, maxdist,
                                                                a_val=w["value"]))
    ms_all, tbl = best_of(args.repeat, lambda: match.true_purity(ctx, lmax, ref, nref, maxdist,
                                                                 tmin, tmax))
    ms_host, ref_tbl = best_of(args.repeat,
                               lambda: host_true_purity(w, ref, nref, maxdist, tmin, tmax))
    doc["true_purity"] = dict(
        candidates_above_threshmin=int(w["z"].size), reference_lines=nref, maxdist=maxdist,
        threshmin=tmin, threshmax=tmax, thresholds=int(tbl["thresh"].size),
        device_ms=dict(where_above=round(ms_where, 3), ball_match=round(ms_match, 3),
                       true_purity_total=round(ms_all, 3)),
        kernel_ms=kernel_split(ctx, lambda: match.ball_match(ctx, cand, ref, maxdist,
                                                             a_val=w["value"])),
        host_ckdtree_30_trees_ms=round(ms_host, 1),
        tables_equal=bool(all(np.array_equal(tbl[k], ref_tbl[k]) for k in ref_tbl)),
        ndetect=[int(tbl["ndetect"][0]), int(tbl["ndetect"][-1])],
        ntrue=[int(tbl["ntrue"][0]), int(tbl["ntrue"][-1])],
        nmiss=[int(tbl["nmiss"][0]), int(tbl["nmiss"][-1])])
    _save(doc, args.out)

    # ---- step 7's std match at the session's thresholds
    thr, thr_std = orig.param["threshold"], orig.param["threshold_std"]
    source = "step 6 (purity 0.9)"
    if not (np.isfinite(thr) and np.isfinite(thr_std)):
        # the purity curve of a small field may not reach 0.9: thresholds that keep the 0.01 %
        # highest voxels of each cube instead
        source = "the 1e-4 quantile of each cube's voxels (step 6 gave no finite threshold)"
        thr, thr_std = (_quantile_threshold(c) for c in (lmax, smax))
    c = cubes.where_above(lmax, thr)
    s = cubes.where_above(smax, thr_std)
    cat = dict(x0=c["x"], y0=c["y"], z0=c["z"])
    cat_std = dict(x0=s["x"], y0=s["y"], z0=s["z"])
    a, b = (s["x"], s["y"], s["z"]), (c["x"], c["y"], c["z"])
    only_a = dict(want=("a_hit",))                     # what threshold_detections asks for
    match.ball_match(ctx, a, b, 2.5, **only_a)
    ms_dev, hit = best_of(args.repeat, lambda: match.ball_match(ctx, a, b, 2.5, **only_a)["a_hit"])
    ms_host, keep = best_of(args.repeat, lambda: detection.unmatched_std(cat, cat_std, 2.5))
    doc["step7_std_match"] = dict(
        thresholds=dict(correl=float(thr), std=float(thr_std), source=source),
        correl_detections=int(c["z"].size), std_detections=int(s["z"].size),
        std_kept=int(len(keep)), maxdist_lines=2.5, device_ms=round(ms_dev, 3),
        kernel_ms=kernel_split(ctx, lambda: match.ball_match(ctx, a, b, 2.5, **only_a)),
        host_ckdtree_ms=round(ms_host, 3),
        rows_equal=bool(np.array_equal(np.flatnonzero(~hit), keep)))
    print(_save(doc, args.out))


def _quantile_threshold(cube):
    from origin_amd import cubes
    grid = np.linspace(2.0, 40.0, 400)
    counts = cubes.count_above(cube, grid)
    want = max(int(1e-4 * np.prod(cube.shape)), 10)
    return float(grid[min(int(np.searchsorted(-counts, -want)), grid.size - 1)])


def _save(doc, out):
    text = json.dumps(doc, indent=1)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")
    return text


if __name__ == "__main__":
    main()
