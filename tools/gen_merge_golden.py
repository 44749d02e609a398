"""Generate tests/golden/g12_merging.npz from the reference's own functions.

    /opt/conda/bin/python3.9 tools/gen_merge_golden.py [--check]

Runs the reference's ``spatiospectral_merging`` and ``purity_estimation`` (loaded through
``oracle.ref_import.load_reference``, on ``astropy.table.Table`` s, with the recursion limit and
the thread stack raised: the recursion is as deep as a group is large) on the cases of
tests/_merge_oracle.py and writes inputs and outputs, the outputs re-ordered to input rows, as
int32 / float64.  Prints one OK / FAIL line per case comparing tests/_merge_oracle.py with the
reference.  The crowded one-component case goes into the fixture only when the reference
finishes it in under a minute.  ``--check``: compare with the committed file instead of writing.
"""
import argparse
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "g12_merging.npz")


def reference_merge(lib, case):
    from astropy.table import Table
    n = len(case["x"])
    tbl = Table(dict(x0=case["x"].astype(int), y0=case["y"].astype(int), z0=case["z"].astype(int),
                     area=case["area"].astype(int), row=np.arange(n)))
    out = lib.spatiospectral_merging(tbl, case["tol_spat"], case["tol_spec"])
    back = np.argsort(np.asarray(out["row"]), kind="stable")
    assert np.array_equal(np.asarray(out["row"])[back], np.arange(n))
    return {k: np.asarray(out[k])[back].astype(np.int64) for k in ("area", "imatch2", "imatch")}


def purity_case():
    rng = np.random.default_rng(12)
    n = 60
    comp = (rng.random(n) < 0.4).astype(int)
    tglr = np.where(comp == 0, rng.uniform(2, 14, n), np.nan)
    std = np.where(comp == 1, rng.uniform(-1, 9, n), np.nan)
    tglr[np.flatnonzero(comp == 0)[:2]] = [np.nan, 40.0]       # NaN in, far extrapolation
    std[np.flatnonzero(comp == 1)[:2]] = [-30.0, np.nan]
    tval = np.linspace(4, 12, 9)
    pval = np.clip(np.sort(rng.uniform(0.1, 1.0, 9)), 0, 1)
    tval_c = np.linspace(1, 7, 7)
    pval_c = np.clip(np.sort(rng.uniform(0.0, 1.0, 7)), 0, 1)
    return dict(comp=comp, T_GLR=tglr, STD=std, Tval=tval, Pval=pval, Tval_comp=tval_c,
                Pval_comp=pval_c)


def reference_purity(lib, p):
    from astropy.table import Table
    cat = Table(dict(comp=p["comp"], T_GLR=p["T_GLR"], STD=p["STD"]))
    out = lib.purity_estimation(cat, Table(dict(Tval_r=p["Tval"], Pval_r=p["Pval"])),
                                Table(dict(Tval_r=p["Tval_comp"], Pval_r=p["Pval_comp"])))
    return np.asarray(out["purity"], dtype=np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import _merge_oracle as oracle
    from oracle.ref_import import load_reference
    lib = load_reference()
    doc, names, ok_all = {}, [], True
    cases = oracle.golden_cases() + [oracle.case_crowded()]
    for case in cases:
        t0 = time.perf_counter()
        ref = reference_merge(lib, case)
        dt = time.perf_counter() - t0
        got = oracle.merge(case["x"], case["y"], case["z"], case["area"], case["tol_spat"],
                           case["tol_spec"])
        ok = all(np.array_equal(ref[k], got[k]) for k in ref)
        ok_all &= ok
        keep = case["name"] != "crowded" or dt < 60
        print(f"{'OK  ' if ok else 'FAIL'} {case['name']:<20} rows {len(case['x']):5d} groups "
              f"{len(np.unique(ref['imatch2'])):4d} -> {len(np.unique(ref['imatch'])):4d} "
              f"reference {dt:6.2f} s{'' if keep else '  (left out of the fixture)'}")
        if not keep:
            continue
        i = len(names)
        names.append(case["name"])
        for k in ("x", "y", "z", "area"):
            doc[f"c{i}_{k}"] = case[k].astype(np.int32)
        doc[f"c{i}_tol"] = np.array([case["tol_spat"], case["tol_spec"]], np.float64)
        doc[f"c{i}_shape"] = np.array(case["shape"], np.int32)
        for k, v in ref.items():
            doc[f"c{i}_out_{k}"] = v.astype(np.int32)
    p = purity_case()
    ref_p = reference_purity(lib, p)
    got_p = oracle.purity(p["comp"], p["T_GLR"], p["STD"], p["Tval"], p["Pval"], p["Tval_comp"],
                          p["Pval_comp"])
    ok = np.array_equal(np.isnan(ref_p), np.isnan(got_p)) and np.nanmax(np.abs(ref_p - got_p)) <= 1e-15
    ok_all &= bool(ok)
    print(f"{'OK  ' if ok else 'FAIL'} purity               rows {len(ref_p):5d} NaN {int(np.isnan(ref_p).sum())}")
    for k, v in p.items():
        doc[f"purity_{k}"] = np.asarray(v, np.int32 if k == "comp" else np.float64)
    doc["purity_out"] = ref_p
    doc["names"] = np.array(names)
    if args.check:
        old = np.load(OUT)
        same = sorted(old.files) == sorted(doc) and all(
            np.array_equal(old[k], doc[k], equal_nan=doc[k].dtype.kind == "f") for k in doc)
        print("fixture reproduced" if same else "fixture DIFFERS")
        ok_all &= same
    else:
        np.savez_compressed(OUT, **doc)
        print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.setrecursionlimit(100000)
    threading.stack_size(1 << 30)
    rc = []
    t = threading.Thread(target=lambda: rc.append(main()))
    t.start()
    t.join()
    sys.exit(rc[0] if rc else 2)
