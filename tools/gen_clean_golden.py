"""Generate tests/golden/g13_clean.npz from the reference's own step-9 functions.

    /opt/conda/bin/python3.9 tools/gen_clean_golden.py [--check]

Runs the reference's ``merge_similar_lines``, ``unique_sources`` and ``add_tglr_stat`` (loaded
through ``oracle.ref_import.load_reference``, on ``astropy.table.Table`` s) on the hand-made and
random line tables below, at ``z_pix_threshold`` 5 and 3, with two small float64 cubes for the
two ``np.std`` calls, and writes the inputs and the reference's outputs: integer columns as
int64, floats as float64, bools as bool, strings and column-name lists as fixed-width bytes.
All fluxes of a table are distinct and non-zero, so the reference itself is well defined
(except for the order of rows with equal ``(ID, z)``: the tests compare after ordering by
``(ID, z, num_line)``).  This file only generates: the package never imports it.
``--check``: compare with the committed file instead of writing (``CAT3_TS`` is not stored).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "g13_clean.npz")
THRESHOLDS = (5, 3)
INPUT_COLUMNS = ("ID", "ra", "dec", "lbda", "x", "y", "z", "comp", "STD", "T_GLR", "seg_label",
                 "purity", "flux", "num_line")

# name -> rows (ID, z, comp); fluxes, positions and statistics are drawn per row below
HAND_CASES = {
    "one_row": [(1, 10, 0)],
    "single_line_source": [(1, 10, 0), (2, 40, 0), (2, 90, 0)],
    "pair_gap_below_and_at_threshold": [(3, 10, 0), (3, 14, 0), (5, 20, 0), (5, 25, 0),
                                        (6, 30, 0), (6, 32, 0), (7, 40, 0), (7, 43, 0)],
    "percolating_chain": [(8, 0, 0), (8, 4, 0), (8, 8, 0)],
    "two_runs_in_one_source": [(9, 100, 0), (9, 102, 0), (9, 300, 0), (9, 303, 0), (9, 304, 0),
                               (9, 200, 0)],
    "five_unmerged_lines": [(12, 10, 0), (12, 100, 0), (12, 200, 0), (12, 300, 0), (12, 400, 0)],
    "comp1_source": [(13, 50, 1), (13, 52, 1), (13, 150, 1)],
    "mixed_comp_source": [(17, 60, 0), (17, 61, 1), (17, 260, 0), (18, 5, 0)],
    "equal_z": [(20, 50, 0), (20, 50, 0), (21, 7, 0)],
    "non_contiguous_ids": [(40, 10, 0), (3, 11, 0), (40, 12, 1), (1000, 13, 0), (3, 300, 0),
                           (7, 1, 1)],
}


def make_table(rows, seed):
    """Input columns for ``rows`` = [(ID, z, comp)], in a shuffled row order."""
    rng = np.random.default_rng(seed)
    rows = [rows[i] for i in rng.permutation(len(rows))]
    n = len(rows)
    ids = np.array([r[0] for r in rows], dtype=np.int64)
    z = np.array([r[1] for r in rows], dtype=np.int64)
    comp = np.array([r[2] for r in rows], dtype=np.int64)
    # distinct, non-zero fluxes: a permutation of a strictly increasing sequence
    flux = (1.0 + np.cumsum(rng.uniform(0.05, 3.0, n)))[rng.permutation(n)]
    stat = rng.uniform(3.0, 40.0, n)
    return dict(
        ID=ids, ra=53.1 + rng.uniform(-0.01, 0.01, n), dec=-27.8 + rng.uniform(-0.01, 0.01, n),
        lbda=4750.0 + 1.25 * z + rng.uniform(0, 1.2, n), x=rng.integers(0, 300, n).astype(np.int64),
        y=rng.integers(0, 300, n).astype(np.int64), z=z, comp=comp,
        STD=np.where(comp == 1, stat, np.nan), T_GLR=np.where(comp == 0, stat, np.nan),
        seg_label=(ids * 7 % 11).astype(np.int64), purity=rng.uniform(0.5, 1.0, n), flux=flux,
        num_line=np.arange(1, n + 1, dtype=np.int64))


def random_rows(seed=13, n=300, nid=60):
    """About ``n`` rows over ``nid`` sources with unique ``(ID, z)`` pairs: which of two rows with
    equal ``(ID, z)`` the reference's sort puts first is open, and ``unique_sources`` takes
    ``comp`` from a source's first row (the ``equal_z`` case has such rows, with one ``comp``)."""
    rng = np.random.default_rng(seed)
    ids = rng.choice(np.arange(1, 4 * nid), nid, replace=False)
    centres = rng.integers(0, 400, (nid, 3))
    m = n + n // 4
    who = rng.integers(0, nid, m)
    z = np.clip(centres[who, rng.integers(0, 3, m)] + rng.integers(-6, 7, m), 0, 420)
    comp = (rng.random(m) < 0.25).astype(int)
    rows, seen = [], set()
    for w, zz, c in zip(who, z, comp):
        if (int(w), int(zz)) not in seen and len(rows) < n:
            seen.add((int(w), int(zz)))
            rows.append((int(ids[w]), int(zz), int(c)))
    assert len(rows) == n and len({r[0] for r in rows}) == nid
    return rows


def cases():
    out = [(name, make_table(rows, seed=100 + i)) for i, (name, rows) in
           enumerate(HAND_CASES.items())]
    out.append(("random_300", make_table(random_rows(), seed=7)))
    return out


def cubes():
    rng = np.random.default_rng(99)
    correl = rng.normal(0.3, 2.5, (7, 5, 6))
    std = rng.normal(1000.0, 1.0, (6, 4, 5))
    return correl, std


def store(col):
    col = np.asarray(col)
    if col.dtype.kind in "US":
        return col.astype("S")
    if col.dtype.kind == "b":
        return col.astype(bool)
    if col.dtype.kind in "iu":
        return col.astype(np.int64)
    return col.astype(np.float64)


def reference(lib, tab, thr, correl, std):
    from astropy.table import Table
    t = Table({k: tab[k] for k in INPUT_COLUMNS}, names=INPUT_COLUMNS)
    lines = lib.merge_similar_lines(t, z_pix_threshold=thr)
    src = lib.unique_sources(lines)
    src = lib.add_tglr_stat(src, lines, correl, std)
    assert "CAT3_TS" in lines.meta
    return lines, src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    from oracle.ref_import import load_reference
    lib = load_reference()
    correl, std = cubes()
    doc = dict(cube_correl=correl, cube_std=std, thresholds=np.array(THRESHOLDS, np.int64),
               input_columns=np.array(INPUT_COLUMNS, dtype="S"))
    names = []
    for i, (name, tab) in enumerate(cases()):
        names.append(name)
        for k in INPUT_COLUMNS:
            doc[f"c{i}_in_{k}"] = store(tab[k])
        for thr in THRESHOLDS:
            lines, src = reference(lib, tab, thr, correl, std)
            for tag, t in (("lines", lines), ("src", src)):
                doc[f"c{i}_t{thr}_{tag}_columns"] = np.array(t.colnames, dtype="S")
                for k in t.colnames:
                    doc[f"c{i}_t{thr}_{tag}_{k}"] = store(t[k])
            print(f"{name:<34} thr {thr}: {len(lines):4d} lines, {len(src):3d} sources, "
                  f"{int(np.sum(np.asarray(lines['merged_in']) != -9999)):3d} merged")
    doc["names"] = np.array(names, dtype="S")
    if args.check:
        old = np.load(OUT)
        same = sorted(old.files) == sorted(doc) and all(
            np.array_equal(old[k], doc[k], equal_nan=np.asarray(doc[k]).dtype.kind == "f")
            for k in doc)
        print("fixture reproduced" if same else "fixture DIFFERS")
        return 0 if same else 1
    np.savez_compressed(OUT, **doc)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
