"""Generate tests/golden/g14_segmap.npz from the reference's own ``compute_segmap_gauss``.

    /opt/conda/bin/python3.9 tools/gen_segmap_golden.py [--check]

The reference function (lib_origin.py:243-280) is loaded through
``oracle.ref_import.load_reference`` and called on three seeded maps (positive noise plus Gaussian
blobs, several of them on the borders); inputs, ``pfa``, ``fwhm_fsf``, ``gamma`` and the labels go
into the fixture.  The script asserts what keeps the tests on it from passing vacuously or hiding a
flipped pixel: no pixel within 1e-6 |gamma| of gamma, at least 5 labels per case, a component on
each of the four borders.  ``--check``: compare with the committed file instead of writing.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "g14_segmap.npz")

#        name  (Ny, Nx)    seed  pfa    fwhm_fsf
CASES = (("a", (96, 128), 141, 0.01, 0),
         ("b", (80, 100), 142, 0.01, 3),
         ("c", (64, 96), 143, 1e-5, 4))


def make_map(shape, seed):
    """Mean of 40 squared normals per pixel (an O2-like positive map) plus Gaussian blobs: one on
    every border, one in a corner, the rest anywhere."""
    rng = np.random.default_rng(seed)
    Ny, Nx = shape
    data = (rng.standard_normal((40, Ny, Nx)) ** 2).mean(axis=0)
    yy, xx = np.mgrid[:Ny, :Nx]
    centres = [(0, Nx // 3), (Ny - 1, 2 * Nx // 3), (Ny // 2, 0), (Ny // 3, Nx - 1), (0, 0)]
    centres += [(int(rng.integers(5, Ny - 5)), int(rng.integers(5, Nx - 5))) for _ in range(9)]
    for cy, cx in centres:
        sig, amp = rng.uniform(1.2, 3.0), rng.uniform(2.0, 6.0)
        data += amp * np.exp(-0.5 * ((yy - cy) ** 2 + (xx - cx) ** 2) / sig ** 2)
    return data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    from oracle.ref_import import load_reference
    lib = load_reference()
    doc = {}
    for name, shape, seed, pfa, fwhm in CASES:
        data = make_map(shape, seed)
        gamma, labels = lib.compute_segmap_gauss(data, pfa, fwhm_fsf=fwhm)
        labels = np.asarray(labels)
        n = int(labels.max())
        assert np.min(np.abs(data - gamma)) > 1e-6 * abs(gamma), f"{name}: a pixel sits on gamma"
        assert n >= 5, f"{name}: only {n} labels"
        for edge in (labels[0], labels[-1], labels[:, 0], labels[:, -1]):
            assert edge.any(), f"{name}: no component on one of the borders"
        print(f"case {name}: {shape} pfa {pfa} fwhm_fsf {fwhm} gamma {gamma:.6f} labels {n}")
        doc.update({f"{name}_data": data, f"{name}_pfa": np.float64(pfa),
                    f"{name}_fwhm_fsf": np.int64(fwhm), f"{name}_gamma": np.float64(gamma),
                    f"{name}_labels": labels.astype(np.int32)})
    if args.check:
        with np.load(OUT) as g:
            for k, v in doc.items():
                assert np.array_equal(g[k], v), k
        print("matches", OUT)
        return
    np.savez_compressed(OUT, **doc)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
