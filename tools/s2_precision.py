"""Host emulation of the matrix-core spatial stage's two-term f16 split (csrc/glr_spatial_mfma.hip)
against float64, per PSF size: taps of the mean-subtracted Moffat PSF of synth.moffat_psf times
2^S2_TAP_LOG2 split into f16 hi + lo as the table build does, the tile scaled by the power of two
that puts max |x| in [2^14, 2^15) and split the same way, the three products hi*hi + hi*lo + lo*hi.

    python tools/s2_precision.py [--p 25,27,...,41] [--tap-log2 12]

Prints per P: the smallest |tap| and |lo tap| (subnormal f16 below 6.1e-5), the share of lo taps
that are f16 subnormal, and the worst error of cube_fsf relative to sum |psf| |x| (the bound the
GLR's fp32-class statement uses) and the worst absolute error of a unit-noise channel, whose
GLR T is a ratio of such sums: |dT| of the whole test scales with the relative error."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from origin_amd import synth  # noqa: E402


def split16(v):
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def corr2_same(img, k):
    P = k.shape[0]
    c = P // 2
    H, W = img.shape
    pad = np.zeros((H + P - 1, W + P - 1))
    pad[c:c + H, c:c + W] = img
    out = np.zeros((H, W))
    for dy in range(P):
        for dx in range(P):
            out += k[dy, dx] * pad[dy:dy + H, dx:dx + W]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", default="25,27,29,31,33,35,37,39,41")
    ap.add_argument("--tap-log2", type=int, default=12)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    print("   P  min|tap|  min|lo|   lo subnormal  max rel err   max abs err (unit noise)")
    for P in [int(v) for v in a.p.split(",")]:
        psf = synth.moffat_psf(3681, P)[[0, 1840, 3680]].astype(np.float64)
        worst_rel = worst_abs = 0.0
        min_tap = min_lo = np.inf
        sub = 0.0
        for k in psf:
            k = (k - k.mean()).astype(np.float32)
            kh, kl = split16(k * np.float32(2.0 ** a.tap_log2))
            nz = kl != 0
            min_tap = min(min_tap, np.abs(k).min())
            min_lo = min(min_lo, np.abs(kl[nz]).min() if nz.any() else np.inf)
            sub = max(sub, np.mean(np.abs(kl) < 6.103515625e-05))
            x = rng.standard_normal((64 + P - 1, 64 + P - 1)).astype(np.float32)
            x[10, 10] += 40.0
            ex = int(np.frexp(np.abs(x).max())[1]) - 1        # max |x| in [2^ex, 2^(ex+1))
            y = (x * np.float32(2.0 ** (14 - ex))).astype(np.float32)
            yh, yl = split16(y)
            kf = k.astype(np.float64)
            ref = corr2_same(x.astype(np.float64), kf)
            got = (corr2_same(yh, kh) + corr2_same(yl, kh) + corr2_same(yh, kl)) * 2.0 ** (
                ex - 14 - a.tap_log2)
            bound = corr2_same(np.abs(x.astype(np.float64)), np.abs(kf))
            worst_rel = max(worst_rel, np.max(np.abs(got - ref) / bound))
            worst_abs = max(worst_abs, np.max(np.abs(got - ref)))
        print(f"{P:4d}  {min_tap:.2e}  {min_lo:.2e}  {100 * sub:9.1f} %   {worst_rel:.2e}     "
              f"{worst_abs:.2e}")


if __name__ == "__main__":
    main()
