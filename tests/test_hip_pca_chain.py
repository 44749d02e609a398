"""GPU tests of the greedy PCA's per-iteration chain (csrc/pca.hip: pca_select_fast_kernel /
pca_select_kernel, cbar_kernel, bmean_kernel, gather_xp_kernel, project_xp_kernel, xv_kernel,
uw_partial_kernel, normalize_kernel, deflate_dot_kernel / deflate_dot_rows_kernel,
deflate_finish_kernel, flush_kernel) against the stepwise float64 restatement of
tests/_pca_chain_oracle.py, after EVERY iteration: ``pipeline.greedy_pca(..., itermax=t)`` for every
checkpoint t of every case of tests/test_pca_chain_cases.py (which names, per case, the branch of
the launch arithmetic it is aimed at and checks on the CPU that the input is decidable).

Per checkpoint:
  * mapO2 and nstop equal the restatement's; ``drv.trace`` equals the restated [(nw, sum n)];
  * t = 0: F is bit for bit X; at every t the spaxels outside all areas and the areas that have
    not removed a vector yet are bit for bit X;
  * |got - F_ref|[z, s] <= 0.5 ulp32(max(|got|, |F_ref|)) + E[s],
    E[s] = T_s * 2 rho / gamma * ||X[:, s]||_2: flush_kernel forms X - U C in float64 and rounds
    once (half an ulp); each of the T_s removed vectors of s's area is the leading eigenvector of
    its Gram matrix to a residual rho = 1e-11 (what test_hip_pca_batches.py asserts of the
    solvers), i.e. within 2 rho / gamma of the true one when gamma is the smallest relative eigen
    gap of the area so far, and moves a column by at most that angle times its norm.  A flush in
    mid-run (case E) rounded the cube once before: + 0.5 sqrt(Nz) ulp32(max_z |X[:, s]|) per such
    flush (a projection cannot grow the 2-norm of that rounding).
  * the geometry the case aims at holds for this device's CU count.

Largest |d| / tol seen per case on the MI355X (256 CUs), t over all checkpoints:
  A 0.999 (per Nz and field 0.982 ... 0.999), B 0.998, C 0.998, D 0.996 / 0.998 / 0.998,
  E 0.997 (0.138 at t = 65, 66, where the term of the mid-run flush dominates), F 0.999 / 0.999:
  the half ulp of flush_kernel's single rounding is all a correct run uses (max |d| 4e-7 ... 4e-6);
  E[s] adds 1e-9 ... 1e-6 of it, except behind E's mid-run flush.
"""
import numpy as np
import pytest

import _pca_chain_oracle as orc
import test_pca_chain_cases as cases
from _gram_geometry import num_cu_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from origin_amd.device import default_context
    return default_context(0)


def run_device(ctx, c, t):
    """pipeline.greedy_pca with itermax = t on a fresh upload of the case's cube.  Out of place the
    output buffer starts as 0x7f bytes, so whatever the run does not write shows."""
    from origin_amd import pipeline
    d = ctx.to_device(np.ascontiguousarray(c.X.reshape((c.Nz,) + c.shape)))
    out = None
    if not c.inplace:
        out = ctx.empty(d.shape, np.float32)
        out.fill_bytes(0x7f)
    F, mapO2, nstop, drv = pipeline.greedy_pca(ctx, d, c.areamap, c.nb, c.thr, c.tests,
                                               c.noise_pop, t, inplace=c.inplace, out=out)
    return F.to_host().reshape(c.Nz, c.S), mapO2.reshape(-1), nstop, drv.trace


@pytest.mark.parametrize("cid", cases.CASE_IDS)
def test_chain_after_every_iteration(ctx, cid):
    c = cases.case(cid)
    cases.check_aim(cid, num_cu_of(ctx))
    worst = (0.0, None)
    for t in c.checkpoints:
        got, mapO2, nstop, trace = run_device(ctx, c, t)
        r, E, untouched = c.bound(t)
        assert nstop == r.nstop, (cid, t, nstop, r.nstop)
        assert np.array_equal(mapO2, r.mapO2), (cid, t, np.flatnonzero(mapO2 != r.mapO2)[:8])
        assert [tuple(map(int, e)) for e in trace] == orc.device_trace(c.records, t), (cid, t, trace)
        if t == 0:
            assert not untouched.size or untouched.all()
            assert nstop == sum(s is not None for s in r.steps)
        assert np.array_equal(got[:, untouched], c.X[:, untouched]), (cid, t)
        d = np.abs(got.astype(np.float64) - r.F)
        tol = 0.5 * orc.ulp32(np.maximum(np.abs(got), np.abs(r.F))) + E[None, :]
        ratio = float(np.max(d / tol))
        if ratio > worst[0]:
            z, s = np.unravel_index(np.argmax(d / tol), d.shape)
            worst = (ratio, (t, int(z), int(s), float(d[z, s]), float(tol[z, s])))
        print(f"{cid} t={t}: max|d|/tol {ratio:.3f} max|d| {d.max():.3e} nstop {nstop} "
              f"trace {trace[-1] if trace else None}")
        assert ratio <= 1.0, (cid, t, worst)
    print(f"{cid}: largest |d|/tol {worst[0]:.3f} at (t, z, s, |d|, tol) = {worst[1]}")
