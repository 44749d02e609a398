"""NumPy float64 restatement of the reference's line estimation (muse_origin/lib_origin.py:
estimation_line :1805-1938, GridAnalysis :1620-1790, method_PCA_wgt :1535-1617, LS_deconv_wgt
:1482-1510, conv_wgt :1513-1532, peakdet :1793-1801, DCTMAT :127-147), the oracle of
tests/test_lines.py.  tools/gen_line_golden.py pins it to the reference's own functions
(tests/golden/g11_lines.npz).

The leading singular vector comes from LAPACK (``np.linalg.svd``) where the reference runs ARPACK
(``svds(k=1)``).  Deviations, the ones origin_amd.lines documents:

* a window that holds a non-finite raw value, a var that is NaN or <= 0, or a channel whose
  ``sum psf^2 / var`` is 0 is *degenerate*: it takes no part in the grid (the reference hands NaN
  to ARPACK there);
* grid offsets outside the field do not compete (the reference leaves 0 / inf in their cells);
* the first best offset in ``np.where`` order wins a tie (the reference raises on ``int(y)``);
* a detection whose offsets are all degenerate, or whose criterion holds a NaN or is not finite at
  the winner, gets the fallback row of :1760-1769;
* weighted fields: ``size_grid == 0`` only.
"""
import numpy as np

FALLBACK_RESIDUAL = 1.0e6


def dctmat(nl, order):
    yy, xx = np.mgrid[:nl, : order + 1]
    D0 = np.sqrt(2 / nl) * np.cos((yy + 0.5) * (np.pi / nl) * xx)
    D0[:, 0] *= 1 / np.sqrt(2)
    return D0


def leading_left_vector(a):
    """First left singular vector of ``a`` (sign free), and the first two singular values."""
    U, s, _ = np.linalg.svd(a, full_matrices=False)
    return U[:, 0], s[:2]


def ls_deconv_wgt(data, var, psf):
    nl = psf.shape[0]
    var, psf, data = var.reshape(nl, -1), psf.reshape(nl, -1), data.reshape(nl, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        varest = 1 / np.sum(psf * psf / var, axis=1)
        deconv = np.sum(psf * data / np.sqrt(var), axis=1) * varest
    return deconv, varest


def conv_wgt(deconv, psf):
    return psf * deconv[:, None, None] * (np.abs(psf) > 0)


def method_pca_wgt(data, var, psf, order_dct, info=None):
    """``info`` (a dict) receives the singular-value ratios s2/s1 of the two decompositions."""
    nl = psf.shape[0]
    data_std = data / np.sqrt(var)
    ds = data_std.reshape(nl, -1)
    a = ds - ds.mean(axis=1)[:, None]
    u, s_a = leading_left_vector(a)
    residual = data_std - (u[:, None] * (u @ a)[None, :]).reshape(psf.shape)
    deconv, _ = ls_deconv_wgt(residual, var, psf)
    clean = ((data - conv_wgt(deconv, psf)) / np.sqrt(var)).reshape(nl, -1)
    clean = clean - clean.mean(axis=1)[:, None]
    u, s_b = leading_left_vector(clean)
    if order_dct is not None:
        D0 = dctmat(nl, order_dct)
        u = D0 @ (D0.T @ u)
    residual = data_std - (u[:, None] * (u @ ds)[None, :]).reshape(psf.shape)
    if info is not None:
        info.setdefault("sv_ratio", []).extend([s_a[1] / s_a[0], s_b[1] / s_b[0]])
    return ls_deconv_wgt(residual, var, psf)


def peakdet(v):
    ind = np.where((v[1:-1] > v[:-2]) & (v[1:-1] > v[2:]))[0] + 1
    imax = v.size // 2
    if len(ind) > 0:
        imax = ind[np.argmin((ind - imax) ** 2)]
    return int(imax)


def degenerate(data, var, psf, inside):
    """The flag of the device gather: ``inside`` marks the window pixels that lie in the field."""
    nl = psf.shape[0]
    d, v = data[:, inside], var[:, inside]
    if not np.all(np.isfinite(d)) or np.any(np.isnan(v)) or np.any(v <= 0):
        return True
    with np.errstate(divide="ignore", invalid="ignore"):
        return bool(np.any(np.sum((psf * psf / var).reshape(nl, -1), axis=1) == 0))


def window(cube, cy, cx, P, fill):
    """(Nz, P, P) window of ``cube`` centred on (cy, cx), ``fill`` outside the field, and the
    (P, P) mask of the pixels inside (overlap_slices + the fills of :1884-1888)."""
    Nz, Ny, Nx = cube.shape
    h = P // 2
    out = np.full((Nz, P, P), fill, dtype=float)
    inside = np.zeros((P, P), bool)
    ys, xs = np.arange(cy - h, cy + h + 1), np.arange(cx - h, cx + h + 1)
    oky, okx = (ys >= 0) & (ys < Ny), (xs >= 0) & (xs < Nx)
    sel = np.ix_(oky, okx)
    out[(slice(None),) + sel] = cube[:, ys[oky]][:, :, xs[okx]]
    inside[sel] = True
    return out, inside


def effective_psf(psf, weights, cy, cx, P):
    """psf for weights=None; else sum_n w_n[window] psf_n (:1713-1717), w_n = 0 outside the field."""
    if weights is None:
        return np.asarray(psf, float)
    out = None
    for w, p in zip(weights, psf):
        wwin = window(np.asarray(w, float)[None], cy, cx, P, 0.0)[0][0]
        term = wwin[None] * np.asarray(p, float)
        out = term if out is None else out + term
    return out


def grid_analysis(raw, var, psf, weights, y0, x0, z0, size_grid, criteria, order_dct, horiz_psf,
                  horiz, info=None):
    """One detection -> (flux5, mse5, line, var, y, x, z, fallback).  ``info`` receives the
    decision margins the GPU test asserts on: ``sv_ratio``, ``peak_margin`` (smallest relative
    neighbour difference inside the peakdet windows) and ``crit_gap`` (relative gap between the
    best and the second-best grid criterion)."""
    if criteria not in ("flux", "mse"):
        raise ValueError("Bad criteria: (flux) or (mse)")
    if weights is not None and size_grid > 0:
        raise ValueError("weighted fields are supported for size_grid == 0 only")
    Nz, Ny, Nx = raw.shape
    P = (psf if weights is None else psf[0]).shape[1]
    c = P // 2
    inds = slice(c - horiz_psf, c + 1 + horiz_psf)
    ind_max = slice(max(0, z0 - 5), min(Nz, z0 + 6))
    cands = []
    for dy in range(-size_grid, size_grid + 1):
        for dx in range(-size_grid, size_grid + 1):
            cy, cx = y0 + dy, x0 + dx
            if not (0 <= cy < Ny and 0 <= cx < Nx):
                continue
            r1, inside = window(raw, cy, cx, P, 0.0)
            v1, _ = window(var, cy, cx, P, np.inf)
            ps = effective_psf(psf, weights, cy, cx, P)
            if degenerate(r1, v1, ps, inside):
                continue
            line, lvar = method_pca_wgt(r1, v1, ps, order_dct, info)
            v = line[ind_max]
            if info is not None and v.size > 1:
                info.setdefault("peak_margin", []).append(
                    float(np.min(np.abs(np.diff(v))) / np.max(np.abs(v))))
            maxz = z0 - 5 + peakdet(v)
            ind_hrz = slice(maxz - horiz, maxz + horiz + 1)
            ind_z5 = np.arange(max(0, maxz - 5), min(maxz + 6, Nz))

            def mse_over(idx):
                LC = conv_wgt(line[idx], ps[idx])[:, inds, inds]
                r = r1[idx][:, inds, inds]
                with np.errstate(divide="ignore", invalid="ignore"):
                    return np.sum((r - LC) ** 2) / np.sum(r ** 2)

            crit = float(np.sum(line[ind_hrz])) if criteria == "flux" else float(mse_over(ind_hrz))
            cands.append(dict(crit=crit, flux5=float(np.sum(line[ind_z5])),
                              mse5=float(mse_over(ind_z5)), line=line, var=lvar, y=cy, x=cx,
                              z=int(maxz)))
    fallback = (0.0, FALLBACK_RESIDUAL, np.zeros(1), np.zeros(1), int(y0), int(x0), int(z0), True)
    if not cands:
        return fallback
    crits = np.array([k["crit"] for k in cands])
    if np.any(np.isnan(crits)):
        return fallback
    best = int(np.argmax(crits) if criteria == "flux" else np.argmin(crits))
    if not np.isfinite(crits[best]):
        return fallback
    if info is not None and len(crits) > 1:
        others = np.delete(crits, best)
        near = others.max() if criteria == "flux" else others.min()
        info.setdefault("crit_gap", []).append(float(abs(crits[best] - near) / abs(crits[best])))
    k = cands[best]
    return k["flux5"], k["mse5"], k["line"], k["var"], k["y"], k["x"], k["z"], False


def estimate_lines(raw, var, psf, weights, z0, y0, x0, size_grid=0, criteria="flux", order_dct=30,
                   horiz_psf=1, horiz=5, info=None):
    """All detections -> dict of flux, residual, y, x, z, fallback (arrays) and line, var (lists)."""
    raw, var = np.asarray(raw, float), np.asarray(var, float)
    rows = [grid_analysis(raw, var, psf, weights, int(y), int(x), int(z), size_grid, criteria,
                          order_dct, horiz_psf, horiz, info) for z, y, x in zip(z0, y0, x0)]
    flux, res, line, lvar, y, x, z, fb = zip(*rows) if rows else ([],) * 8
    return dict(flux=np.array(flux, float), residual=np.array(res, float), line=list(line),
                var=list(lvar), y=np.array(y, int), x=np.array(x, int), z=np.array(z, int),
                fallback=np.array(fb, bool))
