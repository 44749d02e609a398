"""Regenerate tests/golden/g11_lines.npz: the reference's own ``GridAnalysis`` /
``method_PCA_wgt`` (muse_origin/lib_origin.py, imported unmodified) on a handful of small cases,
next to the float64 restatement of tests/_line_oracle.py on the same inputs.

    python tools/gen_line_golden.py [--reference DIR]

``lib_origin.py`` is imported as oracle/ref_import.py does it (a package directory in a temporary
directory that links to the reference file), with inert stand-ins for the packages it imports at
module level and that are not installed (astropy, mpdaf, photutils; matplotlib if absent): every
name of a stand-in raises when it is called.  The line estimation calls none of them; it runs on
the installed NumPy / SciPy (ARPACK ``svds``).

Per case the fixture holds the inputs (float32-representable raw / var / PSF / weights, the
detection, the parameters), the reference's outputs, and ``dist``: the distance between the
reference (ARPACK) and the restatement (LAPACK) as max|d line| / max|line| and max|d var| /
max|var|.  tests/test_lines.py derives its tolerances from ``dist``.
"""
import argparse
import importlib
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "g11_lines.npz")

_STUB = '''\
class _Missing:
    """Inert stand-in: importable, raises when used."""
    def __init__(self, name):
        self._name = name
    def __call__(self, *a, **kw):
        raise RuntimeError(self._name + " stand-in: not on the path of the line estimation")
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Missing(self._name + "." + name)
    def __mul__(self, other):
        return self
    __rmul__ = __truediv__ = __rtruediv__ = __mul__

class AstropyUserWarning(UserWarning):
    pass

def __getattr__(name):
    if name.startswith("__"):
        raise AttributeError(name)
    return _Missing(__name__ + "." + name)
'''

# packages (with the sub-modules lib_origin.py / source_masks.py import from) to stand in for
_PACKAGES = {
    "astropy": ["modeling", "modeling.fitting", "modeling.models", "nddata", "stats", "table",
                "utils", "utils.exceptions", "units"],
    "mpdaf": ["obj", "tools"],
    "photutils": [],
    "matplotlib": ["pyplot"],
}


def _installed(name):
    try:
        importlib.import_module(name)
        return True
    except ImportError:
        return False


def load_reference(reference):
    root = tempfile.mkdtemp(prefix="origin_line_golden_")
    mo = os.path.join(root, "muse_origin")
    os.makedirs(mo)
    open(os.path.join(mo, "__init__.py"), "w").close()
    for name in ("lib_origin.py", "source_masks.py"):
        os.symlink(os.path.join(reference, "muse_origin", name), os.path.join(mo, name))
    for pkg, subs in _PACKAGES.items():
        if _installed(pkg):
            continue
        for mod in [""] + subs:
            d = os.path.join(root, pkg, *mod.split(".")) if mod else os.path.join(root, pkg)
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, "__init__.py"), "w") as f:
                f.write(_STUB)
    sys.path.insert(0, root)
    if _installed("matplotlib"):
        import matplotlib
        matplotlib.use("Agg")
    return importlib.import_module("muse_origin.lib_origin")


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def gaussian_psf(Nz, P, fwhm0=2.6, fwhm1=2.0):
    yy, xx = np.mgrid[:P, :P] - P // 2
    out = np.empty((Nz, P, P))
    for z in range(Nz):
        s = (fwhm0 + (fwhm1 - fwhm0) * z / max(Nz - 1, 1)) / 2.355
        g = np.exp(-(yy ** 2 + xx ** 2) / (2 * s * s))
        out[z] = g / g.sum()
    return f32(out)


def make_case(seed, Nz, Ny, Nx, P, y0, x0, z0, size_grid, criteria, order_dct, shift=(0, 0),
              nfields=0):
    """A noise field with a continuum source and an emission line under the detection (the line
    ``shift`` pixels off the catalogue position)."""
    rng = np.random.default_rng(seed)
    psf = gaussian_psf(Nz, P)
    var = f32(rng.uniform(0.8, 1.3, (Nz, Ny, Nx)))
    raw = rng.standard_normal((Nz, Ny, Nx)) * np.sqrt(var)
    h = P // 2
    cont = 6.0 * (1 + 0.4 * np.sin(np.arange(Nz) / 9.0))
    line = 40.0 * np.exp(-0.5 * ((np.arange(Nz) - z0) / 1.6) ** 2)
    for spec, (cy, cx) in ((cont, (y0, x0)), (line, (y0 + shift[0], x0 + shift[1]))):
        for iy in range(P):
            for ix in range(P):
                y, x = cy - h + iy, cx - h + ix
                if 0 <= y < Ny and 0 <= x < Nx:
                    raw[:, y, x] += spec * psf[:, iy, ix] * 12
    raw = f32(raw)
    weights = None
    if nfields:
        ramp = np.linspace(0.2, 0.8, Nx)[None, :] * np.ones((Ny, 1))
        weights = [f32(ramp), f32(1 - ramp)][:nfields]
        psf = [psf, gaussian_psf(Nz, P, 3.0, 2.4)][:nfields]
    return dict(raw=raw, var=var, psf=psf, weights=weights, det=(z0, y0, x0),
                size_grid=size_grid, criteria=criteria, order_dct=order_dct, horiz_psf=1, horiz=5)


CASES = [
    dict(seed=1, Nz=67, Ny=12, Nx=13, P=5, y0=6, x0=6, z0=30, size_grid=0, criteria="flux",
         order_dct=30),
    dict(seed=2, Nz=80, Ny=14, Nx=15, P=7, y0=7, x0=8, z0=41, size_grid=1, criteria="flux",
         order_dct=30, shift=(1, 0)),
    dict(seed=3, Nz=67, Ny=12, Nx=13, P=5, y0=5, x0=3, z0=3, size_grid=0, criteria="flux",
         order_dct=None),
    dict(seed=4, Nz=70, Ny=13, Nx=12, P=7, y0=1, x0=10, z0=68, size_grid=0, criteria="flux",
         order_dct=10),
    dict(seed=5, Nz=67, Ny=12, Nx=14, P=5, y0=6, x0=7, z0=33, size_grid=0, criteria="flux",
         order_dct=30, nfields=2),
    dict(seed=6, Nz=67, Ny=12, Nx=13, P=5, y0=5, x0=0, z0=36, size_grid=1, criteria="mse",
         order_dct=30),
]


def run_reference(lib, c):
    """GridAnalysis on the minicubes estimation_line cuts (lib :1881-1898), margins filled with
    data 0 / var inf / weight 0."""
    import _line_oracle as oracle
    z0, y0, x0 = c["det"]
    g = c["size_grid"]
    Ny, Nx = c["raw"].shape[1:]
    weights = c["weights"]
    P = (c["psf"] if weights is None else c["psf"][0]).shape[1]
    W = P + 2 * g
    red_dat = oracle.window(c["raw"], y0, x0, W, 0.0)[0]
    red_var = oracle.window(c["var"], y0, x0, W, np.inf)[0]
    red_wgt = red_psf = None
    if weights is None:
        red_psf = c["psf"]
    else:
        red_wgt = [oracle.window(w[None], y0, x0, W, 0.0)[0][0] for w in weights]
        red_psf = list(c["psf"])
    return lib.GridAnalysis(red_dat, red_var, red_psf, red_wgt, c["horiz"], g, y0, x0, z0, Ny, Nx,
                            c["horiz_psf"], c["criteria"], c["order_dct"])


def main():
    ap = argparse.ArgumentParser()
    from oracle.ref_import import REFERENCE
    ap.add_argument("--reference", default=REFERENCE)
    args = ap.parse_args()
    lib = load_reference(args.reference)
    import _line_oracle as oracle
    np.random.seed(11)   # ARPACK's start vector comes from NumPy's global generator
    out = {"ncases": np.array(len(CASES))}
    for i, spec in enumerate(CASES):
        c = make_case(**spec)
        flux, mse, line, lvar, y, x, z = run_reference(lib, c)
        z0, y0, x0 = c["det"]
        got = oracle.grid_analysis(c["raw"], c["var"], c["psf"], c["weights"], y0, x0, z0,
                                   c["size_grid"], c["criteria"], c["order_dct"], c["horiz_psf"],
                                   c["horiz"])
        assert (got[4], got[5], got[6]) == (y, x, z), (i, got[4:7], (y, x, z))
        dist = np.array([np.max(np.abs(got[2] - line)) / np.max(np.abs(line)),
                         np.max(np.abs(got[3] - lvar)) / np.max(np.abs(lvar))])
        print(f"case {i}: y x z = {y} {x} {z}  flux {flux:.6g}  mse {mse:.6g}  "
              f"dist line {dist[0]:.2e} var {dist[1]:.2e}")
        k = f"c{i}_"
        out[k + "raw"] = c["raw"].astype(np.float32)
        out[k + "var"] = c["var"].astype(np.float32)
        out[k + "psf"] = np.asarray(c["psf"], np.float32)
        if c["weights"] is not None:
            out[k + "weights"] = np.asarray(c["weights"], np.float32)
        out[k + "det"] = np.array(c["det"])
        out[k + "params"] = np.array([c["size_grid"], c["criteria"] == "mse",
                                      -1 if c["order_dct"] is None else c["order_dct"],
                                      c["horiz_psf"], c["horiz"]])
        out[k + "line"], out[k + "lvar"] = np.asarray(line), np.asarray(lvar)
        out[k + "scalars"] = np.array([flux, mse])
        out[k + "yxz"] = np.array([y, x, z])
        out[k + "dist"] = dist
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
