"""Shapes and patterns of the segmentation tests (tests/test_segmap_cases.py checks on the CPU
that each pattern is what it claims; tests/test_hip_segmap.py runs them on the device)."""
import numpy as np

FWHM_FSF = (0, 1, 2, 3, 4, 7, 10, 11)     # no disc, f = 0 (empty), f = 1, 1, 2, 3, 5, 5


def label_shapes(tw, th, span):
    """(Ny, Nx) by class of the labeller's geometry: ``tw`` x ``th`` its tile, ``span`` the pixels
    whose roots its one scan workgroup counts in a single pass."""
    side = int(np.ceil(np.sqrt(span + 1)))
    return {
        "one_pixel": (1, 1),
        "one_row": (1, tw + 1),
        "one_column": (th + 1, 1),
        "one_tile": (th, tw),
        "below_a_tile": (th - 1, tw - 1),
        "many_tiles": (2 * th + 3, 3 * tw + 5),
        "two_scan_passes": (side, side),
    }


def mask_shapes(tw, th):
    return {"a": (th - 1, tw + 1), "b": (th + 1, 2 * tw + 3)}


# ------------------------------------------------------------------------------ labeller patterns
def _serpentine(Ny, Nx):
    m = np.zeros((Ny, Nx), bool)
    m[0::2] = True
    for y in range(1, Ny, 2):              # joined alternately at the right and the left end
        m[y, Nx - 1 if (y // 2) % 2 == 0 else 0] = True
    return m


def _comb(Ny, Nx):
    m = np.zeros((Ny, Nx), bool)
    m[:, 0::2] = True                      # the teeth
    m[Ny - 1] = True                       # joined by the last row only
    return m


def _depth(Ny, Nx):
    yy, xx = np.mgrid[:Ny, :Nx]
    return np.minimum(np.minimum(yy, Ny - 1 - yy), np.minimum(xx, Nx - 1 - xx))


def _rings(Ny, Nx):
    return _depth(Ny, Nx) % 2 == 0


def rings_count(Ny, Nx):
    return ((min(Ny, Nx) - 1) // 2) // 2 + 1


def _spiral(Ny, Nx):
    """The rings, each one opened below its top-left corner and joined to the next one inside."""
    m = _rings(Ny, Nx)
    for d in range(0, (min(Ny, Nx) - 1) // 2 - 1, 2):
        m[d + 1, d] = False
        m[d + 2, d + 1] = True
    return m


def _random(density, seed):
    return lambda Ny, Nx: np.random.default_rng(seed).random((Ny, Nx)) < density


LABEL_PATTERNS = {
    "zeros": lambda Ny, Nx: np.zeros((Ny, Nx), bool),
    "ones": lambda Ny, Nx: np.ones((Ny, Nx), bool),
    "checkerboard": lambda Ny, Nx: np.add.outer(np.arange(Ny), np.arange(Nx)) % 2 == 0,
    "rows": lambda Ny, Nx: np.broadcast_to((np.arange(Ny) % 2 == 0)[:, None], (Ny, Nx)).copy(),
    "columns": lambda Ny, Nx: np.broadcast_to((np.arange(Nx) % 2 == 0)[None, :], (Ny, Nx)).copy(),
    "serpentine": _serpentine,
    "comb": _comb,
    "rings": _rings,
    "spiral": _spiral,
    "random_0.3": _random(0.3, 31),
    "random_0.5": _random(0.5, 32),
    "random_0.593": _random(0.593, 33),
    "random_0.8": _random(0.8, 34),
}


# ---------------------------------------------------------------------------------- mask patterns
GAMMA = 1.25
_LO, _HI = 0.5, 3.0


def _borders(Ny, Nx):
    d = np.full((Ny, Nx), _LO)
    d[:4, :4] = d[:3, -5:] = d[-4:, :3] = d[-5:, -4:] = _HI                    # the corners
    d[:3, Nx // 2 - 3:Nx // 2 + 3] = d[-4:, Nx // 2 - 2:Nx // 2 + 2] = _HI      # top, bottom
    d[Ny // 2 - 3:Ny // 2 + 3, :3] = d[Ny // 2 - 2:Ny // 2 + 3, -4:] = _HI      # left, right
    d[0, 8:12] = d[6:10, 0] = _HI          # one pixel thick along a border: eroded away
    return d


def _specks(Ny, Nx):
    d = np.full((Ny, Nx), _LO)
    d[5, 5] = d[0, 9] = d[Ny - 1, Nx - 1] = d[12, 0] = _HI                     # single pixels
    d[9, 9:11] = d[14:16, 20] = d[0, 14:16] = d[20:22, Nx - 1] = _HI            # two-pixel specks
    d[18:21, 4:7] = _HI                    # a 3 x 3 square survives as a plus
    return d


def _cross(Ny, Nx):
    d = np.full((Ny, Nx), _LO)
    for cy, cx in ((6, 6), (1, Nx - 2), (Ny - 2, 1), (15, 16), (16, 31)):
        d[cy, cx - 1:cx + 2] = d[cy - 1:cy + 2, cx] = _HI
    return d


def _nonfinite(Ny, Nx):
    d = np.full((Ny, Nx), _LO)
    d[4:12, 4:12] = d[14:24, 14:26] = _HI
    d[7, 7], d[18, 18], d[18, 22] = np.nan, -np.inf, np.inf
    d[2, 20], d[26, 5], d[27, 27] = np.nan, -np.inf, np.inf
    d[0, 0], d[Ny - 1, 0] = -np.inf, np.nan
    return d


def _equal_gamma(Ny, Nx):
    d = np.full((Ny, Nx), _LO)
    d[5:14, 5:14] = d[:6, 20:29] = _HI
    d[9, 9] = d[0, 24] = GAMMA                                  # not above: a hole
    d[20:26, 8:16] = np.nextafter(GAMMA, np.inf)                # the next float64 is above
    d[22, 11] = np.nextafter(GAMMA, -np.inf)
    return d


def _everything(Ny, Nx):
    rng = np.random.default_rng(77)
    d = np.maximum.reduce([f(Ny, Nx) for f in (_borders, _specks, _cross)])
    d = np.where(rng.random((Ny, Nx)) < 0.08, _HI, d)
    d[rng.random((Ny, Nx)) < 0.02] = np.nan
    d[rng.random((Ny, Nx)) < 0.02] = -np.inf
    d[rng.random((Ny, Nx)) < 0.02] = GAMMA
    return d


MASK_PATTERNS = {
    "borders": _borders,
    "specks": _specks,
    "cross": _cross,
    "nonfinite": _nonfinite,
    "equal_gamma": _equal_gamma,
    "everything": _everything,
}
