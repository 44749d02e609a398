"""Point lists of the matching tests (tests/test_match_cases.py checks on the CPU that each family
is what it claims and that cKDTree agrees with the predicate on it; tests/test_hip_match.py runs
them on the device).

A case is ``(a, b, a_val)``: ``a`` / ``b`` three float64 columns (x, y, z), ``a_val`` float32 with
ties and negative values and without zeros (the sign of a zero is the one thing the maximum of
equal floats leaves open).  The field is (Nz, Ny, Nx) = (40, 23, 17) unless said; A has integer
coordinates.  Families:
  A  sizes 0, 1, 63, 64, 65, 257, 4099 mixed, and a 1 x 1 x 1 field with every point coincident
  B  exact ties: B on the quarter grid, so every d2 is exact
  C  the bounding box: B outside A's range by less and by more than r, negative coordinates, A at
     the eight corners
  D  the shell: B_i = A_i + r u_i with u_i a random unit vector, x moved by -3..+3 ulps
  E  load: 700 points of B in one cell; 600 in one spaxel column of a 3681-deep field;
     duplicates inside A and inside B
  F  b_max: several A with different values around one B, equal values, negative values, a B with
     no A
"""
import functools
from collections import OrderedDict

import numpy as np

RADII = (0.0, 1.0, 2.5, 4.5, 50.0)
FIELD = (40, 23, 17)
SIZES = ((0, 0), (0, 5), (5, 0), (1, 1), (1, 64), (63, 65), (64, 64), (65, 63), (257, 1),
         (257, 4099), (4099, 257), (4099, 65))
SHELL_RADII = (2.5, 4.5)
SHELL_N = 3000


def _values(rng, n):
    v = np.round(rng.normal(0.0, 3.0, n) * 8) / 8
    v[v == 0] = 0.125
    return v.astype(np.float32)


def _int_points(rng, n, field=FIELD):
    Nz, Ny, Nx = field
    return (rng.integers(0, Nx, n).astype(np.float64), rng.integers(0, Ny, n).astype(np.float64),
            rng.integers(0, Nz, n).astype(np.float64))


def _quarter_points(rng, n, field=FIELD, pad=0.0):
    Nz, Ny, Nx = field
    return tuple(rng.integers(int(-4 * pad), int(4 * (N - 1 + pad)) + 1, n) / 4.0
                 for N in (Nx, Ny, Nz))


def _cols(rows):
    rows = np.asarray(rows, np.float64).reshape(-1, 3)
    return rows[:, 0].copy(), rows[:, 1].copy(), rows[:, 2].copy()


def _cat(*lists):
    return tuple(np.concatenate([np.asarray(lst[k], np.float64) for lst in lists]) for k in range(3))


def _sizes(rng):
    out = OrderedDict()
    for n, m in SIZES:
        out[f"A_sizes_{n}_{m}"] = (_int_points(rng, n), _quarter_points(rng, m), _values(rng, n))
    z65, z64 = np.zeros(65), np.zeros(64)
    out["A_coincident_1x1x1"] = ((z65, z65, z65), (z64, z64, z64), _values(rng, 65))
    return out


# offsets (dx, dy, dz) with an exact d2: 6.25 = 2.5^2 twice, 20.25 = 4.5^2 twice, 6 and 8 (integer
# offsets: matched at 2.5 / not), 0, and quarter-grid offsets just inside and outside 1 and 2.5
TIE_OFFSETS = ((1.5, 2, 0), (0, -1.5, 2), (4.5, 0, 0), (0, 0, -4.5), (2, 1, 1), (2, 2, 0),
               (0, 0, 0), (1, 0, 0), (0.75, 0.5, 0.5), (0.75, 0.75, 0), (1.5, 2, 0.25),
               (1.5, 1.75, 0.75), (3.5, 2.75, 0.5), (3, 3, 1.5))


def _ties(rng):
    a = _int_points(rng, 120)
    rows = [(a[0][i] + dx, a[1][i] + dy, a[2][i] + dz)
            for i in range(0, 120, 2) for dx, dy, dz in TIE_OFFSETS[(i // 2) % 3::3]]
    return OrderedDict(B_ties=(a, _cols(rows), _values(rng, 120)))


def _bbox(rng):
    Nz, Ny, Nx = FIELD
    corners = [(x, y, z) for x in (0, Nx - 1) for y in (0, Ny - 1) for z in (0, Nz - 1)]
    a = _cat(_cols(corners), _int_points(rng, 40))
    b = _cols([(-0.75, 0, 0), (-2.5, 0, 0), (-2.75, 0, 0), (-60, 5, 5), (Nx - 1 + 4.5, Ny - 1, 0),
               (Nx - 1 + 4.75, Ny - 1, 0), (Nx + 80, Ny + 80, Nz + 80), (0, -1.5, -2),
               (8, 11, Nz - 1 + 0.75), (8, 11, Nz + 300), (-1, -1, -1), (-3, -3, -3.25),
               (Nx - 1, Ny - 1, Nz - 1 + 2.5), (5, -1000.5, 3)])
    neg = (_int_points(rng, 50), _quarter_points(rng, 60))
    shift = (-200.0, -31.0, -47.0)
    a2 = tuple(c + s for c, s in zip(neg[0], shift))
    b2 = tuple(c + s for c, s in zip(neg[1], shift))
    return OrderedDict(C_bbox_outside=(a, b, _values(rng, a[0].size)),
                       C_bbox_negative=(a2, b2, _values(rng, 50)))


def _shell(rng, r):
    a = _int_points(rng, SHELL_N)
    u = rng.normal(size=(SHELL_N, 3))
    u /= np.sqrt((u * u).sum(axis=1))[:, None]
    bx = a[0] + r * u[:, 0]
    steps = rng.integers(-3, 4, SHELL_N)
    for k in range(1, 4):
        bx = np.where(steps >= k, np.nextafter(bx, np.inf), bx)
        bx = np.where(steps <= -k, np.nextafter(bx, -np.inf), bx)
    return a, (bx, a[1] + r * u[:, 1], a[2] + r * u[:, 2]), _values(rng, SHELL_N)


def _load(rng):
    out = OrderedDict()
    # 700 points of B on the 1/16 grid of one unit cube, A the integer grid around it
    b = tuple(8 + rng.integers(0, 16, 700) / 16.0 for _ in range(3))
    g = np.arange(2, 16, dtype=np.float64)
    ax, ay, az = (c.reshape(-1) for c in np.meshgrid(g, g, g, indexing="ij"))
    out["E_load_one_cell"] = ((ax, ay, az), b, _values(rng, ax.size))
    # the bright source: 600 points of B in the spaxel column (7, 11) of a 3681-deep field, 40 of
    # them repeated; A down that column and its four neighbours
    Nz = 3681
    bz = rng.choice(Nz, 560, replace=False).astype(np.float64)
    bz = np.concatenate([bz, bz[:40]])
    z = np.arange(Nz, dtype=np.float64)
    cols = [(7, 11), (8, 11), (6, 11), (7, 12), (7, 9)]
    a = (np.concatenate([np.full(Nz, float(x)) for x, _ in cols]),
         np.concatenate([np.full(Nz, float(y)) for _, y in cols]), np.tile(z, len(cols)))
    out["E_load_column_3681"] = (a, (np.full(600, 7.0), np.full(600, 11.0), bz),
                                 _values(rng, a[0].size))
    a = _int_points(rng, 100)
    b = _quarter_points(rng, 90)
    out["E_load_duplicates"] = (tuple(np.tile(c, 3) for c in a), tuple(np.repeat(c, 4) for c in b),
                                _values(rng, 300))
    return out


def _bmax(rng):
    # B0 with five A around it (values all different, one negative), B1 with equal values, B2 with
    # negative values only, B3 with no A at all, B4 coincident with one A
    a = _cols([(5, 5, 5), (6, 5, 5), (5, 6, 5), (5, 5, 6), (4, 5, 5),
               (12, 15, 20), (12, 16, 20), (12, 15, 21),
               (3, 20, 33), (3, 21, 33),
               (15, 2, 38)])
    val = np.array([1.5, 7.25, -2.0, 3.0, 7.0, 4.5, 4.5, 4.5, -1.25, -6.0, 2.0], np.float32)
    b = _cols([(5.25, 5.25, 5.25), (12, 15.5, 20.5), (3, 20.5, 33), (10, 10, 0.5), (15, 2, 38)])
    return OrderedDict(F_bmax=(a, b, val))


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20240611)
    out = OrderedDict()
    for part in (_sizes(rng), _ties(rng), _bbox(rng)):
        out.update(part)
    for r in SHELL_RADII:
        out[f"D_shell_{r}"] = _shell(rng, r)
    out.update(_load(rng))
    out.update(_bmax(rng))
    return out


def family(prefix):
    return OrderedDict((k, v) for k, v in cases().items() if k.startswith(prefix))
