"""Step 9: from ``Cat2`` to ``Cat3_lines`` and ``Cat3_sources`` (reference
muse_origin/steps.py:1149-1171, ``CleanResults.run``; lib_origin.py:1994-2222).

The three functions of the reference -- ``merge_similar_lines`` (:2140-2222), ``unique_sources``
(:1994-2091), ``add_tglr_stat`` (:2094-2137) -- are table work on 10^2..10^4 rows and stay on
the host.  What does not stay there are the two ``np.std`` calls over full cubes that open
``add_tglr_stat`` (:2127-2129): with cube_correl and cube_std resident in HBM they are two
reductions on the device (``kernels.cube_std``, csrc/stats.hip) and two scalars cross PCIe.

Tables are plain dicts of NumPy columns, as in ``detection.py`` and ``lines.py``; string
columns are NumPy ``str`` arrays.

Deviations from the reference:

1. rows with equal ``(ID, z)`` come out in input-row order (the reference's ``Table.sort`` is
   not stable there; the same situation as section 3h);
2. a source whose fluxes sum to 0 takes the unweighted mean position (the single fallback row
   of step 8 has flux 0.0; the reference's ``np.average`` raises ``ZeroDivisionError`` there);
3. an empty ``Cat2`` gives empty tables;
4. without ``ra`` / ``dec`` / ``lbda`` columns (a ``SimpleOrig`` has no WCS) the columns derived
   from them (``ra``, ``dec``, ``waves``) are left out.
"""
from collections import OrderedDict
from datetime import datetime

import numpy as np

from . import cubes

NOT_MERGED = -9999
STAT_COLUMNS = ("flux", "STD", "nsigSTD", "T_GLR", "nsigTGLR", "purity")


def _columns(tbl):
    """Any table-like (an astropy Table, a dict of columns) as an OrderedDict of NumPy columns."""
    names = tbl.colnames if hasattr(tbl, "colnames") else list(tbl.keys())
    return OrderedDict((k, np.asarray(tbl[k])) for k in names)


def _groups(ids):
    """(order, starts, keys): a stable sort of the rows by ``ids``, the first position of every
    group in it, and the group keys (ascending)."""
    ids = np.asarray(ids)
    order = np.argsort(ids, kind="stable")
    srt = ids[order]
    starts = np.flatnonzero(np.concatenate(([True], srt[1:] != srt[:-1]))) if len(srt) else \
        np.zeros(0, np.int64)
    return order, starts, srt[starts]


def merge_similar_lines(cat2, z_pix_threshold=5):
    """``merge_similar_lines`` (lib_origin.py:2140-2222).  ``cat2``: columns ``ID``, ``z``,
    ``flux``, ``num_line`` (and whatever else the table carries).  Returns the same rows sorted
    by ``(ID, z, input row)`` with two more columns: ``line_merged_flag`` (bool: the line is part
    of a run of lines of one ``ID`` whose consecutive ``z`` gaps are all below the threshold -- a
    gap equal to it splits the run, runs percolate) and ``merged_in`` (int64: the ``num_line`` of
    the run's line of highest flux for every other line of the run, -9999 otherwise)."""
    cat = _columns(cat2)
    n = len(cat["ID"])
    ids, z = cat["ID"], cat["z"]
    order = np.lexsort((np.arange(n), z, ids))          # deviation 1: ties keep the input order
    out = OrderedDict((k, v[order]) for k, v in cat.items())
    flag = np.zeros(n, dtype=bool)
    merged_in = np.full(n, NOT_MERGED, dtype=np.int64)
    if n:
        ids, z = out["ID"], out["z"]
        first = np.concatenate(([True], (ids[1:] != ids[:-1])
                                | ((z[1:] - z[:-1]) >= z_pix_threshold)))   # :2195-2201
        run = np.cumsum(first) - 1
        flag = np.bincount(run)[run] > 1                                    # :2204-2206
        # the line of highest flux of every run: last of its run in (run, flux, row) order
        byflux = np.lexsort((np.arange(n), out["flux"], run))
        last = np.concatenate((run[byflux][1:] != run[byflux][:-1], [True]))
        winner = np.empty(run[-1] + 1, dtype=np.int64)
        winner[run[byflux][last]] = byflux[last]
        w = winner[run]
        losers = flag & (w != np.arange(n))
        merged_in[losers] = out["num_line"][w[losers]]                      # :2207, :2213-2214
    out["line_merged_flag"] = flag
    out["merged_in"] = merged_in
    return out


def unique_sources(cat3_lines):
    """``unique_sources`` (lib_origin.py:1994-2091): one row per ``ID``, ascending.  ``x``, ``y``
    (``ra``, ``dec`` when the table has them) are flux-weighted averages over all lines of the
    source, ``n_lines`` counts the lines not merged into another, ``seg_label`` and ``comp`` are
    those of the source's first row, ``line_merged_flag`` is true when any line is flagged and
    ``waves`` (when the table has ``lbda``) lists ``str(int(lbda))`` of up to three unmerged lines
    by decreasing flux."""
    cat = _columns(cat3_lines)
    order, starts, keys = _groups(cat["ID"])
    ends = np.concatenate((starts[1:], [len(order)])).astype(np.int64)
    pos = [k for k in ("ra", "dec", "x", "y") if k in cat]
    avg = {k: np.zeros(len(keys)) for k in pos}
    n_lines = np.zeros(len(keys), dtype=np.int64)
    flagged = np.zeros(len(keys), dtype=bool)
    waves = []
    for g, (a, b) in enumerate(zip(starts, ends)):
        rows = order[a:b]
        flux = cat["flux"][rows]
        # deviation 2: np.average raises when the weights sum to 0
        wgt = flux if np.sum(flux) != 0 else None
        for k in pos:
            avg[k][g] = np.average(cat[k][rows], weights=wgt)
        single = cat["merged_in"][rows] == NOT_MERGED
        n_lines[g] = np.sum(single)
        flagged[g] = np.any(cat["line_merged_flag"][rows])
        if "lbda" in cat:
            un = rows[single]
            un = un[np.argsort(cat["flux"][un], kind="stable")]
            waves.append(",".join(str(int(v)) for v in cat["lbda"][un][:-4:-1]))
    first = order[starts]
    out = OrderedDict(ID=keys.astype(np.int64))
    for k in pos:
        out[k] = avg[k]
    out["n_lines"] = n_lines
    out["seg_label"] = cat["seg_label"][first]
    out["comp"] = cat["comp"][first]
    out["line_merged_flag"] = flagged
    if "lbda" in cat:
        out["waves"] = np.array(waves, dtype=str) if waves else np.zeros(0, dtype="U1")
    return out


def add_tglr_stat(src, lines, std_correl, std_std):
    """``add_tglr_stat`` (lib_origin.py:2094-2137) behind its two ``np.std`` calls, which are
    the arguments here.  ``lines`` gains ``nsigTGLR = T_GLR / std_correl`` and ``nsigSTD = STD /
    std_std`` in place, as in the reference; the returned table is ``src`` joined on ``ID`` with
    the per-``ID`` maxima of ``flux, STD, nsigSTD, T_GLR, nsigTGLR, purity`` (in that order,
    behind the columns of ``src``).  The maxima are ``np.maximum.reduceat``'s: a source with a
    NaN in a column gets NaN -- one with ``comp`` 0 and ``comp`` 1 lines has NaN ``T_GLR`` and
    ``STD``."""
    with np.errstate(divide="ignore", invalid="ignore"):
        lines["nsigTGLR"] = np.asarray(lines["T_GLR"], dtype=np.float64) / std_correl
        lines["nsigSTD"] = np.asarray(lines["STD"], dtype=np.float64) / std_std
    order, starts, keys = _groups(lines["ID"])
    src = _columns(src)
    # inner join on ID (both tables hold every source once they come from unique_sources)
    sid = src["ID"]
    sord = np.argsort(sid, kind="stable")
    common = np.intersect1d(sid, keys)
    s_rows = sord[np.searchsorted(sid[sord], common)]
    g_rows = np.searchsorted(keys, common)
    out = OrderedDict((k, v[s_rows]) for k, v in src.items())
    for k in STAT_COLUMNS:
        col = np.asarray(lines[k])[order]
        mx = np.maximum.reduceat(col, starts) if len(starts) else col[:0]
        out[k] = mx[g_rows]
    return out


def cube_std(ctx, cube):
    """``np.std`` of a cube in any of its forms (``cubes.resident``) as a reduction in HBM."""
    return cubes.std(cubes.resident(ctx, cube))


def clean_results(ctx, cat2, cube_correl, cube_std_, merge_lines_z_threshold=5):
    """``CleanResults.run`` (steps.py:1149-1160) on the device cubes ``cube_correl`` and
    ``cube_std``.  Returns ``(cat3_lines, cat3_sources, cat3_ts)``; ``cat3_ts`` is the ISO
    timestamp the reference puts in ``meta['CAT3_TS']`` of both tables (:2220, :2089)."""
    lines = merge_similar_lines(cat2, z_pix_threshold=merge_lines_z_threshold)
    ts = datetime.now().isoformat()
    src = unique_sources(lines)
    src = add_tglr_stat(src, lines, cube_std(ctx, cube_correl), cube_std(ctx, cube_std_))
    return lines, src, ts


def from_session(orig, cat2=None, merge_lines_z_threshold=5):
    """``clean_results`` on what a session holds: ``orig.Cat2`` unless given, and the cube_correl
    and cube_std that steps 5 and 1 left in HBM (read back from their files through the device-side
    FITS decoder when the session was dumped)."""
    return clean_results(cubes.ctx_of(orig), orig.Cat2 if cat2 is None else cat2,
                         cubes.session_cube(orig, "cube_correl"),
                         cubes.session_cube(orig, "cube_std"), merge_lines_z_threshold)
