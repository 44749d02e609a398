"""Test-side restatement of the launch arithmetic of the greedy PCA's per-iteration chain
(csrc/pca.hip: build_work_list, enqueue_chain, flush, the choice of the selection kernel), shared by
test_pca_chain_cases.py (CPU: the inputs reach the shapes they aim at) and test_hip_pca_chain.py
(GPU: the same for the device at hand)."""
from _gram_geometry import gram_geometry

PCA_CAP = 64            # vectors kept per area before the cube is flushed
SEL_EPT = 12            # list entries per thread of the resident selection
LANCZOS_M, PW_N, LP_NMAX = 48, 96, 512
UW_SLICES = 32
FLUSH_ZB = 32


def cdiv(a, b):
    return -(-a // b)


def ld_of(n):
    return (n + 15) // 16 * 16


def selection(sizes):
    """(resident, entries per thread of every area): pca_select_fast_kernel serves a run whose
    largest area has at most 1024 * SEL_EPT spaxels; thread t then owns E = ceil(ns / 1024) entries."""
    resident = max(sizes) <= 1024 * SEL_EPT
    return resident, [cdiv(ns, 1024) for ns in sizes]


def iteration(num_cu, Nz, S, sizes, work):
    """The launches of one iteration.  sizes: spaxels of every area of the run; work: [(area, n, nb,
    T)] of the areas with n >= 2, T = vectors the area holds (since the last flush)."""
    nw = len(work)
    lds = [ld_of(n) for _, n, _, _ in work]
    ldmax = max(lds)
    nsmax = max(sizes[a] for a, _, _, _ in work)
    cb = sum(sizes[a] for a, _, _, _ in work)
    resident, _ = selection(sizes)
    # gather_xp_kernel: 2 * num_cu blocks wanted, at most 16 z slices, slices of whole 16 channels
    cols = cdiv(ldmax, 64) * nw
    nzb = max(1, min((num_cu * 2 + cols - 1) // cols, 16))
    gzper = (cdiv(Nz, nzb) + 15) // 16 * 16
    nzb = cdiv(Nz, gzper)
    # deflate_dot*_kernel: 8 * num_cu blocks wanted, at most 32 slices, at most Nz
    blocks = cdiv(nsmax, 256) * nw
    nzs = max(1, min((num_cu * 8 + blocks - 1) // blocks, 32))
    nzs = min(nzs, Nz)
    zper = cdiv(Nz, nzs)
    nzs = cdiv(Nz, zper)
    ntiles = sum(cdiv(ld, 32) * (cdiv(ld, 32) + 1) // 2 for ld in lds)
    launch = ("small" if ldmax <= LANCZOS_M else "mid" if ldmax <= PW_N else
              "plain" if ldmax <= LP_NMAX else "round2")
    return dict(
        nw=nw, ld=lds, ldmax=ldmax, nsmax=nsmax, cb=cb,
        gather=(nzb, gzper, Nz - (nzb - 1) * gzper), gather_colblocks=cdiv(ldmax, 64),
        deflate=(nzs, zper, Nz - (nzs - 1) * zper),
        rows=2 * cb >= S,
        all_small=ldmax <= LANCZOS_M, eig_launch=launch,
        ksplit=gram_geometry(num_cu, ntiles, Nz)[0], ntiles=ntiles,
        fbold=[T >= 1 for _, _, _, T in work],
        svalid=[resident and T >= 1 for _, _, _, T in work],
        uw_empty_slices=UW_SLICES - cdiv(Nz, cdiv(Nz, UW_SLICES)),
    )


def flush(Nz, sizes, T, everything):
    """The launch of one flush.  T: vectors held per area; everything: the output buffer differs
    from the one read (every area is written), else only the areas that hold vectors."""
    areas = [a for a, ns in enumerate(sizes) if ns > 0 and (everything or T[a] > 0)]
    if not areas:
        return None
    nxb, nzb = cdiv(max(sizes[a] for a in areas), 256), cdiv(Nz, FLUSH_ZB)
    return dict(areas=areas, nxb=nxb, nzb=nzb, padding=cdiv(nxb * nzb, 8) * 8 - nxb * nzb,
                T=[T[a] for a in areas], last_rows=Nz - (nzb - 1) * FLUSH_ZB)


def run(num_cu, Nz, S, sizes, works, inplace):
    """A whole run.  works: per executed iteration [(area, n, nb)] of the areas with n >= 2 (n and nb
    of the restatement).  Tracks the vectors held per area as the driver does: an iterating area at
    PCA_CAP flushes every area before the iteration.  Returns (iterations, flushes): per iteration
    the dict of ``iteration`` plus ``flushed_before``; the flushes in order, the final one last."""
    held = [0] * len(sizes)
    dst_is_src = inplace
    its, flushes = [], []
    for w in works:
        full = any(held[a] >= PCA_CAP for a, _, _ in w)
        if full:
            f = flush(Nz, sizes, held, not dst_is_src)
            f["final"] = False
            flushes.append(f)
            held = [0] * len(sizes)
            dst_is_src = True
        g = iteration(num_cu, Nz, S, sizes, [(a, n, nb, held[a]) for a, n, nb in w])
        g["flushed_before"] = full
        its.append(g)
        for a, _, _ in w:
            held[a] += 1
    f = flush(Nz, sizes, held, not dst_is_src)
    if f is not None:
        f["final"] = True
        flushes.append(f)
    return its, flushes
