"""The one exchange of the tiled path (origin_amd/multigpu.py): its plans as plain index
arithmetic, its host form against slicing, its device form against its host form; and the order
of ``TiledGLR.run``: arguments are refused before any rank enters a collective.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_session import _threads  # noqa: E402


class _Comm:   # the part of TileComm the host exchange uses
    def __init__(self, group):
        self.group = group


def _groups(world):
    from origin_amd.session import ThreadGroup, _Shared
    sh = _Shared(world)
    return [ThreadGroup(sh, r) for r in range(world)]


def _hand_made_owner(world, Ny=23, Nx=31):
    """Rank 1: an L (a bar down, a bar to the right of its foot); rank 2: one spaxel wide; rank 3
    (world 4): a block in the corner; rank 0: the rest."""
    owner = np.zeros((Ny, Nx), int)
    owner[5:20, 10:14] = 1
    owner[16:20, 10:25] = 1
    owner[2:15, 28] = 2
    if world == 4:
        owner[0:4, 0:9] = 3
    return owner


@pytest.mark.parametrize("world", [3, 4])
def test_move_plan_is_consistent(world):
    """What r sends to t is, spaxel for spaxel and in the same order, what t receives from r; all
    plans applied to plain arrays move every spaxel of the field to its new owner."""
    from origin_amd.multigpu import OwnerTiling, move_plan
    Ny, Nx = 23, 31
    src = OwnerTiling.row_bands(Ny, Nx, world, 1)
    dst = OwnerTiling(_hand_made_owner(world), world, 2)
    field = np.arange(Ny * Nx).reshape(Ny, Nx)
    plans = [move_plan(src, dst, r) for r in range(world)]

    def spaxels(tiling, rank, ix):     # flat field indices of a list of tile indices
        t = tiling.tile(rank)
        return field[t.y0:t.y1, t.x0:t.x1].reshape(-1)[ix]
    have = [np.where(src.owned_tile(r), field[src.tile(r).y0:src.tile(r).y1,
                                              src.tile(r).x0:src.tile(r).x1], -1).reshape(-1)
            for r in range(world)]
    got = [np.full(int(np.prod(dst.tile_shape(r))), -1) for r in range(world)]
    n_local = 0
    for r in range(world):
        sends, recvs, local = plans[r]
        assert all(peer != r for peer, _ in sends + recvs)
        for t in range(world):
            out = [ix for peer, ix in sends if peer == t]
            inn = [ix for peer, ix in plans[t][1] if peer == r]
            assert len(out) == len(inn) <= 1
            if out:
                assert out[0].dtype == np.int32 and len(out[0]) == len(inn[0]) > 0
                assert np.array_equal(spaxels(src, r, out[0]), spaxels(dst, t, inn[0]))
                got[t][inn[0]] = have[r][out[0]]
        if local is not None:
            assert np.array_equal(spaxels(src, r, local[0]), spaxels(dst, r, local[1]))
            got[r][local[1]] = have[r][local[0]]
            n_local += 1
    assert n_local > 0
    for r in range(world):
        t, own = dst.tile(r), dst.owned_tile(r)
        assert np.array_equal(got[r].reshape(own.shape)[own], field[t.y0:t.y1, t.x0:t.x1][own])
        assert np.all(got[r].reshape(own.shape)[~own] == -1)


def _partitions():
    from origin_amd.multigpu import OwnerTiling, Tiling
    thin = np.zeros((30, 40), int)       # rank 1's share: two columns, thinner than the halo
    thin[:, 19:21] = 1
    thin[:, 21:] = 2
    return {"bands": Tiling(300, 300, 3, halo=13), "grid": Tiling(200, 200, 4, layout="grid"),
            "thin": OwnerTiling(thin, 3, 4)}


@pytest.mark.parametrize("dtype", [np.float64, np.uint8])
@pytest.mark.parametrize("case", ["bands", "grid", "thin"])
def test_host_exchange_equals_slicing(case, dtype):
    """``exchange_halo_host`` of every rank over a ThreadGroup is the window of the field its
    extended box covers, on every spaxel the rank owns or needs."""
    from origin_amd.multigpu import exchange_halo_host
    tl = _partitions()[case]
    rng = np.random.default_rng(3)
    field = rng.integers(0, 255, (2, tl.Ny, tl.Nx)).astype(dtype)
    groups = _groups(tl.world)

    def halo(r):
        t = tl.tile(r)
        tile = field[:, t.y0:t.y1, t.x0:t.x1]
        if tl.owned_ext(r) is not None:     # (what other ranks own inside the box: junk)
            tile = np.where(tl.owned_tile(r)[None], tile, dtype(7))
        return exchange_halo_host(_Comm(groups[r]), tl, r, tile)
    for r, ext in enumerate(_threads(tl.world, halo)):
        (ey0, ey1, ex0, ex1), _ = tl.extended(r)
        assert ext.dtype == dtype and ext.shape == (2, ey1 - ey0, ex1 - ex0)
        need = np.ones(ext.shape[1:], bool)
        if tl.owned_ext(r) is not None:
            need = tl.needed(r)[ey0:ey1, ex0:ex1] | tl.owned_ext(r)
            assert need.sum() > tl.owned_ext(r).sum()
        assert np.array_equal(ext[:, need], field[:, ey0:ey1, ex0:ex1][:, need])


class _Counting:
    """Stands for the context, the GLR plan and the communicator: counts every call."""
    P = 5

    def __init__(self):
        self.calls = 0

    def __getattr__(self, name):
        def call(*args, **kw):
            self.calls += 1
            return _Array(args[0] if args else (), kw.get("dtype", args[1] if len(args) > 1
                                                          else np.float32))
        return call


class _Array:
    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)


def test_run_refuses_its_arguments_before_any_collective(monkeypatch):
    from origin_amd import multigpu
    plan, ctx, comm = _Counting(), _Counting(), _Counting()
    monkeypatch.setattr(multigpu.kernels, "GLRPlan", lambda *a, **k: plan)
    tl = multigpu.Tiling(40, 52, 2, area_size=13, halo=3)
    glr = multigpu.TiledGLR(ctx, comm, tl, 0, 5, np.ones((5, 5, 5)), None)
    cube = _Array(glr.shape, np.float32)
    before = ctx.calls
    with pytest.raises(ValueError, match="pass all three output cubes or none of them"):
        glr.run(None, None, None, cube, None)
    with pytest.raises(ValueError, match=r"local_max='sparse' goes with correl=None \(no crop"):
        glr.run(None, None, cube, cube, cube, local_max="sparse")
    assert (comm.calls, plan.calls, ctx.calls - before) == (0, 0, 0)


@pytest.mark.gpu
def test_device_exchange_equals_host_exchange():
    """``exchange_halo`` on the device against ``exchange_halo_host``, and ``redistribute`` there
    and back, three contexts on one card: a clipped halo, a pair of ranks with nothing to
    exchange, a corner box, a self-to-self move; every exchange twice, the second time with the
    buffers and index lists the first one left in ``bufs``."""
    from origin_amd import multigpu
    from origin_amd.session import DeviceGroup, redistribute
    Nz, Ny, Nx = 5, 40, 52
    amap = np.ones((Ny, Nx), int)
    amap[:, 24:26] = 2                     # a share two spaxels wide
    amap[:, 26:] = 3
    rect = multigpu.Tiling(Ny, Nx, 3, area_size=13, halo=3)
    areas = multigpu.OwnerTiling.from_areamap(amap, 3, 3)
    rows = multigpu.OwnerTiling.row_bands(Ny, Nx, 3, 3)
    rng = np.random.default_rng(11)
    cubes = [rng.standard_normal((Nz, Ny, Nx)).astype(np.float32),
             rng.integers(0, 255, (Nz, Ny, Nx)).astype(np.uint8)]
    g = DeviceGroup([0, 0, 0], "host")

    def tile_of(tl, r, cube):
        t = tl.tile(r)
        return np.ascontiguousarray(cube[:, t.y0:t.y1, t.x0:t.x1])

    def one(r):
        ctx, comm, out = g.ctxs[r], g.comms[r], []
        for cube in cubes:
            for tl in (rect, areas):
                host = multigpu.exchange_halo_host(comm, tl, r, tile_of(tl, r, cube))
                bufs = {}
                dev = [multigpu.exchange_halo(ctx, comm, tl, r, ctx.to_device(tile_of(tl, r, cube)),
                                              None, bufs).to_host() for _ in range(2)]
                out.append(("halo", tl, cube, host, dev))
            there, back = {}, {}
            moved = []
            for _ in range(2):
                mid = ctx.zeros((Nz,) + areas.tile_shape(r), cube.dtype)
                end = ctx.zeros((Nz,) + rows.tile_shape(r), cube.dtype)
                redistribute(ctx, comm, rows, areas, r, ctx.to_device(tile_of(rows, r, cube)), mid,
                             there)
                redistribute(ctx, comm, areas, rows, r, mid, end, back)
                ctx.sync()
                moved.append((mid.to_host(), end.to_host()))
            out.append(("move", None, cube, None, moved))
        return out
    try:
        res = g.run(one)
    finally:
        g.close()
    for r, items in enumerate(res):
        for kind, tl, cube, host, dev in items:
            if kind == "halo":
                (ey0, ey1, ex0, ex1), _ = tl.extended(r)
                need = np.ones((ey1 - ey0, ex1 - ex0), bool)
                if tl.owned_ext(r) is not None:
                    need = tl.needed(r)[ey0:ey1, ex0:ex1] | tl.owned_ext(r)
                assert np.array_equal(host[:, need], cube[:, ey0:ey1, ex0:ex1][:, need])
                for d in dev:
                    assert d.dtype == cube.dtype and np.array_equal(d[:, need], host[:, need])
            else:
                own = areas.owned_tile(r)
                for mid, end in dev:
                    assert np.array_equal(mid[:, own], tile_of(areas, r, cube)[:, own])
                    assert np.array_equal(end, tile_of(rows, r, cube))
