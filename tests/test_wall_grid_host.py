"""Maps of any size without a GPU: the builder of socialways_amd.WallGrid against its definition, the numpy model of the query
range and the visit-once rule (tests/_wall_grid_ref.py) against the float64 distances of tests/_walls_ref.py - every pair within
reach visited, none twice, whatever the cell -, the host surface of the feature (argument checks of the two entries, of ops /
stats / set_wall_loss / evaluate_walls, the reach refusal, the refusals of the refinement, the graph key), and the tracer
trace_occupancy() on images whose boundary is known."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _wall_grid_ref as G
import _wall_loss_ref as WR
from _ref64 import scene_rows

REACH = 0.55


def _grid(walls, reach=REACH, cell=None):
    import socialways_amd as sw
    return sw.WallGrid(walls, reach, cell, device="cpu")


# ---- the builder --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,cell", [(33, 0.5), (33, 1.0), (130, 3.0), (1500, 1.0), (33, 1e6)])
def test_every_wall_is_listed_in_exactly_the_cells_of_its_range(M, cell):
    case = WR.walls_case(8, 12, M, 1)
    g = _grid(case["walls"], cell=cell)
    assert g.M == M and g.cell == g.cell_asked == cell and g.reach == float(np.float32(REACH))
    assert (g.nx, g.ny) == (1, 1) if cell == 1e6 else g.nx * g.ny > 4
    assert g.origin == tuple(float(v) for v in case["walls"].reshape(-1, 2).min(0))
    assert torch.equal(g.walls, torch.as_tensor(case["walls"])) and g.walls.dtype == torch.float32
    for dev, host in ((g.cell_ptr, g.cell_ptr_host), (g.cell_walls, g.cell_walls_host), (g.wall_cells, g.wall_cells_host)):
        assert dev.dtype == torch.int32 and np.array_equal(dev.numpy(), host)
    G.check_builder(g)
    again = _grid(case["walls"].reshape(-1, 4).tolist(), cell=cell)              # host data, (M, 4): the same grid, bit for bit
    assert np.array_equal(again.cell_walls_host, g.cell_walls_host) and np.array_equal(again.cell_ptr_host, g.cell_ptr_host)
    assert len(g.key()) == 11 and g.key() != again.key(), "the key holds the addresses: another grid, another key"


def test_empty_maps_posts_and_coincident_walls():
    g = _grid(np.zeros((0, 4), np.float32))
    assert (g.M, g.nx, g.ny, g.L) == (0, 1, 1, 0) and g.cell_ptr_host.tolist() == [0, 0] and g.wall_cells.shape == (0, 4)
    G.check_builder(g)
    posts = np.random.RandomState(0).uniform(0, 5, (40, 1, 2)).repeat(2, 1).astype(np.float32)
    g = _grid(posts, cell=0.5)
    G.check_builder(g)
    assert g.L == 40 and (g.wall_cells_host[:, :2] == g.wall_cells_host[:, 2:]).all(), "a post lies in one cell"
    same = np.tile(np.array([[[1.5, 2.5], [1.5, 2.5]]], np.float32), (7, 1, 1))
    g = _grid(same)                                                              # zero extent: one cell lists them all
    G.check_builder(g)
    assert (g.nx, g.ny, g.L) == (1, 1, 7) and g.cell_walls_host.tolist() == list(range(7))
    assert g.cell == 4.0 * g.reach, "the default cell is 4 reach (DESIGN.md section 9)"


def test_the_cell_cap_enlarges_the_cell():
    import socialways_amd as sw
    walls = np.array([[0, 0, 1, 1], [5000, 5000, 5001, 5001]], np.float32)
    g = _grid(walls, reach=0.5, cell=1.0)
    assert g.cell_asked == 1.0 and g.cell > 1.0 and g.nx * g.ny <= sw.WallGrid.MAX_CELLS == 1 << 20
    assert g.nx * g.ny > (1 << 20) / 2 and g.inv_cell == float(np.float32(1.0 / g.cell))
    assert g.wall_cells_host[0].tolist() == [0, 0, int(1 // g.cell), int(1 // g.cell)]
    assert g.wall_cells_host[1].tolist() == [int(5000 // g.cell), int(5000 // g.cell), g.nx - 1, g.ny - 1]


def test_bad_inputs_raise_value_errors():
    import socialways_amd as sw
    from socialways_amd import data
    ok = np.zeros((3, 4), np.float32)
    for kw in (dict(walls=np.zeros((3, 3))), dict(walls=np.zeros((3, 2, 3))), dict(walls=np.full((3, 4), np.nan)),
               dict(walls=np.full((3, 4), np.inf)), dict(reach=0.0), dict(reach=-1.0), dict(reach=math.nan), dict(reach=math.inf),
               dict(reach=1e30), dict(reach=1e-30), dict(cell=0.0), dict(cell=-1.0), dict(cell=math.nan), dict(cell=math.inf)):
        a = dict(walls=ok, reach=0.5, cell=None, device="cpu")
        a.update(kw)
        with pytest.raises(ValueError):
            sw.WallGrid(**a)
    g = _grid(WR.walls_case(8, 12, 33, 1)["walls"], cell=1.0)
    args = lambda **kw: dict(dict(cell_ptr=g.cell_ptr_host.copy(), cell_walls=g.cell_walls_host.copy(),  # noqa: E731
                                  wall_cells=g.wall_cells_host.copy(), nx=g.nx, ny=g.ny, M=g.M), **kw)
    data.check_wall_grid(**args())
    down = g.cell_ptr_host.copy()
    k = int(np.nonzero(np.diff(down) > 0)[0][0])
    down[k + 1] = down[k] - 1
    short = g.cell_ptr_host.copy()
    short[-1] -= 1
    hi, lo = g.cell_walls_host.copy(), g.cell_walls_host.copy()
    hi[0], lo[-1] = g.M, -1
    out_x, out_y, swapped, neg = (g.wall_cells_host.copy() for _ in range(4))
    out_x[0, 2], out_y[1, 3], neg[2, 0] = g.nx, g.ny, -1
    swapped[3] = [2, 0, 1, 0]
    for kw in (dict(cell_ptr=down), dict(cell_ptr=short), dict(cell_ptr=g.cell_ptr_host[:-1]), dict(cell_walls=hi), dict(cell_walls=lo),
               dict(wall_cells=out_x), dict(wall_cells=out_y), dict(wall_cells=neg), dict(wall_cells=swapped),
               dict(wall_cells=g.wall_cells_host[:-1]), dict(nx=0), dict(nx=1 << 11, ny=1 << 10)):
        with pytest.raises(ValueError):
            data.check_wall_grid(**args(**kw))


def test_tensors_keep_their_cap_and_wall_maps_stay_refused():
    import socialways_amd as sw
    from socialways_amd import ops
    assert "WallGrid" in sw.__all__ and "trace_occupancy" in sw.__all__ and "load_occupancy" in sw.__all__
    big = torch.zeros(1025, 2, 2)
    with pytest.raises(ValueError, match="1024"):
        ops.check_walls(big)
    tr = object.__new__(sw.SocialWaysTrainer)
    tr.device = torch.device("cpu")
    with pytest.raises(ValueError, match="1024"):
        tr.set_wall_loss(big, 0.2)
    g = _grid(big)                                               # the same walls under a grid are fine
    assert g.M == 1025
    with pytest.raises(ValueError):
        ops.check_walls(g)                                       # check_walls keeps refusing anything but a tensor
    maps = sw.WallMaps([np.zeros((2, 4)), np.zeros((1, 4))], device="cpu")
    for call in (lambda: ops.check_walls(maps), lambda: ops.walls_arg(maps, "cpu"), lambda: tr.set_wall_loss(maps, 0.2),
                 lambda: sw.WallGrid(maps, 0.5, device="cpu")):
        with pytest.raises((ValueError, TypeError)):
            call()
    assert ops.walls_arg(g, "cpu") is g, "a WallGrid passes through"


# ---- the model: every pair within reach is visited, none twice -----------------------------------------------------------------
@pytest.mark.parametrize("R,Tp,M", [(65, 12, 1500), (70, 12, 33)])
def test_the_rule_visits_every_pair_within_reach_exactly_once(R, Tp, M):
    case = WR.walls_case(R, Tp, M, 1)
    P = G.paths_points(*WR.split_case(case, True))
    need = G.within_reach(P, case["walls"], np.float32(REACH))
    assert need.sum() > (500 if M > 1000 else 20)
    for cell in (0.5, 1.0, 3.0, 1e6):
        g = _grid(case["walls"], cell=cell)
        table, most, total = G.visit_table(P, g)
        assert most == 1, "a pair is visited twice at cell %g" % cell
        assert not (need & ~table).any(), "%d pairs within reach are not visited at cell %g" % ((need & ~table).sum(), cell)
        print("wall grid model  R %d, Tp %d, M %d, cell %g: %d x %d cells, %d of %d pairs visited, %d within reach"
              % (R, Tp, M, cell, g.nx, g.ny, total, table.size, need.sum()))
        if cell == 1e6:
            assert (g.nx, g.ny) == (1, 1) and table.all(), "one cell visits all pairs"
        elif M > 1000:
            assert total < 0.05 * table.size


def test_nan_and_huge_points_index_nothing_out_of_range():
    case = WR.walls_case(8, 12, 33, 1)
    g = _grid(case["walls"], cell=0.5)
    inside = case["walls"][0, 0]
    nan, huge = np.float32(np.nan), np.float32(1e30)
    assert G.visited((nan, nan), (nan, nan), g) == [] and G.query_range((nan, 0), (nan, 0), g)[2] == -1
    for p0, p1 in (((huge, huge), (huge, huge)), ((-huge, 0), (-huge, 0)), ((np.inf, 0), (np.inf, 0)), ((-np.inf, -np.inf), (0, 0))):
        qx0, qy0, qx1, qy1 = G.query_range(p0, p1, g)
        assert 0 <= qx0 <= g.nx and -1 <= qx1 <= g.nx - 1 and 0 <= qy0 <= g.ny and -1 <= qy1 <= g.ny - 1
    assert G.query_range((np.inf, 0), (np.inf, 0), g)[0] == g.nx and G.query_range((-np.inf, 0), (-np.inf, 0), g)[2] == -1, \
        "an infinite coordinate stays finite under the slack: an empty range on its side, not the whole grid"
    big = type(g)(np.array([[0, 0, 1e-30, 1e-30]], np.float32), 1e-18, 1e-30, device="cpu")      # inv_cell 1e30: c overflows
    assert G.query_range((1e20, 0), (1e20, 0), big)[0] == big.nx and G.visited((1e20, 0), (1e20, 0), big) == []
    assert G.visited((huge, huge), (huge, huge), g) == [] and G.visited((-huge, 0), (-huge, 0), g) == []
    q = G.query_range(inside, (huge, huge), g)                   # from inside the grid to 1e30: the rest of the grid, no more
    assert q[2:] == (g.nx - 1, g.ny - 1) and sorted(G.visited(inside, (huge, huge), g)) == sorted(set(G.visited(inside, (huge, huge), g)))
    assert G.query_range(inside, (nan, nan), g) == G.query_range(inside, inside, g), "min / max return the operand that is not NaN"


# ---- the C entries ---------------------------------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments_before_the_device():
    from socialways_amd import _lib as L
    lib = L.load()
    assert "sw_path_walls_grid" in L.PROTOTYPES and "sw_wall_grad_grid" in L.PROTOTYPES
    buf = (ctypes.c_float * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15
    EARG = -1

    def pw(pos=p, pstride=2, start=None, sstride=0, K=1, B=2, Tp=4, walls=p, M=3, ptr=p, lst=p, wc=p, nx=2, ny=3, x0=0.0, y0=0.0,
           inv_cell=1.0, reach=0.6, inv_ss=1.0, dist=0.5, clear=p, first=p, nseg=p):
        return lib.sw_path_walls_grid(pos, pstride, start, sstride, None, K, B, Tp, walls, M, ptr, lst, wc, nx, ny, x0, y0, inv_cell,
                                      reach, inv_ss, dist, clear, first, nseg, None)

    def wg(pos=p, pstride=2, start=None, sstride=0, K=1, B=2, Tp=4, walls=p, M=3, ptr=p, lst=p, wc=p, nx=2, ny=3, x0=0.0, y0=0.0,
           inv_cell=1.0, reach=0.6, dw=0.5, scale=1.0, dpos=p, dstride=2):
        return lib.sw_wall_grad_grid(pos, pstride, start, sstride, None, K, B, Tp, walls, M, ptr, lst, wc, nx, ny, x0, y0, inv_cell,
                                     reach, dw, scale, dpos, dstride, None, None, None)
    shared = [dict(pos=None), dict(walls=None), dict(ptr=None), dict(lst=None), dict(wc=None), dict(K=0), dict(B=-1), dict(Tp=0),
              dict(M=-1), dict(pstride=3), dict(pos=p + 4), dict(start=p, sstride=1), dict(walls=p + 8), dict(wc=p + 8), dict(nx=0),
              dict(ny=0), dict(nx=-1), dict(nx=1 << 11, ny=(1 << 9) + 1), dict(x0=math.nan), dict(y0=math.inf), dict(inv_cell=0.0),
              dict(inv_cell=-1.0), dict(inv_cell=math.nan), dict(inv_cell=math.inf), dict(reach=0.0), dict(reach=-1.0),
              dict(reach=math.nan), dict(reach=math.inf), dict(reach=1e30), dict(reach=1e-30)]
    for call, own in ((pw, [dict(clear=None), dict(first=None), dict(nseg=None), dict(inv_ss=0.0), dict(inv_ss=math.nan), dict(dist=-1.0),
                            dict(dist=math.nan), dict(dist=0.6), dict(dist=0.7), dict(dist=0.599999), dict(dist=1.0, inv_ss=1.6)]),
                      (wg, [dict(dpos=None), dict(dw=0.0), dict(dw=-1.0), dict(dw=math.inf), dict(dw=math.nan), dict(dw=1e-30),
                            dict(scale=math.inf), dict(scale=math.nan), dict(dstride=1), dict(dstride=3), dict(dpos=p + 4),
                            dict(dw=0.6), dict(dw=0.7), dict(dw=0.599999)])):
        for kw in shared + own:
            assert call(**kw) == EARG, (call.__name__, kw)
            if "B" not in kw:
                assert call(B=0, **kw) == EARG, (call.__name__, kw, "the argument checks come before the empty batch")
        assert call(B=0) == 0 and call(B=0, M=0, walls=None, lst=None, wc=None, nx=1, ny=1) == 0, "an empty batch: SW_OK, no launch"
        assert call(B=0, M=1 << 20, nx=1 << 10, ny=1 << 10) == 0, "no cap on M; 2^20 cells are allowed"
    assert pw(B=0, dist=0.5999) == 0 and pw(B=0, dist=1.0, inv_ss=1.7) == 0 and wg(B=0, dw=0.5999) == 0, "just inside the margin"
    assert pw(B=0, dist=0.0) == 0


# ---- the Python layers -------------------------------------------------------------------------------------------------------------
def test_ops_and_stats_check_before_any_launch():
    import socialways_amd as sw
    from socialways_amd import ops, stats
    g = _grid(WR.walls_case(8, 12, 33, 1)["walls"], cell=1.0)
    pos, dpos = torch.zeros(6, 12, 4), torch.zeros(6, 12, 4)
    for bad in (dict(pos=torch.zeros(6, 12, 3)), dict(dpos=torch.zeros(6, 11, 4)), dict(start=torch.zeros(2, 2)), dict(loss=torch.zeros(5)),
                dict(dw=0.0), dict(dw=float("nan")), dict(scale=float("inf")), dict(lens=torch.zeros(3)), dict(K=4),
                dict(dw=0.55), dict(dw=0.6), dict(dw=REACH * (1 - 0.5e-5))):
        a = dict(pos=pos, start=None, K=2, walls=g, dw=0.5, scale=1.0, dpos=dpos, loss=None, count=None, lens=None)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.wall_grad(**a)
    for bad in (dict(pos=torch.zeros(6, 12, 3)), dict(start=torch.zeros(2, 2)), dict(dist=-1.0), dict(inv_ss=0.0), dict(lens=torch.zeros(3)),
                dict(K=4), dict(dist=0.6), dict(dist=1.0, inv_ss=1.8), dict(dist=0.55)):
        a = dict(pos=pos, start=None, K=2, walls=g, dist=0.5, inv_ss=1.0, lens=None)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.path_walls(**a)
    with pytest.raises(ValueError, match="reach"):
        ops.wall_grad(pos, None, 2, g, 0.6, 1.0, dpos)
    for call in (lambda: ops.wall_grad(pos, None, 2, g, 0.5, 1.0, dpos), lambda: ops.path_walls(pos, None, 2, g, 0.5),
                 lambda: ops.path_walls(pos, None, 2, g, 1.0, inv_ss=2.0),
                 lambda: stats.path_walls(torch.zeros(5, 12, 2), g, 0.5, device="cpu"),
                 lambda: stats.wall_penalty(torch.zeros(2, 5, 12, 2), g, 1.0, scale=2.0, device="cpu")):
        with pytest.raises(sw.SocialWaysHipError, match="MI355X"):
            call()                                               # everything checked: only the device is missing
    for call in (lambda: stats.path_walls(torch.zeros(5, 12, 2), g, 0.6, device="cpu"),
                 lambda: stats.path_walls(torch.zeros(5, 12, 3), g, 0.5, device="cpu"),
                 lambda: stats.wall_penalty(torch.zeros(5, 12, 2), g, 0.6, device="cpu"),
                 lambda: stats.wall_penalty(torch.zeros(5, 12, 2), g, 1.0, scale=1.5, device="cpu"),
                 lambda: stats.wall_penalty(torch.zeros(5, 12, 2), g, 0.5, start=torch.zeros(5, 3), device="cpu"),
                 lambda: stats.path_walls(torch.zeros(5, 12, 2), g, 0.5, device="meta")):
        with pytest.raises(ValueError):
            call()


def test_the_refinement_refuses_a_grid():
    import socialways_amd as sw
    from socialways_amd import ops, stats
    g = _grid(np.zeros((3, 4), np.float32))
    sc = ops.SceneIndex.get(scene_rows([4]), 4, "cpu")
    z = torch.zeros
    with pytest.raises(ValueError, match="WallGrid"):
        ops.plan_refine(z(4, 12, 2), z(4, 2), sc, 1, z(1, 1, 12, 2), z(1, 2), z(1, dtype=torch.int32), None, 0.5, walls=g)
    with pytest.raises(ValueError, match="WallGrid"):
        stats.refine_plans(z(4, 12, 2), [[0, 4]], z(1, 1, 12, 2), 0.5, z(1, 2), z(4, 2), device="cpu", walls=g)
    tr = object.__new__(sw.SocialWaysTrainer)
    tr.device, tr.n_next = torch.device("cpu"), 12
    with pytest.raises(ValueError, match="WallGrid"):
        tr.refine_plans(z(4, 8, 2), z(1, 1, 12, 2), 4, 0.5, sub_batches=[[0, 4]], plan_start=z(1, 2), walls=g)
    with pytest.raises(ValueError, match="WallGrid"):
        tr.evaluate_refine(SimpleNamespace(ss=0.25, obs_len=None), walls=g)


def test_set_wall_loss_holds_the_grid_and_the_step_checks_the_reach():
    import socialways_amd as sw
    from socialways_amd import generic, wide
    from socialways_amd.trainer import _wall_reach
    g = _grid(np.zeros((3, 4), np.float32))
    tr = object.__new__(sw.SocialWaysTrainer)
    tr.device = torch.device("cpu")
    tr.set_wall_loss(g, 2.0, 1.5)
    assert tr.wall_loss[0] is g and tr.wall_loss[1:] == (2.0, 1.5)
    for dist, weight in ((0.0, 1.0), (float("nan"), 1.0), (2.0, -1.0)):
        with pytest.raises(ValueError):
            tr.set_wall_loss(g, dist, weight)
    assert tr.wall_loss[0] is g
    _wall_reach(tr.wall_loss, 0.25)                              # dw = 0.5 < 0.55
    _wall_reach(None, 1.0)
    _wall_reach((torch.zeros(3, 2, 2), 2.0, 1.0), 100.0)         # a tensor has no reach
    o, p, z = torch.zeros(4, 8, 2), torch.zeros(4, 12, 2), torch.zeros(4, 32)
    for ss in (0.275, 0.3, 1.0):
        with pytest.raises(ValueError, match="reach"):
            tr.step(o, p, [[0, 4]], 0.0, 1.0, z, ss)             # refused before the trainer is touched: it has no state here
        with pytest.raises(ValueError, match="reach"):
            tr.step_many([(o, p, 0.0, 1.0, z)] * 2, [[0, 4]], ss)
    with pytest.raises(ValueError, match="reach"):
        tr.evaluate_walls(SimpleNamespace(ss=0.25), g, wall_dist=2.4)
    with pytest.raises(ValueError):
        tr.evaluate_walls(SimpleNamespace(ss=0.25), g, wall_dist=-1.0)
    far = sw.WallGrid(np.zeros((3, 4), np.float32), REACH, device="meta")
    with pytest.raises(ValueError, match="device"):
        tr.set_wall_loss(far, 2.0)
    for cls in (generic.GenericTrainer, wide.WideTrainer):
        t = object.__new__(cls)
        t.device = torch.device("cpu")
        with pytest.raises(sw.SocialWaysHipError, match="wall"):
            t.set_wall_loss(g, 0.2)


def test_the_graph_key_tells_grids_dists_and_weights_apart():
    from socialways_amd.trainer import _wall_key
    case = WR.walls_case(8, 12, 33, 1)
    a, b = _grid(case["walls"]), _grid(case["walls"])
    assert _wall_key(None) is None
    assert _wall_key((a, 0.2, 1.0)) == a.key() + (0.2, 1.0) and len(a.key()) == 11
    keys = {_wall_key(w) for w in ((a, 0.2, 1.0), (b, 0.2, 1.0), (a, 0.3, 1.0), (a, 0.2, 0.5))}
    assert len(keys) == 4
    t = torch.zeros(5, 2, 2)
    assert _wall_key((t, 0.2, 1.0)) == (t.data_ptr(), 5, 0.2, 1.0), "unchanged for tensors"


def test_wall_grid_from_world_goes_through_the_scale():
    import socialways_amd as sw
    rng = np.random.RandomState(0)
    o, p = rng.uniform(0, 20, (6, 8, 2)), rng.uniform(0, 20, (6, 12, 2))
    data = sw.SceneDataset(o, p, [[0, 3], [3, 6]], device="cpu")
    seg = rng.uniform(0, 20, (50, 4)).astype(np.float32)
    g = data.wall_grid_from_world(seg, 2.0, 4.0)
    assert torch.equal(g.walls, data.walls_from_world(seg)) and g.reach == float(np.float32(2.0 * data.ss))
    assert g.cell == 4.0 * float(data.ss) and g.M == 50
    assert data.wall_grid_from_world(seg, 2.0).cell == 4.0 * g.reach
    G.check_builder(g)


# ---- the tracer ----------------------------------------------------------------------------------------------------------------
def _length(segs):
    return float(np.abs(segs[:, 2:] - segs[:, :2]).sum())


def test_the_tracer_on_images_whose_boundary_is_known():
    import socialways_amd as sw
    for occ in (np.zeros((5, 7), bool), np.zeros((0, 0), bool)):
        assert sw.trace_occupancy(occ).shape == (0, 4) and sw.trace_occupancy(occ).dtype == np.float32
    full = np.ones((5, 7), bool)
    segs = sw.trace_occupancy(full)
    assert segs.tolist() == [[0, 0, 7, 0], [0, 5, 7, 5], [0, 0, 0, 5], [7, 0, 7, 5]] and _length(segs) == 24
    assert G.check_trace(segs, full) == (2, 2)
    one = np.zeros((4, 6), bool)
    one[2, 3] = True                                             # pixel (r 2, c 3) covers [3, 4] x [2, 3]
    segs = sw.trace_occupancy(one)
    assert segs.tolist() == [[3, 2, 4, 2], [3, 3, 4, 3], [3, 2, 3, 3], [4, 2, 4, 3]] and G.check_trace(segs, one) == (2, 2)
    board = np.add.outer(np.arange(4), np.arange(4)) % 2 == 0
    segs = sw.trace_occupancy(board)
    assert len(segs) == 14 and _length(segs) == 32 and G.check_trace(segs, board) == (7, 7)
    ring = np.ones((6, 6), bool)
    ring[2:4, 2:4] = False                                       # a hole has a boundary of its own
    assert len(sw.trace_occupancy(ring)) == 8 and G.check_trace(sw.trace_occupancy(ring), ring) == (4, 4)
    for bad in (np.zeros((3, 3)), np.zeros((3,), bool), np.zeros((2, 2, 2), bool)):
        with pytest.raises(ValueError):
            sw.trace_occupancy(bad)


def test_the_homography_is_applied_to_the_end_points():
    import socialways_amd as sw
    occ = np.zeros((4, 6), bool)
    occ[1:3, 2:5] = True
    plain = sw.trace_occupancy(occ).astype(np.float64)
    H = np.array([[0.5, 0.1, 3.0], [-0.2, 0.25, -1.0], [0.01, 0.02, 1.0]])
    got = sw.trace_occupancy(occ, H)
    pts = np.concatenate([plain.reshape(-1, 2), np.ones((2 * len(plain), 1))], 1) @ H.T
    assert np.allclose(got, (pts[:, :2] / pts[:, 2:]).reshape(-1, 4), rtol=1e-6, atol=0) and got.dtype == np.float32
    assert np.array_equal(sw.trace_occupancy(occ, np.eye(3)), plain.astype(np.float32))
    with pytest.raises(ValueError):
        sw.trace_occupancy(occ, np.eye(2))


def test_the_seeded_image_needs_a_grid(tmp_path):
    import socialways_amd as sw
    from socialways_amd.data import synth_occupancy
    occ = synth_occupancy(0)
    assert occ.shape == (480, 640) and occ.dtype == np.bool_ and np.array_equal(occ, synth_occupancy(0)) and 0.05 < occ.mean() < 0.6
    segs = sw.trace_occupancy(occ)
    nh, nv = G.check_trace(segs, occ)
    print("traced map  480 x 640, 40 rectangles, 30 discs: %d runs (%d horizontal, %d vertical) from %d unit edges"
          % (len(segs), nh, nv, G.boundary_edges(occ)))
    assert len(segs) > 1024
    with pytest.raises(ValueError, match="1024"):
        sw.stats.path_walls(torch.zeros(5, 12, 2), segs, 4.0, device="cpu")      # a flat call refuses that map
    g = sw.WallGrid(segs, 8.0, device="cpu")
    assert g.M == len(segs) and g.cell == 32.0
    # load_occupancy: a .npy always - boolean as it is, grey levels against the threshold
    np.save(tmp_path / "occ.npy", occ)
    np.save(tmp_path / "grey.npy", np.where(occ, 200, 30).astype(np.uint8))
    assert np.array_equal(sw.load_occupancy(str(tmp_path / "occ.npy")), occ)
    assert np.array_equal(sw.load_occupancy(str(tmp_path / "grey.npy")), occ)
    assert np.array_equal(sw.load_occupancy(str(tmp_path / "grey.npy"), threshold=201), np.zeros_like(occ))
    assert np.array_equal(sw.load_occupancy(str(tmp_path / "grey.npy"), invert=True), ~occ)
    np.save(tmp_path / "cube.npy", np.zeros((2, 2, 2)))
    with pytest.raises(ValueError):
        sw.load_occupancy(str(tmp_path / "cube.npy"))
    try:
        from PIL import Image
    except ImportError:
        with pytest.raises(ValueError, match="PIL"):
            sw.load_occupancy(str(tmp_path / "map.png"))
    else:
        Image.fromarray(np.where(occ, 255, 0).astype(np.uint8)).save(tmp_path / "map.png")
        assert np.array_equal(sw.load_occupancy(str(tmp_path / "map.png")), occ)
