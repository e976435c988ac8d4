"""Maps of any size on the GPU: sw_path_walls_grid / sw_wall_grad_grid behind socialways_amd.WallGrid against the float64
references of tests/_wall_loss_ref.py and tests/_walls_ref.py, against the flat kernels wherever a map fits them, and through
stats, SocialWaysTrainer.step() and evaluate_walls().

a. float64  WR.pick_case / reference / compare at reach 0.55, cell 1.0: (R, Tp, M) = (65, 12, 1500), (2 x 65, 12, 2049) ragged with
            NaN behind the lengths, (64, 17, 1025) without start at pstride 4 / dstride 4, (65, 40, 1500) ragged over three time
            chunks, (70, 12, 33), (1, 1, 5), (63, 12, 0); dpos zero and pre-filled.  Bound: max|err| <= 2e-5 max|ref| (GRAD_REL) for
            dpos and loss, count equal off the near mask; split-ambiguous paths at most 5 %, near ones at most 1 % of a case.
b. flat     M = 33, 130, 1024 on the _wall_loss_ref inputs and every case of _walls_ref.path_cases(), at cell 0.5, 1 and one
            cell: count, nseg and first equal exactly; clear bit-equal where the flat clear / inv_ss < reach, +inf elsewhere.
c. beyond   M = 2049 against the flat kernels on three slices of the walls: nseg and count the sums, first the smallest
            non-negative one, clear the minimum under the saturation rule.
d. exact    two calls, a path alone / in its batch / with the others permuted, the same integers and clear at every cell, rows
            with count 0 and paths outside the grid untouched, a point at 1e30 and NaN padding, posts at reach (1 - 1e-6) and at
            dw (1 - 1e-6) from segments that straddle a cell line; a wall EXACTLY dist, dw and reach away (no conflict, no pair,
            clear +inf; profiles/seeded_faults_r2.txt), a segment whose query range loses the post's cell without the slack.
e. stats    stats.path_walls / stats.wall_penalty = the ops calls, bit for bit.
f. step     the setup of test_gpu_wall_loss.py part d with its 5 walls in a WallGrid: generator gradients against step64 + the
            float64 gradient of L_wall at that test's bound, D's gradients and the loss rows bit-identical to the step without the
            term; eager, captured, step_many of 3, ragged, ragged_fused captured, both terms on; the flat tensor agrees.
g. evaluate_walls on tests/golden/biwi_synth.npz: the box of the true futures as a WallGrid and as a tensor, every number equal.

Everything here fails without WallGrid.  Observed on an MI355X (pytest -s), largest max|err| / max|ref|: a. dpos 9.88e-7 (R 64, Tp 17,
M 1025), loss 1.86e-7 (R 65, Tp 40, M 1500), every count equal; no near path, 2 / 2 / 1 / 1 / 1 split-ambiguous paths in the first
five rows at seed 1.  b. integers and clear equal everywhere, dpos / loss against the flat kernels 2.09e-7.  d. between cells 7.34e-8,
the rest exact.  f. generator gradients: eager 3.86e-6, graph 1.96e-5, step_many 4.34e-6, ragged 5.18e-6, ragged_fused 3.59e-6, both
terms 3.79e-6; outputs 3.4e-7; grid against the flat tensor 5.75e-7, counts equal; no ambiguous unit.  The 34 cases take 10.6 s
together.  """
import numpy as np
import pytest
import torch

import _step_ref as S
import _wall_grid_ref as G
import _wall_loss_ref as WR
import _walls_ref as W
import test_gpu_wall_loss as TW
from _ref64 import GRAD_REL, _close_grad, _note, _report  # noqa: F401
from test_gpu_clearance_loss import DIST as CDIST, WEIGHT as CWEIGHT, _col_ref
from test_gpu_ragged_train import dev_len
from test_gpu_step_reference import SS, _names, _step, calls, rule_a  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DW, REACH, CELL = WR.DW, 0.55, 1.0
CELLS = (0.5, 1.0, 1e6)                  # 1e6: one cell
_bits, _widen = TW._bits, TW._widen


def _grid(walls, reach=REACH, cell=CELL):
    import socialways_amd as sw
    return sw.WallGrid(walls, reach, cell, device=DEV)


def _dev(x, dtype=None):
    return None if x is None else torch.as_tensor(x, dtype=dtype).to(DEV)


def _as_map(walls):
    return walls if not isinstance(walls, np.ndarray) else _dev(walls.reshape(-1, 2, 2), torch.float32)


def _grad(pos, start, K, walls, dw, scale, dpos, lens=None):
    """ops.wall_grad with a tensor map or a WallGrid -> (loss, count), NaN / -1 where the kernel did not write"""
    from socialways_amd import ops
    R = dpos.shape[0] * (dpos.shape[1] if dpos.dim() == 4 else 1)
    loss = torch.full((R,), float("nan"), device=DEV)
    count = torch.full((R,), -1, dtype=torch.int32, device=DEV)
    ops.wall_grad(_dev(pos), _dev(start), K, _as_map(walls), dw, scale, dpos, loss, count, _dev(lens))
    torch.cuda.synchronize()
    return loss, count


def _pw(pos, start, K, walls, dist, inv_ss=1.0, lens=None):
    from socialways_amd import ops
    out = ops.path_walls(_dev(pos), _dev(start), K, _as_map(walls), dist, inv_ss, lens=_dev(lens))
    torch.cuda.synchronize()
    return tuple(o.reshape(-1) for o in out)


def _saturate(clear, inv_ss, reach):
    """The documented difference: the flat clear where clear / inv_ss < reach, +inf elsewhere"""
    return torch.where(clear / inv_ss < reach, clear, torch.full_like(clear, float("inf")))


# ---- a. against float64 -----------------------------------------------------------------------------------------------------------
# (K, B, Tp, M, with_start, ragged, pstride, dstride)
ROWS = [(1, 65, 12, 1500, True, False, 2, 2), (2, 65, 12, 2049, True, True, 2, 2), (1, 64, 17, 1025, False, False, 4, 4),
        (1, 65, 40, 1500, True, True, 2, 2), (1, 70, 12, 33, True, False, 2, 2), (1, 1, 1, 5, True, False, 2, 2),
        (1, 63, 12, 0, True, False, 2, 2)]
_picked = {}


def _case(row):
    """WR.pick_case for a row, computed once and left unchanged"""
    if row[:6] not in _picked:
        K, B, Tp, M, with_start, ragged = row[:6]
        _picked[row[:6]] = WR.pick_case(K * B, Tp, M, K, with_start, WR.ragged_lens if ragged else None)
    return _picked[row[:6]]


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "k%d_b%d_tp%d_m%d_%s%s_p%dd%d" % (
    r[0], r[1], r[2], r[3], "start" if r[4] else "nostart", "_ragged" if r[5] else "", r[6], r[7]))
def test_kernel_against_float64(row):
    K, B, Tp, M, with_start, ragged, pstride, dstride = row
    case, pos, start, lens, ref = _case(row)
    R, tag = K * B, "%s, seed %d" % (row, case["seed"])
    assert ref["split"].sum() <= WR.CAP_SPLIT * R and ref["near"].sum() <= WR.CAP_NEAR * R
    grid = _grid(case["walls"])
    assert grid.M == M
    p = _widen(pos, pstride, 7.0)
    if ragged:
        for a in range(B):
            p[:, a, int(np.clip(lens[a], 1, Tp)):] = float("nan")
    p = p.to(DEV)
    gmax = float(np.abs(ref["grad"]).max())
    scale = 2.0 / gmax if gmax > 0 else 1.0
    gen = torch.Generator().manual_seed(case["seed"])
    for what, pre in (("dpos from zero", torch.zeros(R, Tp, 2)), ("dpos accumulated", torch.randn(R, Tp, 2, generator=gen))):
        before = _widen(pre, dstride, 3.0).reshape(K, B, Tp, dstride)
        dpos = before.to(DEV)
        loss, count = _grad(p, start, K, grid, DW, scale, dpos, lens)
        got = dpos.cpu()
        err, lerr = WR.compare(got[..., :2].numpy(), loss.cpu().numpy(), count.cpu().numpy(), ref, scale, pre.numpy())
        print("wall grid kernel  %-52s %-16s dpos %.2e  loss %.2e  (split %d, near %d, active %d of %d; %d x %d cells, L %d)"
              % (tag, what, err, lerr, ref["split"].sum(), ref["near"].sum(), ref["active"].sum(), R, grid.nx, grid.ny, grid.L))
        _note("a.kernel", "grad", err)
        _note("a.kernel", "out", lerr)
        if dstride == 4:
            assert bool((got[..., 2:] == 3.0).all()), "columns 2 and 3 of dpos (%s)" % tag
        if ragged:
            for a in range(B):
                ln = int(np.clip(lens[a], 1, Tp))
                assert torch.equal(_bits(got[:, a, ln:]), _bits(before[:, a, ln:])), "rows behind a length are not written (%s)" % tag
    if M and Tp > 1:
        assert ref["active"].sum() >= 0.1 * R


# ---- b. against the flat kernels -----------------------------------------------------------------------------------------------
def _flat_and_grid(pos, start, K, walls, dist, inv_ss, lens, Tp, cells=CELLS):
    """path_walls and wall_grad (dw = dist / inv_ss) of the flat kernels and of the grid at every cell: integers equal, clear
    under the saturation rule, loss and dpos to rounding -> the flat (clear, first, nseg, count)"""
    R = int(np.prod(np.asarray(pos).shape[:-2]))
    B = R // K
    dw = dist / inv_ss
    reach = 1.1 * dw
    clear, first, nseg = _pw(pos, start, K, walls, dist, inv_ss, lens)
    d0 = torch.zeros(K, B, Tp, 2, device=DEV)
    loss, count = _grad(pos, start, K, walls, dw, 1.0, d0, lens)
    want_clear = _saturate(clear, inv_ss, float(np.float32(reach)))
    for cell in cells:
        grid = _grid(walls, reach, cell * dw / DW)
        c2, f2, n2 = _pw(pos, start, K, grid, dist, inv_ss, lens)
        assert torch.equal(n2, nseg) and torch.equal(f2, first), "nseg / first at cell %g" % cell
        assert torch.equal(_bits(c2), _bits(want_clear)), "clear at cell %g" % cell
        d1 = torch.zeros(K, B, Tp, 2, device=DEV)
        l2, k2 = _grad(pos, start, K, grid, dw, 1.0, d1, lens)
        assert torch.equal(k2, count), "count at cell %g" % cell
        if float(d0.abs().max()) > 0:
            _close_grad(d1, d0, "dpos, grid against flat", "b.flat", "cell %g" % cell)
            _close_grad(l2, loss, "loss, grid against flat", "b.flat", "cell %g" % cell)
        else:
            assert not bool(d1.any()) and not bool(l2.any())
    return clear, first, nseg, count


@pytest.mark.parametrize("M", [33, 130, 1024])
def test_integers_equal_the_flat_kernels(M):
    case = WR.walls_case(130, 12, M, 1)
    pos, start = WR.split_case(case, True)
    clear, first, nseg, count = _flat_and_grid(pos, start, 1, case["walls"], DW, 1.0, None, 12)
    assert int(nseg.sum()) > 0 and torch.equal(nseg, count) and bool((first >= 0).any())


@pytest.mark.parametrize("name,case", W.path_cases(), ids=[n for n, _ in W.path_cases()])
def test_path_cases_equal_the_flat_kernels(name, case):
    pos = case["pos"]
    clear, first, nseg, _ = _flat_and_grid(pos, case["start"], case["K"], case["walls"], case["dist"], case["inv_ss"], case["lens"],
                                           case["Tp"])
    if case["M"] >= 33 and (case["Tp"] > 1 or case["start"] is not None):
        assert int(nseg.sum()) > 0, "the case has hits"


# ---- c. beyond the cap -----------------------------------------------------------------------------------------------------------
def test_a_map_beyond_the_cap_is_the_sum_of_its_slices():
    row = ROWS[1]
    K, B, Tp, M = row[:4]
    case, pos, start, lens, ref = _case(row)
    p = torch.as_tensor(pos).clone()
    for a in range(B):
        p[:, a, int(np.clip(lens[a], 1, Tp)):] = float("nan")
    walls = case["walls"]
    parts = [walls[0:683], walls[683:1366], walls[1366:2049]]
    assert M == 2049 and all(len(w) <= 1024 for w in parts)
    flat = [_pw(p, start, K, w, DW, 1.0, lens) for w in parts]
    cnt = [_grad(p, start, K, w, DW, 1.0, torch.zeros(K, B, Tp, 2, device=DEV), lens)[1] for w in parts]
    big = torch.full_like(flat[0][1], 0x7fffffff)
    first = torch.stack([torch.where(f[1] >= 0, f[1], big) for f in flat]).min(0).values
    first = torch.where(first == 0x7fffffff, torch.full_like(first, -1), first)
    clear = _saturate(torch.stack([f[0] for f in flat]).min(0).values, 1.0, float(np.float32(REACH)))
    grid = _grid(walls)
    c2, f2, n2 = _pw(p, start, K, grid, DW, 1.0, lens)
    k2 = _grad(p, start, K, grid, DW, 1.0, torch.zeros(K, B, Tp, 2, device=DEV), lens)[1]
    assert torch.equal(n2, sum(f[2] for f in flat)) and torch.equal(k2, sum(cnt)) and int(n2.sum()) > 0
    assert torch.equal(f2, first) and torch.equal(_bits(c2), _bits(clear))
    assert bool(torch.isfinite(c2).any())


# ---- d. exactness -----------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_a_path_does_not_see_the_batch():
    case = WR.walls_case(130, 25, 1500, 1)
    pos, start = WR.split_case(case, True)
    pos, grid = pos[0], _grid(case["walls"])

    def run(rows):
        dpos = torch.zeros(len(rows), 25, 4, device=DEV)
        loss, count = _grad(_widen(pos[rows], 4, 7.0), start[rows], 1, grid, DW, 0.5, dpos)
        return (dpos, loss, count) + _pw(_widen(pos[rows], 4, 7.0), start[rows], 1, grid, DW)
    every = np.arange(130)
    one, two = run(every), run(every)
    assert bool(one[0].any()) and int(one[2].sum()) > 0 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(one, two))
    perm = np.random.RandomState(3).permutation(130)
    pt = torch.as_tensor(perm).to(DEV)
    assert all(torch.equal(_bits(a), _bits(b[pt])) for a, b in zip(run(perm), one))
    r = int(np.nonzero(one[2].cpu().numpy() > 0)[0][-1])           # an active path, alone: another lane, another workgroup
    assert r >= 64
    assert all(torch.equal(_bits(a[0]), _bits(b[r])) for a, b in zip(run(np.array([r])), one))
    # K = 2: the second draw of agent a is row B + a and reads start[a]
    dk = torch.zeros(2, 130, 25, 4, device=DEV)
    lk, ck = _grad(_widen(np.stack([pos, pos]), 4, 7.0), start, 2, grid, DW, 0.5, dk)
    assert torch.equal(_bits(dk[0]), _bits(one[0])) and torch.equal(_bits(dk[1]), _bits(one[0])) and torch.equal(ck[130:], one[2])


def test_the_cell_changes_only_the_order_of_the_sums():
    case = WR.walls_case(130, 17, 1500, 1)
    pos, start = WR.split_case(case, True)
    outs = []
    for cell in (0.5, 1.0, 3.0, 1e6):
        grid = _grid(case["walls"], cell=cell)
        dpos = torch.zeros(130, 17, 2, device=DEV)
        loss, count = _grad(pos[0], start, 1, grid, DW, 1.0, dpos)
        outs.append((dpos, loss, count) + _pw(pos[0], start, 1, grid, DW))
    assert int(outs[0][2].sum()) > 0
    for o in outs[1:]:
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(o[2:], outs[0][2:])), "count, clear, first, nseg at every cell"
        _close_grad(o[0], outs[0][0], "dpos at another cell", "d.exact", "cells")
        _close_grad(o[1], outs[0][1], "loss at another cell", "d.exact", "cells")


def test_rows_with_nothing_counted_and_paths_outside_the_grid_are_not_touched():
    case, pos, _, _, ref = WR.gpu_case(1, 130, 12, 5, False, False)
    idle = (ref["count"] == 0) & ~ref["near"]
    assert 20 <= idle.sum() <= 110
    pre = torch.randn(130, 12, 4, generator=torch.Generator().manual_seed(4))
    pre[:, 0, 0], pre[:, 3, 1], pre[:, :, 3] = -0.0, float("nan"), float("nan")
    grid = _grid(case["walls"])
    dpos = pre.to(DEV)
    loss, count = _grad(pos[0], None, 1, grid, DW, 1.0, dpos)
    idle_t = _dev(idle)
    assert torch.equal(_bits(dpos[idle_t]), _bits(pre.to(DEV)[idle_t])), "rows of paths with every |c| >= dw"
    assert not bool(loss[idle_t].any()) and not bool(count[idle_t].any()) and bool((count[~idle_t] > 0).any())
    assert not torch.equal(_bits(dpos[~idle_t][..., :2]), _bits(pre.to(DEV)[~idle_t][..., :2]))
    assert torch.equal(_bits(dpos[..., 2:]), _bits(pre[..., 2:].to(DEV))), "columns 2 and 3, NaN included"
    # wholly outside the grid, on every side and far away: nothing visited, nothing written, clear +inf
    shift = np.array([[100.0, 0.0], [-100.0, 0.0], [0.0, 100.0], [0.0, -100.0], [3e4, -3e4]], np.float32)
    out = (pos[0, :5] + shift[:, None]).astype(np.float32)
    dpos = pre[:5].to(DEV)
    loss, count = _grad(out, None, 1, grid, DW, 1.0, dpos)
    clear, first, nseg = _pw(out, None, 1, grid, DW)
    assert torch.equal(_bits(dpos), _bits(pre[:5].to(DEV))) and not bool(loss.any()) and not bool(count.any())
    assert bool(torch.isinf(clear).all()) and bool((first == -1).all()) and not bool(nseg.any())
    empty = _grid(np.zeros((0, 4), np.float32))                    # M = 0: every row
    dpos = pre.to(DEV)
    loss, count = _grad(pos[0], None, 1, empty, DW, 1.0, dpos)
    assert torch.equal(_bits(dpos), _bits(pre.to(DEV))) and not bool(loss.any()) and not bool(count.any())
    assert bool(torch.isinf(_pw(pos[0], None, 1, empty, DW)[0]).all())


def test_a_point_at_1e30_and_nan_padding_reach_nothing():
    case = WR.walls_case(70, 12, 33, 1)
    pos, start = WR.split_case(case, True)
    pos = pos[0].copy()
    lens = np.full(70, 12, np.int32)
    lens[:35] = np.random.RandomState(5).randint(1, 12, 35)
    cut = pos.copy()
    for a in range(35):
        cut[a, lens[a]:] = np.nan if a % 2 else 1e30              # behind a length: never looked at
    cut[40, 5], cut[41, 0], cut[42, 11] = 1e30, -1e30, [1e30, np.nan]      # inside the length: the flat kernels' numbers
    grid = _grid(case["walls"])
    dg, df = torch.zeros(70, 12, 2, device=DEV), torch.zeros(70, 12, 2, device=DEV)
    lg, cg = _grad(cut, start, 1, grid, DW, 1.0, dg, lens)
    lf, cf = _grad(cut, start, 1, case["walls"], DW, 1.0, df, lens)
    assert torch.equal(cg, cf) and int(cg[:35].sum()) > 0
    pg, pf = _pw(cut, start, 1, grid, DW, 1.0, lens), _pw(cut, start, 1, case["walls"], DW, 1.0, lens)
    assert torch.equal(pg[1], pf[1]) and torch.equal(pg[2], pf[2])
    assert torch.equal(_bits(pg[0]), _bits(_saturate(pf[0], 1.0, float(np.float32(REACH)))))
    ref = WR.reference(pos, start, case["walls"], DW, lens, want_masks=True)      # the clean paths: the float64 numbers
    clean = np.ones(70, bool)
    clean[40:43] = False
    keep = clean & ~ref["near"]
    assert np.array_equal(cg.cpu().numpy()[keep], ref["count"][keep])
    assert bool(torch.isfinite(dg[_dev(clean)]).all()) and bool(torch.isfinite(lg[_dev(clean)]).all())
    for a in range(35):
        assert not bool(dg[a, lens[a]:].any()), "rows behind a length"


def test_walls_just_inside_the_reach_across_a_cell_line_are_visited():
    """Posts at the distance d (1 - 1e-6), d = reach and d = dw, from segments that cross the cell line x = 3, y = 4 or the corner (7, 7) of a grid
    with cell 1 over [0, 10]^2: above, below, beyond either end and off a corner, so that the post lies in another cell than
    either end of the segment.  Built in float64, checked against the float64 distance after the rounding to fp32."""
    segs = np.array([[[2.8, 4.3], [3.2, 4.3]], [[6.3, 3.8], [6.3, 4.2]], [[6.9, 6.9], [7.1, 7.1]]])
    for d in (REACH, DW):
        e = d * (1 - 1e-6)
        posts, owner = [], []
        for i, (a, b) in enumerate(segs):
            t = (b - a) / np.linalg.norm(b - a)
            n = np.array([-t[1], t[0]])
            for q in ((a + b) / 2 + e * n, (a + b) / 2 - e * n, a - e * t, b + e * t, a - e * (t + n) / np.sqrt(2), b + e * (t - n) / np.sqrt(2)):
                posts.append([q, q])
                owner.append(i)
        walls = np.concatenate([np.array(posts), [[[0, 0], [0, 0]], [[10, 10], [10, 10]]]]).astype(np.float32)
        pos = segs[:, 1:].astype(np.float32)                       # one segment per path: start -> pos[0]
        start = segs[:, 0].astype(np.float32)
        near = G.within_reach(G.paths_points(pos[None], start), walls, np.float32(REACH))[:, 0]
        assert all(near[owner[k], k] for k in range(len(owner))), "the posts are within reach in float64"
        grid = _grid(walls)
        assert (grid.nx, grid.ny) == (11, 11)
        dist = 0.9 * REACH
        flat, got = _pw(pos, start, 1, walls, dist), _pw(pos, start, 1, grid, dist)
        assert torch.equal(got[1], flat[1]) and torch.equal(got[2], flat[2]) and torch.equal(_bits(got[0]), _bits(flat[0]))
        assert bool((got[0] < REACH).all()) and bool((got[0] > 0.9 * d).all())
        df, dg = torch.zeros(3, 1, 2, device=DEV), torch.zeros(3, 1, 2, device=DEV)
        cf, cg = _grad(pos, start, 1, walls, DW, 1.0, df)[1], _grad(pos, start, 1, grid, DW, 1.0, dg)[1]
        assert torch.equal(cf, cg), "counted as the flat kernel counts them"
        if d == DW:
            assert int(cg.sum()) >= 12, "posts at dw (1 - 1e-6) are counted"
            assert int(_pw(pos, start, 1, grid, DW)[2].sum()) == int(_pw(pos, start, 1, walls, DW)[2].sum()) >= 12


def _one_segment():
    """(0, 0.5) -> (1, 0.5), no start point, above a wall on the x axis: |c|^2 = 0.25 exactly (asserted in float64)"""
    pos, walls = np.array([[[0.0, 0.5], [1.0, 0.5]]], np.float32), np.array([[[-1.0, 0.0], [2.0, 0.0]]], np.float32)
    assert float(W.closest(pos[0, 0].astype(np.float64), pos[0, 1].astype(np.float64), walls[0, 0], walls[0, 1])[2]) == 0.25
    return pos, walls


def test_a_wall_exactly_dist_or_dw_away_is_no_conflict_and_no_pair():
    """The strictness of `< dist` and `< dw` where the reference's margin is 0: at dist = 0.5 the pair is no conflict (nseg 0,
    first -1), at dw = 0.5 it is not counted and the pre-filled -0.0 of its dpos rows keeps its bits (a `+= 0` would leave +0.0);
    at 0.75 both count it, the gradient against the float64 reference."""
    pos, walls = _one_segment()
    grid = _grid(walls, reach=1.0)
    assert G.visited(pos[0, 0], pos[0, 1], grid) == [0]
    assert W.path_walls_reference(pos[None], None, walls, 0.5)["margin"] == 0.0
    clear, first, nseg = _pw(pos, None, 1, grid, 0.5)
    assert float(clear[0]) == 0.5 and int(first[0]) == -1 and int(nseg[0]) == 0
    clear, first, nseg = _pw(pos, None, 1, grid, 0.75)
    assert float(clear[0]) == 0.5 and int(first[0]) == 1 and int(nseg[0]) == 1
    ref = WR.reference(pos, None, walls, 0.5)
    assert ref["count"][0] == 0 and not ref["grad"].any()
    dpos = torch.full((1, 2, 2), -0.0, device=DEV)
    loss, count = _grad(pos, None, 1, grid, 0.5, 1.0, dpos)
    assert int(count[0]) == 0 and float(loss[0]) == 0.0
    assert torch.equal(_bits(dpos), _bits(torch.full((1, 2, 2), -0.0, device=DEV))), "a pair that is not counted makes no read-modify-write"
    ref = WR.reference(pos, None, walls, 0.75)
    assert ref["count"][0] == 1 and abs(ref["grad"][0, 0, 1]) > 1.0
    dpos = torch.zeros(1, 2, 2, device=DEV)
    loss, count = _grad(pos, None, 1, grid, 0.75, 1.0, dpos)
    WR.compare(dpos.cpu().numpy(), loss.cpu().numpy(), count.cpu().numpy(), ref)


def test_clear_saturates_at_a_wall_exactly_reach_away():
    """reach = 0.5 and the only wall at distance 0.5 exactly: the wall is visited (the numpy model of the walk says so) and
    clear is +inf, `|c|^2 < reach^2` being strict; with a second wall at distance 0.25 it is 0.25."""
    pos, walls = _one_segment()
    grid = _grid(walls, reach=0.5)
    assert G.visited(pos[0, 0], pos[0, 1], grid) == [0] and grid.reach == 0.5
    clear, first, nseg = _pw(pos, None, 1, grid, 0.25)
    assert float(clear[0]) == float("inf") and int(first[0]) == -1 and int(nseg[0]) == 0
    both = np.concatenate([walls, [[[-1.0, 0.25], [2.0, 0.25]]]]).astype(np.float32)
    grid = _grid(both, reach=0.5)
    assert sorted(G.visited(pos[0, 0], pos[0, 1], grid)) == [0, 1]
    clear, first, nseg = _pw(pos, None, 1, grid, 0.25)
    assert float(clear[0]) == 0.25 and int(first[0]) == -1 and int(nseg[0]) == 0
    clear, first, nseg = _pw(pos, None, 1, grid, 0.375)
    assert float(clear[0]) == 0.25 and int(first[0]) == 1 and int(nseg[0]) == 1


def test_the_slack_of_the_query_range_keeps_a_cell_the_fp32_floor_loses():
    """A case where the slack of wq_axis decides an output.  Found on the CPU by a vectorised twin of G.axis_range over random
    (v, reach, x0, cell) - cell uniform in 0.05 .. 2, reach / cell in 0.25 .. 1, |x0| / cell log-uniform in 1e3 .. 1e5, the post's
    cell k log-uniform up to 3e5, the post on the first fp32 number inside cell k and the path's end v the first fp32 number
    within reach (1 - 1e-5) of it - RandomState(1), the first hit among the first 1e6 candidates: the upper side's
    c = ((v + reach) - x0) * fl(1 / cell) comes out below k = 13187 by the rounding of the product at |c| ~ 1.3e4, the float64
    quotient lies above it.  Here the model says so with the slack and without, and the kernels are held to the flat ones."""
    v, reach, x0, cell, k, post = -12390.9951171875, 1.8098340034484863, -38694.34375, 1.994779558380387, 13187, -12389.185546875
    walls = np.array([[[x0, 0.0], [x0, 0.0]], [[post, 0.0], [post, 0.0]]], np.float32)
    pos, start = np.array([[[v, 0.0]]], np.float32), np.array([[v - 0.5, 0.0]], np.float32)
    assert float(pos[0, 0, 0]) == v and float(walls[1, 0, 0]) == post and float(np.float32(reach)) == reach
    grid = _grid(walls, reach=reach, cell=cell)
    assert grid.cell == cell and (grid.nx, grid.ny) == (k + 1, 1) and tuple(grid.wall_cells_host[1]) == (k, 0, k, 0)
    d = (post - v) / reach
    assert 0.999 < d <= 1 - 1e-5, "the post is within reach (1 - 1e-5) of the path's end in float64"
    assert G.axis_range(v - 0.5, v, x0, grid.inv_cell, reach, grid.nx)[1] >= k and G.visited(start[0], pos[0, 0], grid) == [1]
    slack, G.SLACK = G.SLACK, np.float32(0)
    try:
        assert G.axis_range(v - 0.5, v, x0, grid.inv_cell, reach, grid.nx)[1] == k - 1, "without the slack the post's cell is not asked about"
    finally:
        G.SLACK = slack
    dist, dw = 0.9 * reach, 0.9999 * reach
    flat, got = _pw(pos, start, 1, walls, dist), _pw(pos, start, 1, grid, dist)
    want = W.path_walls_reference(pos[None], start, walls, dist)
    assert abs(float(want["clear"][0, 0]) - (post - v)) < 1e-12 and int(want["nseg"][0, 0]) == 0
    assert bool(torch.isfinite(got[0]).all()) and torch.equal(_bits(got[0]), _bits(flat[0])), "clear is the flat kernel's: the post was visited"
    assert torch.equal(got[1], flat[1]) and torch.equal(got[2], flat[2])
    ref = WR.reference(pos, start, walls, dw)
    assert ref["count"][0] == 1 and not WR.reference(pos, start, walls, dw, want_masks=True)["near"][0]
    # u = 1 - |c|^2 / dw^2 is 9e-5 here, a difference of two fp32 numbers near 1: the count is held to float64, dpos and
    # loss to the flat kernel by the rule of part b
    df, dg = torch.zeros(1, 1, 2, device=DEV), torch.zeros(1, 1, 2, device=DEV)
    (lf, cf), (lg, cg) = _grad(pos, start, 1, walls, dw, 1.0, df), _grad(pos, start, 1, grid, dw, 1.0, dg)
    assert int(cg[0]) == int(cf[0]) == ref["count"][0] and bool(dg.any())
    _close_grad(dg, df, "dpos, grid against flat", "d.exact", "slack")
    _close_grad(lg, lf, "loss, grid against flat", "d.exact", "slack")


# ---- e. stats -----------------------------------------------------------------------------------------------------------------------
def test_stats_forms_are_the_ops_calls():
    from socialways_amd import stats
    case = WR.walls_case(3 * 43, 12, 1500, 1, K=3)
    pos, start = WR.split_case(case, True)
    scale, dist = 4.0, 2.0                                         # trajs in quarter units: dw = dist / scale in theirs
    lens = np.random.RandomState(2).randint(1, 13, 43)
    grid = _grid(case["walls"])
    loss, grad, count = stats.wall_penalty(pos, grid, dist, start=start, scale=scale, lens=lens, device=DEV)
    dpos = torch.zeros(3, 43, 12, 2, device=DEV)
    l2, c2 = _grad(pos, start, 3, grid, dist / scale, 1.0, dpos, lens.astype(np.int32))
    assert grad.shape == (3, 43, 12, 2) and loss.shape == count.shape == (3, 43) and count.dtype == torch.int32 and bool(grad.any())
    assert torch.equal(_bits(grad), _bits(dpos)) and torch.equal(_bits(loss.reshape(-1)), _bits(l2)) and torch.equal(count.reshape(-1), c2)
    clear, first, nseg = stats.path_walls(pos, grid, dist, start=start, scale=scale, lens=lens, device=DEV)
    c3, f3, n3 = _pw(pos, start, 3, grid, dist, scale, lens.astype(np.int32))
    assert clear.shape == (3, 43) and int(nseg.sum()) > 0
    assert torch.equal(_bits(clear.reshape(-1)), _bits(c3)) and torch.equal(first.reshape(-1), f3) and torch.equal(nseg.reshape(-1), n3)
    c4 = stats.path_walls(torch.as_tensor(pos[1]), grid, dist, scale=scale, device=DEV)[0]      # (B, .), no start
    assert c4.shape == (43,) and torch.equal(_bits(c4), _bits(_pw(pos[1], None, 1, grid, dist, scale)[0]))
    with pytest.raises(ValueError, match="reach"):
        stats.wall_penalty(pos, grid, 2.4, scale=scale, device=DEV)


# ---- f. the step ------------------------------------------------------------------------------------------------------------------
def _on(c):
    """the case's 5 walls under a grid, switched on"""
    c.grid = _grid(c.walls)
    c.tr.set_wall_loss(c.grid, TW.DIST, TW.WEIGHT)
    assert c.tr.wall_loss[0] is c.grid
    return c


def test_step_eager_with_the_grid_and_with_the_tensor(calls):
    c = TW._case(on=False, use_graph=False)
    _step(c, 0)
    out0 = _step(c, 0).clone()
    d0, g0 = S.trainer_grads(c.tr)
    _on(c)
    del calls[:]
    out1 = _step(c, 0).clone()
    d1, g1 = S.trainer_grads(c.tr)
    names = _names(calls)
    assert names.count("sw_wall_grad_grid") == 1 and "sw_wall_grad" not in names and "sw_dec_rollout_bwd_dfuse" not in names
    assert names.index("sw_disc_dpred") < names.index("sw_wall_grad_grid")
    TW._check_on(c, out1, 0, "grid eager")
    assert torch.equal(out0, out1), "the loss rows do not see the term"
    assert all(torch.equal(d0[k], d1[k]) for k in d0), "D's gradients do not see the term"
    assert any(not torch.equal(g0[k], g1[k]) for k in g0)
    lg, cg = (t.clone() for t in c.tr.last_wall_loss)
    c.tr.set_wall_loss(c.walls, TW.DIST, TW.WEIGHT)              # the same map as a tensor: the flat kernel
    del calls[:]
    out2 = _step(c, 0)
    d2, g2 = S.trainer_grads(c.tr)
    assert _names(calls).count("sw_wall_grad") == 1 and "sw_wall_grad_grid" not in _names(calls)
    assert torch.equal(out2, out1) and all(torch.equal(d2[k], d1[k]) for k in d1)
    assert torch.equal(c.tr.last_wall_loss[1], cg) and int(cg.sum()) > 0, "the counts are equal exactly"
    _close_grad(lg, c.tr.last_wall_loss[0], "last_wall_loss, grid against flat", "f.grid-flat", "eager")
    for k in g1:
        _close_grad(g1[k], g2[k], "d/d%s, grid against flat" % k, "f.grid-flat", "eager")
    with pytest.raises(ValueError, match="reach"):                  # dw = dist * ss beyond the reach: before any launch
        c.tr.set_wall_loss(c.grid, 2.3, TW.WEIGHT)
        del calls[:]
        _step(c, 0)
    assert not calls


def test_step_through_the_graph(calls):
    c = _on(TW._case(n_steps=5, on=False))
    assert c.tr.use_graph
    for i in range(5):
        del calls[:]
        out = _step(c, i)
        assert len(c.tr._graphs) == 1 and [k[-5] for k in c.tr._graphs] == [c.grid.key() + (TW.DIST, TW.WEIGHT)]
        st = next(iter(c.tr._graphs.values()))
        assert (st["graph"] is not None) == (i >= 2)
        if i >= 3:
            assert not calls, "a replayed step makes no launch of its own"
        elif i < 2:
            assert _names(calls).count("sw_wall_grad_grid") == 1
        TW._check_on(c, out, i, "grid graph")
    c.tr.set_wall_loss(_grid(c.walls), TW.DIST, TW.WEIGHT)          # another grid: another key
    _step(c, 0)
    assert len(c.tr._graphs) == 2


def test_step_many_of_three():
    c = _on(TW._case(n_steps=9, on=False))
    for r in range(3):
        outs = c.tr.step_many([c.device_draw(i) for i in range(3 * r, 3 * r + 3)], c.sb, SS)
        torch.cuda.synchronize()
        assert [k[5] for k in c.tr._graphs] == [3]
        assert (next(iter(c.tr._graphs.values()))["graph"] is not None) == (r >= 2)
        TW._check_on(c, outs[2], 3 * r + 2, "grid step_many, launch %d" % (r + 1))


def test_step_ragged(calls):
    c = _on(TW._case(lens=[rule_a(29)], on=False))
    out = _step(c, 0, obs_len=c.lens[0])
    assert not c.tr._graphs and "sw_disc_fwd_ragged" in _names(calls) and "sw_wall_grad_grid" in _names(calls)
    TW._check_on(c, out, 0, "grid ragged")


def test_step_ragged_fused_captured():
    c = _on(TW._case(n_steps=4, lens=[rule_a(29)] * 4, ragged_fused=True, on=False))
    for i in range(4):
        out = _step(c, i, obs_len=dev_len(c.lens[i]))
        st = next(iter(c.tr._graphs.values()))
        assert [k[-2] for k in c.tr._graphs] == [True] and (st["graph"] is not None) == (i >= 2)
        if i >= 2:
            TW._check_on(c, out, i, "grid ragged_fused, %s" % ("captured" if i == 2 else "replayed"))


def test_both_terms_on(calls):
    c = TW._case(on=False, use_graph=False)
    c.tr.set_clearance_loss(CDIST, CWEIGHT)
    _step(c, 0)
    _on(c)
    del calls[:]
    out = _step(c, 0)
    names = _names(calls)
    assert names.index("sw_disc_dpred") < names.index("sw_clearance_grad") < names.index("sw_wall_grad_grid")
    TW._check_on(c, out, 0, "grid both terms", also=_col_ref(c, 0)[0])


# ---- g. evaluate_walls --------------------------------------------------------------------------------------------------------------
def test_evaluate_walls_with_a_grid_equals_the_tensor():
    import socialways_amd as sw
    from _util import golden
    g = golden("biwi_synth")
    data = sw.SceneDataset(g["obsvs"], g["preds"], g["batches"], g["times"], device=DEV)
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(data.pred.shape[1], use_social=True, device=DEV)
    lo, hi = g["preds"].reshape(-1, 2).min(0), g["preds"].reshape(-1, 2).max(0)
    box = np.array([[lo[0], lo[1], hi[0], lo[1]], [hi[0], lo[1], hi[0], hi[1]], [hi[0], hi[1], lo[0], hi[1]], [lo[0], hi[1], lo[0], lo[1]]],
                   np.float32)
    grid = data.wall_grid_from_world(box, 0.5)
    assert isinstance(grid, sw.WallGrid) and grid.M == 4
    torch.manual_seed(31)
    want = tr.evaluate_walls(data, data.walls_from_world(box), n_gen_samples=20, wall_dist=0.3)
    torch.manual_seed(31)
    records = []
    got = tr.evaluate_walls(data, grid, n_gen_samples=20, wall_dist=0.3, collect=records)
    assert got == want and got["wall_draws"] > 0
    clear = np.concatenate([r["wall_clear"] for r in records], 1)
    assert clear.shape[0] == 20 and (clear[np.isfinite(clear)] <= 0.5 * (1 + 1e-5)).all(), "clear saturates at the reach (world units)"
    with pytest.raises(ValueError, match="reach"):
        tr.evaluate_walls(data, grid, n_gen_samples=20, wall_dist=0.5)
