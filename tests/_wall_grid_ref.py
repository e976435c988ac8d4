"""The grid of socialways_amd.WallGrid as a numpy model, written from the GRID comment of include/socialways_hip.h alone: the
query range of a path segment (in fp32, with the slack of the header) and the visit-once rule, which together say WHICH walls
sw_path_walls_grid / sw_wall_grad_grid look at for a segment and in which order; and the properties of trace_occupancy().
test_wall_grid_host.py (CPU) holds the model to the float64 distances of tests/_walls_ref.py; test_gpu_wall_grid.py holds the
kernels to the float64 references of tests/_wall_loss_ref.py and tests/_walls_ref.py, which are imported, not copied."""
import numpy as np

import _wall_loss_ref as WR  # noqa: F401  (the float64 penalty reference and its cases)
import _walls_ref as W

F = np.float32
SLACK = F(2.0 ** -21)
CMAX = F(2.0 ** 22)
MARGIN = 1e-5                  # dw and dist / inv_ss stay below reach by this relative margin


# ---- the query range --------------------------------------------------------------------------------------------------------
def axis_range(a, b, org, inv_cell, reach, n):
    """The cells 0 .. n - 1 of one axis a segment with the coordinates a, b asks about -> (q0, q1), empty when q0 > q1: fp32,
    expression by expression as the header writes it; the clamps come before the conversion to int."""
    a, b, org, inv_cell, reach = F(a), F(b), F(org), F(inv_cell), F(reach)
    with np.errstate(invalid="ignore", over="ignore"):
        bias = np.abs(org) * inv_cell
        lo, hi = (b if np.isnan(a) else a if np.isnan(b) else min(a, b)), (b if np.isnan(a) else a if np.isnan(b) else max(a, b))
        c0, c1 = F(F(F(lo - reach) - org) * inv_cell), F(F(F(hi + reach) - org) * inv_cell)
        c0, c1 = (-CMAX if np.isnan(c) else min(max(c, -CMAX), CMAX) for c in (c0, c1))      # finite before the slack
        f0 = np.floor(F(c0 - F(SLACK * F(np.abs(c0) + bias))))
        f1 = np.floor(F(c1 + F(SLACK * F(np.abs(c1) + bias))))
    q0 = 0.0 if np.isnan(f0) else min(max(float(f0), 0.0), float(n))
    q1 = -1.0 if np.isnan(f1) else min(max(float(f1), -1.0), float(n - 1))
    return int(q0), int(q1)


def query_range(p0, p1, grid):
    """-> (qx0, qy0, qx1, qy1) of the segment p0 -> p1 under a WallGrid (or anything with its attributes)"""
    qx0, qx1 = axis_range(p0[0], p1[0], grid.origin[0], grid.inv_cell, grid.reach, grid.nx)
    qy0, qy1 = axis_range(p0[1], p1[1], grid.origin[1], grid.inv_cell, grid.reach, grid.ny)
    return qx0, qy0, qx1, qy1


def visited(p0, p1, grid):
    """The walls the segment visits, in the order of the walk: cells row-major (iy outer, ix inner), a cell's list ascending,
    wall m only in the first cell of the intersection of its range with the query's."""
    qx0, qy0, qx1, qy1 = query_range(p0, p1, grid)
    ptr, lst, wc = grid.cell_ptr_host, grid.cell_walls_host, grid.wall_cells_host
    out = []
    for iy in range(qy0, qy1 + 1):
        for ix in range(qx0, qx1 + 1):
            c = iy * grid.nx + ix
            ms = lst[ptr[c]:ptr[c + 1]]
            out.extend(ms[(np.maximum(wc[ms, 0], qx0) == ix) & (np.maximum(wc[ms, 1], qy0) == iy)].tolist())
    return out


def paths_points(pos, start):
    """pos (K, B, Tp, >= 2), start (B, >= 2) or None -> points (K * B, NP, 2) float32 with the start in front"""
    pos = np.asarray(pos, np.float32)[..., :2]
    K, B = pos.shape[:2]
    P = pos.reshape(K * B, pos.shape[2], 2)
    if start is not None:
        st = np.broadcast_to(np.asarray(start, np.float32)[None, :, None, :2], (K, B, 1, 2)).reshape(K * B, 1, 2)
        P = np.concatenate([st, P], 1)
    return P


def visit_table(P, grid):
    """P (R, NP, 2) -> (table bool (R, NP - 1, M): the pair is visited; the largest number of visits of one pair; visits in
    all)"""
    R, NP = P.shape[:2]
    n = np.zeros((R, NP - 1, max(grid.M, 1)), np.int64)
    for r in range(R):
        for j in range(NP - 1):
            for m in visited(P[r, j], P[r, j + 1], grid):
                n[r, j, m] += 1
    return n[:, :, :grid.M] > 0, int(n.max(initial=0)), int(n.sum())


def within_reach(P, walls, reach):
    """float64: the pairs (R, NP - 1, M) with |c|^2 < reach^2"""
    walls = np.asarray(walls, np.float64).reshape(-1, 2, 2)
    P = np.asarray(P, np.float64)
    out = np.zeros((P.shape[0], P.shape[1] - 1, walls.shape[0]), bool)
    for r in range(P.shape[0]):
        cc = W.closest(P[r, :-1, None], P[r, 1:, None], walls[None, :, 0], walls[None, :, 1], np.float64)[2]
        out[r] = cc < float(reach) ** 2
    return out


# ---- the builder ------------------------------------------------------------------------------------------------------------
def listed_cells(grid):
    """-> per wall the set of cells (ix, iy) that list it, from the lists alone"""
    out = [set() for _ in range(grid.M)]
    ptr, lst = grid.cell_ptr_host, grid.cell_walls_host
    for c in range(grid.nx * grid.ny):
        for m in lst[ptr[c]:ptr[c + 1]]:
            assert (c % grid.nx, c // grid.nx) not in out[m], "a wall twice in one cell"
            out[m].add((c % grid.nx, c // grid.nx))
    return out


def check_builder(grid):
    """Wall m is listed in exactly the cells of its range, the range holds its bounding box, the lists ascend."""
    ptr, lst, wc = grid.cell_ptr_host, grid.cell_walls_host, grid.wall_cells_host
    assert ptr.dtype == lst.dtype == wc.dtype == np.int32 and ptr.shape == (grid.nx * grid.ny + 1,) and wc.shape == (grid.M, 4)
    assert ptr[0] == 0 and ptr[-1] == len(lst) == grid.L and (np.diff(ptr) >= 0).all()
    for c in range(grid.nx * grid.ny):
        assert (np.diff(lst[ptr[c]:ptr[c + 1]]) > 0).all(), "the indices ascend within a cell"
    cells = listed_cells(grid)
    walls = grid.walls.cpu().numpy().astype(np.float64)
    org = np.asarray(grid.origin)
    for m in range(grid.M):
        ix0, iy0, ix1, iy1 = (int(v) for v in wc[m])
        assert 0 <= ix0 <= ix1 < grid.nx and 0 <= iy0 <= iy1 < grid.ny
        assert cells[m] == {(ix, iy) for ix in range(ix0, ix1 + 1) for iy in range(iy0, iy1 + 1)}
        lo, hi = (walls[m].min(0) - org) / grid.cell, (walls[m].max(0) - org) / grid.cell
        want0 = np.clip(np.floor(lo), 0, [grid.nx - 1, grid.ny - 1])
        want1 = np.clip(np.floor(hi), 0, [grid.nx - 1, grid.ny - 1])
        assert (ix0, iy0) == tuple(want0.astype(int)) and (ix1, iy1) == tuple(want1.astype(int))


# ---- the tracer ----------------------------------------------------------------------------------------------------------------
def boundary_edges(occ):
    """The number of unit edges with exactly one occupied side, counted with np.diff on the padded array."""
    P = np.pad(np.asarray(occ, bool), 1).astype(np.int8)
    return int(np.abs(np.diff(P, axis=0)).sum() + np.abs(np.diff(P, axis=1)).sum())


def check_trace(segs, occ):
    """Integer axis-aligned runs, total length = the boundary edges, no two runs on one line touch or overlap, horizontal runs
    ordered by (y, x0), then vertical ones by (x, y0) -> (number of horizontal runs, of vertical runs)."""
    segs = np.asarray(segs)
    assert segs.dtype == np.float32 and segs.ndim == 2 and segs.shape[1] == 4
    assert (segs == np.round(segs)).all()
    s = segs.astype(np.int64)
    hor = s[:, 1] == s[:, 3]
    nh = int(hor.sum())
    assert hor[:nh].all() and not hor[nh:].any(), "horizontal runs first"
    ver = s[nh:]
    assert (ver[:, 0] == ver[:, 2]).all() and (s[:nh, 2] > s[:nh, 0]).all() and (ver[:, 3] > ver[:, 1]).all()
    assert int((s[:nh, 2] - s[:nh, 0]).sum() + (ver[:, 3] - ver[:, 1]).sum()) == boundary_edges(occ)
    for line, a, b in ((s[:nh, 1], s[:nh, 0], s[:nh, 2]), (ver[:, 0], ver[:, 1], ver[:, 3])):
        key = list(zip(line.tolist(), a.tolist()))
        assert key == sorted(key), "the order rule"
        same = line[1:] == line[:-1]
        assert (a[1:][same] > b[:-1][same]).all(), "two runs on one line touch: they are not maximal"
    return nh, len(s) - nh
