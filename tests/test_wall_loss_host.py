"""The wall term of the generator loss without a GPU: the float64 reference of tests/_wall_loss_ref.py against itself (the
closed form the kernel implements, autograd of the torch.where form, central differences, a crossing, the threshold), the caps
on split-ambiguous and near paths for every case test_gpu_wall_loss.py uses, and the host surface of the feature - the argument
checks of sw_wall_grad / ops.wall_grad / stats.wall_penalty, set_wall_loss(), the refusals of the wide and generic trainers,
the place of the setting in the graph key and the signatures."""
import ctypes
import inspect
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _wall_loss_ref as WR
from _ref64 import scene_rows


def _autograd(pos, start, walls, dw):
    q = torch.tensor(pos, dtype=torch.float64, requires_grad=True)
    st = None if start is None else torch.tensor(start, dtype=torch.float64)
    loss, count = WR.penalty_torch(q, st, walls, dw)
    loss.sum().backward()
    return loss.detach().numpy(), count.numpy(), q.grad.numpy()


@pytest.mark.parametrize("with_start", [True, False])
@pytest.mark.parametrize("Tp,M", [(1, 5), (12, 5), (17, 33), (12, 1)])
def test_closed_form_equals_autograd(Tp, M, with_start):
    case = WR.walls_case(40, Tp, M, 3)
    pos, start = WR.split_case(case, with_start)
    ref = WR.reference(pos, start, case["walls"], case["dw"])
    loss, count, g = _autograd(pos[0], start, case["walls"], case["dw"])
    if Tp > 1 or with_start:
        assert int(count.sum()) > 0 and float(np.abs(g).max()) > 0, "the case has counted pairs"
    else:
        assert not count.any() and not g.any(), "a path of one point has no segment"
    assert np.array_equal(count, ref["count"])
    assert float(np.abs(loss - ref["loss"]).max()) <= 1e-10 * max(float(ref["loss"].max()), 1.0)
    assert float(np.abs(g - ref["grad"]).max()) <= 1e-10 * max(float(np.abs(g).max()), 1.0)


def test_lens_and_draws_gate_the_reference():
    """K = 3 draws share their agents' start points; what lies behind a length, NaN included, is never read; a length beyond Tp
    and one below 1 are clamped."""
    case = WR.walls_case(3 * 7, 12, 9, 5, K=3)
    pos, start = WR.split_case(case, True)
    lens = WR.ragged_lens(case, np.random.RandomState(0))
    full = WR.reference(pos, start, case["walls"], case["dw"], None, 3)
    cut = pos.copy()
    for a in range(7):
        cut[:, a, int(np.clip(lens[a], 1, 12)):] = np.nan
    rag = WR.reference(cut, start, case["walls"], case["dw"], lens, 3)
    assert np.isfinite(rag["grad"]).all() and rag["count"].sum() < full["count"].sum()
    assert np.array_equal(rag["grad"][0], full["grad"][0]) and rag["count"][6] <= full["count"][6]      # len 17 -> 12, 0 -> 1
    for r in range(21):
        ln = int(np.clip(lens[r % 7], 1, 12))
        assert not rag["grad"][r, ln:].any()
        one = WR.reference(pos[r // 7, r % 7, :ln][None], start[r % 7][None], case["walls"], case["dw"])
        assert one["loss"][0] == rag["loss"][r] and np.array_equal(one["grad"][0], rag["grad"][r, :ln])


def test_closed_form_equals_central_differences():
    case = WR.walls_case(24, 5, 40, 2)
    pos, start = WR.split_case(case, True)
    pos = pos.astype(np.float64)
    ref = WR.reference(pos, start, case["walls"], case["dw"], want_masks=True)
    clean = ~(ref["split"] | ref["near"]) & ref["active"]
    assert clean.sum() >= 5
    h, num = 1e-6, np.zeros_like(ref["grad"])
    for r in np.nonzero(clean)[0]:
        for i in range(5 * 2):
            e = np.zeros(10)
            e[i] = h
            e = e.reshape(1, 5, 2)
            up = WR.reference(pos[0, r][None] + e, start[r][None], case["walls"], case["dw"])["loss"][0]
            dn = WR.reference(pos[0, r][None] - e, start[r][None], case["walls"], case["dw"])["loss"][0]
            num[r].reshape(-1)[i] = (up - dn) / (2 * h)
    scale = float(np.abs(num).max())
    # phi is C1 with a bounded second derivative (curvature ~ 12 / dw^2): the central difference errs by O(h) only where a kink
    # of the clamps, of the candidate order or of the threshold lies within h, by O(h^2) elsewhere
    assert scale > 0 and float(np.abs(ref["grad"] - num)[clean].max()) <= 1e-4 * scale


def test_a_crossing_has_phi_one_and_no_gradient():
    walls = np.array([[[0.0, -1.0], [0.0, 1.0]]])
    pos = np.array([[[0.5, 0.25]]])                   # from (-0.5, 0.25): crosses the wall at s = 1/2, both ends at distance dw
    ref = WR.reference(pos, np.array([[-0.5, 0.25]]), walls, 0.5)
    assert ref["loss"][0] == 1.0 and ref["count"][0] == 1 and not ref["grad"].any()
    loss, count, g = _autograd(pos, np.array([[-0.5, 0.25]]), walls, 0.5)
    assert loss[0] == 1.0 and count[0] == 1 and not g.any()
    # a post on the path: distance 0 through candidate 3, no crossing - gradient 0 because c = 0
    post = WR.reference(pos, np.array([[-0.5, 0.25]]), np.array([[[0.25, 0.25], [0.25, 0.25]]]), 0.5)
    assert post["loss"][0] == 1.0 and not post["grad"].any()


def test_the_penalty_is_c1_at_the_threshold():
    """A point that passes a long wall at distance dw (1 -+ eps): phi and its gradient go to 0 like eps^2 and eps."""
    walls, dw = np.array([[[-5.0, 0.0], [5.0, 0.0]]]), 0.5
    for eps in (1e-3, 1e-5):
        inside = WR.reference(np.array([[[0.0, dw * (1 - eps)], [1.0, dw * (1 - eps)]]]), None, walls, dw)
        outside = WR.reference(np.array([[[0.0, dw * (1 + eps)], [1.0, dw * (1 + eps)]]]), None, walls, dw)
        assert inside["count"][0] == 1 and outside["count"][0] == 0 and outside["loss"][0] == 0 and not outside["grad"].any()
        assert 0 < inside["loss"][0] <= (2.1 * eps) ** 2 and 0 < np.abs(inside["grad"]).max() <= 4 * 2.1 * eps / dw


@pytest.mark.parametrize("row", WR.GPU_CASES, ids=lambda r: "k%d_b%d_tp%d_m%d_%s%s" % (r[0], r[1], r[2], r[3], "s" if r[4] else "n", "_rag" if r[5] else ""))
def test_caps_hold_for_every_gpu_case(row):
    K, B, Tp, M, with_start, ragged = row[:6]
    case, pos, start, lens, ref = WR.gpu_case(*row)
    R = K * B
    assert ref["split"].sum() <= WR.CAP_SPLIT * R and ref["near"].sum() <= WR.CAP_NEAR * R
    print("wall case %s: seed %d, split-ambiguous %d / %d, near %d, active %d" % (row[:6], case["seed"], ref["split"].sum(), R,
                                                                                  ref["near"].sum(), ref["active"].sum()))
    if M > 0 and (Tp > 1 or with_start):
        assert ref["active"].sum() >= (0.1 * R if M >= 5 else 2), "the case has active paths"
    else:
        assert not ref["active"].any()


# ---- the host surface ------------------------------------------------------------------------------------------------------------
def test_entry_point_checks_its_arguments_before_the_device():
    from socialways_amd import _lib as L
    lib = L.load()
    assert "sw_wall_grad" in L.PROTOTYPES
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def call(pos=p, pstride=2, start=None, sstride=0, K=1, B=2, Tp=4, walls=p, M=3, dw=0.5, scale=1.0, dpos=p, dstride=2):
        return lib.sw_wall_grad(pos, pstride, start, sstride, None, K, B, Tp, walls, M, dw, scale, dpos, dstride, None, None, None)
    EARG, ESHAPE = -1, lib.sw_path_walls(p, 2, None, 0, None, 1, 2, 4, p, 1025, 1.0, 0.5, p, p, p, None)
    assert ESHAPE not in (0, EARG)
    assert call(pos=None) == EARG and call(dpos=None) == EARG and call(walls=None) == EARG
    assert call(K=0) == EARG and call(B=-1) == EARG and call(Tp=0) == EARG and call(M=-1) == EARG
    for dw in (0.0, -1.0, math.inf, math.nan, 1e-30, 1e30):
        assert call(dw=dw) == EARG, dw
    assert call(scale=math.inf) == EARG and call(scale=math.nan) == EARG
    assert call(pstride=3) == EARG and call(dstride=1) == EARG and call(dstride=3) == EARG
    assert call(pos=p + 4) == EARG and call(dpos=p + 4) == EARG
    assert call(start=p, sstride=1) == EARG
    assert call(M=1025) == ESHAPE and call(M=1025, B=0) == ESHAPE
    for kw in (dict(dw=0.0), dict(dw=1e-30), dict(scale=math.nan), dict(pstride=3), dict(pos=p + 4), dict(dpos=p + 4), dict(start=p, sstride=1),
               dict(dstride=3)):
        assert call(M=1025, **kw) == EARG and call(B=0, **kw) == EARG, kw      # the argument checks come first
    assert call(B=0) == 0 and call(B=0, M=0, walls=None) == 0, "an empty batch is SW_OK without a launch"


def test_ops_and_stats_check_shapes_and_refuse_cpu_tensors():
    import socialways_amd as sw
    from socialways_amd import ops, stats
    pos, dpos, walls = torch.zeros(6, 12, 4), torch.zeros(6, 12, 4), torch.zeros(3, 2, 2)
    for bad in (dict(pos=torch.zeros(6, 12, 3)), dict(pos=torch.zeros(7, 12, 4)), dict(dpos=torch.zeros(6, 11, 4)),
                dict(dpos=torch.zeros(6, 12, 3)), dict(dpos=torch.zeros(5, 12, 4)), dict(start=torch.zeros(2, 2)),
                dict(start=torch.zeros(3, 1)), dict(loss=torch.zeros(5)), dict(count=torch.zeros(6)), dict(dw=0.0),
                dict(dw=float("nan")), dict(scale=float("inf")), dict(walls=torch.zeros(3, 4)), dict(walls=torch.zeros(1025, 2, 2)),
                dict(lens=torch.zeros(3)), dict(K=4), dict(pos=pos.double())):
        a = dict(pos=pos, start=None, K=2, walls=walls, dw=0.5, scale=1.0, dpos=dpos, loss=None, count=None, lens=None)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.wall_grad(**a)
    with pytest.raises(sw.SocialWaysHipError):
        ops.wall_grad(pos, torch.zeros(3, 2), 2, walls, 0.5, 1.0, dpos)
    for bad in (dict(trajs=torch.zeros(5, 12, 3)), dict(trajs=torch.zeros(12, 2)), dict(start=torch.zeros(5, 3)), dict(dist=0.0),
                dict(dist=float("inf")), dict(scale=0.0), dict(walls=np.zeros((3, 3))), dict(lens=[1] * 4)):
        a = dict(trajs=torch.zeros(5, 12, 2), walls=np.zeros((3, 4)), dist=0.5, device="cpu")
        a.update(bad)
        with pytest.raises(ValueError):
            stats.wall_penalty(**a)
    with pytest.raises(sw.SocialWaysHipError):
        stats.wall_penalty(torch.zeros(2, 5, 12, 2), np.zeros((0, 4)), 0.5, device="cpu")


def test_set_wall_loss_and_the_refusals():
    import socialways_amd as sw
    from socialways_amd import generic, wide
    assert sw.SocialWaysTrainer.wall_loss is None and sw.SocialWaysTrainer.last_wall_loss is None
    tr = object.__new__(sw.SocialWaysTrainer)
    tr.device = torch.device("cpu")
    tr.set_wall_loss([[0, 0, 1, 1], [2, 2, 2, 3]], 0.2)
    w, dist, weight = tr.wall_loss
    assert tuple(w.shape) == (2, 2, 2) and w.dtype == torch.float32 and (dist, weight) == (0.2, 1.0)
    mine = torch.zeros(4, 2, 2)
    tr.set_wall_loss(mine, np.float32(0.5), weight=0)
    assert tr.wall_loss[0].data_ptr() == mine.data_ptr(), "a tensor on the device is held, not copied"
    assert tr.wall_loss[1:] == (0.5, 0.0) and all(type(v) is float for v in tr.wall_loss[1:])
    tr.set_wall_loss(np.zeros((0, 4)), 0.5)
    assert tuple(tr.wall_loss[0].shape) == (0, 2, 2), "an empty map is accepted"
    held = tr.wall_loss
    for walls, dist, weight in ((mine, 0.0, 1.0), (mine, -1.0, 1.0), (mine, float("nan"), 1.0), (mine, float("inf"), 1.0),
                                (mine, 0.2, -0.1), (mine, 0.2, float("inf")), (mine, 0.2, float("nan")),
                                (torch.zeros(4, 3), 0.2, 1.0), (torch.zeros(2, 2, 3), 0.2, 1.0), (torch.zeros(1025, 2, 2), 0.2, 1.0)):
        with pytest.raises(ValueError):
            tr.set_wall_loss(walls, dist, weight)
    assert tr.wall_loss is held, "a refused value leaves the setting alone"
    tr.set_wall_loss(None)
    assert tr.wall_loss is None and tr.last_wall_loss is None
    for cls in (generic.GenericTrainer, wide.WideTrainer):
        t = object.__new__(cls)
        t.device = torch.device("cpu")
        assert t.wall_loss is None
        with pytest.raises(sw.SocialWaysHipError, match="wall"):
            t.wall_loss = (mine, 0.2, 1.0)
        with pytest.raises(sw.SocialWaysHipError, match="wall"):
            t.set_wall_loss(mine, 0.2)
        with pytest.raises(ValueError):
            t.set_wall_loss(mine, -1.0)
        t.set_wall_loss(None)
        t.wall_loss = None
        assert t.wall_loss is None


def test_graph_key_carries_the_setting_in_front_of_the_clearance_entry():
    from socialways_amd import ops
    from socialways_amd.trainer import SocialWaysTrainer
    grp = [{"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8}]
    fake = SimpleNamespace(predictor_optimizer=SimpleNamespace(param_groups=grp), D_optimizer=SimpleNamespace(param_groups=grp),
                           _row0=0, n_unrolling_steps=1, use_info_loss=True, loss_info_w=0.5, use_l2_loss=False,
                           use_variety_loss=False, loss_l2_w=0.5, variety_k=1, use_social=True)
    sc = ops.SceneIndex.get(scene_rows([8] * 4), 32, "cpu")
    key = lambda: SocialWaysTrainer._graph_key(fake, sc, 8, 1.0, 32.0, 3, False, False)  # noqa: E731
    off = key()                               # a namespace without the attribute: the term is off
    assert off[-5] is None and off[-4] is None and off[5] == 3 and off[-2:] == (False, False)
    fake.wall_loss, fake.clearance_loss = None, (0.2, 1.0)
    assert key()[-5] is None and key()[-4] == (0.2, 1.0)
    fake.clearance_loss = None
    a, b = torch.zeros(5, 2, 2), torch.zeros(7, 2, 2)
    keys = {off}
    for wall in ((a, 0.2, 1.0), (b, 0.2, 1.0), (a, 0.3, 1.0), (a, 0.2, 0.5), (a[:3], 0.2, 1.0)):
        fake.wall_loss = wall
        on = key()
        assert on[-5] == (wall[0].data_ptr(), wall[0].shape[0], wall[1], wall[2])
        assert len(on) == len(off) and on[:-5] == off[:-5] and on[-4:] == off[-4:]
        keys.add(on)
    assert len(keys) == 6


def test_signatures():
    from socialways_amd import ops, stats
    from socialways_amd.trainer import SocialWaysTrainer

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(ops.wall_grad) == [("pos", E), ("start", E), ("K", E), ("walls", E), ("dw", E), ("scale", E), ("dpos", E),
                                  ("loss", None), ("count", None), ("lens", None)]
    assert sig(stats.wall_penalty) == [("trajs", E), ("walls", E), ("dist", E), ("start", None), ("scale", 1.0), ("lens", None),
                                       ("device", "cuda")]
    assert sig(SocialWaysTrainer.set_wall_loss) == [("self", E), ("walls", E), ("dist", None), ("weight", 1.0)]
