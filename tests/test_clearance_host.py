"""The scene-clearance term without a GPU: the float64 reference of tests/_clear_ref.py against itself (autograd, the closed
form the kernel implements, central differences, shards, the dv = 0 definition) and the host surface of the feature - the
argument checks of sw_clearance_grad / ops.clearance_grad / stats.clearance_penalty, set_clearance_loss(), the refusals of the
wide and generic trainers and the place of the setting in the graph key."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _clear_ref as C
from _ref64 import scene_rows
from _step_ref import make_draws

SIZES = [1, 2, 8, 5, 3]
D0 = 0.6


def _walks(sizes, To, Tp, seed, dtype=torch.float64):
    o, p = make_draws(sizes, To, Tp)(seed)[0][:2]
    return o.to(dtype), p.to(dtype)


def _autograd(pos, start, sb, d0):
    q = pos.clone().requires_grad_(True)
    loss, count = C.penalty(q, start, sb, d0)
    loss.sum().backward()
    return loss.detach(), count, q.grad


@pytest.mark.parametrize("with_start", [True, False])
@pytest.mark.parametrize("Tp", [1, 12, 17])
def test_autograd_equals_the_closed_form(Tp, with_start):
    o, p = _walks(SIZES, 8, Tp, 3)
    sb, start = scene_rows(SIZES), (o[:, -1] if with_start else None)
    loss, count, g = _autograd(p, start, sb, D0)
    cf = C.closed_form_grad(p, start, sb, D0)
    assert cf.shape == g.shape == (sum(SIZES), Tp, 2)
    if Tp > 1 or with_start:
        assert float(g.abs().max()) > 0 and int(count.sum()) > 0, "the case has active pairs"
    assert float((g - cf).abs().max()) <= 1e-12 * max(float(g.abs().max()), 1.0)
    assert loss[0] == 0 and count[0] == 0 and not bool(g[0].any()), "a single-agent scene has no term"
    assert abs(float(loss[1] - loss[2])) <= 1e-14 * float(loss[1]) and torch.equal(cf[1], -cf[2]), "a two-agent scene is antisymmetric"


def test_both_agree_with_central_differences():
    o, p = _walks(SIZES, 8, 5, 5)
    sb, start = scene_rows(SIZES), o[:, -1]
    _, _, g = _autograd(p, start, sb, D0)
    cf = C.closed_form_grad(p, start, sb, D0)
    h, num = 1e-6, torch.zeros_like(p)
    for i in range(p.numel()):
        e = torch.zeros(p.numel(), dtype=p.dtype)
        e[i] = h
        e = e.view_as(p)
        num.view(-1)[i] = (C.penalty(p + e, start, sb, D0)[0].sum() - C.penalty(p - e, start, sb, D0)[0].sum()) / (2 * h)
    scale = float(num.abs().max())
    assert scale > 0
    # phi is C1 with a bounded second derivative (curvature ~ 12 / d0^2): the central difference errs by O(h) only where a
    # kink of the clamps or of the threshold lies within h, by O(h^2) elsewhere
    assert float((g - num).abs().max()) <= 1e-4 * scale and float((cf - num).abs().max()) <= 1e-4 * scale


def test_shards_add_up_to_the_full_batch():
    sizes, w = [3, 1, 4, 2, 6], 0.7
    o, p = _walks(sizes, 8, 12, 8)
    sb, B = scene_rows(sizes), sum(sizes)
    q = p.clone().requires_grad_(True)
    full = C.l_col(q, o[:, -1], sb, D0, w)
    full.backward()
    assert float(full.detach()) > 0
    total, g = 0.0, torch.zeros_like(p)
    for lo, hi in ((0, 2), (2, 5)):
        r0, r1 = int(sb[lo, 0]), int(sb[hi - 1, 1])
        qs = p[r0:r1].clone().requires_grad_(True)
        part = C.l_col(qs, o[r0:r1, -1], sb[lo:hi], D0, w, global_B=B, global_row0=r0)
        part.backward()
        total, g[r0:r1] = total + float(part.detach()), qs.grad
    assert abs(total - float(full.detach())) <= 1e-12 * float(full.detach())
    assert float((g - q.grad).abs().max()) <= 1e-12 * float(q.grad.abs().max())


def test_no_relative_motion_takes_tau_zero():
    """Two agents in parallel equal motion: dv = 0 in every segment, tau = 0 is the definition, c = r0."""
    a = torch.tensor([[0.0, 0.0], [0.5, 0.25], [1.0, 0.5], [1.5, 0.75]], dtype=torch.float64)
    P = torch.stack([a, a + torch.tensor([0.25, 0.0], dtype=torch.float64)])
    tau, c, cc, u = C.terms(P, 0.5)
    assert not bool(tau.any()) and torch.equal(c[0, 1], (P[0] - P[1])[:-1]) and bool((cc[0, 1] == 0.0625).all())
    loss, count, g = _autograd(P, None, [], 0.5)
    assert bool(torch.isfinite(g).all()) and count.tolist() == [3, 3] and float(loss[0]) == 0.5 * 3 * 0.75 ** 2
    cf = C.closed_form_grad(P, None, [], 0.5)
    assert torch.allclose(g, cf, rtol=0, atol=1e-15)
    assert not bool(cf[:, -1].any()) and bool(cf[:, 0].any()), "with tau = 0 a segment's gradient lands on its r0 end"
    # coincident agents: c = 0, gradient exactly 0 and finite
    z = C.closed_form_grad(torch.stack([a, a]), None, [], 0.5)
    assert not bool(z.any())


# ---- the host surface ------------------------------------------------------------------------------------------------------------
def test_entry_point_checks_its_arguments_before_the_device():
    from socialways_amd import _lib as L
    lib = L.load()
    assert "sw_clearance_grad" in L.PROTOTYPES
    buf = (ctypes.c_float * 64)()
    off = (ctypes.c_int * 2)(0, 2)
    p, so = ctypes.addressof(buf), ctypes.addressof(off)

    def call(pos=p, pstride=2, start=None, sstride=0, scene_off=so, S=1, B=2, Tp=4, d0=0.5, scale=1.0, dpos=p, dstride=2):
        return lib.sw_clearance_grad(pos, pstride, start, sstride, scene_off, S, B, Tp, d0, scale, dpos, dstride, None, None, None)
    assert call(pos=None) == -1 and call(dpos=None) == -1 and call(scene_off=None) == -1
    assert call(d0=0.0) == -1 and call(d0=-1.0) == -1 and call(d0=math.inf) == -1 and call(d0=math.nan) == -1
    assert call(pstride=3) == -1 and call(dstride=1) == -1 and call(start=p, sstride=1) == -1 and call(Tp=0) == -1
    assert call(d0=1e-30) == -1 and call(d0=1e30) == -1, "d0^2 and its inverse are fp32 numbers"
    assert call(scale=math.inf) == -1 and call(scale=math.nan) == -1 and call(dstride=3) == -1 and call(pstride=0) == -1
    assert call(pos=p + 4) == -1 and call(dpos=p + 4) == -1 and call(S=-1) == -1 and call(B=-1) == -1
    for kw in (dict(pos=None), dict(d0=0.0), dict(pstride=3), dict(dpos=p + 4), dict(start=p, sstride=1), dict(scale=math.nan)):
        assert call(B=0, **kw) == -1 and call(S=0, **kw) == -1, "the checks come before the early return"
    assert call(B=0) == 0 and call(S=0) == 0, "an empty batch is SW_OK without a launch"
    assert call(B=0, start=p, sstride=2) == 0 and call(B=0, pstride=4, dstride=4) == 0 and call(S=0, sstride=1) == 0      # sstride is read only with a start


def test_ops_and_stats_check_shapes_and_refuse_cpu_tensors():
    import socialways_amd as sw
    from socialways_amd import ops, stats
    sc = ops.SceneIndex.get(scene_rows([2, 3]), 5, "cpu")
    pos, dpos = torch.zeros(5, 12, 4), torch.zeros(5, 12, 4)
    for bad in (dict(pos=torch.zeros(5, 12, 3)), dict(pos=torch.zeros(4, 12, 4)), dict(dpos=torch.zeros(5, 11, 4)),
                dict(dpos=torch.zeros(5, 12, 3)), dict(start=torch.zeros(4, 2)), dict(start=torch.zeros(5, 1)),
                dict(loss=torch.zeros(4)), dict(count=torch.zeros(5)), dict(d0=0.0), dict(d0=float("nan"))):
        a = dict(pos=pos, start=None, scenes=sc, d0=0.5, scale=1.0, dpos=dpos, loss=None, count=None)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.clearance_grad(**a)
    with pytest.raises(sw.SocialWaysHipError):
        ops.clearance_grad(pos, torch.zeros(5, 2), sc, 0.5, 1.0, dpos)
    for bad in (dict(trajs=torch.zeros(5, 12, 3)), dict(trajs=torch.zeros(2, 5, 12, 2)), dict(start=torch.zeros(5, 3)),
                dict(dist=0.0), dict(dist=float("inf")), dict(scale=0.0)):
        a = dict(trajs=torch.zeros(5, 12, 2), sub_batches=scene_rows([2, 3]), dist=0.5, device="cpu")
        a.update(bad)
        with pytest.raises(ValueError):
            stats.clearance_penalty(**a)
    with pytest.raises(sw.SocialWaysHipError):
        stats.clearance_penalty(torch.zeros(5, 12, 2), scene_rows([2, 3]), 0.5, device="cpu")


def test_set_clearance_loss_and_the_refusals():
    import socialways_amd as sw
    from socialways_amd import generic, wide
    assert sw.SocialWaysTrainer.clearance_loss is None and sw.SocialWaysTrainer.last_clearance is None
    tr = object.__new__(sw.SocialWaysTrainer)
    tr.set_clearance_loss(0.2)
    assert tr.clearance_loss == (0.2, 1.0)
    tr.set_clearance_loss(np.float32(0.5), weight=0)
    assert tr.clearance_loss == (0.5, 0.0) and all(type(v) is float for v in tr.clearance_loss)
    for dist, weight in ((0.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (0.2, -0.1), (0.2, float("inf")),
                         (0.2, float("nan"))):
        with pytest.raises(ValueError):
            tr.set_clearance_loss(dist, weight)
    assert tr.clearance_loss == (0.5, 0.0), "a refused value leaves the setting alone"
    tr.set_clearance_loss(None)
    assert tr.clearance_loss is None
    tr.clearance_loss = (0.3, 2.0)            # plain assignment works too
    assert tr.clearance_loss == (0.3, 2.0)
    for cls in (generic.GenericTrainer, wide.WideTrainer):
        t = object.__new__(cls)
        assert t.clearance_loss is None
        with pytest.raises(sw.SocialWaysHipError, match="clearance"):
            t.clearance_loss = (0.2, 1.0)
        with pytest.raises(sw.SocialWaysHipError, match="clearance"):
            t.set_clearance_loss(0.2)
        with pytest.raises(ValueError):
            t.set_clearance_loss(-1.0)
        t.set_clearance_loss(None)
        t.clearance_loss = None
        assert t.clearance_loss is None


def test_graph_key_carries_the_setting_in_front_of_the_last_three():
    from socialways_amd import ops
    from socialways_amd.trainer import SocialWaysTrainer
    grp = [{"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8}]
    fake = SimpleNamespace(predictor_optimizer=SimpleNamespace(param_groups=grp), D_optimizer=SimpleNamespace(param_groups=grp),
                           _row0=0, n_unrolling_steps=1, use_info_loss=True, loss_info_w=0.5, use_l2_loss=False,
                           use_variety_loss=False, loss_l2_w=0.5, variety_k=1, use_social=True)
    sc = ops.SceneIndex.get(scene_rows([8] * 4), 32, "cpu")
    key = lambda: SocialWaysTrainer._graph_key(fake, sc, 8, 1.0, 32.0, 1, False, False)  # noqa: E731
    off = key()                               # a namespace without the attribute: the term is off
    assert off[-4] is None and off[-3] is True and off[-2:] == (False, False)
    fake.clearance_loss = None
    assert key() == off
    fake.clearance_loss = (0.2, 1.0)
    on = key()
    fake.clearance_loss = (0.3, 1.0)
    other = key()
    fake.clearance_loss = (0.3, 0.5)
    assert len({off, on, other, key()}) == 4
    assert on[-4] == (0.2, 1.0) and on[:-4] == off[:-4] and on[-3:] == off[-3:]
