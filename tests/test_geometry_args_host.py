"""The argument front of the path-geometry calls without a GPU.  On a CPU tensor every geometry call of ops and stats ends in
one of three ways - ValueError (a check refused it), TypeError, or SocialWaysHipError (it passed every check and reached
require_gpu) - so which argument sets are accepted and which are refused is observable here, call by call.  TABLE holds, per
call, one good argument set and one variation per check; the outcome column was printed by running these rows against the
commit in front of the one that folded the checks into shared helpers, not written from the helpers."""
import numpy as np
import pytest
import torch

from socialways_amd import ops, stats

K, B, TP, Q, P, M = 2, 4, 3, 2, 2, 3
SUB = [[0, 2], [2, 4]]                                   # Q = S = 2 scenes of two agents
V, T, HIP = "ValueError", "TypeError", "SocialWaysHipError"
INF, NAN = float("inf"), float("nan")


def Z(*shape, dtype=torch.float32, device="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=device)


def I(*shape, dtype=torch.int32, device="cpu"):
    return torch.ones(*shape, dtype=dtype, device=device)


def scenes(rows=B):
    return ops.SceneIndex.get(SUB if rows == B else [], rows, "cpu")


# variations that many calls share: (name, overrides, outcome)
def pos_rows(name="pos", dtype_outcome=HIP, lead=(K * B,), lead4=(K, B)):
    return [(name + " 4-d, 4 wide", {name: Z(*lead4, TP, 4)}, HIP),
            (name + " rank 2", {name: Z(*lead, TP)}, V),
            (name + " last dimension 3", {name: Z(*lead, TP, 3)}, V),
            (name + " without steps", {name: Z(*lead, 0, 2)}, V),
            (name + " one row short", {name: Z(lead[0] - 1, TP, 2)}, V),
            (name + " 4-d, other K", {name: Z(lead4[0] + 1, lead4[1], TP, 2)}, V),
            (name + " 4-d, other B", {name: Z(lead4[0], lead4[1] - 1, TP, 2)}, V),
            (name + " float64", {name: Z(*lead, TP, 2, dtype=torch.float64)}, dtype_outcome)]


def start_rows(name="start"):
    return [(name + " None", {name: None}, HIP),
            (name + " 4 wide", {name: Z(B, 4)}, HIP),
            (name + " float64", {name: Z(B, 2, dtype=torch.float64)}, HIP),
            (name + " a strided view", {name: Z(B, 8, 2)[:, -1]}, HIP),
            (name + " one row short", {name: Z(B - 1, 2)}, V),
            (name + " 1 wide", {name: Z(B, 1)}, V),
            (name + " rank 1", {name: Z(B)}, V),
            (name + " on another device", {name: Z(B, 2, device="meta")}, V)]


def lens_rows(name="lens", n=B):
    return [(name + " None", {name: None}, HIP),
            (name + " int64", {name: I(n, dtype=torch.int64)}, V),
            (name + " float32", {name: Z(n)}, V),
            (name + " one short", {name: I(n - 1)}, V),
            (name + " a list", {name: [1] * n}, V),
            (name + " on another device", {name: I(n, device="meta")}, V)]


def positive_rows(name, bad=V):                          # inv_ss and its like: > 0, +inf passes
    return [(name + " 0", {name: 0.0}, bad), (name + " negative", {name: -1.0}, bad), (name + " nan", {name: NAN}, bad),
            (name + " inf", {name: INF}, HIP)]


def distance_rows(name, bad=V):                          # coll_dist and its like: >= 0, +inf passes
    return [(name + " 0", {name: 0.0}, HIP), (name + " negative", {name: -1.0}, bad), (name + " nan", {name: NAN}, bad),
            (name + " inf", {name: INF}, HIP)]


def penalty_rows(name, tiny=HIP):                        # d0 and its like: finite and > 0
    return [(name + " 0", {name: 0.0}, V), (name + " negative", {name: -1.0}, V), (name + " nan", {name: NAN}, V),
            (name + " inf", {name: INF}, V), (name + " below fp32 squares", {name: 1e-30}, tiny),
            (name + " above fp32 squares", {name: 1e30}, tiny)]


def walls_rows(name="walls", host=False):
    rows = [(name + " empty", {name: Z(0, 2, 2)}, HIP),
            (name + " 1024", {name: Z(1024, 2, 2)}, HIP),
            (name + " 1025", {name: Z(1025, 2, 2)}, V),
            (name + " (M, 3)", {name: Z(M, 3)}, V),
            (name + " (M, 2, 3)", {name: Z(M, 2, 3)}, V)]
    if host:
        return rows + [(name + " (M, 4) host rows", {name: np.zeros((M, 4))}, HIP), (name + " float64", {name: Z(M, 2, 2, dtype=torch.float64)}, HIP)]
    return rows + [(name + " (M, 4)", {name: Z(M, 4)}, V), (name + " float64", {name: Z(M, 2, 2, dtype=torch.float64)}, V),
                   (name + " host rows", {name: np.zeros((M, 2, 2), dtype=np.float32)}, V),
                   (name + " on another device", {name: Z(M, 2, 2, device="meta")}, V)]


def out_rows(lead, also=None):                           # loss / count of the gradient calls
    rows = [("loss None", dict(loss=None), HIP), ("count None", dict(count=None), HIP),
            ("loss one short", dict(loss=Z(lead[-1] - 1)), V), ("loss float64", dict(loss=Z(*lead, dtype=torch.float64)), V),
            ("loss not contiguous", dict(loss=Z(*lead, 2)[..., 0]), V), ("loss on another device", dict(loss=Z(*lead, device="meta")), V),
            ("count one short", dict(count=I(lead[-1] - 1)), V), ("count int64", dict(count=I(*lead, dtype=torch.int64)), V),
            ("count float32", dict(count=Z(*lead)), V)]
    if also is not None:
        rows += [("loss flat", dict(loss=Z(*also)), HIP), ("count flat", dict(count=I(*also)), HIP)]
    return rows


def plan_rows(np_plans=V, strict=True, one_more=()):
    """plans, plan_start, the queries: ops takes checked device tensors (np_plans V), stats host data as well; one_more: what
    else a call with one query has to change."""
    one = dict(dict(one_more), plans=Z(P, TP, 2), plan_start=Z(1, 2))
    rows = [("plans float64", dict(plans=Z(Q, P, TP, 2, dtype=torch.float64)), V if strict else HIP),
            ("plans host rows", dict(plans=np.zeros((Q, P, TP, 2), dtype=np.float32)), np_plans),
            ("plans rank 2", dict(plans=Z(TP, 2)), V),
            ("plans rank 5", dict(plans=Z(1, Q, P, TP, 2)), V),
            ("plans without a plan", dict(plans=Z(Q, 0, TP, 2)), V),
            ("plans of other length", dict(plans=Z(Q, P, TP + 1, 2)), V),
            ("plans 4 wide", dict(plans=Z(Q, P, TP, 4)), V),
            ("plans one query more", dict(plans=Z(Q + 1, P, TP, 2)), V),
            ("plans 3-d against Q = 2", dict(plans=Z(P, TP, 2)), V),
            ("plan_start one row short", dict(plan_start=Z(Q - 1, 2)), V),
            ("plan_start 3 wide", dict(plan_start=Z(Q, 3)), V),
            ("plan_start float64", dict(plan_start=Z(Q, 2, dtype=torch.float64)), HIP),
            ("plan_start host rows", dict(plan_start=np.zeros((Q, 2), dtype=np.float32)), np_plans)]
    if strict:
        rows += [("plans on another device", dict(plans=Z(Q, P, TP, 2, device="meta")), V),
                 ("plan_start on another device", dict(plan_start=Z(Q, 2, device="meta")), V),
                 ("plans 3-d, one query", dict(one, q_scene=I(1), q_ego=I(1)), HIP),
                 ("q_scene int64", dict(q_scene=I(Q, dtype=torch.int64)), V), ("q_scene one short", dict(q_scene=I(Q - 1)), V),
                 ("q_scene a list", dict(q_scene=[0, 1]), V), ("q_scene on another device", dict(q_scene=I(Q, device="meta")), V),
                 ("q_ego None", dict(q_ego=None), HIP), ("q_ego int64", dict(q_ego=I(Q, dtype=torch.int64)), V),
                 ("q_ego one short", dict(q_ego=I(Q - 1)), V), ("q_ego float32", dict(q_ego=Z(Q)), V)]
    else:
        rows += [("plans 3-d, one query of one scene", dict(one, sub_batches=[], scene=None, ego=None), HIP),
                 ("scene None with Q = S", dict(scene=None), HIP),
                 ("scene None with Q != S", dict(scene=None, sub_batches=[]), V),
                 ("scene a tensor", dict(scene=I(Q, dtype=torch.int64)), HIP), ("scene one short", dict(scene=[0]), V),
                 ("scene of floats", dict(scene=[0.0, 1.0]), V), ("ego None", dict(ego=None), HIP), ("ego one short", dict(ego=[1]), V),
                 ("ego of floats", dict(ego=np.zeros(Q)), V), ("ego a tensor", dict(ego=I(Q)), HIP)]
    return rows


def descent_rows():
    return [("n_iter 0", dict(n_iter=0), HIP), ("n_iter 1024", dict(n_iter=1024), HIP), ("n_iter negative", dict(n_iter=-1), V),
            ("n_iter 1025", dict(n_iter=1025), V), ("n_iter 1.5", dict(n_iter=1.5), V), ("n_iter True", dict(n_iter=True), V),
            ("lr negative", dict(lr=-0.1), V), ("lr nan", dict(lr=NAN), V), ("lr unstable", dict(lr=1.0), V),
            ("lr 0", dict(lr=0.0), HIP), ("w_track inf", dict(w_track=INF), V), ("w_smooth negative", dict(w_smooth=-1.0), V),
            ("w_smooth unstable", dict(w_smooth=1.0), V), ("max_move negative", dict(max_move=-0.5), V), ("max_move nan", dict(max_move=NAN), V),
            ("max_move 0", dict(max_move=0.0), HIP), ("w_wall 0", dict(w_wall=0.0), HIP), ("w_wall negative", dict(w_wall=-1.0), V),
            ("w_wall inf", dict(w_wall=INF), V), ("w_wall nan", dict(w_wall=NAN), V)]


def host_lens_rows(name="lens", n=B):
    return [(name + " None", {name: None}, HIP), (name + " a tensor", {name: I(n, dtype=torch.int64)}, HIP),
            (name + " an array", {name: np.ones(n, dtype=np.int16)}, HIP), (name + " beyond T", {name: [TP + 1] + [1] * (n - 1)}, V),
            (name + " 0", {name: [0] + [1] * (n - 1)}, V), (name + " of floats", {name: [1.0] * n}, V), (name + " one short", {name: [1] * (n - 1)}, V)]


def host_start_rows():
    return [("start None", dict(start=None), HIP), ("start host rows", dict(start=[[0.0, 0.0]] * B), HIP),
            ("start float64", dict(start=Z(B, 2, dtype=torch.float64)), HIP), ("start 3 wide", dict(start=Z(B, 3)), V),
            ("start one row short", dict(start=Z(B - 1, 2)), V), ("start rank 1", dict(start=Z(B)), V)]


def trajs_rows(three_d, also=()):
    """also: what else a call without steps has to change (its lens)"""
    lift = HIP if three_d else V
    return [("trajs host rows", dict(trajs=np.zeros((K, B, TP, 2))), HIP), ("trajs 4 wide", dict(trajs=Z(K, B, TP, 4)), HIP),
            ("trajs float64", dict(trajs=Z(K, B, TP, 2, dtype=torch.float64)), HIP),
            ("trajs 3-d", dict(trajs=Z(B, TP, 2)), lift), ("trajs rank 2", dict(trajs=Z(TP, 2)), V),
            ("trajs rank 5", dict(trajs=Z(1, K, B, TP, 2)), V), ("trajs 3 wide", dict(trajs=Z(K, B, TP, 3)), V),
            ("trajs without steps", dict(dict(also), trajs=Z(K, B, 0, 2)), V), ("trajs without draws", dict(trajs=Z(0, B, TP, 2)), V)]


def sub_rows(bad):                                       # HIP where the form reaches require_gpu before it builds the scene index
    return [("sub_batches [] = one scene", dict(sub_batches=[]), HIP), ("sub_batches with a gap", dict(sub_batches=[[0, 2], [3, 4]]), bad),
            ("sub_batches short of B", dict(sub_batches=[[0, 2], [2, 3]]), bad), ("sub_batches with an empty scene", dict(sub_batches=[[0, 0], [0, 4]]), bad)]


NO_LENS = dict(lens=None)
SCALE_DIV = [("scale 0", dict(scale=0.0), V), ("scale negative", dict(scale=-1.0), V), ("scale nan", dict(scale=NAN), V), ("scale inf", dict(scale=INF), V)]

TABLE = {
    "ops.scene_clearance": (
        lambda: dict(pos=Z(K * B, TP, 2), start=Z(B, 2), scenes=scenes(), K=K, inv_ss=1.0, lens=I(B)),
        pos_rows() + start_rows() + lens_rows()
        + [("K 0", dict(K=0), V), ("K 4", dict(K=4), V), ("scenes of other B", dict(scenes=scenes(B - 1)), V),
           ("inv_ss 0 (left to the entry point)", dict(inv_ss=0.0), HIP), ("inv_ss nan (left to the entry point)", dict(inv_ss=NAN), HIP),
           ("inv_ss None", dict(inv_ss=None), HIP)]),
    "ops.clearance_grad": (
        lambda: dict(pos=Z(B, TP, 2), start=Z(B, 2), scenes=scenes(), d0=0.5, scale=1.0, dpos=Z(B, TP, 2), loss=Z(B), count=I(B)),
        [("pos 4 wide", dict(pos=Z(B, TP, 4)), HIP), ("pos rank 4", dict(pos=Z(1, B, TP, 2)), V), ("pos 3 wide", dict(pos=Z(B, TP, 3)), V),
         ("pos one row short", dict(pos=Z(B - 1, TP, 2)), V), ("pos without steps", dict(pos=Z(B, 0, 2), dpos=Z(B, 0, 2)), V),
         ("pos float64", dict(pos=Z(B, TP, 2, dtype=torch.float64)), V), ("dpos 4 wide", dict(dpos=Z(B, TP, 4)), HIP),
         ("dpos one step short", dict(dpos=Z(B, TP - 1, 2)), V), ("dpos one row short", dict(dpos=Z(B - 1, TP, 2)), V),
         ("dpos 3 wide", dict(dpos=Z(B, TP, 3)), V), ("dpos float64", dict(dpos=Z(B, TP, 2, dtype=torch.float64)), V),
         ("dpos not contiguous", dict(dpos=Z(B, TP, 4)[..., :2]), V), ("dpos on another device", dict(dpos=Z(B, TP, 2, device="meta")), V),
         ("scale 0", dict(scale=0.0), HIP), ("scale negative", dict(scale=-1.0), HIP), ("scale inf", dict(scale=INF), V),
         ("scale nan", dict(scale=NAN), V), ("d0 None", dict(d0=None), T)]
        + penalty_rows("d0") + start_rows() + out_rows((B,))),
    "ops.sample_nms": (
        lambda: dict(pos=Z(K * B, TP, 2), score=Z(K, B), K=K, M=2, radius=0.5, metric="fde", scenes=scenes(), inv_ss=1.0, err=Z(K, B, 2), best=I(B)),
        pos_rows() + distance_rows("radius") + positive_rows("inv_ss")
        + [("pos on another device", dict(pos=Z(K * B, TP, 2, device="meta")), V), ("score rank 1", dict(score=Z(K * B)), V),
           ("score of other K", dict(score=Z(K + 1, B)), V), ("score of other B", dict(score=Z(K, B - 1)), V),
           ("score float64", dict(score=Z(K, B, dtype=torch.float64)), HIP), ("K 0", dict(K=0), V), ("M 0", dict(M=0), V), ("M above K", dict(M=K + 1), V),
           ("M 1", dict(M=1), HIP), ("K above 4096", dict(K=4097, score=Z(4097, 1), pos=Z(4097, TP, 2), scenes=None, err=None, best=None), V),
           ("err None", dict(err=None, best=None), HIP), ("err of other B", dict(err=Z(K, B - 1, 2)), V), ("err 3 wide", dict(err=Z(K, B, 3)), V),
           ("err on another device", dict(err=Z(K, B, 2, device="meta")), V), ("best None", dict(best=None), HIP),
           ("best without err", dict(err=None), V), ("best int64", dict(best=I(B, dtype=torch.int64)), V), ("best one short", dict(best=I(B - 1)), V),
           ("best on another device", dict(best=I(B, device="meta")), V), ("metric ade", dict(metric="ade"), HIP), ("metric unknown", dict(metric="l1"), V),
           ("scenes None", dict(scenes=None), HIP), ("scenes of other B", dict(scenes=scenes(B - 1)), V), ("radius None", dict(radius=None), T)]),
    "ops.scene_compose": (
        lambda: dict(pos=Z(K * B, TP, 2), start=Z(B, 2), score=Z(K, B), scenes=scenes(), K=K, coll_dist=0.2, inv_ss=1.0, sweeps=8, lens=I(B),
                     err=Z(K, B, 2)),
        pos_rows() + start_rows() + lens_rows() + distance_rows("coll_dist") + positive_rows("inv_ss")
        + [("pos on another device", dict(pos=Z(K * B, TP, 2, device="meta")), V), ("score rank 1", dict(score=Z(K * B)), V),
           ("score of other K", dict(score=Z(K + 1, B)), V), ("score of other B", dict(score=Z(K, B - 1)), V), ("K 0", dict(K=0), V),
           ("K above 4096", dict(K=4097, score=Z(4097, B), pos=Z(4097 * B, TP, 2), err=None), V), ("sweeps 0", dict(sweeps=0), V),
           ("sweeps 1", dict(sweeps=1), HIP), ("err None", dict(err=None), HIP), ("err of other K", dict(err=Z(K + 1, B, 2)), V),
           ("scenes of other B", dict(scenes=scenes(B - 1)), V), ("coll_dist None", dict(coll_dist=None), T)]),
    "ops.plan_risk": (
        lambda: dict(pos=Z(K * B, TP, 2), start=Z(B, 2), scenes=scenes(), K=K, plans=Z(Q, P, TP, 2), plan_start=Z(Q, 2), q_scene=I(Q), q_ego=I(Q),
                     coll_dist=0.2, inv_ss=1.0, lens=I(B), plan_lens=I(Q)),
        pos_rows() + start_rows()[1:] + lens_rows() + lens_rows("plan_lens", Q) + distance_rows("coll_dist") + positive_rows("inv_ss") + plan_rows(one_more=dict(plan_lens=I(1)))
        + [("start without plan_start", dict(plan_start=None), V), ("plan_start without start", dict(start=None), V),
           ("neither start nor plan_start", dict(start=None, plan_start=None), HIP), ("K 0", dict(K=0), V)]),
    "ops.path_walls": (
        lambda: dict(pos=Z(K * B, TP, 2), start=Z(B, 2), K=K, walls=Z(M, 2, 2), dist=0.2, inv_ss=1.0, lens=I(B)),
        pos_rows()[:6] + pos_rows()[7:] + start_rows() + lens_rows() + distance_rows("dist") + positive_rows("inv_ss") + walls_rows()
        + [("pos 4-d, other B, start to match", dict(pos=Z(K, B - 1, TP, 2), start=None, lens=None), HIP), ("K 0", dict(K=0), V),
           ("K not dividing the rows", dict(K=3), V), ("K 4 against start", dict(K=4), V), ("K 4 and B to match", dict(K=4, start=None, lens=None), HIP),
           ("dist None", dict(dist=None), T)]),
    "ops.wall_grad": (
        lambda: dict(pos=Z(K * B, TP, 2), start=Z(B, 2), K=K, walls=Z(M, 2, 2), dw=0.5, scale=1.0, dpos=Z(K * B, TP, 2), loss=Z(K, B), count=I(K, B),
                     lens=I(B)),
        [("pos and dpos 4-d", dict(pos=Z(K, B, TP, 4), dpos=Z(K, B, TP, 2)), HIP), ("pos 3-d, dpos 4-d", dict(dpos=Z(K, B, TP, 4)), HIP),
         ("pos rank 2", dict(pos=Z(K * B, TP)), V), ("pos 3 wide", dict(pos=Z(K * B, TP, 3)), V), ("pos one row short", dict(pos=Z(K * B - 1, TP, 2)), V),
         ("pos 4-d, other K", dict(pos=Z(K + 1, B, TP, 2)), V), ("pos float64", dict(pos=Z(K * B, TP, 2, dtype=torch.float64)), V),
         ("K 0", dict(K=0), V), ("K not dividing the rows", dict(K=3), V), ("dpos one step short", dict(dpos=Z(K * B, TP - 1, 2)), V),
         ("dpos one row short", dict(dpos=Z(K * B - 1, TP, 2)), V), ("dpos 3 wide", dict(dpos=Z(K * B, TP, 3)), V), ("dpos rank 2", dict(dpos=Z(K * B, TP)), V),
         ("dpos float64", dict(dpos=Z(K * B, TP, 2, dtype=torch.float64)), V), ("dpos not contiguous", dict(dpos=Z(K * B, TP, 4)[..., :2]), V),
         ("dpos on another device", dict(dpos=Z(K * B, TP, 2, device="meta")), V), ("scale 0", dict(scale=0.0), HIP), ("scale inf", dict(scale=INF), V),
         ("scale nan", dict(scale=NAN), V), ("dw None", dict(dw=None), T)]
        + penalty_rows("dw") + start_rows() + lens_rows() + walls_rows() + out_rows((K, B), (K * B,))),
    "ops.plan_refine": (
        lambda: dict(pos=Z(K * B, TP, 2), start=Z(B, 2), scenes=scenes(), K=K, plans=Z(Q, P, TP, 2), plan_start=Z(Q, 2), q_scene=I(Q), q_ego=I(Q),
                     d0=0.5, inv_ss=1.0, lens=I(B), walls=Z(M, 2, 2), wall_d0=0.4, w_wall=1.0),
        pos_rows() + start_rows()[1:] + lens_rows() + penalty_rows("d0", V) + penalty_rows("wall_d0", V) + positive_rows("inv_ss") + plan_rows()
        + descent_rows() + walls_rows()
        + [("start None", dict(start=None), V), ("plan_start None", dict(plan_start=None), V), ("neither start nor plan_start", dict(start=None, plan_start=None), V),
           ("walls None", dict(walls=None), HIP), ("walls None, wall_d0 unread", dict(walls=None, wall_d0=0.0, w_wall=-1.0), HIP),
           ("wall_d0 None = d0", dict(wall_d0=None), HIP), ("K above 4096", dict(K=4097, pos=Z(4097 * B, TP, 2)), V),
           ("more than 1024 steps", dict(pos=Z(K * B, 1025, 2), plans=Z(Q, P, 1025, 2)), V)]),
    "stats.scene_clearance_len": (
        lambda: dict(trajs=Z(K, B, TP, 2), sub_batches=SUB, lens=[TP, TP, 2, 1], start=Z(B, 2), scale=1.0, device="cpu"),
        trajs_rows(True, NO_LENS) + host_lens_rows() + host_start_rows() + sub_rows(HIP)
        + [("trajs 3-d without agents (left to the scene index)", dict(trajs=Z(0, TP, 2), lens=None, start=None), HIP),
           ("scale 0 (left to the entry point)", dict(scale=0.0), HIP), ("scale nan (left to the entry point)", dict(scale=NAN), HIP)]),
    "stats.clearance_penalty": (
        lambda: dict(trajs=Z(B, TP, 2), sub_batches=SUB, dist=0.5, start=Z(B, 2), scale=1.0, device="cpu"),
        [("trajs host rows", dict(trajs=np.zeros((B, TP, 2))), HIP), ("trajs 4 wide", dict(trajs=Z(B, TP, 4)), HIP), ("trajs 4-d", dict(trajs=Z(K, B, TP, 2)), V),
         ("trajs rank 2", dict(trajs=Z(TP, 2)), V), ("trajs 3 wide", dict(trajs=Z(B, TP, 3)), V), ("trajs without steps", dict(trajs=Z(B, 0, 2)), V),
         ("trajs without agents (left to the scene index)", dict(trajs=Z(0, TP, 2), start=None), HIP)]
        + penalty_rows("dist") + SCALE_DIV + host_start_rows() + sub_rows(HIP)),
    "stats.sample_modes": (
        lambda: dict(trajs=Z(K, B, TP, 2), score=Z(K, B), radius=0.5, top_m=2, metric="fde", sub_batches=SUB, scale=1.0, device="cpu"),
        trajs_rows(False) + distance_rows("radius", HIP) + positive_rows("scale", HIP) + sub_rows(HIP)
        + [("score host rows", dict(score=np.zeros((K, B))), HIP), ("score of other K", dict(score=Z(K + 1, B)), V), ("score of other B", dict(score=Z(K, B - 1)), V),
           ("score rank 1", dict(score=Z(K * B)), V), ("top_m 0", dict(top_m=0), HIP), ("top_m above K", dict(top_m=K + 1), HIP), ("metric ade", dict(metric="ade"), HIP),
           ("metric unknown", dict(metric="l1"), HIP), ("sub_batches None: every agent alone", dict(sub_batches=None), HIP)]),
    "stats.compose_scenes": (
        lambda: dict(trajs=Z(K, B, TP, 2), score=Z(K, B), sub_batches=SUB, coll_dist=0.2, start=Z(B, 2), scale=1.0, sweeps=8, lens=[TP, TP, 2, 1], device="cpu"),
        trajs_rows(False, NO_LENS) + distance_rows("coll_dist", HIP) + positive_rows("scale", HIP) + host_lens_rows() + host_start_rows() + sub_rows(HIP)
        + [("score of other K", dict(score=Z(K + 1, B)), V), ("score of other B", dict(score=Z(K, B - 1)), V), ("sweeps 0", dict(sweeps=0), HIP)]),
    "stats.plan_risk": (
        lambda: dict(trajs=Z(K, B, TP, 2), sub_batches=SUB, plans=Z(Q, P, TP, 2), coll_dist=0.2, plan_start=Z(Q, 2), start=Z(B, 2), scene=[0, 1], ego=[0, -1],
                     scale=1.0, lens=[TP, TP, 2, 1], plan_lens=[TP, 1], device="cpu"),
        trajs_rows(False, dict(lens=None, plan_lens=None)) + distance_rows("coll_dist") + positive_rows("scale") + host_lens_rows()
        + host_lens_rows("plan_lens", Q) + host_start_rows()[1:] + sub_rows(V) + plan_rows(HIP, strict=False, one_more=dict(plan_lens=None))
        + [("start without plan_start", dict(plan_start=None), V), ("plan_start without start", dict(start=None), V),
           ("neither start nor plan_start", dict(start=None, plan_start=None), HIP)]),
    "stats.path_walls": (
        lambda: dict(trajs=Z(K, B, TP, 2), walls=Z(M, 2, 2), dist=0.2, start=Z(B, 2), scale=1.0, lens=[TP, TP, 2, 1], device="cpu"),
        trajs_rows(True, NO_LENS) + distance_rows("dist") + positive_rows("scale") + host_lens_rows() + host_start_rows() + walls_rows(host=True)
        + [("trajs 3-d without agents", dict(trajs=Z(0, TP, 2), lens=None, start=None), V)]),
    "stats.wall_penalty": (
        lambda: dict(trajs=Z(K, B, TP, 2), walls=Z(M, 2, 2), dist=0.5, start=Z(B, 2), scale=1.0, lens=[TP, TP, 2, 1], device="cpu"),
        trajs_rows(True, NO_LENS) + penalty_rows("dist") + SCALE_DIV + host_lens_rows() + host_start_rows() + walls_rows(host=True)
        + [("trajs 3-d without agents", dict(trajs=Z(0, TP, 2), lens=None, start=None), V)]),
    "stats.refine_plans": (
        lambda: dict(trajs=Z(K, B, TP, 2), sub_batches=SUB, plans=Z(Q, P, TP, 2), dist=0.5, plan_start=Z(Q, 2), start=Z(B, 2), scene=[0, 1], ego=[0, -1],
                     scale=1.0, lens=[TP, TP, 2, 1], device="cpu", walls=Z(M, 2, 2), wall_dist=0.4, w_wall=1.0),
        trajs_rows(False, NO_LENS) + penalty_rows("dist", V) + penalty_rows("wall_dist", V) + SCALE_DIV + host_lens_rows() + host_start_rows()[1:] + sub_rows(V)
        + plan_rows(HIP, strict=False) + descent_rows() + walls_rows(host=True)
        + [("start None", dict(start=None), V), ("plan_start None", dict(plan_start=None), V), ("walls None", dict(walls=None), HIP),
           ("walls None, wall_dist unread", dict(walls=None, wall_dist=0.0, w_wall=-1.0), HIP), ("wall_dist None = dist", dict(wall_dist=None), HIP),
           ("an unknown descent keyword", dict(momentum=0.9), T)]),
}

CASES = [(call, name, change, outcome) for call, (_, rows) in TABLE.items() for name, change, outcome in [("the good set", {}, HIP)] + rows]


def outcome_of(call, change):
    """The class name of what `call` raises on its good argument set with `change` applied."""
    import socialways_amd as sw
    mod, fn = call.split(".")
    args = dict(TABLE[call][0](), **change)
    try:
        getattr({"ops": ops, "stats": stats}[mod], fn)(**args)
    except (ValueError, TypeError, sw.SocialWaysHipError) as e:
        return type(e).__name__
    return "returned"


def test_the_table_covers_every_call_and_names_every_row_once():
    assert len(TABLE) == 16 and len({(c, n) for c, n, _, _ in CASES}) == len(CASES)
    assert sorted(c for c in TABLE if c.startswith("ops.")) == ["ops.clearance_grad", "ops.path_walls", "ops.plan_refine", "ops.plan_risk",
                                                               "ops.sample_nms", "ops.scene_clearance", "ops.scene_compose", "ops.wall_grad"]


@pytest.mark.parametrize("call", list(TABLE))
def test_every_argument_set_ends_as_the_table_says(call):
    wrong = [(name, outcome, got) for c, name, change, outcome in CASES if c == call
             for got in [outcome_of(call, change)] if got != outcome]
    assert not wrong, "%s: (variation, expected, got) %s" % (call, wrong)
