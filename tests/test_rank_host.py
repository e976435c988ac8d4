"""Host side of scoring and ranking K sampled futures (no GPU): the two C-ABI entry points are declared and bound, reject
bad arguments before the device is touched, and the ops wrappers name the shape they expect."""
import ctypes

import pytest
import torch

from test_sample_host import declared_arguments

EARG, ESHAPE = -1, -2


def test_header_and_binding_agree_on_the_ranking_entry_points():
    from socialways_amd import _lib as L
    lib = L.load()
    for name, n_args in (("sw_disc_score", 11), ("sw_sample_rank", 9)):
        assert name in L.PROTOTYPES, name
        res, args = L.PROTOTYPES[name]
        assert declared_arguments(name) == len(args) == n_args
        assert res is L._i and args[-1] is L._vp           # status int, void* stream last
        assert hasattr(lib, name)


def test_argument_validation_without_gpu():
    """Every SW_EARG / SW_ESHAPE condition of both functions; `p` is a non-NULL address nobody dereferences: each call
    returns from its argument checks (B == 0 included: SW_OK without a launch)."""
    from socialways_amd import _lib as L
    lib = L.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def score(obsv=p, To=8, x_mode=0, pred4=p, d_w=p, B=0, K=3, Tp=12, out=p, code=p):
        return lib.sw_disc_score(obsv, To, x_mode, pred4, d_w, B, K, Tp, out, code, None)
    assert score() == 0 and score(code=None) == 0 and score(x_mode=1, To=1) == 0
    for kw in (dict(obsv=None), dict(pred4=None), dict(d_w=None), dict(out=None), dict(K=0), dict(K=-3), dict(B=-1),
               dict(x_mode=2), dict(x_mode=-1), dict(To=1), dict(To=0, x_mode=1), dict(Tp=0)):
        assert score(**kw) == EARG, kw
        assert score(B=5, **{k: v for k, v in kw.items() if k != "B"}) == EARG or "B" in kw, kw
    assert score(Tp=65) == ESHAPE and score(B=5, Tp=65) == ESHAPE and score(Tp=64) == 0

    def rank(score=p, err=p, best=p, B=0, K=20, M=5, order=p, per_agent=p):
        return lib.sw_sample_rank(score, err, best, B, K, M, order, per_agent, None)
    assert rank() == 0 and rank(err=None, best=None, per_agent=None) == 0 and rank(best=None) == 0 and rank(M=20) == 0
    assert rank(K=1, M=1) == 0 and rank(K=4096) == 0
    for kw in (dict(score=None), dict(order=None), dict(B=-1), dict(K=0), dict(M=0), dict(M=21), dict(M=-1),
               dict(err=None), dict(err=None, best=None)):      # per_agent needs err
        assert rank(**kw) == EARG, kw
        assert rank(B=7, **{k: v for k, v in kw.items() if k != "B"}) == EARG or "B" in kw, kw
    assert rank(K=4097) == ESHAPE and rank(B=7, K=4097) == ESHAPE


def test_ops_wrappers_name_the_expected_shape():
    from socialways_amd import ops, SocialWaysHipError
    d_w = torch.zeros(8)
    obsv, pred4 = torch.zeros(5, 8, 2), torch.zeros(3 * 5, 12, 4)
    for bad_o, bad_p, K in ((obsv[0], pred4, 3), (torch.zeros(5, 8, 3), pred4, 3), (torch.zeros(5, 1, 2), pred4, 3),
                            (obsv, pred4[:14], 3), (obsv, torch.zeros(3, 4, 12, 4), 3), (obsv, torch.zeros(15, 12, 2), 3),
                            (obsv, pred4, 4), (obsv, pred4, 0)):
        with pytest.raises(ValueError):
            ops.disc_score(d_w, bad_o, bad_p, K)
    with pytest.raises(ValueError, match=r"\(K \* B, Tp, 4\)"):
        ops.disc_score(d_w, obsv, pred4[:14], 3)
    with pytest.raises(SocialWaysHipError):                # well-formed, but not on the GPU: no CPU fallback
        ops.disc_score(d_w, obsv, pred4, 3)
    score, err, best = torch.zeros(20, 7), torch.zeros(20, 7, 2), torch.zeros(7, dtype=torch.int32)
    for kw in (dict(score=score[0]), dict(K=19), dict(M=0), dict(M=21), dict(err=err[:, :6]), dict(err=err[..., :1]),
               dict(best=best[:6]), dict(best=best.long()), dict(err=None), dict(score=torch.zeros(5000, 2), K=5000)):
        a = dict(score=score, K=20, M=5, err=err, best=best)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.sample_rank(a["score"], a["K"], a["M"], err=a["err"], best=a["best"])
    with pytest.raises(ValueError, match=r"\(K, B, 2\) = \(20, 7, 2\)"):
        ops.sample_rank(score, 20, 5, err=err[:, :6])
    with pytest.raises(SocialWaysHipError):
        ops.sample_rank(score, 20, 5, err=err, best=best)


def test_public_surface():
    import socialways_amd as sw
    from socialways_amd import generic, wide
    for cls in (sw.Discriminator, generic.Discriminator):
        assert callable(getattr(cls, "score_samples"))
    for cls in (sw.SocialWaysTrainer, generic.GenericTrainer, wide.WideTrainer):
        assert callable(getattr(cls, "sample_ranked")) and callable(getattr(cls, "evaluate_ranked"))
    with pytest.raises(ValueError):
        sw.Discriminator(12, 64, 2).score_samples(torch.zeros(5, 8, 2), torch.zeros(3, 5, 11, 4))
    with pytest.raises(ValueError):
        generic.Discriminator(12, 80, 3).score_samples(torch.zeros(5, 8, 2), torch.zeros(3, 4, 12, 4))
