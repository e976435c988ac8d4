"""Host side of the K-sample inference path (no GPU): the two C-ABI entry points are declared and bound, and
evaluate()'s noise drawing consumes the torch CPU generator exactly as test()'s loop does."""
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_arguments(name):
    """Number of parameters of `name` in include/socialways_hip.h (comments stripped)."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "socialways_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, "include/socialways_hip.h does not declare %s" % name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_and_binding_agree_on_the_sampling_entry_points():
    from socialways_amd import _lib as L
    lib = L.load()
    for name, n_args in (("sw_dec_sample_fwd", 16), ("sw_sample_reduce", 6)):
        assert name in L.PROTOTYPES, name
        res, args = L.PROTOTYPES[name]
        assert declared_arguments(name) == len(args) == n_args
        assert res is L._i and args[-1] is L._vp           # status int, void* stream last
        assert hasattr(lib, name)
    # rejected before the device is touched
    assert lib.sw_dec_sample_fwd(None, 8, None, None, None, None, None, None, 4, 2, 12, None, None, 1.0, None, None) == -1
    assert lib.sw_sample_reduce(None, 4, 2, None, None, None) == -1


def test_public_surface():
    import socialways_amd as sw
    from socialways_amd import generic
    assert callable(sw.sample) and "sample" in sw.__all__
    for cls in (sw.Generator, generic.Generator):
        assert callable(getattr(cls, "sample"))
    for cls in (sw.SocialWaysTrainer, generic.GenericTrainer):
        assert callable(getattr(cls, "evaluate"))


def test_evaluate_draws_the_noise_of_test():
    """test() (trainer.py): scene by scene, K draws of (n, noise_len) each; copy k of the chunk's rows is noise[k]."""
    from socialways_amd.trainer import SocialWaysTrainer as T
    K, noise_len, chunk = 3, 32, 40
    sizes = [4, 1, 7, 2, 9, 3, 30, 5]
    ends = np.cumsum(sizes) + 100          # held-out scenes do not start at row 0
    batches = [(int(e - s), int(e)) for s, e in zip(sizes, ends)]
    runs = list(T.eval_chunks(batches, K, chunk))
    assert runs[0] == (0, 3) and runs[-1][1] == len(batches) and len(runs) > 2        # (4 + 1 + 7) * 3 <= 40 < (.. + 2) * 3
    assert all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
    assert (6, 7) in runs                                                          # a scene above the chunk goes alone
    torch.manual_seed(5)
    want = []
    for i, j in runs:                      # the loop of test()
        lo, n = batches[i][0], batches[j - 1][1] - batches[i][0]
        noise = torch.empty(K, n, noise_len)
        for a, b in batches[i:j]:
            for k in range(K):
                noise[k, a - lo:b - lo] = torch.rand(b - a, noise_len)
        want.append(noise)
    state = torch.get_rng_state()
    torch.manual_seed(5)
    got = [T.eval_noise(batches[i:j], K, noise_len) for i, j in runs]
    assert torch.equal(torch.get_rng_state(), state)
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(a, b)
    # and it is the reference's stream: one torch.rand(n, noise_len) per scene and draw, in that order
    torch.manual_seed(5)
    for (i, j), noise in zip(runs, got):
        lo = batches[i][0]
        for a, b in batches[i:j]:
            for k in range(K):
                assert torch.equal(noise[k, a - lo:b - lo], torch.rand(b - a, noise_len))
