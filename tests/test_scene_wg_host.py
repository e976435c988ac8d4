"""Which batch layouts run the scene-per-workgroup backward launch (ops.scene_wg), and that a captured step's key carries the
decision: no GPU."""
from types import SimpleNamespace

import numpy as np
import pytest


def _scenes(sizes, device="cpu"):
    from socialways_amd import ops
    off = np.concatenate([[0], np.cumsum(sizes)])
    return ops.SceneIndex.get(np.stack([off[:-1], off[1:]], 1), int(off[-1]), device)


@pytest.mark.parametrize("sizes, want", [
    ([8] * 256, True),            # the metric shape
    ([8] * 32, True),
    ([1, 16, 2], True),
    ([2] * 40, True),
    ([16, 15], True),
    ([1], False),                 # no pair: there is no social backward
    ([1] * 5, False),
    ([16], False),                # P = 256 S: the in-register social backward, which the rows body does not reproduce bit for bit
    ([16] * 3, False),
    ([17], False),                # a scene is the columns of one 16-agent tile
    ([8, 17, 8], False),
    ([64] * 64, False),           # dense crowds
    ([8, 70], False),             # row-block scenes
    ([8] * 257, False),           # one CU per scene
    ([8] * 1024, False),
])
def test_eligibility(sizes, want):
    from socialways_amd import ops
    sc = _scenes(sizes)
    assert ops.scene_wg(sc, True) is want
    assert ops.scene_wg(sc, False) is False, "no social block"
    assert ops.scene_wg(sc, True, ragged=True) is False, "ragged histories keep their launches"


def test_the_bounds_are_the_librarys():
    from socialways_amd import _lib as L
    from socialways_amd import ops
    lib = L.load()
    assert lib.sw_scene_wg_max_scenes() == ops.SCENE_WG_MAX_SCENES == 256
    assert lib.sw_social_rows_max_pairs() == ops.SOCIAL_ROWS_MAX_PAIRS
    assert ops.SCENE_WG_MAX_AGENTS == 16 and ops.SCENE_WG is True
    # refused before the device is touched (no GPU here): a layout outside the bounds, and a NULL argument
    assert lib.sw_social_enc_bwd(*([1, 8] + [1] * 3 + [1, 16, 16, 256] + [1] * 13 + [None, None, None, 0, None, None])) == -2
    assert lib.sw_social_enc_bwd(*([None, 8] + [1] * 3 + [1, 16, 16, 64] + [1] * 13 + [None, None, None, 0, None, None])) == -1


def test_switch_and_graph_key(monkeypatch):
    from socialways_amd import ops
    from socialways_amd.trainer import SocialWaysTrainer
    grp = [{"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8}]
    fake = SimpleNamespace(predictor_optimizer=SimpleNamespace(param_groups=grp), D_optimizer=SimpleNamespace(param_groups=grp),
                           _row0=0, n_unrolling_steps=1, use_info_loss=True, loss_info_w=0.5, use_l2_loss=False,
                           use_variety_loss=False, loss_l2_w=0.5, variety_k=1, use_social=True)
    key = lambda sc, ragged=False: SocialWaysTrainer._graph_key(fake, sc, 8, 1.0, float(sc.B), 1, False, ragged)  # noqa: E731
    small, big = _scenes([8] * 4), _scenes([17, 3])
    at = -3                       # the decision sits in front of (ragged, z by address), which stay last
    on = key(small)
    assert on[at] is True and key(big)[at] is False and key(small, ragged=True)[at] is False
    assert on[-2:] == (False, False) and key(small, ragged=True)[-2:] == (True, False)
    monkeypatch.setattr(ops, "SCENE_WG", False)
    assert not ops.scene_wg(small, True)
    off = key(small)
    assert off[at] is False and off[:at] + off[-2:] == on[:at] + on[-2:], "only the decision tells the two captures apart"
    assert key(big) == key(big)
    fake.use_social = False
    monkeypatch.setattr(ops, "SCENE_WG", True)
    assert key(small)[at] is False
