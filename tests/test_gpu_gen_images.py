"""The generator kernels with the weight images registered (sw_gen_images) against the same kernels without them, bit for
bit.  The image prologues load what the no-image prologues derive for themselves - the composed input map, fc4 . fc3, the
A-operand images - so both must run the very same arithmetic: ops.gen_forward(save=True) + ops.gen_backward once on the
raw weights and once inside _images (test_gpu_gen_reference.py; that also selects the eight-wave encoder), with
ops.SCENE_WG on and off, so that the scene-workgroup launch and the social-backward + observation-BPTT pair both read
their images.

17 agents in scenes of 1, 5 and 11: two 16-agent tiles, the second with one live lane, and a single-agent scene.  To = 3,
Tp = 3: the first, middle and last step forms of the backward all run.  The saved rows are compared on a NaN-prefilled
buffer, as bits: the same values in the same places."""
import pytest
import torch

from _ref64 import scene_rows
from test_gpu_gen_reference import _images, _inputs

pytestmark = pytest.mark.gpu

SIZES, TO, TP = (1, 5, 11), 3, 3


def _run(G, obsv, z, cot, scenes, images):
    from socialways_amd import _lib as L
    from socialways_amd import ops
    dev = obsv.device
    mods = (G.encoder, G.feature_embedder, G.attention, G.decoder)
    w = [m._flat for m in mods]
    grads = [torch.full_like(f, float("nan")) for f in w]
    ws = ops.Workspaces(dev)
    n_save = L.workspace_floats(L.WS_GSAVE, obsv.shape[0], TO, TP)
    ws.get("g.gsave", n_save).fill_(float("nan"))
    with _images(G, images):
        pred4, ctx = ops.gen_forward(*w, obsv, z, scenes, TP, True, save=True, ws=ws)
        ops.gen_backward(*w, ctx, cot, *grads, ws=ws)
        torch.cuda.synchronize()
    out = {"pred4": pred4, "hT": ctx.hT, "cT": ctx.cT, "S": ctx.S, "saved rows": ctx.gsave[:n_save].view(torch.int32)}
    for s0, s1 in scene_rows(SIZES):
        if s1 - s0 > 1:         # a single agent has no attention row; columns past the scene's agents are never written
            out["attn of the scene at %d" % s0] = ctx.attn[s0:s1, :s1 - s0]
    for m, g in zip(("encoder", "feature_embedder", "attention", "decoder"), grads):
        out["d " + m] = g
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("scene_wg", (True, False), ids=("scene_wg", "two_launches"))
def test_images_against_weights_bit_for_bit(scene_wg):
    import socialways_amd as sw
    from socialways_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(2064)
    G = sw.Generator(hidden_size=64, use_social=True, device=dev)
    G.unify()
    B = sum(SIZES)
    obsv, z, cot = (t.to(dev) for t in _inputs(B, TO, TP)(7))
    scenes = ops.SceneIndex(scene_rows(SIZES), B, dev)
    old, ops.SCENE_WG = ops.SCENE_WG, scene_wg
    try:
        assert ops.scene_wg(scenes, True) is scene_wg
        want = _run(G, obsv, z, cot, scenes, images=False)
        got = _run(G, obsv, z, cot, scenes, images=True)
    finally:
        ops.SCENE_WG = old
    for name in want:
        if not name.startswith("saved"):
            assert torch.isfinite(want[name]).all(), name
        n_diff = int((got[name] != want[name]).sum())
        print("%s: %d of %d differ" % (name, n_diff, want[name].numel()))
    for name in want:
        assert torch.equal(got[name], want[name]), name
    assert float(want["d decoder"].abs().max()) > 0 and float(want["d attention"].abs().max()) > 0
