"""Several recordings in one dataset, without a GPU: WallMaps (a set of maps, one after the other, with offsets),
SceneDataset.set_wall_map (the map every row sees), SceneDataset.from_recordings (one dataset from several recordings: one
scale, the first 4/5 of every recording's scenes train, a recording's scenes adjacent, wall_map = the recording of every row)
and SceneDataset.maps_from_world; every single map of a WallMaps stays a valid `walls` of the single-map calls."""
import inspect

import numpy as np
import pytest
import torch

import _wall_maps_cases as C


# ---- WallMaps ----------------------------------------------------------------------------------------------------------------
def test_wall_maps_holds_the_sets_one_after_the_other():
    import socialways_amd as sw
    from socialways_amd import _lib as L
    rng = np.random.RandomState(0)
    sets = [np.zeros((0, 4), np.float32), rng.rand(5, 4).astype(np.float32), torch.rand(L.WALLS_MAX, 2, 2), rng.rand(3, 2, 2).tolist(),
            torch.zeros(0, 2, 2)]
    m = sw.WallMaps(sets, device="cpu")
    assert m.n_maps == len(m) == 5 and tuple(m.walls.shape) == (5 + L.WALLS_MAX + 3, 2, 2) and m.walls.dtype == torch.float32
    assert m.ptr.dtype == torch.int32 and m.ptr.tolist() == [0, 0, 5, 5 + L.WALLS_MAX, 8 + L.WALLS_MAX, 8 + L.WALLS_MAX]
    assert m.ptr_host.dtype == np.int32 and m.ptr_host.tolist() == m.ptr.tolist() and m.walls.is_contiguous()
    for i, s in enumerate(sets):
        want = torch.as_tensor(np.asarray(s) if not torch.is_tensor(s) else s, dtype=torch.float32).reshape(-1, 2, 2)
        assert torch.equal(m[i], want), i
    assert m[1].data_ptr() == m.walls.data_ptr() and m[2].data_ptr() == m.walls[5:].data_ptr(), "maps[i] is a view"
    m.walls[5, 0, 0] = 42.0
    assert float(m[2][0, 0, 0]) == 42.0 and torch.equal(m[-1], m[4])
    with pytest.raises(IndexError):
        m[5]
    from socialways_amd import ops
    assert ops.check_walls(m[2])[1] == L.WALLS_MAX and ops.walls_arg(m[1], "cpu").data_ptr() == m[1].data_ptr(), \
        "maps[i] is a valid walls argument of the single-map calls"
    one = sw.WallMaps([np.zeros((0, 4))], device="cpu")
    assert one.n_maps == 1 and one.ptr.tolist() == [0, 0] and tuple(one.walls.shape) == (0, 2, 2)


def test_wall_maps_refuses_what_no_call_could_take():
    import socialways_amd as sw
    from socialways_amd import _lib as L
    ok = np.zeros((3, 4), np.float32)
    for bad in ([], [ok, np.zeros((L.WALLS_MAX + 1, 4))], [np.zeros((3, 3))], [ok, np.zeros((2, 2, 3))], [np.zeros(4)], [np.zeros((2, 3, 2))],
                torch.zeros(3, 2, 2), torch.zeros(3, 4)):
        with pytest.raises(ValueError):
            sw.WallMaps(bad, device="cpu")


# ---- the data layer ------------------------------------------------------------------------------------------------------------
def test_set_wall_map_per_row_and_per_scene():
    import socialways_amd as sw
    tracks = sw.synth_tracks(5, [3, 1, 4, 2, 6], seed=3)
    data = sw.SceneDataset(tracks["obsvs"], tracks["preds"], tracks["batches"], device="cpu")
    assert data.wall_map is None and sw.SceneDataset.wall_map is None
    per_scene = [2, 0, -1, 1, 7]
    per_row = np.repeat(per_scene, [3, 1, 4, 2, 6])
    assert data.set_wall_map(per_scene) is data
    a = data.wall_map.clone()
    assert a.dtype == torch.int32 and a.tolist() == per_row.tolist()
    assert torch.equal(data.set_wall_map(per_row).wall_map, a) and torch.equal(data.set_wall_map(torch.as_tensor(per_row)).wall_map, a)
    assert data.set_wall_map(None).wall_map is None
    for bad in ([0.5] * 16, [0] * 4, np.zeros((16, 1), np.int32)):
        with pytest.raises(ValueError):
            data.set_wall_map(bad)
    held = sw.SceneDataset.held_out(data, tracks["obsvs"][:8], tracks["preds"][:8], [[0, 3], [3, 4], [4, 8]])
    assert held.set_wall_map([1, 0, 1]).wall_map.tolist() == [1, 1, 1, 0, 1, 1, 1, 1]


def test_from_recordings(tmp_path):
    import socialways_amd as sw
    parts = [C.recording(tmp_path, 3), C.recording(tmp_path, 4, one_scene=True), C.recording(tmp_path, 5, n_frames=50, n_ped=16)]
    assert len(parts[1][2]) == 1 and all(len(p[2]) >= 5 for p in (parts[0], parts[2]))
    data = sw.SceneDataset.from_recordings(parts, device="cpu")
    N = sum(len(p[0]) for p in parts)
    split = [max(1, len(p[2]) * 4 // 5) for p in parts]
    tb = data.the_batches
    assert tuple(data.obsv.shape) == (N, 8, 2) and tuple(data.pred.shape) == (N, 12, 2)
    assert tb[0, 0] == 0 and tb[-1, 1] == N and (tb[1:, 0] == tb[:-1, 1]).all() and (tb[:, 1] > tb[:, 0]).all(), "rows are contiguous"
    assert data.train_size == sum(split) and len(data.train_batches) == sum(split) and len(tb) == sum(len(p[2]) for p in parts)
    assert data.n_train_samples == int(data.train_batches[-1, 1]) and data.n_test_samples == N - data.n_train_samples
    # every scene, in the order training scenes recording by recording, then test scenes: de-normalised it is the input
    want = [(i, s) for i in range(3) for s in range(split[i])] + [(i, s) for i in range(3) for s in range(split[i], len(parts[i][2]))]
    o = data.scale.denormalize(data.obsv.numpy())
    p = data.scale.denormalize(data.pred.numpy())
    wm = data.wall_map.numpy()
    assert data.wall_map.dtype == torch.int32 and wm.shape == (N,)
    for (lo, hi), (i, s) in zip(tb, want):
        a, b = parts[i][2][s]
        assert hi - lo == b - a and (wm[lo:hi] == i).all(), "wall_map is the recording of the row"
        np.testing.assert_allclose(o[lo:hi], parts[i][0][a:b], rtol=0, atol=2e-5 * np.abs(parts[i][0]).max())
        np.testing.assert_allclose(p[lo:hi], parts[i][1][a:b], rtol=0, atol=2e-5 * np.abs(parts[i][1]).max())
    assert [i for i, _ in want[:sum(split)]] == sorted(i for i, _ in want[:sum(split)]), "a recording's scenes stay adjacent"
    assert float(data.obsv.min()) >= 0 and float(data.pred.min()) >= 0 and max(float(data.obsv.max()), float(data.pred.max())) <= 1 + 1e-6
    assert min(float(data.obsv.min()), float(data.pred.min())) == 0.0, "one Scale over all parts"
    assert len(data.times) == N and all(len(q[3]) == len(q[0]) for q in parts)
    for (lo, hi), (i, k) in zip(tb, want):
        a, b = parts[i][2][k]
        assert list(data.times[lo:hi]) == list(parts[i][3][a:b]), "times follow their rows"
    # packed_steps: the training scenes in order, whole, none lost
    seen = []
    for a, b, sb in data.packed_steps(24):
        assert sb[0, 0] == 0 and (sb[1:, 0] == sb[:-1, 1]).all() and sb[-1, 1] == b - a
        seen += [(a + lo, a + hi) for lo, hi in sb]
    assert seen == [tuple(r) for r in data.train_batches.tolist()]
    # the maps of the recordings in the dataset's coordinates
    maps = data.maps_from_world([C.box_walls(q[1]) for q in parts])
    assert isinstance(maps, sw.WallMaps) and maps.n_maps == 3 and maps.ptr.tolist() == [0, 4, 8, 12]
    assert torch.equal(maps[1], data.walls_from_world(C.box_walls(parts[1][1])))
    # the held-out scenes of one recording: rows where they were, the counts cut down
    n_test = [sum(int(b - a) for a, b in q[2][split[i]:]) for i, q in enumerate(parts)]
    for i in range(3):
        d = data.test_part(i)
        assert d.obsv is data.obsv and d.scale is data.scale and d.n_test_samples == n_test[i] and d is not data
        assert all((wm[a:b] == i).all() for a, b in d.test_batches) and len(d.test_batches) == len(parts[i][2]) - split[i]
    assert n_test[1] == 0 and sum(n_test) == data.n_test_samples and len(data.test_part(7).test_batches) == 0
    assert len(data.test_batches) == sum(len(q[2]) - k for q, k in zip(parts, split)), "the whole set is untouched"
    with pytest.raises(ValueError):
        sw.SceneDataset(parts[0][0], parts[0][1], parts[0][2], device="cpu").test_part(0)
    with pytest.raises(ValueError):
        sw.SceneDataset.from_recordings([], device="cpu")
    with pytest.raises(ValueError):
        sw.SceneDataset.from_recordings([parts[0], parts[2] + (np.full(len(parts[2][0]), 8),)], device="cpu")
    ragged = sw.SceneDataset.from_recordings([q + (np.full(len(q[0]), 2 + i, np.int32),) for i, q in enumerate(parts)], device="cpu")
    assert torch.equal(ragged.obs_len, ragged.wall_map + 2)


def test_a_map_of_the_set_goes_to_the_single_map_calls_and_the_set_itself_is_refused():
    """maps[i] is what set_wall_loss / ops.check_walls take; the WallMaps itself is no `walls` of a call that takes one map."""
    import socialways_amd as sw
    from socialways_amd import ops
    m = sw.WallMaps([np.zeros((3, 4)), np.ones((2, 4))], device="cpu")
    tr = object.__new__(sw.SocialWaysTrainer)
    tr.device = torch.device("cpu")
    tr.set_wall_loss(m[1], 0.2)
    assert tr.wall_loss[0].data_ptr() == m[1].data_ptr() and tuple(tr.wall_loss[0].shape) == (2, 2, 2), "held, not copied"
    for call in (lambda: tr.set_wall_loss(m, 0.2), lambda: ops.walls_arg(m, "cpu"), lambda: ops.check_walls(m)):
        with pytest.raises((ValueError, TypeError)):
            call()


def test_signatures():
    import socialways_amd as sw

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(sw.WallMaps.__init__) == [("self", E), ("maps", E), ("device", "cuda")]
    assert sig(sw.SceneDataset.from_recordings) == [("parts", E), ("device", "cuda")]
    assert sig(sw.SceneDataset.set_wall_map) == [("self", E), ("ids", E)]
    assert sig(sw.SceneDataset.maps_from_world) == [("self", E), ("list_of_segments", E)]
    assert sig(sw.SceneDataset.test_part) == [("self", E), ("i", E)]
    assert "WallMaps" in sw.__all__
