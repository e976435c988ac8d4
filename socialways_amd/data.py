"""Host-side data glue of the training loop (reference train.py:86-124, 446-461 and the dataset
schema of create_toy.py:187 / create_dataset.py:14): npz {obsvs (N,To,2), preds (N,Tp,2), times (N,),
batches (S,2)} -> normalised device tensors + scene ranges, the greedy scene packing of train(),
and synthetic generators for the benchmark shapes (no dataset ships with the reference).
"""
import copy

import numpy as np
import torch

from ._lib import WALLS_MAX


class Scale(object):
    """Min-max, keep-ratio normalisation (utils/parse_utils.py:11-76)."""

    def __init__(self):
        self.min_x, self.max_x = +np.inf, -np.inf
        self.min_y, self.max_y = +np.inf, -np.inf
        self.sx, self.sy = 1, 1

    def calc_scale(self, keep_ratio=True):
        self.sx = 1 / (self.max_x - self.min_x)
        self.sy = 1 / (self.max_y - self.min_y)
        if keep_ratio:
            self.sx = self.sy = min(self.sx, self.sy)

    def normalize(self, data, shift=True, inPlace=True):
        out = data if inPlace else np.copy(data)
        out[..., 0] = (data[..., 0] - self.min_x * shift) * self.sx
        out[..., 1] = (data[..., 1] - self.min_y * shift) * self.sy
        return out

    def denormalize(self, data, shift=True, inPlace=False):
        out = data if inPlace else np.copy(data)
        out[..., 0] = data[..., 0] / self.sx + self.min_x * shift
        out[..., 1] = data[..., 1] / self.sy + self.min_y * shift
        return out


def check_obs_len(obs_len, B, To, lo):
    """Host data (list / numpy) given as obs_len -> int32 numpy (B,), or ValueError: not integers, not (B,), or a value
    outside lo .. To (lo = 2 for positions - the velocity rule needs two frames -, 1 for 4-d input)."""
    a = np.asarray(obs_len)
    if a.dtype.kind not in "iu":
        raise ValueError("obs_len must hold integers, got dtype %s" % a.dtype)
    if a.shape != (B,):
        raise ValueError("obs_len must be (B,) = (%d,), got %s" % (B, a.shape))
    if B and (a.min() < lo or a.max() > To):
        raise ValueError("obs_len must lie in %d .. To = %d, got %d .. %d" % (lo, To, a.min(), a.max()))
    return a.astype(np.int32)


def check_pred_len(pred_len, B, Tp):
    """The twin of check_obs_len for ragged FUTURES: host data (list / numpy) given as pred_len -> int32 numpy (B,), or
    ValueError: not integers, not (B,), or a value outside 1 .. Tp (valid frames per row of a left-aligned (B, Tp, .) future)."""
    a = np.asarray(pred_len)
    if a.dtype.kind not in "iu":
        raise ValueError("pred_len must hold integers, got dtype %s" % a.dtype)
    if a.shape != (B,):
        raise ValueError("pred_len must be (B,) = (%d,), got %s" % (B, a.shape))
    if B and (a.min() < 1 or a.max() > Tp):
        raise ValueError("pred_len must lie in 1 .. Tp = %d, got %d .. %d" % (Tp, a.min(), a.max()))
    return a.astype(np.int32)


class SceneDataset:
    """train.py:89-124: 4/5 of the scenes train, the rest test; float32 keep-ratio normalisation;
    tracks resident on the device for the whole run.  `batches` may be int16 on disk
    (utils/parse_utils.py:490 overflows above 32767 rows): widened to int64 here."""

    def __init__(self, obsvs, preds, batches, times=None, device="cuda", obs_len=None):
        obsvs = np.array(obsvs, dtype=np.float32, copy=True)
        preds = np.array(preds, dtype=np.float32, copy=True)
        self.the_batches = np.asarray(batches).astype(np.int64)
        self.times = None if times is None else np.asarray(times)
        self.train_size = max(1, (len(self.the_batches) * 4) // 5)
        # train.py:95-98: both splits are taken BEFORE the single-scene substitution below, which only feeds the
        # look-ahead `the_batches[ii + 1]` of the packing loop (a one-scene dataset has NO test scene: test() = zeros)
        self.train_batches = self.the_batches[:self.train_size]
        self.test_batches = self.the_batches[self.train_size:]
        self.n_past, self.n_next = obsvs.shape[1], preds.shape[1]
        self.n_train_samples = int(self.the_batches[self.train_size - 1][1])
        self.n_test_samples = obsvs.shape[0] - self.n_train_samples
        if self.n_test_samples == 0:                                         # train.py:107-109
            self.n_test_samples = 1
            self.the_batches = np.array([self.the_batches[0], self.the_batches[0]])
        sc = Scale()
        sc.max_x = max(np.max(obsvs[:, :, 0]), np.max(preds[:, :, 0]))
        sc.min_x = min(np.min(obsvs[:, :, 0]), np.min(preds[:, :, 0]))
        sc.max_y = max(np.max(obsvs[:, :, 1]), np.max(preds[:, :, 1]))
        sc.min_y = min(np.min(obsvs[:, :, 1]), np.min(preds[:, :, 1]))
        sc.calc_scale(keep_ratio=True)
        self.scale, self.ss = sc, sc.sx
        self.obsv = torch.from_numpy(sc.normalize(obsvs)).to(device)
        self.pred = torch.from_numpy(sc.normalize(preds)).to(device)
        # ragged histories (create_dataset_ragged): valid frames per row, right-aligned in obsv; int32 on the device, or None
        self.obs_len = None
        if obs_len is not None:
            self.obs_len = torch.from_numpy(check_obs_len(obs_len, obsvs.shape[0], self.n_past, 2)).to(device)

    # ragged futures (create_dataset_ragged(min_next=...)): valid frames per row, left-aligned in pred; int32 on the device,
    # or None.  Evaluation only: set through set_pred_len(), read by evaluate*(); the training calls refuse such a dataset.
    pred_len = None

    def set_pred_len(self, pred_len):
        """Attach the future lengths (N,) of create_dataset_ragged(min_next=...) - list, numpy array or tensor, 1 .. n_next -
        checked on the host and uploaded as int32; None detaches them.  Works on held_out() datasets too.  Returns self."""
        if pred_len is None:
            self.pred_len = None
            return self
        host = pred_len.cpu().numpy() if isinstance(pred_len, torch.Tensor) else pred_len
        self.pred_len = torch.from_numpy(check_pred_len(host, self.pred.shape[0], self.n_next)).to(self.pred.device)
        return self

    def walls_from_world(self, segments):
        """The static map of the recording in the coordinates of this dataset: world-coordinate segments (M, 4) - x0 y0 x1 y1 -
        or (M, 2, 2) - [w0, w1] -, M = 0 included, pass through the dataset's Scale.normalize (shift included) like the tracks
        -> float32 (M, 2, 2) on the device of the tracks: what path_walls / refine_plans / evaluate_walls take as `walls`."""
        seg = wall_segments(np.array(segments, dtype=np.float32, copy=True))
        return torch.from_numpy(self.scale.normalize(seg)).to(self.obsv.device)

    def maps_from_world(self, list_of_segments):
        """The maps of several recordings in the coordinates of this dataset: a sequence of world-coordinate wall sets, each as
        walls_from_world() takes it -> a WallMaps on the device of the tracks (set i = walls_from_world(list_of_segments[i]))."""
        return WallMaps([self.walls_from_world(s) for s in list_of_segments], self.obsv.device)

    # which map of a WallMaps every row sees (from_recordings(): the recording of the row): int32 (N,) on the device, or None.
    # Read by test_part(); the training and evaluation calls take one map and do not look at it.
    wall_map = None

    def set_wall_map(self, ids):
        """Attach the map index of every row: ids (N,) per row, or (S,) per scene of the_batches (every row of a scene then
        sees its scene's map) - list, numpy array or tensor of integers; an index outside the WallMaps it is used with means
        "no map".  Uploaded as int32; None detaches it.  Works on held_out() datasets too.  Returns self."""
        if ids is None:
            self.wall_map = None
            return self
        a = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids)
        if a.dtype.kind not in "iu":
            raise ValueError("wall_map ids must hold integers, got dtype %s" % a.dtype)
        N, S = self.obsv.shape[0], len(self.the_batches)
        if a.shape == (S,) and a.shape != (N,):
            sizes = self.the_batches[:, 1] - self.the_batches[:, 0]
            if int(sizes.sum()) != N:
                raise ValueError("per-scene ids need the_batches to cover the %d rows, they cover %d" % (N, int(sizes.sum())))
            rows = np.empty(N, dtype=a.dtype)
            for (lo, hi), v in zip(self.the_batches, a):
                rows[lo:hi] = v
            a = rows
        if a.shape != (N,):
            raise ValueError("wall_map ids must be (N,) = (%d,) per row or (S,) = (%d,) per scene, got %s" % (N, S, a.shape))
        self.wall_map = torch.from_numpy(a.astype(np.int32)).to(self.obsv.device)
        return self

    def test_part(self, i):
        """This dataset with the held-out scenes that see map i alone (a scene's map is that of its first row): the same
        tensors and coordinates, rows where they were - a DeviceNoise draws what it draws for the whole set -, test_batches
        and n_test_samples cut down.  evaluate_walls(data.test_part(i), maps[i]) judges recording i against its own map;
        the shares of the whole held-out set are the n_agents-weighted means of the parts."""
        if self.wall_map is None:
            raise ValueError("test_part() needs wall_map (SceneDataset.from_recordings, set_wall_map)")
        wm = self.wall_map.cpu().numpy()
        d = copy.copy(self)
        keep = [k for k, (a, b) in enumerate(self.test_batches) if int(wm[int(a)]) == int(i)]
        d.test_batches = self.test_batches[keep]
        d.n_test_samples = int(sum(int(b - a) for a, b in d.test_batches))
        return d

    @classmethod
    def from_recordings(cls, parts, device="cuda"):
        """One dataset from several recordings: parts = [(obsvs, preds, batches, times[, obs_len]), ...] in WORLD coordinates,
        each as the constructor takes it (batches covering the part's rows in order).  One Scale over all parts; the training
        part is the first 4/5 of EACH recording's scenes (at least one), and scenes and rows are laid out as all training
        scenes, recording by recording, then all test scenes, recording by recording: the_batches, train_batches,
        test_batches, n_train_samples and packed_steps() work as for one recording, and a recording's scenes stay adjacent (a
        packed batch holds the scenes of two recordings only where one ends).  wall_map = the recording of every row, the
        index into maps_from_world([...]) given in the same order.  times with one entry per row follow their rows, any other
        times are concatenated as they are; obs_len is given for every part or for none."""
        parts = [tuple(p) for p in parts]
        if not parts or any(len(p) not in (4, 5) for p in parts):
            raise ValueError("from_recordings takes a non-empty list of (obsvs, preds, batches, times[, obs_len])")
        if len(set(len(p) == 5 and p[4] is not None for p in parts)) != 1:
            raise ValueError("from_recordings: obs_len is given for every recording or for none")
        ragged = len(parts[0]) == 5 and parts[0][4] is not None
        obs = [np.asarray(p[0], dtype=np.float32) for p in parts]
        prd = [np.asarray(p[1], dtype=np.float32) for p in parts]
        bat = [np.asarray(p[2]).astype(np.int64).reshape(-1, 2) for p in parts]
        if any(len(b) == 0 for b in bat):
            raise ValueError("from_recordings: a recording without scenes")
        split = [max(1, (len(b) * 4) // 5) for b in bat]
        order = [(i, s) for i, b in enumerate(bat) for s in range(split[i])] \
            + [(i, s) for i, b in enumerate(bat) for s in range(split[i], len(b))]
        rows = [(i, int(bat[i][s, 0]), int(bat[i][s, 1])) for i, s in order]
        ends = np.cumsum([hi - lo for _, lo, hi in rows])
        d = cls.__new__(cls)
        d.the_batches = np.stack([ends - np.asarray([hi - lo for _, lo, hi in rows]), ends], axis=1).astype(np.int64)
        d.times = None
        if all(p[3] is not None for p in parts):
            tms = [np.asarray(p[3]) for p in parts]
            if all(len(t) == len(o) for t, o in zip(tms, obs)):      # one per row: they follow their rows (test() labels by row)
                d.times = np.concatenate([tms[i][lo:hi] for i, lo, hi in rows])
            else:
                d.times = np.concatenate(tms)
        d.train_size = int(sum(split))
        d.train_batches, d.test_batches = d.the_batches[:d.train_size], d.the_batches[d.train_size:]
        obsvs = np.concatenate([obs[i][lo:hi] for i, lo, hi in rows])
        preds = np.concatenate([prd[i][lo:hi] for i, lo, hi in rows])
        d.n_past, d.n_next = obsvs.shape[1], preds.shape[1]
        d.n_train_samples = int(d.the_batches[d.train_size - 1][1])
        d.n_test_samples = obsvs.shape[0] - d.n_train_samples
        sc = Scale()
        sc.max_x = max(np.max(obsvs[:, :, 0]), np.max(preds[:, :, 0]))
        sc.min_x = min(np.min(obsvs[:, :, 0]), np.min(preds[:, :, 0]))
        sc.max_y = max(np.max(obsvs[:, :, 1]), np.max(preds[:, :, 1]))
        sc.min_y = min(np.min(obsvs[:, :, 1]), np.min(preds[:, :, 1]))
        sc.calc_scale(keep_ratio=True)
        d.scale, d.ss = sc, sc.sx
        d.obsv = torch.from_numpy(sc.normalize(obsvs)).to(device)
        d.pred = torch.from_numpy(sc.normalize(preds)).to(device)
        d.obs_len = None
        if ragged:
            ol = np.concatenate([np.asarray(parts[i][4])[lo:hi] for i, lo, hi in rows])
            d.obs_len = torch.from_numpy(check_obs_len(ol, obsvs.shape[0], d.n_past, 2)).to(device)
        return d.set_wall_map(np.concatenate([np.full(hi - lo, i, dtype=np.int32) for i, lo, hi in rows]))

    @classmethod
    def held_out(cls, like, obsvs, preds, batches, times=None, obs_len=None, train=False):
        """Windows that a model trained on `like` is evaluated on: EVERY scene is a test scene (no training part), the
        coordinates are those of `like` - its scale, not one of these windows' own - and the tensors live on its device.
        What evaluate*() / evaluate_history() read; batches (S, 2) must cover rows 0 .. N-1.
        train=True: the other way round - every scene is a TRAINING scene (no test part) in like's coordinates: what
        train_epoch_ragged() reads when the ragged windows in front of like's held-out part join its training."""
        d = cls.__new__(cls)
        obsvs = np.array(obsvs, dtype=np.float32, copy=True)
        preds = np.array(preds, dtype=np.float32, copy=True)
        d.the_batches = np.asarray(batches).astype(np.int64).reshape(-1, 2)
        d.times = None if times is None else np.asarray(times)
        d.train_size, d.train_batches, d.test_batches = 0, d.the_batches[:0], d.the_batches
        d.n_past, d.n_next = obsvs.shape[1], preds.shape[1]
        d.n_train_samples, d.n_test_samples = 0, obsvs.shape[0]
        d.scale, d.ss = like.scale, like.ss
        d.obsv = torch.from_numpy(like.scale.normalize(obsvs)).to(like.obsv.device)
        d.pred = torch.from_numpy(like.scale.normalize(preds)).to(like.obsv.device)
        d.obs_len = None
        if obs_len is not None:
            d.obs_len = torch.from_numpy(check_obs_len(obs_len, obsvs.shape[0], d.n_past, 2)).to(like.obsv.device)
        if train:
            d.train_size, d.train_batches, d.test_batches = len(d.the_batches), d.the_batches, d.the_batches[:0]
            d.n_train_samples, d.n_test_samples = obsvs.shape[0], 0
        return d

    @classmethod
    def from_npz(cls, path, device="cuda"):
        d = np.load(path)
        out = cls(d["obsvs"], d["preds"], d["batches"], d["times"] if "times" in d.files else None, device,
                  d["obs_len"] if "obs_len" in d.files else None)
        return out.set_pred_len(d["pred_len"]) if "pred_len" in d.files else out

    def packed_steps(self, batch_size):
        """Greedy scene packing of train() (train.py:446-456): scenes are appended until the next one
        would exceed `batch_size` AGENTS.  Yields (row_start, row_end, sub_batches)
        with sub_batches already relative to row_start (train.py:461)."""
        tb, allb = self.train_batches, self.the_batches
        acc, subs = 0, []
        for ii, b in enumerate(tb):
            acc += int(b[1] - b[0])
            subs.append(b)
            if ii >= self.train_size - 1 or acc + int(allb[ii + 1][1] - allb[ii + 1][0]) > batch_size:
                a = int(subs[0][0])
                yield a, int(subs[-1][1]), np.asarray(subs, dtype=np.int64) - a
                acc, subs = 0, []


def wall_segments(x):
    """The one shape rule of a map: a numpy array or a tensor (M, 4) - x0 y0 x1 y1 - or (M, 2, 2) - [w0, w1] -, M = 0 included
    -> its view (M, 2, 2), or ValueError."""
    sh = tuple(x.shape)
    n = int(np.prod(sh))
    if n and (len(sh) not in (2, 3) or n // sh[0] != 4 or n % sh[0]):
        raise ValueError("walls must be (M, 2, 2) or (M, 4): the segments [w0, w1] = x0 y0 x1 y1, got %s" % (sh,))
    return x.reshape(-1, 2, 2)


class WallMaps:
    """A set of maps for batches whose agents see different ones - scenes of several recordings in one packed batch:
    maps = a sequence of n_maps >= 1 wall sets, each what a single-map call takes - a tensor or host data, (M_i, 2, 2) or
    (M_i, 4), M_i = 0 .. 1024 (SW_WALLS_MAX), in the coordinates of the paths.  Checked on the host (ValueError).
      walls    (Mtot, 2, 2) float32 on `device`: the sets one after the other; Mtot is not capped, only int32;
      ptr      (n_maps + 1,) int32 on `device`: set i = walls[ptr[i]:ptr[i + 1]]; ptr_host: its numpy copy;
      n_maps, len(maps);  maps[i]: the view of set i - a valid `walls` of every single-map call.
    Which set a row sees is given per row, like obs_len: SceneDataset.wall_map (N,) int32, an index outside 0 .. n_maps - 1
    meaning "this agent has no map".  The wall calls take ONE map per call (path_walls, wall_penalty, set_wall_loss,
    evaluate_walls, refine_plans): a mixed set is worked through map by map - maps[i] on the rows with wall_map == i."""

    def __init__(self, maps, device="cuda"):
        sets = []
        for m in maps:
            w = torch.as_tensor(m if isinstance(m, torch.Tensor) else np.asarray(m), dtype=torch.float32)
            w = wall_segments(w)
            if w.shape[0] > WALLS_MAX:
                raise ValueError("a map holds at most %d walls, got %d" % (WALLS_MAX, w.shape[0]))
            sets.append(w)
        if not sets:
            raise ValueError("WallMaps needs at least one map (an empty one counts)")
        ptr = np.concatenate([[0], np.cumsum([w.shape[0] for w in sets], dtype=np.int64)])
        if ptr[-1] > 0x7fffffff:
            raise ValueError("the maps hold %d walls in all: more than int32 offsets reach" % ptr[-1])
        self.n_maps = len(sets)
        self.ptr_host = ptr.astype(np.int32)
        self.walls = torch.cat([w.to(device) for w in sets]).contiguous()
        self.ptr = torch.from_numpy(self.ptr_host).to(device)

    def __len__(self):
        return self.n_maps

    def __getitem__(self, i):
        i = range(self.n_maps)[i]
        return self.walls[int(self.ptr_host[i]):int(self.ptr_host[i + 1])]


def load_walls(path):
    """A map file -> world-coordinate segments (M, 4) float32: one `x0 y0 x1 y1` line per wall, `#` starts a comment, blank
    lines are skipped; a file without walls gives (0, 4).  SceneDataset.walls_from_world() takes them into a dataset's
    coordinates."""
    rows = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            line = line.split("#", 1)[0].split()
            if not line:
                continue
            if len(line) != 4:
                raise ValueError("%s:%d: a wall is `x0 y0 x1 y1`, got %d fields" % (path, n, len(line)))
            rows.append([float(v) for v in line])
    return np.asarray(rows, dtype=np.float32).reshape(-1, 4)


def synth_tracks(n_scenes, agents, n_past=8, n_next=12, seed=1234):
    """Synthetic crowd of SURVEY §8d: p0~U[0,10)^2, v = N(0,0.3^2) (per agent) + cumsum_t N(0,0.05^2),
    track = p0 + cumsum_t v, float32, scenes contiguous.  `agents`: int or per-scene list."""
    rng = np.random.default_rng(seed)
    sizes = [int(agents)] * n_scenes if np.isscalar(agents) else [int(a) for a in agents]
    N, T = int(np.sum(sizes)), n_past + n_next
    p0 = rng.uniform(0, 10, size=(N, 1, 2))
    v = rng.normal(0, 0.3, size=(N, 1, 2)) + np.cumsum(rng.normal(0, 0.05, size=(N, T, 2)), axis=1)
    track = (p0 + np.cumsum(v, axis=1)).astype(np.float32)
    ends = np.cumsum(sizes)
    batches = np.stack([ends - np.asarray(sizes), ends], axis=1).astype(np.int64)
    times = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    return dict(obsvs=track[:, :n_past], preds=track[:, n_past:], times=times, batches=batches)


def ragged_scene_sizes(n_agents=2048, max_agents=8, seed=77):
    """Scene sizes of a real-shaped packed batch: ETH/UCY recordings hold 1..8 pedestrians per timestamp and
    train.py:446-461 packs whole scenes up to --batch-size agents; uniform 1..max_agents until the batch holds exactly
    `n_agents` agents (single-agent scenes included)."""
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < n_agents:
        sizes.append(int(rng.integers(1, max_agents + 1)))
    sizes[-1] -= sum(sizes) - n_agents
    return [a for a in sizes if a > 0]


def toy_tracks(n_samples=768, n_conditions=8, n_modes=3, n_per_batch=6, seed=30):
    """The toy multi-modal set of create_toy.py:11-54 + its npz packing (:162-187): 4-point tracks
    (2 observed + 2 to predict) approaching the origin from `n_conditions` directions and turning
    by one of `n_modes` angles.  Draw order per sample: one uniform for the 3rd point, one for the
    4th, numpy legacy seed 30 (create_toy.py:37-48,145)."""
    rs = np.random.RandomState(seed)
    samples, stamps = np.zeros((n_samples, 4, 2)), np.zeros(n_samples)
    for ii in range(n_samples):
        way = (ii * n_conditions) // n_samples
        w_i = way % (n_conditions / n_per_batch)
        t0 = ii % (n_samples // n_conditions) + w_i * (n_samples // n_conditions)
        ang = way * (2.0 * np.pi / n_conditions)
        turn = ((ii % n_modes) - n_modes // 2) * 16 * np.pi / 180
        r2 = (rs.rand() - 0.5) * 4 * np.pi / 180
        r3 = (rs.rand() - 0.5) * 6 * np.pi / 180
        samples[ii] = [[np.cos(ang) * 4, np.sin(ang) * 4], [np.cos(ang) * 3, np.sin(ang) * 3],
                       [np.cos(ang + turn + r2) * 2, np.sin(ang + turn + r2) * 2],
                       [np.cos(ang + turn + r2 + r3), np.sin(ang + turn + r2 + r3)]]
        stamps[ii] = t0 * 4
    samples = samples / 4
    groups = {}
    for ii in range(n_samples):                                              # scene = identical first timestamp
        groups.setdefault(stamps[ii], []).append(ii)
    obsvs, preds, times, batches = [], [], [], []
    for key, idx in groups.items():
        batches.append([len(obsvs), len(obsvs) + len(idx)])
        for k in idx:
            obsvs.append(samples[k][:2])
            preds.append(samples[k][2:])
            times.append(stamps[k])
    return dict(obsvs=np.array(obsvs).astype(np.float32), preds=np.array(preds).astype(np.float32),
                times=np.array(times).astype(np.int32), batches=np.array(batches))


def shard_scenes(sub_batches, world_size):
    """Contiguous, scene-aligned split of one packed batch over `world_size` ranks (never splits a
    scene), balanced by a per-scene cost of agents + pairs/8 (the social block is O(n^2), the LSTM
    / decoder O(n)).  Returns [(scene_lo, scene_hi)] per rank; trailing ranks may get (k,k)."""
    sb = np.asarray(sub_batches, dtype=np.int64).reshape(-1, 2)
    n = sb[:, 1] - sb[:, 0]
    cost = n + (n * n) / 8.0
    csum = np.concatenate([[0.0], np.cumsum(cost)])
    total = csum[-1]
    cuts = [0]
    for r in range(1, world_size):
        target = total * r / world_size
        k = int(np.searchsorted(csum, target, side="left"))
        if k > 0 and abs(csum[k - 1] - target) <= abs(csum[min(k, len(csum) - 1)] - target):
            k -= 1
        cuts.append(min(max(k, cuts[-1]), len(sb)))
    cuts.append(len(sb))
    return [(cuts[r], cuts[r + 1]) for r in range(world_size)]


# ------------------------------------------------------------------------------------------------
# Dataset preparation: BIWI/ETH "obsmat.txt" -> sliding windows -> scenes.
# Reference: utils/parse_utils.py:231-320 (BIWIParser.load), :457-508 (create_dataset),
# create_dataset.py:1-15.  Offline, host-side, numpy.
# ------------------------------------------------------------------------------------------------
def write_biwi_obsmat(path, frames, ids, pos, vel=None):
    """Write tracks in the BIWI column layout [frame, id, px, pz, py, vx, vz, vy] (the parser reads
    columns 0,1,2,4,5,7; parse_utils.py:273-283).  Rows are written in the order given."""
    frames, ids, pos = np.asarray(frames), np.asarray(ids), np.asarray(pos, dtype=np.float64)
    vel = np.zeros_like(pos) if vel is None else np.asarray(vel, dtype=np.float64)
    with open(path, "w") as f:
        for t, i, p, v in zip(frames, ids, pos, vel):
            f.write("%.7e %.7e %.7e %.7e %.7e %.7e %.7e %.7e\n" % (t, i, p[0], 0.0, p[1], v[0], 0.0, v[1]))


def parse_biwi(path, down_sample=1):
    """BIWIParser.load for a single file: per-pedestrian position / time arrays in first-appearance
    order and the frame interval of the first pedestrian with two samples (parse_utils.py:300-305).
    Returns (p_data, t_data, interval)."""
    delim = "\t" if "zara" in path else " "
    order, pos, tim = [], {}, {}
    with open(path) as f:
        for line in f:
            row = [c for c in line.split(delim) if c != ""]
            if len(row) < 8:
                continue
            ts = float(row[0])
            pid = round(float(row[1]))
            if ts % down_sample != 0:
                continue
            if pid not in pos:
                order.append(pid)
                pos[pid], tim[pid] = [], []
            pos[pid].append((float(row[2]), float(row[4])))
            tim[pid].append(ts)
    interval = -1
    for pid in order:
        if len(tim[pid]) > 1:
            d = int(round(tim[pid][1] - tim[pid][0]))
            if d > 0:
                interval = d
                break
    p_data = [np.array(pos[k]) for k in order]
    t_data = [np.array(tim[k]).astype(np.int32) for k in order]
    return p_data, t_data, interval


def create_dataset(p_data, t_data, t_range, n_past=8, n_next=12):
    """Sliding windows of n_past + n_next samples (parse_utils.py:457-508): for every integer t of
    `t_range` (stepping by 1, like the reference) and every pedestrian that has samples at
    t - step*n_past, t and t + step*(n_next-1): obs = the n_past samples before t, pred = the n_next
    from t on.  A scene = the windows sharing t.  Returns (obsvs f32, preds f32, times list,
    batches int64); the reference stores `batches` as int16 (overflow above 32767 rows)."""
    step = t_range.step
    index = [dict((int(t), k) for k, t in reversed(list(enumerate(td)))) for td in t_data]   # first occurrence wins
    t0s, xs, ys = [], [], []
    for t in range(t_range.start, t_range.stop, 1):
        for i, ix in enumerate(index):
            a, b, c = ix.get(t - step * n_past), ix.get(t), ix.get(t + step * (n_next - 1))
            if a is None or b is None or c is None:
                continue
            t0s.append(t)
            xs.append(p_data[i][a:b])
            ys.append(p_data[i][b:c + 1])
    keep, batches = _scene_runs(t0s)
    obsvs = np.array([xs[k] for k in keep]).astype(np.float32)
    preds = np.array([ys[k] for k in keep]).astype(np.float32)
    return obsvs, preds, t0s, batches


def _scene_runs(t0s):
    """The scenes of create_dataset(): runs of windows sharing t (min_interval = 1, parse_utils.py:481-489) ->
    (rows kept, in order; batches int64 (S, 2) over the kept rows)."""
    batches, keep, last_t = [], [], -1000
    for i, t in enumerate(t0s):
        if t > last_t + 1:
            batches.append([i, i + 1])
            last_t = t
        if t == last_t:
            batches[-1][1] = i + 1
    out_b, last = [], 0
    for a, b in batches:
        keep += list(range(a, b))
        out_b.append([last, last + (b - a)])
        last += b - a
    return keep, np.array(out_b, dtype=np.int64)


def create_dataset_ragged(p_data, t_data, t_range, n_past=8, n_next=12, min_past=2, min_next=None):
    """create_dataset() that also keeps the pedestrians with a SHORT history: one is kept at t if it has samples at t and at
    t + step*(n_next-1), and its history n is the largest j in min_past .. n_past with a sample at t - step*j exactly j
    entries before t (none: dropped).  obsvs stay (N, n_past, 2), RIGHT-ALIGNED: row r holds its obs_len[r] samples before
    t in its last columns, the columns in front repeat the first valid sample (a real, finite position, so the
    normalisation of SceneDataset is the one of the valid samples).  Windows are ordered and grouped into scenes as in
    create_dataset(); with min_past == n_past the first four outputs are create_dataset()'s for tracks without gaps (a gap
    inside the history: create_dataset() only asks for a sample at t - step*n_past, this builder for n_past samples).
    Returns (obsvs f32, preds f32, times list, batches int64, obs_len int32 (N,)).
    min_next (1 .. n_next; None = the above): pedestrians with a SHORT FUTURE are kept as well - evaluation windows.  One is
    kept at t if it has a sample at t and a history as above; its future m is the largest j in min_next .. n_next with the
    sample at t + step*(j-1) exactly j-1 entries after the one at t (no gap inside the future; none: dropped).  preds stay
    (N, n_next, 2), LEFT-ALIGNED, the columns behind the m valid ones repeating the last valid sample (finite, a real
    position), and a sixth output pred_len int32 (N,) holds m.  With min_next == n_next the first five outputs are those of
    min_next=None for tracks without gaps."""
    n_past, min_past = int(n_past), int(min_past)
    if not 1 <= min_past <= n_past:
        raise ValueError("min_past must lie in 1 .. n_past = %d, got %d" % (n_past, min_past))
    if min_next is not None:
        if int(min_next) != min_next or not 1 <= int(min_next) <= int(n_next):
            raise ValueError("min_next must be an integer in 1 .. n_next = %d, got %r" % (n_next, min_next))
        min_next = int(min_next)
    step = t_range.step
    index = [dict((int(t), k) for k, t in reversed(list(enumerate(td)))) for td in t_data]   # first occurrence wins
    t0s, xs, ys, ns, ms = [], [], [], [], []
    for t in range(t_range.start, t_range.stop, 1):
        for i, ix in enumerate(index):
            b = ix.get(t)
            if b is None:
                continue
            if min_next is None:
                c, m = ix.get(t + step * (n_next - 1)), n_next
            else:
                m = next((j for j in range(n_next, min_next - 1, -1) if ix.get(t + step * (j - 1)) == b + j - 1), 0)
                c = b + m - 1 if m else None
            if c is None:
                continue
            n = next((j for j in range(n_past, min_past - 1, -1) if ix.get(t - step * j) == b - j and b - j >= 0), 0)
            if n == 0:
                continue
            o = p_data[i][b - n:b]
            t0s.append(t)
            xs.append(np.concatenate([np.repeat(o[:1], n_past - n, axis=0), o]))
            y = p_data[i][b:c + 1]
            ys.append(y if min_next is None else np.concatenate([y, np.repeat(y[-1:], n_next - m, axis=0)]))
            ns.append(n)
            ms.append(m)
    keep, batches = _scene_runs(t0s)
    obsvs = np.array([xs[k] for k in keep]).astype(np.float32)
    preds = np.array([ys[k] for k in keep]).astype(np.float32)
    obs_len = np.array([ns[k] for k in keep], dtype=np.int32)
    if min_next is None:
        return obsvs, preds, t0s, batches, obs_len
    return obsvs, preds, t0s, batches, obs_len, np.array([ms[k] for k in keep], dtype=np.int32)


def biwi_to_npz(obsmat_path, npz_path, n_past=8, n_next=12, min_past=None):
    """create_dataset.py:1-15: obsmat.txt -> npz {obsvs, preds, times, batches}.  min_past: the windows of
    create_dataset_ragged(min_past=...) instead, and `obs_len` with them (also returned, fifth)."""
    p_data, t_data, interval = parse_biwi(obsmat_path)
    t_range = range(int(t_data[0][0]), int(t_data[-1][-1]), interval)
    if min_past is None:
        obsvs, preds, times, batches = create_dataset(p_data, t_data, t_range, n_past, n_next)
        np.savez(npz_path, obsvs=obsvs, preds=preds, times=times, batches=batches)
        return obsvs, preds, times, batches
    obsvs, preds, times, batches, obs_len = create_dataset_ragged(p_data, t_data, t_range, n_past, n_next, min_past)
    np.savez(npz_path, obsvs=obsvs, preds=preds, times=times, batches=batches, obs_len=obs_len)
    return obsvs, preds, times, batches, obs_len


def biwi_to_npz_ragged(obsmat_path, npz_path, n_past=8, n_next=12, min_past=2, min_next=1):
    """biwi_to_npz for evaluation windows with short histories AND short futures: obsmat.txt -> npz {obsvs, preds, times,
    batches, obs_len, pred_len} of create_dataset_ragged(min_past=, min_next=); the six arrays are returned as well."""
    p_data, t_data, interval = parse_biwi(obsmat_path)
    t_range = range(int(t_data[0][0]), int(t_data[-1][-1]), interval)
    obsvs, preds, times, batches, obs_len, pred_len = create_dataset_ragged(p_data, t_data, t_range, n_past, n_next, min_past,
                                                                            min_next)
    np.savez(npz_path, obsvs=obsvs, preds=preds, times=times, batches=batches, obs_len=obs_len, pred_len=pred_len)
    return obsvs, preds, times, batches, obs_len, pred_len


def synth_crowd_frames(n_frames=60, n_ped=24, interval=6, seed=3, max_life=40):
    """A synthetic ETH-like recording (no ETH/UCY data is available): pedestrians enter at
    random frames, walk with slowly varying velocity for a random life span; returned frame-major
    like obsmat.txt (frames, ids, positions, velocities)."""
    rng = np.random.default_rng(seed)
    rows = []
    for pid in range(1, n_ped + 1):
        t_in = int(rng.integers(0, max(1, n_frames - 22)))
        life = int(rng.integers(21, max_life))
        p = rng.uniform(-5, 5, size=2)
        v = rng.normal(0, 0.4, size=2)
        for k in range(min(life, n_frames - t_in)):
            rows.append(((t_in + k) * interval, pid, p.copy(), v.copy()))
            v = v + rng.normal(0, 0.03, size=2)
            p = p + v * 0.4
    rows.sort(key=lambda r: (r[0], r[1]))
    return (np.array([r[0] for r in rows], dtype=np.float64), np.array([r[1] for r in rows], dtype=np.float64),
            np.array([r[2] for r in rows]), np.array([r[3] for r in rows]))
