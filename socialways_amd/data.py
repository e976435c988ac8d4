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

    def wall_grid_from_world(self, segments, reach, cell=None):
        """A map of any size in the coordinates of this dataset, under a grid: world-coordinate segments as walls_from_world()
        takes them, reach and cell in world units (both are multiplied by ss) -> a WallGrid on the device of the tracks."""
        ss = float(self.ss)
        return WallGrid(self.walls_from_world(segments), float(reach) * ss, None if cell is None else float(cell) * ss,
                        self.obsv.device)

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


def check_wall_grid(cell_ptr, cell_walls, wall_cells, nx, ny, M):
    """What the grid kernels index, checked on the host (numpy integer arrays): cell_ptr (nx ny + 1,) starts at 0, never
    descends and ends at len(cell_walls); every index of cell_walls lies in [0, M); wall_cells is (M, 4) and every range
    ix0 <= ix1, iy0 <= iy1 lies inside the nx x ny grid.  ValueError otherwise."""
    cell_ptr, cell_walls, wall_cells = np.asarray(cell_ptr), np.asarray(cell_walls), np.asarray(wall_cells)
    if nx < 1 or ny < 1 or nx * ny > WallGrid.MAX_CELLS:
        raise ValueError("a wall grid has 1 .. %d cells, got %d x %d" % (WallGrid.MAX_CELLS, nx, ny))
    if cell_ptr.shape != (nx * ny + 1,) or cell_ptr[0] != 0 or (np.diff(cell_ptr) < 0).any():
        raise ValueError("cell_ptr must be (nx ny + 1,), start at 0 and never descend")
    if cell_walls.ndim != 1 or int(cell_ptr[-1]) != cell_walls.shape[0]:
        raise ValueError("cell_ptr must end at the length of cell_walls, got %d and %d" % (cell_ptr[-1], cell_walls.size))
    if cell_walls.size and (cell_walls.min() < 0 or cell_walls.max() >= M):
        raise ValueError("cell_walls must hold wall indices in [0, %d)" % M)
    if wall_cells.shape != (M, 4):
        raise ValueError("wall_cells must be (M, 4) = (%d, 4), got %s" % (M, wall_cells.shape))
    if M and ((wall_cells[:, :2] < 0).any() or (wall_cells[:, 0] > wall_cells[:, 2]).any() or (wall_cells[:, 1] > wall_cells[:, 3]).any()
              or (wall_cells[:, 2] >= nx).any() or (wall_cells[:, 3] >= ny).any()):
        raise ValueError("every range of wall_cells must lie inside the %d x %d grid" % (nx, ny))


class WallGrid:
    """A map of any size under a uniform grid - the second form of "the map of a call": wherever a single-map call takes a
    (M, 2, 2) tensor as `walls` (ops / stats path_walls, wall_grad / wall_penalty, set_wall_loss, evaluate_walls) it takes a
    WallGrid, and then runs the grid kernels (sw_path_walls_grid, sw_wall_grad_grid), which visit only the walls near each path
    segment.  walls: a tensor or host data, (M, 2, 2) or (M, 4), in the coordinates of the paths, M >= 0 with no cap but int32.
    reach > 0, finite: the largest distance, in the walls' coordinates, any call may ask about (dw of the penalty, dist / inv_ss
    of path_walls - each must stay below reach by a relative 1e-5); kept as the fp32 number the kernels see.  cell: the edge of
    the square cells, default DEFAULT_CELL * reach (of reach, 2 reach and 4 reach the best over the launches measured: DESIGN.md section 9); the grid
    covers the bounding box of the walls and has at most MAX_CELLS cells - a smaller `cell` is enlarged to fit: `cell` holds
    the edge in use, `cell_asked` what was asked for.  Built with numpy in float64 from the float32 coordinates,
    deterministically, and checked on the host (ValueError).
      walls (M, 2, 2) float32, cell_ptr (nx ny + 1,) int32, cell_walls (L,) int32, wall_cells (M, 4) int32 on `device`: wall m
      is listed in EVERY cell of the cell range wall_cells[m] = (ix0, iy0, ix1, iy1) of its bounding box, cell c = iy nx + ix
      lists cell_walls[cell_ptr[c]:cell_ptr[c + 1]] in ascending order; cell_ptr_host, cell_walls_host, wall_cells_host: their
      numpy copies; origin (x0, y0): the fp32 lower corner; nx, ny, M, L, inv_cell (fp32).
    M = 0 gives a 1 x 1 grid with an empty list.  clear of path_walls saturates at +inf beyond reach (the one documented
    difference from a tensor map); refine_plans / plan_refine keep their walls in LDS and refuse a WallGrid."""
    MAX_CELLS = 1 << 20
    DEFAULT_CELL = 4.0       # in units of reach

    def __init__(self, walls, reach, cell=None, device="cuda"):
        w = torch.as_tensor(walls if isinstance(walls, torch.Tensor) else np.asarray(walls), dtype=torch.float32)
        host = np.ascontiguousarray(wall_segments(w).detach().cpu().numpy())
        M = host.shape[0]
        if not np.isfinite(host).all():
            raise ValueError("the walls of a WallGrid must be finite")
        if M > 0x7fffffff // 4:
            raise ValueError("a WallGrid holds %d walls: more than int32 offsets reach" % M)
        with np.errstate(over="ignore"):
            r32 = np.float32(reach)
            ok = np.isfinite(r32) and r32 > 0 and np.isfinite(r32 * r32) and r32 * r32 > 0
        if not ok:
            raise ValueError("reach must be finite and > 0 (and its square an fp32 number), got %r" % (reach,))
        self.reach = float(r32)
        asked = self.DEFAULT_CELL * self.reach if cell is None else float(cell)
        if not (np.isfinite(asked) and asked > 0.0):
            raise ValueError("cell must be finite and > 0, got %r" % (cell,))
        pts = host.reshape(-1, 2).astype(np.float64)
        lo = pts.min(0) if M else np.zeros(2)
        ext = pts.max(0) - lo if M else np.zeros(2)
        c = asked

        def dims(c):
            return int(np.floor(ext[0] / c)) + 1, int(np.floor(ext[1] / c)) + 1
        with np.errstate(over="ignore", divide="ignore"):
            while not (np.isfinite(ext / c).all() and dims(c)[0] * dims(c)[1] <= self.MAX_CELLS):
                c *= 1.25                                          # the cell cap: enlarge until the box fits
            inv32 = np.float32(1.0 / c)
        if not (np.isfinite(inv32) and inv32 > 0):
            raise ValueError("cell %r has no fp32 inverse" % c)
        nx, ny = dims(c)
        self.cell_asked, self.cell, self.inv_cell = asked, float(c), float(inv32)
        self.origin, self.nx, self.ny, self.M = (float(lo[0]), float(lo[1])), nx, ny, M
        # the cell range of every wall's bounding box, clamped into the grid
        seg = host.astype(np.float64)
        i0 = np.floor((seg.min(1) - lo) / c).astype(np.int64)
        i1 = np.floor((seg.max(1) - lo) / c).astype(np.int64)
        top = np.array([nx - 1, ny - 1])
        i0, i1 = np.clip(i0, 0, top), np.clip(i1, 0, top)
        wc = np.concatenate([i0, i1], 1).reshape(M, 4)
        wx, wy = i1[:, 0] - i0[:, 0] + 1, i1[:, 1] - i0[:, 1] + 1
        n = wx * wy
        Ltot = int(n.sum())
        if Ltot > 0x7fffffff:
            raise ValueError("the cell lists hold %d entries: more than int32 offsets reach - use a larger cell" % Ltot)
        wid = np.repeat(np.arange(M, dtype=np.int64), n)
        local = np.arange(Ltot, dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
        cid = (i0[wid, 1] + local // wx[wid]) * nx + i0[wid, 0] + local % wx[wid]
        order = np.argsort(cid, kind="stable")                    # wid ascends: the indices ascend within a cell
        self.cell_walls_host = wid[order].astype(np.int32)
        self.cell_ptr_host = np.concatenate([[0], np.cumsum(np.bincount(cid, minlength=nx * ny))]).astype(np.int32)
        self.wall_cells_host = wc.astype(np.int32)
        self.L = Ltot
        check_wall_grid(self.cell_ptr_host, self.cell_walls_host, self.wall_cells_host, nx, ny, M)
        self.walls = torch.from_numpy(host).to(device).contiguous()
        self.cell_ptr = torch.from_numpy(self.cell_ptr_host).to(device)
        self.cell_walls = torch.from_numpy(self.cell_walls_host).to(device)
        self.wall_cells = torch.from_numpy(self.wall_cells_host).to(device)

    @property
    def device(self):
        return self.walls.device

    def key(self):
        """The device addresses and sizes a captured launch bakes in: the grid's part of a graph key."""
        return (self.walls.data_ptr(), self.M, self.cell_ptr.data_ptr(), self.cell_walls.data_ptr(), self.L, self.wall_cells.data_ptr(),
                self.nx, self.ny, self.origin, self.inv_cell, self.reach)


def trace_occupancy(occ, to_world=None):
    """An obstacle image -> the walls around its obstacles: occ (H, W) boolean, True = occupied; pixel (r, c) covers
    [c, c + 1] x [r, r + 1], x the column and y the row; what lies outside the array is free.  A unit edge is a wall where
    exactly one of the two pixels it separates is occupied, and consecutive edges on one grid line merge into one maximal
    run.  Returns (M, 4) float32 `x0 y0 x1 y1`: the horizontal runs ordered by (y, x0), then the vertical ones by (x, y0).
    to_world: a 3 x 3 homography applied to (x, y, 1) of the end points (divided by the third component).  ETH's H.txt acts
    on (row, col, 1): swapping the first two columns of that matrix (`H[:, [1, 0, 2]]`) is the caller's."""
    occ = np.asarray(occ)
    if occ.ndim != 2 or occ.dtype != np.bool_:
        raise ValueError("occ must be a boolean (H, W) array, got %s %s" % (occ.dtype, occ.shape))
    P = np.pad(occ, 1)

    def runs(edge):
        """edge (n_lines, n): -> (line, first, behind-last) of every maximal run of True, in row-major order"""
        d = np.diff(np.pad(edge, ((0, 0), (1, 1))).astype(np.int8), axis=1)
        line, a = np.nonzero(d == 1)
        _, b = np.nonzero(d == -1)
        return line, a, b
    y, xa, xb = runs(P[:-1, 1:-1] != P[1:, 1:-1])                  # line y separates rows y - 1 and y
    x, ya, yb = runs((P[1:-1, :-1] != P[1:-1, 1:]).T)              # line x separates columns x - 1 and x
    seg = np.concatenate([np.stack([xa, y, xb, y], 1), np.stack([x, ya, x, yb], 1)]).astype(np.float64).reshape(-1, 4)
    if to_world is not None:
        Hm = np.asarray(to_world, np.float64)
        if Hm.shape != (3, 3):
            raise ValueError("to_world must be a 3 x 3 homography, got %s" % (Hm.shape,))
        p = np.concatenate([seg.reshape(-1, 2), np.ones((2 * seg.shape[0], 1))], 1) @ Hm.T
        seg = (p[:, :2] / p[:, 2:]).reshape(-1, 4)
    return seg.astype(np.float32)


def synth_occupancy(seed=0, H=480, W=640, n_rect=40, n_disc=30):
    """A synthetic obstacle image for trace_occupancy(): n_rect axis-aligned rectangles (sides 8 .. 60 pixels) and n_disc discs
    (radii 5 .. 30) at seeded random places of an (H, W) boolean array - the map the timing tools trace."""
    rng = np.random.RandomState(seed)
    occ = np.zeros((H, W), dtype=np.bool_)
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(n_rect):
        h, w = rng.randint(8, 61, 2)
        r, c = rng.randint(0, H - h), rng.randint(0, W - w)
        occ[r:r + h, c:c + w] = True
    for _ in range(n_disc):
        rad = rng.randint(5, 31)
        r, c = rng.randint(rad, H - rad), rng.randint(rad, W - rad)
        occ |= (yy - r) ** 2 + (xx - c) ** 2 <= rad * rad
    return occ


def load_occupancy(path, threshold=128, invert=False):
    """An obstacle image file -> (H, W) boolean for trace_occupancy(): a `.npy` array always, any image format through PIL when
    PIL is importable (imported here, not a dependency).  A boolean array is taken as it is, anything else is occupied where
    its value (grey level) >= threshold; invert flips the result."""
    if str(path).lower().endswith(".npy"):
        a = np.load(path)
    else:
        try:
            from PIL import Image
        except ImportError:
            raise ValueError("%s: reading an image needs PIL, which is not installed - convert it to a .npy array" % path)
        a = np.asarray(Image.open(path).convert("L"))
    if a.ndim != 2:
        raise ValueError("%s: an occupancy map is (H, W), got %s" % (path, a.shape))
    occ = a if a.dtype == np.bool_ else a >= threshold
    return ~occ if invert else occ


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
