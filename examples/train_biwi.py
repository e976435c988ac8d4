"""End-to-end example on a BIWI / ETH-format recording: the on-disk path a user of crowdbotp/socialways takes with
`create_dataset.py` + `train.py`, on the MI355X path.

    python examples/train_biwi.py --obsmat /data/eth/hotel/obsmat.txt --epochs 50 --out /tmp/sw_hotel
    python examples/train_biwi.py --epochs 10          # no recording at hand: a synthetic crowd in the same file format

* obsmat.txt [frame id px pz py vx vz vy] -> 8 + 12 step windows, one scene per timestamp   socialways_amd.biwi_to_npz
                                                               (utils/parse_utils.py:231-320, :457-508; create_dataset.py)
* the npz train.py loads ('../hotel-8-12.npz', train.py:56, 89-127)                          SceneDataset.from_npz
* packed batches of whole scenes up to --batch-size agents (train.py:446-456), train(), test() every 5 epochs with the
  prediction npz files visualize.py / calc_statistics.py read, checkpoint in the reference's format
* data parallel: `python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 examples/train_biwi.py ...`
  (one rank per GPU over RCCL; every packed batch is sharded scene-aligned, rank 0 evaluates and saves)
  `SW_ALLREDUCE=direct` exchanges the gradients through the library's own two-hop kernel over hipIpc-mapped peer buffers
  (one launch per optimizer step: exchange + Adam, inside the step's hipGraph) instead of RCCL's ring
* `--compose DIST`: the composed scene futures (evaluate_composed): one draw per agent - given the observations the agents'
  draws are independent, so any tuple of them is a joint sample -, the top-scored ones moved to other draws until no two chosen
  paths come closer than DIST; errors, scores and collision rates before and after.
* `--risk DIST`: the generator as a collision predictor (evaluate_risk): every held-out agent with company is the ego once, its
  true future the plan, the others' K draws the crowd; the predicted chance of coming within DIST of somebody against what
  happened (Brier score, against the index-paired estimate and the constant base rate).
* `--walls FILE[:DIST]`: the static map (`x0 y0 x1 y1` lines, world coordinates): the share of the K draws that walk through a
  wall (evaluate_walls); with `--refine` the walls join the refinement (evaluate_refine(walls=...)).
* `--refine DIST`: plan refinement (evaluate_refine): every held-out agent with company is the ego once, its naive plan the
  constant-velocity extrapolation of its track, moved away from the others' K draws by gradient descent on the expected
  clearance penalty at DIST - does the refined plan collide less with what the others really did?
* `--min-past M`: the held-out windows also keep the pedestrians seen for only M .. 7 frames (create_dataset_ragged:
  right-aligned observations + obs_len), so they are predicted and their neighbours see them; the errors are reported per
  history length (evaluate_history).  Training stays on full windows unless
* `--train-ragged` (with `--min-past M`): the ragged windows in front of the held-out part are what the model trains on
  (train_epoch_ragged: one eager step per packed batch on the unfused route, no graph capture - slower per step than
  train_epoch)
* `--ragged-fused` (with `--train-ragged`): SocialWaysTrainer(ragged_fused=True) - the ragged D updates in one launch each and
  the ragged steps graph-captured per layout like the dense ones (same weights and losses bit for bit)
* `--min-next M`: the held-out windows also keep the pedestrians whose track ends M .. 11 frames after t (ragged futures:
  create_dataset_ragged(min_next=M), left-aligned futures + pred_len), so they are predicted, scored against the frames
  they were seen for and stay in their neighbours' scenes; the errors are reported per future length (evaluate_horizon).
  Combines with `--min-past`.  Training windows are always built without it: a truncated future is no discriminator input.
* `--clearance-loss DIST[:W]`: train against collisions - the generator loss gains the scene-clearance term
  (set_clearance_loss(DIST, W), W default 1: pairs of predicted futures that come closer than DIST world units within a
  segment are pushed apart), and every test prints col_joint and col_agent of evaluate_scenes(coll_dist=DIST) beside ADE/FDE.
* `--map-image FILE[:HFILE]` (in place of `--walls`): the map from an obstacle image, as BIWI/ETH ship it (`map.png`, `H.txt`): the
  image (a `.npy` array, or any format PIL reads) is traced into the runs of its obstacle boundary (trace_occupancy), the runs go
  through the 3 x 3 homography of HFILE - ETH's acts on (row, col, 1) - and under a grid (data.wall_grid_from_world): thousands
  of walls, no cap, and the wall calls look only at the walls within `--map-reach D` (world units, default 1) of a path.
  `--refine` leaves such a map out: the refinement takes at most 1024 walls.
* `--wall-loss DIST[:W]` (with `--walls FILE` or `--map-image FILE`): train against the map - the generator loss gains the wall term
  (set_wall_loss(walls, DIST, W), W default 1: predicted segments closer than DIST world units to a wall are pushed off it);
  the numbers `--walls` prints at every test (wall_draws, wall_agents, wall_blocked) show what it buys.
* several recordings: give `--obsmat` more than once, and `--walls` as often and in the same order - one model on all of them
  (SceneDataset.from_recordings: one scale, the first 4/5 of every recording's scenes train, every row knows its recording);
  the maps become one WallMaps in the dataset's coordinates (data.maps_from_world) and the wall numbers are printed per
  recording: the held-out scenes of recording i against its own map (evaluate_walls(data.test_part(i), maps[i])).  The wall
  calls take one map per call, so `--wall-loss`, `--refine` and the ragged options stay with one recording.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import socialways_amd as sw  # noqa: E402


def ragged_windows(npz, like, train):
    """Of the recording's windows with histories of min_past .. n_past frames (`npz`, written by biwi_to_npz(min_past=...), or
    by biwi_to_npz_ragged(min_next=...) with futures of min_next .. n_next frames and `pred_len` as well) the
    scenes at or after the first held-out timestamp of `like` - the dataset of full windows, so none of them holds a
    training window - as an evaluation set in like's coordinates (SceneDataset.held_out), or with `train` the scenes in
    front of that timestamp as a training set in the same coordinates."""
    d = np.load(npz)
    obsvs, preds, times, batches, obs_len = d["obsvs"], d["preds"], np.asarray(d["times"]), d["batches"], d["obs_len"]
    t_split = like.times[like.n_train_samples]
    keep = [(a, b) for a, b in batches if (times[a] < t_split) == bool(train)]
    rows = np.concatenate([np.arange(a, b) for a, b in keep])
    ends = np.cumsum([b - a for a, b in keep])
    scenes = np.stack([np.concatenate([[0], ends[:-1]]), ends], axis=1)
    out = sw.SceneDataset.held_out(like, obsvs[rows], preds[rows], scenes, times[rows], obs_len[rows], train=train)
    return out.set_pred_len(d["pred_len"][rows]) if "pred_len" in d.files and not train else out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--obsmat", default=None, action="append",
                    help="BIWI obsmat.txt; default: a synthetic recording written to --out; more than once: one model on several "
                         "recordings")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=256)           # train.py --batch-size (agents per packed batch)
    ap.add_argument("--hidden-size", type=int, default=64)
    ap.add_argument("--social", type=int, default=1)
    ap.add_argument("--test-every", type=int, default=5)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--out", default="/tmp/sw_biwi")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-noise", type=int, default=None, metavar="SEED",
                    help="draw z on the device from the counter-based stream with this seed (sw.DeviceNoise: every rank fills "
                         "the rows of its shard, evaluation repeats call to call); default: the reference's host streams")
    ap.add_argument("--diverse", type=float, default=None, metavar="RADIUS",
                    help="also report the diverse top-5 of the K draws: modes kept by suppressing, in the discriminator's score "
                         "order, every draw whose end point lies within RADIUS (world units) of a kept one")
    ap.add_argument("--compose", type=float, default=None, metavar="DIST",
                    help="also report the composed scene futures: one draw per agent, the discriminator's top-scored ones moved to "
                         "other draws until no two chosen paths come closer than DIST (world units)")
    ap.add_argument("--risk", type=float, default=None, metavar="DIST",
                    help="also report the collision risk of every held-out agent's true future against the K draws of the others "
                         "(closer than DIST, world units) and how well it is calibrated")
    ap.add_argument("--refine", type=float, default=None, metavar="DIST",
                    help="also refine every held-out agent's constant-velocity plan against the K draws of the others (clearance "
                         "penalty at DIST, world units) and report predicted risk and true collisions before and after")
    ap.add_argument("--walls", default=None, metavar="FILE[:DIST]", action="append",
                    help="the static map of the recording: a text file of `x0 y0 x1 y1` lines in world coordinates (# comments); "
                         "also report how many of the K draws come within DIST (default 0.1, world units) of a wall "
                         "(evaluate_walls); with --refine the refinement keeps the plans off the walls too; with several "
                         "--obsmat: one per recording, in their order")
    ap.add_argument("--map-image", default=None, metavar="FILE[:HFILE]",
                    help="the map from an obstacle image (.npy, or what PIL reads) and its homography file (3 x 3, on (row, col, 1) "
                         "as ETH's H.txt; none: pixels are world units): traced and put under a grid; takes the place of --walls")
    ap.add_argument("--map-reach", type=float, default=1.0, metavar="D",
                    help="with --map-image: the largest distance (world units) a wall call may ask about")
    ap.add_argument("--min-past", type=int, default=None, metavar="M",
                    help="also evaluate on held-out windows that keep the pedestrians seen for only M .. 7 frames (ragged "
                         "histories) and report the errors per history length; training stays on full windows unless "
                         "--train-ragged is given")
    ap.add_argument("--min-next", type=int, default=None, metavar="M",
                    help="also evaluate on held-out windows that keep the pedestrians whose track ends M .. 11 frames after t "
                         "(ragged futures) and report the errors per future length; combines with --min-past; training windows "
                         "are always full")
    ap.add_argument("--train-ragged", action="store_true",
                    help="with --min-past M: train on the ragged windows in front of the held-out part (train_epoch_ragged: "
                         "eager steps on the unfused route) instead of the full windows only")
    ap.add_argument("--ragged-fused", action="store_true",
                    help="with --train-ragged: the fused ragged step (ragged_fused=True: one-launch D updates, graph-captured steps)")
    ap.add_argument("--clearance-loss", default=None, metavar="DIST[:W]",
                    help="add the scene-clearance term to the generator loss: futures of one scene closer than DIST (world "
                         "units) are penalised with weight W (default 1); reports the collision rates at DIST")
    ap.add_argument("--wall-loss", default=None, metavar="DIST[:W]",
                    help="with --walls FILE: add the wall term to the generator loss: predicted segments closer than DIST (world "
                         "units) to a wall of the map are penalised with weight W (default 1)")
    args = ap.parse_args(argv)
    wall_loss = None
    if args.wall_loss is not None:
        try:
            dist, _, w = args.wall_loss.partition(":")
            wall_loss = (float(dist), float(w) if w else 1.0)
        except ValueError:
            ap.error("--wall-loss takes DIST or DIST:W, got %r" % args.wall_loss)
        if args.walls is None and args.map_image is None:
            ap.error("--wall-loss needs --walls FILE or --map-image FILE: the map to train against")
        if args.hidden_size != 64:
            ap.error("--wall-loss: the wall term is implemented for the fused 64-unit path (--hidden-size 64)")
    clearance = None
    if args.clearance_loss is not None:
        try:
            dist, _, w = args.clearance_loss.partition(":")
            clearance = (float(dist), float(w) if w else 1.0)
        except ValueError:
            ap.error("--clearance-loss takes DIST or DIST:W, got %r" % args.clearance_loss)
        if args.hidden_size != 64:
            ap.error("--clearance-loss: the clearance term is implemented for the fused 64-unit path (--hidden-size 64)")
    wall_files, wall_dist = [], 0.1
    for entry in args.walls or []:
        head, sep, tail = entry.rpartition(":")
        try:
            if sep and head:
                entry, wall_dist = head, float(tail)
        except ValueError:               # a colon that belongs to the file name
            pass
        wall_files.append(entry)
    obsmats = args.obsmat or [None]
    many = len(obsmats) > 1
    if wall_files and len(wall_files) != len(obsmats):
        ap.error("--walls is given once per --obsmat, in the same order: %d maps for %d recordings" % (len(wall_files), len(obsmats)))
    if many and (args.min_past is not None or args.min_next is not None or args.train_ragged or args.refine is not None
                 or wall_loss is not None):
        ap.error("several --obsmat: --min-past, --min-next, --train-ragged, --refine and --wall-loss take one recording")
    wall_file = wall_files[0] if wall_files else None
    if args.map_image is not None and (wall_files or many):
        ap.error("--map-image takes the place of --walls and one recording")
    if args.ragged_fused and not args.train_ragged:
        ap.error("--ragged-fused needs --train-ragged")
    if args.train_ragged and args.min_past is None:
        ap.error("--train-ragged needs --min-past M")
    if args.min_next is not None and args.hidden_size != 64:
        ap.error("--min-next: ragged futures are implemented for the fused 64-unit path (--hidden-size 64)")
    if args.train_ragged and args.hidden_size != 64:
        ap.error("--train-ragged: ragged histories are implemented for the fused 64-unit path (--hidden-size 64)")

    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    pg = None
    if world > 1:                                                    # launched by torch.distributed.run: one rank per GPU
        torch.cuda.set_device(dev)
        torch.distributed.init_process_group("nccl", device_id=dev)
        pg = torch.distributed.group.WORLD
    os.makedirs(args.out, exist_ok=True)
    obsmat = obsmats[0]
    if obsmat is None:
        obsmat = os.path.join(args.out, "obsmat.txt")
        if rank == 0:
            fr, ids, pos, vel = sw.synth_crowd_frames(n_frames=400, n_ped=160, interval=6, seed=args.seed + 3)
            sw.write_biwi_obsmat(obsmat, fr, ids, pos, vel)
    npz = os.path.join(args.out, "crowd-8-12.npz")
    npzs = [npz] + [os.path.join(args.out, "crowd-8-12-%d.npz" % i) for i in range(1, len(obsmats))]
    if rank == 0:
        for o, f in zip([obsmat] + obsmats[1:], npzs):
            obsvs, preds, times, batches = sw.biwi_to_npz(o, f, 8, 12)
            print("%s: %d samples in %d scenes (largest %d agents)" % (o, len(obsvs), len(batches),
                                                                        int(np.max(batches[:, 1] - batches[:, 0]))))
    if world > 1:
        torch.distributed.barrier()
    ragged_npz = os.path.join(args.out, "crowd-8-12-ragged.npz")
    if args.min_past is not None and rank == 0:
        sw.biwi_to_npz(obsmat, ragged_npz, 8, 12, min_past=args.min_past)
    next_npz = os.path.join(args.out, "crowd-8-12-next.npz")
    if args.min_next is not None and rank == 0:      # evaluation windows only: min_past 8 (full histories) unless --min-past
        sw.biwi_to_npz_ragged(obsmat, next_npz, 8, 12, min_past=args.min_past if args.min_past is not None else 8,
                              min_next=args.min_next)
    if world > 1:
        torch.distributed.barrier()
    if many:
        parts = [np.load(f) for f in npzs]
        data = sw.SceneDataset.from_recordings([(d["obsvs"], d["preds"], d["batches"], d["times"]) for d in parts], device=dev)
    else:
        data = sw.SceneDataset.from_npz(npz, device=dev)
    ragged = train_set = short = None
    if args.min_next is not None and rank == 0:
        short = ragged_windows(next_npz, data, train=False)
        print("ragged-future held-out set: %d windows in %d scenes, %d of them with fewer than %d future frames"
              % (short.n_test_samples, len(short.test_batches), int((short.pred_len < data.n_next).sum()), data.n_next))
    if args.min_past is not None and rank == 0:
        ragged = ragged_windows(ragged_npz, data, train=False)
        print("ragged held-out set: %d windows in %d scenes, %d of them with fewer than %d frames"
              % (ragged.n_test_samples, len(ragged.test_batches), int((ragged.obs_len < data.n_past).sum()), data.n_past))
    if args.train_ragged:                 # every rank: the packed batches are sharded scene-aligned as in train_epoch()
        train_set = ragged_windows(ragged_npz, data, train=True)
        if rank == 0:
            print("ragged training set: %d windows in %d scenes, %d of them with fewer than %d frames (full windows: %d)"
                  % (train_set.n_train_samples, len(train_set.train_batches), int((train_set.obs_len < data.n_past).sum()),
                     data.n_past, data.n_train_samples))
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    walls = data.walls_from_world(sw.load_walls(wall_file)) if wall_file is not None else None
    if args.map_image is not None:        # image -> boundary runs -> world coordinates -> a grid over them
        image, sep, hfile = args.map_image.rpartition(":")
        if not sep or not image or not os.path.exists(hfile):      # no homography file: the whole argument is the image
            image, hfile = args.map_image, None
        to_world = None
        if hfile is not None:
            to_world = np.loadtxt(hfile).reshape(3, 3)[:, [1, 0, 2]]       # H acts on (row, col, 1), the tracer gives (x = col, y = row, 1)
        runs = sw.trace_occupancy(sw.load_occupancy(image), to_world)
        walls = data.wall_grid_from_world(runs, args.map_reach)
        if rank == 0:
            print("Map image %s: %d boundary runs under a grid of %d x %d cells (cell %.3f, reach %.3f world units)"
                  % (image, walls.M, walls.nx, walls.ny, walls.cell / data.ss, args.map_reach))
    n_walls = 0 if walls is None else walls.M if isinstance(walls, sw.WallGrid) else walls.shape[0]
    flat_walls = None if isinstance(walls, sw.WallGrid) else walls           # what the refinement takes
    maps = None
    if many and wall_files:               # one map per recording: its held-out scenes are judged against its own
        walls, maps = None, data.maps_from_world([sw.load_walls(f) for f in wall_files])
    tr = sw.SocialWaysTrainer(data.n_next, hidden_size=args.hidden_size, use_social=bool(args.social), device=dev,
                              process_group=pg, **(dict(ragged_fused=True) if args.ragged_fused else {}))
    if args.device_noise is not None:     # the same seed on every rank: the union of the shards is the single-process z
        tr.noise = sw.DeviceNoise(args.device_noise)
    if clearance is not None:
        tr.set_clearance_loss(*clearance)
    if wall_loss is not None:
        tr.set_wall_loss(walls, *wall_loss)
        if rank == 0:
            print("Wall loss: %d walls, dist %.2f, weight %.2f" % (n_walls, wall_loss[0], wall_loss[1]))
    for epoch in range(1, args.epochs + 1):
        t0 = time.perf_counter()
        if train_set is not None:
            ade, fde, losses, sizes = tr.train_epoch_ragged(train_set, args.batch_size)
        else:
            ade, fde, losses, sizes = tr.train_epoch(data, args.batch_size)
        if rank == 0:
            print("Epc=%4d, Train ADE,FDE = (%.3f, %.3f) | time = %.2f | %d packed batches | D/G losses %.4f %.4f"
                  % (epoch, ade, fde, time.perf_counter() - t0, len(sizes), losses[:, 0].mean() + losses[:, 2].mean(),
                     losses[:, -2].mean()))
        if rank == 0 and (epoch % args.test_every == 0 or epoch == args.epochs):
            run_test = tr.test if tr.noise is None else tr.evaluate      # evaluate(): test()'s contract, z from tr.noise
            m = run_test(data, n_gen_samples=args.k, write_to_file=os.path.join(args.out, "preds", str(epoch)))
            print("Avg ADE,FDE = (%.3f, %.3f) | Min(%d) ADE,FDE = (%.3f, %.3f)" % (m[0], m[1], args.k, m[2], m[3]))
            sm = tr.evaluate_scenes(data, n_gen_samples=args.k)      # the K draws as JOINT futures of each scene
            print("Scene level: joint Min(%d) ADE,FDE = (%.3f, %.3f) | collisions < 0.1: %.1f %% of draws, %.1f %% of best draws, "
                  "%.1f %% of agents (ground truth %.1f %%) | %d scenes, %d with company"
                  % (args.k, sm["jade_min"], sm["jfde_min"], 100 * sm["col_joint"], 100 * sm["col_best"], 100 * sm["col_agent"],
                     100 * sm["col_gt"], sm["n_scenes"], sm["n_multi"]))
            if clearance is not None:
                sc = tr.evaluate_scenes(data, n_gen_samples=args.k, coll_dist=clearance[0])
                print("Clearance loss (dist %.2f, weight %.2f): Min(%d) ADE,FDE = (%.3f, %.3f) | collisions < %.2f: col_joint %.1f %%, "
                      "col_agent %.1f %% (ground truth %.1f %%)"
                      % (clearance[0], clearance[1], args.k, sc["ade_min"], sc["fde_min"], clearance[0], 100 * sc["col_joint"],
                         100 * sc["col_agent"], 100 * sc["col_gt"]))
            if args.diverse is not None:
                dv = tr.evaluate_diverse(data, n_gen_samples=args.k, top_m=min(5, args.k), radius=args.diverse)
                print("Diverse top-%d (radius %.2f): ADE,FDE first = (%.3f, %.3f), best mode = (%.3f, %.3f) | %.2f modes per agent, "
                      "first mode holds %.0f %% of the draws, the min-ADE mode %.0f %%"
                      % (dv["top_m"], args.diverse, dv["ade_div1"], dv["fde_div1"], dv["ade_divm"], dv["fde_divm"], dv["n_modes"],
                         100 * dv["w_first"], 100 * dv["w_hit"]))
            if args.compose is not None:
                cp = tr.evaluate_composed(data, n_gen_samples=args.k, coll_dist=args.compose)
                print("Composed futures (one of %d draws per agent, no two paths within %.2f): ADE,FDE top-scored = (%.3f, %.3f), "
                      "composed = (%.3f, %.3f) | scenes with a collision %.1f %% -> %.1f %%, pairs per scene %.2f -> %.2f, %.1f %% of "
                      "agents moved, mean score %.3f -> %.3f | %d scenes, %d with company"
                      % (args.k, args.compose, cp["ade_top1"], cp["fde_top1"], cp["ade_comp"], cp["fde_comp"], 100 * cp["col_top1"],
                         100 * cp["col_comp"], cp["pairs_top1"], cp["pairs_comp"], 100 * cp["moved"], cp["score_top1"],
                         cp["score_comp"], cp["n_scenes"], cp["n_multi"]))
            if args.risk is not None:
                rk = tr.evaluate_risk(data, n_gen_samples=args.k, coll_dist=args.risk)
                print("Plan risk (leave-one-out, %d draws, within %.2f): mean risk %.3f, %.1f %% of the agents do collide | Brier %.4f "
                      "(index-paired %.4f, base rate %.4f) | mean risk of those who collide %.3f, of the others %.3f | first conflict "
                      "off by %.2f frames | %d agents with company"
                      % (args.k, args.risk, rk["risk_mean"], 100 * rk["col_gt_agent"], rk["brier"], rk["brier_diag"], rk["brier_base"],
                         rk["risk_hit"], rk["risk_miss"], rk["t_first_err"], rk["n_ego"]))
            if args.refine is not None:
                rf = tr.evaluate_refine(data, n_gen_samples=args.k, dist=args.refine, walls=flat_walls)
                print("Plan refinement (leave-one-out, %d draws, penalty within %.2f, conflict within %.2f): predicted risk %.3f -> %.3f | "
                      "collisions with the true futures %.1f %% -> %.1f %% | expected penalty %.3f -> %.3f | mean largest move %.3f | "
                      "%d agents with company"
                      % (args.k, args.refine, rf["coll_dist"], rf["risk_cv"], rf["risk_ref"], 100 * rf["col_cv"], 100 * rf["col_ref"],
                         rf["pen_cv"], rf["pen_ref"], rf["moved"], rf["n_ego"]))
                if flat_walls is not None:
                    print("  with %d walls: plans within %.2f of a wall %.1f %% -> %.1f %% | wall penalty %.3f -> %.3f"
                          % (n_walls, rf["coll_dist"], 100 * rf["wall_cv"], 100 * rf["wall_ref"], rf["penw_cv"], rf["penw_ref"]))
            if walls is not None:
                wl = tr.evaluate_walls(data, walls, n_gen_samples=args.k, wall_dist=wall_dist)
                print("Walls (%d segments, within %.2f): %.1f %% of the draws, %.1f %% of the agents in some draw, %.1f %% in every draw "
                      "(ground truth %.1f %%) | Min(%d) ADE,FDE over the clear draws = (%.3f, %.3f) | first conflict at frame %.2f"
                      % (n_walls, wall_dist, 100 * wl["wall_draws"], 100 * wl["wall_agents"], 100 * wl["wall_blocked"],
                         100 * wl["wall_gt"], args.k, wl["ade_min_free"], wl["fde_min_free"], wl["t_first"]))
            for i in range(len(maps) if maps is not None else 0):
                part = data.test_part(i)
                if not part.n_test_samples:       # a recording too short to hold a scene out
                    continue
                wl = tr.evaluate_walls(part, maps[i], n_gen_samples=args.k, wall_dist=wall_dist)
                print("Walls of recording %d (%d segments, within %.2f, %d held-out agents): %.1f %% of the draws, %.1f %% of the agents "
                      "in some draw, %.1f %% in every draw (ground truth %.1f %%)"
                      % (i, maps[i].shape[0], wall_dist, wl["n_agents"], 100 * wl["wall_draws"], 100 * wl["wall_agents"],
                         100 * wl["wall_blocked"], 100 * wl["wall_gt"]))
            if ragged is not None:
                hist = tr.evaluate_history(ragged, n_gen_samples=args.k)
                print("Ragged held-out set: Avg ADE,FDE = (%.3f, %.3f) | Min(%d) ADE,FDE = (%.3f, %.3f) | by history length: %s"
                      % (hist["ade_avg"], hist["fde_avg"], args.k, hist["ade_min"], hist["fde_min"],
                         ", ".join("%d frames (%d agents) %.3f / %.3f" % (n, v["count"], v["ade_min"], v["fde_min"])
                                   for n, v in sorted(hist["by_len"].items()))))
            if short is not None:
                hz = tr.evaluate_horizon(short, n_gen_samples=args.k)
                print("Ragged-future held-out set: Avg ADE,FDE = (%.3f, %.3f) | Min(%d) ADE,FDE = (%.3f, %.3f) | by future length: %s"
                      % (hz["ade_avg"], hz["fde_avg"], args.k, hz["ade_min"], hz["fde_min"],
                         ", ".join("%d frames (%d agents) %.3f / %.3f" % (n, v["count"], v["ade_min"], v["fde_min"])
                                   for n, v in sorted(hz["by_next"].items()))))
            tr.save(os.path.join(args.out, "socialWays-crowd.pt"), epoch=epoch)
    if world > 1:
        tr.close()              # captured collectives and the direct exchange's buffers go before their process group
        torch.distributed.destroy_process_group()
    return tr


if __name__ == "__main__":
    main()
