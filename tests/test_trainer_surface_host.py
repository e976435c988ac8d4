"""The surface of the three trainers (no GPU): every public callable with its signature, every public class constant with
its value, and the underscore names that generic.py, wide.py, tools/ and tests/ reach on a trainer.  The table is compared
as a whole, so a method lost or renamed when code moves between classes or modules (trainer.py holds the training step and
the whole evaluation and planning family), or one whose parameters or defaults changed, fails here, and so does a public
name that appears without an entry."""
import inspect

FUSED = {
    "callables": {
        'checkpoint': '(self, epoch=None)',
        'close': '(self)',
        'eval_chunks': '(batches, K, chunk)',
        'eval_noise': '(batches, K, noise_len)',
        'evaluate': '(self, data, n_gen_samples=20, write_to_file=None, just_one=False, collect=None, noise=None)',
        'evaluate_composed': '(self, data, n_gen_samples=20, coll_dist=0.1, sweeps=8, just_one=False, collect=None, noise=None)',
        'evaluate_diverse': "(self, data, n_gen_samples=20, top_m=5, radius=0.5, metric='fde', joint=False, just_one=False, "
                            "collect=None, noise=None)",
        'evaluate_history': '(self, data, n_gen_samples=20, just_one=False, noise=None)',
        'evaluate_horizon': '(self, data, n_gen_samples=20, just_one=False, noise=None)',
        'evaluate_ranked': '(self, data, n_gen_samples=20, top_m=5, just_one=False, collect=None, noise=None)',
        'evaluate_refine': '(self, data, n_gen_samples=20, dist=0.5, coll_dist=0.1, just_one=False, collect=None, noise=None, '
                           'walls=None, wall_dist=None, w_wall=1.0, **descent)',
        'evaluate_risk': '(self, data, n_gen_samples=20, coll_dist=0.1, just_one=False, collect=None, noise=None)',
        'evaluate_scenes': '(self, data, n_gen_samples=20, coll_dist=0.1, just_one=False, collect=None)',
        'evaluate_walls': '(self, data, walls, n_gen_samples=20, wall_dist=0.1, just_one=False, collect=None, noise=None)',
        'load_checkpoint': '(self, ck)',
        'losses_from': '(self, out, B_global, Tp=None, ss=1.0)',
        'plan_risk': '(self, obsv_p, plans, n_samples, coll_dist, sub_batches=[], scene=None, ego=None, plan_start=None, '
                     'noise=None, row0=0, scale=1.0, obs_len=None)',
        'refine_plans': '(self, obsv_p, plans, n_samples, dist, coll_dist=None, sub_batches=[], scene=None, ego=None, '
                        'plan_start=None, noise=None, row0=0, scale=1.0, obs_len=None, walls=None, wall_dist=None, w_wall=1.0, '
                        '**descent)',
        'release_graphs': '(self)',
        'sample_composed': '(self, obsv_p, n_samples, coll_dist, sub_batches=[], noise=None, row0=0, scale=1.0, sweeps=8, '
                           'obs_len=None)',
        'sample_diverse': "(self, obsv_p, n_samples, top_m, radius, metric='fde', joint=False, sub_batches=[], noise=None, row0=0, "
                          "scale=1.0, obs_len=None)",
        'sample_ranked': '(self, obsv_p, n_samples, top_m, sub_batches=[], noise=None, row0=0, obs_len=None)',
        'save': '(self, path, epoch=None)',
        'set_clearance_loss': '(self, dist, weight=1.0)',
        'set_wall_loss': '(self, walls, dist=None, weight=1.0)',
        'step': '(self, obsv, pred, sub_batches, zeros_val, ones_val, noise, ss=1.0, global_B=None, out=None, global_row0=0, '
                'variety_noise=None, obs_len=None)',
        'step_many': '(self, batches, sub_batches, ss=1.0, global_B=None, out=None, global_row0=0, **ragged)',
        'sync_replicas': '(self)',
        'sync_rng': '(self)',
        'test': '(self, data, n_gen_samples=20, linear=False, write_to_file=None, just_one=False, collect=None)',
        'train_epoch': '(self, data, batch_size, draw=None)',
        'train_epoch_ragged': '(self, data, batch_size, draw=None)',
    },
    "constants": {
        'COMPOSED_KEYS': ('ade_top1', 'fde_top1', 'ade_comp', 'fde_comp', 'score_top1', 'score_comp', 'moved', 'col_top1', 'col_comp',
                          'pairs_top1', 'pairs_comp'),
        'DIVERSE_KEYS': ('ade_div1', 'fde_div1', 'ade_divm', 'fde_divm', 'rank_hit', 'w_hit', 'n_modes', 'w_first'),
        'RANKED_KEYS': ('ade_top1', 'fde_top1', 'ade_topm', 'fde_topm', 'best_rank', 'score_draws', 'score_gt', 'code_mse'),
        'REFINE_KEYS': ('risk_cv', 'risk_ref', 'col_cv', 'col_ref', 'pen_cv', 'pen_ref', 'moved'),
        'REFINE_WALL_KEYS': ('wall_cv', 'wall_ref', 'penw_cv', 'penw_ref'),
        'RISK_KEYS': ('risk_mean', 'col_gt_agent', 'brier', 'brier_diag', 'risk_hit', 'risk_miss', 't_first_err'),
        'STEPS_PER_LAUNCH': 4,
        'TEST_CHUNK': 16384,
        'WALL_KEYS': ('wall_draws', 'wall_agents', 'wall_blocked', 'wall_gt', 'ade_min_free', 'fde_min_free', 't_first'),
        'Z_COLS': 32,
    },
    "private": {
        '_allreduce': '(self, flat)',
        '_check_compose': '(coll_dist, sweeps)',
        '_device_noise': '(self, noise)',
        '_empty_step': '(self)',
        '_eval_draws': '(self, data, K, just_one, dn, base, want_pred=True)',
        '_eval_emit': '(self, rec, collect, write_to_file=None)',
        '_eval_fold': '(self, data, K, just_one)',
        '_eval_records': '(self, data, c, preds_k, extra={})',
        '_gather_picks': '(values, idx, fill)',
        '_graph_key': '(self, scenes, To, ss, Bg, K, zdev=False, ragged=False)',
        '_pad_z': '(self, z)',
        '_sample_draws': '(self, c, K, ss, want_pred)',
        '_step_impl': '(self, obsv, pred, pred4, scenes, targets, noise, ss, Bg, out, steps=None)',
        '_z_resident': '(self, batches)',
    },
}

# the generic-width path: the fused trainer's surface, dense steps only
GENERIC = {
    "callables": dict(
        FUSED["callables"],
        step='(self, obsv, pred, sub_batches, zeros_val, ones_val, noise, ss=1.0, global_B=None, out=None, global_row0=0, '
             'variety_noise=None)',
        step_many='(self, batches, sub_batches, ss=1.0, global_B=None, out=None, global_row0=0)'),
    "constants": FUSED["constants"],
    "private": dict(FUSED["private"], _reduce_grads='(self, optim)'),
}

# the wide path: the generic one's, plus its own step machinery
WIDE = {
    "callables": dict(GENERIC["callables"],
                      supports='(hidden_size, n_latent_codes=2, use_variety_loss=False, process_group=None)'),
    "constants": dict(FUSED["constants"], MAX_GRAPHS=96, MAX_WORKSPACES=64, WORKSPACE_BYTES=25769803776),
    "private": dict(
        GENERIC["private"],
        _buffers='(self, B, To, P)',
        _capture='(self, key, w, sc, B, To, ss, Bg)',
        _disc_backward='(self, w, B, To)',
        _disc_forward='(self, w, B, To, nb, loss=None)',
        _disc_heads_backward='(self, w, B, nb, want_dpred, need_obs=False)',
        _gen_backward='(self, w, sc, B, To, dpred4)',
        _gen_forward='(self, w, sc, B, To)',
        _heads_args='(self, w, B, To, nb, backward, need_obs, want_dpred, loss=None)',
        _image_table='(self, fl, entries)',
        _images='(self, args)',
        _lstm_step_bwd='(self, t, T, B, whhT, gates, cs, dg, dc, dh_ext, dhe_ld, dh_ext2=None, dhe2_ld=0)',
        _lstm_step_fwd='(self, t, B, x4, hs, cs, gates, Wx, b1, b2, whh, h2=None, h2_ld=0)',
        _replay='(self, g)',
        _sq='(self, a, lda, b, ldb, targets, t_idx, R, C, gscale, out, da, ldda)',
        _step_device='(self, w, sc, B, To, ss, Bg)',
        _transpose_table='(self, fl, mats)',
        _transposes='(self, args)',
        _wgrad='(self, w, problems)'),
}


def surface(cls, private):
    """The table of one class: public callables and constants as found, the underscore names asked for."""
    calls, consts = {}, {}
    for name in dir(cls):
        if name.startswith("_"):
            continue
        value = getattr(cls, name)
        if callable(value):
            calls[name] = str(inspect.signature(value))
        elif name.isupper():
            consts[name] = value
    return {"callables": calls, "constants": consts, "private": {name: str(inspect.signature(getattr(cls, name))) for name in private}}


def test_the_trainers_keep_their_surface():
    from socialways_amd.generic import GenericTrainer
    from socialways_amd.trainer import SocialWaysTrainer
    from socialways_amd.wide import WideTrainer
    for cls, table in ((SocialWaysTrainer, FUSED), (GenericTrainer, GENERIC), (WideTrainer, WIDE)):
        found = surface(cls, table["private"])
        for part in ("callables", "constants", "private"):
            assert found[part] == table[part], (cls.__name__, part, set(found[part].items()) ^ set(table[part].items()))


def test_names_imported_from_the_trainer_module_resolve():
    """What generic.py, wide.py, tests/ and tools/ (nms_timing.py: sw.trainer._EvalSums) import from socialways_amd.trainer."""
    import socialways_amd as sw
    from socialways_amd import trainer
    from socialways_amd.trainer import _PRED_LEN_TRAIN, PackedAdam, SocialWaysTrainer, _EvalSums, _refuse_pred_len
    assert sw.SocialWaysTrainer is SocialWaysTrainer and sw.trainer is trainer
    assert isinstance(_PRED_LEN_TRAIN, str) and callable(_refuse_pred_len)
    assert inspect.isclass(PackedAdam) and inspect.isclass(_EvalSums) and _EvalSums.KEYS == ("ade_avg", "fde_avg", "ade_min", "fde_min")
