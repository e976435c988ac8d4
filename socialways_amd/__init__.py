"""socialways_amd - the Social Ways GAN training inner loop (crowdbotp/socialways train.py) as
hand-written HIP for MI355X (gfx950) behind the reference's own Python surface.

    from socialways_amd import Generator, Discriminator, predict, get_traj_4d, SocialWaysTrainer
"""
from .model import (AttentionPooling, DecoderFC, Discriminator, EmbedSocialFeatures, EncoderLstm, Generator,  # noqa: F401
                    SocialFeatures, get_traj_4d, predict, predict_cv, sample, set_default_generator)
from ._lib import SocialWaysHipError, load as load_library  # noqa: F401
from .noise import DeviceNoise  # noqa: F401
from .trainer import SocialWaysTrainer  # noqa: F401
from .data import (SceneDataset, Scale, synth_tracks, toy_tracks, shard_scenes, ragged_scene_sizes,  # noqa: F401
                   parse_biwi, create_dataset, create_dataset_ragged, biwi_to_npz, biwi_to_npz_ragged, write_biwi_obsmat,
                   synth_crowd_frames, check_pred_len, load_walls, WallMaps, WallGrid, trace_occupancy, load_occupancy)
from . import stats  # noqa: F401

__all__ = ["AttentionPooling", "DecoderFC", "Discriminator", "EmbedSocialFeatures", "EncoderLstm", "Generator",
           "SocialFeatures", "get_traj_4d", "predict", "predict_cv", "sample", "set_default_generator", "SocialWaysHipError",
           "load_library", "DeviceNoise", "SocialWaysTrainer", "SceneDataset", "Scale", "synth_tracks", "toy_tracks", "shard_scenes", "ragged_scene_sizes", "stats",
           "parse_biwi", "create_dataset", "create_dataset_ragged", "biwi_to_npz", "biwi_to_npz_ragged", "write_biwi_obsmat", "synth_crowd_frames",
           "check_pred_len", "load_walls", "WallMaps", "WallGrid", "trace_occupancy", "load_occupancy"]
