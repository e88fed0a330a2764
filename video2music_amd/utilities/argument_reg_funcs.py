"""``parse_eval_args`` of the regression head: the flag names and defaults of the reference's
``utilities/argument_reg_funcs.py:125-179``, plus the input switches ``argument_eval_funcs.py`` adds (the reference tree ships
neither weights nor dataset features)."""
import argparse

from .argument_eval_funcs import MUSIC_TYPE, VIS_MODELS_SORTED
from .constants import IS_VIDEO

# module defaults of utilities/argument_reg_funcs.py:7-17
regModel = "bilstm"
augmentation = False
d_model = 64
d_ff = 256
n_layers = 2
motion_type = 0
scene_embed = False


def parse_eval_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("-dataset_dir", type=str, default="./dataset/", help="Folder of VEVO dataset")
    parser.add_argument("-input_dir_music", type=str, default="./dataset/vevo_chord/" + MUSIC_TYPE, help="Kept for flag compatibility")
    parser.add_argument("-input_dir_video", type=str, default="./dataset/vevo_vis", help="Kept for flag compatibility")
    parser.add_argument("-model_weights", type=str, default="./saved_models/AMT/best_rmse_weights.pickle",
                        help="state_dict saved with torch.save (reference key names)")
    parser.add_argument("-n_workers", type=int, default=4, help="Kept for flag compatibility; the feature files are read in-process")
    parser.add_argument("--force_cpu", type=bool, default=False, help="Kept for flag compatibility; this build has no CPU path")
    parser.add_argument("-batch_size", type=int, default=1, help="Clips per get_feature / metrics call; the figures do not depend on it")
    parser.add_argument("-max_sequence_midi", type=int, default=2048)
    parser.add_argument("-max_sequence_video", type=int, default=300)
    parser.add_argument("-max_sequence_chord", type=int, default=300)
    parser.add_argument("-n_layers", type=int, default=n_layers)
    parser.add_argument("-d_model", type=int, default=d_model)
    parser.add_argument("-dim_feedforward", type=int, default=d_ff)
    parser.add_argument("-use_KAN", type=bool, default=False, help="Kept for flag compatibility; not built")
    parser.add_argument("-regModel", type=str, default=regModel,
                        help="lstm, bilstm, gru, bigru, cnngru, cnnbigru, mamba, mamba+, bimamba, bimamba+, moemamba, moe_bimamba+, "
                             "sharedmoe_bimamba+")
    parser.add_argument("-is_video", type=bool, default=IS_VIDEO)
    parser.add_argument("-vis_models", type=str, default=VIS_MODELS_SORTED)
    parser.add_argument("-emo_model", type=str, default="6c_l14p")
    parser.add_argument("-augmentation", type=bool, default=augmentation, help="Kept for flag compatibility; not built")
    parser.add_argument("-motion_type", type=int, default=motion_type, help="0 as original, 1 as option 1, 2 as option 2")
    parser.add_argument("-scene_embed", type=bool, default=scene_embed)
    # additions of this build
    parser.add_argument("-output_dir", type=str, default="./log", help="Folder for metrics.json")
    parser.add_argument("--test_ids", type=str, default="split:test",
                        help="clip ids to read from -dataset_dir, comma separated, or split:<name> for vevo_meta/split/v1/<name>.txt")
    parser.add_argument("--synthetic_weights", action="store_true", help="random-init procedural weights with real feature files")
    return parser.parse_known_args(argv)


# module defaults of utilities/argument_reg_funcs.py:9-18 that only training uses
batch_size = 32
epochs = 50
dropout = 0.2
lr = None
optimizer = "Adam"          # Adam / AdamW (RAdam / RAdamW are refused)


def parse_train_args(argv=None):
    """The flag names and defaults of the reference's ``parse_train_args`` (``utilities/argument_reg_funcs.py:20-77``), plus the
    switches this build adds."""
    parser = argparse.ArgumentParser()
    parser.add_argument("-dataset_dir", type=str, default="./dataset/", help="Folder of VEVO dataset")
    parser.add_argument("-input_dir_music", type=str, default="./dataset/vevo_chord/" + MUSIC_TYPE, help="Kept for flag compatibility")
    parser.add_argument("-input_dir_video", type=str, default="./dataset/vevo_vis", help="Kept for flag compatibility")
    parser.add_argument("-output_dir", type=str, default="./saved_models", help="Folder to save model weights")
    parser.add_argument("-weight_modulus", type=int, default=10, help="How often to save epoch weights (10 = every 10 epochs)")
    parser.add_argument("-print_modulus", type=int, default=100, help="How often to print a batch's loss and learn rate")
    parser.add_argument("-n_workers", type=int, default=4, help="Kept for flag compatibility; the feature files are read in-process")
    parser.add_argument("--force_cpu", type=bool, default=False, help="Kept for flag compatibility; this build has no CPU path")
    parser.add_argument("--no_tensorboard", type=bool, default=True, help="Kept for flag compatibility; tensorboard reporting is not built")
    parser.add_argument("-continue_weights", type=str, default=None, help="Model weights to continue training from")
    parser.add_argument("-continue_epoch", type=int, default=None, help="Epoch the continue_weights model was at")
    parser.add_argument("-lr", type=float, default=lr, help="Constant learn rate. Leave as None for the warm-up schedule")
    parser.add_argument("-batch_size", type=int, default=batch_size)
    parser.add_argument("-epochs", type=int, default=epochs)
    parser.add_argument("-max_sequence_midi", type=int, default=2048)
    parser.add_argument("-max_sequence_video", type=int, default=300)
    parser.add_argument("-max_sequence_chord", type=int, default=300)
    parser.add_argument("-n_layers", type=int, default=n_layers)
    parser.add_argument("-d_model", type=int, default=d_model)
    parser.add_argument("-dim_feedforward", type=int, default=d_ff)
    parser.add_argument("-dropout", type=float, default=dropout)
    parser.add_argument("-use_KAN", type=bool, default=False, help="Kept for flag compatibility; not built")
    parser.add_argument("-is_video", type=bool, default=IS_VIDEO)
    parser.add_argument("-regModel", type=str, default=regModel, help="lstm, bilstm, gru, bigru (the regModels whose backward is built)")
    parser.add_argument("-vis_models", type=str, default=VIS_MODELS_SORTED)
    parser.add_argument("-emo_model", type=str, default="6c_l14p")
    parser.add_argument("-augmentation", type=bool, default=augmentation, help="Kept for flag compatibility; not built")
    parser.add_argument("-motion_type", type=int, default=motion_type, help="0 as original, 1 as option 1, 2 as option 2")
    parser.add_argument("-scene_embed", type=bool, default=scene_embed)
    parser.add_argument("-optimizer", type=str, default=optimizer, help="Adam or AdamW")
    # additions of this build
    parser.add_argument("--seed", type=int, default=0, help="seeds the initial weights, the per-epoch clip order and the dropout masks")
    parser.add_argument("--train_ids", type=str, default="split:train",
                        help="clip ids to read from -dataset_dir, comma separated, or split:<name> for vevo_meta/split/v1/<name>.txt")
    parser.add_argument("--val_ids", type=str, default="split:val", help="as --train_ids, for the validation figures")
    return parser.parse_known_args(argv)
