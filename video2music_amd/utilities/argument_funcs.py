"""``parse_train_args`` of the chord model: the flag names, types and defaults of the reference's
``utilities/argument_funcs.py:4-75``, plus the switches this build adds (the reference tree ships neither weights nor dataset
features).  The reference's ``type=bool`` flags are kept as they are: any non-empty value reads as True."""
import argparse

from .argument_eval_funcs import MUSIC_TYPE, VIS_MODELS_SORTED
from .constants import IS_VIDEO

# module defaults of utilities/argument_funcs.py:4-20
rpr = True
augmentation = False
chord_embed = True
music_gen_version = "1.2.3"
batch_size = 32
epochs = 50
motion_type = 2
dropout = 0.2
droptoken = 0.0
lr = None
optimizer = "AdamW"         # Adam / AdamW (the others are refused)
auxiliary_loss = False
drop_loss = False
balancing = False

ADDED = ("seed", "train_ids", "val_ids", "synthetic_weights", "chord_embed_table")      # flags the reference does not have


def parse_train_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("-dataset_dir", type=str, default="./dataset/", help="Folder of VEVO dataset")
    parser.add_argument("-input_dir_music", type=str, default="./dataset/vevo_chord/" + MUSIC_TYPE, help="Kept for flag compatibility")
    parser.add_argument("-input_dir_video", type=str, default="./dataset/vevo_vis", help="Kept for flag compatibility")
    parser.add_argument("-output_dir", type=str, default="./saved_models", help="Folder to save model weights")
    parser.add_argument("-weight_modulus", type=int, default=10, help="How often to save epoch weights (10 = every 10 epochs)")
    parser.add_argument("-print_modulus", type=int, default=100, help="How often to print a batch's losses and learn rate")
    parser.add_argument("-n_workers", type=int, default=4, help="Kept for flag compatibility; the feature files are read in-process")
    parser.add_argument("--force_cpu", type=bool, default=False, help="Kept for flag compatibility; this build has no CPU path")
    parser.add_argument("--no_tensorboard", type=bool, default=True, help="Kept for flag compatibility; tensorboard reporting is not built")
    parser.add_argument("-continue_weights", type=str, default=None, help="Model weights to continue training from")
    parser.add_argument("-continue_epoch", type=int, default=None, help="Epoch the continue_weights model was at")
    parser.add_argument("-lr", type=float, default=lr, help="Constant learn rate. Leave as None for the warm-up schedule")
    parser.add_argument("-ce_smoothing", type=float, default=0.1, help="Label smoothing of the chord cross-entropy")
    parser.add_argument("-batch_size", type=int, default=batch_size)
    parser.add_argument("-epochs", type=int, default=epochs)
    parser.add_argument("-max_sequence_midi", type=int, default=2048)
    parser.add_argument("-max_sequence_video", type=int, default=300)
    parser.add_argument("-max_sequence_chord", type=int, default=300)
    parser.add_argument("-n_layers", type=int, default=6)
    parser.add_argument("-num_heads", type=int, default=8)
    parser.add_argument("-d_model", type=int, default=512)
    parser.add_argument("-dim_feedforward", type=int, default=1024)
    parser.add_argument("-dropout", type=float, default=dropout)
    parser.add_argument("-rms_norm", type=bool, default=False)
    parser.add_argument("-is_video", type=bool, default=IS_VIDEO)
    parser.add_argument("-music_gen_version", type=str, default=music_gen_version, help="None is the base AMT model, the one that trains here")
    parser.add_argument("-vis_models", type=str, default=VIS_MODELS_SORTED)
    parser.add_argument("-emo_model", type=str, default="6c_l14p")
    parser.add_argument("-motion_type", type=int, default=motion_type, help="0 as original, 1 as option 1, 2 as option 2")
    parser.add_argument("-scene_embed", type=bool, default=False)
    parser.add_argument("-chord_embed", type=bool, default=chord_embed)
    parser.add_argument("-rpr", type=bool, default=rpr)
    parser.add_argument("-augmentation", type=bool, default=augmentation)
    parser.add_argument("-droptoken", type=float, default=droptoken)
    parser.add_argument("-optimizer", type=str, default=optimizer, help="Adam or AdamW")
    parser.add_argument("-auxiliary_loss", type=bool, default=auxiliary_loss)
    parser.add_argument("-drop_loss", type=bool, default=drop_loss)
    parser.add_argument("-balancing", type=bool, default=balancing)
    # additions of this build
    parser.add_argument("--seed", type=int, default=0, help="seeds the initial weights, the per-epoch clip order and the dropout masks")
    parser.add_argument("--train_ids", type=str, default="split:train",
                        help="clip ids to read from -dataset_dir, comma separated, or split:<name> for vevo_meta/split/v1/<name>.txt")
    parser.add_argument("--val_ids", type=str, default="split:val", help="as --train_ids, for the validation figures")
    parser.add_argument("--synthetic_weights", action="store_true", help="start from the procedural weights instead of torch's initialisation")
    parser.add_argument("--chord_embed_table", type=str, default=None,
                        help="the frozen chord table of -chord_embed: a .npy of shape (n_chords, d_model), float32 (train_families)")
    return parser.parse_known_args(argv)
