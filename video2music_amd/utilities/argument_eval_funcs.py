"""``parse_eval_args``: the flag names and defaults of the reference's ``utilities/argument_funcs.py:131-174`` (and the two
flags ``evaluate.py:168-171`` parses itself), plus the input switches ``generate`` has (the reference tree ships neither weights
nor dataset features)."""
import argparse

from .constants import IS_VIDEO, VERSION

MUSIC_TYPE = "lab_v2_norm"            # utilities/constants.py:28
VIS_MODELS_SORTED = "2d/clip_l14p"    # utilities/constants.py:25,39-47
# module defaults of utilities/argument_funcs.py:4-20
rpr = True
chord_embed = True
music_gen_version = "1.2.3"
motion_type = 2
balancing = False


def parse_eval_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("-dataset_dir", type=str, default="./dataset/", help="Folder of VEVO dataset")
    parser.add_argument("-input_dir_music", type=str, default="./dataset/vevo_chord/" + MUSIC_TYPE, help="Kept for flag compatibility")
    parser.add_argument("-input_dir_video", type=str, default="./dataset/vevo_vis", help="Kept for flag compatibility")
    parser.add_argument("-model_weights", type=str, default="./saved_models/" + VERSION + "/best_loss_weights.pickle",
                        help="state_dict saved with torch.save (reference key names)")
    parser.add_argument("-n_workers", type=int, default=4, help="Kept for flag compatibility; the feature files are read in-process")
    parser.add_argument("--force_cpu", type=bool, default=False, help="Kept for flag compatibility; this build has no CPU path")
    parser.add_argument("-batch_size", type=int, default=1, help="Clips per forward / metrics call; the figures do not depend on it")
    parser.add_argument("-max_sequence_midi", type=int, default=2048)
    parser.add_argument("-max_sequence_video", type=int, default=300)
    parser.add_argument("-max_sequence_chord", type=int, default=300)
    parser.add_argument("-n_layers", type=int, default=6)
    parser.add_argument("-num_heads", type=int, default=8)
    parser.add_argument("-d_model", type=int, default=512)
    parser.add_argument("-dim_feedforward", type=int, default=1024)
    parser.add_argument("-rms_norm", type=bool, default=False)
    parser.add_argument("-music_gen_version", type=str, default=music_gen_version,
                        help="'1.x' / '2.x' / '3.x': VideoMusicTransformer_V1 / _V2 / _V3; 'None': the base AMT")
    parser.add_argument("-is_video", type=bool, default=IS_VIDEO)
    parser.add_argument("-vis_models", type=str, default=VIS_MODELS_SORTED)
    parser.add_argument("-emo_model", type=str, default="6c_l14p")
    parser.add_argument("-motion_type", type=int, default=motion_type, help="0 as original, 1 as option 1, 2 as option 2")
    parser.add_argument("-scene_embed", type=bool, default=False)
    parser.add_argument("-chord_embed", type=bool, default=chord_embed)
    parser.add_argument("-rpr", type=bool, default=rpr)
    parser.add_argument("-balancing", type=bool, default=balancing)
    # evaluate.py:168-171
    parser.add_argument("-save_conf_matrix", type=bool, nargs="?", const=True, default=False,
                        help="also write chord.npy / chord_root.npy / chord_attr.npy (confusion matrices) to -output_dir")
    parser.add_argument("-save_expert_emotion_plot", type=bool, default=False, help="Kept for flag compatibility; not built")
    # additions of this build
    parser.add_argument("-output_dir", type=str, default="./log", help="Folder for metrics.json and the confusion matrices "
                        "(the reference writes its matrices to ./log)")
    parser.add_argument("--test_ids", type=str, default="split:test",
                        help="clip ids to read from -dataset_dir, comma separated, or split:<name> for vevo_meta/split/v1/<name>.txt")
    parser.add_argument("--synthetic_weights", action="store_true", help="random-init procedural weights with real feature files")
    return parser.parse_known_args(argv)
