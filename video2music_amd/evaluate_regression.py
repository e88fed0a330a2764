"""``evaluate_regression.py`` entry point (reference ``evaluate_regression.py:33-107``, ``utilities/run_model_regression.py:70-125``):
the test-split figures of the loudness / note-density / instrument head -- total loss, RMSE note density, RMSE loudness, BCE
instrument.

``VideoRegression.get_feature`` runs over the split in batches of ``-batch_size`` clips; the encoder output stays on the device and
goes through one kernel per batch (``metrics.regression_metrics``) that applies both heads and reduces against the targets.  Its four
numbers per clip are the only thing copied back (one host synchronisation per batch).  The figures are formed per clip and averaged
over clips, as the reference does with its ``DataLoader(batch_size=1)``, whatever ``-batch_size`` is here: every layer of every
regModel works on a clip's own rows (the recurrences and scans run per clip, the mixture layers route token by token), so the clips
of a batch do not meet.  ``-augmentation``, ``-use_KAN``, ``-is_video False`` and sharding over ranks are not built.

    python -m video2music_amd.evaluate_regression -dataset_dir ./dataset/ -regModel bimamba+ -d_model 128 -batch_size 32
"""
import json
import os
import sys

import torch

from . import metrics
from .dataset import vevo_features as VF
from .model.video_regression import VideoRegression
from .utilities.argument_reg_funcs import parse_eval_args
from .utilities.device import get_device

LINES = (("avg_total_loss", "Avg Total loss"), ("avg_rmse_note_density", "Avg RMSE (Note Density)"),
         ("avg_rmse_loudness", "Avg RMSE (Loudness)"), ("avg_bce_instrument", "Avg BCE (Instrument)"))     # evaluate_regression.py:101-104


def parse_args(argv=None):
    return parse_eval_args(argv)[0]


def build_model(args, sem_dim):
    """evaluate_regression.py:68-87: total_vf_dim = semantic width + 6 or 5 emotion classes."""
    return VideoRegression(n_layers=args.n_layers, d_model=args.d_model, d_hidden=args.dim_feedforward, use_KAN=args.use_KAN,
                           max_sequence_video=args.max_sequence_video, total_vf_dim=sem_dim + (6 if args.emo_model.startswith("6c") else 5),
                           regModel=args.regModel, wide_recurrent=True)


def load_model(args, sem_dim, device):
    """build_model with -model_weights (or the procedural weights of --synthetic_weights) loaded, on the device, in eval mode."""
    model = build_model(args, sem_dim)
    if args.synthetic_weights:
        from . import synthetic
        shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(shapes, seed=0).items()})
    else:
        model.load_state_dict(torch.load(args.model_weights, map_location="cpu"))
    return model.to(device).eval()


def main(argv=None):
    args = parse_args(argv)
    if args.force_cpu:
        raise SystemExit("--force_cpu: video2music_amd has no CPU path (the CPU oracle lives in oracle/ for tests only)")
    if not args.is_video:
        raise SystemExit("-is_video False is not built")
    if args.use_KAN:
        raise SystemExit("-use_KAN: KANLinear heads are not built")
    if args.augmentation:
        raise SystemExit("-augmentation is not built: the test split is read as it is")
    device = get_device()
    if device.type != "cuda":
        raise SystemExit("no GPU visible: video2music_amd runs on MI355X only")
    names = (VF.read_split(args.dataset_dir, args.test_ids[6:], "v1") if args.test_ids.startswith("split:")
             else [t.strip() for t in args.test_ids.split(",") if t.strip()])
    if not names:
        raise SystemExit("no clips to evaluate")
    feats = VF.load_clips(args.dataset_dir, names, vis_models=args.vis_models, emo_model=args.emo_model, motion_type=args.motion_type,
                          max_seq_video=args.max_sequence_video, max_seq_chord=args.max_sequence_chord, regression_targets=True)
    model = load_model(args, feats["semantic"].shape[-1], device)

    rows = []
    bs = max(1, args.batch_size)
    keys = ("semantic", "scene_offset", "motion", "emotion", "note_density", "loudness", "instrument")
    with torch.set_grad_enabled(False):
        for b0 in range(0, len(names), bs):
            f = {k: torch.from_numpy(feats[k][b0:b0 + bs]).to(device) for k in keys}
            feat = model.get_feature(f["semantic"], f["scene_offset"], f["motion"], f["emotion"])
            m = metrics.regression_metrics(model, feat, f["note_density"], f["loudness"], f["instrument"])
            rows.append(torch.stack([m[k] for k in metrics.REG_FIELDS], dim=1).cpu())      # the batch's one host synchronisation
    per_clip = {k: torch.cat(rows)[:, i].numpy() for i, k in enumerate(metrics.REG_FIELDS)}
    summary = metrics.summarize_regression(per_clip)
    figures = metrics.regression_clip_figures(per_clip)

    for key, label in LINES:
        print(f"{label}: {summary[key]}")

    os.makedirs(args.output_dir, exist_ok=True)
    clips = [dict({"id": name}, **{k: float(per_clip[k][i]) for k in metrics.REG_FIELDS}, **{k: float(v[i]) for k, v in figures.items()})
             for i, name in enumerate(names)]
    with open(os.path.join(args.output_dir, "metrics.json"), "w") as fh:
        json.dump({"summary": summary, "clips": clips}, fh, indent=1)
    return summary


if __name__ == "__main__":
    main(sys.argv[1:])
