"""``evaluate.py`` entry point (reference ``evaluate.py:39-165``, ``utilities/run_model_vevo.py:198-452``): the test-split
figures of a chord model -- chord / emotion / total loss, hits@1/3/5, accuracy and emotion-chord correspondence.

The model's teacher-forced ``forward`` runs over the split in batches of ``-batch_size`` clips (each clip computed as the
reference's batch of one); the logits stay on the device and
go through one metrics kernel per batch (``metrics.chord_metrics``), whose ten numbers per clip are the only thing copied back
(one host synchronisation per batch).  The per-clip ratios are then averaged over clips as the reference does at its default
``batch_size`` 1, whatever ``-batch_size`` is here.  Plots, the expert-emotion log, ``-is_video False`` and sharding over ranks
are not built.

    python -m video2music_amd.evaluate -dataset_dir ./dataset/ -music_gen_version 2.2 -motion_type 1 -batch_size 32
"""
import json
import os
import sys

import numpy as np
import torch

from . import metrics
from .dataset import vevo_features as VF
from .generate import total_vf_dim_of
from .model.video_music_transformer import (VideoMusicTransformer, VideoMusicTransformer_V1, VideoMusicTransformer_V2,
                                            VideoMusicTransformer_V3)
from .utilities.argument_eval_funcs import parse_eval_args
from .utilities.device import get_device


def read_top_chords(dataset_root, n=10):
    """Ids of the n leading chords of ``vevo_meta/top_chord.txt`` ("<name> <id> <count>" lines, :467-476), or None without the file."""
    path = os.path.join(dataset_root, "vevo_meta", "top_chord.txt")
    if not os.path.exists(path):
        return None
    with open(path, encoding="utf-8") as fh:
        rows = [line.strip().split(" ") for line in fh]
    return np.array([int(r[1]) for r in rows if len(r) == 3], dtype=np.int64)[:n]


def build_model(args, sem_dim):
    """The model family of -music_gen_version, as generate.py builds it (reference evaluate.py:101-131)."""
    common = dict(n_layers=args.n_layers, num_heads=args.num_heads, d_model=args.d_model, dim_feedforward=args.dim_feedforward,
                  max_sequence_midi=args.max_sequence_midi, max_sequence_video=args.max_sequence_video,
                  max_sequence_chord=args.max_sequence_chord, total_vf_dim=total_vf_dim_of(args, sem_dim=sem_dim))
    if args.music_gen_version is None:
        return VideoMusicTransformer(rpr=args.rpr, **common)
    if args.music_gen_version.startswith("1."):
        return VideoMusicTransformer_V1(version_name=args.music_gen_version, rms_norm=args.rms_norm, **common)
    if args.music_gen_version.startswith("3."):
        return VideoMusicTransformer_V3(version_name=args.music_gen_version, rms_norm=args.rms_norm, **common)
    return VideoMusicTransformer_V2(version_name=args.music_gen_version, rms_norm=args.rms_norm, **common)


def load_model(args, sem_dim, device):
    """build_model with -model_weights (or the procedural weights of --synthetic_weights) loaded, on the device, in eval mode."""
    model = build_model(args, sem_dim)
    if args.synthetic_weights:
        from . import synthetic
        shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(shapes, seed=0).items()}, strict=False)
    else:
        model.load_state_dict(torch.load(args.model_weights, map_location="cpu"))
    return model.to(device).eval()


def parse_args(argv=None):
    args = parse_eval_args(argv)[0]
    if args.music_gen_version in ("None", "none", ""):
        args.music_gen_version = None
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.music_gen_version is not None and not args.music_gen_version.startswith(("1.", "2.", "3.")):
        raise SystemExit("music_gen_version must be None (base AMT) or start with '1.', '2.' or '3.' (evaluate.py:101-131)")
    if args.force_cpu:
        raise SystemExit("--force_cpu: video2music_amd has no CPU path (the CPU oracle lives in oracle/ for tests only)")
    if not args.is_video:
        raise SystemExit("-is_video False (MusicTransformer) is not built")
    device = get_device()
    if device.type != "cuda":
        raise SystemExit("no GPU visible: video2music_amd runs on MI355X only")
    names = (VF.read_split(args.dataset_dir, args.test_ids[6:], "v1") if args.test_ids.startswith("split:")
             else [t.strip() for t in args.test_ids.split(",") if t.strip()])
    if not names:
        raise SystemExit("no clips to evaluate")
    Tc = args.max_sequence_chord
    feats = VF.load_clips(args.dataset_dir, names, vis_models=args.vis_models, emo_model=args.emo_model, motion_type=args.motion_type,
                          max_seq_video=args.max_sequence_video, max_seq_chord=Tc)
    if "tgt" not in feats:
        raise SystemExit("evaluation needs max_sequence_video >= max_sequence_chord (the emotion row of every target second)")
    model = load_model(args, feats["semantic"].shape[-1], device)

    rows, preds = [], []
    bs = max(1, args.batch_size)
    with torch.set_grad_enabled(False):
        for b0 in range(0, len(names), bs):
            f = {k: torch.from_numpy(v[b0:b0 + bs]).to(device) for k, v in feats.items()}
            # the reference evaluates clip by clip (batch_size 1); the V classes tie the clips of a batch together (raw RoPE view),
            # so their batches run as independent clips -- the base class's clips are independent anyway
            fwd = model.forward_clips if hasattr(model, "forward_clips") else model
            y = fwd(f["chord"][:, :Tc - 1].contiguous(), f["chord_root"][:, :Tc - 1].contiguous(), f["chord_attr"][:, :Tc - 1].contiguous(),
                      f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
            m = metrics.chord_metrics(y, f["tgt"], f["emo_class"], f["emo_prob"], return_rows=args.save_conf_matrix)
            if args.save_conf_matrix:
                host = torch.empty(m["pred"].shape, dtype=torch.int32, pin_memory=True)
                host.copy_(m["pred"], non_blocking=True)            # lands with the copy below
                preds.append(host)
            rows.append(torch.stack([m[k] for k in metrics.FIELDS], dim=1).cpu())      # the batch's one host synchronisation
    per_clip = {k: torch.cat(rows)[:, i].numpy() for i, k in enumerate(metrics.FIELDS)}
    summary = metrics.summarize(per_clip)
    ratios = metrics.clip_ratios(per_clip)

    print(f"Avg test loss (total): {summary['avg_total_loss']:.4f}")       # evaluate.py:155-160
    print(f"Avg test loss (chord): {summary['avg_loss_chord']:.4f}")
    print(f"Avg test loss (emotion): {summary['avg_loss_emotion']:.4f}")
    print(f"Avg test h1: {summary['avg_h1']:.4f}")
    print(f"Avg test h3: {summary['avg_h3']:.4f}")
    print(f"Avg test h5: {summary['avg_h5']:.4f}")

    os.makedirs(args.output_dir, exist_ok=True)
    clips = [dict({"id": name}, **{k: float(per_clip[k][i]) for k in metrics.FIELDS}, **{k: float(v[i]) for k, v in ratios.items()})
             for i, name in enumerate(names)]
    with open(os.path.join(args.output_dir, "metrics.json"), "w") as fh:
        json.dump({"summary": summary, "clips": clips}, fh, indent=1)
    if args.save_conf_matrix:       # run_model_vevo.py:334-368,454-560: true labels over all positions, ignored ones included
        pred = torch.cat(preds).numpy().reshape(-1)
        pred_root, pred_attr = metrics.pred_root_attr(pred)
        np.save(os.path.join(args.output_dir, "chord_root.npy"),
                metrics.confusion_matrix(feats["tgt_root"].reshape(-1), pred_root, np.arange(1, 13)))
        np.save(os.path.join(args.output_dir, "chord_attr.npy"),
                metrics.confusion_matrix(feats["tgt_attr"].reshape(-1), pred_attr, np.arange(1, 14)))
        top = read_top_chords(args.dataset_dir)
        if top is not None:
            np.save(os.path.join(args.output_dir, "chord.npy"), metrics.confusion_matrix(feats["tgt"].reshape(-1), pred, top))
    return summary


if __name__ == "__main__":
    main(sys.argv[1:])
