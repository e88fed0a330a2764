"""One training step of the base VideoMusicTransformer at the reference's training shape (6 + 6 layers, d_model 512, 8 heads,
dim_feedforward 1024, 32 clips x 299 chord positions x 300 video rows, motion_type 1, dropout 0.2, AdamW): training-state forward,
fused loss, backward, optimiser (not a test; run on the GPU box).

    python tools/bench_train.py --which ours            # the project's step alone
    python tools/bench_train.py --which both            # then, alternating with it, the comparison
    python tools/bench_train.py --auxiliary_loss        # the step with the -auxiliary_loss chord loss, alternating with the plain one
    python tools/bench_train.py --music_gen_version 1.2.3 2.2      # the base model's step, then the named V1 / V2 models' in the same
                                                                   # session (chord_embed, the same shape and optimiser; --rms_norm)

The comparison is the torch restatement of tests/helpers_train.py -- the same network written in torch operators, fp32 autograd on
the same GPU, torch's two loss expressions, the same AdamW -- from the same state dict, with a mask drawn on the device for every one
of the 122 dropout sites each step, as our step draws them.
Method: device events around --steps steps after --warmup, best of --rounds, profiler off.
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import helpers_train as T                                                # noqa: E402
from video2music_amd import synthetic, train_regression as TR                       # noqa: E402
from video2music_amd.losses import chord_train_loss                                 # noqa: E402
from video2music_amd.model.video_music_transformer import VideoMusicTransformer     # noqa: E402
from video2music_amd.utilities import constants as C                                # noqa: E402


def timed(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", choices=("ours", "both"), default="ours")
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dropout", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--music_gen_version", nargs="*", default=[], help="also time these V1 / V2 versions (train_families.TRAINABLE)")
    ap.add_argument("--rms_norm", action="store_true", help="build the V1 versions with rms_norm=True")
    ap.add_argument("--auxiliary_loss", action="store_true", help="also time the base model's step with the -auxiliary_loss chord loss "
                    "(train_losses; profiles/train_losses_step.json)")
    ap.add_argument("--skip_base", action="store_true", help="with --music_gen_version: do not time the base model (kernel traces)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, L, S = a.clips, 299, 300
    cfg = dict(n_layers=6, num_heads=8, d_model=512, dim_feedforward=1024, max_sequence_chord=300, max_sequence_video=300,
               total_vf_dim=synthetic.total_vf_dim(1), rpr=True)
    f = synthetic.synthetic_features(B, seed=1, n_frames=S, motion_type=1)
    rng = np.random.default_rng(0)
    ids = rng.integers(1, C.CHORD_END, size=(B, L + 1))
    ra = np.array([C.chord_to_root_attr(i) for i in range(C.CHORD_END)])
    bt = {"x": ids[:, :-1], "x_root": ra[ids[:, :-1], 0], "x_attr": ra[ids[:, :-1], 1], "tgt": ids[:, 1:],
          "emo_class": rng.integers(0, 6, size=(B, L)).astype(np.int32), "semantic": f["semantic"], "scene_offset": f["scene_offset"],
          "motion": f["motion"], "emotion": f["emotion"], "key": np.zeros((B, 1), dtype=np.float32)}
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in bt.items()}
    sd = T.state_dict(cfg)

    class Args:
        optimizer = "AdamW"
    ours = VideoMusicTransformer(dropout=a.dropout, **cfg)
    ours.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    ours = ours.to(dev).train()
    opt = TR.make_optimizer(Args, ours.parameters(), 1e-4)

    def step_ours():
        opt.zero_grad()
        y = ours(d["x"], d["x_root"], d["x_attr"], d["semantic"], d["key"], d["scene_offset"], d["motion"], d["emotion"])
        chord_train_loss(y, d["tgt"], d["emo_class"], C.LOSS_LAMBDA, 0.1).backward()
        opt.step()

    def step_ours_aux():
        opt.zero_grad()
        y = ours(d["x"], d["x_root"], d["x_attr"], d["semantic"], d["key"], d["scene_offset"], d["motion"], d["emotion"])
        chord_train_loss(y, d["tgt"], d["emo_class"], C.LOSS_LAMBDA, 0.1, auxiliary=True, layout="view").backward()
        opt.step()

    def family_step(version):
        """One training step of the V1 / V2 model `version` (chord_embed, synthetic weights) on the same batch."""
        from video2music_amd.model import video_music_transformer as M
        kw = {k: v for k, v in cfg.items() if k != "rpr"}
        if version[0] == "1":
            fam = M.VideoMusicTransformer_V1(version_name=version, dropout=a.dropout, chord_embed=True, rms_norm=a.rms_norm, **kw)
        else:
            fam = M.VideoMusicTransformer_V2(version_name=version, dropout=a.dropout, chord_embed=True, **kw)
        shapes = [(k, tuple(v.shape)) for k, v in fam.state_dict().items()]
        fam.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(shapes, seed=0).items()}, strict=False)
        fam = fam.to(dev).train()
        fopt = TR.make_optimizer(Args, [p for p in fam.parameters() if p.requires_grad], 1e-4)

        def step():
            fopt.zero_grad()
            y = fam(d["x"], d["x_root"], d["x_attr"], d["semantic"], d["key"], d["scene_offset"], d["motion"], d["emotion"])
            chord_train_loss(y, d["tgt"], d["emo_class"], C.LOSS_LAMBDA, 0.1).backward()
            fopt.step()
        return step

    res = {"shape": dict(cfg, clips=B, L=L, S=S, dropout=a.dropout), "steps": a.steps, "warmup": a.warmup, "ours_ms": [], "torch_ms": None}
    families = {v: family_step(v) for v in a.music_gen_version}
    if families:
        res["family_ms"] = {v: [] for v in families}
        res["rms_norm"] = bool(a.rms_norm)
    if a.auxiliary_loss:
        res["ours_aux_ms"] = []
    if a.which == "both":
        P = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in sd.items()}
        used = [p for k, p in P.items() if k not in T.UNUSED]
        topt = TR.make_optimizer(Args, used, 1e-4)

        def device_masks(p):
            """helpers_train.draw_masks, drawn by torch on the device."""
            dm, ff, H = cfg["d_model"], cfg["dim_feedforward"], cfg["num_heads"]
            el = lambda rows, w: (torch.rand(rows, w, device=dev) >= p).float() / (1.0 - p)
            at = lambda Lq, Lk: (torch.rand(B, H, Lq, Lk, device=dev) >= p).to(torch.uint8)
            m = T.Masks([], p)
            m += [el(B * S, dm), el(B * L, dm)]
            for _ in range(cfg["n_layers"]):
                m += [at(S, S), el(B * S, dm), el(B * S, ff), el(B * S, dm)]
            for _ in range(cfg["n_layers"]):
                m += [at(L, L), el(B * L, dm), at(L, S), el(B * L, dm), el(B * L, ff), el(B * L, dm)]
            return m

        def torch_forward():
            # helpers_train.forward concatenates a scalar motion column; the 512-wide motion of motion_type 1 goes in directly
            vfc = torch.cat([d["semantic"], d["scene_offset"].unsqueeze(-1), d["motion"], d["emotion"]], dim=-1)
            return T.forward(P, cfg, dict(bt, _vfc=vfc), masks=device_masks(a.dropout) if a.dropout > 0 else None)

        def step_torch():
            topt.zero_grad()
            T.loss(torch_forward(), bt, 0.1, C.LOSS_LAMBDA)[0].backward()
            topt.step()
        res["torch_ms"] = []
    for _ in range(a.rounds):
        if not (families and a.skip_base):
            res["ours_ms"].append(timed(step_ours, a.steps, a.warmup))
        if a.auxiliary_loss:
            res["ours_aux_ms"].append(timed(step_ours_aux, a.steps, a.warmup))
        for v, step in families.items():
            res["family_ms"][v].append(timed(step, a.steps, a.warmup))
        if a.which == "both":
            res["torch_ms"].append(timed(step_torch, a.steps, a.warmup))
    if res["ours_ms"]:
        res["ours_ms_best"] = min(res["ours_ms"])
    if a.auxiliary_loss:
        res["ours_aux_ms_best"] = min(res["ours_aux_ms"])
    if families:
        res["family_ms_best"] = {v: min(t) for v, t in res["family_ms"].items()}
    if res["torch_ms"]:
        res["torch_ms_best"] = min(res["torch_ms"])
    res["peak_memory_gb"] = torch.cuda.max_memory_allocated() / 2 ** 30
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
