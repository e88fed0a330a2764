"""Where a training step of a V3 chord model spends its device time, beside the '2.2' step at the same shape (the shape of
tools/bench_train.py: 6 + 6 layers, d_model 512, 8 heads, d_ff 1024, 32 clips of 299 chord positions and 300 frames, dropout 0.2):

    python tools/v3_train_breakdown.py > profiles/v3_train_step.json

Step times are CUDA-event medians over `--steps` steps after `--warmup`; the time per kernel family comes from torch.profiler's
device-side kernel records of `--trace_steps` further steps (the families are told apart by kernel name; the attention backward's
kernels serve both attentions of '2.2' and both maps of every differential attention).  The last block times amt_diff_subln_bwd alone
at the step's own rows x head_dim next to amt_rmsnorm_bwd at the same rows x width -- the existing kernel of the same shape of work -- and
reports the bytes each moves per second (diff_subln_bwd: 5 streams of rows x hd x 4 B; rmsnorm_bwd: 3)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video2music_amd import ops, synthetic                                 # noqa: E402
from video2music_amd import train_regression as TR                         # noqa: E402
from video2music_amd.losses import chord_train_loss                        # noqa: E402
from video2music_amd.model import video_music_transformer as M             # noqa: E402
from video2music_amd.utilities import constants as C                       # noqa: E402

FAMILIES = (("diff_subln_bwd_kernel", "differential tail backward (diff_subln_bwd_kernel)"),
            ("diff_subln_dev_lambda_kernel", "differential tail forward (diff_subln_dev_lambda_kernel)"),
            ("attn_bwd_", "attention backward (attn_bwd_dq / attn_bwd_dkv kernels)"), ("dq_finish", "attention backward (dq_finish_kernel)"),
            ("attn_", "attention forward (tiled / split-key kernels)"), ("gemm_f32", "GEMM (gemm_f32_kernel)"), ("decode_gemm", "skinny GEMM"),
            ("moe_wgrad", "weight-gradient product (moe_wgrad_kernel / _reduce)"), ("moe_route_biased", "balancing router (moe_route_biased_kernel)"),
            ("moe_", "other mixture kernels"), ("norm_bwd_kernel", "norm backward"), ("norm_kernel", "norm forward"), ("rope", "rotary forward / backward"))


def events_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def kernel_families(fn, steps):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
        rows = [(e.key, e.count, getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)) for e in prof.key_averages()
                if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()]
    except Exception as exc:                                               # the profiler is optional: the step times stand without it
        return {"unavailable": repr(exc)}
    total = sum(r[2] for r in rows)
    if not rows or total <= 0:
        return {"unavailable": "the profiler returned no device-side kernel records"}
    left, fam = list(rows), {}
    for key, label in FAMILIES:
        sel = [r for r in left if key in r[0]]
        left = [r for r in left if key not in r[0]]
        if sel:
            fam[label] = {"launches_per_step": round(sum(r[1] for r in sel) / steps, 1), "us_per_step": round(sum(r[2] for r in sel) / steps, 1),
                          "share": round(sum(r[2] for r in sel) / total, 4)}
    fam["everything else (torch's own kernels, copies)"] = {"us_per_step": round(sum(r[2] for r in left) / steps, 1),
                                                           "share": round(sum(r[2] for r in left) / total, 4)}
    return {"device_ms_per_step": round(total / 1e3 / steps, 3), "families": fam}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace_steps", type=int, default=3)
    ap.add_argument("--dropout", type=float, default=0.2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, L, S = a.clips, 299, 300
    cfg = dict(n_layers=6, num_heads=8, d_model=512, dim_feedforward=1024, max_sequence_chord=300, max_sequence_video=300,
               total_vf_dim=synthetic.total_vf_dim(1))
    f = synthetic.synthetic_features(B, seed=1, n_frames=S, motion_type=1)
    rng = np.random.default_rng(0)
    ids = rng.integers(1, C.CHORD_END, size=(B, L + 1))
    ra = np.array([C.chord_to_root_attr(i) for i in range(C.CHORD_END)])
    bt = {"x": ids[:, :-1], "x_root": ra[ids[:, :-1], 0], "x_attr": ra[ids[:, :-1], 1], "tgt": ids[:, 1:],
          "emo_class": rng.integers(0, 6, size=(B, L)).astype(np.int32), "semantic": f["semantic"], "scene_offset": f["scene_offset"],
          "motion": f["motion"], "emotion": f["emotion"], "key": np.zeros((B, 1), dtype=np.float32)}
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in bt.items()}

    class Args:
        optimizer = "AdamW"

    def step_of(version):
        cls = M.VideoMusicTransformer_V3 if version[0] == "3" else M.VideoMusicTransformer_V2
        m = cls(version_name=version, dropout=a.dropout, chord_embed=True, **cfg)
        shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(shapes, seed=0).items()}, strict=False)
        m = m.to(dev).train().enable_training()
        opt = TR.make_optimizer(Args, [p for p in m.parameters() if p.requires_grad], 1e-4)

        def step():
            opt.zero_grad()
            y = m(d["x"], d["x_root"], d["x_attr"], d["semantic"], d["key"], d["scene_offset"], d["motion"], d["emotion"])
            chord_train_loss(y, d["tgt"], d["emo_class"], C.LOSS_LAMBDA, 0.1).backward()
            opt.step()
        return step

    res = {"shape": dict(cfg, clips=B, L=L, S=S, dropout=a.dropout), "steps": a.steps, "warmup": a.warmup, "trace_steps": a.trace_steps,
           "device": torch.cuda.get_device_name(0)}
    for version in ("3.1", "2.2"):
        step = step_of(version)
        ms = events_ms(step, a.steps, a.warmup)
        res[version] = {"step_ms_median": round(statistics.median(ms), 3), "step_ms_min": round(min(ms), 3), "step_ms_max": round(max(ms), 3),
                        "kernels": kernel_families(step, a.trace_steps)}
    fam = res["3.1"]["kernels"].get("families", {})
    if fam:
        res["3.1"]["share_diff_subln_bwd"] = fam.get(FAMILIES[0][1], {}).get("share")
        res["3.1"]["share_attention_backward"] = round(sum(fam.get(FAMILIES[i][1], {}).get("share", 0.0) for i in (2, 3)), 4)
    # the tail's backward alone, next to the RMSNorm backward at the same rows x width
    H, hd = cfg["num_heads"], cfg["d_model"] // cfg["num_heads"]
    rows = B * H * L
    t = lambda *s: torch.randn(*s, device=dev)
    dy, o1, o2, w, lam = t(rows, hd), t(rows, hd), t(rows, hd), t(hd), torch.full((1,), 0.3, device=dev)
    tail = events_ms(lambda: ops.diff_subln_bwd(dy, o1, o2, w, lam, 0.6), 50, 10)
    rms = events_ms(lambda: ops.rmsnorm_bwd(dy, o1, w), 50, 10)
    res["diff_subln_bwd_alone"] = {
        "rows": rows, "hd": hd, "workgroups": ops.diff_subln_bwd_blocks(rows, hd),
        "diff_subln_bwd_us_median": round(1e3 * statistics.median(tail), 2), "diff_subln_bwd_bytes": 5 * rows * hd * 4,
        "diff_subln_bwd_GBps": round(5 * rows * hd * 4 / (statistics.median(tail) * 1e-3) / 1e9, 1),
        "rmsnorm_bwd_workgroups": ops.rmsnorm_bwd_blocks(rows),
        "rmsnorm_bwd_us_median": round(1e3 * statistics.median(rms), 2), "rmsnorm_bwd_bytes": 3 * rows * hd * 4,
        "rmsnorm_bwd_GBps": round(3 * rows * hd * 4 / (statistics.median(rms) * 1e-3) / 1e9, 1),
        "note": "event timings of the Python wrapper, which allocates the outputs and the workspace and zeroes the ticket: both kernels alike"}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
