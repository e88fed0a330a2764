"""One training step of VideoRegression at the reference's defaults ('bilstm', d_model 64, 2 layers, dropout 0.2, B 32, S 300,
768 + 6 features): forward, fused loss, backward, Adam (not a test; run on the GPU box).

    python tools/bench_reg_train.py --which ours            # the project's step alone
    python tools/bench_reg_train.py --which both            # then, alternating with it, the comparison
    python tools/bench_reg_train.py --which ours --regModel bimamba+      # any head whose backward is built; the comparison stack
                                                                          # below is the recurrent heads' only

The comparison is the way the reference itself would run on this GPU: torch's own nn.Linear / nn.LSTM modules and autograd on the
device, built from the same state dict, the reference's loss expressions, the same Adam.  Method: device events around --steps
steps after --warmup, best of --rounds, profiler off.  Prints one JSON line; "torch_ms": null with "torch_error" where torch's GPU
recurrent path does not run."""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video2music_amd import train_regression as TR                                  # noqa: E402
from video2music_amd.losses import regression_train_loss                            # noqa: E402
from video2music_amd.model.video_regression import VideoRegression                  # noqa: E402


class TorchStack(nn.Module):
    """The recurrent VideoRegression on torch's own modules (the reference's module structure and state-dict keys)."""

    def __init__(self, F, d, n_layers, dropout, reg_model):
        super().__init__()
        bi = "bi" in reg_model
        self.model = (nn.LSTM if "lstm" in reg_model else nn.GRU)(d, d, n_layers, bidirectional=bi, dropout=dropout, batch_first=True)
        self.in_proj = nn.Sequential(nn.Linear(F, d), nn.Dropout(dropout))
        self.regressor = nn.Linear(d * (2 if bi else 1), 2)
        self.classifier = nn.Sequential(nn.Linear(d * (2 if bi else 1), 40), nn.Sigmoid())

    def forward(self, sem, scene, motion, emo):
        out = self.model(self.in_proj(torch.cat([sem, emo], dim=-1)))[0]
        return self.regressor(out), self.classifier(out)


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
    ap.add_argument("--regModel", default="bilstm")
    ap.add_argument("--d_model", type=int, default=64)
    ap.add_argument("--n_layers", type=int, default=2)
    ap.add_argument("--dropout", type=float, default=0.2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=300)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.which == "both" and "mamba" in a.regModel:
        ap.error("--which both compares against torch's nn.LSTM / nn.GRU: use --which ours for a Mamba head")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, S, F = a.batch, a.seq, 774
    sem, emo = torch.randn(B, S, F - 6, device=dev), torch.softmax(torch.randn(B, S, 6, device=dev), -1)
    nd, ld = 8 * torch.rand(B, S, device=dev), 4 * torch.rand(B, S, device=dev)
    inst = (torch.rand(B, S, 40, device=dev) < 0.25).float()
    tgt = torch.stack([nd.reshape(-1), ld.reshape(-1)], dim=1)

    ours = VideoRegression(n_layers=a.n_layers, d_model=a.d_model, d_hidden=256, dropout=a.dropout, total_vf_dim=F, regModel=a.regModel).to(dev).train()
    adam = lambda m: torch.optim.Adam(m.parameters(), lr=1e-4, betas=(TR.ADAM_BETA_1, TR.ADAM_BETA_2), eps=TR.ADAM_EPSILON)
    opt = adam(ours)

    def step_ours():
        opt.zero_grad()
        ln_nd, p = ours(sem, None, None, emo)
        regression_train_loss(ln_nd, p, nd, ld, inst).backward()
        opt.step()

    res = {"config": vars(a), "ours_ms": None, "torch_ms": None}
    ref_step = None
    if a.which == "both":
        try:
            ref = TorchStack(F, a.d_model, a.n_layers, a.dropout, a.regModel)
            ref.load_state_dict({k: v.detach().cpu().clone() for k, v in ours.state_dict().items()}, strict=True)
            ref = ref.to(dev).train()
            ropt = adam(ref)

            def ref_step():
                ropt.zero_grad()
                ln_nd, p = ref(sem, None, None, emo)
                (nn.SmoothL1Loss()(ln_nd.reshape(-1, 2), tgt) + nn.functional.binary_cross_entropy(p, inst)).backward()
                ropt.step()
            ref_step()
            torch.cuda.synchronize()
        except Exception as e:                              # torch's GPU recurrent path is not available here: say so, keep our figure
            res["torch_error"] = f"{type(e).__name__}: {e}"[:300]
            ref_step = None
    t_ours, t_ref = [], []
    for _ in range(a.rounds):
        t_ours.append(timed(step_ours, a.steps, a.warmup))
        if ref_step is not None:
            t_ref.append(timed(ref_step, a.steps, a.warmup))
    res["ours_ms"], res["ours_rounds_ms"] = min(t_ours), t_ours
    if t_ref:
        res["torch_ms"], res["torch_rounds_ms"] = min(t_ref), t_ref
    print(json.dumps(res))


if __name__ == "__main__":
    main()
