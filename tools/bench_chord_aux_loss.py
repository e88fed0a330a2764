"""profiles/chord_aux_loss.json: the chord training loss with the auxiliary terms, forward plus gradient, at the training shape
(32 clips x 299 positions x 159 classes) on one MI355X (not a test; run on the GPU box).

    python tools/bench_chord_aux_loss.py --out profiles/chord_aux_loss.json

Timed, alternating in one process, device events around --iters calls after --warmup, --rounds rounds, profiler off:
  aux_view / aux_rows   ops.chord_loss_aux with backward=True (amt_chord_loss_aux_fwd_bwd: the memset, the loss kernel, the combine
                        kernel) in the two layouts, with the three torch.empty of a call
  plain                 ops.chord_loss with backward=True (amt_chord_loss_fwd_bwd), the loss without the auxiliary terms, for scale
  torch_view            the reference's composition written in torch operators on the same device tensors -- CrossEntropyLoss,
                        two top-k hinge terms as model/loss.py:85-141 forms them (one_hot, softmax, topk, relu, masked_fill, mean
                        over the valid targets), the `> 1e-10` count read on the host as CombinedLoss reads it, BCEWithLogitsLoss on
                        prebuilt emotion rows -- and `backward()` to the logits
The record also holds the largest difference between torch_view's loss / gradient and aux_view's on the timed inputs."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import helpers_eval as HE                                                # noqa: E402
from video2music_amd import ops                                                     # noqa: E402
from video2music_amd.utilities import constants as C                                # noqa: E402

NC = C.CHORD_SIZE


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3           # microseconds per call


def topk_hinge(y_bcl, tgt, k, weight):
    """TopKAuxiliaryLoss(k, weight, vocab_size=159, ignore_index=PAD)(y.permute(0, 2, 1), tgt), operator for operator."""
    mask = (tgt == C.CHORD_PAD).unsqueeze(-1)
    onehot = torch.nn.functional.one_hot(tgt, NC).float().masked_fill(mask, 0)
    pred = torch.softmax(y_bcl.reshape(onehot.shape), dim=-1)
    top, _ = torch.topk(pred, k=k, dim=-1)
    loss = torch.relu(top.sum(-1) / k - (pred * onehot).sum(-1)).masked_fill(mask.squeeze(), 0)
    return loss.sum() / (tgt != C.CHORD_PAD).sum() * weight


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, L, lam, eps = a.clips, 299, C.LOSS_LAMBDA, 0.1
    rng = np.random.default_rng(0)
    tgt_np = rng.integers(0, C.CHORD_END, size=(B, L))
    tgt_np[:, L - 20:] = C.CHORD_PAD                        # clips end in padding, as the dataset's do
    emo_np = rng.integers(0, 6, size=(B, L)).astype(np.int32)
    y = torch.from_numpy((3 * rng.standard_normal((B, L, NC))).astype(np.float32)).to(dev)
    tgt, emo = torch.from_numpy(tgt_np).to(dev), torch.from_numpy(emo_np).to(dev)
    rows = torch.from_numpy(HE.emotion_rows(tgt_np, np.where(emo_np < 5, emo_np, 5))).float().to(dev)
    ce = torch.nn.CrossEntropyLoss(ignore_index=C.CHORD_PAD, label_smoothing=eps)
    bce = torch.nn.BCEWithLogitsLoss()
    leaf = y.clone().requires_grad_(True)

    def torch_view():
        leaf.grad = None
        yp = leaf.permute(0, 2, 1)
        total, count = torch.zeros((), device=dev), 0
        for term in (ce(yp, tgt), topk_hinge(yp, tgt, 3, 3.0), topk_hinge(yp, tgt, 5, 5.0)):
            if term > 1e-10:                                 # CombinedLoss: a host read per term
                count += 1
            total = total + term
        loss = lam * (total / count) + (1 - lam) * bce(yp, rows.permute(0, 2, 1))
        loss.backward()
        return loss

    cases = {"aux_view": lambda: ops.chord_loss_aux(y, tgt, emo, lam, 1 - lam, eps, "view"),
             "aux_rows": lambda: ops.chord_loss_aux(y, tgt, emo, lam, 1 - lam, eps, "rows"),
             "plain": lambda: ops.chord_loss(y, tgt, emo, lam, eps),
             "torch_view": torch_view}
    loss_k, _, d_k = cases["aux_view"]()
    loss_t = torch_view()
    res = {"shape": {"clips": B, "L": L, "classes": NC, "smoothing": eps, "weights": [lam, 1 - lam]}, "iters": a.iters, "warmup": a.warmup,
           "unit": "microseconds per call, forward + gradient", "us": {k: [] for k in cases},
           "aux_view_vs_torch_view": {"loss": [float(loss_k[0]), float(loss_t.detach())],
                                      "dlogits_max_abs_diff": float((d_k - leaf.grad).abs().max()), "dlogits_max_abs": float(leaf.grad.abs().max())}}
    for _ in range(a.rounds):
        for k, fn in cases.items():
            res["us"][k].append(timed(fn, a.iters, a.warmup))
    res["us_best"] = {k: min(v) for k, v in res["us"].items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
