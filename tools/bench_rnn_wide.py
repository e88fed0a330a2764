"""profiles/rnn_wide.json: one bidirectional nn.LSTM / nn.GRU layer at B = 32 clips, L = 300 steps, d in {128, 256, 512}, forward and
forward + backward, on one MI355X (not a test; run on the GPU box).

    python tools/bench_rnn_wide.py --out profiles/rnn_wide.json

Arms, alternating in one process, one pair of device events around each of --reps calls after --warmup, profiler off; the record holds
the median and the min / max per arm, in microseconds per call:
  wide     the layer on the wide kernels (csrc/rnn_wide.hip): forward = the input GEMM + ops.rnn_wide_seq (L step launches); forward +
           backward = autograd.RnnLayerFn (amt_rnn_wide_seq_train_fwd, amt_rnn_wide_seq_bwd, the weight-gradient GEMMs), at d = 128 with
           ops.RNN_NARROW_MAX lowered to 0 for the call
  narrow   d = 128 only: the same two calls on the register kernels (csrc/rnn.hip), what RnnLayerFn runs there by default
  torch    torch's own nn.LSTM / nn.GRU on the same device with the same weights (eval + no_grad for the forward, train mode and
           y.backward(dy) for forward + backward); if it does not run, the record says why
and, for the wide and narrow arms, `recurrence`: the recurrence call alone (no input GEMM), plus `host_enqueue_us`: the host's wall time
to enqueue one wide forward (no synchronise inside the window), which bounds the call from below when it exceeds the device time."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video2music_amd import ops                                                     # noqa: E402
from video2music_amd.autograd import RnnLayerFn                                     # noqa: E402

NAMES = ("weight_ih", "bias_ih", "weight_hh", "bias_hh")
FW_U, BW_U = 4, 16                      # units per workgroup of the step kernels (csrc/rnn_wide.hip)


@contextlib.contextmanager
def narrow_max(v):
    old, ops.RNN_NARROW_MAX = ops.RNN_NARROW_MAX, v
    try:
        yield
    finally:
        ops.RNN_NARROW_MAX = old


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def summary(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--widths", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, L = a.clips, a.steps
    res = {"what": "one bidirectional layer, microseconds per call: median and min / max of --reps calls, each between its own device events",
           "shape": {"clips": B, "steps": L, "directions": 2}, "reps": a.reps, "warmup": a.warmup,
           "units_per_workgroup": {"forward": FW_U, "backward": BW_U},
           "launches_per_layer": {"wide forward": L, "wide backward": L, "narrow forward": 1, "narrow backward": 1}, "cases": []}
    for d in a.widths:
        for G, kind in ((4, "lstm"), (3, "gru")):
            rng = np.random.default_rng(d + G)
            mod = (torch.nn.LSTM if G == 4 else torch.nn.GRU)(d, d, 1, bidirectional=True, batch_first=True).to(dev)
            ps = [getattr(mod, nm + "_l0" + sfx) for sfx in ("", "_reverse") for nm in NAMES]
            stacked = tuple(torch.cat([ps[4 * r + k].detach() for r in range(2)]).contiguous() for k in range(4))
            x = torch.from_numpy(rng.standard_normal((B, L, d)).astype(np.float32)).to(dev)
            dy = torch.from_numpy(rng.standard_normal((B, L, 2 * d)).astype(np.float32)).to(dev)
            rows, dyr = x.view(B * L, d), dy.view(B * L, 2 * d)
            wi, bi, wh, bh = stacked
            xproj = ops.linear_ex(rows, wi, bi)
            yb = torch.empty(B * L, 2 * d, device=dev)

            def fwd(seq):
                return lambda: seq(ops.linear_ex(rows, wi, bi), wh, bh, yb, 0, B, L, d, G, n_dirs=2)

            def rec(seq):
                return lambda: seq(xproj, wh, bh, yb, 0, B, L, d, G, n_dirs=2)

            def train(switch):
                def run():
                    for q in ps:
                        q.grad = None
                    xt = rows.detach().requires_grad_(True)
                    with narrow_max(switch):
                        RnnLayerFn.apply(xt, B, L, G, False, stacked, *ps).backward(dyr)
                return run

            def torch_fwd():
                with torch.no_grad():
                    mod(x)

            def torch_train():
                for q in ps:
                    q.grad = None
                xt = x.detach().requires_grad_(True)
                mod(xt)[0].backward(dy)

            arms = {"wide": {"forward": fwd(ops.rnn_wide_seq), "forward_backward": train(0), "recurrence": rec(ops.rnn_wide_seq)}}
            if d <= 128:
                arms["narrow"] = {"forward": fwd(ops.rnn_seq), "forward_backward": train(128), "recurrence": rec(ops.rnn_seq)}
            case = {"d": d, "kind": kind, "us": {}}
            try:
                mod.eval()
                torch_fwd()
                mod.train()
                torch_train()
                torch.cuda.synchronize()
                arms["torch"] = {"forward": torch_fwd, "forward_backward": torch_train}
                with torch.no_grad():
                    mod.eval()
                    y_t = mod(x)[0].reshape(B * L, 2 * d)
                    fwd(ops.rnn_wide_seq)()
                    case["wide_vs_torch_max_abs_diff_y"] = float((yb - y_t).abs().max())
            except Exception as e:                                       # torch's module does not run on this machine: say so
                case["torch"] = f"did not run: {type(e).__name__}: {e}"
            times = {arm: {k: [] for k in fns} for arm, fns in arms.items()}
            for i in range(a.warmup + a.reps):
                for arm, fns in arms.items():
                    for k, fn in fns.items():
                        if arm == "torch":
                            mod.eval() if k == "forward" else mod.train()
                        t = one(fn)
                        if i >= a.warmup:
                            times[arm][k].append(t)
            case["us"] = {arm: {k: summary(v) for k, v in ks.items()} for arm, ks in times.items()}
            host = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rec(ops.rnn_wide_seq)()
                host.append((time.perf_counter() - t0) * 1e6)
            torch.cuda.synchronize()
            case["host_enqueue_us"] = summary(host)
            m = case["us"]["wide"]["recurrence"]["median"]
            case["wide_us_per_step"] = round(m / L, 2)
            print(json.dumps(case), flush=True)
            res["cases"].append(case)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
