"""profiles/optim.json: one optimiser `step()` over a model's parameter list on one MI355X (not a test; run on the GPU box).

    python tools/bench_optim.py --out profiles/optim.json

Parameter lists (shapes of the trainable parameters; values and gradients are seeded noise):
  base       the base model as `train` builds it at the parser's defaults apart from -music_gen_version None -chord_embed ""
  v123       '1.2.3', the parser's default family model
  bimamba+   the 'bimamba+' regression head at d_model 64
Timed per list, alternating in one process, device events around --iters `step()` calls after --warmup (more than 6: every timed step
takes the rectified branch), best of --rounds rounds, profiler off; the gradients stay where they are (a training loop's are new
allocations, which costs the fused path nothing: it reads the pointers every step):
  ours_radam / ours_radamw / ours_radanw_foreach / ours_radanw_single   `video2music_amd.optim` on `amt_optim_step`
  torch_radam / torch_radamw        torch.optim.RAdam(foreach=True) without / with decoupled decay
  foreach_radanw                    the foreach variant of RAdanW in torch._foreach operators (tests/helpers_optim.py): the reference's
                                    own file does not exist on the GPU box
Per case: microseconds per step, kernel launches per step (ours: counted by the optimiser; torch's: device kernels of one step seen by
torch.profiler in a run of its own, null if the profiler is unavailable), and achieved bytes/s = 4 bytes x elements x (tensors read +
written per element by the mode: ops.OPTIM_TENSORS_MOVED; the torch cases are rated by the same necessary traffic) / time, next to the
6.29 TB/s float4-copy rate of the chip."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import helpers_optim as HO                                              # noqa: E402
from video2music_amd import ops, optim                                             # noqa: E402

COPY_RATE = 6.29e12
LR, BETAS, EPS, WD = 1e-3, (0.9, 0.98, 0.92, 0.99), 1e-8, 0.01


def shapes_of(name):
    from video2music_amd import train
    from video2music_amd.model.video_regression import VideoRegression
    if name == "bimamba+":
        m = VideoRegression(n_layers=2, d_model=64, d_hidden=256, dropout=0.2, total_vf_dim=768 + 6, regModel="bimamba+")
    else:
        args = train.parse_args(["-music_gen_version", "None", "-chord_embed", ""] if name == "base" else ["-music_gen_version", "1.2.3", "-chord_embed", ""])
        from video2music_amd.generate import total_vf_dim_of
        m = train.build_model(args, total_vf_dim_of(args, sem_dim=768))
    return [tuple(p.shape) for p in m.parameters() if p.requires_grad]


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
    return a.elapsed_time(b) / iters * 1e3


def kernels_of_one_step(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception:
        return None


class ForeachRAdanW:
    """helpers_optim.foreach_radanw_step with the optimiser's bookkeeping around it."""

    def __init__(self, params):
        self.params, self.t = params, 0
        self.state = [[torch.zeros_like(p) for p in params] for _ in range(4)]
        self.npg = None

    @torch.no_grad()
    def step(self):
        self.t += 1
        grads = [p.grad for p in self.params]
        if self.npg is None or self.t == 2:
            self.npg = [g.neg() for g in grads]
        HO.foreach_radanw_step(self.params, grads, *self.state, self.npg, HO.coefficients("radanw_foreach", self.t, LR, BETAS, EPS, WD))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lists", default="base,v123,bimamba+")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.warmup > 6
    dev = torch.device("cuda:0")
    makers = {"ours_radam": lambda ps: optim.RAdam(ps, lr=LR, betas=BETAS[:2], eps=EPS),
              "ours_radamw": lambda ps: optim.RAdam(ps, lr=LR, betas=BETAS[:2], eps=EPS, weight_decay=WD, decoupled_weight_decay=True),
              "ours_radanw_foreach": lambda ps: optim.RAdanW(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD),
              "ours_radanw_single": lambda ps: optim.RAdanW(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, variant="single"),
              "torch_radam": lambda ps: torch.optim.RAdam(ps, lr=LR, betas=BETAS[:2], eps=EPS, foreach=True),
              "torch_radamw": lambda ps: torch.optim.RAdam(ps, lr=LR, betas=BETAS[:2], eps=EPS, weight_decay=WD, decoupled_weight_decay=True,
                                                           foreach=True),
              "foreach_radanw": ForeachRAdanW}
    moved = {"ours_radam": "radam", "ours_radamw": "radamw", "ours_radanw_foreach": "radanw_foreach", "ours_radanw_single": "radanw_single",
             "torch_radam": "radam", "torch_radamw": "radamw", "foreach_radanw": "radanw_foreach"}
    res = {"unit": "microseconds per step(), device events", "iters": a.iters, "warmup": a.warmup, "rounds": a.rounds, "copy_rate_bytes_per_s": COPY_RATE,
           "plan": ops.optim_plan(), "tensors_moved_per_element": {k: list(v) for k, v in ops.OPTIM_TENSORS_MOVED.items()}, "lists": {}}
    for name in a.lists.split(","):
        shapes = shapes_of(name)
        elements = sum(int(torch.Size(s).numel()) for s in shapes)
        g = torch.Generator(device=dev).manual_seed(0)
        cases = {}
        for case, make in makers.items():
            params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g) * 0.1) for s in shapes]
            for p in params:
                p.grad = torch.randn(p.shape, device=dev, generator=g) * 0.01
            cases[case] = make(params)
        rec = {"tensors": len(shapes), "elements": elements, "us": {k: [] for k in cases}}
        for _ in range(a.rounds):
            for case, opt in cases.items():
                rec["us"][case].append(timed(opt.step, a.iters, a.warmup))
        rec["us_best"] = {k: min(v) for k, v in rec["us"].items()}
        rec["launches_per_step"] = {k: (o.last_step_launches if hasattr(o, "last_step_launches") else kernels_of_one_step(o.step)) for k, o in cases.items()}
        rec["bytes_per_step"] = {k: 4 * elements * sum(ops.OPTIM_TENSORS_MOVED[moved[k]]) for k in cases}
        rec["bytes_per_s"] = {k: rec["bytes_per_step"][k] / (rec["us_best"][k] * 1e-6) for k in cases}
        rec["share_of_copy_rate"] = {k: v / COPY_RATE for k, v in rec["bytes_per_s"].items()}
        res["lists"][name] = rec
        del cases
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
