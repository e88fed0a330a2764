"""Golden fixture for the RAdanW optimiser, produced by the REFERENCE's own `model/RAdanW.py` run on the CPU in fp32, in both of its
variants passed explicitly (`foreach=False`: `_single_tensor_radanw`, `foreach=True`: `_multi_tensor_radanw`; the class default picks
the second on a GPU and the first on the CPU, and they are different optimisers).

TEST INFRASTRUCTURE.  Only arrays go in.  The reference file imports `torch.optim.optimizer._dispatch_sqrt`, which newer torch
releases no longer have; the tool puts a stand-in there before the import (`x.sqrt()` for tensors, `math.sqrt` for floats: what the
helper did).

tests/golden/g_optim.npz -- settings once (`lr`, `betas`, `eps`, `weight_decay`, `sizes` = 1, 5, 33 elements, `steps` = 8), then per
variant <v> in (single, foreach) and run <r>:
    <v>_<r>_p0_<i>            the initial parameter i
    <v>_<r>_grad_in_<i>       (steps, n) the gradients fed in (rows of NaN where the run feeds none)
    <v>_<r>_lrs               (steps,) the learning rate of every step
    <v>_<r>_<name>_<i>        (steps, n) after every step: name in p, exp_avg, exp_avg_sq, exp_diff, exp_diff_sq, neg_prev_grad, and
                              grad_out, the gradient tensor as the optimiser left it
    <v>_<r>_step_<i>          (steps,) the stored step count after every step
  runs: plain (a gradient every step, one rate), lag (parameter 1 has no gradient in steps 3 and 4), lr (the rate changes every step),
  decay (lr 0.1 and weight decay `decay_weight_decay` = 0.5: at the settings above 1 - lr wd = 0.9999 moves the Adan term by less than
  an fp32 rounding of the parameter).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_optim.py
"""
import math
import os
import sys

sys.dont_write_bytecode = True
import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle.make_goldens import REF                                     # noqa: E402

SIZES, STEPS = (1, 5, 33), 8
LR, BETAS, EPS, WD = 1e-2, (0.9, 0.98, 0.92, 0.99), 1e-9, 0.01
DECAY_LR, DECAY_WD = 0.1, 0.5             # 1 - lr wd = 0.95: a run on which the foreach variant's second (1 - lr wd) is visible in fp32
NAMES = ("exp_avg", "exp_avg_sq", "exp_diff", "exp_diff_sq", "neg_prev_grad")


def import_radanw():
    import torch
    import torch.optim.optimizer as O
    if not hasattr(O, "_dispatch_sqrt"):
        O._dispatch_sqrt = lambda x: x.sqrt() if isinstance(x, torch.Tensor) else math.sqrt(x)
    sys.path.insert(0, REF)
    from model import RAdanW
    return RAdanW


def record(RAdanW, out, tag, foreach, absent=(), lrs=None, wd=WD):
    import torch
    rng = np.random.default_rng(20)
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n).astype(np.float32))) for n in SIZES]
    grads = [rng.standard_normal((STEPS, n)).astype(np.float32) * np.float32(0.5) for n in SIZES]
    lrs = [LR] * STEPS if lrs is None else lrs
    opt = RAdanW.RAdanW(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, foreach=foreach)
    rows = {(name, i): [] for name in ("p", "grad_out", "step") + NAMES for i in range(len(SIZES))}
    for i, p in enumerate(params):
        out[f"{tag}_p0_{i}"] = p.detach().numpy().copy()
    for s in range(STEPS):
        opt.param_groups[0]["lr"] = lrs[s]
        for i, p in enumerate(params):
            if (i, s + 1) in absent:
                p.grad = None
                grads[i][s] = np.nan
            else:
                p.grad = torch.from_numpy(grads[i][s].copy())
        opt.step()
        for i, p in enumerate(params):
            st = opt.state[p]
            rows[("p", i)].append(p.detach().numpy().copy())
            rows[("grad_out", i)].append(np.full(SIZES[i], np.nan, np.float32) if p.grad is None else p.grad.numpy().copy())
            rows[("step", i)].append(float(st["step"]))
            for name in NAMES:
                rows[(name, i)].append(st[name].numpy().copy())
    for (name, i), v in rows.items():
        out[f"{tag}_{name}_{i}"] = np.array(v)
    for i in range(len(SIZES)):
        out[f"{tag}_grad_in_{i}"] = grads[i]
    out[f"{tag}_lrs"] = np.array(lrs)


def main():
    import torch
    torch.set_num_threads(1)
    RAdanW = import_radanw()
    out = {"lr": np.array(LR), "betas": np.array(BETAS), "eps": np.array(EPS), "weight_decay": np.array(WD), "sizes": np.array(SIZES),
           "steps": np.array(STEPS), "decay_weight_decay": np.array(DECAY_WD)}
    for v, foreach in (("single", False), ("foreach", True)):
        record(RAdanW, out, f"{v}_plain", foreach)
        record(RAdanW, out, f"{v}_lag", foreach, absent={(1, 3), (1, 4)})
        record(RAdanW, out, f"{v}_lr", foreach, lrs=[LR * (1 + 0.5 * math.sin(1.0 + s)) for s in range(STEPS)])
        record(RAdanW, out, f"{v}_decay", foreach, lrs=[DECAY_LR] * STEPS, wd=DECAY_WD)
    diff = max(float(np.abs(out[f"single_plain_p_{i}"][-1] - out[f"foreach_plain_p_{i}"][-1]).max()) for i in range(len(SIZES)))
    print("largest difference between the variants' parameters after", STEPS, "steps:", diff)
    path = os.path.join(REPO, "tests", "golden", "g_optim.npz")
    np.savez_compressed(path, **out)
    print("wrote g_optim.npz", len(out), "arrays,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 2 ** 20


if __name__ == "__main__":
    main()
