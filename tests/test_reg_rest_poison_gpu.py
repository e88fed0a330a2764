"""Poisoned allocations (tests/helpers_poison.py, the four runs of tests/test_poison_gpu.py: twice plain, once per pattern -- every byte
0xFF, fp32 1e30 --, bit-equal throughout, finite, guards intact) for what the last five regression heads add: the wide-state training
scan and its backward, ConvSiluFn, and one training step of 'moemamba' after enable_training().  Every float of the new workspaces
(amt_selective_scan_wide_bwd_ws_floats: the per-block dB | dC copies, the per-clip dA / dD, the per-slice partials) and of the
checkpoints is written before the second launch or the backward reads it, or is never read."""
import numpy as np
import pytest
import torch

from tests import test_conv_silu_train_gpu as CS
from tests import test_scan_wide_bwd_gpu as SW
from tests.test_poison_gpu import four_runs
from video2music_amd import autograd as AG
from video2music_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("reverse", [0, 1])
def test_wide_scan_train_and_backward(reverse, version):
    N = 64
    B, L, ED = shape = (2, 33, 24)                       # one step past a checkpoint interval, a half-empty second channel block, 4 slices
    assert N in SW.WIDTHS
    c = SW.scan_case(B, L, ED, N, seed=B * 1000 + L)
    R, M = c["R"], B * L
    d = {k: v.to(DEV) for k, v in c.items() if k != "R"}

    def run():
        y, y_pre, h_chunks = ops.selective_scan_train(d["xc"], d["draw"], d["dt_bias"], d["A_log"], d["dbc"], R, d["D"], d["xz"], B, L,
                                                      version=version, reverse=reverse)
        dxz, ddbc = torch.zeros(M, 2 * ED, device=DEV), torch.zeros_like(d["dbc"])
        dx, ddraw, dA_log, dD = ops.selective_scan_bwd(d["dout"], d["xc"], d["draw"], d["dt_bias"], d["A_log"], d["dbc"], R, d["D"], d["xz"], y_pre,
                                                       h_chunks, dxz, ddbc, B, L, version=version, reverse=reverse)
        return {"y": y, "y_pre": y_pre, "h_chunks": h_chunks, "dx": dx, "ddraw": ddraw, "dz": dxz[:, ED:], "dBC": ddbc[:, R:R + 2 * N],
                "dA_log": dA_log, "dD": dD}

    four_runs(f"wide scan N {N} {shape} reverse {reverse} version {version}", run, ("ops",))


def test_conv_silu_fn():
    B, S, d = shape = (2, 7, 40)                         # S = K, a clip border inside the batch, a width the GEMM pads to 64
    x, w, b, dy = CS.case(B, S, d)

    def run():
        xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
        y = AG.ConvSiluFn.apply(xd, B, S, wd, bd)
        y.backward(dy.to(DEV))
        return {"y": y, "dx": xd.grad, "dW": wd.grad, "db": bd.grad}

    got = four_runs(f"ConvSiluFn {shape}", run, ("ops",))
    want = CS.autograd(x, w, b, dy, B, S, d, torch.float64)
    g32 = CS.autograd(x, w, b, dy, B, S, d, torch.float32)
    for k, n in (("y", CS.K * d), ("dx", CS.K * d), ("dW", B * S), ("db", B * S)):
        assert CS.rel_err(got[k].detach().cpu().numpy(), want[k]) <= max(8 * CS.rel_err(g32[k], want[k]), n * CS.U), k


def test_moemamba_training_step(golden):
    from tests import test_reg_rest_train_gpu as RG
    g = {**golden("g_reg_rest_train.npz"), **golden("g_reg_rest_train_b.npz"), **golden("g_reg_rest_train_64.npz")}
    name, b = "moemamba", RG.batch(g)

    def step(m):
        m.train()
        loss = RG.step_loss(m, b)
        loss.backward()
        return {"loss": loss, "grads": {k: p.grad for k, p in m.named_parameters()}}

    got = four_runs("moemamba training step", step, ("ops", "autograd"), make=lambda: RG.build(g, name))
    o, e32 = RG.oracle(g, name), float(g[f"{name}_e32_grad"])
    for k, v in got["grads"].items():
        assert RG.T.rel_err(v.cpu().numpy().astype(np.float64), o["grads"][k]) <= RG.bound(e32), k
