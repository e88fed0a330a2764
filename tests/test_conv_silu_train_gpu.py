"""autograd.ConvSiluFn (CNN_GRU's Conv1d(d, d, 7, padding 3) + SiLU: seven accumulating GEMMs, backward through amt_silu_bwd) and
amt_silu_bwd alone, against torch's CPU autograd of F.conv1d + F.silu in fp64.

Bound, the project's own (tests/test_mamba_bwd_gpu.py): rel_err(got, g64) <= max(8 e32, n U), e32 torch's fp32 CPU autograd of the same
function against the same fp64, n the longest sum behind a value (7 d for dx, B S for dW / db), U = 2^-24."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers_reg_train import U, rel_err
from video2music_amd import autograd as AG
from video2music_amd import ops
from video2music_amd.model.video_regression import VideoRegression

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 7
# (B, S, d): one frame (every tap but the centre in padding) at a width the GEMM pads to 32; S below the pad; S = K with a clip border
# inside the batch; two borders at the widest head; S over a tile of rows at a width that is no multiple of 32
SHAPES = [(1, 1, 8), (1, 3, 32), (2, 7, 32), (3, 8, 128), (2, 33, 40)]


def case(B, S, d):
    g = torch.Generator().manual_seed(100 * S + d)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(B * S, d), r(d, d, K) / (K * d) ** 0.5, 0.5 * r(d), r(B * S, d)


def autograd(x, w, b, dy, B, S, d, dtype):
    x_, w_, b_ = (t.to(dtype).clone().requires_grad_(True) for t in (x, w, b))
    y = F.silu(F.conv1d(x_.view(B, S, d).transpose(1, 2), w_, b_, padding=K // 2)).transpose(1, 2).reshape(B * S, d)
    (y * dy.to(dtype)).sum().backward()
    n64 = lambda t: t.detach().numpy().astype(np.float64)
    return {"y": n64(y), "dx": n64(x_.grad), "dW": n64(w_.grad), "db": n64(b_.grad)}


@pytest.mark.parametrize("shape", SHAPES)
def test_conv_silu_fn(shape):
    B, S, d = shape
    x, w, b, dy = case(B, S, d)

    def run():
        xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
        y = AG.ConvSiluFn.apply(xd, B, S, wd, bd)
        y.backward(dy.to(DEV))
        return {"y": y.detach(), "dx": xd.grad, "dW": wd.grad, "db": bd.grad}
    got, again = run(), run()
    assert all(torch.equal(got[k], again[k]) for k in got)
    if d % 32 == 0:                                     # a width VideoRegression takes: the module's own inference launches, same bits
        m = VideoRegression(n_layers=1, d_model=d, d_hidden=32, dropout=0.0, total_vf_dim=8, regModel="cnngru").to(DEV)
        with torch.no_grad():
            m.model.cnn[0].weight.copy_(w)
            m.model.cnn[0].bias.copy_(b)
        assert torch.equal(got["y"], m._conv7_silu(x.to(DEV), B, S))
    g64, g32 = autograd(x, w, b, dy, B, S, d, torch.float64), autograd(x, w, b, dy, B, S, d, torch.float32)
    report, bad = [], []
    for k, want in g64.items():
        n = B * S if k in ("dW", "db") else K * d
        bound = max(8 * rel_err(g32[k], want), n * U)
        e = rel_err(got[k].cpu().numpy(), want)
        report.append(f"{k} {e:.2e}/{bound:.2e}")
        if not e <= bound:
            bad.append(k)
    print(shape, " ".join(report))
    assert not bad, (bad, report)


def test_no_input_gradient_when_the_input_needs_none():
    B, S, d = 2, 7, 32
    x, w, b, dy = case(B, S, d)
    wd, bd = (t.to(DEV).requires_grad_(True) for t in (w, b))
    AG.ConvSiluFn.apply(x.to(DEV), B, S, wd, bd).backward(dy.to(DEV))
    want = autograd(x, w, b, dy, B, S, d, torch.float64)
    assert rel_err(wd.grad.cpu().numpy(), want["dW"]) <= B * S * U * 8 and rel_err(bd.grad.cpu().numpy(), want["db"]) <= B * S * U * 8


def test_silu_bwd_range():
    """|a| up to 90: exp(90) overflows fp32.  The derivative goes to 0 on the left and to 1 on the right, never NaN.  In between it is
    fp64's at (4 + 17) U |dy|: a few U for one expf, one division and three products, and the cancellation in 1 - s, whose absolute
    error U / 2 (s rounded; past a = 24 ln 2 = 16.6 the difference is 0 against a true e^-a <= U) is multiplied by a <= 17."""
    a = torch.cat([torch.linspace(-90.0, 90.0, 1441), torch.tensor([-90.0, -88.8, -20.0, 0.0, 20.0, 88.8, 90.0])])
    dy = torch.full_like(a, 1.5)
    got = ops.silu_bwd(dy.to(DEV), a.to(DEV)).cpu().double()
    assert torch.isfinite(got).all()
    a64 = a.double()
    s = torch.sigmoid(a64)
    want = 1.5 * s * (1 + a64 * (1 - s))
    assert float((got - want).abs().max()) <= 21 * U * 1.5
    assert float(got[a == -90.0].abs().max()) <= 1e-30 and float((got[a == 90.0] - 1.5).abs().max()) == 0.0
    with pytest.raises(AssertionError):
        ops.silu_bwd(dy.to(DEV)[:3], a.to(DEV))
