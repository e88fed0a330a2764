"""amt_selective_scan_train_fwd / amt_selective_scan_bwd / amt_dwconv1d_silu_bwd (csrc/mamba.hip, csrc/mamba_bwd.hip) alone, against
torch's CPU autograd in fp64 on the restatement of tests/helpers_reg_mamba_train.py (the scan as the plain sequential recurrence).

Bound, the project's own (tests/test_rnn_train_gpu.py, tests/test_layernorm_bwd_gpu.py): for every gradient
rel_err(got, g64) <= max(8 e32, n U), e32 torch's fp32 CPU autograd of the same restatement against the same fp64, n the longest
sum behind a value (B L for a parameter's gradient, L N for a value at the end of a state chain), U = 2^-24."""
import numpy as np
import pytest
import torch

from tests import helpers_reg_mamba_train as T
from video2music_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 16
# (B, L, ED): one step; one short chunk and a half-empty second block; a chunk boundary + 1; three chunks and a channel tail
SHAPES = [(1, 1, 16), (2, 31, 24), (2, 33, 64), (1, 70, 40)]


def err(got, want):
    """T.rel_err; where the gradient is exactly zero (dA_log of a one-step sequence) the kernel's must be too."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if not np.abs(want).max():
        return float(np.abs(got).max())
    return T.rel_err(got, want)


def scan_case(B, L, ED, seed):
    g = torch.Generator().manual_seed(seed)
    R = -(-(ED // 2) // 16)                             # dt_rank of the block whose d_inner is ED
    ld = (R + 2 * N + 3) // 4 * 4                       # the row stride of the model's x_proj output
    M = B * L
    r = lambda *s: torch.randn(*s, generator=g)
    c = {"xc": r(M, ED), "draw": 0.5 * r(M, ED), "dt_bias": r(ED) - 1.0,
         "A_log": torch.log(torch.arange(1, N + 1, dtype=torch.float32)).repeat(ED, 1) + 0.1 * r(ED, N),
         "dbc": 0.5 * r(M, ld), "D": 1.0 + 0.1 * r(ED), "xz": r(M, 2 * ED), "dout": r(M, ED), "R": R}
    c["draw"][0, 0] = 25.0                              # past softplus's threshold
    return c


def scan_autograd(c, B, L, ED, version, reverse, dtype):
    R = c["R"]
    leaf = lambda t: t.to(dtype).clone().requires_grad_(True)
    x, draw, z = (leaf(t.view(B, L, -1)) for t in (c["xc"], c["draw"], c["xz"][:, ED:]))
    Bm, Cm = leaf(c["dbc"][:, R:R + N].reshape(B, L, N)), leaf(c["dbc"][:, R + N:R + 2 * N].reshape(B, L, N))
    dt_bias, A_log, D = leaf(c["dt_bias"]), leaf(c["A_log"]), leaf(c["D"])
    out = T.scan_gate(x, draw, dt_bias, A_log, Bm, Cm, D, z, version, reverse)
    (out * c["dout"].view(B, L, ED).to(dtype)).sum().backward()
    flat = lambda t: t.grad.reshape(B * L, -1).numpy().astype(np.float64)
    return {"dx": flat(x), "ddraw": flat(draw), "dz": flat(z), "dB": flat(Bm), "dC": flat(Cm), "d_dt_bias": dt_bias.grad.numpy().astype(np.float64),
            "dA_log": A_log.grad.numpy().astype(np.float64), "dD": D.grad.numpy().astype(np.float64)}


@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_selective_scan_backward(shape, reverse, version):
    B, L, ED = shape
    c = scan_case(B, L, ED, seed=B * 1000 + L)
    R, M = c["R"], B * L
    d = {k: v.to(DEV) for k, v in c.items() if k != "R"}
    fwd = (d["xc"], d["draw"], d["dt_bias"], d["A_log"], d["dbc"], R, d["D"], d["xz"], B, L)
    y_eval = ops.selective_scan(*fwd, version=version, reverse=reverse)
    y, y_pre, h_chunks = ops.selective_scan_train(*fwd, version=version, reverse=reverse)
    assert torch.equal(y, y_eval)                                           # the training forward: the same bits
    assert h_chunks.shape == (B, (L + 31) // 32, ED, N) and not h_chunks[:, 0].any()

    def run():
        dxz = torch.full((M, 2 * ED), float("nan"), device=DEV)
        ddbc = torch.full_like(d["dbc"], float("nan"))
        dx, ddraw, dA_log, dD = ops.selective_scan_bwd(d["dout"], d["xc"], d["draw"], d["dt_bias"], d["A_log"], d["dbc"], R, d["D"], d["xz"], y_pre,
                                                       h_chunks, dxz, ddbc, B, L, version=version, reverse=reverse)
        assert torch.isnan(dxz[:, :ED]).all() and torch.isnan(ddbc[:, :R]).all() and torch.isnan(ddbc[:, R + 2 * N:]).all()   # not its columns
        return {"dx": dx, "ddraw": ddraw, "dz": dxz[:, ED:], "dB": ddbc[:, R:R + N], "dC": ddbc[:, R + N:R + 2 * N],
                "d_dt_bias": ddraw.sum(0), "dA_log": dA_log, "dD": dD}
    got, again = run(), run()
    for k in got:
        if k != "d_dt_bias":
            assert torch.equal(got[k], again[k]), k                         # no atomics: the same bits twice
    g64, g32 = scan_autograd(c, B, L, ED, version, reverse, torch.float64), scan_autograd(c, B, L, ED, version, reverse, torch.float32)
    report, bad = [], []
    for k, want in g64.items():
        n = B * L if k in ("dA_log", "dD", "d_dt_bias") else L * N
        bound = max(8 * err(g32[k], want), n * T.U)
        e = err(got[k].cpu().numpy(), want)
        report.append(f"{k} {e:.2e}/{bound:.2e}")
        if not e <= bound:
            bad.append(k)
    print(shape, "reverse", reverse, "version", version, " ".join(report))
    assert not bad, (bad, report)


# the kernel's block is 64 channels x 64 rows.  (3, 50, 80): three row slices, the last of 22 rows, and a second channel block of 16;
# (1, 3, 130) at K = 8: fewer steps than taps, a third channel block of 2; K = 1: no neighbour at all
DWCONV = [(s, 4) for s in SHAPES] + [((2, 33, 64), 8), ((3, 50, 80), 4), ((1, 3, 130), 8), ((2, 33, 24), 1)]


def dwconv_case(shape, K):
    B, L, C = shape
    g = torch.Generator().manual_seed(L * 10 + K)
    M = B * L
    return torch.randn(M, 2 * C, generator=g), 0.5 * torch.randn(C, K, generator=g), torch.randn(C, generator=g), torch.randn(M, C, generator=g)


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("shape,K", DWCONV)
def test_dwconv_silu_backward(shape, K, reverse):
    B, L, C = shape
    M = B * L
    xz, w, bias, dy = dwconv_case(shape, K)

    def autograd(dtype):
        x, w_, b_ = (t.to(dtype).clone().requires_grad_(True) for t in (xz[:, :C].reshape(B, L, C), w, bias))
        (T.conv_silu(x, w_, b_, bool(reverse)) * dy.view(B, L, C).to(dtype)).sum().backward()
        return {"dx": x.grad.reshape(M, C).numpy().astype(np.float64), "dw": w_.grad.numpy().astype(np.float64), "dbias": b_.grad.numpy().astype(np.float64)}

    def run():
        dxz = torch.full((M, 2 * C), float("nan"), device=DEV)
        dw, dbias = ops.dwconv1d_silu_bwd(dy.to(DEV), xz.to(DEV), C, w.to(DEV), bias.to(DEV), dxz, B, L, bool(reverse))
        assert torch.isnan(dxz[:, C:]).all()
        return {"dx": dxz[:, :C], "dw": dw, "dbias": dbias}
    got, again = run(), run()
    assert all(torch.equal(got[k], again[k]) for k in got)
    g64, g32 = autograd(torch.float64), autograd(torch.float32)
    report, bad = [], []
    for k, want in g64.items():
        n = K if k == "dx" else B * L
        bound = max(8 * err(g32[k], want), n * T.U)
        e = err(got[k].cpu().numpy(), want)
        report.append(f"{k} {e:.2e}/{bound:.2e}")
        if not e <= bound:
            bad.append(k)
    print(shape, "K", K, "reverse", reverse, " ".join(report))
    assert not bad, (bad, report)


@pytest.mark.parametrize("reverse", [0, 1])
def test_dwconv_silu_backward_without_a_bias(reverse):
    """bias = dbias = null at the library call (ops.dwconv1d_silu_bwd always passes one): against autograd of the convolution without
    a bias; and a bias without its gradient is refused."""
    shape, K = (3, 50, 80), 4
    B, L, C = shape
    M = B * L
    xz, w, _, dy = dwconv_case(shape, K)

    def autograd(dtype):
        x, w_ = (t.to(dtype).clone().requires_grad_(True) for t in (xz[:, :C].reshape(B, L, C), w))
        (T.conv_silu(x, w_, torch.zeros(C, dtype=dtype), bool(reverse)) * dy.view(B, L, C).to(dtype)).sum().backward()
        return {"dx": x.grad.reshape(M, C).numpy().astype(np.float64), "dw": w_.grad.numpy().astype(np.float64)}

    P = _lib.ptr
    dyd, xzd, wd = dy.to(DEV), xz.to(DEV), w.to(DEV)
    dxz, dw = torch.full((M, 2 * C), float("nan"), device=DEV), torch.full((C, K), float("nan"), device=DEV)
    ws = torch.empty(_lib.call("amt_dwconv1d_silu_bwd_ws_floats", B, L, C, K), device=DEV)
    _lib.call("amt_dwconv1d_silu_bwd", P(dyd), C, P(xzd), 2 * C, P(wd), None, P(dxz), 2 * C, P(dw), None, P(ws), B, L, C, K, reverse,
              _lib.stream_ptr())
    assert torch.isnan(dxz[:, C:]).all()
    got = {"dx": dxz[:, :C], "dw": dw}
    g64, g32 = autograd(torch.float64), autograd(torch.float32)
    report = []
    for k, want in g64.items():
        bound = max(8 * err(g32[k], want), (K if k == "dx" else M) * T.U)
        e = err(got[k].cpu().numpy(), want)
        report.append(f"{k} {e:.2e}/{bound:.2e}")
        assert e <= bound, (k, e, bound)
    print(shape, "K", K, "reverse", reverse, "no bias", " ".join(report))
    with pytest.raises(_lib.AmtError, match="go together"):
        _lib.call("amt_dwconv1d_silu_bwd", P(dyd), C, P(xzd), 2 * C, P(wd), P(wd), P(dxz), 2 * C, P(dw), None, P(ws), B, L, C, K, reverse, None)


def test_refusals():
    P = _lib.ptr
    t = torch.zeros(64, 64, device=DEV)
    with pytest.raises(_lib.AmtError, match="16 states"):                  # a wide-state scan: inference only
        _lib.call("amt_selective_scan_train_fwd", P(t), 16, P(t), 16, P(t), P(t), P(t), P(t), 64, P(t), P(t), 16, P(t), 16, P(t), 16, P(t),
                  1, 4, 16, 32, 1, 0, None)
    with pytest.raises(_lib.AmtError, match="16 states"):
        _lib.call("amt_selective_scan_bwd", *([P(t), 16] * 3), P(t), P(t), P(t), P(t), 64, P(t), P(t), 16, P(t), 16, P(t), P(t), 16, P(t), 16,
                  P(t), 16, P(t), P(t), 64, P(t), P(t), P(t), 1, 4, 16, 32, 1, 0, None)
    with pytest.raises(_lib.AmtError, match="leading dimension"):
        _lib.call("amt_selective_scan_bwd", *([P(t), 8] * 3), P(t), P(t), P(t), P(t), 64, P(t), P(t), 16, P(t), 16, P(t), P(t), 16, P(t), 16,
                  P(t), 16, P(t), P(t), 64, P(t), P(t), P(t), 1, 4, 16, 16, 1, 0, None)
    with pytest.raises(_lib.AmtError, match="null"):
        _lib.call("amt_selective_scan_bwd", *([None, 16] * 3), P(t), P(t), P(t), P(t), 64, P(t), P(t), 16, P(t), 16, P(t), P(t), 16, P(t), 16,
                  P(t), 16, P(t), P(t), 64, P(t), P(t), P(t), 1, 4, 16, 16, 1, 0, None)
    with pytest.raises(_lib.AmtError, match="at most 8"):
        _lib.call("amt_dwconv1d_silu_bwd", P(t), 16, P(t), 16, P(t), P(t), P(t), 16, P(t), P(t), P(t), 1, 4, 16, 9, 0, None)
    with pytest.raises(_lib.AmtError, match="bad shape"):
        _lib.call("amt_dwconv1d_silu_bwd", P(t), 16, P(t), 8, P(t), P(t), P(t), 16, P(t), P(t), P(t), 1, 4, 16, 4, 0, None)
    assert _lib.call("amt_selective_scan_bwd_ws_floats", 2, 33, 24, 16) == 2 * 2 * 33 * 32 + 2 * 24 * 17
    assert _lib.call("amt_dwconv1d_silu_bwd_ws_floats", 2, 33, 24, 4) == 66 * 24 + 2 * 24 * 5
