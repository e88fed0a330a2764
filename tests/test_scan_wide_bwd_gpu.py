"""amt_selective_scan_wide_train_fwd / amt_selective_scan_wide_bwd (csrc/mamba.hip, csrc/mamba_bwd.hip) alone, at N = 32 / 64 / 128 /
256 states per channel, against torch's CPU autograd in fp64 on `helpers_reg_mamba_train.scan_gate` (the plain sequential recurrence).

The cases are tests/test_mamba_bwd_gpu.py's at the new widths: A_log = log(1..N) + noise (the upper states' exp underflows, as at the
reference's initialisation), one draw past softplus's threshold.  Bound, the project's own: for every gradient
rel_err(got, g64) <= max(8 e32, n U), e32 torch's fp32 CPU autograd of the same restatement against the same fp64, n the longest sum
behind a value (B L for a parameter's gradient, L N for a value at the end of a state chain), U = 2^-24.

y_pre and the checkpoints are held to the fp64 recurrence at 4 (L + N) U of the largest value: per step the state takes one rounded
product-sum and a fast exp whose argument's rounding weighs a |x| <= 1 / e, each a few U of the largest state and damped by a < 1
afterwards, so at most ~4 U per step accumulate along a chain of L steps; y_pre adds a sum of N products."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers_reg_mamba_train as T
from video2music_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS = [32, 64, 128, 256]
# (B, L, ED): one step; one short chunk and a half-empty second block; a chunk boundary + 1; three chunks and a channel tail
SHAPES = [(1, 1, 16), (2, 31, 24), (2, 33, 64), (1, 70, 40)]


def err(got, want):
    """T.rel_err; where the gradient is exactly zero (dA_log of a one-step sequence) the kernel's must be too."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if not np.abs(want).max():
        return float(np.abs(got).max())
    return T.rel_err(got, want)


def scan_case(B, L, ED, N, seed):
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


def scan_autograd(c, B, L, ED, N, version, reverse, dtype):
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


def states64(c, B, L, ED, N, reverse, I):
    """-> y_pre (B*L, ED) at the original positions and the state at the start of every I-step chunk in walking order
    (B, ceil(L / I), ED, N), of the fp64 recurrence."""
    R = c["R"]
    d = lambda t: t.double()
    x, draw = d(c["xc"]).view(B, L, ED), d(c["draw"]).view(B, L, ED)
    Bm, Cm = d(c["dbc"][:, R:R + N]).reshape(B, L, N), d(c["dbc"][:, R + N:R + 2 * N]).reshape(B, L, N)
    delta, A = F.softplus(draw + d(c["dt_bias"])), -torch.exp(d(c["A_log"]))
    h = torch.zeros(B, ED, N, dtype=torch.float64)
    y_pre, cks = torch.zeros(B, L, ED, dtype=torch.float64), []
    for s in range(L):
        t = L - 1 - s if reverse else s
        if s % I == 0:
            cks.append(h.clone())
        h = torch.exp(delta[:, t, :, None] * A) * h + (delta[:, t, :, None] * Bm[:, t, None, :]) * x[:, t, :, None]
        y_pre[:, t] = (h * Cm[:, t, None, :]).sum(-1) + d(c["D"]) * x[:, t]
    return y_pre.view(B * L, ED).numpy(), torch.stack(cks, dim=1).numpy()


@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("N", WIDTHS)
def test_wide_scan_backward(N, shape, reverse, version):
    B, L, ED = shape
    c = scan_case(B, L, ED, N, seed=B * 1000 + L)
    R, M = c["R"], B * L
    d = {k: v.to(DEV) for k, v in c.items() if k != "R"}
    fwd = (d["xc"], d["draw"], d["dt_bias"], d["A_log"], d["dbc"], R, d["D"], d["xz"], B, L)
    I = ops.scan_ckpt_steps(N)
    assert I == _lib.call("amt_selective_scan_wide_ckpt_steps", N) == 32 and I % 16 == 0     # SHAPES straddle 32: L = 31, 33
    y_eval = ops.selective_scan(*fwd, version=version, reverse=reverse)
    y, y_pre, h_chunks = ops.selective_scan_train(*fwd, version=version, reverse=reverse)
    assert torch.equal(y, y_eval)                                           # the training forward: the same bits
    assert h_chunks.shape == (B, (L + I - 1) // I, ED, N) and not h_chunks[:, 0].any()
    yp64, ck64 = states64(c, B, L, ED, N, reverse, I)
    e_yp, e_ck = err(y_pre.cpu().numpy(), yp64), err(h_chunks.cpu().numpy(), ck64)
    print(shape, "N", N, f"y_pre {e_yp:.2e} checkpoints {e_ck:.2e} / {4 * (L + N) * T.U:.2e}")
    assert e_yp <= 4 * (L + N) * T.U and e_ck <= 4 * (L + N) * T.U

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
    g64, g32 = (scan_autograd(c, B, L, ED, N, version, reverse, dt) for dt in (torch.float64, torch.float32))
    if L == 1:
        assert not g64["dA_log"].any() and not got["dA_log"].any()          # no earlier state: exactly zero
    report, bad = [], []
    for k, want in g64.items():
        n = B * L if k in ("dA_log", "dD", "d_dt_bias") else L * N
        bound = max(8 * err(g32[k], want), n * T.U)
        e = err(got[k].cpu().numpy(), want)
        report.append(f"{k} {e:.2e}/{bound:.2e}")
        if not e <= bound:
            bad.append(k)
    print(shape, "N", N, "reverse", reverse, "version", version, " ".join(report))
    assert not bad, (bad, report)


def test_refusals():
    P = _lib.ptr
    t = torch.zeros(64, 600, device=DEV)

    def fwd(N, ld_bc=512, x=t):
        _lib.call("amt_selective_scan_wide_train_fwd", P(x), 16, P(t), 16, P(t), P(t), P(t), P(t), ld_bc, P(t), P(t), 16, P(t), 16, P(t), 16, P(t),
                  1, 4, 16, N, 1, 0, None)

    def bwd(N, ld=16, dout=t):
        _lib.call("amt_selective_scan_wide_bwd", P(dout), ld, P(t), ld, P(t), ld, P(t), P(t), P(t), P(t), 512, P(t), P(t), 16, P(t), 16, P(t),
                  P(t), 16, P(t), 16, P(t), 16, P(t), P(t), 512, P(t), P(t), P(t), 1, 4, 16, N, 1, 0, None)

    for call in (fwd, bwd):
        with pytest.raises(_lib.AmtError, match="amt_selective_scan_train_fwd"):     # 16 states: the existing calls
            call(16)
        with pytest.raises(_lib.AmtError, match="d_state=48"):
            call(48)
    with pytest.raises(_lib.AmtError, match="leading dimension"):
        fwd(64, ld_bc=32)
    with pytest.raises(_lib.AmtError, match="leading dimension"):
        bwd(64, ld=8)
    with pytest.raises(_lib.AmtError, match="null"):
        fwd(64, x=None)
    with pytest.raises(_lib.AmtError, match="null"):
        bwd(64, dout=None)
    assert _lib.call("amt_selective_scan_wide_ckpt_steps", 16) == 0 and _lib.call("amt_selective_scan_wide_ckpt_steps", 48) == 0
    with pytest.raises(ValueError, match="states per channel"):
        ops.scan_ckpt_steps(48)
    # (B, L, ED, N) = (2, 33, 24, 64): 2 channel blocks x dB | dC (2 * 33 rows x 128), dA + dD per clip, 4 slices x 2 partials (66 x 24)
    assert _lib.call("amt_selective_scan_wide_bwd_ws_floats", 2, 33, 24, 64) == 2 * 2 * 33 * 128 + 2 * 24 * 65 + 2 * 4 * 66 * 24
    assert _lib.call("amt_selective_scan_wide_bwd_ws_floats", 2, 33, 24, 16) == 0
