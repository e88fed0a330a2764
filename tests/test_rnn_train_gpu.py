"""One recurrent layer through `autograd.RnnLayerFn` (amt_rnn_seq_train_fwd + amt_rnn_seq_bwd + the GEMMs around them) against
torch's CPU autograd on nn.LSTM / nn.GRU in fp64: the gradients of x, weight_ih, bias_ih, weight_hh, bias_hh of each direction.

Bound per tensor, err = max|g - g64| / max|g64|:   err <= max(8 err_torch32, (B L + G d) 2^-24)
err_torch32 is the same measure for torch's own fp32 CPU autograd on the same inputs (the reference's arithmetic, computed here).
The factor 8 covers another summation order over the B L rows and the device's __expf / tanhf, a few ulps wide, against CPU
functions rounded to under one; the second term is the longest sum's length times the unit roundoff, for the cases where torch's
own error happens to be near zero."""
import numpy as np
import pytest
import torch

from tests.helpers_numeric_range import rnn_torch_cpu as torch_cpu      # nn.LSTM / nn.GRU on the CPU, shared with the range tests
from tests.helpers_reg_train import U, rel_err
from video2music_amd import _lib, ops
from video2music_amd.autograd import RnnLayerFn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("weight_ih", "bias_ih", "weight_hh", "bias_hh")
CASES = [(G, n, d, B, L) for G in (4, 3) for n in (1, 2) for d in (8, 24, 64, 128) for (B, L) in ((1, 1), (1, 2), (3, 5), (2, 37))]


def inputs(G, n_dirs, d, B, L, seed=None):
    """Weights uniform in +-1/sqrt(d) (torch's own initialisation), x and dy standard normal; the layer's input width is d."""
    rng = np.random.default_rng(1000 * G + 100 * n_dirs + 7 * d + 31 * B + L if seed is None else seed)
    k = 1.0 / np.sqrt(d)
    par = {}
    for sfx in ("", "_reverse")[:n_dirs]:
        for nm in NAMES:
            shape = (G * d, d) if nm.startswith("weight") else (G * d,)
            par[nm + "_l0" + sfx] = rng.uniform(-k, k, shape).astype(np.float32)
    return par, rng.standard_normal((B, L, d)).astype(np.float32), rng.standard_normal((B, L, n_dirs * d)).astype(np.float32)


def device(G, n_dirs, d, par, x, dy, reverse=False):
    B, L = x.shape[:2]
    ps = [torch.from_numpy(par[nm + "_l0" + sfx]).to(DEV).requires_grad_(True) for sfx in ("", "_reverse")[:n_dirs] for nm in NAMES]
    stacked = tuple(torch.cat([ps[4 * r + k].detach() for r in range(n_dirs)]).contiguous() for k in range(4))
    xt = torch.from_numpy(x).to(DEV).view(B * L, d).requires_grad_(True)
    y = RnnLayerFn.apply(xt, B, L, G, reverse, stacked, *ps)
    y.backward(torch.from_numpy(dy).to(DEV).view(B * L, n_dirs * d))
    torch.cuda.synchronize()
    out = {"y": y.detach().cpu().numpy().reshape(B, L, -1), "x": xt.grad.cpu().numpy().reshape(B, L, d)}
    out.update({k: p.grad.cpu().numpy() for k, p in zip(par, ps)})
    return out


def check(G, n_dirs, d, B, L, reverse=False, tag=""):
    par, x, dy = inputs(G, n_dirs, d, B, L)
    g64 = torch_cpu(G, n_dirs, d, par, x, dy, torch.float64, reverse)
    g32 = torch_cpu(G, n_dirs, d, par, x, dy, torch.float32, reverse)
    got = device(G, n_dirs, d, par, x, dy, reverse)
    assert np.abs(got["y"] - g64["y"]).max() <= 64 * U                  # the forward itself: |h| < 1
    worst = 0.0
    for k in g64:
        if k == "y":
            continue
        if np.abs(g64[k]).max() == 0.0:                                 # L = 1: no recurrent term
            assert k.startswith("weight_hh") and L == 1
            assert not got[k].any(), k
            continue
        err, e32 = rel_err(got[k], g64[k]), rel_err(g32[k], g64[k])
        bound = max(8 * e32, (B * L + G * d) * U)
        worst = max(worst, err / max(e32, U))
        assert err <= bound, (tag, k, err, e32, bound)
    print(f"G {G} dirs {n_dirs} d {d} B {B} L {L}{tag}: worst err / max(err_torch32, 2^-24) = {worst:.2f}")
    return worst


@pytest.mark.parametrize("G,n_dirs,d,B,L", CASES)
def test_gradients_vs_torch_fp64(G, n_dirs, d, B, L):
    check(G, n_dirs, d, B, L)


@pytest.mark.parametrize("G", (4, 3))
def test_single_reversed_direction(G):
    check(G, 1, 24, 3, 5, reverse=True, tag=" reversed")
    check(G, 1, 64, 2, 37, reverse=True, tag=" reversed")


@pytest.mark.parametrize("G", (4, 3))
def test_gradients_are_bit_identical_across_calls(G):
    par, x, dy = inputs(G, 2, 64, 3, 37)
    a, b = device(G, 2, 64, par, x, dy), device(G, 2, 64, par, x, dy)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def raw(G, n_dirs, d, B, L, pad, reverse=False):
    """The two recurrence kernels called directly, every matrix with `pad` extra columns per row set to 1e4."""
    rng = np.random.default_rng(5)
    M, R, C = B * L, G * d, ops.rnn_reserve_cols(G)
    def mat(cols, fill=None):
        t = torch.full((M, cols + pad), 1.0e4, device=DEV)
        t[:, :cols] = torch.from_numpy(rng.standard_normal((M, cols)).astype(np.float32)).to(DEV) if fill is None else fill
        return t
    xp, dyv = mat(n_dirs * R), mat(n_dirs * d)
    y, rsv, dxp, dhn = mat(n_dirs * d, -7.0), mat(n_dirs * C * d, -7.0), mat(n_dirs * R, -7.0), mat(n_dirs * d, -7.0)
    wh = torch.from_numpy(rng.uniform(-0.2, 0.2, (n_dirs * R, d)).astype(np.float32)).to(DEV)
    bh = torch.from_numpy(rng.uniform(-0.2, 0.2, (n_dirs * R,)).astype(np.float32)).to(DEV)
    ops.rnn_seq_train(xp, wh, bh, y, 0, rsv, B, L, d, G, reverse=reverse, n_dirs=n_dirs)
    y_eval = torch.full_like(y, 1.0e4)
    ops.rnn_seq(xp, wh, bh, y_eval, 0, B, L, d, G, reverse=reverse, n_dirs=n_dirs)
    ops.rnn_seq_bwd(dyv, 0, rsv, y, 0, wh, dxp, dhn if G == 3 else None, B, L, d, G, reverse=reverse, n_dirs=n_dirs)
    torch.cuda.synchronize()
    outs = {"y": (y, n_dirs * d), "rsv": (rsv, n_dirs * C * d), "dxp": (dxp, n_dirs * R), "y_eval": (y_eval, n_dirs * d)}
    if G == 3:
        outs["dhn"] = (dhn, n_dirs * d)
    for k, (t, cols) in outs.items():
        if pad:
            assert (t[:, cols:] == 1.0e4).all(), k + ": padding columns were written"
    return {k: t[:, :cols].cpu().numpy() for k, (t, cols) in outs.items()}


@pytest.mark.parametrize("G,n_dirs,reverse", [(4, 2, False), (3, 2, False), (4, 1, True), (3, 1, True)])
def test_padded_leading_dimensions_and_train_forward_equals_eval_forward(G, n_dirs, reverse):
    """Poisoned padding columns are neither read (the results equal the unpadded call's, bit for bit) nor written; the training
    forward's y is the inference kernel's, bit for bit."""
    a, b = raw(G, n_dirs, 24, 3, 5, 0, reverse), raw(G, n_dirs, 24, 3, 5, 12, reverse)
    for k in a:
        assert np.isfinite(a[k]).all() and np.abs(a[k]).max() < 1.0e3, k
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["y"], a["y_eval"])


def test_bad_arguments_are_refused_before_any_launch():
    t = torch.zeros(4, 4 * 5 * 136, device=DEV)
    w = torch.zeros(4 * 136, 136, device=DEV)
    for d, gates, msg in ((136, 4, "hidden size"), (12, 4, "hidden size"), (8, 5, "gates=5")):
        with pytest.raises(_lib.AmtError, match=msg):
            ops.rnn_seq_bwd(t, 0, t, t, 0, w, t, t, 1, 4, d, gates)
        with pytest.raises(_lib.AmtError, match=msg):
            ops.rnn_seq_train(t, w, w, t, 0, t, 1, 4, d, gates)
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_rnn_seq_bwd", None, 8, _lib.ptr(t), 40, _lib.ptr(t), 8, _lib.ptr(w), _lib.ptr(t), 32, None, 0, 1, 4, 8, 4, 0, 1, None)
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_rnn_seq_train_fwd", _lib.ptr(t), 32, _lib.ptr(w), _lib.ptr(w), _lib.ptr(t), 8, None, 40, 1, 4, 8, 4, 0, 1, None)
    with pytest.raises(_lib.AmtError, match="GRU needs dhn"):
        _lib.call("amt_rnn_seq_bwd", _lib.ptr(t), 8, _lib.ptr(t), 32, _lib.ptr(t), 8, _lib.ptr(w), _lib.ptr(t), 24, None, 0, 1, 4, 8, 3, 0, 1, None)
    with pytest.raises(_lib.AmtError, match="leading dimensions"):
        _lib.call("amt_rnn_seq_bwd", _lib.ptr(t), 8, _lib.ptr(t), 39, _lib.ptr(t), 8, _lib.ptr(w), _lib.ptr(t), 32, None, 0, 1, 4, 8, 4, 0, 1, None)
    torch.cuda.synchronize()
