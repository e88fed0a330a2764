"""The wide recurrence kernels (csrc/rnn_wide.hip: amt_rnn_wide_seq_fwd / _train_fwd / _bwd, one MFMA step launch per time step) through
`autograd.RnnLayerFn` and directly, against torch's CPU nn.LSTM / nn.GRU in fp64.

RnnLayerFn takes the wide pair above `ops.RNN_NARROW_MAX`; the cases at d <= 128 (the overlap with the register kernels of csrc/rnn.hip)
lower that switch to 0 for the call, so that every case here runs the wide kernels.

Gradients, per tensor, err = max|g - g64| / max|g64| (the bound of tests/test_rnn_train_gpu.py):   err <= max(8 err_torch32, (B L + G d) 2^-24)
Forward:   max|y - y64| <= max(8 e32_fwd, 64 2^-24),   e32_fwd = max|y32 - y64| of torch's own fp32 CPU forward on the same inputs: the flat
64 2^-24 of the register kernels' test was set for dot products of length <= 128, the measured term lets a length-512 sum in.
Overlap at d = 128, both kernel families on the same projected inputs: y and every reserve block within twice the forward bound of each
other (the gates and n are bounded by 1; the LSTM's c and the GRU's W_hn h + b_hn block are held relative to their largest value),
every dxproj block and dhn within the gradient bound, the measured terms from torch's nn.LSTM / nn.GRU fed the same projected inputs."""
import contextlib

import numpy as np
import pytest
import torch

from tests.helpers_numeric_range import rnn_torch_cpu as torch_cpu
from tests.helpers_reg_train import U, rel_err
from tests.test_rnn_train_gpu import NAMES, inputs
from video2music_amd import _lib, ops
from video2music_amd.autograd import RnnLayerFn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(32, 3, 5), (128, 3, 5), (128, 2, 37), (160, 1, 1), (160, 1, 2), (160, 3, 5), (160, 33, 3), (256, 3, 5), (256, 2, 37), (512, 3, 5),
          (512, 33, 3)]
CASES = [(G, n, d, B, L) for G in (4, 3) for n in (1, 2) for (d, B, L) in SHAPES]


@contextlib.contextmanager
def wide_at_every_width():
    """RnnLayerFn reads the switch at call time: 0 sends every width to the wide pair."""
    old, ops.RNN_NARROW_MAX = ops.RNN_NARROW_MAX, 0
    try:
        yield
    finally:
        ops.RNN_NARROW_MAX = old


def device(G, n_dirs, d, par, x, dy, reverse=False):
    B, L = x.shape[:2]
    ps = [torch.from_numpy(par[nm + "_l0" + sfx]).to(DEV).requires_grad_(True) for sfx in ("", "_reverse")[:n_dirs] for nm in NAMES]
    stacked = tuple(torch.cat([ps[4 * r + k].detach() for r in range(n_dirs)]).contiguous() for k in range(4))
    xt = torch.from_numpy(x).to(DEV).view(B * L, d).requires_grad_(True)
    with wide_at_every_width():
        y = RnnLayerFn.apply(xt, B, L, G, reverse, stacked, *ps)
        y.backward(torch.from_numpy(dy).to(DEV).view(B * L, n_dirs * d))
    torch.cuda.synchronize()
    out = {"y": y.detach().cpu().numpy().reshape(B, L, -1), "x": xt.grad.cpu().numpy().reshape(B, L, d)}
    out.update({k: p.grad.cpu().numpy() for k, p in zip(par, ps)})
    return out


def fwd_bound(e32_fwd):
    return max(8 * e32_fwd, 64 * U)


def check(G, n_dirs, d, B, L, reverse=False, tag=""):
    par, x, dy = inputs(G, n_dirs, d, B, L)
    g64 = torch_cpu(G, n_dirs, d, par, x, dy, torch.float64, reverse)
    g32 = torch_cpu(G, n_dirs, d, par, x, dy, torch.float32, reverse)
    got = device(G, n_dirs, d, par, x, dy, reverse)
    ef, e32f = np.abs(got["y"] - g64["y"]).max(), np.abs(g32["y"] - g64["y"]).max()
    worst = 0.0
    fails = []
    if not ef <= fwd_bound(e32f):
        fails.append(("y", ef, e32f, fwd_bound(e32f)))
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
        if not err <= bound:
            fails.append((k, err, e32, bound))
    print(f"G {G} dirs {n_dirs} d {d} B {B} L {L}{tag}: forward err / max(e32_fwd, 2^-24) = {ef / max(e32f, U):.2f}, "
          f"worst gradient err / max(err_torch32, 2^-24) = {worst:.2f}")
    assert not fails, (tag, fails)


@pytest.mark.parametrize("G,n_dirs,d,B,L", CASES)
def test_forward_and_gradients_vs_torch_fp64(G, n_dirs, d, B, L):
    check(G, n_dirs, d, B, L)


@pytest.mark.parametrize("G", (4, 3))
def test_single_reversed_direction(G):
    check(G, 1, 160, 3, 5, reverse=True, tag=" reversed")


@pytest.mark.parametrize("G", (4, 3))
def test_bit_repeatability(G):
    par, x, dy = inputs(G, 2, 160, 3, 5)
    a, b = device(G, 2, 160, par, x, dy), device(G, 2, 160, par, x, dy)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    r1, r2 = raw(G, 2, 160, 33, 3, 0), raw(G, 2, 160, 33, 3, 0)
    for k in r1:
        assert np.array_equal(r1[k], r2[k]), k


def raw_inputs(G, n_dirs, d, B, L):
    """-> xproj (B, L, n_dirs G d), w_hh (n_dirs, G d, d), b_hh (n_dirs, G d), dy (B, L, n_dirs d): the kernels' own inputs, weights as
    torch initialises them."""
    rng = np.random.default_rng(5)
    k = 1.0 / np.sqrt(d)
    return (rng.standard_normal((B, L, n_dirs * G * d)).astype(np.float32), rng.uniform(-k, k, (n_dirs, G * d, d)).astype(np.float32),
            rng.uniform(-k, k, (n_dirs, G * d)).astype(np.float32), rng.standard_normal((B, L, n_dirs * d)).astype(np.float32))


def raw(G, n_dirs, d, B, L, pad, reverse=False, narrow=False):
    """The three kernels called directly (narrow: the register kernels of csrc/rnn.hip on the same inputs), every matrix with `pad`
    extra columns per row set to 1e4."""
    M, R, C = B * L, G * d, ops.rnn_reserve_cols(G)
    xproj, w_hh, b_hh, dy = raw_inputs(G, n_dirs, d, B, L)

    def mat(cols, fill):
        t = torch.full((M, cols + pad), 1.0e4, device=DEV)
        t[:, :cols] = torch.from_numpy(fill.reshape(M, cols)).to(DEV) if isinstance(fill, np.ndarray) else fill
        return t

    xp, dyv = mat(n_dirs * R, xproj), mat(n_dirs * d, dy)
    y, rsv, dxp, dhn = mat(n_dirs * d, -7.0), mat(n_dirs * C * d, -7.0), mat(n_dirs * R, -7.0), mat(n_dirs * d, -7.0)
    wh, bh = torch.from_numpy(w_hh.reshape(n_dirs * R, d)).to(DEV), torch.from_numpy(b_hh.reshape(n_dirs * R)).to(DEV)
    train, fwd, bwd = (ops.rnn_seq_train, ops.rnn_seq, ops.rnn_seq_bwd) if narrow else (ops.rnn_wide_seq_train, ops.rnn_wide_seq, ops.rnn_wide_seq_bwd)
    train(xp, wh, bh, y, 0, rsv, B, L, d, G, reverse=reverse, n_dirs=n_dirs)
    y_eval = torch.full_like(y, 1.0e4)
    fwd(xp, wh, bh, y_eval, 0, B, L, d, G, reverse=reverse, n_dirs=n_dirs)
    bwd(dyv, 0, rsv, y, 0, wh, dxp, dhn if G == 3 else None, B, L, d, G, reverse=reverse, n_dirs=n_dirs)
    torch.cuda.synchronize()
    outs = {"y": (y, n_dirs * d), "rsv": (rsv, n_dirs * C * d), "dxp": (dxp, n_dirs * R), "y_eval": (y_eval, n_dirs * d)}
    if G == 3:
        outs["dhn"] = (dhn, n_dirs * d)
    for key, (t, cols) in outs.items():
        if pad:
            assert (t[:, cols:] == 1.0e4).all(), key + ": padding columns were written"
    return {key: t[:, :cols].cpu().numpy() for key, (t, cols) in outs.items()}


@pytest.mark.parametrize("G,n_dirs,reverse", [(4, 2, False), (3, 2, False), (4, 1, True), (3, 1, True)])
def test_padded_leading_dimensions_and_train_forward_equals_eval_forward(G, n_dirs, reverse):
    """Poisoned padding columns are neither read (bit-equal to the unpadded call) nor written; the training forward's y is the eval
    forward's, bit for bit.  33 clips: a second, nearly empty tile."""
    for d, B, L in ((160, 3, 5), (160, 33, 3)):
        a, b = raw(G, n_dirs, d, B, L, 0, reverse), raw(G, n_dirs, d, B, L, 12, reverse)
        for k in a:
            assert np.isfinite(a[k]).all() and np.abs(a[k]).max() < 1.0e3, k
            assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a["y"], a["y_eval"])


@pytest.mark.parametrize("G,n_dirs", [(4, 2), (3, 2), (4, 1), (3, 1)])
@pytest.mark.parametrize("B,L", [(3, 5), (2, 37)])
def test_overlap_with_the_register_kernels_block_by_block(G, n_dirs, B, L):
    """d = 128, both families on the same inputs: the shared layout of y, reserve, dxproj and dhn.  The bounds' measured terms come from
    torch's nn.LSTM / nn.GRU fed the same projected inputs (helpers_numeric_range.rnn_run), fp32 against fp64."""
    from tests.helpers_numeric_range import rnn_run
    d, C, R = 128, ops.rnn_reserve_cols(G), G * 128
    w, n = raw(G, n_dirs, d, B, L, 0), raw(G, n_dirs, d, B, L, 0, narrow=True)
    a = raw_inputs(G, n_dirs, d, B, L)
    r64, r32 = rnn_run(G, n_dirs, d, *a, torch.float64), rnn_run(G, n_dirs, d, *a, torch.float32)
    fb = 2 * fwd_bound(np.abs(r32["y"] - r64["y"]).max())
    gb = max(8 * rel_err(r32["dxproj"], r64["dxproj"]), (B * L + G * d) * U)
    print(f"G {G} dirs {n_dirs} B {B} L {L}: forward bound x 2 = {fb:.3e}, gradient bound = {gb:.3e}")
    for v in (w, n):                                        # both families stand where the reference stands
        assert np.abs(v["y"] - r64["y"]).max() <= fb / 2 and rel_err(v["dxp"], r64["dxproj"]) <= gb
    assert np.abs(w["y"] - n["y"]).max() <= fb
    for r in range(n_dirs):
        for c in range(C):
            x, y = (v["rsv"][:, (r * C + c) * d:(r * C + c + 1) * d] for v in (w, n))
            scale = max(1.0, np.abs(y).max())               # gates and n are bounded by 1; the LSTM's c and the GRU's W_hn h + b_hn are held
            assert np.abs(x - y).max() <= fb * scale, ("reserve", r, c)                    # relative to their largest value
        for g in range(G):
            x, y = (v["dxp"][:, r * R + g * d:r * R + (g + 1) * d] for v in (w, n))
            assert rel_err(x, y) <= gb, ("dxproj", r, g)
        if G == 3:
            x, y = (v["dhn"][:, r * d:(r + 1) * d] for v in (w, n))
            assert rel_err(x, y) <= gb, ("dhn", r)


def test_bad_arguments_are_refused_before_any_launch():
    t = torch.zeros(4, 4 * 5 * 544, device=DEV)
    w = torch.zeros(4 * 544, 544, device=DEV)
    for d, gates, msg in ((136, 4, "hidden size 136 must be a multiple of 32"), (544, 4, "hidden size 544"), (16, 3, "hidden size 16"), (160, 5, "gates=5")):
        with pytest.raises(_lib.AmtError, match=msg):
            ops.rnn_wide_seq_bwd(t, 0, t, t, 0, w, t, t, 1, 4, d, gates)
        with pytest.raises(_lib.AmtError, match=msg):
            ops.rnn_wide_seq_train(t, w, w, t, 0, t, 1, 4, d, gates)
        with pytest.raises(_lib.AmtError, match=msg):
            ops.rnn_wide_seq(t, w, w, t, 0, 1, 4, d, gates)
        with pytest.raises(_lib.AmtError, match=msg):
            _lib.call("amt_rnn_wide_seq_fwd", _lib.ptr(t), 4 * 544, _lib.ptr(w), _lib.ptr(w), _lib.ptr(t), 544, 1, 4, d, gates, 0, 1, _lib.ptr(t), None)
    assert _lib.call("amt_rnn_wide_ws_floats", 33, 160, 3, 2) == 33 * 2 * 160 and _lib.call("amt_rnn_wide_ws_floats", 33, 136, 3, 2) == -1
    P = _lib.ptr
    with pytest.raises(_lib.AmtError, match="amt_rnn_wide_seq_bwd: null pointer"):
        _lib.call("amt_rnn_wide_seq_bwd", None, 32, P(t), 160, P(t), 32, P(w), P(t), 128, None, 0, 1, 4, 32, 4, 0, 1, P(t), None)
    with pytest.raises(_lib.AmtError, match="amt_rnn_wide_seq_bwd: null pointer"):          # the workspace
        _lib.call("amt_rnn_wide_seq_bwd", P(t), 32, P(t), 160, P(t), 32, P(w), P(t), 128, None, 0, 1, 4, 32, 4, 0, 1, None, None)
    with pytest.raises(_lib.AmtError, match="amt_rnn_wide_seq_train_fwd: null pointer"):
        _lib.call("amt_rnn_wide_seq_train_fwd", P(t), 128, P(w), P(w), P(t), 32, None, 160, 1, 4, 32, 4, 0, 1, P(t), None)
    with pytest.raises(_lib.AmtError, match="amt_rnn_wide_seq_fwd: null pointer"):
        _lib.call("amt_rnn_wide_seq_fwd", P(t), 128, None, P(w), P(t), 32, 1, 4, 32, 4, 0, 1, P(t), None)
    with pytest.raises(_lib.AmtError, match="GRU needs dhn"):
        _lib.call("amt_rnn_wide_seq_bwd", P(t), 32, P(t), 128, P(t), 32, P(w), P(t), 96, None, 0, 1, 4, 32, 3, 0, 1, P(t), None)
    with pytest.raises(_lib.AmtError, match="leading dimensions .*ldr=159"):
        _lib.call("amt_rnn_wide_seq_bwd", P(t), 32, P(t), 159, P(t), 32, P(w), P(t), 128, None, 0, 1, 4, 32, 4, 0, 1, P(t), None)
    with pytest.raises(_lib.AmtError, match="leading dimensions .*ldy=63"):                # two directions need 64
        _lib.call("amt_rnn_wide_seq_fwd", P(t), 256, P(w), P(w), P(t), 63, 1, 4, 32, 4, 0, 2, P(t), None)
    with pytest.raises(_lib.AmtError, match="float4"):                                     # wide enough, rows not 16-byte
        _lib.call("amt_rnn_wide_seq_fwd", P(t), 128, P(w), P(w), P(t), 34, 1, 4, 32, 4, 0, 1, P(t), None)
    torch.cuda.synchronize()
