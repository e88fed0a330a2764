"""amt_attn_train_fwd / amt_attn_bwd (csrc/attn_prefill.hip TRAIN instantiations, csrc/attn_bwd.hip) through `autograd.AttentionFn`
against torch's CPU autograd in fp64 on the written-out formula, with qs = q q_scale:

    S_ij = qs_i . k_j (+ qs_i . Er[er_len-1-(i-j)] for j <= i),  P = softmax_j(S) under the mask,  O = (P o keep keep_scale) V

Forward: O and lse within 3e-5 absolute of fp64, the bound tests/test_ops_gpu.py uses for the prefill kernel on unit-scale inputs.
Gradients, the bound of tests/test_rnn_train_gpu.py per tensor: err = max|g - g64| / max|g64| <= max(8 err_torch32, n 2^-24) with
err_torch32 torch's own fp32 CPU autograd on the same inputs and n the longest sum's length: Lk + hd for dq, kv_group Lq for dk / dv,
B H L for dEr.  A gradient that vanishes identically (a single key: dS = P (dP - D) = 0) is held to 8 n 2^-24 absolute: dP and D are the
same unit-scale sum of hd products in two orders.  Shapes: the smallest at which the tiling (query block 128, key tile 32, 32-key waves of the dk / dv pass) can go wrong."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers_numeric_range import attn_train_torch_cpu
from tests.helpers_reg_train import U, rel_err
from video2music_amd import _lib, ops
from video2music_amd.autograd import AttentionFn, blh_strides

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_DROP = 0.2

# (B, H, Lq, Lk, hd, causal, rpr, er_len, kv_group)
CASES = [(1, 1, 1, 1, 32, 1, r, 1, 1) for r in (0, 1)] + [(2, 2, 37, 37, 32, 1, r, 37, 1) for r in (0, 1)] + \
        [(1, 2, 129, 129, 64, 1, r, 129, 1) for r in (0, 1)] + [(1, 8, 300, 300, 64, 1, r, 300, 1) for r in (0, 1)] + \
        [(2, 2, 37, 37, 32, 1, 1, 300, 1),            # a table longer than the sequence
         (2, 2, 70, 70, 64, 0, 0, 0, 1),              # non-causal self-attention (the encoder)
         (2, 2, 33, 70, 64, 0, 0, 0, 1),              # cross-attention
         (1, 8, 299, 300, 64, 0, 0, 0, 1),            # cross-attention on the split-key kernel
         (2, 4, 37, 37, 32, 1, 0, 0, 2),              # two query heads per key head
         (1, 2, 37, 37, 128, 1, 1, 37, 1)]            # head_dim 128
CASES = [c + (m,) for c in CASES for m in (0, 1)]


def make(B, H, Lq, Lk, hd, causal, rpr, er_len, g, mask):
    rng = np.random.default_rng(B + 10 * H + 100 * Lq + 7 * Lk + hd + causal + rpr + er_len + g)
    a = {"q": rng.standard_normal((B, Lq, H * hd)), "k": rng.standard_normal((B, Lk, H // g * hd)),
         "v": rng.standard_normal((B, Lk, H // g * hd)), "dO": rng.standard_normal((B, Lq, H * hd))}
    if rpr:
        a["Er"] = rng.standard_normal((er_len, hd))
    a = {k: v.astype(np.float32) for k, v in a.items()}
    keep = None
    if mask:
        keep = (rng.random((B, H, Lq, Lk)) >= P_DROP).astype(np.uint8)
        keep[0, 0, Lq // 2, :] = 0                      # a fully dropped row
    return a, keep


def torch_cpu(a, keep, H, causal, g, dtype):
    return attn_train_torch_cpu(a, keep, H, causal, g, dtype, P_DROP)          # the written-out formula, shared with the range tests


def device(a, keep, H, causal, g):
    t = {k: torch.from_numpy(v).to(DEV).requires_grad_(k != "dO") for k, v in a.items()}
    kd = None if keep is None else torch.from_numpy(keep).to(DEV)
    hd = t["q"].shape[2] // H
    O = AttentionFn.apply(t["q"], t["k"], t["v"], t.get("Er"), kd, H, causal, hd ** -0.5, 1.0 / (1.0 - P_DROP), g)
    O.backward(t["dO"])
    torch.cuda.synchronize()
    out = {"O": O.detach().cpu().numpy()}
    out.update({k: t[k].grad.cpu().numpy() for k in t if k != "dO"})
    return out


def lse_on_device(a, keep, H, causal, g):
    t = {k: torch.from_numpy(v).to(DEV) for k, v in a.items()}
    B, Lq, E = t["q"].shape
    Lk, hd = t["k"].shape[1], E // H
    kd = None if keep is None else torch.from_numpy(keep).to(DEV)
    o, lse = ops.attention_train(t["q"], t["k"], t["v"], blh_strides(Lq, Lk, H, hd, g), B, H, Lq, Lk, hd, causal, hd ** -0.5,
                                 torch.empty_like(t["q"]), kv_group=g, Er=t.get("Er"), keep=kd, keep_scale=1.0 / (1.0 - P_DROP))
    return o, lse


def inference_output(a, H, causal, g):
    """The same shape through the inference entry points: amt_rpr_attn_fwd / amt_cross_attn_fwd, amt_attn_fwd for grouped heads."""
    t = {k: torch.from_numpy(v).to(DEV) for k, v in a.items()}
    B, Lq, E = t["q"].shape
    Lk, hd = t["k"].shape[1], E // H
    o = torch.empty_like(t["q"])
    P = _lib.ptr
    if "Er" in t:
        qs = (t["q"] * hd ** -0.5).contiguous()             # this entry point takes the scaled query; the product rounds the same way
        _lib.call("amt_rpr_attn_fwd", P(qs), P(t["k"]), P(t["v"]), P(t["Er"]), P(o), B, H, Lq, hd, t["Er"].shape[0], _lib.stream_ptr())
    elif g == 1:
        qs = (t["q"] * hd ** -0.5).contiguous()
        _lib.call("amt_cross_attn_fwd", P(qs), P(t["k"]), P(t["v"]), P(o), B, H, Lq, Lk, hd, int(causal), _lib.stream_ptr())
    else:
        s = (C.c_int64 * 12)(*blh_strides(Lq, Lk, H, hd, g))
        _lib.call("amt_attn_fwd", P(t["q"]), P(t["k"]), P(t["v"]), P(o), s, B, H, Lq, Lk, hd, int(causal), g, hd ** -0.5, _lib.stream_ptr())
    return o


@pytest.mark.parametrize("B,H,Lq,Lk,hd,causal,rpr,er_len,g,mask", CASES)
def test_forward_and_gradients_against_fp64(B, H, Lq, Lk, hd, causal, rpr, er_len, g, mask):
    a, keep = make(B, H, Lq, Lk, hd, causal, rpr, er_len, g, mask)
    w64, w32 = torch_cpu(a, keep, H, causal, g, torch.float64), torch_cpu(a, keep, H, causal, g, torch.float32)
    got, again = device(a, keep, H, causal, g), device(a, keep, H, causal, g)
    o, lse = lse_on_device(a, keep, H, causal, g)
    assert np.array_equal(o.cpu().numpy(), got["O"])
    for k in got:
        assert np.array_equal(got[k], again[k]), k                       # no atomics: equal bits on repeat
        assert np.isfinite(got[k]).all(), k
    assert np.abs(got["O"] - w64["O"]).max() <= 3e-5
    assert np.abs(lse.cpu().numpy() - w64["lse"]).max() <= 3e-5
    n = {"q": Lk + hd, "k": g * Lq, "v": g * Lq, "Er": B * H * Lq}
    for k in n:
        if k not in got:
            continue
        if np.abs(w64[k]).max() <= 1e-12:               # one key, or a dropped row alone: dS = P (dP - D) cancels to zero
            assert np.abs(got[k]).max() <= 8 * n[k] * U, k
            continue
        err, e32 = rel_err(got[k], w64[k]), rel_err(w32[k], w64[k])
        bound = max(8 * e32, n[k] * U)
        print(f"{(B, H, Lq, Lk, hd)} causal {causal} rpr {rpr} er_len {er_len} g {g} mask {mask} d{k}: err {err:.3e} torch32 {e32:.3e} bound {bound:.3e}")
        assert err <= bound, (k, err, e32, bound)
    if rpr:
        assert not got["Er"][:er_len - Lq].any()                         # rows no pair reaches: exact zeros
    if mask:
        assert not got["O"][0, Lq // 2, :hd].any()                       # the fully dropped row of head 0
    else:
        assert torch.equal(o, inference_output(a, H, causal, g))         # the inference kernels' bits


def test_padding_of_strided_buffers_is_neither_read_nor_written():
    """Head-major (B, H, cap, hd) buffers with cap > L: NaN in the rows past L of every input, a sentinel in those of every output."""
    B, H, L, hd, cap = 2, 2, 37, 32, 45
    a, keep = make(B, H, L, L, hd, 1, 1, L, 1, 1)
    ref = {k: torch.from_numpy(v).to(DEV) for k, v in a.items()}
    kd = torch.from_numpy(keep).to(DEV)
    strides = blh_strides(L, L, H, hd)
    o, lse = ops.attention_train(ref["q"], ref["k"], ref["v"], strides, B, H, L, L, hd, 1, hd ** -0.5, torch.empty_like(ref["q"]), Er=ref["Er"],
                                 keep=kd, keep_scale=1.25)
    dq, dk, dv = (torch.empty_like(ref["q"]) for _ in range(3))
    dEr = ops.attention_bwd(ref["dO"], ref["q"], ref["k"], ref["v"], o, lse, strides, B, H, L, L, hd, 1, hd ** -0.5, dq, dk, dv, Er=ref["Er"],
                            keep=kd, keep_scale=1.25)

    def padded(t, fill):
        buf = torch.full((B, H, cap, hd), fill, device=DEV)
        if t is not None:
            buf[:, :, :L] = t.view(B, L, H, hd).transpose(1, 2)
        return buf
    nan = float("nan")
    q, k, v, g = (padded(ref[n], nan) for n in ("q", "k", "v", "dO"))
    os_, dqs, dks, dvs = (padded(None, 7.0) for _ in range(4))
    s2 = (H * cap * hd, cap * hd, hd) * 4
    o2, lse2 = ops.attention_train(q, k, v, s2, B, H, L, L, hd, 1, hd ** -0.5, os_, Er=ref["Er"], keep=kd, keep_scale=1.25)
    g[:, :, :L] = ref["dO"].view(B, L, H, hd).transpose(1, 2)
    dEr2 = ops.attention_bwd(g, q, k, v, o2, lse2, s2, B, H, L, L, hd, 1, hd ** -0.5, dqs, dks, dvs, Er=ref["Er"], keep=kd, keep_scale=1.25)
    assert torch.equal(lse, lse2) and torch.equal(dEr, dEr2)
    for strided, flat in ((o2, o), (dqs, dq), (dks, dk), (dvs, dv)):
        assert (strided[:, :, L:] == 7.0).all()
        assert torch.equal(strided[:, :, :L], flat.view(B, L, H, hd).transpose(1, 2))


def test_refusals_carry_their_reason():
    z = torch.zeros(1, 4, 64, device=DEV)
    lse = torch.zeros(1, 4, 4, device=DEV)
    with pytest.raises(_lib.AmtError, match="head_dim 16 is not built for training"):
        ops.attention_train(z, z, z, blh_strides(4, 4, 4, 16), 1, 4, 4, 4, 16, 1, 0.25, torch.empty_like(z))
    with pytest.raises(_lib.AmtError, match="causal"):
        ops.attention_train(z, z, z, blh_strides(4, 4, 2, 32), 1, 2, 4, 4, 32, 0, 0.25, torch.empty_like(z), Er=torch.zeros(4, 32, device=DEV))
    with pytest.raises(_lib.AmtError, match="head_dim 16"):
        ops.attention_bwd(z, z, z, z, z, lse, blh_strides(4, 4, 4, 16), 1, 4, 4, 4, 16, 1, 0.25, *(torch.empty_like(z) for _ in range(3)))
