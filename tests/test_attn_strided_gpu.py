"""amt_attn_fwd, the strided / grouped / scaled form of the prefill attention (the V2 / V3 stacks, MultiheadGQA), against
softmax((q * qs) k^T + mask) v in fp64 read through the same strides: the split-K kernel (head_dim 32 / 64, Lk >= 256, small grid)
with the causal mask, idle waves, score spikes and grouped heads, and the 128-row kernel incl. Lk >= 256 on a grid of 512.
Cases and references: tests/helpers_ops_edges.py.  o is allocated with padding and a sentinel."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers_ops_edges as H
from video2music_amd import _lib

pytestmark = pytest.mark.gpu


def _call(c, inp, t, o, B=None, H_=None, hd=None, kv_group=None, strides=None):
    lay = inp["lay"]
    st = (C.c_int64 * 12)(*(strides or inp["strides"]))
    addr = lambda k: C.c_void_p(t[k].data_ptr() + 4 * lay[k][0])
    _lib.call("amt_attn_fwd", addr("q"), addr("k"), addr("v"), C.c_void_p(o.addr(lay["o"][0])), st, B or c.B, H_ or c.H, c.Lq, c.Lk,
              hd or c.hd, c.causal, kv_group or c.g, inp["q_scale"], _lib.stream_ptr())


@pytest.mark.parametrize("name", [c.name for c in H.ATTN_CASES])
def test_attn_strided(name):
    c = H.ATTN_BY_NAME[name]
    inp = H.attn_inputs(name)
    t = {k: H.dev(v) for k, v in inp["bufs"].items()}
    oi, osize = H.attn_o_index(c)
    o = H.Guarded(osize)
    _call(c, inp, t, o)
    torch.cuda.synchronize()
    out = o.check(oi)[oi]                                   # (B, H, Lq, hd), everything else still the sentinel
    err = float(np.abs(out.astype(np.float64) - H.attn_ref64(name)).max())
    print(f"{name}: max |o - fp64| = {err:.3e}   ({c.edge})")
    assert np.isfinite(out).all() and err < H.TOL


@pytest.mark.parametrize("what", ["kv_group_3_of_4_heads", "k_ls_not_mult4", "head_dim_48"])
def test_attn_refusals(what):
    c = H.ATTN_BY_NAME["splitk_hd32_40x300c_clip_qs1"]
    inp = H.attn_inputs(c.name)
    t = {k: H.dev(v) for k, v in inp["bufs"].items()}
    oi, osize = H.attn_o_index(c)
    o = H.Guarded(osize)
    with pytest.raises(_lib.AmtError):
        if what == "kv_group_3_of_4_heads":
            assert c.H == 4
            _call(c, inp, t, o, kv_group=3)
        elif what == "k_ls_not_mult4":
            st = list(inp["strides"])
            st[5] += 2
            _call(c, inp, t, o, strides=st)
        else:
            _call(c, inp, t, o, hd=48)
    torch.cuda.synchronize()
    o.check(np.zeros(o.n, dtype=bool))
