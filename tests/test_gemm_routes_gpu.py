"""Dense GEMM dispatch and epilogues through the C ABI (amt_linear_ex_fwd; amt_linear_fwd for the route-switch pair) against fp64:
the skinny route with every leading dimension off its natural width, both tile sizes with both epilogues, nk = 1 and odd nk, each
clause of vec_ok, and the launcher's refusals.  Cases, inputs, references and tolerances: tests/helpers_ops_edges.py (their input
conditions are checked on the CPU by test_ops_edges_host.py).  Every output sits in a sentinel-filled buffer wider than the product."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers_ops_edges as H
from video2music_amd import _lib

pytestmark = pytest.mark.gpu


def _p(addr):
    return C.c_void_p(addr) if addr is not None else None


def _launch(c, t, x_addr, y, ldx=None, ldw=None, ldr=None, ldy=None, act=None):
    inp = H.gemm_inputs(c.name)
    ldx, ldw, ldr, ldy = ldx or inp["ldx"], ldw or inp["ldw"], ldr or inp["ldr"], ldy or inp["ldy"]
    act = c.act if act is None else act
    if c.entry == "plain":
        _lib.call("amt_linear_fwd", _p(x_addr), _lib.ptr(t["w"]), _lib.ptr(t["bias"]), _lib.ptr(t["resid"]), _p(y.addr()), c.M, c.N, c.K, act,
                  _lib.stream_ptr())
    else:
        _lib.call("amt_linear_ex_fwd", _p(x_addr), ldx, _lib.ptr(t["w"]), ldw, _lib.ptr(t["bias"]), _lib.ptr(t["resid"]), ldr, _p(y.addr()), ldy,
                  c.M, c.N, c.K, act, _lib.stream_ptr())


def _device_inputs(c):
    inp = H.gemm_inputs(c.name)
    return {k: H.dev(inp[k]) for k in ("xbuf", "w", "bias", "resid")}


@pytest.mark.parametrize("name", [c.name for c in H.GEMM_CASES])
def test_gemm_route(name):
    c = H.GEMM_BY_NAME[name]
    inp = H.gemm_inputs(name)
    t = _device_inputs(c)
    y = H.Guarded(c.M * inp["ldy"])
    _launch(c, t, t["xbuf"].data_ptr() + 4 * c.xcol, y)
    torch.cuda.synchronize()
    out = y.check(H.rect_mask(c.M, inp["ldy"], c.N)).reshape(c.M, inp["ldy"])[:, :c.N]
    err = float(np.abs(out.astype(np.float64) - H.gemm_ref64(name)).max())
    tol = H.gemm_tol(name)
    print(f"{name} [{c.route}, {'vector' if c.vec else 'element-wise'} epilogue]: max |y - fp64| = {err:.3e} (tolerance {tol:.2e})")
    assert np.isfinite(out).all() and err < tol


@pytest.mark.parametrize("what", ["x_unaligned", "ldw_below_k", "ldx_not_mult4", "act_4"])
def test_gemm_refusals(what):
    """Raised on the host before any launch: the output keeps its sentinel."""
    c = H.GEMM_BY_NAME["skinny_strided"]
    inp = H.gemm_inputs(c.name)
    t = _device_inputs(c)
    y = H.Guarded(c.M * inp["ldy"])
    x_addr = t["xbuf"].data_ptr() + 4 * c.xcol
    with pytest.raises(_lib.AmtError):
        if what == "x_unaligned":            # column offset 1: not 16-byte aligned
            _launch(c, t, t["xbuf"].data_ptr() + 4, y)
        elif what == "ldw_below_k":
            _launch(c, t, x_addr, y, ldw=c.K - 4)
        elif what == "ldx_not_mult4":
            _launch(c, t, x_addr, y, ldx=c.K + 2)
        else:
            _launch(c, t, x_addr, y, act=4)
    torch.cuda.synchronize()
    y.check(np.zeros(y.n, dtype=bool))
