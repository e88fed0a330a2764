"""The MoE plan (csrc/moe.hip: route -> count -> 128-aligned offsets -> place -> three grouped GEMMs -> combine) with STEERED routing,
so that the plan is known: empty experts, exactly full and full-plus-one segments, expert 63 of 64, 5 and 2 experts, narrow and ragged
widths, no gate bias, logit ties, k = 1 / 3 / 8 -- and the pieces of the expert-parallel form.  Cases, fp64 restatements and
tolerances: tests/helpers_ops_edges.py.  Every call runs on scratch pre-filled with NaN and again on zeros: same bits, all finite."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers_ops_edges as H
from video2music_amd import _lib

pytestmark = pytest.mark.gpu
P = _lib.ptr


def _sp():
    return _lib.stream_ptr()


def _expert_tensors(w, e=None):
    """Device copies of (w1, b1, wg, bg, w2, b2), stacked, or expert e alone; null where the expert kind has none."""
    if w is None:
        return [None] * 6
    return [H.dev(w[k] if e is None or w[k] is None else w[k][e]) for k in ("w1", "b1", "wg", "bg", "w2", "b2")]


class MoeRun:
    """Device inputs of one case and a scratch buffer: call() launches amt_moe_fwd (k = 2) or amt_moe_topk_fwd on it."""

    def __init__(self, name, scratch=None):
        self.c = c = H.MOE_BY_NAME[name]
        inp = H.moe_inputs(name)
        self.x, self.gw, self.gb = H.dev(inp["x"]), H.dev(inp["gate_w"]), H.dev(inp["gate_b"])
        self.ex, self.sh = _expert_tensors(inp["experts"]), _expert_tensors(inp["shared"], 0)
        n = _lib.call("amt_moe_topk_scratch_floats", c.n_tok, c.d, c.dff, c.n_exp, c.k)
        assert n == _lib.call("amt_moe_scratch_floats", c.n_tok, c.d, c.dff, c.n_exp) or c.k != 2
        self.scratch = scratch if scratch is not None else torch.empty(n, device="cuda")
        assert self.scratch.numel() >= n

    def call(self, fill=None):
        c = self.c
        if fill is not None:
            self.scratch.fill_(fill)
        out = H.Guarded(c.n_tok * c.d)
        idx = torch.full((c.n_tok, c.k), -1, dtype=torch.int32, device="cuda")
        wts = torch.full((c.n_tok, c.k), float("nan"), device="cuda")
        args = [P(self.x), P(self.gw), P(self.gb), *[P(t) for t in self.ex], *[P(t) for t in self.sh], C.c_void_p(out.addr()), P(idx), P(wts),
                P(self.scratch), c.n_tok, c.d, c.dff, c.n_exp]
        if c.k == 2:
            _lib.call("amt_moe_fwd", *args, _sp())
        else:
            _lib.call("amt_moe_topk_fwd", *args, c.k, _sp())
        torch.cuda.synchronize()
        return out.check(np.ones(out.n, dtype=bool)).reshape(c.n_tok, c.d).copy(), idx.cpu().numpy(), wts.cpu().numpy()

    def check(self, out, idx, wts, tag=""):
        c = self.c
        assert np.array_equal(idx, c.chosen), f"{c.name}{tag}: routing differs from the steered ids (largest first, lower id first among equals)"
        w_err = float(np.abs(wts.astype(np.float64) - H.moe_weights64(c.name)).max())
        err = float(np.abs(out.astype(np.float64) - H.moe_ref64(c.name)).max())
        tol, _ = H.moe_tol(c.name)
        print(f"{c.name}{tag}: max |out - fp64| = {err:.3e} (tolerance {tol:.2e}), max |w - fp64| = {w_err:.1e}   ({c.edge})")
        assert np.isfinite(out).all() and w_err < 1e-6 and err < tol and tol <= H.MOE_TOL_CAP


@pytest.mark.parametrize("name", [c.name for c in H.MOE_CASES])
def test_moe_steered(name):
    run = MoeRun(name)
    c = run.c
    out_nan, idx, wts = run.call(fill=float("nan"))
    run.check(out_nan, idx, wts, " [NaN scratch]")
    out_zero, idx0, wts0 = run.call(fill=0.0)
    assert np.array_equal(H.bits(out_nan), H.bits(out_zero)), "the result depends on what the scratch held"
    assert np.array_equal(idx, idx0) and np.array_equal(H.bits(wts), H.bits(wts0))
    if c.k == 2:                                         # the router alone returns the same bits
        ridx = torch.full((c.n_tok, 2), -1, dtype=torch.int32, device="cuda")
        rw = torch.full((c.n_tok, 2), float("nan"), device="cuda")
        _lib.call("amt_moe_route_fwd", P(run.x), P(run.gw), P(run.gb), P(ridx), P(rw), c.n_tok, c.d, c.n_exp, _sp())
        torch.cuda.synchronize()
        assert np.array_equal(ridx.cpu().numpy(), idx) and np.array_equal(H.bits(rw.cpu().numpy()), H.bits(wts))


def test_moe_second_call_on_the_same_scratch():
    """Two consecutive calls with different routings on one scratch, nothing re-initialised in between (and back again)."""
    a = MoeRun("ragged_counts")
    a.scratch.zero_()
    b = MoeRun("ragged_counts_other", scratch=a.scratch)
    assert (a.c.n_tok, a.c.d, a.c.dff, a.c.n_exp) == (b.c.n_tok, b.c.d, b.c.dff, b.c.n_exp)
    for run, tag in ((a, " [first call]"), (b, " [second call, other routing]"), (a, " [third call]")):
        run.check(*run.call(), tag)


# ---- pieces ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,dff,glu", H.GLU_PIECES)
def test_glu_expert(n, d, dff, glu):
    x, w = H.glu_piece_inputs(n, d, dff, glu)
    tol, _, ref = H.glu_piece_tol(n, d, dff, glu)
    t = _expert_tensors(w, 0)
    dx = H.dev(x)
    scratch = torch.full((2 * n * dff,), float("nan"), device="cuda")
    out = H.Guarded(n * d)
    _lib.call("amt_glu_expert_fwd", P(dx), *[P(v) for v in t], C.c_void_p(out.addr()), P(scratch), n, d, dff, _sp())
    torch.cuda.synchronize()
    y = out.check(np.ones(out.n, dtype=bool)).reshape(n, d)
    err = float(np.abs(y.astype(np.float64) - ref).max())
    print(f"glu expert n={n} d={d} dff={dff} {'GLU' if glu else 'Linear-SiLU-Linear'}: max |y - fp64| = {err:.3e} (tolerance {tol:.2e})")
    assert np.isfinite(y).all() and err < tol


@pytest.mark.parametrize("d", [4, 516])
@pytest.mark.parametrize("with_shared", [False, True])
def test_moe_combine(d, with_shared):
    """out[t] = wa * y[slot_pos[t, a]] + wb * y[slot_pos[t, b]] (+ s * shared[t]) with a the slot of the LOWER expert id."""
    rs = np.random.RandomState(d + with_shared)
    n_tok, n_rows = 37, 90
    idx = H._route_mixed(n_tok, 8, 2).astype(np.int32)
    slot_pos = rs.permutation(n_rows)[:2 * n_tok].reshape(n_tok, 2).astype(np.int32)
    wts = rs.uniform(0.1, 0.9, size=(n_tok, 2)).astype(np.float32)
    y = rs.standard_normal((n_rows, d)).astype(np.float32)
    shared = rs.standard_normal((n_tok, d)).astype(np.float32) if with_shared else None
    a = np.argmin(idx, axis=1)
    tok = np.arange(n_tok)
    f = lambda v: v.astype(np.float64)
    ref = f(wts[tok, a])[:, None] * f(y[slot_pos[tok, a]]) + f(wts[tok, 1 - a])[:, None] * f(y[slot_pos[tok, 1 - a]])
    if with_shared:
        ref = ref + np.float64(np.float32(0.5)) * f(shared)
    assert (idx[:, 0] > idx[:, 1]).any() and (idx[:, 0] < idx[:, 1]).any()
    out = H.Guarded(n_tok * d)
    D = [H.dev(v) for v in (y, slot_pos, idx, wts, shared)]
    _lib.call("amt_moe_combine_fwd", *[P(v) for v in D], 0.5, C.c_void_p(out.addr()), n_tok, d, _sp())
    torch.cuda.synchronize()
    got = out.check(np.ones(out.n, dtype=bool)).reshape(n_tok, d)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"combine d={d} shared={with_shared}: max err {err:.2e} of max |out| {np.abs(ref).max():.2f}")
    assert err <= 1e-6 * np.abs(ref).max()


@pytest.mark.parametrize("d", [4, 260])
def test_gather_rows(d):
    rs = np.random.RandomState(d)
    src = rs.standard_normal((7, d)).astype(np.float32)
    index = np.asarray([3, -1, 6, 0, 3], dtype=np.int32)
    ds, di = H.dev(src), H.dev(index)
    dst = H.Guarded(5 * d)
    assert _lib.call("amt_gather_rows_fwd", P(ds), P(di), C.c_void_p(dst.addr()), 0, d, _sp()) == 0       # n_rows = 0: nothing happens
    torch.cuda.synchronize()
    dst.check(np.zeros(dst.n, dtype=bool))
    _lib.call("amt_gather_rows_fwd", P(ds), P(di), C.c_void_p(dst.addr()), 5, d, _sp())
    torch.cuda.synchronize()
    got = dst.check(np.ones(dst.n, dtype=bool)).reshape(5, d)
    want = np.where(index[:, None] >= 0, src[np.maximum(index, 0)], np.float32(0.0))
    assert np.array_equal(H.bits(got), H.bits(want))


def test_ep_dispatch_plan():
    """counts exact; perm[slot_pos[i]] == i // 2; each expert's send rows contiguous, in expert order, exactly packed; a second call with
    another routing on the same `ints` is right as well (the plan leaves its counters zero)."""
    ints = torch.zeros(256, dtype=torch.int32, device="cuda")
    for name in ("ragged_counts", "ragged_counts_other", "experts_63_and_0"):
        c = H.MOE_BY_NAME[name]
        idx = c.chosen.astype(np.int32)
        n_assign = 2 * c.n_tok
        didx = H.dev(idx)
        counts = torch.full((c.n_exp + 8,), -5, dtype=torch.int32, device="cuda")
        perm = torch.full((n_assign + 8,), -5, dtype=torch.int32, device="cuda")
        slot_pos = torch.full((n_assign + 8,), -5, dtype=torch.int32, device="cuda")
        _lib.call("amt_moe_ep_dispatch_plan_fwd", P(didx), c.n_tok, c.n_exp, P(counts), P(perm), P(slot_pos), P(ints), _sp())
        torch.cuda.synchronize()
        counts, perm, slot_pos = counts.cpu().numpy(), perm.cpu().numpy(), slot_pos.cpu().numpy()
        assert (counts[c.n_exp:] == -5).all() and (perm[n_assign:] == -5).all() and (slot_pos[n_assign:] == -5).all()
        want = H.plan_counts(c.chosen, c.n_exp)
        assert np.array_equal(counts[:c.n_exp], want), name
        sp_, flat = slot_pos[:n_assign], idx.reshape(-1)
        assert np.array_equal(np.sort(sp_), np.arange(n_assign)), "exact packing: the send rows are a permutation of 0 .. 2 n_tok - 1"
        assert np.array_equal(perm[:n_assign][sp_], np.arange(n_assign) // 2)
        start = np.concatenate([[0], np.cumsum(want)])
        assert ((sp_ >= start[flat]) & (sp_ < start[flat + 1])).all(), "an expert's rows are contiguous and the experts in order"
        assert (ints.cpu().numpy()[:64] == 0).all(), "counts must be zero again for the next call"


@pytest.mark.parametrize("glu", [True, False])
def test_ep_expert_on_one_gpu(glu):
    """world = 2, e_local = 2, recv_counts [[129, 0], [3, 64]]: y_out in arrival order against the per-row fp64 expert."""
    d, dff = 128, 192
    rc = H.EP_RECV_COUNTS
    expert = H.ep_expert_of_row(rc)
    n_recv = len(expert)
    rs = np.random.RandomState(41 + glu)
    lin = lambda *s: (rs.standard_normal(s) * s[-1] ** -0.5).astype(np.float32)
    small = lambda *s: (rs.standard_normal(s) * 0.1).astype(np.float32)
    w = dict(w1=lin(2, dff, d) if glu else None, b1=small(2, dff) if glu else None, wg=lin(2, dff, d), bg=small(2, dff), w2=lin(2, d, dff), b2=small(2, d))
    rows = rs.standard_normal((n_recv, d)).astype(np.float32)
    ref = np.zeros((n_recv, d))
    err32 = 0.0
    for e in (0, 1):
        ref[expert == e] = H.expert_apply(rows[expert == e], w, e, torch.float64).numpy()
        err32 = max(err32, float(np.abs(H.expert_apply(rows[expert == e], w, e, torch.float32).numpy() - ref[expert == e]).max()))
    tol = max(H.TOL, 8 * err32)
    assert tol <= H.MOE_TOL_CAP
    n = _lib.call("amt_moe_ep_expert_scratch_floats", n_recv, d, dff, 2)
    scratch = torch.full((n,), float("nan"), device="cuda")
    t = _expert_tensors(w)
    drows, drc = H.dev(rows), H.dev(rc)
    y = H.Guarded(n_recv * d)
    _lib.call("amt_moe_ep_expert_fwd", P(drows), P(drc), 2, 2, n_recv, *[P(v) for v in t], C.c_void_p(y.addr()), P(scratch), d, dff, _sp())
    torch.cuda.synchronize()
    got = y.check(np.ones(y.n, dtype=bool)).reshape(n_recv, d)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"ep expert {'GLU' if glu else 'Linear-SiLU-Linear'}: max |y - fp64| = {err:.3e} (tolerance {tol:.2e})")
    assert np.isfinite(got).all() and err < tol
