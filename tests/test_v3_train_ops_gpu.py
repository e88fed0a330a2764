"""The operators the V3 training adds, alone, against fp64 (tests/helpers_v3_train.py): `ops.diff_subln_train` / `diff_subln_bwd`
(csrc/diff_subln_train.hip), `autograd.DiffAttentionFn`, and `amt_moe_train_fwd_balanced` through `ops.moe_train` and a bare
`SharedMoELayer`.  Bounds: FACTOR x e32 by `rel_err`, e32 the same restatement in fp32 on one CPU thread; dlambda at the scale
A = sum |du o2| with the floor FACTOR x U.  Row counts around the launcher's workgroup rule are asked from the rule itself."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers_v3_train as V
from tests.helpers_family_train import one_thread
from tests.helpers_train_edges import rel_err
from video2music_amd import autograd as AG
from video2music_amd import ops
from video2music_amd.model.moe import GLUExpert, SharedMoELayer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def host(t):
    return t.detach().cpu().numpy()


# ---- the tail ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [16, 32, 36, 64, 128])
def test_diff_subln_train_is_diff_subln_bit_for_bit(hd):
    a = V.subln_inputs(37, hd)
    o1, o2, w, lam = dev(a["o1"]), dev(a["o2"]), dev(a["w"]), dev(a["lam"])
    y_dev = ops.diff_subln_train(o1, o2, w, lam, V.SUBLN_SCALE, eps=V.SUBLN_EPS)
    y_host = ops.diff_subln(o1, o2, w, float(a["lam"][0]), V.SUBLN_SCALE, eps=V.SUBLN_EPS)
    assert torch.equal(y_dev, y_host)


@functools.lru_cache(maxsize=None)
def plan_boundaries(hd):
    """Row counts one below / at every change of the plan kind of `diff_subln_bwd`: from one workgroup to several, and from the fixed
    rows per workgroup to the even spread over all of them.  Asked from the launcher's own rule."""
    blocks = lambda r: ops.diff_subln_bwd_blocks(r, hd)
    per0 = 1
    while blocks(per0 + 1) == 1:
        per0 += 1
    limit = 2 * max(blocks(1 << 20), 2) * per0 + 8
    kind = lambda r: (blocks(r) > 1, -(-r // blocks(r)) > per0)
    edges = [r for edge in range(2, limit) if kind(edge) != kind(edge - 1) for r in (edge - 1, edge)]
    assert len(edges) == 4, (hd, edges)
    return edges


def subln_rows(hd, which):
    rpw = 256 // hd                                         # rows per wave
    if which.startswith("edge"):
        return plan_boundaries(hd)[int(which[4:])], None
    return {"one": (1, None), "empty_lane_group": (4 * rpw + rpw - 1, None), "zero_row": (3 * rpw + 2, 1)}[which]


SUBLN_WHICH = ("one", "empty_lane_group", "edge0", "edge1", "edge2", "edge3", "zero_row")


def run_subln_bwd(a):
    o1, o2, w, lam, dy = (dev(a[k]) for k in ("o1", "o2", "w", "lam", "dy"))
    d_o1, d_o2, dw, dlam = ops.diff_subln_bwd(dy, o1, o2, w, lam, V.SUBLN_SCALE, eps=V.SUBLN_EPS)
    return {"o1": host(d_o1), "o2": host(d_o2), "w": host(dw), "lam": host(dlam)}


@pytest.mark.parametrize("which", SUBLN_WHICH)
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_diff_subln_bwd_against_fp64(hd, which):
    rows, zero_row = subln_rows(hd, which)
    a = V.subln_inputs(rows, hd, zero_row)
    r64, r32 = V.subln_restated(a, torch.float64), one_thread(V.subln_restated, a, torch.float32)
    got, again = run_subln_bwd(a), run_subln_bwd(a)
    for k in got:
        assert np.array_equal(got[k], again[k]), k
        assert np.isfinite(got[k]).all(), k
    for k in ("o1", "o2", "w"):
        err, e32 = rel_err(got[k], r64[k]), rel_err(r32[k], r64[k])
        print(f"diff_subln_bwd hd {hd} rows {rows}: d{k} {err:.3e} (e32 {e32:.3e})")
        assert err <= max(V.FACTOR * e32, V.FACTOR * V.U), (k, err, e32)
    A = r64["A"]
    err, e32 = rel_err(got["lam"], r64["lam"], A), rel_err(r32["lam"], r64["lam"], A)
    print(f"diff_subln_bwd hd {hd} rows {rows}: dlam {err:.3e} at A = {A:.3e} (e32 {e32:.3e})")
    assert err <= max(V.FACTOR * e32, V.FACTOR * V.U)


# ---- DiffAttentionFn -----------------------------------------------------------------------------------------------------------------
ATTN = [(1, 1, 1, 1, 32, True), (2, 2, 129, 129, 32, True), (3, 1, 33, 300, 128, False), (2, 2, 5, 17, 64, False)]


def run_diff_attention(a, B, H, Lq, Lk, hd, causal):
    t = {k: dev(v, k != "dy") for k, v in a.items()}
    y = AG.DiffAttentionFn.apply(t["q"], t["k"], t["v"], t["lam"], t["w"], B, H, Lq, Lk, causal, V.SUBLN_SCALE, V.SUBLN_EPS)
    y.backward(t["dy"])
    out = {k: host(t[k].grad) for k in ("q", "k", "v", "lam", "w")}
    out["y"] = host(y)
    return out


@pytest.mark.parametrize("B,H,Lq,Lk,hd,causal", ATTN)
def test_diff_attention_fn_against_fp64(B, H, Lq, Lk, hd, causal):
    a = V.diff_attention_inputs(B, H, Lq, Lk, hd)
    r64 = V.diff_attention_restated(a, B, H, Lq, Lk, hd, causal, torch.float64)
    r32 = one_thread(V.diff_attention_restated, a, B, H, Lq, Lk, hd, causal, torch.float32)
    got, again = run_diff_attention(a, B, H, Lq, Lk, hd, causal), run_diff_attention(a, B, H, Lq, Lk, hd, causal)
    assert got["y"].shape == (B, H, Lq, hd)
    for k in got:
        assert np.array_equal(got[k], again[k]), k
    for k in ("y", "q", "k", "v", "w"):
        # one key: both maps are [1] and q, k have no gradient in exact arithmetic; what fp32 leaves is held at the scale of dv
        scale = None if np.abs(r64[k]).max() > 0 else float(np.abs(r64["v"]).max())
        err, e32 = rel_err(got[k], r64[k], scale), rel_err(r32[k], r64[k], scale)
        print(f"DiffAttentionFn {(B, H, Lq, Lk, hd, causal)}: {k} {err:.3e} (e32 {e32:.3e})")
        assert err <= max(V.FACTOR * e32, V.FACTOR * V.U), (k, err, e32)
    A = r64["A"]
    err, e32 = rel_err(got["lam"], r64["lam"], A), rel_err(r32["lam"], r64["lam"], A)
    print(f"DiffAttentionFn {(B, H, Lq, Lk, hd, causal)}: dlam {err:.3e} at A = {A:.3e} (e32 {e32:.3e})")
    assert err <= max(V.FACTOR * e32, V.FACTOR * V.U)


# ---- the balancing router ------------------------------------------------------------------------------------------------------------
def moe_inputs(n_tok, d, dff, n_exp, seed=5):
    rng = np.random.default_rng(seed + n_tok)
    n = lambda *s: (rng.standard_normal(s) / np.sqrt(s[-1])).astype(np.float32)
    x = rng.standard_normal((n_tok, d)).astype(np.float32)
    gate_w, gate_b = (4.0 * n(n_exp, d)).astype(np.float32), (0.1 * rng.standard_normal(n_exp)).astype(np.float32)
    experts = (n(n_exp, dff, d), 0.1 * n(n_exp, dff), n(n_exp, dff, d), 0.1 * n(n_exp, dff), n(n_exp, d, dff), 0.1 * n(n_exp, d))
    shared = (n(dff, d), 0.1 * n(dff), n(dff, d), 0.1 * n(dff), n(d, dff), 0.1 * n(d))
    return x, gate_w, gate_b, tuple(np.ascontiguousarray(t, dtype=np.float32) for t in experts), tuple(np.ascontiguousarray(t, dtype=np.float32) for t in shared)


def case_bias(x, gate_w, gate_b):
    logits = x.astype(np.float64) @ gate_w.astype(np.float64).T + gate_b
    n_exp = gate_w.shape[0]
    order = list(V.BIAS_ORDER) if n_exp == 6 else list(range(n_exp))[::-1]
    return (logits.std() * np.linspace(-1.0, 1.0, n_exp)[order]).astype(np.float32), logits


def balanced(x, gate_w, gate_b, experts, shared, k, bias):
    return ops.moe_train(dev(x), dev(gate_w), dev(gate_b), [dev(t) for t in experts], [dev(t) for t in shared], (None, None, None), k,
                         experts[2].shape[1], sel_bias=None if bias is None else dev(bias), update_rate=V.UPDATE_RATE)


@pytest.mark.parametrize("n_tok,k", [(1, 2), (131, 2), (131, 1), (131, 3)])
def test_zero_bias_gives_the_plain_forwards_bits(n_tok, k):
    a = moe_inputs(n_tok, 64, 96, 6)
    plain = balanced(*a, k, None)
    zero = balanced(*a, k, np.zeros(6, dtype=np.float32))
    for p, z, what in zip(plain, zero, ("out", "idx", "wts")):         # `saved` holds rows nobody writes: the layer test below reads it
        assert torch.equal(p, z), what
    cnt = torch.bincount(plain[1].flatten().long().cpu(), minlength=6).to(torch.float32)
    assert torch.equal(zero[4].cpu(), V.UPDATE_RATE * (torch.mean(cnt) - cnt))


@pytest.mark.parametrize("n_tok,k", [(131, 2), (70, 1), (70, 3)])
def test_case_bias_selects_on_the_sum_and_weighs_with_the_raw_logits(n_tok, k):
    x, gate_w, gate_b, experts, shared = a = moe_inputs(n_tok, 64, 96, 6)
    bias, logits = case_bias(x, gate_w, gate_b)
    sel = torch.from_numpy(logits + bias.astype(np.float64))
    top = sel.topk(k + 1, dim=-1).values
    assert float((top[:, :-1] - top[:, 1:]).min()) >= V.ROUTE_GAP       # no row's choice or order hangs on fp32 rounding
    want_idx = sel.topk(k, dim=-1).indices
    flipped = (want_idx.sort(-1).values != torch.from_numpy(logits).topk(k, dim=-1).indices.sort(-1).values).any(-1).double().mean()
    assert float(flipped) >= 0.25
    out, idx, wts, saved, delta = balanced(*a, k, bias)
    again = balanced(*a, k, bias)
    for p, q in zip((out, idx, wts, delta), (again[0], again[1], again[2], again[4])):
        assert torch.equal(p, q)
    idx_h = idx.cpu().long()
    assert torch.equal(idx_h.sort(-1).values, want_idx.sort(-1).values)
    assert torch.equal(idx_h, want_idx)                                 # largest sum first
    want_w = torch.softmax(torch.gather(torch.from_numpy(logits), -1, idx_h), dim=-1)
    w32 = torch.softmax(torch.gather(torch.from_numpy(logits).float(), -1, idx_h), dim=-1)
    err, e32 = rel_err(host(wts), want_w.numpy()), rel_err(w32.numpy(), want_w.numpy())
    print(f"balanced router n_tok {n_tok} k {k}: wts {err:.3e} (e32 {e32:.3e}), {float(flipped):.2f} of the rows flipped")
    assert err <= max(V.FACTOR * e32, V.FACTOR * V.U)
    cnt = torch.bincount(idx_h.flatten(), minlength=6).to(torch.float32)
    assert torch.equal(delta.cpu(), V.UPDATE_RATE * (torch.mean(cnt) - cnt))


def bare_layer(starve=None):
    torch.manual_seed(3)
    layer = SharedMoELayer(GLUExpert(64, 96, 0.0), 64, n_experts=6, dropout=0.0, balancing=True)
    with torch.no_grad():
        layer.gate.weight.mul_(6.0)
        if starve is not None:
            layer.bias[starve] = -1.0e4
    return layer.to(DEV).train()


def test_a_zero_bias_layer_trains_to_the_bits_of_one_without_balancing():
    """`saved` of the balanced forward is what amt_moe_bwd reads: with a zero bias every gradient is the plain layer's."""
    x = torch.randn(131, 1, 64, generator=torch.Generator().manual_seed(4)).to(DEV)
    a = bare_layer()
    a.train_balancing = True
    a.update_rate = 0.0
    torch.manual_seed(3)
    b = SharedMoELayer(GLUExpert(64, 96, 0.0), 64, n_experts=6, dropout=0.0, balancing=False)
    b.load_state_dict({k: v for k, v in a.state_dict().items() if k != "bias"})
    b = b.to(DEV).train()
    res = []
    for layer in (a, b):
        xi = x.clone().requires_grad_(True)
        y = layer(xi)
        y.square().sum().backward()
        res.append([y.detach(), xi.grad] + [q.grad for q in layer.parameters()])
    assert len(res[0]) == len(res[1])
    for p, q in zip(*res):
        assert torch.equal(p, q)
    assert not bool(a.bias.any())


def test_a_bare_balancing_layer_refuses_until_told_and_then_trains_and_moves_its_bias():
    x = torch.randn(33, 2, 64, generator=torch.Generator().manual_seed(1)).to(DEV).requires_grad_(True)
    layer = bare_layer()
    with pytest.raises(NotImplementedError, match="balancing=True"):
        layer(x)
    layer.train_balancing = True
    before, version = layer.bias.clone(), layer.bias._version
    y = layer(x)
    y.sum().backward()
    idx = layer.last_routing[0].reshape(-1, 2).cpu().long()
    cnt = torch.bincount(idx.flatten(), minlength=6).to(torch.float32)
    assert torch.equal(layer.bias.cpu(), before.cpu() + (V.UPDATE_RATE * (torch.mean(cnt) - cnt)).unsqueeze(1))
    assert layer.bias._version > version and not torch.equal(layer.bias, before)
    assert x.grad is not None and layer.gate.weight.grad is not None and bool(torch.isfinite(x.grad).all())
    assert layer.eval()(x.detach()).shape == x.shape                    # eval ignores the bias, as before


def test_an_expert_the_bias_starves_gets_exact_zero_gradients():
    x = torch.randn(40, 2, 64, generator=torch.Generator().manual_seed(2)).to(DEV)
    layer = bare_layer(starve=4)
    layer.train_balancing = True
    layer(x).square().sum().backward()
    assert not bool((layer.last_routing[0] == 4).any())
    for q in layer.experts[4].parameters():
        assert q.grad is not None and not bool(q.grad.any())
    assert bool(layer.experts[0].linear1.weight.grad.any())
    assert not bool(layer.gate.weight.grad[4].any()) and not bool(layer.gate.bias.grad[4].any())


# ---- poisoned allocations and a side stream --------------------------------------------------------------------------------------------
B_, H_, LQ_, LK_, HD_ = 2, 2, 33, 17, 32


def _make_layer():
    layer = bare_layer()
    layer.train_balancing = True
    return layer


def _attention_and_mixture(layer):
    """A fresh layer per run: its bias starts at zero and its parameters' gradient accumulators belong to the run's own stream."""
    a = V.diff_attention_inputs(B_, H_, LQ_, LK_, HD_)
    t = {k: dev(v, k != "dy") for k, v in a.items()}
    y = AG.DiffAttentionFn.apply(t["q"], t["k"], t["v"], t["lam"], t["w"], B_, H_, LQ_, LK_, False, V.SUBLN_SCALE, V.SUBLN_EPS)
    z = layer(y.view(LQ_, B_, H_ * HD_))
    (z * t["dy"].view(LQ_, B_, H_ * HD_)).sum().backward()
    return (y.detach(), z.detach(), [t[k].grad for k in ("q", "k", "v", "lam", "w")], [q.grad for q in layer.parameters()], layer.bias.clone(),
            layer.last_routing)


def test_on_poisoned_allocations():
    from tests.test_poison_gpu import four_runs
    out = four_runs("DiffAttentionFn + balanced mixture", _attention_and_mixture, ("ops", "autograd"), make=_make_layer)
    assert bool(out[4].any())                                           # the bias moved


def test_on_a_side_stream():
    from tests import helpers_streams as HS
    HS.busy_null("DiffAttentionFn + balanced mixture", _attention_and_mixture, make=_make_layer)
