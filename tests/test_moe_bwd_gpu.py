"""`autograd.MoEFn` (amt_moe_train_fwd / amt_moe_bwd) alone against the fp64 restatement of tests/helpers_moe_train.py: the layer's
output, the gradient of its input, of the router and of every expert's and the shared expert's parameters.

Bound of every gradient tensor: rel_err(got, g64) <= max(8 e32, n U) with e32 the error of torch's fp32 CPU autograd of the same
restatement against the same fp64 gradients, U = 2^-24 and n the longest sum behind the value: the rows a weight or bias gradient adds
up (at most n_tok) or the widest inner product (d_ff, d), whichever is longer; for the input's gradient the inner products and the k
expert rows.  Where the fp64 gradient is exactly zero the kernel's is exactly zero.  The kernel's routing must equal the fp64 top-k
for every token; the seeds were picked on the CPU so that the fp64 gap between the k-th and (k+1)-th gate logit is at least 1e-4 of the
largest |logit| (asserted on the fp64 side), two orders above fp32 rounding of a d <= 64 dot product.

The split* cases are the ones where the grouped weight-gradient product cuts an expert's tiles into S > 1 runs and adds the partials in
a second pass (ops.moe_wgrad_splits; tests/test_reg_moe_train_host.py asserts each case's S and the per-expert tiles its comment
claims, and that every other case has S = 1 for the experts)."""
import numpy as np
import pytest
import torch

from tests import helpers_moe_train as T
from video2music_amd import ops
from video2music_amd.model.moe import GLUExpert, MoELayer, SharedMoELayer, SiLUExpert, TopKScheduler, expert_tensors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name: (n_tok, d, dff_raw, n_exp, k, shared, GLU experts, gate bias of expert 0 (True: 8, expert 0 in every top-k; False: as drawn),
#        seed[, (seed, gap): rows of x with a smaller fp64 gate gap are drawn again])
CASES = {
    "one_token": (1, 32, 65, 6, 2, True, True, False, 0),            # four empty experts, odd width
    "full_tile": (128, 32, 64, 6, 2, False, True, True, 0),          # expert 0: one exactly full tile
    "tile_plus_one": (129, 32, 64, 6, 2, True, True, True, 0),       # a second tile holding one row
    "head_width": (200, 64, 129, 6, 2, True, True, False, 1),       # free routing; the heads' real width at d = 64
    "silu": (70, 32, 64, 6, 2, True, False, False, 0),               # no up branch
    "k1": (50, 32, 64, 4, 1, False, True, False, 0),                 # the k != 2 route and combine kernels
    "k3": (50, 32, 64, 4, 3, False, True, False, 0),
    "all_experts": (40, 32, 64, 2, 2, False, True, False, 0),        # every expert sees every token
    # S > 1 runs per expert in the weight-gradient products
    "split2_even": (256, 32, 64, 2, 2, False, True, False, 0),       # S 2; both experts 256 rows: two runs of one full tile
    "split2_empty_group": (520, 32, 65, 2, 1, True, True, 8.0, 0),   # S 2; expert 0 all 520 rows: runs of 3 + 2 tiles, the last tile 8
                                                                     # rows; expert 1 none: two empty runs, exact zeros; shared S 5
    "split3_empty_run": (700, 32, 64, 2, 1, False, True, 0.5, 0),    # S 3; 447 / 253 rows: runs 2 + 2 + 0 and 1 + 1 + 0 tiles
    "split2_head_width": (705, 64, 129, 6, 2, True, True, False, 1),  # the heads' layer at its first S 2: segments of 2 and 3 tiles
    "split3_silu": (1089, 32, 65, 6, 2, True, False, False, 5),      # S 3 without the up branch (seeds 0-4 leave a gap under T.GAP)
    "split10": (4100, 32, 64, 6, 2, True, True, False, 0, (99, 2e-4)),  # S 10; 33 trips of the stable placement; the dY / dU / dG
                                                                     # data products over more than 4096 plan rows; 8 rows redrawn
}
SPLIT = [name for name in CASES if name.startswith("split")]
MASKED = {"tile_plus_one": (129, 32, 65, 6, 2, True, True, False, 0),
          "split2_empty_group": CASES["split2_empty_group"]}      # the masks go by assignment, the runs cut the segments

_ORACLE = {}


def oracle(case, masks=None, tag=None):
    """(inputs, fp64 result, per-tensor e32) of a case, computed once."""
    key = (case, tag)
    if key not in _ORACLE:
        n_tok, d, raw, n_exp, k, shared, glu, force0, seed = case[:9]
        x, dout, P = T.layer_params(n_tok, d, raw, n_exp, k, shared, glu, seed, force0, *case[9:])
        o64 = T.layer_grads(x, dout, P, n_exp, k, shared, masks)
        o32 = T.layer_grads(x, dout, P, n_exp, k, shared, masks, dtype=torch.float32)
        e32 = {name: (T.rel_err(o32["grads"][name], g) if np.abs(g).max() > 0 else 0.0) for name, g in o64["grads"].items()}
        _ORACLE[key] = (x, dout, P, o64, e32)
    return _ORACLE[key]


def build(case, P, p_inner=0.0, p_out=0.0):
    n_tok, d, raw, n_exp, k, shared, glu = case[:7]
    expert = GLUExpert(d, raw, dropout=p_inner) if glu else SiLUExpert(d, raw, dropout=p_inner)
    layer = (SharedMoELayer if shared else MoELayer)(expert, d, n_experts=n_exp, n_experts_per_token=k, dropout=p_out)
    layer.load_state_dict({name: torch.from_numpy(v) for name, v in P.items()}, strict=True)
    return layer.to(DEV)


def run(layer, x, dout):
    """One training forward and backward: out, {name: gradient}."""
    layer.zero_grad()
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    out = layer.train()(xt.view(x.shape[0], 1, x.shape[1]))
    out.backward(torch.from_numpy(dout).to(DEV).view(out.shape))
    grads = {name: q.grad.detach().cpu().numpy().astype(np.float64) for name, q in layer.named_parameters()}
    grads["x"] = xt.grad.detach().cpu().numpy().astype(np.float64)
    return out.detach().reshape(x.shape), grads


def check(case, got_out, got, layer, o64, e32):
    n_tok, d, raw, n_exp, k = case[:5]
    assert o64["gap"] >= T.GAP, ("the case's seed leaves a gate gap of", o64["gap"])
    idx, wts = layer.last_routing
    assert np.array_equal(idx.reshape(n_tok, k).cpu().numpy(), o64["idx"])                      # every token
    assert np.abs(wts.reshape(n_tok, k).cpu().numpy() - o64["weights"]).max() <= 64 * T.U
    assert T.rel_err(got_out.cpu().numpy(), o64["out"]) <= max(raw, d) * T.U
    assert set(got) == set(o64["grads"])
    worst = {}
    for name, want in o64["grads"].items():
        assert got[name].shape == want.shape, name
        assert (got[name][want == 0.0] == 0.0).all(), (name, "nonzero where the fp64 gradient is exactly zero")
        if np.abs(want).max() == 0.0:
            continue
        n = max(raw, d) + k if name == "x" else max(n_tok, raw, d)
        err, bound = T.rel_err(got[name], want), max(8 * e32[name], n * T.U)
        worst[name] = err / bound
        assert err <= bound, (name, err, bound, e32[name])
    top = max(worst, key=worst.get)
    print("worst err / bound =", round(worst[top], 3), "at", top)


@pytest.mark.parametrize("name", list(CASES))
def test_layer_output_and_every_gradient_against_fp64(name):
    case = CASES[name]
    x, dout, P, o64, e32 = oracle(case)
    layer = build(case, P)
    out, got = run(layer, x, dout)
    check(case, out, got, layer, o64, e32)
    if name == "one_token":                       # four experts without a row: their buffers are written, as exact zeros
        empty = sorted(set(range(6)) - set(o64["idx"].ravel().tolist()))
        assert len(empty) == 4 and all(not got[f"experts.{e}.linear2.bias"].any() for e in empty)
    if name in ("full_tile", "tile_plus_one", "split2_empty_group"):    # the gate bias did what the case is about
        assert (o64["idx"] == 0).any(axis=1).all()
    if name == "split2_empty_group":              # expert 1 without a row under a split: both its runs are empty
        assert all(not v.any() for key, v in got.items() if key.startswith("experts.1."))
        assert sum(key.startswith("experts.1.") for key in got) == 6


@pytest.mark.parametrize("name", list(MASKED))
def test_given_masks_on_all_three_sites(name):
    case, p = MASKED[name], 0.5
    n_tok, d, raw, n_exp, k = case[:5]
    rng = np.random.default_rng(7)
    masks = [((rng.random(s) >= p) / (1 - p)).astype(np.float32) for s in ((n_tok * k, raw), (n_tok * k, d), (n_tok, raw))]
    x, dout, P, o64, e32 = oracle(case, masks, "masked")
    layer = build(case, P, p_inner=p, p_out=p)
    layer.dropout_masks = [torch.from_numpy(m).to(DEV) for m in masks]
    out, got = run(layer, x, dout)
    assert len(layer.last_dropout_masks) == 3 and all(torch.equal(a, b) for a, b in zip(layer.last_dropout_masks, layer.dropout_masks))
    check(case, out, got, layer, o64, e32)
    plain = oracle(case)[3]
    assert T.rel_err(o64["out"], plain["out"]) > 0.1               # the masks did something


@pytest.mark.parametrize("name", list(CASES))
def test_training_forward_without_masks_equals_the_eval_forward(name):
    case = CASES[name]
    x, dout, P, o64, e32 = oracle(case)
    layer = build(case, P)
    xt = torch.from_numpy(x).to(DEV).view(x.shape[0], 1, x.shape[1])
    with torch.no_grad():
        want = layer.eval()(xt)
        ridx, rw = layer.last_routing
    got = layer.train()(xt.clone().requires_grad_(True))
    assert got.requires_grad and layer.last_dropout_masks == []
    assert torch.equal(got.detach(), want) and torch.equal(layer.last_routing[0], ridx) and torch.equal(layer.last_routing[1], rw)


@pytest.mark.parametrize("name", ["tile_plus_one", "head_width", "silu", "k3"] + SPLIT)
def test_two_backward_calls_give_the_same_bits(name):
    case = CASES[name]
    x, dout, P, o64, e32 = oracle(case)
    layer = build(case, P)
    first = run(layer, x, dout)[1]
    again = run(layer, x, dout)[1]
    assert all(np.array_equal(first[k], again[k]) for k in first)


def test_temperature_scales_the_router_gradient():
    """ops.moe_bwd's temperature: the forward takes gate_w / t and gate_b / t (the logits divided by t), the backward the undivided
    gate_w and t; against the restatement with the logits divided by t before topk / softmax.  At t = 1 the result is another one."""
    case, t = CASES["tile_plus_one"], 0.7
    n_tok, d, raw, n_exp, k = case[:5]
    x, dout, P, _, _ = oracle(case)
    if ("temperature", t) not in _ORACLE:
        o64 = T.layer_grads(x, dout, P, n_exp, k, True, temperature=t)
        o32 = T.layer_grads(x, dout, P, n_exp, k, True, dtype=torch.float32, temperature=t)
        _ORACLE[("temperature", t)] = (o64, {name: T.rel_err(o32["grads"][name], g) for name, g in o64["grads"].items()})
    o64, e32 = _ORACLE[("temperature", t)]
    assert o64["gap"] >= T.GAP
    layer = build(case, P)
    stacked, shared = layer._stacked_expert_weights(), expert_tensors(layer.shared_expert)
    tr = lambda w: w.transpose(-1, -2).contiguous()
    xt, gw, gb = torch.from_numpy(x).to(DEV), layer.gate.weight.detach().contiguous(), layer.gate.bias.detach().contiguous()
    out, idx, wts, saved = ops.moe_train(xt, (gw / t).contiguous(), (gb / t).contiguous(), stacked, shared, (None, None, None), k, raw)
    assert np.array_equal(idx.cpu().numpy(), o64["idx"])
    assert T.rel_err(out.cpu().numpy(), o64["out"]) <= max(raw, d) * T.U

    def grads(temperature):
        dx, dgw, dgb, de, _ = ops.moe_bwd(torch.from_numpy(dout).to(DEV), xt, gw, saved, (tr(stacked[0]), tr(stacked[2]), tr(stacked[4])),
                                          (tr(shared[0]), tr(shared[2]), tr(shared[4])), (None, None, None), k, raw, n_exp, temperature=temperature)
        g = {"x": dx, "gate.weight": dgw, "gate.bias": dgb}
        for e in range(n_exp):
            for key, v in zip(("linear1.weight", "linear1.bias", "gate.weight", "gate.bias", "linear2.weight", "linear2.bias"), de):
                g[f"experts.{e}.{key}"] = v[e][:, :raw] if key == "linear2.weight" else v[e] if key == "linear2.bias" else v[e][:raw]
        return {key: v.cpu().numpy().astype(np.float64) for key, v in g.items()}

    got, plain = grads(t), grads(1.0)
    worst = {}
    for name, have in got.items():
        want = o64["grads"][name]
        n = max(raw, d) + k if name == "x" else max(n_tok, raw, d)
        err, bound = T.rel_err(have, want), max(8 * e32[name], n * T.U)
        worst[name] = err / bound
        assert err <= bound, (name, err, bound, e32[name])
        if name in ("x", "gate.weight", "gate.bias"):                 # what the temperature reaches
            assert T.rel_err(plain[name], want) > bound, (name, "the same at temperature 1")
    top = max(worst, key=worst.get)
    print("worst err / bound =", round(worst[top], 3), "at", top)


def test_training_mode_refusals_say_why():
    x = torch.zeros(4, 1, 32, device=DEV)
    with pytest.raises(NotImplementedError, match="scheduler"):
        MoELayer(GLUExpert(32, 64), 32, n_experts=4, topk_scheduler=TopKScheduler(4, 2)).to(DEV).train()(x)
    with pytest.raises(NotImplementedError, match="balancing"):
        SharedMoELayer(GLUExpert(32, 64), 32, n_experts=4, balancing=True).to(DEV).train()(x)
    layer = MoELayer(GLUExpert(32, 64), 32, n_experts=4).to(DEV).train()
    layer.expert_parallel = True
    with pytest.raises(NotImplementedError, match="expert-parallel"):
        layer(x)
    with pytest.raises(NotImplementedError, match="n_experts_per_token"):
        MoELayer(GLUExpert(32, 64), 32, n_experts=4, n_experts_per_token=5).to(DEV).train()(x)
