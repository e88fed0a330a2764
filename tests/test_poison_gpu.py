"""Every kernel path behind the package's Python-side allocations, run on poisoned memory (tests/helpers_poison.py).

Each case runs four times: twice plain, once under pass N (every allocated byte 0xFF: fp32 NaN, integers -1) and once under pass F (fp32
1.0e30; the mixed float / integer layouts listed there keep pass N's bytes).  Held:
  1  the two plain runs are equal on every output and gradient, bit for bit;
  2  each poisoned run equals the plain run on every output and gradient, with no tolerance, and everything is finite: a read of scratch
     nobody wrote and an output element nobody wrote both show here;
  3  both guards of every intercepted allocation still hold the pattern: the workspaces are allocated at exactly the size the
     *_floats functions report, so those sizes are sufficient;
  4  the plain result meets the case's existing fp64 bound, by the existing helper's own check (or, where that check lives inside a test
     function, by that function on the same inputs), so that the runs are not four equally wrong results.
Inputs, references and bounds are the existing helpers'; nothing here has a tolerance of its own.  Modules are built and their weights
loaded outside the scope (a fresh module for every run at model level, so that lazily built tables and caches are poisoned too)."""
import numpy as np
import pytest
import torch

from tests.helpers_poison import Poison

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = "video2music_amd."


# ---- the four runs -----------------------------------------------------------------------------------------------------------------
def flatten(out, prefix=""):
    """Nested tuples / lists / dicts of tensors, arrays, numbers and None -> {path: numpy array or None}."""
    if isinstance(out, dict):
        return {f"{prefix}{k}.{kk}": v for k, item in out.items() for kk, v in flatten(item).items()}
    if isinstance(out, (tuple, list)):
        return {f"{prefix}{i}.{kk}": v for i, item in enumerate(out) for kk, v in flatten(item).items()}
    if out is None:
        return {prefix: None}
    if isinstance(out, torch.Tensor):
        return {prefix: out.detach().cpu().numpy()}
    return {prefix: np.asarray(out)}


def same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
            continue
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k)
        if not np.array_equal(a[k], b[k]):
            bad = np.argwhere(np.atleast_1d(a[k] != b[k]))
            raise AssertionError(f"{what}: {k} differs at {len(bad)} of {a[k].size} elements, first at {bad[0].tolist()}: "
                                 f"{np.atleast_1d(a[k])[tuple(bad[0])]} vs {np.atleast_1d(b[k])[tuple(bad[0])]}")


def finite(a, what):
    for k, v in a.items():
        assert v is None or np.isfinite(v).all(), (what, k, "not finite")


def four_runs(tag, run, modules=("ops",), make=None, pass_f=True):
    """run(obj) with obj = make() (made outside the scope, once per run) or run() -> the first plain result as it came.  `modules`: the
    patched modules whose allocations the case must reach (a renamed import would bypass the proxy silently)."""
    def once():
        return run(make()) if make is not None else run()

    first = once()
    plain, again = flatten(first), flatten(once())
    same(plain, again, f"{tag}: two plain runs")
    finite(plain, f"{tag}: plain")
    for mode in ("N", "F") if pass_f else ("N",):
        obj = make() if make is not None else None
        with Poison(mode) as ps:
            got = flatten(run(obj) if make is not None else run())
        n = ps.check()
        counts = ps.counts()
        print(f"POISON {tag} pass {mode}: {n} allocations {dict(counts)} captured {ps.captured}")
        for m in modules:
            assert counts[PKG + m] > 0, (tag, m, "no allocation of this module went through the proxy")
        finite(got, f"{tag}: pass {mode}")
        same(got, plain, f"{tag}: pass {mode} against the plain run")
    return first


def dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


# ---- MoEFn -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,masked", [("one_token", False), ("tile_plus_one", False), ("tile_plus_one", True), ("silu", False), ("k3", False),
                                         ("split2_empty_group", False)])
def test_moe_fn(name, masked):
    from tests import test_moe_bwd_gpu as MB
    if masked:                                           # the masks of MB.test_given_masks_on_all_three_sites
        case, p = MB.MASKED[name], 0.5
        n_tok, d, raw, n_exp, k = case[:5]
        rng = np.random.default_rng(7)
        masks = [((rng.random(s) >= p) / (1 - p)).astype(np.float32) for s in ((n_tok * k, raw), (n_tok * k, d), (n_tok, raw))]
        x, dout, P, o64, e32 = MB.oracle(case, masks, "masked")
        layer = MB.build(case, P, p_inner=p, p_out=p)
        layer.dropout_masks = [dev(m) for m in masks]
    else:
        case = MB.CASES[name]
        x, dout, P, o64, e32 = MB.oracle(case)
        layer = MB.build(case, P)

    def run():
        out, grads = MB.run(layer, x, dout)
        return out, grads, layer.last_routing

    out, grads, _ = four_runs(f"MoEFn {name}{' masked' if masked else ''}", run, ("ops",))
    MB.check(case, out, grads, layer, o64, e32)


# ---- GluFn, RopeFn, RMSNormFn, LayerNormFn -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("silu", [False, True])
def test_glu_fn(silu, masked):
    from tests import helpers_family_train as FT, test_family_train_ops_gpu as FO
    n, d, dff = 129, 32, 100                             # one row past a tile, a hidden width padded to 128
    sd, a, mask = FT.glu_inputs(n, d, dff, silu, masked)
    e = FO.expert_module(sd, d, dff, silu)
    got = four_runs(f"GluFn silu {silu} masked {masked}", lambda: FO.glu_device(e, a, mask), ("ops",))
    FO.check("glu", got, FT.glu_restated(sd, a, mask, torch.float64), FT.one_thread(FT.glu_restated, sd, a, mask, torch.float32))


def test_rope_fn_last_cache_row():
    from tests import helpers_family_train as FT, test_family_train_ops_gpu as FO
    from video2music_amd import autograd as AG
    x, dy, cache = FT.rope_inputs("last_row")
    c = cache.to(DEV)

    def run():
        xt = dev(x, True)
        y = AG.RopeFn.apply(xt, c)
        y.backward(dev(dy))
        return {"y": y, "dx": xt.grad}

    got = four_runs("RopeFn last_row", run, ("ops",))
    y64, dx64 = FT.rope_restated(x, dy, cache, torch.float64)
    y32, dx32 = FT.rope_restated(x, dy, cache, torch.float32)
    FO.check("rope", {k: v.detach().cpu().numpy() for k, v in got.items()}, {"y": y64, "dx": dx64}, {"y": y32, "dx": dx32})


NORM_CASES = [(rows, dim, resid) for rows in (1, 37, 600) for dim in (100, 512) for resid in (False, True)]


@pytest.mark.parametrize("rows,dim,resid", NORM_CASES)
def test_rmsnorm_fn(rows, dim, resid):
    from tests import helpers_family_train as FT, test_family_train_ops_gpu as FO
    from video2music_amd import ops
    assert ops.norm_bwd_blocks(1) == 1 < ops.norm_bwd_blocks(37) < ops.norm_bwd_blocks(600)       # one workgroup, and several
    a = FT.rms_inputs(rows, dim, resid)
    got = four_runs(f"RMSNormFn {rows}x{dim} resid {resid}", lambda: FO.rms_device(a), ("ops",))
    FO.check("rms", got, FT.rms_restated(a, torch.float64), FT.one_thread(FT.rms_restated, a, torch.float32))


@pytest.mark.parametrize("rows,dim,resid", NORM_CASES)
def test_layernorm_fn(rows, dim, resid):
    from tests import test_layernorm_bwd_gpu as LN
    assert (rows, dim, resid) in LN.CASES
    a = LN.inputs(rows, dim, resid)
    four_runs(f"LayerNormFn {rows}x{dim} resid {resid}", lambda: LN.device(a), ("ops",))
    LN.test_gradients_against_fp64(rows, dim, resid)


# ---- AttentionFn -------------------------------------------------------------------------------------------------------------------
# (B, H, Lq, Lk, hd, causal, rpr, er_len, kv_group, mask) of tests/test_attn_train_gpu.py
ATTN_CASES = [(1, 1, 1, 1, 32, 1, r, 1, 1, m) for r in (0, 1) for m in (0, 1)] + [(2, 2, 37, 37, 32, 1, r, 37, 1, m) for r in (0, 1) for m in (0, 1)] + \
             [(2, 4, 37, 37, 32, 1, 0, 0, 2, m) for m in (0, 1)]


@pytest.mark.parametrize("case", ATTN_CASES)
def test_attention_fn(case):
    from tests import test_attn_train_gpu as AT
    assert case in AT.CASES
    B, H, Lq, Lk, hd, causal, rpr, er_len, g, mask = case
    a, keep = AT.make(*case)
    four_runs(f"AttentionFn {case}", lambda: AT.device(a, keep, H, causal, g), ("ops", "autograd"))
    AT.test_forward_and_gradients_against_fp64(*case)


def test_attention_fn_seq_first_strides():
    """(2, 2, 37, 37, 32) with Er-free causal attention and a keep mask through `lbh_strides`; the plain result is held to the bits of
    the batch-first call, which test_attention_fn holds to fp64."""
    from tests import test_attn_train_gpu as AT
    from video2music_amd import autograd as AG
    case = (2, 2, 37, 37, 32, 1, 0, 0, 1, 1)
    B, H, Lq, Lk, hd, causal, rpr, er_len, g, mask = case
    a, keep = AT.make(*case)
    kd = dev(keep)

    def run():
        t = {k: dev(a[k].transpose(1, 0, 2), True) for k in ("q", "k", "v")}
        o = AG.AttentionFn.apply(t["q"], t["k"], t["v"], None, kd, H, causal, hd ** -0.5, 1.0 / (1.0 - AT.P_DROP), g, AG.lbh_strides(B, H, hd, g))
        o.backward(dev(a["dO"].transpose(1, 0, 2)))
        return {"O": o, "q": t["q"].grad, "k": t["k"].grad, "v": t["v"].grad}

    got = four_runs("AttentionFn seq-first", run, ("ops", "autograd"))
    want = AT.device(a, keep, H, causal, g)
    for k, v in got.items():
        assert np.array_equal(v.detach().cpu().numpy().transpose(1, 0, 2), want[k]), k


# ---- losses and metrics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backward", [True, False])
@pytest.mark.parametrize("B,L", [(1, 1), (2, 39)])
def test_chord_loss(B, L, backward):
    from tests import test_chord_loss_gpu as CL
    from video2music_amd import ops
    ld, eps = 160, 0.1
    assert (B, L, ld, eps) in CL.CASES
    y, tgt, emo = CL.make_case(B, L, ld)
    yd, td, ed = dev(y), dev(tgt), dev(emo)
    loss, clip, dlogits = four_runs(f"chord_loss {B}x{L} backward {backward}", lambda: ops.chord_loss(yd, td, ed, CL.LAM, eps, backward=backward), ("ops",))
    assert (dlogits is None) == (not backward)
    CL.test_kernel_equals_torch_fp64(B, L, ld, eps)      # asserts that backward=False leaves loss and clip the same bits, too


@pytest.mark.parametrize("S", [1, 65])
def test_reg_loss(S):
    from tests import helpers_reg_eval as H, test_reg_loss_gpu as RL
    from video2music_amd import ops
    assert (1, S) in RL.CASES
    c = H.make_case(1, S, RL.W)
    nd, lo, inst = RL.targets(c)

    def run():
        ln_nd, p = RL.heads_on_device(c)                 # the head GEMMs' outputs are poisoned allocations as well
        return ln_nd, p, ops.reg_loss(ln_nd, p, nd, lo, inst)

    four_runs(f"reg_loss rows {S}", run, ("ops",))
    RL.test_kernel_equals_fp64_restatement_and_torch_on_the_device(1, S)


def test_chord_metrics_with_rows():
    from tests import helpers_eval as H, test_chord_metrics_gpu as CM
    from video2music_amd import ops
    from video2music_amd.utilities import constants as C
    B, L, ld = 3, 65, 160
    y, tgt, emo, prob = CM.make_case(B, L, seed=1000 * B + 10 * L + ld)
    yp = torch.full((B, L, ld), 1.0e4, device=DEV)
    yp[:, :, :C.CHORD_SIZE] = dev(y)
    t, e, p = dev(tgt.astype(np.int64)), dev(emo.astype(np.int32)), dev(prob.astype(np.float32))
    got = four_runs("chord_metrics L 65", lambda: ops.chord_metrics(yp, t, e, p, CM.THR, return_rows=True), ("ops",))
    CM.check(*got, H.restate(y, tgt, emo, prob, CM.THR), L)


def test_reg_metrics_with_rows():
    from tests import helpers_reg_eval as H, test_reg_metrics_gpu as RM
    from video2music_amd import ops
    B, S, W, pad = 3, 65, 40, 8
    assert (B, S, W) in H.KERNEL_CASES
    c = H.make_case(B, S, W)
    feat = torch.full((B, S, W + pad), 1.0e4, device=DEV)
    feat[:, :, :W] = dev(c["feat"])
    heads = dev(H.pack_heads(c["reg_w"], c["reg_b"], c["cls_w"], c["cls_b"]))
    nd, lo, inst = (dev(c[k]) for k in ("note_density", "loudness", "instrument"))
    got = four_runs("reg_metrics S 65", lambda: ops.reg_metrics(feat[:, :, :W], heads, nd, lo, inst, return_rows=True), ("ops",))
    RM.check(got, H.restate(**c), "poison")


# ---- RnnLayerFn, the training scan, the conv backward ------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [4, 3])
def test_rnn_layer_fn(G):
    from tests import test_rnn_train_gpu as RN
    n_dirs, d, B, L = 2, 24, 3, 5
    assert (G, n_dirs, d, B, L) in RN.CASES
    par, x, dy = RN.inputs(G, n_dirs, d, B, L)
    four_runs(f"RnnLayerFn G {G}", lambda: RN.device(G, n_dirs, d, par, x, dy), ("ops", "autograd"))
    RN.check(G, n_dirs, d, B, L)


@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("reverse", [0, 1])
def test_selective_scan_train_and_backward(reverse, version):
    from tests import test_mamba_bwd_gpu as MW
    from video2music_amd import ops
    B, L, ED = shape = (2, 33, 24)                       # one step past a 32-step chunk, ED no multiple of the 64-channel block
    c = MW.scan_case(B, L, ED, seed=B * 1000 + L)
    R, M, N = c["R"], B * L, MW.N
    d = {k: v.to(DEV) for k, v in c.items() if k != "R"}

    def run():
        y, y_pre, h_chunks = ops.selective_scan_train(d["xc"], d["draw"], d["dt_bias"], d["A_log"], d["dbc"], R, d["D"], d["xz"], B, L,
                                                      version=version, reverse=reverse)
        dxz, ddbc = torch.zeros(M, 2 * ED, device=DEV), torch.zeros_like(d["dbc"])
        dx, ddraw, dA_log, dD = ops.selective_scan_bwd(d["dout"], d["xc"], d["draw"], d["dt_bias"], d["A_log"], d["dbc"], R, d["D"], d["xz"], y_pre,
                                                       h_chunks, dxz, ddbc, B, L, version=version, reverse=reverse)
        return {"y": y, "y_pre": y_pre, "h_chunks": h_chunks, "dx": dx, "ddraw": ddraw, "dz": dxz[:, ED:], "dBC": ddbc[:, R:R + 2 * N],
                "dA_log": dA_log, "dD": dD}

    four_runs(f"selective_scan {shape} reverse {reverse} version {version}", run, ("ops",))
    MW.test_selective_scan_backward(shape, reverse, version)


@pytest.mark.parametrize("reverse", [0, 1])
def test_dwconv1d_silu_bwd_with_fewer_steps_than_taps(reverse):
    from tests import test_mamba_bwd_gpu as MW
    from video2music_amd import ops
    shape, K = (1, 3, 130), 8
    assert (shape, K) in MW.DWCONV
    B, L, C = shape
    xz, w, bias, dy = (t.to(DEV) for t in MW.dwconv_case(shape, K))

    def run():
        dxz = torch.zeros(B * L, 2 * C, device=DEV)
        dw, dbias = ops.dwconv1d_silu_bwd(dy, xz, C, w, bias, dxz, B, L, bool(reverse))
        return {"dx": dxz[:, :C], "dw": dw, "dbias": dbias}

    four_runs(f"dwconv1d_silu_bwd reverse {reverse}", run, ("ops",))
    MW.test_dwconv_silu_backward(shape, K, reverse)


# ---- inference scratch -------------------------------------------------------------------------------------------------------------
MOE_FIRST_TWO = ("full_two_segments", "full_plus_one")


def test_moe_cases_are_the_helpers_first_two():
    from tests import helpers_ops_edges as H
    assert tuple(c.name for c in H.MOE_CASES[:2]) == MOE_FIRST_TWO


@pytest.mark.parametrize("name", MOE_FIRST_TWO)
def test_moe_fwd_on_a_poisoned_scratch(name):
    """amt_moe_fwd (no Python wrapper calls it) through the existing runner, its scratch from the proxy.  The scratch holds the plan's
    integers, so pass F does not apply to it, and it is this case's only poisoned allocation."""
    from tests import test_moe_plan_gpu as MP
    plain = MP.MoeRun(name)
    first, again = plain.call(fill=0.0), plain.call()
    same(flatten(first), flatten(again), f"{name}: two plain runs")
    ps = Poison("N", modules=[])
    run = MP.MoeRun(name, scratch=ps.proxy.empty(plain.scratch.numel(), device=DEV, dtype=torch.float32))
    got = run.call()
    assert ps.check() == 1
    finite(flatten(got), name)
    same(flatten(got), flatten(first), f"{name}: pass N against the plain run")
    plain.check(*first)


@pytest.mark.parametrize("name", MOE_FIRST_TWO)
def test_moe_layer_eval_forward(name):
    """amt_moe_topk_fwd through MoELayer / SharedMoELayer's own allocations (model/moe.py), on the same steered case."""
    from tests import helpers_ops_edges as H, test_moe_plan_gpu as MP
    from video2music_amd.model.moe import GLUExpert, MoELayer, SharedMoELayer
    c, inp = H.MOE_BY_NAME[name], H.moe_inputs(name)
    assert c.glu and c.gate_b and c.k == 2
    layer = (SharedMoELayer if c.shared else MoELayer)(GLUExpert(c.d, c.dff), c.d, n_experts=c.n_exp, n_experts_per_token=c.k)
    sd = {"gate.weight": inp["gate_w"], "gate.bias": inp["gate_b"]}
    for pre, w, es in [("experts.%d." % e, inp["experts"], e) for e in range(c.n_exp)] + ([("shared_expert.", inp["shared"], 0)] if c.shared else []):
        for mine, theirs in (("linear1", "1"), ("gate", "g"), ("linear2", "2")):
            sd[pre + mine + ".weight"], sd[pre + mine + ".bias"] = w["w" + theirs][es], w["b" + theirs][es]
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    layer = layer.to(DEV).eval()
    x = dev(inp["x"]).view(c.n_tok, 1, c.d)

    def run():
        with torch.no_grad():
            out = layer(x)
        return out.reshape(c.n_tok, c.d), layer.last_routing[0].reshape(c.n_tok, c.k), layer.last_routing[1].reshape(c.n_tok, c.k)

    out, idx, wts = four_runs(f"MoELayer eval {name}", run, ("model.moe",))
    MP.MoeRun(name).check(out.cpu().numpy(), idx.cpu().numpy(), wts.cpu().numpy(), " [layer]")


def test_glu_expert_forward():
    from tests import helpers_ops_edges as H
    from video2music_amd import ops
    from video2music_amd.model.moe import GLUExpert
    n, d, dff, glu = piece = (129, 32, 96, True)
    assert piece in H.GLU_PIECES
    x, w = H.glu_piece_inputs(*piece)
    tol, _, ref = H.glu_piece_tol(*piece)
    e = GLUExpert(d, dff)
    e.load_state_dict({f"{mine}.{kind}": torch.from_numpy(w[pre + theirs][0]) for mine, theirs in (("linear1", "1"), ("gate", "g"), ("linear2", "2"))
                       for kind, pre in (("weight", "w"), ("bias", "b"))}, strict=True)
    e = e.to(DEV).eval()
    xd = dev(x)
    y = four_runs("ops.glu 129 rows", lambda: ops.glu(xd, e), ("ops",))
    assert float(np.abs(y.cpu().numpy().astype(np.float64) - ref).max()) < tol


def test_ep_expert_on_one_gpu():
    """amt_moe_ep_expert_fwd through `_HipEpOps.experts` (its y and scratch), at test_ep_expert_on_one_gpu's shape, inputs and bound."""
    from tests import helpers_ops_edges as H
    from video2music_amd.model.moe import GLUExpert, MoELayer, _HipEpOps
    d, dff, glu = 128, 192, True
    rc = H.EP_RECV_COUNTS
    expert = H.ep_expert_of_row(rc)
    n_recv = len(expert)
    rs = np.random.RandomState(41 + glu)                 # the draws of tests/test_moe_plan_gpu.py, in its order
    lin = lambda *s: (rs.standard_normal(s) * s[-1] ** -0.5).astype(np.float32)
    small = lambda *s: (rs.standard_normal(s) * 0.1).astype(np.float32)
    w = dict(w1=lin(2, dff, d), b1=small(2, dff), wg=lin(2, dff, d), bg=small(2, dff), w2=lin(2, d, dff), b2=small(2, d))
    rows = rs.standard_normal((n_recv, d)).astype(np.float32)
    ref, err32 = np.zeros((n_recv, d)), 0.0
    for e in (0, 1):
        ref[expert == e] = H.expert_apply(rows[expert == e], w, e, torch.float64).numpy()
        err32 = max(err32, float(np.abs(H.expert_apply(rows[expert == e], w, e, torch.float32).numpy() - ref[expert == e]).max()))
    tol = max(H.TOL, 8 * err32)
    assert tol <= H.MOE_TOL_CAP
    layer = MoELayer(GLUExpert(d, dff), d, n_experts=2)
    for e in (0, 1):
        layer.experts[e].load_state_dict({f"{mine}.{kind}": torch.from_numpy(w[pre + theirs][e]) for mine, theirs in (("linear1", "1"), ("gate", "g"), ("linear2", "2"))
                                          for kind, pre in (("weight", "w"), ("bias", "b"))}, strict=True)
    layer = layer.to(DEV).eval()
    drows, drc = dev(rows), dev(rc)
    epo = _HipEpOps(layer, drows, None, None, 0, 2)
    y = four_runs("ep expert", lambda: epo.experts(drows, drc, n_recv), ("model.moe",))
    assert float(np.abs(y.cpu().numpy().astype(np.float64) - ref).max()) < tol


# ---- one step of the models --------------------------------------------------------------------------------------------------------
def test_base_model_training_step():
    from tests import helpers_train_edges as E, test_train_edges_gpu as TE
    name = "one_by_one"                                  # the smallest case: one key everywhere, dEr identically zero
    c, bt = E.CASES[name], E.batch(name)
    assert all(q["B"] * q["L"] >= c["B"] * c["L"] for q in E.CASES.values())
    make = lambda: TE.build(c["cfg"], E.state_dict(name), dropout=c["p"])
    four_runs(f"base train {name}", lambda m: TE.step(m, name, bt), ("ops", "autograd"), make=make)
    TE.test_loss_logits_and_every_gradient_against_fp64(name)


@pytest.mark.parametrize("name", ["rms_hd128", "v22"])
def test_family_training_step(name):
    from tests import test_family_train_gpu as FG
    four_runs(f"family train {name}", lambda m: FG.step(name, m), ("ops", "autograd"), make=lambda: FG.build(name))
    FG.test_one_step_against_fp64(name)


@pytest.mark.parametrize("name", ["lstm_one_row", "bimambap_below_conv"])
def test_regression_training_step(name, monkeypatch):
    from tests import helpers_reg_train_edges as E, test_reg_train_edges_gpu as RG
    c = E.CASES[name]
    assert (c.B * c.S == 1) if name == "lstm_one_row" else (c.S < 4)          # one row; S below d_conv = 4
    data = [dev(a) for a in E.batch(name)]
    four_runs(f"regression train {name}", lambda m: RG.step(m, data), ("ops", "autograd"), make=lambda: RG.build(name))
    RG.test_loss_outputs_and_every_gradient_against_fp64(name, monkeypatch)


@pytest.mark.parametrize("name,modules", [("s5_v13", ("ops", "model.vmt_v2", "model.moe")), ("s5_v20", ("ops", "model.vmt_v2")),
                                          ("s5_v32", ("ops", "model.vmt_v3"))])
def test_family_forward(name, modules):
    from tests import helpers_family_parity as HF, test_family_forward_parity_gpu as FP
    c = HF.BY_NAME[name]
    assert c.shape == "s5" and not c.drop               # one query, one key, one frame
    f = HF.inputs(name)

    def run(m):
        with torch.no_grad():
            return m(f["ids"], f["root"], f["attr"], f["semantic"].cuda(), f["key"].cuda(), f["scene_offset"].cuda(), f["motion"].cuda(),
                     f["emotion"].cuda(), mask=c.mask)

    four_runs(f"family forward {name}", run, modules, make=lambda: FP.build(c))
    FP.test_family_forward_vs_fp64_oracle(name)


@pytest.mark.parametrize("name,modules", [("bimambap_256_64_37_1x3_L1", ("ops",)), ("moe_bimambap_64_64_37_1x1_L2", ("ops", "model.moe")),
                                          ("bilstm_64_64_64_3x1_L1", ("ops", "model.video_regression"))])
def test_regression_forward(name, modules):
    from tests import helpers_reg_parity as HR, test_reg_forward_parity_gpu as RP
    c = HR.BY_NAME[name]
    f = HR.inputs(name)
    sem, emo = f["semantic"].cuda(), f["emotion"].cuda()

    def run(m):
        with torch.no_grad():
            return m.get_feature(sem, None, None, emo), m(sem, None, None, emo)

    four_runs(f"regression forward {name}", run, modules, make=lambda: RP.build(c))
    RP.test_reg_forward_vs_fp64_oracle(name)


def test_base_model_python_side_buffers(golden):
    """The base model's eval forward and generate: their decode workspaces live inside the C handle, out of the proxy's reach; what
    is poisoned here is what the module allocates itself -- `logits` of forward, `tokens` / `out` of generate_batch, `probs` of the
    host-side multinomial draw.  Bounds: the reference's recorded logits (tests/test_model_gpu.py's LOGIT_TOL), the oracle's greedy ids."""
    from oracle import amt_oracle as O
    from tests import test_model_gpu as MM
    from tests.helpers import CFG1, feats_t
    from video2music_amd import synthetic
    g = golden("g_fwd_cfg1.npz")
    f = MM.cu(feats_t(synthetic.synthetic_features(3, seed=1234), key=g["key"]))
    root, attr = dev(g["root_B3_L12"]), dev(g["attr_B3_L12"])
    fc = feats_t(synthetic.synthetic_features(1, seed=1))
    f1, f2 = MM.cu(fc), MM.cu(feats_t(synthetic.synthetic_features(2, seed=5)))
    pr, prr, pra = torch.tensor([1]), torch.tensor([1]), torch.tensor([0])
    T = 16
    built = []

    def make():
        built.append(MM.build(CFG1))
        return built[-1][0]

    def run(m):
        feats = lambda q: (q["semantic"], q["key"], q["scene_offset"], q["motion"], q["emotion"])
        with torch.no_grad():
            logits = m(torch.zeros_like(root), root, attr, *feats(f))
        greedy = m.generate_batch(*feats(f1), pr, prr, pra, target_seq_length=T, beam=0, sampler="argmax")
        top1 = m.generate_batch(*feats(f1), pr, prr, pra, target_seq_length=T, beam=1)
        torch.manual_seed(3)
        drawn = m.generate_batch(*feats(f2), pr, prr, pra, target_seq_length=T, beam=0, sampler="multinomial")
        return logits, greedy, top1, drawn

    logits, greedy, top1, drawn = four_runs("base eval", run, ("model.video_music_transformer",), make=make)
    assert np.abs(logits.cpu().numpy() - g["logits_B3_L12"]).max() < MM.LOGIT_TOL
    ref = O.generate(built[0][1], CFG1["num_heads"], fc["semantic"], fc["key"], fc["scene_offset"], fc["motion"], fc["emotion"], pr, prr, pra,
                     target_seq_length=T, beam=0)
    assert np.array_equal(greedy.cpu().numpy(), ref.numpy())
    assert top1.shape == (1, T) and drawn.shape == (2, T) and int(drawn.min()) >= 1


def test_stand_alone_modules(golden):
    """MultiheadGQA (its output and scratch), RMSNorm and RotaryPositionalEmbeddings: the modules' own allocations, at the shapes and
    within the bounds of tests/test_modules_gpu.py's reference goldens."""
    from tests import test_modules_gpu as MG
    g, gr = golden("g_gqa.npz"), golden("g_rms_rope.npz")
    gqa, _ = MG.load(MG.MultiheadGQA(256, 8, 2), MG.GQA_SHAPES, 3)
    rms = MG.RMSNorm(128).cuda()
    rms.weight.data = dev(gr["rms_w"])
    rope = MG.RotaryPositionalEmbeddings(128, 300).cuda()
    x, rx, px = dev(g["x_L6_B3"]), dev(gr["rms_x"]), dev(gr["rope_x_B2"])
    L = px.shape[0]

    def run():
        return gqa(x, x, x, is_causal=True)[0], rms(rx), rope(px.view(4, L, 2, 32)).view(L, 2, 128)

    y, ry, py = four_runs("stand-alone modules", run, ("model.grouped_query_attention", "model.custom_transformer", "model.rotate_operation"))
    assert np.abs(y.detach().cpu().numpy() - g["y_L6_B3_c1"]).max() < 1e-4
    assert np.abs(ry.detach().cpu().numpy() - gr["rms_y"]).max() < 1e-5 and np.abs(py.detach().cpu().numpy() - gr["rope_y_B2"]).max() < 1e-5


@pytest.mark.parametrize("cls_name,version", [("V2", "2.2"), ("V1", "1.1")])
def test_lockstep_step_with_poisoned_tables_and_caches(cls_name, version):
    """B = 2 at the narrowest width of tests/test_lockstep_parity_gpu.py (E 128), teacher-forced for 8 of the caches' 300 positions:
    the K/V rows past the position hold poison while the earlier ones are read; the step's ws, packed weights and logits are poisoned
    as well (a fresh model per run: the packed weights are cached on it)."""
    from tests import test_lockstep_parity_gpu as LP
    from tests.helpers import feats_t, lockstep_step_logits
    from video2music_amd import synthetic
    from video2music_amd.model import video_music_transformer as M
    cls = {"V1": M.VideoMusicTransformer_V1, "V2": M.VideoMusicTransformer_V2}[cls_name]
    B, S, T, seed = 2, 17, 8, 97
    kw = dict(version_name=version, n_layers=6 if cls_name == "V2" else 4, num_heads=4, d_model=128, dim_feedforward=256)
    built = []

    def make():
        built.append(LP.build(cls, seed=8, recipe="feedback", **kw))
        return built[-1][0]

    f = {k: v.cuda() for k, v in feats_t(synthetic.synthetic_features(B, seed=seed, n_frames=S)).items()}
    roots, attrs = LP.chord_inputs(make(), B, T, seed)
    four_runs(f"lockstep {cls_name}", lambda m: lockstep_step_logits(m, f, roots, attrs),
              ("ops", "model.vmt_v2", "model.moe", "model.v2_step_table"), make=make)
    m, sd = built[-1]
    assert m._max_dec > T
    LP.check_config("h/poison", m, sd, B=B, S=S, T=T, seed=seed)        # the same inputs: fp32 forward, and the fp64 oracle for '2.2'
