"""The softmax-shaped, scan, gate and row-statistics kernels against fp64 on the recipes of tests/helpers_numeric_range.py: inputs
away from N(0,1), where the running-max rescale, `m + log l`, `__expf` at large arguments, softplus's threshold, a sigmoid past the
exponential's overflow and the row statistics decide the answer.  tests/test_numeric_range_host.py shows on the CPU that every recipe
reaches its regime, that its bound stays under 1e-3 and that the wrong variant it exists for misses it.  The families that came later
run the same recipes: the auxiliary chord loss, the wide recurrence and wide-state scan kernels, the differential sub-norm's backward
and the balanced router.

Bound for every output: rel_err(got, ref64) <= max(8 e32, n U) (see the helper); every test prints err/bound per output."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import helpers_eval as HE
from tests import helpers_numeric_range as R
from tests import helpers_ops_edges as HO
from video2music_amd import _lib, ops
from video2music_amd.autograd import blh_strides

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = _lib.ptr


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def check(tag, got, w64, w32, n_of, vanish=0.0, only=None):
    """`got` holds every output of the reference, or exactly those named in `only`."""
    line, bad, _ = R.judge(got, w64, w32, n_of, tag, vanish, only)
    print(line)
    assert not bad, (bad, line)


# ---- A. softmax-shaped ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("shape", R.ATTN_FWD_SHAPES)
@pytest.mark.parametrize("recipe", R.ATTN_RECIPES)
def test_attention_forward(recipe, shape, causal):
    Lq, Lk, hd, kernel = shape
    c, inp = R.attn_fwd_case(recipe, Lq, Lk, hd, kernel, causal)
    assert ops.attn_route(c.B, c.H, Lq, Lk, hd) == kernel
    t = {k: dev(v) for k, v in inp["bufs"].items()}
    oi, osize = HO.attn_o_index(c)
    o = HO.Guarded(osize)
    _lib.call("amt_attn_fwd", P(t["q"]), P(t["k"]), P(t["v"]), C.c_void_p(o.addr()), (C.c_int64 * 12)(*inp["strides"]), c.B, c.H, Lq, Lk, hd,
              causal, 1, inp["q_scale"], _lib.stream_ptr())
    torch.cuda.synchronize()
    w64, w32 = R.attn_fwd_refs(recipe, Lq, Lk, hd, kernel, causal)
    check(f"attention {recipe} {shape} causal {causal}", {"o": o.check(oi)[oi]}, w64, w32, lambda k: Lk + hd)


@pytest.mark.parametrize("case", R.ATTN_TRAIN_CASES)
@pytest.mark.parametrize("recipe", R.ATTN_RECIPES)
def test_attention_training_forward_and_backward(recipe, case):
    H, Lq, Lk, hd, g, causal, rpr, mask = case
    B = 1
    a, keep = R.attn_recipe(recipe, B, H, Lq, Lk, hd, g, rpr, mask, R.onehot_train(causal))
    t = {k: dev(v) for k, v in a.items()}
    kd = None if keep is None else dev(keep)
    strides, qs, ks = blh_strides(Lq, Lk, H, hd, g), hd ** -0.5, 1.0 / (1.0 - R.P_DROP)
    o, lse = ops.attention_train(t["q"], t["k"], t["v"], strides, B, H, Lq, Lk, hd, causal, qs, torch.empty_like(t["q"]), kv_group=g,
                                 Er=t.get("Er"), keep=kd, keep_scale=ks)
    dq, dk, dv = (torch.full_like(t[n], float("nan")) for n in ("q", "k", "v"))
    dEr = ops.attention_bwd(t["dO"], t["q"], t["k"], t["v"], o, lse, strides, B, H, Lq, Lk, hd, causal, qs, dq, dk, dv, kv_group=g,
                            Er=t.get("Er"), keep=kd, keep_scale=ks)
    torch.cuda.synchronize()
    got = {"O": host(o), "lse": host(lse), "q": host(dq), "k": host(dk), "v": host(dv)}
    if rpr:
        got["Er"] = host(dEr)
    w64, w32 = R.attn_train_refs(recipe, *case)
    check(f"attention_train {recipe} {case}", got, w64, w32, R.attn_train_n(H, Lq, Lk, hd, g), R.VANISH)


@pytest.mark.parametrize("recipe", R.ATTN_RECIPES)
def test_rpr_prefill(recipe):
    """amt_rpr_attn_fwd at L = 130, head_dim 64, `onehot` at the full 100: from its key on every other probability of a row and the
    rescale factor of the tile that brings it are exactly 0."""
    H, L, hd = R.RPR_PREFILL
    a, _ = R.attn_recipe(recipe, 1, H, L, L, hd, 1, 1, 0)
    t = {k: dev(v) for k, v in a.items()}
    qs = (t["q"] * hd ** -0.5).contiguous()                 # this entry point takes the scaled query; 1 / 8 is exact
    o = torch.full_like(t["q"], float("nan"))
    _lib.call("amt_rpr_attn_fwd", P(qs), P(t["k"]), P(t["v"]), P(t["Er"]), P(o), 1, H, L, hd, L, _lib.stream_ptr())
    w64, w32 = R.rpr_prefill_refs(recipe)
    check(f"rpr_attn {recipe}", {"O": host(o)}, w64, w32, lambda k: L + hd)


@pytest.mark.parametrize("pos", [299, 20])                   # in the last key batch and in the first
@pytest.mark.parametrize("recipe", R.ATTN_RECIPES)
def test_attention_decode(recipe, pos):
    """amt_attn_decode_fwd at cap 300: row `pos` of the causal self-attention of the recipe at (300, 300)."""
    cap, hd, H = 300, 64, 2
    a, _ = R.attn_recipe(recipe, 1, H, cap, cap, hd)
    q = (dev(a["q"])[:, pos] * hd ** -0.5).contiguous()                                      # (1, H hd)
    kc, vc = (dev(a[n]).view(1, cap, H, hd).transpose(1, 2).contiguous() for n in ("k", "v"))
    o = torch.full_like(q, float("nan"))
    _lib.call("amt_attn_decode_fwd", P(q), P(kc), P(vc), None, P(o), 1, H, hd, cap, pos, 0, _lib.stream_ptr())
    w64, w32 = R.attn_fwd_refs(recipe, cap, cap, hd, "row", 1)
    row = lambda w: {"o": w["o"][0, :, pos].reshape(1, H * hd)}
    check(f"attn_decode {recipe} pos {pos}", {"o": host(o)}, row(w64), row(w32), lambda k: pos + 1 + hd)


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("treatment", R.LOGIT_TREATMENTS)
def test_chord_loss_and_metrics(treatment, smoothing):
    from tests.test_chord_loss_gpu import LAM as lam             # the weighting its torch_cpu, the reference, uses
    y, tgt, emo, prob = R.chord_logits(treatment)
    B, L = tgt.shape
    yd, td, ed = dev(y), dev(tgt), dev(emo)
    loss, clip, dlogits = ops.chord_loss(yd, td, ed, lam, smoothing)
    w64, w32 = R.chord_refs(treatment, smoothing)
    got = R.chord_split({"loss": host(loss), "clip": host(clip), "dlogits": host(dlogits)})
    check(f"chord_loss {treatment} smoothing {smoothing}", got, w64, w32, R.chord_n(B, L))
    if smoothing == 0.0:                                         # the evaluation kernel forms the same two per-clip sums
        m, pred, _, _ = ops.chord_metrics(yd, td, ed, dev(prob), 0.8, return_rows=True)
        f = {k: i for i, k in enumerate(HE.FIELDS)}
        m = host(m)
        check(f"chord_metrics {treatment}", {"clip_ce": m[:, f["ce_sum"]], "clip_bce": m[:, f["bce_sum"]]}, w64, w32, R.chord_n(B, L),
              only=("clip_ce", "clip_bce"))
        assert np.array_equal(m[:, f["n_valid"]], host(clip)[:, 0]) and np.array_equal(pred.cpu().numpy(), y.argmax(-1))


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("layout", ["rows", "view"])
@pytest.mark.parametrize("recipe", R.AUX_RECIPES)
def test_chord_aux_loss(recipe, layout, smoothing):
    """amt_chord_loss_aux_fwd_bwd at (2, 65): the six losses, `count`, the six per-clip columns and dlogits, each at its own scale.  An
    inactive hinge of the `count_flip_guard` recipes is exactly 0, and with neither active the gradient is the plain loss kernel's."""
    from tests import helpers_chord_aux as HA
    y, tgt, emo = R.chord_aux_case(recipe, layout)
    B, L = tgt.shape
    yd, td, ed = dev(y), dev(tgt), dev(emo)
    loss, clip, dlogits = ops.chord_loss_aux(yd, td, ed, R.AUX_W[0], R.AUX_W[1], smoothing, layout)
    w64, w32 = R.chord_aux_refs(recipe, layout, smoothing)
    got = R.chord_aux_split({"loss": host(loss), "clip": host(clip), "dlogits": host(dlogits)})
    assert got["count"][0] == w64["count"][0]
    check(f"chord_aux {recipe} {layout} smoothing {smoothing}", got, w64, w32, R.chord_aux_n(B, L))
    for k in ("loss_aux3", "loss_aux5", "clip_a3", "clip_a5"):
        if not w64[k].any():
            assert not got[k].any(), k
    if recipe.startswith("count_flip_guard"):                   # small cross-entropies at + 1000: the plain loss and the metrics kernel too
        _, pclip, plain = ops.chord_loss(yd, td, ed, R.AUX_W[0], smoothing)
        sums = lambda c, i, j: {"clip_ce": host(c)[:, i], "clip_bce": host(c)[:, j]}
        check(f"chord_loss {recipe} {layout} smoothing {smoothing}", sums(pclip, 1, 2), w64, w32, R.chord_aux_n(B, L), only=("clip_ce", "clip_bce"))
        if smoothing == 0.0:
            f = {k: i for i, k in enumerate(HE.FIELDS)}
            m = ops.chord_metrics(yd, td, ed, dev(np.full((B, L), 0.9, dtype=np.float32)), 0.8, return_rows=True)[0]
            check(f"chord_metrics {recipe} {layout}", sums(m, f["ce_sum"], f["bce_sum"]), w64, w32, R.chord_aux_n(B, L), only=("clip_ce", "clip_bce"))
        if recipe == "count_flip_guard1":
            assert R.rel_err(host(dlogits), host(plain)) <= R.bound(R.rel_err(w32["dlogits"], w64["dlogits"]), HA.NC)


# ---- B. selective scan ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("shape", R.SCAN_SHAPES)
@pytest.mark.parametrize("recipe", R.SCAN_RECIPES)
def test_selective_scan(recipe, shape, reverse, version):
    scan_forward_and_backward(recipe, shape, 16, reverse, version)


@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("N", R.SCAN_WIDE_N)
@pytest.mark.parametrize("shape", R.SCAN_SHAPES)
@pytest.mark.parametrize("recipe", R.SCAN_RECIPES)
def test_selective_scan_wide_training(recipe, shape, N, reverse, version):
    """amt_selective_scan_wide_train_fwd / amt_selective_scan_wide_bwd at 32 and 256 states: checkpoints every 32 steps (L = 33 and 70
    cross one and two), N / 16 slices whose partial state sums a second launch adds."""
    assert ops.scan_ckpt_steps(N) == R.SCAN_CHUNK
    scan_forward_and_backward(recipe, shape, N, reverse, version)


def scan_forward_and_backward(recipe, shape, N, reverse, version):
    B, L, ED = shape
    c = R.scan_recipe(recipe, B, L, ED, N)
    Rk, M = c["R"], B * L
    d = {k: v.to(DEV) for k, v in c.items() if k != "R"}
    fwd = (d["xc"], d["draw"], d["dt_bias"], d["A_log"], d["dbc"], Rk, d["D"], d["xz"], B, L)
    y_eval = ops.selective_scan(*fwd, version=version, reverse=reverse)
    y, y_pre, h_chunks = ops.selective_scan_train(*fwd, version=version, reverse=reverse)
    assert torch.equal(y, y_eval)
    dxz = torch.full((M, 2 * ED), float("nan"), device=DEV)
    ddbc = torch.full_like(d["dbc"], float("nan"))
    dx, ddraw, dA_log, dD = ops.selective_scan_bwd(d["dout"], d["xc"], d["draw"], d["dt_bias"], d["A_log"], d["dbc"], Rk, d["D"], d["xz"], y_pre,
                                                   h_chunks, dxz, ddbc, B, L, version=version, reverse=reverse)
    got = {"y": y, "dx": dx, "ddraw": ddraw, "dz": dxz[:, ED:], "dB": ddbc[:, Rk:Rk + N], "dC": ddbc[:, Rk + N:Rk + 2 * N],
           "d_dt_bias": ddraw.sum(0), "dA_log": dA_log, "dD": dD}
    got = R.scan_split(recipe, {k: host(v) for k, v in got.items()})
    w64, w32 = R.scan_refs(recipe, B, L, ED, N, version, reverse)
    check(f"scan {recipe} {shape} N {N} reverse {reverse} version {version}", got, w64, w32, R.scan_n(B, L, N), R.SCAN_VANISH)


@pytest.mark.parametrize("reverse", [0, 1])
def test_selective_scan_wide_state(reverse):
    """N = 64 (inference only) on `slow_decay`."""
    B, L, ED, N = 1, 70, 40, 64
    c = R.scan_recipe("slow_decay", B, L, ED, N)
    d = {k: v.to(DEV) for k, v in c.items() if k != "R"}
    y = ops.selective_scan(d["xc"], d["draw"], d["dt_bias"], d["A_log"], d["dbc"], c["R"], d["D"], d["xz"], B, L, version=1, reverse=reverse)
    w64, w32 = R.scan_refs("slow_decay", B, L, ED, N, 1, reverse, False)
    check(f"scan slow_decay N 64 reverse {reverse}", {"y": host(y)}, w64, w32, R.scan_n(B, L, N))


# ---- C. gates --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("recipe,G,n_dirs", R.RNN_CASES)
def test_recurrent_gates(recipe, G, n_dirs):
    xproj, w_hh, b_hh, dy = R.rnn_recipe(recipe, G, n_dirs)
    B, L, d = xproj.shape[0], xproj.shape[1], R.RNN_SHAPE[2]
    M, Cc = B * L, ops.rnn_reserve_cols(G)
    xp, wh, bh, dyd = dev(xproj.reshape(M, -1)), dev(w_hh), dev(b_hh), dev(dy.reshape(M, -1))
    nan = lambda cols: torch.full((M, cols), float("nan"), device=DEV)
    y, y_eval, rsv, dxp = nan(n_dirs * d), nan(n_dirs * d), nan(n_dirs * Cc * d), nan(n_dirs * G * d)
    dhn = nan(n_dirs * d) if G == 3 else None
    ops.rnn_seq(xp, wh, bh, y_eval, 0, B, L, d, G, n_dirs=n_dirs)
    ops.rnn_seq_train(xp, wh, bh, y, 0, rsv, B, L, d, G, n_dirs=n_dirs)
    ops.rnn_seq_bwd(dyd, 0, rsv, y, 0, wh, dxp, dhn, B, L, d, G, n_dirs=n_dirs)
    assert torch.equal(y, y_eval)
    hidden = dxp.view(M, n_dirs, G, d).clone()               # the hidden side's pre-activation gradients: a GRU's n block is dhn
    if G == 3:
        hidden[:, :, 2] = dhn.view(M, n_dirs, d)
    got = {"y": host(y), "dxproj": host(dxp), "db_hh": host(hidden.sum(0).reshape(n_dirs, G * d))}
    w64, w32 = R.rnn_refs(recipe, G, n_dirs)
    check(f"rnn {recipe} G {G} dirs {n_dirs}", got, w64, w32, R.rnn_n(recipe, G))


@pytest.mark.parametrize("recipe,G,n_dirs,d", R.RNN_WIDE_CASES)
def test_wide_recurrent_gates(recipe, G, n_dirs, d):
    """amt_rnn_wide_seq_fwd / _train_fwd / _bwd (csrc/rnn_wide.hip) at d = 160 and 256, driven as `test_recurrent_gates` drives the
    register kernels."""
    xproj, w_hh, b_hh, dy = R.rnn_recipe(recipe, G, n_dirs, R.RNN_SHAPE[0], d)
    B, L = xproj.shape[:2]
    M, Cc = B * L, ops.rnn_reserve_cols(G)
    xp, wh, bh, dyd = dev(xproj.reshape(M, -1)), dev(w_hh.reshape(n_dirs * G * d, d)), dev(b_hh.reshape(-1)), dev(dy.reshape(M, -1))
    nan = lambda cols: torch.full((M, cols), float("nan"), device=DEV)
    y, y_eval, rsv, dxp = nan(n_dirs * d), nan(n_dirs * d), nan(n_dirs * Cc * d), nan(n_dirs * G * d)
    dhn = nan(n_dirs * d) if G == 3 else None
    ops.rnn_wide_seq(xp, wh, bh, y_eval, 0, B, L, d, G, n_dirs=n_dirs)
    ops.rnn_wide_seq_train(xp, wh, bh, y, 0, rsv, B, L, d, G, n_dirs=n_dirs)
    ops.rnn_wide_seq_bwd(dyd, 0, rsv, y, 0, wh, dxp, dhn, B, L, d, G, n_dirs=n_dirs)
    assert torch.equal(y, y_eval)
    hidden = dxp.view(M, n_dirs, G, d).clone()               # the hidden side's pre-activation gradients: a GRU's n block is dhn
    if G == 3:
        hidden[:, :, 2] = dhn.view(M, n_dirs, d)
    got = {"y": host(y), "dxproj": host(dxp), "db_hh": host(hidden.sum(0).reshape(n_dirs, G * d))}
    w64, w32 = R.rnn_refs(recipe, G, n_dirs, d)
    check(f"rnn_wide {recipe} G {G} dirs {n_dirs} d {d}", got, w64, w32, R.rnn_n(recipe, G, d=d))


@pytest.mark.parametrize("M,N,K,act,resid", R.ACT_CASES)
def test_activation_epilogues(M, N, K, act, resid):
    x, w, b, r = R.act_inputs(M, N, K, act, resid)
    y = ops.linear_ex(dev(x), dev(w), dev(b), None if r is None else dev(r), act=act)
    w64, w32 = R.act_run(x, w, b, r, act, torch.float64), R.act_run(x, w, b, r, act, torch.float32)
    check(f"linear_ex act {act} N {N} resid {resid}", {"y": host(y)}, w64, w32, lambda k: K, only=("y",))      # "pre" is the host test's


# ---- D. row statistics -----------------------------------------------------------------------------------------------------------

NORM_CASES = [(kind, recipe, shape, resid) for kind in R.NORM_KINDS for recipe in R.norm_recipes_for(kind) for shape in R.NORM_SHAPES
              for resid in (False, True) if resid or recipe != "cancel"]


@pytest.mark.parametrize("kind,recipe,shape,resid", NORM_CASES)
def test_norms_forward_and_backward(kind, recipe, shape, resid):
    rows, dim = shape
    a = R.norm_recipe(recipe, rows, dim, resid)
    t = {k: dev(v) for k, v in a.items()}
    if kind == "rmsnorm":
        y = ops.rmsnorm(t["x"], t["w"], t.get("resid"))
        dx, dw = ops.rmsnorm_bwd(t["dy"], t["x"], t["w"], t.get("resid"))
        got = {"y": y, "dx": dx, "dw": dw}
    else:
        y = ops.layernorm(t["x"], t["w"], t["b"], t.get("resid")) if kind == "layernorm" else \
            ops.layernorm_post(t["x"], t["w"], t["b"], t.get("resid"), t["post"])
        dx, dw, db = ops.layernorm_bwd(t["dy"], t["x"], t["w"], t.get("resid"))
        got = {"y": y, "dx": dx, "dw": dw, "db": db}
    w64, w32 = R.norm_refs(kind, recipe, rows, dim, resid)
    check(f"{kind} {recipe} {shape} resid {resid}", {k: host(v) for k, v in got.items()}, w64, w32, R.norm_n(rows, dim))


@pytest.mark.parametrize("shape", R.SUBLN_SHAPES)
@pytest.mark.parametrize("recipe", R.SUBLN_RECIPES)
def test_diff_subln(recipe, shape):
    o1, o2, w = R.subln_inputs(recipe, *shape)
    y = ops.diff_subln(dev(o1), dev(o2), dev(w), R.SUBLN_LAM, R.SUBLN_SCALE)
    check(f"diff_subln {recipe} {shape}", {"y": host(y)}, R.subln_run(o1, o2, w, torch.float64), R.subln_run(o1, o2, w, torch.float32),
          lambda k: shape[1])


@pytest.mark.parametrize("shape", R.SUBLN_BWD_SHAPES)
@pytest.mark.parametrize("recipe", R.SUBLN_BWD_RECIPES)
def test_diff_subln_training_forward_and_backward(recipe, shape):
    """amt_diff_subln_train_fwd / amt_diff_subln_bwd with lambda on the device: y is `ops.diff_subln`'s bits; d_o1, d_o2, dw and dlambda
    each at its own scale.  On `constant` o2 is 0 and dlambda exactly 0."""
    o1, o2, w, dy = (dev(a) for a in R.subln_bwd_inputs(recipe, *shape))
    lam = torch.tensor([R.SUBLN_LAM], dtype=torch.float32, device=DEV)
    y = ops.diff_subln_train(o1, o2, w, lam, R.SUBLN_SCALE)
    assert torch.equal(y, ops.diff_subln(o1, o2, w, R.SUBLN_LAM, R.SUBLN_SCALE))
    d_o1, d_o2, dw, dlam = ops.diff_subln_bwd(dy, o1, o2, w, lam, R.SUBLN_SCALE)
    got = {"y": host(y), "d_o1": host(d_o1), "d_o2": host(d_o2), "dw": host(dw), "dlambda": host(dlam)}
    w64, w32 = R.subln_bwd_refs(recipe, *shape)
    check(f"diff_subln backward {recipe} {shape}", got, w64, w32, R.subln_bwd_n(*shape))
    if recipe == "constant":
        assert w64["dlambda"][0] == 0.0 and got["dlambda"][0] == 0.0


# ---- the folded LayerNorm at the mean / std ladder -----------------------------------------------------------------------------

def fold_report(form, m, got, fn, yardstick):
    """Asserts `got` against 8 x the fp32 yardstick's error (floor K U) and prints one FOLD line: per output the kernel's error and the
    folded and unfolded fp32 errors beside it.  With NUMERIC_RANGE_FOLD_JSON set to a path the line also goes into that file
    (profiles/numeric_range_fold.json is written this way)."""
    row = R.fold_row(form, m, got, fn)
    print("FOLD " + json.dumps(row))
    if os.environ.get(R.FOLD_JSON_ENV):
        R.fold_write(os.environ[R.FOLD_JSON_ENV], row)
    check(f"{form} mean/std {m}", got, fn(m, "ref64"), fn(m, yardstick), lambda k: R.FOLD_K)


@pytest.mark.parametrize("m", R.FOLD_LADDER)
def test_folded_decode_attention(m):
    """amt_attn_decode_fold_fwd, called as test_folded_decode_attention_random_sweep calls it, with the new key / value row."""
    f, kc, vc = R.fold_decode_case(m)
    B, H, hd, cap = (R.FOLD_DECODE[k] for k in ("B", "H", "hd", "cap"))
    d, t = H * hd, cap - 1
    D = {k: dev(v) for k, v in f.items()}
    dk, dv = dev(kc), dev(vc)
    o, xo = torch.full((B, d), float("nan"), device=DEV), torch.full((B, d), float("nan"), device=DEV)
    pos = torch.tensor([t], dtype=torch.int32, device=DEV)
    _lib.call("amt_attn_decode_fold_fwd", P(D["raw"]), 3 * d, P(dk), P(dv), None, P(D["u"]), P(D["g"]), P(D["c"]), P(D["gam"]), P(D["bet"]),
              P(xo), P(o), B, H, hd, cap, P(pos), t + 1, 0, 1, 1e-5, hd ** -0.5, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(dk[:, :, :t].cpu(), torch.from_numpy(kc[:, :, :t]))            # only row t of the cache is touched
    got = {"xo": host(xo), "k_new": host(dk[:, :, t]), "v_new": host(dv[:, :, t]), "o": host(o)}
    fold_report("attn_decode_fold", m, got, R.fold_decode_outputs, "folded32")


@pytest.mark.parametrize("m", R.FOLD_LADDER)
def test_folded_ffn_prologue(m):
    """The FoldedFfn prologue of amt_decode_gemm_ex_fwd, as in test_skinny_gemm_two_sources_split_and_folded_ffn_prologue."""
    f, w = R.fold_ffn_case(m)
    B, K1, n_low, n_high = (R.FOLD_FFN[k] for k in ("B", "K1", "n_low", "n_high"))
    K2, K = R.FOLD_K, K1 + R.FOLD_K
    D = {k: dev(v) for k, v in {**f, **w}.items()}
    yl, yh = torch.full((B, n_low), float("nan"), device=DEV), torch.full((B, n_high), float("nan"), device=DEV)
    sl, sh = torch.empty((n_low + 15) // 16 * 16 * K1, device=DEV), torch.empty((n_high + 15) // 16 * 16 * K, device=DEV)
    A = lambda k: _lib.addr(D[k])
    args = _lib.DecodeGemmArgs(x=A("raw"), ldx=K1, x2=A("u"), ldx2=K2, K1=K1, K=K, w_low=A("wl"), bias_low=A("bl"), resid=None, relu=0,
                               w_high=A("wh"), bias_high=A("bh"), n_low=n_low, n_high=n_high, pro=1, fold_g=A("g"), fold_c=A("c"),
                               ln_w=A("gam"), ln_b=A("bet"), y_low=_lib.addr(yl), y_high=_lib.addr(yh), scratch_low=_lib.addr(sl),
                               scratch_high=_lib.addr(sh), B=B, eps=1e-5)
    _lib.call("amt_decode_gemm_ex_fwd", C.byref(args), _lib.stream_ptr())
    torch.cuda.synchronize()
    fold_report("decode_gemm_folded_ffn", m, {"y_low": host(yl), "y_high": host(yh)}, R.fold_ffn_outputs, "folded32")


@pytest.mark.parametrize("m", R.FOLD_LADDER)
def test_decode_linear_with_fused_layernorm(m):
    B, N, K = R.FOLD_LINEAR["B"], R.FOLD_LINEAR["N"], R.FOLD_K
    f = R.fold_inputs(m, B, N, seed=2)
    D = {k: dev(v) for k, v in f.items()}
    y, xn = torch.full((B, N), float("nan"), device=DEV), torch.full((B, K), float("nan"), device=DEV)
    scratch = torch.empty((N + 15) // 16 * 16 * K, device=DEV)
    _lib.call("amt_decode_linear_fwd", P(D["u"]), P(D["W"]), P(D["bW"]), P(D["gam"]), P(D["bet"]), None, P(y), P(xn), P(scratch), B, N, K, 0, 1e-5,
              _lib.stream_ptr())
    torch.cuda.synchronize()
    fold_report("decode_linear_layernorm", m, {"y": host(y), "xn": host(xn)}, R.fold_linear_outputs, "unfolded32")


# ---- saturated gates in the mixture layer and the gated experts ------------------------------------------------------------------

@pytest.mark.parametrize("case", R.MOE_CASES)
def test_moe_with_saturated_router(case):
    """ops.moe_train / ops.moe_bwd through the layer (as tests/test_moe_bwd_gpu.py drives them), and amt_moe_route_fwd alone at k = 2."""
    from tests.test_moe_bwd_gpu import build, run
    n_tok, d, raw, n_exp, k = case
    x, dout, Pm, o64, o32 = R.moe_recipe(*case)
    layer = build((n_tok, d, raw, n_exp, k, True, True), Pm)
    out, grads = run(layer, x, dout)
    idx, wts = layer.last_routing
    assert np.array_equal(idx.reshape(n_tok, k).cpu().numpy(), o64["idx"])
    got = {"out": host(out), "weights": host(wts.reshape(n_tok, k)), **grads}
    check(f"moe gate x100 {case}", got, R.moe_tensors(o64), R.moe_tensors(o32), R.moe_n(n_tok, d, raw, k))
    with torch.no_grad():                                        # the inference forward: the gate epilogue of csrc/gemm_f32.hip (silu_mul)
        out_eval = layer.eval()(dev(x).view(n_tok, 1, d)).reshape(n_tok, d)
    check(f"moe eval forward gate x100 {case}", {"out": host(out_eval)}, R.moe_tensors(o64), R.moe_tensors(o32), R.moe_n(n_tok, d, raw, k),
          only=("out",))
    if k == 2:
        ridx = torch.full((n_tok, 2), -1, dtype=torch.int32, device=DEV)
        rw = torch.full((n_tok, 2), float("nan"), device=DEV)
        xd, gw, gb = dev(x), dev(Pm["gate.weight"]), dev(Pm["gate.bias"])            # named: the device copies stay alive over the call
        _lib.call("amt_moe_route_fwd", P(xd), P(gw), P(gb), P(ridx), P(rw), n_tok, d, n_exp, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(ridx.cpu().numpy(), o64["idx"])
        check(f"moe_route gate x100 {case}", {"weights": host(rw)}, R.moe_tensors(o64), R.moe_tensors(o32), R.moe_n(n_tok, d, raw, k),
              only=("weights",))


@pytest.mark.parametrize("case", R.MOE_CASES)
def test_balanced_moe_with_saturated_router(case):
    """amt_moe_train_fwd_balanced and amt_moe_bwd through a SharedMoELayer that trains its balancing: the experts chosen on
    logits + bias in fp64's order, the weights from the raw logits, the output and every gradient."""
    from tests.test_moe_bwd_gpu import run
    from video2music_amd.model.moe import GLUExpert, SharedMoELayer
    n_tok, d, raw, n_exp, k = case
    x, dout, Pm, bias, o64, o32 = R.moe_biased_recipe(*case)
    layer = SharedMoELayer(GLUExpert(d, raw, dropout=0.0), d, n_experts=n_exp, n_experts_per_token=k, dropout=0.0, balancing=True)
    layer.load_state_dict({**{name: torch.from_numpy(v) for name, v in Pm.items()}, "bias": torch.from_numpy(bias).view(n_exp, 1)}, strict=True)
    layer = layer.to(DEV)
    layer.train_balancing = True
    out, grads = run(layer, x, dout)
    idx, wts = layer.last_routing
    assert np.array_equal(idx.reshape(n_tok, k).cpu().numpy(), o64["idx"])
    got = {"out": host(out), "weights": host(wts.reshape(n_tok, k)), **grads}
    check(f"moe gate x100 biased {case}", got, R.moe_tensors(o64), R.moe_tensors(o32), R.moe_n(n_tok, d, raw, k))


@pytest.mark.parametrize("case", R.GLU_CASES)
def test_glu_with_saturated_gate(case):
    """ops.glu_train / ops.glu_bwd through `autograd.GluFn` (as tests/test_family_train_ops_gpu.py drives them)."""
    from tests.test_family_train_ops_gpu import expert_module, glu_device
    n, d, dff, silu = case
    sd, a = R.glu_recipe(*case)
    e = expert_module(sd, d, dff, silu)
    got = glu_device(e, a, None)
    w64, w32 = R.glu_refs(*case)
    check(f"glu gate x40 {case}", got, w64, w32, lambda k: max(n, dff))
    with torch.no_grad():                                        # ops.glu, the inference path: the gate epilogue of csrc/gemm_f32.hip (silu_mul)
        y_eval = ops.glu(dev(a["x"]), e.eval())
    check(f"glu eval forward gate x40 {case}", {"y": host(y_eval)}, w64, w32, lambda k: max(n, dff), only=("y",))


def test_regression_head_on_slow_decay_weights():
    """VideoRegression('bimamba+').get_feature at S = 129: three 64-row blocks of the forward scan with a state that barely decays."""
    from video2music_amd.model.video_regression import VideoRegression
    sd, sem, emo = R.reg_slow_case()
    m = VideoRegression(**R.REG_SLOW).eval()
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    with torch.no_grad():
        feat = m.get_feature(sem.cuda(), None, None, emo.cuda())
    w64, w32 = R.reg_slow_refs()
    check("VideoRegression bimamba+ slow_decay", {"feature": host(feat)}, w64, w32, lambda k: R.REG_SLOW_BS[1] * 16)
