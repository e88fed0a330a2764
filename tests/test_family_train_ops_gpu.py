"""The operators the V1 / V2 chord models train through (csrc/family_train.hip, csrc/norm_bwd.hip) against the fp64 oracle: `autograd.RopeFn`, `RMSNormFn`,
`GluFn`, and `AttentionFn` with seq-first strides.  Bound per tensor: 8 x e32 (tests/helpers_family_train.py), e32 the same restatement in
float32 on the CPU."""
import numpy as np
import pytest
import torch

from tests import helpers_family_train as FT
from tests.helpers_train_edges import rel_err
from video2music_amd import _lib, autograd as AG, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, grad=False):
    return torch.from_numpy(np.asarray(a)).to(DEV).requires_grad_(grad)


def check(tag, got, r64, r32):
    for k, (err, e32) in FT.op_errors(got, r64, r32).items():
        bound = FT.FACTOR * e32
        print(f"{tag} {k}: err {err:.3e} e32 {e32:.3e} bound {bound:.3e}")
        assert bound <= FT.CAP, (tag, k, bound)
        assert err <= bound, (tag, k, err, e32, bound)


# ---- RopeFn ----
@pytest.mark.parametrize("name", list(FT.ROPE_CASES))
def test_rope_backward(name):
    x, dy, cache = FT.rope_inputs(name)
    y64, dx64 = FT.rope_restated(x, dy, cache, torch.float64)
    y32, dx32 = FT.rope_restated(x, dy, cache, torch.float32)
    xt, c = dev(x, True), cache.to(DEV)
    y = AG.RopeFn.apply(xt, c)
    y.backward(dev(dy))
    dx = xt.grad.cpu().numpy()
    check(name, {"y": y.detach().cpu().numpy(), "dx": dx}, {"y": y64, "dx": dx64}, {"y": y32, "dx": dx32})
    # in place over dy: the same bits
    buf = dev(dy).clone()
    assert ops.rope_bwd(buf, c, out=buf) is buf
    assert np.array_equal(buf.cpu().numpy(), dx)
    # an orthogonal map per pair: |dx| = |dy| to the rounding of cos^2 + sin^2 (2 U) and of three operations per component
    n_dy = (dy.astype(np.float64).reshape(-1, 2) ** 2).sum(1)
    n_dx = (dx.astype(np.float64).reshape(-1, 2) ** 2).sum(1)
    assert np.abs(n_dx - n_dy).max() <= 8 * FT.U * n_dy.max()
    assert np.all(np.abs(n_dx - n_dy) <= 8 * FT.U * n_dy + 1e-30)
    # the un-conjugated rotation is far outside the bound wherever an angle is not 0
    wrong = FT.rope_restated(x, dy, cache, torch.float64, conjugate=False)[1]
    assert rel_err(wrong, dx64) >= FT.MISS * FT.FACTOR * rel_err(dx32, dx64)


def test_rope_bwd_refuses_what_the_forward_refuses():
    x = torch.zeros(2, 4, 1, 32, device=DEV)
    with pytest.raises(_lib.AmtError, match="pairs per position"):
        ops.rope_bwd(x, torch.zeros(4, 24, 2, device=DEV))          # 48 wide: neither 32 nor >= 64
    with pytest.raises(_lib.AmtError, match="bad shape"):
        _lib.call("amt_rope_bwd", _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), 2, 4, 1, 31, 16, None)


# ---- RMSNormFn ----
def test_plan_rule_has_the_boundaries_the_cases_use():
    assert FT.norm_bwd_plan_boundaries() == [16, 17, 2048, 2049]
    assert ops.rmsnorm_bwd_blocks(1) == 1 and ops.rmsnorm_bwd_blocks(2049) == 128


def rms_device(a):
    t = {k: dev(v, k != "dy") for k, v in a.items()}
    y = AG.RMSNormFn.apply(t["x"], t.get("resid"), t["w"], FT.RMS_EPS)
    y.backward(t["dy"])
    out = {k: t[k].grad.cpu().numpy() for k in t if k != "dy"}
    out["y"] = y.detach().cpu().numpy()
    return out


RMS_ROWS = sorted({1, 17, 16, 2048, 2049})


@pytest.mark.parametrize("resid", [False, True])
@pytest.mark.parametrize("dim", [4, 100, 1024])
@pytest.mark.parametrize("rows", RMS_ROWS)
def test_rmsnorm_backward(rows, dim, resid):
    assert set(FT.norm_bwd_plan_boundaries()) <= set(RMS_ROWS)
    a = FT.rms_inputs(rows, dim, resid)
    r64, r32 = FT.rms_restated(a, torch.float64), FT.one_thread(FT.rms_restated, a, torch.float32)
    got, again = rms_device(a), rms_device(a)
    for k in got:
        assert np.array_equal(got[k], again[k]), k                  # fixed summation order: equal bits on repeat
    check(f"rows {rows} dim {dim} resid {resid}", got, r64, r32)
    if resid:
        assert np.array_equal(got["x"], got["resid"])
    # eps 1e-5 in its place would miss the bound: the rows have a mean square of 1e-2
    wrong = FT.rms_restated(a, torch.float64, eps=1e-5)
    assert rel_err(wrong["x"], r64["x"]) >= FT.MISS * FT.FACTOR * rel_err(r32["x"], r64["x"])


@pytest.mark.parametrize("resid", [False, True])
def test_rmsnorm_backward_of_a_row_of_zeros(resid):
    """u = 0: rstd = eps^-1/2 = 1000, dx = 1000 dy w, finite; that row is a thousand times the others, so it is judged on its own."""
    rows, dim, z = 17, 100, 5
    a = FT.rms_inputs(rows, dim, resid, zero_row=z)
    r64, r32, got = FT.rms_restated(a, torch.float64), FT.one_thread(FT.rms_restated, a, torch.float32), rms_device(a)
    assert all(np.isfinite(v).all() for v in got.values())
    want = 1000.0 * a["dy"][z].astype(np.float64) * a["w"].astype(np.float64)
    assert rel_err(r64["x"][z], want) < 1e-9                        # the oracle itself: eps 1e-6
    assert not got["y"][z].any() and not r64["y"][z].any()          # the row's output is zero: nothing to take an error relative to
    rest = np.arange(rows) != z
    check("zero row", *({"x": r["x"][z]} for r in (got, r64, r32)))
    check("other rows", *({k: (v[rest] if k != "w" else v) for k, v in r.items()} for r in (got, r64, r32)))


def test_rmsnorm_bwd_bad_arguments():
    t, w = torch.zeros(4, 32, device=DEV), torch.zeros(32, device=DEV)
    ws = torch.zeros(4 + 128 * 32, device=DEV)
    P = _lib.ptr
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_rmsnorm_bwd", P(t), P(t), None, P(w), P(t), P(w), None, 4, 32, 1e-6, None)
    with pytest.raises(_lib.AmtError, match="dim=30"):
        _lib.call("amt_rmsnorm_bwd", P(t), P(t), None, P(w), P(t), P(w), P(ws), 4, 30, 1e-6, None)
    with pytest.raises(_lib.AmtError, match="dim=1028"):
        _lib.call("amt_rmsnorm_bwd", P(t), P(t), None, P(w), P(t), P(w), P(ws), 4, 1028, 1e-6, None)
    with pytest.raises(_lib.AmtError, match="rows=0"):
        _lib.call("amt_rmsnorm_bwd", P(t), P(t), None, P(w), P(t), P(w), P(ws), 0, 32, 1e-6, None)


# ---- GluFn ----
def expert_module(sd, d, dff, silu):
    from video2music_amd.model.moe import GLUExpert, SiLUExpert
    e = SiLUExpert(d, dff, 0.2) if silu else GLUExpert(d, dff, 0.2)
    e.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return e.to(DEV)


def glu_device(e, a, mask):
    from video2music_amd.model.moe import expert_parts, expert_tensors
    x = dev(a["x"], True)
    parts = expert_parts(e)
    params = [q for name in ("linear1", "gate", "linear2") if parts[name] is not None for q in (parts[name].weight, parts[name].bias)]
    raw = parts["gate"].out_features
    e.zero_grad()
    y = AG.GluFn.apply(x, expert_tensors(e), None if mask is None else dev(mask), raw, *params)
    y.backward(dev(a["dy"]))
    out = {k: v.grad.cpu().numpy() for k, v in e.named_parameters()}
    for k, v in e.named_parameters():
        assert out[k].shape == tuple(v.shape), k                   # the parameters' own widths
    out["x"], out["y"] = x.grad.cpu().numpy(), y.detach().cpu().numpy()
    return out


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("d,dff,silu", [(32, 64, False), (32, 100, False), (32, 64, True), (32, 100, True)])
@pytest.mark.parametrize("n", [1, 128, 129])
def test_glu_forward_and_backward(n, d, dff, silu, masked):
    sd, a, mask = FT.glu_inputs(n, d, dff, silu, masked)
    r64, r32 = FT.glu_restated(sd, a, mask, torch.float64), FT.one_thread(FT.glu_restated, sd, a, mask, torch.float32)
    e = expert_module(sd, d, dff, silu)
    got, again = glu_device(e, a, mask), glu_device(e, a, mask)
    for k in got:
        assert np.array_equal(got[k], again[k]), k
    check(f"n {n} dff {dff} silu {silu} masked {masked}", got, r64, r32)
    if not masked:
        with torch.no_grad():
            assert torch.equal(ops.glu(dev(a["x"]), e.eval()), dev(got["y"]))       # the eval path's bits


def test_glu_mask_in_the_forward_only_is_told_apart():
    sd, a, mask = FT.glu_inputs(129, 32, 100, False, True)
    r64, r32 = FT.glu_restated(sd, a, mask, torch.float64), FT.one_thread(FT.glu_restated, sd, a, mask, torch.float32)
    P = {k: FT.cast(v, torch.float64, True) for k, v in sd.items()}
    x = FT.cast(a["x"], torch.float64, True)
    FT.expert_restated(x, P, "", FT.cast(mask, torch.float64), mask_in_backward=False).backward(FT.cast(a["dy"], torch.float64))
    assert rel_err(x.grad.numpy(), r64["x"]) >= FT.MISS * FT.FACTOR * rel_err(r32["x"], r64["x"])


# ---- AttentionFn with seq-first strides ----
@pytest.mark.parametrize("Lq,Lk,causal,dropped", [(33, 33, True, False), (33, 17, False, True), (129, 129, True, True)])
def test_attention_seq_first_strides_give_the_bits_of_the_transposed_copies(Lq, Lk, causal, dropped):
    B, H, hd = 3, 2, 32
    E = H * hd
    rng = np.random.default_rng(Lq + Lk)
    q, k, v = (rng.standard_normal((L, B, E)).astype(np.float32) for L in (Lq, Lk, Lk))
    dO = rng.standard_normal((Lq, B, E)).astype(np.float32)
    keep = dev((rng.random((B, H, Lq, Lk)) >= 0.2).astype(np.uint8)) if dropped else None
    scale = 1.25 if dropped else 1.0

    def run(seq_first):
        t = [dev(x if seq_first else np.ascontiguousarray(x.transpose(1, 0, 2)), True) for x in (q, k, v)]
        st = AG.lbh_strides(B, H, hd) if seq_first else None
        o = AG.AttentionFn.apply(*t, None, keep, H, causal, hd ** -0.5, scale, 1, st)
        o.backward(dev(dO if seq_first else np.ascontiguousarray(dO.transpose(1, 0, 2))))
        out = [o.detach()] + [x.grad for x in t]
        return [x if seq_first else x.transpose(0, 1) for x in out]

    for name, a, b in zip(("o", "dq", "dk", "dv"), run(True), run(False)):
        assert a.shape == b.shape and torch.equal(a, b), name
