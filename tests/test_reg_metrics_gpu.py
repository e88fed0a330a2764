"""amt_reg_metrics_fwd (csrc/reg_metrics.hip) against the fp64 restatement of tests/helpers_reg_eval.py, within the bounds derived
there; tests/test_reg_eval_host.py shows on the same inputs that the reference's own fp32 expressions meet them."""
import numpy as np
import pytest
import torch

from tests import helpers_reg_eval as H
from video2music_amd import _lib, metrics, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def call(c, rows=True, pad=8, B=None, S=None, W=None, ld=None):
    """The C entry point on a case of `H.make_case`: feat rows strided by W + pad with the padding columns set to 1e4.
    -> clip (B, 4), ln_nd (B, S, 2), inst (B, S, 40) device tensors (None without `rows`)."""
    Bv, Sv, Wv = c["feat"].shape
    feat = torch.full((Bv, Sv, Wv + pad), 1.0e4, device=DEV)
    feat[:, :, :Wv] = torch.from_numpy(c["feat"]).to(DEV)
    heads = torch.from_numpy(H.pack_heads(c["reg_w"], c["reg_b"], c["cls_w"], c["cls_b"])).to(DEV)
    nd, lo, inst_t = (torch.from_numpy(c[k]).to(DEV).contiguous() for k in ("note_density", "loudness", "instrument"))
    clip = torch.full((Bv, 4), -7.0, device=DEV)
    ln_nd = torch.full((Bv, Sv, 2), -7.0, device=DEV) if rows else None
    inst = torch.full((Bv, Sv, 40), -7.0, device=DEV) if rows else None
    _lib.call("amt_reg_metrics_fwd", _lib.ptr(feat), Wv + pad if ld is None else ld, Wv if W is None else W, _lib.ptr(heads), _lib.ptr(nd),
              _lib.ptr(lo), _lib.ptr(inst_t), Bv if B is None else B, Sv if S is None else S, _lib.ptr(clip), _lib.ptr(ln_nd),
              _lib.ptr(inst), _lib.stream_ptr())
    torch.cuda.synchronize()
    return clip, ln_nd, inst


def check(got, want, tag):
    clip, ln_nd, inst = got
    clip = clip.cpu().numpy().astype(np.float64)
    err = np.abs(clip - want["clip"])
    print(tag, "max error / bound (sse_nd, sse_l, bce)", (err[:, :3] / want["bound"][:, :3]).max(axis=0))
    assert (err <= want["bound"]).all(), (clip, want["clip"], want["bound"])
    if ln_nd is not None:
        assert (np.abs(ln_nd.cpu().numpy() - want["ln_nd"]) <= want["d_ln_nd"]).all()
        assert (np.abs(inst.cpu().numpy().astype(np.float64) - want["p32"]) <= want["d_z"] / 4 + 4 * H.U).all()    # |dp / dz| <= 1/4


@pytest.mark.parametrize("B,S,W", H.KERNEL_CASES)
def test_kernel_equals_fp64_restatement(B, S, W):
    c = H.make_case(B, S, W)
    want = H.restate(**c)
    assert np.abs(want["z"]).max() <= H.Z_MAX
    assert (want["clip"][:, 3] == S).all()
    check(call(c), want, f"B {B} S {S} W {W}")


def test_more_rows_than_one_ordered_pass_holds():
    """S = 1030: the per-row sums of a clip wait in LDS 1024 rows at a time."""
    c = H.make_case(1, 1030, 40)
    check(call(c), H.restate(**c), "S 1030")


def test_saturated_probabilities_give_the_clamped_terms():
    """Clip 0 is planted through a one-hot feature column and chosen classifier weights: row 0 has z = +40 with target 0 and z = -120
    with target 1 (each term exactly 100: p rounds to 1 / 0 in fp32 and the log is clamped at -100) and z = +40 with target 1 on its
    37 other outputs (exactly 0); row 1 has z = +40 with target 0 twice and z = -120 with target 0 elsewhere (200 again).  The clip's
    BCE sum is exactly 400.  Clip 1 holds ordinary rows, checked to the bound.  Every logit is +40, -120 or within +-6, so none lies
    in (8, 25), where 1 - p is a few ulps of noise in the reference itself, or in (-104, -80), where p is denormal and
    flush-to-zero decides the result."""
    W = 8
    c = H.make_case(2, 2, W, seed=77)
    c["feat"][:, :, :2] = 0.0
    c["feat"][0] = 0.0
    c["feat"][0, 0, 0] = c["feat"][0, 1, 1] = 1.0
    c["cls_b"][:] = 0.0
    c["cls_w"][:, 0], c["cls_w"][:, 1] = 40.0, -120.0
    c["cls_w"][1, 0] = -120.0
    c["cls_w"][[4, 9], 1] = 40.0
    c["instrument"][0, 0], c["instrument"][0, 1] = 1.0, 0.0
    c["instrument"][0, 0, 0] = 0.0
    want = H.restate(**c)
    z = want["z"]
    assert z[0, 0].tolist() == [40.0, -120.0] + [40.0] * 38 and sorted(set(z[0, 1].tolist())) == [-120.0, 40.0]
    assert np.abs(z[1]).max() <= H.Z_MAX
    assert want["terms"][0, 0].tolist() == [100.0, 100.0] + [0.0] * 38 and want["clip"][0, 2] == 400.0
    clip, ln_nd, inst = call(c)
    assert float(clip[0, 2]) == 400.0
    assert np.array_equal(inst[0].cpu().numpy(), (z[0] > 0).astype(np.float32))          # p is exactly 1 or 0
    got = clip.cpu().numpy().astype(np.float64)
    assert (np.abs(got[1] - want["clip"][1]) <= want["bound"][1]).all() and np.isfinite(want["bound"][1]).all()
    assert (np.abs(got[0, :2] - want["clip"][0, :2]) <= want["bound"][0, :2]).all()


def test_calls_are_deterministic_and_optional_outputs_do_not_change_the_sums():
    c = H.make_case(3, 300, 128)
    a, b, n = call(c), call(c), call(c, rows=False)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert n[1] is None and n[2] is None and torch.equal(a[0], n[0])


def test_wrapper_takes_the_module_and_strided_rows():
    from video2music_amd.model.video_regression import VideoRegression
    c = H.make_case(2, 37, 128)
    m = VideoRegression(n_layers=1, d_model=64, d_hidden=64, total_vf_dim=30, regModel="bilstm").to(DEV).eval()
    with torch.no_grad():
        m.regressor.weight.copy_(torch.from_numpy(c["reg_w"]))
        m.regressor.bias.copy_(torch.from_numpy(c["reg_b"]))
        m.classifier[0].weight.copy_(torch.from_numpy(c["cls_w"]))
    stale = m.packed_heads()
    with torch.no_grad():
        m.classifier[0].bias.copy_(torch.from_numpy(c["cls_b"]))           # a parameter changes: the packed copy is rebuilt
    heads = m.packed_heads()
    assert heads is not stale and heads is m.packed_heads()
    assert np.array_equal(heads.cpu().numpy(), H.pack_heads(c["reg_w"], c["reg_b"], c["cls_w"], c["cls_b"]))
    wide = torch.zeros(2, 37, 192, device=DEV)
    wide[:, :, :128] = torch.from_numpy(c["feat"]).to(DEV)
    r = metrics.regression_metrics(m, wide[:, :, :128], c["note_density"], c["loudness"], c["instrument"], return_rows=True)
    check((torch.stack([r[k] for k in metrics.REG_FIELDS], dim=1), r["ln_nd"], r["inst"]), H.restate(**c), "wrapper")
    assert ops.REG_METRIC_FIELDS == H.FIELDS


def test_bad_arguments_raise():
    c = H.make_case(1, 5, 16)
    with pytest.raises(_lib.AmtError, match="multiple of 8"):
        call(c, W=12)
    with pytest.raises(_lib.AmtError, match="multiple of 8"):
        call(c, W=1032, ld=1040)
    with pytest.raises(_lib.AmtError, match="row stride"):
        call(c, ld=8)
    with pytest.raises(_lib.AmtError, match="positive"):
        call(c, B=0)
    with pytest.raises(_lib.AmtError, match="positive"):
        call(c, S=0)
    f = torch.zeros(5, 16, device=DEV)
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_reg_metrics_fwd", _lib.ptr(f), 16, 16, None, None, None, None, 1, 5, None, None, None, _lib.stream_ptr())
