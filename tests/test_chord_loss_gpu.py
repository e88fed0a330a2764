"""amt_chord_loss_fwd_bwd (csrc/chord_loss.hip) against torch's CPU autograd in fp64 on the two loss expressions of the reference's
train_epoch (utilities/run_model_vevo.py:101-119):

    lambda CrossEntropyLoss(ignore_index=CHORD_PAD, label_smoothing=eps)(y, tgt) + (1 - lambda) BCEWithLogitsLoss()(y, tgt_emotion)

Bounds.  Per-clip sums: `helpers_eval.loss_bound(L, value)`, the worst case of a 159-term tree inside a row followed by a sum over
the clip's L rows.  The three losses: the clips' bounds through the two quotients, plus 4 U of the value for the divisions and the
final combination.  dlogits: the bound of tests/test_rnn_train_gpu.py, err = max|g - g64| / max|g64| <= max(8 err_torch32, n 2^-24)
with err_torch32 torch's own fp32 CPU autograd on the same inputs and n = 159, the softmax normaliser's length."""
import numpy as np
import pytest
import torch

from tests import helpers_eval as HE
from tests.helpers_reg_train import U, rel_err
from video2music_amd import _lib, losses, ops
from video2music_amd.utilities import constants as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAM = 0.4
NC = C.CHORD_SIZE
CASES = [(B, L, ld, eps) for (B, L) in ((1, 1), (2, 39), (3, 299)) for ld in (159, 160) for eps in (0.0, 0.1)]


def make_case(B, L, ld):
    """Logits 3 N(0, 1) with a boosted target on every third row; targets over the whole vocabulary with an END, trailing PADs, an id
    outside the vocabulary, a clip that is all PAD next to valid ones (B > 1) and emotion classes outside 0..5.  Columns past 159 hold
    NaN: they take no part."""
    rng = np.random.default_rng(100 * B + L)
    tgt = rng.integers(0, C.CHORD_END, size=(B, L))
    emo = rng.integers(0, 6, size=(B, L))
    if L > 1:
        tgt[0, L - L // 4:] = C.CHORD_PAD
        tgt[0, L - L // 4 - 1] = C.CHORD_END
        tgt[0, 1] = 400                                     # outside the vocabulary: ignored like PAD
        emo[0, 0], emo[0, 2] = -1, 7                        # outside 0..5: no quality accepted
    if B > 1:
        tgt[1, :] = C.CHORD_PAD
    y = np.full((B, L, ld), np.nan, dtype=np.float32)
    y[..., :NC] = 3 * rng.standard_normal((B, L, NC))
    safe = np.where(tgt < NC, tgt, 0)
    boost = np.zeros((B, L), dtype=np.float32)
    boost[:, ::3] = 6
    np.put_along_axis(y[..., :NC], safe[..., None], np.take_along_axis(y[..., :NC], safe[..., None], -1) + boost[..., None], -1)
    return y, tgt.astype(np.int64), emo.astype(np.int32)


def torch_cpu(y, tgt, emo, eps, dtype):
    """The reference's expressions on the CPU; ids outside the vocabulary read as PAD and classes outside 0..4 as neutral, as
    include/amt_hip.h documents.  Returns the three losses, the per-clip sums and dlogits."""
    B, L = tgt.shape
    t = np.where((tgt >= 0) & (tgt < NC), tgt, C.CHORD_PAD)
    e = np.where((emo >= 0) & (emo < 5), emo, 5)
    rows = torch.from_numpy(HE.emotion_rows(t, e)).to(dtype).reshape(B * L, NC)
    yt = torch.from_numpy(y[..., :NC].copy()).to(dtype).reshape(B * L, NC).requires_grad_(True)
    tt = torch.from_numpy(t).reshape(B * L)
    ce = torch.nn.CrossEntropyLoss(ignore_index=C.CHORD_PAD, label_smoothing=eps)
    chord, emotion = ce(yt, tt), torch.nn.BCEWithLogitsLoss()(yt, rows)
    total = LAM * chord + (1 - LAM) * emotion
    total.backward()
    with torch.no_grad():
        ce_rows = torch.nn.CrossEntropyLoss(ignore_index=C.CHORD_PAD, label_smoothing=eps, reduction="none")(yt, tt).reshape(B, L)
        bce_rows = torch.nn.BCEWithLogitsLoss(reduction="none")(yt, rows).reshape(B, L, NC)
    valid = (t != C.CHORD_PAD)
    clip = np.stack([valid.sum(1), ce_rows.numpy().sum(1), bce_rows.numpy().sum((1, 2)), np.full(B, L)], axis=1).astype(np.float64)
    return {"loss": np.array([float(total), float(chord), float(emotion)]), "clip": clip, "dlogits": yt.grad.numpy().reshape(B, L, NC)}


@pytest.mark.parametrize("B,L,ld,eps", CASES)
def test_kernel_equals_torch_fp64(B, L, ld, eps):
    y, tgt, emo = make_case(B, L, ld)
    w64, w32 = torch_cpu(y, tgt, emo, eps, torch.float64), torch_cpu(y, tgt, emo, eps, torch.float32)
    yd, td, ed = torch.from_numpy(y).to(DEV), torch.from_numpy(tgt).to(DEV), torch.from_numpy(emo).to(DEV)
    loss, clip, dlogits = ops.chord_loss(yd, td, ed, LAM, eps)
    loss2, clip2, dlogits2 = ops.chord_loss(yd, td, ed, LAM, eps)
    loss3, clip3, none = ops.chord_loss(yd, td, ed, LAM, eps, backward=False)
    assert torch.equal(loss, loss2) and torch.equal(clip, clip2) and torch.equal(dlogits, dlogits2)      # fixed summation order
    assert none is None and torch.equal(loss, loss3) and torch.equal(clip, clip3)                      # forward only: the same bits
    clip, loss = clip.cpu().numpy().astype(np.float64), loss.cpu().numpy().astype(np.float64)

    want = w64["clip"]
    assert np.array_equal(clip[:, 0], want[:, 0]) and np.array_equal(clip[:, 3], want[:, 3])
    b_ce, b_bce = HE.loss_bound(L, want[:, 1]), HE.loss_bound(L, want[:, 2])
    print(f"B {B} L {L} ld {ld} eps {eps}: clip ce err/bound {np.max(np.abs(clip[:, 1] - want[:, 1]) / b_ce):.3f}, "
          f"bce {np.max(np.abs(clip[:, 2] - want[:, 2]) / b_bce):.3f}")
    assert (np.abs(clip[:, 1] - want[:, 1]) <= b_ce).all() and (np.abs(clip[:, 2] - want[:, 2]) <= b_bce).all()
    assert clip[1, 1] == 0.0 if B > 1 else True                                                        # the all-PAD clip

    n_valid = want[:, 0].sum()
    b_chord = b_ce.sum() / n_valid + 4 * U * abs(w64["loss"][1])
    b_emo = b_bce.sum() / (B * L * NC) + 4 * U * abs(w64["loss"][2])
    bounds = [LAM * b_chord + (1 - LAM) * b_emo + 4 * U * abs(w64["loss"][0]), b_chord, b_emo]
    for i, name in enumerate(("total", "chord", "emotion")):
        print(f"  {name}: {loss[i]:.7f} fp64 {w64['loss'][i]:.7f} err/bound {abs(loss[i] - w64['loss'][i]) / bounds[i]:.3f}")
        assert abs(loss[i] - w64["loss"][i]) <= bounds[i], name

    err, e32 = rel_err(dlogits.cpu().numpy(), w64["dlogits"]), rel_err(w32["dlogits"], w64["dlogits"])
    print(f"  dlogits err {err:.3e} torch32 {e32:.3e}")
    assert err <= max(8 * e32, NC * U)

    if eps == 0.0:                                          # the evaluation's kernel forms the same per-clip cross-entropy sum
        m = ops.chord_metrics(yd, td, ed, torch.ones(B, L, device=DEV), 0.8).cpu().numpy().astype(np.float64)
        assert (np.abs(m[:, 5] - clip[:, 1]) <= b_ce).all() and np.array_equal(m[:, 0], clip[:, 0])
        assert (np.abs(m[:, 6] - clip[:, 2]) <= b_bce).all()


@pytest.mark.parametrize("ld,eps", [(159, 0.1), (160, 0.0)])
def test_chord_train_loss_backward_reaches_the_logits(ld, eps):
    """losses.chord_train_loss on a leaf: its .grad is the kernel's dlogits times the incoming gradient, zero past the 159 classes."""
    B, L = 2, 39
    y, tgt, emo = make_case(B, L, ld)
    y[..., NC:] = 0.0
    yd = torch.from_numpy(y).to(DEV).requires_grad_(True)
    loss = losses.chord_train_loss(yd, torch.from_numpy(tgt), torch.from_numpy(emo), LAM, eps)
    assert loss.requires_grad and loss.dim() == 0
    (2.0 * loss).backward()
    want = torch_cpu(y, tgt, emo, eps, torch.float64)
    assert abs(float(loss) - want["loss"][0]) <= 1e-5 * abs(want["loss"][0])
    assert rel_err(yd.grad[..., :NC].cpu().numpy(), 2.0 * want["dlogits"]) <= NC * U
    assert not yd.grad[..., NC:].any()
    # torch's own two expressions on device logits give the same gradient to rounding
    yt = torch.from_numpy(y[..., :NC].copy()).to(DEV).requires_grad_(True)
    t = np.where((tgt >= 0) & (tgt < NC), tgt, C.CHORD_PAD)
    rows = torch.from_numpy(HE.emotion_rows(t, np.where((emo >= 0) & (emo < 5), emo, 5))).float().to(DEV)
    tl = LAM * torch.nn.CrossEntropyLoss(ignore_index=C.CHORD_PAD, label_smoothing=eps)(yt.reshape(-1, NC), torch.from_numpy(t).to(DEV).reshape(-1)) \
        + (1 - LAM) * torch.nn.BCEWithLogitsLoss()(yt, rows)
    (2.0 * tl).backward()
    assert rel_err(yd.grad[..., :NC].cpu().numpy(), yt.grad.cpu().numpy()) <= 2 * NC * U


def test_bad_arguments():
    y = torch.zeros(2, 3, 159, device=DEV)
    t = torch.zeros(2, 3, dtype=torch.int64, device=DEV)
    e = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    out = torch.zeros(64, device=DEV)
    P = _lib.ptr
    assert _lib.call("amt_chord_loss_ws_floats", 2, 3) == 4 + 3 * 2 and _lib.call("amt_chord_loss_ws_floats", 3, 299) == 4 + 3 * 3 * 5
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_chord_loss_fwd_bwd", P(y), 159, P(t), P(e), 2, 3, 0.4, 0.0, P(out), P(out), None, None, None)
    with pytest.raises(_lib.AmtError, match="row stride 158"):
        _lib.call("amt_chord_loss_fwd_bwd", P(y), 158, P(t), P(e), 2, 3, 0.4, 0.0, P(out), P(out), None, P(out), None)
    with pytest.raises(_lib.AmtError, match="smoothing"):
        _lib.call("amt_chord_loss_fwd_bwd", P(y), 159, P(t), P(e), 2, 3, 0.4, 1.0, P(out), P(out), None, P(out), None)
    with pytest.raises(_lib.AmtError, match="2\\^24"):
        _lib.call("amt_chord_loss_fwd_bwd", P(y), 159, P(t), P(e), 1024, 299, 0.4, 0.0, P(out), P(out), None, P(out), None)
