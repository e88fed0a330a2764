"""amt_chord_loss_aux_fwd_bwd (csrc/chord_aux_loss.hip) against the fp64 restatement of tests/helpers_chord_aux.py, differentiated by
torch's CPU autograd, in both layouts of the auxiliary rows.  tests/test_chord_aux_host.py holds that restatement to the reference's
own classes and asserts, on these very inputs, that every valid auxiliary row stays 1e-4 (in the logits) from a tie at the top-k
border and 2e-5 from the hinge's kink: away from the two places where the gradient jumps.

Bounds, as tests/test_chord_loss_gpu.py sets them.  Per-clip sums (ce, bce, a_3, a_5): `helpers_eval.loss_bound(L, value)`, a
159-term tree inside a row followed by a sum over the clip's L rows.  The losses: those bounds carried through the quotients (an
auxiliary term also through its weight, chord through 1 / count), plus 4 U of the value for the divisions and the combination.
dlogits: max|g - g64| / max|g64| <= max(8 e32, 159 U), e32 torch's own fp32 CPU autograd of the restatement on the same inputs against
fp64 -- never measured against the kernel.  n_valid and count are exact."""
import numpy as np
import pytest
import torch

from tests import helpers_chord_aux as H
from tests import helpers_eval as HE
from video2music_amd import _lib, losses, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NC, U = H.NC, H.U
W = (0.4, 0.6)
CASES = [(B, L, layout, ld, eps) for (B, L) in H.SHAPES for layout in H.LAYOUTS for ld in (159, 160) for eps in (0.0, 0.1)]


def run_kernel(y, tgt, emo, w, eps, layout):
    """Two full calls and a forward-only one: bit-equal; returns the first's (loss (7,), clip (B, 6), dlogits) as float64 arrays."""
    yd, td, ed = torch.from_numpy(y).to(DEV), torch.from_numpy(tgt).to(DEV), torch.from_numpy(emo).to(DEV)
    loss, clip, dlogits = ops.chord_loss_aux(yd, td, ed, w[0], w[1], eps, layout)
    loss2, clip2, dlogits2 = ops.chord_loss_aux(yd, td, ed, w[0], w[1], eps, layout)
    loss3, clip3, none = ops.chord_loss_aux(yd, td, ed, w[0], w[1], eps, layout, backward=False)
    assert torch.equal(loss, loss2) and torch.equal(clip, clip2) and torch.equal(dlogits, dlogits2)      # fixed summation order
    assert none is None and torch.equal(loss, loss3) and torch.equal(clip, clip3)                      # forward only: the same bits
    assert loss.shape == (7,) and clip.shape == (tgt.shape[0], 6) and dlogits.shape == tgt.shape + (NC,)
    return loss.cpu().numpy().astype(np.float64), clip.cpu().numpy().astype(np.float64), dlogits.cpu().numpy().astype(np.float64)


def check(tag, got, w64, w32, w, L):
    loss, clip, dlogits = got
    want, B = w64["clip"], w64["clip"].shape[0]
    assert np.array_equal(clip[:, 0], want[:, 0]) and np.array_equal(clip[:, 3], want[:, 3])           # n_valid, L
    assert loss[6] == w64["loss"][6], ("count", loss[6], w64["loss"][6])
    b = {}
    for name, col in (("ce", 1), ("bce", 2), ("a3", 4), ("a5", 5)):
        b[name] = HE.loss_bound(L, want[:, col])
        err = np.abs(clip[:, col] - want[:, col])
        print(f"{tag}: clip {name} err/bound {np.max(err / b[name]):.3f}")
        assert (err <= b[name]).all(), name
    n_valid, count, wl = want[:, 0].sum(), w64["loss"][6], w64["loss"]
    b_ce = b["ce"].sum() / n_valid + 4 * U * abs(wl[3])
    b_a3 = 3.0 * b["a3"].sum() / n_valid + 4 * U * abs(wl[4])
    b_a5 = 5.0 * b["a5"].sum() / n_valid + 4 * U * abs(wl[5])
    b_chord = (b_ce + b_a3 + b_a5) / count + 4 * U * abs(wl[1])
    b_emo = b["bce"].sum() / (B * L * NC) + 4 * U * abs(wl[2])
    bounds = [w[0] * b_chord + w[1] * b_emo + 4 * U * abs(wl[0]), b_chord, b_emo, b_ce, b_a3, b_a5]
    for i, name in enumerate(("total", "chord", "emotion", "ce", "aux3", "aux5")):
        print(f"  {name}: {loss[i]:.7f} fp64 {wl[i]:.7f} err/bound {abs(loss[i] - wl[i]) / bounds[i]:.3f}")
        assert abs(loss[i] - wl[i]) <= bounds[i], name
    err, e32 = H.rel_err(dlogits, w64["dlogits"]), H.rel_err(w32["dlogits"], w64["dlogits"])
    print(f"  dlogits err {err:.3e} torch32 {e32:.3e}")
    assert err <= max(8 * e32, NC * U)


@pytest.mark.parametrize("B,L,layout,ld,eps", CASES)
def test_kernel_equals_fp64(B, L, layout, ld, eps):
    y, tgt, emo = H.make_case(B, L, ld)                     # NaN in the padding column of ld = 160
    w64, w32 = H.reference(B, L, eps, W, layout)
    check(f"B {B} L {L} {layout} ld {ld} eps {eps}", run_kernel(y, tgt, emo, W, eps, layout), w64, w32, W, L)


@pytest.mark.parametrize("layout", H.LAYOUTS)
@pytest.mark.parametrize("w", [(0.4, 0.6), (1.0, 0.0), (0.0, 1.0)])
def test_weights(w, layout):
    """-drop_loss's three weightings; (1, 0) leaves the chord part alone in total and dlogits, (0, 1) the emotion part."""
    B, L = 2, 65
    y, tgt, emo = H.make_case(B, L, 160)
    w64, w32 = H.reference(B, L, 0.1, w, layout)
    got = run_kernel(y, tgt, emo, w, 0.1, layout)
    check(f"weights {w} {layout}", got, w64, w32, w, L)
    if 0.0 in w:
        assert got[0][0] == got[0][1 if w[0] else 2]           # the dropped term leaves no trace in the total


@pytest.mark.parametrize("layout", H.LAYOUTS)
@pytest.mark.parametrize("count", [3, 2, 1])
def test_count_regimes(count, layout):
    """The divisor of the chord part takes each of its three values; with count = 1 both hinges are inactive everywhere and the
    gradient is the plain loss kernel's."""
    B, L = H.REGIME_SHAPE
    y, tgt, emo = H.regime_case(count, layout, 160)
    w64, w32 = H.reference(B, L, 0.1, W, layout, count)
    assert w64["loss"][6] == count
    got = run_kernel(y, tgt, emo, W, 0.1, layout)
    check(f"count {count} {layout}", got, w64, w32, W, L)
    if count == 2:
        assert got[0][4] > 0.2 and got[0][5] == 0.0
    if count == 1:
        assert got[0][4] == 0.0 and got[0][5] == 0.0
        _, _, plain = ops.chord_loss(torch.from_numpy(y).to(DEV), torch.from_numpy(tgt).to(DEV), torch.from_numpy(emo).to(DEV), W[0], 0.1)
        e32 = H.rel_err(w32["dlogits"], w64["dlogits"])
        assert H.rel_err(got[2], plain.cpu().numpy()) <= max(8 * e32, NC * U)


@pytest.mark.parametrize("layout,ld,eps", [("view", 159, 0.1), ("rows", 160, 0.0), ("view", 160, 0.0)])
def test_chord_train_loss_backward_reaches_the_logits(layout, ld, eps):
    """losses.chord_train_loss(auxiliary=True) on a leaf: its .grad is the kernel's dlogits times the incoming gradient, zero past the
    159 classes."""
    B, L = 2, 39
    y, tgt, emo = H.make_case(B, L, ld)
    y[..., NC:] = 0.0
    yd = torch.from_numpy(y).to(DEV).requires_grad_(True)
    loss = losses.chord_train_loss(yd, torch.from_numpy(tgt), torch.from_numpy(emo), W[0], eps, auxiliary=True, layout=layout)
    assert loss.requires_grad and loss.dim() == 0
    (2.0 * loss).backward()
    w64, w32 = H.reference(B, L, eps, W, layout)
    assert abs(float(loss) - w64["loss"][0]) <= 1e-5 * abs(w64["loss"][0])
    assert H.rel_err(yd.grad[..., :NC].cpu().numpy(), 2.0 * w64["dlogits"]) <= max(8 * H.rel_err(w32["dlogits"], w64["dlogits"]), NC * U)
    assert not yd.grad[..., NC:].any()
    # the default layout is the training one, and the plain call is ChordLossFn's, bit for bit
    d = losses.chord_train_loss(yd.detach(), torch.from_numpy(tgt), torch.from_numpy(emo), W[0], eps, auxiliary=True)
    v = losses.chord_train_loss(yd.detach(), torch.from_numpy(tgt), torch.from_numpy(emo), W[0], eps, auxiliary=True, layout="view")
    assert torch.equal(d, v)
    plain = ops.chord_loss(yd.detach(), torch.from_numpy(tgt).to(DEV), torch.from_numpy(emo).to(DEV), W[0], eps, backward=False)[0][0]
    assert torch.equal(losses.chord_train_loss(yd.detach(), torch.from_numpy(tgt), torch.from_numpy(emo), W[0], eps), plain)
    with pytest.raises(ValueError, match="layout"):
        ops.chord_loss_aux(yd.detach(), torch.from_numpy(tgt).to(DEV), torch.from_numpy(emo).to(DEV), 0.4, 0.6, eps, "columns")
    with pytest.raises(ValueError, match="without auxiliary"):
        losses.chord_train_loss(yd.detach(), torch.from_numpy(tgt), torch.from_numpy(emo), W[0], eps, weights=(0.5, 0.7))


def test_bad_arguments():
    y = torch.zeros(2, 3, 159, device=DEV)
    t = torch.zeros(2, 3, dtype=torch.int64, device=DEV)
    e = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    out = torch.zeros(64, device=DEV)
    ws = torch.zeros(4 + 12 + 2 * 6 * 159, device=DEV)
    P = _lib.ptr
    name = "amt_chord_loss_aux_fwd_bwd"
    assert _lib.call("amt_chord_loss_aux_ws_floats", 2, 3) == 4 + 12 + 2 * 2 * 3 * 159              # five sums per workgroup, padded to 4
    assert _lib.call("amt_chord_loss_aux_ws_floats", 3, 299) == 4 + 76 + 2 * 3 * 299 * 159
    assert _lib.call("amt_chord_loss_aux_ws_floats", 0, 3) == 0
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call(name, P(y), 159, P(t), P(e), 2, 3, 0.4, 0.6, 0.0, 1, P(out), P(out), None, None, None)
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call(name, P(y), 159, None, P(e), 2, 3, 0.4, 0.6, 0.0, 1, P(out), P(out), None, P(ws), None)
    with pytest.raises(_lib.AmtError, match="row stride 158"):
        _lib.call(name, P(y), 158, P(t), P(e), 2, 3, 0.4, 0.6, 0.0, 1, P(out), P(out), None, P(ws), None)
    with pytest.raises(_lib.AmtError, match="smoothing"):
        _lib.call(name, P(y), 159, P(t), P(e), 2, 3, 0.4, 0.6, 1.0, 0, P(out), P(out), None, P(ws), None)
    with pytest.raises(_lib.AmtError, match="2\\^24"):
        _lib.call(name, P(y), 159, P(t), P(e), 1024, 299, 0.4, 0.6, 0.0, 0, P(out), P(out), None, P(ws), None)
    with pytest.raises(_lib.AmtError, match="layout=2"):
        _lib.call(name, P(y), 159, P(t), P(e), 2, 3, 0.4, 0.6, 0.0, 2, P(out), P(out), None, P(ws), None)
    with pytest.raises(_lib.AmtError, match="must be positive"):
        _lib.call(name, P(y), 159, P(t), P(e), 2, 0, 0.4, 0.6, 0.0, 0, P(out), P(out), None, P(ws), None)
