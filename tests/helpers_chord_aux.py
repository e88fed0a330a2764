"""Test infrastructure of the auxiliary chord loss (reference train.py:221-229, model/loss.py:85-141): a torch restatement that runs
on the CPU in fp64 or fp32 and is differentiated by torch's autograd, the inputs of the kernel tests, and `unview`.  Nothing under
video2music_amd/ imports it, and it imports nothing of the kernel's.

    chord = (CE + A_3 + A_5) / count,  A_k = w_k sum_{valid rows} relu(mean(top-k of softmax(z)) - softmax(z)_t) / n_valid
    total = w_chord chord + w_emotion BCEWithLogitsLoss()(y, tgt_emotion)

count: how many of the three terms exceed 1e-10, a constant under differentiation.  The auxiliary row (b, r) is logits[b, r, :] in the
"rows" layout (eval_model's call) and, in the "view" layout (train_epoch's call, `y.permute(0, 2, 1)` RESHAPED to (B, L, 159)), the
159 consecutive elements from 159 r of the clip's class-major flattening; both pair with tgt[b, r]."""
import functools

import numpy as np
import torch

from tests import helpers_eval as HE
from video2music_amd.utilities import constants as C

NC = C.CHORD_SIZE
U = 2.0 ** -24
TERMS = ((3, 3.0), (5, 5.0))                   # (k, w_k): train.py:227-228
COUNT_FLOOR = 1e-10
LAYOUTS = ("rows", "view")
# the shapes of the kernel tests (seed 100 B + L of `make_case`): L = 1, 2 -- a view row spans many class columns; 39; 64 / 65 -- a
# workgroup's row block; 158 / 159 / 160 -- at 159 view row r is class column r; 299 -- the training length, five row blocks per clip
SHAPES = ((1, 1), (2, 1), (3, 2), (2, 39), (3, 64), (2, 65), (2, 158), (2, 159), (3, 159), (2, 160), (3, 299))
MIN_GAP, MIN_MARGIN = 1e-4, 2e-5               # what every case keeps from the two places where the gradient jumps
REGIME_SHAPE = (2, 65)


def aux_rows(y, layout):
    """The auxiliary rows (B, L, 159) of logits y (B, L, 159), torch or numpy."""
    assert layout in LAYOUTS
    B, L, n = y.shape
    if layout == "rows":
        return y
    return (y.permute(0, 2, 1) if isinstance(y, torch.Tensor) else y.transpose(0, 2, 1)).reshape(B, L, n)


def unview(z):
    """The y (B, L, 159) whose view-layout auxiliary rows are z (B, L, 159)."""
    B, L, n = z.shape
    z = z.reshape(B, n, L)
    return (z.permute(0, 2, 1) if isinstance(z, torch.Tensor) else z.transpose(0, 2, 1))


def clean_targets(tgt, emo):
    """Ids outside the vocabulary read as PAD and classes outside 0..4 as neutral, as include/amt_hip.h documents."""
    return np.where((tgt >= 0) & (tgt < NC), tgt, C.CHORD_PAD), np.where((emo >= 0) & (emo < 5), emo, 5)


def make_case(B, L, ld=NC):
    """The recipe of tests/test_chord_loss_gpu.py::make_case, restated here because test modules are not imported: logits 3 N(0, 1)
    with a boosted target on every third row; an END, trailing PADs, an id outside the vocabulary, an all-PAD clip (B > 1), emotion
    classes outside 0..5; NaN past column 159."""
    rng = np.random.default_rng(100 * B + L)
    tgt = rng.integers(0, C.CHORD_END, size=(B, L))
    emo = rng.integers(0, 6, size=(B, L))
    if L > 1:
        tgt[0, L - L // 4:] = C.CHORD_PAD
        tgt[0, L - L // 4 - 1] = C.CHORD_END
        tgt[0, 1] = 400
        emo[0, 0], emo[0, min(2, L - 1)] = -1, 7                # L = 2 has no third second: the same draws, one slot nearer
    if B > 1:
        tgt[1, :] = C.CHORD_PAD
    y = np.full((B, L, ld), np.nan, dtype=np.float32)
    y[..., :NC] = 3 * rng.standard_normal((B, L, NC))
    safe = np.where(tgt < NC, tgt, 0)
    boost = np.zeros((B, L), dtype=np.float32)
    boost[:, ::3] = 6
    np.put_along_axis(y[..., :NC], safe[..., None], np.take_along_axis(y[..., :NC], safe[..., None], -1) + boost[..., None], -1)
    return y, tgt.astype(np.int64), emo.astype(np.int32)


def regime_case(count, layout, ld=NC):
    """Inputs on which `count` is 3, 2 or 1, of shape REGIME_SHAPE with `make_case`'s targets.  3: `make_case` itself.  2: in every
    valid auxiliary row the top logit is 4.0, the target 4 - ln 2.4, a third 4 - ln 6 and the rest N(0, 1) - 12, so that p is about
    (.632, .263, .105): the top-3 mean 1/3 exceeds p_t and the top-5 mean 1/5 does not.  1: the target is the top logit (6.0, then 4.0
    and 1.0): neither hinge is active.  The auxiliary rows are built and, for "view", carried to y by `unview`."""
    B, L = REGIME_SHAPE
    y, tgt, emo = make_case(B, L, ld)
    if count == 3:
        return y, tgt, emo
    rng = np.random.default_rng(7 + count)
    z = (rng.standard_normal((B, L, NC)) - 12.0).astype(np.float32)
    t = np.where((tgt >= 0) & (tgt < NC), tgt, 0)[..., None]
    a, b = (t + 1 + rng.integers(0, 70, size=t.shape)) % NC, (t + 80 + rng.integers(0, 70, size=t.shape)) % NC   # two other columns
    vals = (np.float32(4.0 - np.log(2.4)), 4.0, np.float32(4.0 - np.log(6.0))) if count == 2 else (6.0, 4.0, 1.0)
    for idx, v in zip((t, a, b), vals):
        np.put_along_axis(z, idx, np.float32(v), -1)
    y[..., :NC] = z if layout == "rows" else unview(z)
    return y, tgt, emo


def hinge_rows(z, t, k, of="p"):
    """relu(mean(top-k) - value at t) per row of z (..., 159) (torch), t an index tensor of z's leading shape; of="p": of softmax(z)."""
    p = torch.softmax(z, dim=-1) if of == "p" else z
    top = torch.sort(p, dim=-1, descending=True).values[..., :k].sum(-1) / k
    return torch.relu(top - torch.gather(p, -1, t.unsqueeze(-1)).squeeze(-1))


def loss_terms(yt, tgt, emo, smoothing, weights, layout, variant=None):
    """The semantics above on a torch tensor yt (B, L, 159) of any float dtype (it may require grad) and numpy targets.  Returns a dict
    of tensors -- total, chord, emotion, ce, aux3, aux5, the per-clip sums ce_sum, bce_sum, a3_sum, a5_sum, n_valid -- and the int
    `count`.  variant: one of WRONG's names, a deliberately wrong reading for the host tests."""
    B, L = tgt.shape
    dtype, dev = yt.dtype, yt.device
    t_np, e_np = clean_targets(np.asarray(tgt), np.asarray(emo))
    t = torch.from_numpy(t_np).to(dev)
    valid = t != C.CHORD_PAD
    n_valid = valid.sum()
    zero = torch.zeros((), dtype=dtype, device=dev)
    rows = torch.from_numpy(HE.emotion_rows(t_np, e_np)).to(dev, dtype)
    ce_rows = torch.nn.CrossEntropyLoss(ignore_index=C.CHORD_PAD, label_smoothing=smoothing, reduction="none")(
        yt.reshape(B * L, NC), t.reshape(B * L)).reshape(B, L)
    bce_rows = torch.nn.BCEWithLogitsLoss(reduction="none")(yt, rows)
    ce = ce_rows.sum() / n_valid
    emotion = bce_rows.sum() / (B * L * NC)
    z = yt if variant == "permute" else aux_rows(yt, layout)       # "permute": the view layout's reshape read as the inverse permute
    terms = ((TERMS[0][0], TERMS[1][1]), (TERMS[1][0], TERMS[0][1])) if variant == "crossed" else TERMS
    aux, sums = [], []
    for k, w in terms:
        h = torch.where(valid, hinge_rows(z, t, k, "z" if variant == "logits" else "p"), zero)
        sums.append(h.sum(1))
        aux.append(h.sum() / (B * L if variant == "all_rows" else n_valid) * w)
    parts = [ce] + aux
    count = 3 if variant == "count3" else sum(int(float(v.detach().to(torch.float32)) > np.float32(COUNT_FLOOR)) for v in parts)
    chord = ((parts[0] + parts[1]) + parts[2]) / (count if count else zero)
    total = weights[0] * chord + weights[1] * emotion
    return {"total": total, "chord": chord, "emotion": emotion, "ce": ce, "aux3": aux[0], "aux5": aux[1], "count": count,
            "n_valid": valid.sum(1), "ce_sum": torch.where(valid, ce_rows, zero).sum(1), "bce_sum": bce_rows.sum((1, 2)),
            "a3_sum": sums[0], "a5_sum": sums[1]}


def chord_aux(y, tgt, emo, smoothing, weights, layout, dtype=torch.float64, grad=True, variant=None):
    """`loss_terms` on numpy inputs (y (B, L, >=159), columns past 159 ignored).  Returns a dict: loss (7,) = {total, chord, emotion,
    ce, aux3, aux5, count}, clip (B, 6) = {n_valid, ce sum, bce sum, L, a_3 sum, a_5 sum} and, with grad, dlogits (B, L, 159) from
    torch's autograd."""
    B, L = tgt.shape
    yt = torch.from_numpy(np.ascontiguousarray(y[..., :NC])).to(dtype).requires_grad_(grad)
    r = loss_terms(yt, tgt, emo, smoothing, weights, layout, variant)
    out = {"loss": np.array([float(r[k].detach()) for k in ("total", "chord", "emotion", "ce", "aux3", "aux5")] + [float(r["count"])]),
           "clip": np.stack([r["n_valid"].numpy()] + [r[k].detach().numpy() for k in ("ce_sum", "bce_sum")] + [np.full(B, L)]
                            + [r[k].detach().numpy() for k in ("a3_sum", "a5_sum")], axis=1).astype(np.float64)}
    if grad:
        r["total"].backward()
        out["dlogits"] = yt.grad.numpy()
    return out


WRONG = ("permute", "logits", "count3", "all_rows", "crossed")


def conditions(y, tgt, layout):
    """(smallest gap between the k-th and (k+1)-th largest logit, smallest |mean top-k of p - p_t|) over the valid auxiliary rows and
    k = 3, 5, in fp64: how far the case stays from the two places where the gradient is discontinuous.  (inf, inf) without a valid row."""
    z = aux_rows(np.asarray(y[..., :NC], dtype=np.float64), layout)
    t = np.where((tgt >= 0) & (tgt < NC), tgt, C.CHORD_PAD)
    valid = t != C.CHORD_PAD
    if not valid.any():
        return np.inf, np.inf
    z, t = z[valid], t[valid]
    s = -np.sort(-z, axis=-1)
    p = np.exp(z - z.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    ps, pt = -np.sort(-p, axis=-1), np.take_along_axis(p, t[:, None], -1)[:, 0]
    gap = min(float((s[:, k - 1] - s[:, k]).min()) for k, _ in TERMS)
    margin = min(float(np.abs(ps[:, :k].sum(-1) / k - pt).min()) for k, _ in TERMS)
    return gap, margin


@functools.lru_cache(maxsize=None)
def reference(B, L, smoothing, weights, layout, regime=3):
    """fp64 and fp32 restatement results of a kernel-test case, computed once and shared; treat the arrays as read-only."""
    y, tgt, emo = make_case(B, L) if regime == 3 else regime_case(regime, layout)
    return (chord_aux(y, tgt, emo, smoothing, weights, layout, torch.float64), chord_aux(y, tgt, emo, smoothing, weights, layout, torch.float32))


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())
