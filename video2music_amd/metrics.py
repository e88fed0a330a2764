"""Test-split chord metrics of the reference's ``evaluate.py`` (``utilities/run_model_vevo.py:198-452``): chord / emotion / total
loss, accuracy, hits@1/3/5 and the emotion-chord correspondence, from teacher-forced logits.

The per-token work (arg-max, rank of the target, cross-entropy, BCE against the emotion row, correspondence) is one device kernel,
``amt_chord_metrics_fwd`` (``csrc/metrics.hip``), which returns ten numbers per clip; ``summarize`` forms the reference's per-clip
ratios from them on the host and averages over clips the way ``eval_model`` does at its default ``batch_size`` 1 (one clip per
"batch": ``compute_hits_k`` only squeezes a batch of one, ``dataset/vevo_dataset.py:682``).

The regression head's figures (``evaluate_regression.py``, ``utilities/run_model_regression.py:70-125``: total loss, RMSE note
density, RMSE loudness, BCE instrument) come the same way: ``amt_reg_metrics_fwd`` (``csrc/reg_metrics.hip``) applies both heads to the
encoder output and returns four numbers per clip; ``regression_clip_figures`` / ``summarize_regression`` form the figures.
"""
import numpy as np
import torch

from . import ops
from .utilities import constants as C
from .utilities.constants import EMOTION_THRESHOLD, LOSS_LAMBDA

FIELDS = ops.CLIP_METRIC_FIELDS


def chord_metrics(logits, tgt, emo_class, emo_prob, threshold=EMOTION_THRESHOLD, return_rows=False):
    """Per-clip sums of the evaluation metrics.  logits (B, L, 159) fp32 on the GPU (any even row stride); tgt (B, L) chord ids
    (CHORD_PAD = ignored); emo_class / emo_prob (B, L): arg-max emotion class of the target's second and its probability
    (``dataset.vevo_features.eval_targets``).  Returns {field: (B,) fp32 tensor} for the fields of ``FIELDS``; with
    ``return_rows`` also "pred", "rank" (B, L) int32 and "ce" (B, L) fp32 (0 on ignored rows).  No host synchronisation."""
    if C.IS_SEPERATED or isinstance(logits, (tuple, list)):
        raise TypeError("softmax(): argument 'input' must be Tensor, not tuple (IS_SEPERATED heads, as in the reference)")
    dev = logits.device
    if logits.dim() != 3 or logits.shape[2] != C.CHORD_SIZE:
        raise ValueError(f"logits must be (B, L, {C.CHORD_SIZE}), got {tuple(logits.shape)}")
    B, L = logits.shape[:2]
    tgt = torch.as_tensor(tgt).to(device=dev, dtype=torch.long).reshape(B, L).contiguous()
    emo_class = torch.as_tensor(emo_class).to(device=dev, dtype=torch.int32).reshape(B, L).contiguous()
    emo_prob = torch.as_tensor(emo_prob).to(device=dev, dtype=torch.float32).reshape(B, L).contiguous()
    out = ops.chord_metrics(logits, tgt, emo_class, emo_prob, threshold, return_rows=return_rows)
    clip = out[0] if return_rows else out
    res = {k: clip[:, i] for i, k in enumerate(FIELDS)}
    if return_rows:
        res.update(pred=out[1], rank=out[2], ce=out[3])
    return res


def _f32_ratio(a, b):
    """a / b as the reference forms it: an fp32 tensor division (``num_right / len(tgt)``), read back as a Python float."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.asarray(a, dtype=np.float32) / np.asarray(b, dtype=np.float32)).astype(np.float64)


def clip_ratios(per_clip):
    """The per-clip figures ``eval_model`` accumulates (:306-332), as float64 arrays over clips: acc, h1, h3, h5, loss_chord,
    loss_emotion, total_loss and cor (-1 where no position of the clip is counted, :804-805).  A clip of PAD targets only has
    acc 1 (:665-666) and NaN hits / chord loss, as in the reference."""
    c = {k: np.asarray(per_clip[k].detach().cpu() if torch.is_tensor(per_clip[k]) else per_clip[k], dtype=np.float64).reshape(-1)
         for k in FIELDS}
    nv = c["n_valid"]
    out = {"acc": np.where(nv > 0, _f32_ratio(c["n_top1"], nv), 1.0)}
    for k in (1, 3, 5):
        out[f"h{k}"] = _f32_ratio(c[f"n_hit{k}"], nv)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["loss_chord"] = c["ce_sum"] / nv
        out["loss_emotion"] = c["bce_sum"] / (C.CHORD_SIZE * c["n_rows"])
    out["total_loss"] = LOSS_LAMBDA * out["loss_chord"] + (1 - LOSS_LAMBDA) * out["loss_emotion"]
    out["cor"] = np.where(c["n_counted"] > 0, _f32_ratio(c["n_right"], c["n_counted"]), -1.0)
    return out


def summarize(per_clip):
    """The dictionary ``eval_model`` returns (:441-452): means over clips of the per-clip figures; avg_cor over the clips whose
    correspondence is defined (cor >= 0; NaN when there is none, where the reference divides by zero)."""
    r = clip_ratios(per_clip)

    def mean(a):            # the reference's running Python sum, clip after clip
        return sum(a.tolist()) / len(a) if len(a) else float("nan")
    avg_acc, avg_cor = mean(r["acc"]), mean(r["cor"][r["cor"] >= 0])
    return {"avg_total_loss": mean(r["total_loss"]), "avg_loss_chord": mean(r["loss_chord"]), "avg_loss_emotion": mean(r["loss_emotion"]),
            "avg_acc": avg_acc, "avg_cor": avg_cor, "avg_acc_cor": (avg_acc + avg_cor) / 2.0,
            "avg_h1": mean(r["h1"]), "avg_h3": mean(r["h3"]), "avg_h5": mean(r["h5"])}


def pred_root_attr(pred):
    """Chord ids -> (root ids, quality ids) by the rule of ``eval_model`` (:339-353): N -> (0, 0), END / PAD -> their root / attr
    ids, else (id - 1) // 13 + 1 and (id - 1) % 13 + 1."""
    p = np.asarray(pred, dtype=np.int64)
    chord = (p > 0) & (p < C.CHORD_END)
    root = np.where(chord, (p - 1) // 13 + 1, np.where(p == C.CHORD_END, C.CHORD_ROOT_END, np.where(p == C.CHORD_PAD, C.CHORD_ROOT_PAD, 0)))
    attr = np.where(chord, (p - 1) % 13 + 1, np.where(p == C.CHORD_END, C.CHORD_ATTR_END, np.where(p == C.CHORD_PAD, C.CHORD_ATTR_PAD, 0)))
    return root, attr


def confusion_matrix(true, pred, labels):
    """sklearn.metrics.confusion_matrix(true, pred, labels=labels): m[i, j] = positions with true == labels[i] and pred ==
    labels[j]; a position whose true or predicted label is not listed is left out."""
    true, pred, labels = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (true, pred, labels))
    where = np.full(int(max(true.max(initial=0), pred.max(initial=0), labels.max(initial=0))) + 1, -1, dtype=np.int64)
    where[labels] = np.arange(len(labels))
    i, j = where[true], where[pred]
    keep = (i >= 0) & (j >= 0)
    m = np.zeros((len(labels), len(labels)), dtype=np.int64)
    np.add.at(m, (i[keep], j[keep]), 1)
    return m


REG_FIELDS = ops.REG_METRIC_FIELDS


def regression_metrics(model, feat, note_density, loudness, instrument, return_rows=False):
    """Per-clip sums of the regression evaluation.  model: a `VideoRegression` on the GPU; feat (B, S, W): its `get_feature` output;
    note_density / loudness (B, S), instrument (B, S, 40): the targets.  Returns {field: (B,) fp32 tensor} for the fields of
    ``REG_FIELDS``; with ``return_rows`` also "ln_nd" (B, S, 2) = (note density, loudness) and "inst" (B, S, 40), what the model's
    `forward` returns.  No host synchronisation."""
    dev = feat.device
    if feat.dim() != 3:
        raise ValueError(f"feat must be (B, S, W), got {tuple(feat.shape)}")
    B, S = feat.shape[:2]
    f32 = lambda t, shape: torch.as_tensor(t).to(device=dev, dtype=torch.float32).reshape(shape).contiguous()
    out = ops.reg_metrics(feat, model.packed_heads(), f32(note_density, (B, S)), f32(loudness, (B, S)),
                          f32(instrument, (B, S, C.INSTRUMENT_SIZE)), return_rows=return_rows)
    clip = out[0] if return_rows else out
    res = {k: clip[:, i] for i, k in enumerate(REG_FIELDS)}
    if return_rows:
        res.update(ln_nd=out[1], inst=out[2])
    return res


def regression_clip_figures(per_clip):
    """The per-clip figures ``eval_model`` accumulates at its batch size of 1 (:106-118), as float64 arrays over clips:
    rmse_note_density = sqrt(sse_nd / S), rmse_loudness = sqrt(sse_l / S), bce_instrument = bce_sum / (40 S) and
    total_loss = sqrt((sse_nd + sse_l) / (2 S)) + bce_instrument (the mse_loss over both columns at once)."""
    c = {k: np.asarray(per_clip[k].detach().cpu() if torch.is_tensor(per_clip[k]) else per_clip[k], dtype=np.float64).reshape(-1)
         for k in REG_FIELDS}
    S = c["n_rows"]
    out = {"rmse_note_density": np.sqrt(c["sse_note_density"] / S), "rmse_loudness": np.sqrt(c["sse_loudness"] / S),
           "bce_instrument": c["bce_sum"] / (C.INSTRUMENT_SIZE * S)}
    out["total_loss"] = np.sqrt((c["sse_note_density"] + c["sse_loudness"]) / (2 * S)) + out["bce_instrument"]
    return out


def summarize_regression(per_clip):
    """The four averages ``eval_model`` returns (:120-125): the per-clip figures -- each clip's own square root taken first --
    added as running Python sums in clip order and divided by the number of clips."""
    r = regression_clip_figures(per_clip)

    def mean(a):
        return sum(a.tolist()) / len(a) if len(a) else float("nan")
    return {"avg_total_loss": mean(r["total_loss"]), "avg_rmse_note_density": mean(r["rmse_note_density"]),
            "avg_rmse_loudness": mean(r["rmse_loudness"]), "avg_bce_instrument": mean(r["bce_instrument"])}
