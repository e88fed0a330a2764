"""Test-split chord metrics of the reference's ``evaluate.py`` (``utilities/run_model_vevo.py:198-452``): chord / emotion / total
loss, accuracy, hits@1/3/5 and the emotion-chord correspondence, from teacher-forced logits.

The per-token work (arg-max, rank of the target, cross-entropy, BCE against the emotion row, correspondence) is one device kernel,
``amt_chord_metrics_fwd`` (``csrc/metrics.hip``), which returns ten numbers per clip; ``summarize`` forms the reference's per-clip
ratios from them on the host and averages over clips the way ``eval_model`` does at its default ``batch_size`` 1 (one clip per
"batch": ``compute_hits_k`` only squeezes a batch of one, ``dataset/vevo_dataset.py:682``).
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
