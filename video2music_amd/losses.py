"""Training losses.  `regression_train_loss` is the loss of the reference's `utilities/run_model_regression.train_epoch`,

    SmoothL1Loss()(ln_nd, cat(note_density, loudness)) + F.binary_cross_entropy(inst, instrument),

as one kernel launch that also forms both gradients (`amt_reg_loss_fwd_bwd`); `backward()` on the result then starts at the heads'
GEMMs.  The torch expressions above work on the same model outputs and give the same gradients to rounding; this is the fast form.

`chord_train_loss` is the loss of the reference's `utilities/run_model_vevo.train_epoch` (:101-119),

    lambda CrossEntropyLoss(ignore_index=CHORD_PAD, label_smoothing=ce_smoothing)(y, tgt) + (1 - lambda) BCEWithLogitsLoss()(y, tgt_emotion),

with the emotion rows built on the device from the targets and the emotion classes, as the evaluation's metrics kernel builds them
(`amt_chord_loss_fwd_bwd`); with `auxiliary=True` the chord part is the reference's -auxiliary_loss `CombinedLoss` (train.py:221-229),
from `amt_chord_loss_aux_fwd_bwd`.
"""
import torch

from .autograd import ChordAuxLossFn, ChordLossFn, RegLossFn


def regression_train_loss(ln_nd, inst, note_density, loudness, instrument):
    """ln_nd (B, S, 2) and inst (B, S, 40) as `VideoRegression.forward` returned them in the training state; note_density / loudness
    (B, S) and instrument (B, S, 40) the targets.  Returns the scalar loss, attached to the graph."""
    logits = getattr(inst, "_amt_logits", None)
    if logits is None:
        raise ValueError("regression_train_loss takes the `inst` that VideoRegression.forward returned in the training state (its "
                         "gradient goes to the classifier's logits); use torch's SmoothL1Loss + binary_cross_entropy on other tensors")
    dev = inst.device
    tgt = [t.to(device=dev, dtype=torch.float32).contiguous() for t in (note_density, loudness, instrument)]
    return RegLossFn.apply(ln_nd.reshape(-1, 2), logits, inst.detach().reshape(-1, inst.shape[-1]), tgt[0].reshape(-1), tgt[1].reshape(-1),
                           tgt[2].reshape(-1, inst.shape[-1]))


def chord_train_loss(logits, tgt, emo_class, lam, smoothing=0.0, *, auxiliary=False, layout="view", weights=None):
    """logits (B, L, >=159) fp32 on the device (any tensor: a leaf with requires_grad or a model's output); tgt (B, L) chord ids,
    CHORD_PAD ignored; emo_class (B, L) the arg-max emotion class of each target's second; lam the weight of the chord part;
    smoothing the reference's -ce_smoothing (0 or None = none).  Returns the scalar loss, attached to the graph.

    auxiliary: the chord part is the reference's -auxiliary_loss one, (CE + A_3 + A_5) / count (`amt_chord_loss_aux_fwd_bwd`), its
    auxiliary rows in `layout`: "view" as the reference's train_epoch forms them, "rows" as its eval_model does.  weights = (w_chord,
    w_emotion) replaces (lam, 1 - lam): -drop_loss passes (1, 0) or (0, 1).  With neither, the call is `ChordLossFn`'s."""
    dev = logits.device
    tgt, emo_class = tgt.to(device=dev, dtype=torch.int64).contiguous(), emo_class.to(device=dev, dtype=torch.int32).contiguous()
    if auxiliary:
        w_c, w_e = (lam, 1.0 - lam) if weights is None else weights
        return ChordAuxLossFn.apply(logits, tgt, emo_class, float(w_c), float(w_e), float(smoothing or 0.0), layout)
    if weights is not None:
        w_c, w_e = (float(w) for w in weights)
        if (w_c, w_e) not in ((1.0, 0.0), (0.0, 1.0), (float(lam), 1.0 - float(lam))):
            raise ValueError(f"weights {weights} without auxiliary=True: the plain loss kernel takes (lam, 1 - lam), (1, 0) or (0, 1)")
        lam = w_c
    return ChordLossFn.apply(logits, tgt, emo_class, float(lam), float(smoothing or 0.0))
