"""Training losses.  `regression_train_loss` is the loss of the reference's `utilities/run_model_regression.train_epoch`,

    SmoothL1Loss()(ln_nd, cat(note_density, loudness)) + F.binary_cross_entropy(inst, instrument),

as one kernel launch that also forms both gradients (`amt_reg_loss_fwd_bwd`); `backward()` on the result then starts at the heads'
GEMMs.  The torch expressions above work on the same model outputs and give the same gradients to rounding; this is the fast form.

`chord_train_loss` is the loss of the reference's `utilities/run_model_vevo.train_epoch` (:101-119),

    lambda CrossEntropyLoss(ignore_index=CHORD_PAD, label_smoothing=ce_smoothing)(y, tgt) + (1 - lambda) BCEWithLogitsLoss()(y, tgt_emotion),

with the emotion rows built on the device from the targets and the emotion classes, as the evaluation's metrics kernel builds them
(`amt_chord_loss_fwd_bwd`).
"""
import torch

from .autograd import ChordLossFn, RegLossFn


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


def chord_train_loss(logits, tgt, emo_class, lam, smoothing=0.0):
    """logits (B, L, >=159) fp32 on the device (any tensor: a leaf with requires_grad or a model's output); tgt (B, L) chord ids,
    CHORD_PAD ignored; emo_class (B, L) the arg-max emotion class of each target's second; lam the weight of the chord part;
    smoothing the reference's -ce_smoothing (0 or None = none).  Returns the scalar loss, attached to the graph."""
    dev = logits.device
    return ChordLossFn.apply(logits, tgt.to(device=dev, dtype=torch.int64).contiguous(), emo_class.to(device=dev, dtype=torch.int32).contiguous(),
                             float(lam), float(smoothing or 0.0))
