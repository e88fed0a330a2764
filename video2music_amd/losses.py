"""Training losses.  `regression_train_loss` is the loss of the reference's `utilities/run_model_regression.train_epoch`,

    SmoothL1Loss()(ln_nd, cat(note_density, loudness)) + F.binary_cross_entropy(inst, instrument),

as one kernel launch that also forms both gradients (`amt_reg_loss_fwd_bwd`); `backward()` on the result then starts at the heads'
GEMMs.  The torch expressions above work on the same model outputs and give the same gradients to rounding; this is the fast form.
"""
import torch

from .autograd import RegLossFn


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
