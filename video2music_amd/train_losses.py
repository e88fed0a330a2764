"""``train`` with the reference's two loss switches, for every model ``train_v3`` trains (the base model, the V1 / V2 versions of
``train_families``, '3.0' / '3.1' / '3.2', ``-balancing``).

``-auxiliary_loss 1`` (reference ``train.py:221-229``, ``model/loss.py:85-141``): the chord part of the loss becomes
``CombinedLoss([CrossEntropy, TopKAuxiliaryLoss(k=3, weight=3), TopKAuxiliaryLoss(k=5, weight=5)], type='avg')``, one launch pair of
``amt_chord_loss_aux_fwd_bwd`` (``csrc/chord_aux_loss.hip``).  The two call sites of the reference give the auxiliary terms different
rows, and both are kept: a training step reads them as ``train_epoch`` does -- ``y.permute(0, 2, 1)`` RESHAPED to (B, L, 159), 159
consecutive elements of the clip's class-major flattening per row (``layout="view"``) --, the epoch figures as ``eval_model`` does,
on the natural rows, per clip and with the clip's own count of live terms (``train.clip_chord_losses``).  As in the reference the
switch acts only with ``-ce_smoothing`` set (the default 0.1 is).

``-drop_loss 1`` (``utilities/run_model_vevo.py:110-117``): one draw p per step; p < 0.6 keeps the weights (lambda, 1 - lambda),
p < 0.8 trains on the chord loss alone, otherwise on the emotion loss alone.  The reference draws from the unseeded global generator;
here the draws come from a private ``random.Random(--seed)``, so a run repeats.

Still refused, each with its reason: '2.0' / '2.1', '2.3', ``-augmentation``, tensorboard, optimisers other than Adam / AdamW, head
dims other than 32 / 64 / 128.  ``train``, ``train_families`` and ``train_v3`` refuse both switches as before.

    python -m video2music_amd.train_losses -dataset_dir ./dataset/ -music_gen_version None -chord_embed "" -motion_type 1 -auxiliary_loss 1
"""
import sys

from . import train, train_v3

TRAINABLE = train_v3.TRAINABLE


def main(argv=None):
    return train.main(list(sys.argv[1:] if argv is None else argv), families=TRAINABLE, opt_in=True, losses=True)


if __name__ == "__main__":
    main()
