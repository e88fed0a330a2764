"""``train`` for the V3 chord models, ``VideoMusicTransformer_V3`` ('3.0', '3.1', '3.2': the class the reference's ``train.py:162-168``
builds), beside every version ``train_families`` trains; and ``-balancing 1`` for '2.2' (``SharedMoELayer(balancing=True)``).

Flags, loop, output files, CSV header, schedule and optimisers are ``train``'s.  After the model is built its ``enable_training()`` is
called: the opt-in that admits ``autograd.DiffAttentionFn`` (two ``amt_attn_train_fwd`` / ``amt_attn_bwd`` calls around
``amt_diff_subln_train_fwd`` / ``amt_diff_subln_bwd``, ``csrc/diff_subln_train.hip``) and the mixture layers' balancing router with its
routing-bias step (``amt_moe_train_fwd_balanced``).  Every V3 mixture layer is a balancing one.

Still refused, each with its reason: '2.0' / '2.1' (a top-k scheduler that acts in training), '2.3', ``-auxiliary_loss``,
``-drop_loss``, ``-augmentation``, tensorboard, optimisers other than Adam / AdamW, head dims other than 32 / 64 / 128.

    python -m video2music_amd.train_v3 -dataset_dir ./dataset/ -music_gen_version 3.1 -chord_embed "" -motion_type 1
"""
import sys

from . import train, train_families

TRAINABLE = train_families.TRAINABLE + ("3.0", "3.1", "3.2")


def main(argv=None):
    return train.main(list(sys.argv[1:] if argv is None else argv), families=TRAINABLE, opt_in=True)


if __name__ == "__main__":
    main()
