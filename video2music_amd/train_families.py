"""``train`` for the V1 and V2 chord models: ``VideoMusicTransformer_V1`` ('1.0', '1.1', '1.2', '1.2.3', '1.3', '1.3.3', '1.3.4') and
``VideoMusicTransformer_V2`` ('2.2'), the class the reference's ``train.py:136-168`` builds from ``-music_gen_version``, ``-rms_norm``,
``-scene_embed``, ``-chord_embed`` and ``-droptoken``.  The bare command trains the reference's default, '1.2.3' with the chord table.

Flags, loop, output files, CSV header, schedule and optimisers are ``train``'s.  A step runs ``VideoMusicTransformer_V2._forward_train``:
``autograd.RopeFn``, ``GluFn`` (``csrc/family_train.hip``) and ``RMSNormFn`` (``csrc/norm_bwd.hip``) beside ``AttentionFn``,
``LayerNormFn``, ``LinearFn``, ``EmbeddingFn`` and the mixture layers' ``MoEFn``.

The frozen table of ``-chord_embed`` (the reference fills it from a gensim Word2Vec file) comes from ``--chord_embed_table PATH`` (a
``.npy`` of shape (n_chords, d_model), float32), from ``--synthetic_weights`` (the procedural fill), or with ``-continue_weights`` in the
state dict; with none of the three the command refuses.  Still refused, each with its reason: '2.0' / '2.1' (a top-k scheduler that acts
in training), '2.3', every 3.x and ``-balancing`` (both train through ``train_v3``, which opts in to the differential attention's
backward and the routing-bias step), ``-auxiliary_loss``, ``-drop_loss``, ``-augmentation``, tensorboard, optimisers other than
Adam / AdamW, head dims other than 32 / 64 / 128.

    python -m video2music_amd.train_families -dataset_dir ./dataset/ --chord_embed_table chord_table.npy -motion_type 1
"""
import sys

from . import train

TRAINABLE = ("1.0", "1.1", "1.2", "1.2.3", "1.3", "1.3.3", "1.3.4", "2.2")


def main(argv=None):
    return train.main(list(sys.argv[1:] if argv is None else argv), families=TRAINABLE)


if __name__ == "__main__":
    main()
