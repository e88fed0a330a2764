"""``train_losses`` with the reference's ``-optimizer`` choices (``train.py:237-250``) for every model it trains:

    Adam, AdamW   what ``train`` builds (torch's)
    RAdam         ``optim.RAdam`` without decay
    RAdamW        ``optim.RAdam(weight_decay=0.01, decoupled_weight_decay=True)``
    RAdanW        ``optim.RAdanW(betas=(ADAM_BETA_1, ADAM_BETA_2, 0.92, 0.99), weight_decay=0.01)``: the reference's own optimiser
                  (``model/RAdanW.py``) in the foreach variant it runs on a GPU

The last three run on the fused multi-tensor kernel ``amt_optim_step`` (``video2music_amd/optim.py``, ``csrc/optim.hip``): one launch
per ``_lib.OPTIM_MAX_TENSORS`` tensors of a step, no host synchronisation.  ``Lion`` is refused: ``lion_pytorch`` is a package the reference does not vendor,
and it is not installed.  Everything ``train_losses`` refuses stays refused; ``train``, ``train_families``, ``train_v3`` and
``train_losses`` still take Adam / AdamW alone.

    python -m video2music_amd.train_optim -dataset_dir ./dataset/ -music_gen_version None -chord_embed "" -motion_type 1 -optimizer RAdanW
"""
import sys

from . import train, train_losses

TRAINABLE = train_losses.TRAINABLE


def main(argv=None):
    return train.main(list(sys.argv[1:] if argv is None else argv), families=TRAINABLE, opt_in=True, losses=True, optimizers=True)


if __name__ == "__main__":
    main()
