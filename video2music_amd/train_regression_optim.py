"""``train_regression_all`` with the reference's ``-optimizer`` choices (``train_regression.py:145-154``) for every ``-regModel``:
Adam and AdamW as before (torch's), ``RAdam`` (no decay) and ``RAdamW`` (``weight_decay=1e-5``, decoupled) on the fused multi-tensor
kernel ``amt_optim_step`` (``video2music_amd/optim.py``).  ``RAdanW`` and ``Lion`` are refused: the reference's
``train_regression.py`` has no such branch.  Everything else ``train_regression_all`` refuses stays refused, and the other regression
entry points still take Adam / AdamW alone.

    python -m video2music_amd.train_regression_optim -dataset_dir ./dataset/ -regModel bimamba+ -optimizer RAdamW -epochs 50
"""
import sys

from . import train_regression, train_regression_all

TRAINABLE = train_regression_all.TRAINABLE


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    return train_regression.run(argv, trainable=TRAINABLE, opt_in=True, optimizers=True)


if __name__ == "__main__":
    main()
