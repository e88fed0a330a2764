"""``train_regression`` for every ``-regModel`` the reference's ``train_regression.py`` accepts (model/video_regression.py:124-183):
the eight heads ``train_regression_moe`` trains and the five that build their autograd graph only after
``VideoRegression.enable_training()`` -- ``mamba`` / ``mamba+`` (``RMSNormFn`` around ``MambaBlockFn``), ``moemamba`` (the same over
blocks with ``d_state = dim_feedforward`` states per channel: ``amt_selective_scan_wide_train_fwd`` / ``amt_selective_scan_wide_bwd``,
and ``MoEFn``), ``cnngru`` / ``cnnbigru`` (``ConvSiluFn`` in front of ``RnnLayerFn``).

Flags, loop, output files, CSV header and ``weights_regression_<regModel>/`` naming are ``train_regression``'s, ``-regModel`` keeps the
parser's default.  Still refused, with ``train_regression``'s reasons: ``minGRU``, ``-use_KAN``, ``-optimizer RAdam / RAdamW``,
``-augmentation``, tensorboard reporting, ``--force_cpu``, ``-is_video False``.

    python -m video2music_amd.train_regression_all -dataset_dir ./dataset/ -regModel moemamba -epochs 50
"""
import sys

from . import train_regression, train_regression_moe

TRAINABLE = train_regression_moe.TRAINABLE + ("mamba", "mamba+", "moemamba", "cnngru", "cnnbigru")


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    return train_regression.main(argv, trainable=TRAINABLE, opt_in=True)


if __name__ == "__main__":
    main()
