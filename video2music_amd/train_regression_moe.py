"""``train_regression`` for the mixture regression heads: ``VideoRegression(regModel = moe_bimamba+ | sharedmoe_bimamba+)`` --
``BiMambaEncoderLayer_V1`` with a 6-expert top-2 mixture of ``GLUExpert(d, 2d + 1)`` in the FFN's place (reference
model/video_regression.py:143-178) -- and the six heads ``train_regression_mamba`` trains.

Flags, loop, output files, CSV header and ``weights_regression_<regModel>/`` naming are ``train_regression``'s; ``-regModel``
defaults to ``sharedmoe_bimamba+`` here.  A step runs ``autograd.MoEFn`` (``amt_moe_train_fwd``, ``amt_moe_bwd``: the grouped
weight-gradient product of ``csrc/moe_bwd.hip`` and the library's grouped GEMMs) beside ``MambaBlockFn``, ``LayerNormFn`` and
``LinearFn``.  Refused here, with a pointer to ``python -m video2music_amd.train_regression_all``, which trains them: ``moemamba``,
``mamba`` / ``mamba+``, ``cnngru`` / ``cnnbigru`` (they build a graph only after ``VideoRegression.enable_training()``, which that
entry calls).

    python -m video2music_amd.train_regression_moe -dataset_dir ./dataset/ -epochs 50
"""
import sys

from . import train_regression, train_regression_mamba

TRAINABLE = train_regression_mamba.TRAINABLE + ("moe_bimamba+", "sharedmoe_bimamba+")
DEFAULT_REGMODEL = "sharedmoe_bimamba+"


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if "-regModel" not in argv:
        argv += ["-regModel", DEFAULT_REGMODEL]
    return train_regression.main(argv, trainable=TRAINABLE)


if __name__ == "__main__":
    main()
