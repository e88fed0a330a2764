"""``train_regression`` for the Mamba regression heads: ``VideoRegression(regModel = bimamba+ | bimamba)``, the head both reference
callers build by default and its original-gate sibling, and the four recurrent heads as before.

Flags, loop, output files, CSV header and ``weights_regression_<regModel>/`` naming are ``train_regression``'s; ``-regModel``
defaults to ``bimamba+`` here.  A step runs ``autograd.MambaBlockFn`` (``amt_selective_scan_train_fwd``, ``amt_selective_scan_bwd``,
``amt_dwconv1d_silu_bwd`` and the library's GEMMs), ``LayerNormFn`` and ``LinearFn``.  Still refused, with the reason: ``mamba`` /
``mamba+`` / ``moemamba`` (no RMSNorm backward), ``moe_bimamba+`` / ``sharedmoe_bimamba+`` (they train through
``python -m video2music_amd.train_regression_moe``), ``cnngru`` / ``cnnbigru``.

    python -m video2music_amd.train_regression_mamba -dataset_dir ./dataset/ -epochs 50
"""
import sys

from . import train_regression

TRAINABLE = train_regression.TRAINABLE + ("bimamba+", "bimamba")
DEFAULT_REGMODEL = "bimamba+"


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if "-regModel" not in argv:
        argv += ["-regModel", DEFAULT_REGMODEL]
    return train_regression.main(argv, trainable=TRAINABLE)


if __name__ == "__main__":
    main()
