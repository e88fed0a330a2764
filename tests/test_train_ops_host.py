"""Host-side surface of the chord-training operators: what can be checked without a GPU."""
import re
import os

import pytest
import torch

from video2music_amd import _lib, autograd, losses, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_entry_points_are_declared_bound_and_versioned():
    header = open(os.path.join(ROOT, "include", "amt_hip.h")).read()
    for name in ("amt_attn_train_fwd", "amt_attn_bwd", "amt_attn_bwd_ws_floats", "amt_layernorm_bwd", "amt_chord_loss_fwd_bwd",
                 "amt_chord_loss_ws_floats"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert _lib.ABI_VERSION >= 7
    assert callable(ops.layernorm_bwd) and callable(ops.chord_loss) and callable(losses.chord_train_loss)
    assert callable(ops.attention_train) and callable(ops.attention_bwd)
    for fn in (autograd.AttentionFn, autograd.LayerNormFn, autograd.ChordLossFn, autograd.EmbeddingFn):
        assert issubclass(fn, torch.autograd.Function)


def test_workspace_sizes():
    """One ticket block of 4 floats, then three sums per workgroup of 64 rows of a clip (chord loss)."""
    assert _lib.call("amt_chord_loss_ws_floats", 1, 1) == 7
    assert _lib.call("amt_chord_loss_ws_floats", 32, 299) == 4 + 3 * 32 * 5
    assert _lib.call("amt_chord_loss_ws_floats", 0, 5) == 0
    header = open(os.path.join(ROOT, "include", "amt_hip.h")).read()
    assert "#define AMT_LAYERNORM_BWD_WS_FLOATS(dim) (4 + 256 * (dim))" in header        # ops.layernorm_bwd allocates this


def test_arguments_are_refused_before_any_device_work():
    import ctypes
    s = (ctypes.c_int64 * 12)(*autograd.blh_strides(4, 4, 4, 32, 2))
    one = ctypes.c_void_p(16)                               # never dereferenced: the refusal comes first
    with pytest.raises(_lib.AmtError, match="kv_group 2"):
        _lib.call("amt_attn_train_fwd", one, one, one, one, s, 1, 4, 4, 4, 32, 1, 2, 0.25, one, 4, None, 1.0, one, None)
    assert _lib.call("amt_attn_bwd_ws_floats", 1, 2, 37, 37, 32, 0) == 2 * 2 * 37 * 64
    assert _lib.call("amt_attn_bwd_ws_floats", 1, 2, 37, 37, 32, 1) == 2 * 2 * 37 * 64 + 32 * 64 + 2 * 2 * 37 * 32
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_layernorm_bwd", None, None, None, None, None, None, None, None, 4, 32, 1e-5, None)
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_chord_loss_fwd_bwd", None, 159, None, None, 1, 1, 0.4, 0.0, None, None, None, None, None)
