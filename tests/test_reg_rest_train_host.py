"""Training the last five regression heads, host side: what `python -m video2music_amd.train_regression_all` accepts and refuses (and
that the three older entries answer as before), the mask shapes the restatement consumes per head, the fp64 restatement of
tests/helpers_reg_rest_train.py against what the reference recorded in g_reg_rest_train*.npz (so that the GPU tests judge the
kernels by an oracle that is itself pinned), that deliberately wrong restatements miss the recorded gradients by more than the
GPU tests' bound, and the library's new symbols."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import helpers_reg_rest_train as T
from video2music_amd import _lib, synthetic
from video2music_amd import train_regression as TR, train_regression_all as TRA, train_regression_mamba as TRM, train_regression_moe as TRX
from video2music_amd.utilities.argument_reg_funcs import parse_train_args

ROWS = 600
ALL13 = ("lstm", "bilstm", "gru", "bigru", "cnngru", "cnnbigru", "mamba", "mamba+", "moemamba", "bimamba", "bimamba+", "moe_bimamba+",
         "sharedmoe_bimamba+")            # model/video_regression.py:124-183


def _args(*argv):
    return parse_train_args(list(argv))[0]


def state_dict_of(g, name):
    keys = [k[len(name) + 6:] for k in g if k.startswith(name + "_grad_")]
    return synthetic.synthetic_state_dict([(k, g[f"{name}_grad_{k}"].shape) for k in keys], seed=T.SEEDS[name])


def batch_of(g):
    return g["sem"], g["emo"], g["note_density"], g["loudness"], g["instrument"]


def bound(e32):
    return 8 * e32                     # tests/test_reg_rest_train_gpu.py's


# ---- the entries ----

def test_the_new_entry_accepts_all_thirteen_heads_and_refuses_the_rest_with_train_regressions_reasons():
    assert TRA.TRAINABLE == TRX.TRAINABLE + ("mamba", "mamba+", "moemamba", "cnngru", "cnnbigru")
    assert sorted(TRA.TRAINABLE) == sorted(ALL13)
    for name in ALL13:
        assert TR.refuse(_args("-regModel", name), trainable=TRA.TRAINABLE) is None
    why = TR.refuse(_args("-regModel", "minGRU"), trainable=TRA.TRAINABLE)
    assert why and "no such" in why
    for argv, word in ((["-regModel", "minGRU"], "no such"), (["-regModel", "moemamba", "-use_KAN", "1"], "KANLinear"),
                       (["-regModel", "mamba", "-optimizer", "RAdam"], "RAdam"), (["-regModel", "cnngru", "-optimizer", "RAdamW"], "RAdam"),
                       (["-regModel", "cnnbigru", "-augmentation", "1"], "-augmentation is not built"),
                       (["-regModel", "mamba+", "--no_tensorboard", ""], "tensorboard reporting is not built"),
                       (["-regModel", "moemamba", "--force_cpu", "1"], "no CPU path"), (["-regModel", "mamba", "-is_video", ""], "-is_video False")):
        assert word in TR.refuse(_args(*argv), trainable=TRA.TRAINABLE)
        with pytest.raises(SystemExit, match=re.escape(word)):
            TRA.main(argv)


def test_the_new_entry_keeps_the_parsers_default_and_opts_in(monkeypatch):
    seen = {}

    def fake_main(argv, trainable, opt_in=False):
        seen.update(regModel=parse_train_args(argv)[0].regModel, trainable=trainable, opt_in=opt_in)
    monkeypatch.setattr(TR, "main", fake_main)
    TRA.main(["-epochs", "1"])
    assert seen == {"regModel": _args().regModel, "trainable": TRA.TRAINABLE, "opt_in": True} and seen["regModel"] == "bilstm"
    TRA.main(["-regModel", "cnnbigru"])
    assert seen["regModel"] == "cnnbigru"
    for entry, trainable in ((TRM, TRM.TRAINABLE), (TRX, TRX.TRAINABLE)):       # the two older wrappers: main(argv, trainable=...)
        seen.clear()
        entry.main(["-epochs", "1"])
        assert seen["trainable"] == trainable and seen["opt_in"] is False


def test_opt_in_is_off_by_default():
    sig = inspect.signature(TR.main)
    assert list(sig.parameters) == ["argv", "trainable", "opt_in"] and sig.parameters["opt_in"].default is False
    assert sig.parameters["trainable"].default == TR.TRAINABLE == ("lstm", "bilstm", "gru", "bigru")


def test_the_three_older_entries_answer_as_before_and_point_at_the_new_one():
    for name in TRA.TRAINABLE[len(TRX.TRAINABLE):]:
        for entry, trainable in ((TR, TR.TRAINABLE), (TRM, TRM.TRAINABLE), (TRX, TRX.TRAINABLE)):
            why = TR.refuse(_args("-regModel", name), trainable=trainable)
            assert why and "run inference here" in why
            with pytest.raises(SystemExit, match=re.escape(why)):
                entry.main(["-regModel", name])
        assert "train_regression_all" in TR.refuse(_args("-regModel", name), trainable=TRX.TRAINABLE)
    assert all(v.endswith("train_regression_all") for k, v in TR.UNBUILT.items() if k in TRA.TRAINABLE[len(TRX.TRAINABLE):])
    assert "no such" in TR.refuse(_args("-regModel", "minGRU"), trainable=TRX.TRAINABLE)
    for name in TRX.TRAINABLE:
        assert TR.refuse(_args("-regModel", name), trainable=TRX.TRAINABLE) is None


def test_enable_training_is_an_opt_in_of_the_five_heads():
    from video2music_amd.model.video_regression import VideoRegression
    assert VideoRegression.OPT_IN_TRAINABLE == TRA.TRAINABLE[len(TRX.TRAINABLE):]
    for name in ALL13:
        m = VideoRegression(n_layers=1, d_model=32, d_hidden=32, dropout=0.0, total_vf_dim=8, regModel=name).train()
        assert m._training_enabled is False and m._train_path() == (name in TRX.TRAINABLE)
        assert m.enable_training() is m and m._train_path() and not m.eval()._train_path()


# ---- the restatement's mask shapes (the module's own plan is held to them on the GPU: test_reg_rest_train_gpu.py's injected and drawn masks) ----

def test_mask_shapes_of_the_restatement():
    assert T.mask_shapes("mamba", 2, ROWS, 32, 0.2) == [(ROWS, 32)] == T.mask_shapes("mamba+", 1, ROWS, 32, 0.2)
    assert T.mask_shapes("moemamba", 2, ROWS, 32, 0.2) == [(ROWS, 32)] + [(2 * ROWS, 65), (2 * ROWS, 32), (ROWS, 65)] * 2
    assert T.mask_shapes("cnngru", 2, ROWS, 32, 0.2) == [(ROWS, 32), (ROWS, 32), (ROWS, 32)]
    assert T.mask_shapes("cnnbigru", 3, ROWS, 32, 0.2) == [(ROWS, 32), (ROWS, 32), (ROWS, 64), (ROWS, 64)]
    assert T.mask_shapes("cnnbigru", 1, ROWS, 32, 0.2) == [(ROWS, 32), (ROWS, 32)]
    for name in ("mamba", "mamba+", "cnngru", "cnnbigru"):
        assert T.mask_shapes(name, 2, ROWS, 32, 0.0) == []
    assert T.mask_shapes("moemamba", 1, ROWS, 32, 0.0) == [(2 * ROWS, 65), (ROWS, 65)]          # the experts' own 0.1 alone
    assert T.mask_shapes("moemamba", 2, ROWS, 32, 0.0, 0.0) == []


# ---- the restatement against the fixture ----

@pytest.fixture(scope="module")
def g(golden):
    return {**golden("g_reg_rest_train.npz"), **golden("g_reg_rest_train_b.npz")}


_O = {}


def oracle(g, name):
    if name not in _O:
        cfg = T.MODELS[name]
        _O[name] = T.model_grads(state_dict_of(g, name), cfg["regModel"], cfg["n_layers"], *batch_of(g))
    return _O[name]


# _e32_upd is no arithmetic noise: it is the spacing of the fp32 numbers the parameters are stored in, relative to a three-step update.
# 'mamba+': dt_proj.bias reaches 6.7 (one ulp 4.8e-7) and moves by 7.2e-5 in three steps, so its stored value cannot follow the fp64
# update closer than 7e-3 of it, in the reference's run or in any other that keeps fp32 parameters
# (`test_update_noise_is_the_storage_of_fp32_parameters`).  The arithmetic is held by the gradients' 8 e32_grad < 4e-5.
E32_UPD_LIMIT = {name: 1e-3 for name in T.MODELS}
E32_UPD_LIMIT["mamba+"] = 1e-2


def test_update_noise_is_the_storage_of_fp32_parameters(g):
    """Three SGD steps with the restatement's fp64 gradients and the parameters rounded to fp32 after every step miss the all-fp64
    updates by the recorded _e32_upd of the reference's fp32 run (to 5 %), at the tensor named above."""
    name = "mamba+"
    cfg, sd, data = T.MODELS[name], state_dict_of(g, name), batch_of(g)
    want = T.sgd_updates(sd, T.SGD_STEPS, T.SGD_LR, cfg["regModel"], cfg["n_layers"], *data)
    P = {k: np.asarray(v, dtype=np.float32) for k, v in sd.items()}
    for _ in range(T.SGD_STEPS):
        gr = T.model_grads(P, cfg["regModel"], cfg["n_layers"], *data)["grads"]
        P = {k: (P[k].astype(np.float64) - T.SGD_LR * gr[k]).astype(np.float32) for k in P}
    errs = {k: T.rel_err(P[k].astype(np.float64) - np.asarray(sd[k], dtype=np.float64), want[k]) for k in P}
    worst = max(errs, key=errs.get)
    e32 = float(g[f"{name}_e32_upd"])
    assert worst == "model.layers.0.mixer.dt_proj.bias" and abs(errs[worst] - e32) <= 0.05 * e32
    ulp = float(np.spacing(np.float32(np.abs(sd[worst]).max())))
    assert 0.5 * ulp / np.abs(want[worst]).max() <= e32 <= 2 * ulp / np.abs(want[worst]).max()


@pytest.mark.parametrize("name", list(T.MODELS))
def test_restatement_equals_the_reference_gradients(golden, g, name):
    g64 = golden("g_reg_rest_train_64.npz")
    r, sd = oracle(g, name), state_dict_of(g, name)
    assert abs(r["loss"] - float(g[f"{name}_loss64"])) <= 1e-12 * abs(r["loss"])
    assert abs(r["loss"] - float(g[f"{name}_loss"])) <= 16 * T.U * abs(r["loss"])         # the reference's fp32 loss: a mean of fp32 terms
    e32 = float(g[f"{name}_e32_grad"])
    assert 0 < e32 < 1e-3 and 0 < float(g[f"{name}_e32_upd"]) < E32_UPD_LIMIT[name]         # 8 e32 is a bound that can fail
    assert set(r["grads"]) == set(sd)
    for k in sd:
        assert T.rel_err(g[f"{name}_grad_{k}"], r["grads"][k]) <= e32 * (1 + 1e-9), k     # e32 is the largest of exactly these
        if name in T.FULL64:
            assert T.rel_err(r["grads"][k], g64[f"{name}_grad64_{k}"]) <= 1e-11, k         # the recorded fp64 gradients
    assert all(k.startswith(tuple(n + "_grad64_" for n in T.FULL64)) for k in g64)
    assert g[f"{name}_figs_after"][0] < g[f"{name}_figs_before"][0]
    gap = T.min_gap([r["routing"]])
    assert len(r["routing"]) == (T.MODELS[name]["n_layers"] if "moemamba" in name else 0)
    assert gap >= float(g[f"{name}_min_gap"]) >= T.GAP                                    # the recorded one spans the SGD steps too


def test_gate_gaps_hold_at_every_sgd_step(g):
    name = "moemamba"                       # the two-layer model's are recorded by the tool (asserted above against GAP)
    cfg, routings = T.MODELS[name], []
    T.sgd_updates(state_dict_of(g, name), T.SGD_STEPS, T.SGD_LR, cfg["regModel"], cfg["n_layers"], *batch_of(g), routings=routings)
    assert len(routings) == T.SGD_STEPS and T.min_gap(routings) >= float(g[f"{name}_min_gap"]) >= T.GAP


WRONG = [("mamba+", "rms_weight_detached"), ("moemamba", "rms_weight_detached"), ("moemamba", "states_from_16_dropped"),
         ("moemamba", "d_conv_4"), ("cnnbigru", "conv_taps_mirrored")]


@pytest.mark.parametrize("name,wrong", WRONG)
def test_wrong_restatements_miss_the_recorded_gradients_by_more_than_the_bound(g, name, wrong):
    cfg = T.MODELS[name]
    r = T.model_grads(state_dict_of(g, name), cfg["regModel"], cfg["n_layers"], *batch_of(g), wrong=(wrong,))
    e32 = float(g[f"{name}_e32_grad"])
    worst = max(T.rel_err(r["grads"][k], g[f"{name}_grad_{k}"]) for k in r["grads"])
    print(name, wrong, "worst", worst, "bound", bound(e32) + e32)
    assert worst > 10 * (bound(e32) + e32)


def test_silu_dropout_before_the_silu_is_told_from_after_it(g):
    """At the fixture's rate 0 there is no mask to misplace: with the same injected multipliers, the restatement with CNN_GRU's Dropout
    in front of the SiLU misses the one with it behind by more than the bound."""
    name = "cnngru"
    cfg, sd = T.MODELS[name], state_dict_of(g, name)
    rng = np.random.default_rng(10)
    masks = [((rng.random(s) >= 0.2) / 0.8).astype(np.float32) for s in T.mask_shapes(name, cfg["n_layers"], ROWS, cfg["d_model"], 0.2)]
    right, wrong = (T.model_grads(sd, cfg["regModel"], cfg["n_layers"], *batch_of(g), masks=masks, wrong=w) for w in ((), ("silu_dropout_before_silu",)))
    e32 = float(g[f"{name}_e32_grad"])
    assert max(T.rel_err(wrong["grads"][k], right["grads"][k]) for k in sd) > 10 * bound(e32)


# ---- the library ----

def test_library_exports_the_new_symbols_at_abi_14():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "amt_hip.h")).read()
    assert _lib.ABI_VERSION == 14 == int(re.search(r"#define AMT_ABI_VERSION (\d+)", header).group(1))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.amt_abi_version.restype = ctypes.c_int32
    assert lib.amt_abi_version() == 14
    for name in ("amt_selective_scan_wide_train_fwd", "amt_selective_scan_wide_ckpt_steps", "amt_selective_scan_wide_bwd",
                 "amt_selective_scan_wide_bwd_ws_floats", "amt_silu_bwd"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name in header, name
    lib.amt_selective_scan_wide_ckpt_steps.restype = ctypes.c_int32
    assert [lib.amt_selective_scan_wide_ckpt_steps(ctypes.c_int32(n)) for n in (16, 32, 48, 64, 128, 256, 512)] == [0, 32, 0, 32, 32, 32, 0]
    lib.amt_selective_scan_wide_bwd_ws_floats.restype = ctypes.c_int64
    ws = lambda *a: lib.amt_selective_scan_wide_bwd_ws_floats(*[ctypes.c_int32(v) for v in a])
    assert ws(2, 33, 24, 64) == 2 * 2 * 33 * 128 + 2 * 24 * 65 + 2 * 4 * 66 * 24 and ws(2, 33, 24, 16) == 0 and ws(0, 33, 24, 64) == 0
