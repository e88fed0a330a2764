"""Training the mixture regression heads, host side: the fp64 restatement of tests/helpers_moe_train.py against what the reference
recorded in g_reg_moe_train*.npz (so that the GPU tests judge the kernels by an oracle that is itself pinned), and what
`python -m video2music_amd.train_regression_moe` accepts and refuses."""
import numpy as np
import pytest

from tests import helpers_moe_train as T
from video2music_amd import synthetic, train_regression as TR, train_regression_mamba as TRM, train_regression_moe as TRX
from video2music_amd.utilities.argument_reg_funcs import parse_train_args


def state_dict_of(g, name):
    """The procedural weights the generator loaded: the recorded gradient keys carry the reference's key order and shapes."""
    keys = [k[len(name) + 6:] for k in g if k.startswith(name + "_grad_")]
    return synthetic.synthetic_state_dict([(k, g[f"{name}_grad_{k}"].shape) for k in keys], seed=T.SEED)


def batch_of(g):
    return g["sem"], g["emo"], g["note_density"], g["loudness"], g["instrument"]


@pytest.mark.parametrize("name", list(T.MODELS))
def test_restatement_equals_the_reference_gradients_and_routing(golden, name):
    g, g64 = golden("g_reg_moe_train.npz"), golden("g_reg_moe_train_64.npz")
    cfg, sd = T.MODELS[name], state_dict_of(g, name)
    r = T.model_grads(sd, cfg["regModel"], cfg["n_layers"], *batch_of(g))
    assert abs(r["loss"] - float(g[f"{name}_loss64"])) <= 1e-12 * abs(r["loss"])
    assert abs(r["loss"] - float(g[f"{name}_loss"])) <= 16 * T.U * abs(r["loss"])         # the reference's fp32 loss: a mean of fp32 terms
    e32 = float(g[f"{name}_e32_grad"])
    assert set(r["grads"]) == set(sd)
    for k in sd:
        assert T.rel_err(g[f"{name}_grad_{k}"], r["grads"][k]) <= e32 * (1 + 1e-9), k     # e32 is the largest of exactly these
        if name in T.FULL64:
            assert T.rel_err(r["grads"][k], g64[f"{name}_grad64_{k}"]) <= 1e-11, k         # the recorded fp64 gradients
    assert all(k.startswith(tuple(T.FULL64)) for k in g64)
    routing = r["routing"][0]
    assert np.array_equal(routing["idx"].numpy(), g[f"{name}_routing"])                    # the reference's own choices, every token
    assert T.gate_gap(routing["logits"], T.TOP_K) >= float(g[f"{name}_min_gate_gap"]) >= T.GAP


def test_fixture_holds_what_the_gpu_tests_read(golden):
    g, mamba = golden("g_reg_moe_train.npz"), golden("g_reg_mamba_train.npz")
    for name in T.MODELS:
        assert g[f"{name}_figs_after"][0] < g[f"{name}_figs_before"][0]
        for k in ("e32_grad", "e32_upd"):                                                  # the tool's noise-level condition
            assert 0 < float(g[f"{name}_{k}"]) <= 10 * float(mamba["bimamba+_" + k])
        assert g[f"{name}_routing"].shape == (600, 2) and len(np.unique(g[f"{name}_routing"])) == T.N_EXPERTS
        assert any("ffn.shared_expert." in k for k in g if k.startswith(name + "_grad_")) == name.startswith("shared")
    assert g["sem"].shape[:2] == (2, 300) and g["emo"].shape == (2, 300, 6)


def test_mask_plan():
    assert T.mask_shapes("sharedmoe_bimamba+", 1, 600, 32, 0.2) == [(600, 32)] * 3 + [(1200, 65), (1200, 32), (600, 65), (600, 32)]
    assert T.mask_shapes("moe_bimamba+", 1, 600, 32, 0.2) == [(600, 32)] * 3 + [(1200, 65), (1200, 32), (600, 32)]
    assert T.mask_shapes("sharedmoe_bimamba+", 1, 600, 32, 0.0) == [(1200, 65), (600, 65)]      # the experts' own 0.1 alone
    assert T.mask_shapes("moe_bimamba+", 2, 600, 32, 0.0, 0.0) == []


def _args(*argv):
    return parse_train_args(list(argv))[0]


def test_moe_entry_accepts_its_eight_heads_and_refuses_the_rest_with_the_reason():
    assert TRX.TRAINABLE == TRM.TRAINABLE + ("moe_bimamba+", "sharedmoe_bimamba+") and len(TRX.TRAINABLE) == 8
    for name in TRX.TRAINABLE:
        assert TR.refuse(_args("-regModel", name), trainable=TRX.TRAINABLE) is None
    for name, word in (("moemamba", "RMSNorm"), ("mamba", "RMSNorm"), ("mamba+", "RMSNorm"), ("cnngru", "convolution")):
        why = TR.refuse(_args("-regModel", name), trainable=TRX.TRAINABLE)
        assert why and word in why and "sharedmoe_bimamba+" in why, (name, why)
        with pytest.raises(SystemExit, match=word):
            TRX.main(["-regModel", name])


def test_moe_entry_defaults_to_sharedmoe_bimamba_plus(monkeypatch):
    seen = {}

    def fake_main(argv, trainable):
        seen["regModel"], seen["trainable"] = parse_train_args(argv)[0].regModel, trainable
    monkeypatch.setattr(TR, "main", fake_main)
    TRX.main(["-epochs", "1"])
    assert seen == {"regModel": "sharedmoe_bimamba+", "trainable": TRX.TRAINABLE} and TRX.DEFAULT_REGMODEL == "sharedmoe_bimamba+"
    TRX.main(["-regModel", "moe_bimamba+"])
    assert seen["regModel"] == "moe_bimamba+"


def test_train_regression_mamba_still_refuses_the_mixture_heads_and_points_at_the_new_entry():
    for name in ("moe_bimamba+", "sharedmoe_bimamba+"):
        why = TR.refuse(_args("-regModel", name), trainable=TRM.TRAINABLE)
        assert why and "mixture" in why and "train_regression_moe" in why
        with pytest.raises(SystemExit, match="train_regression_moe"):
            TRM.main(["-regModel", name])
        assert "backward pass is built for the recurrent heads" in TR.refuse(_args("-regModel", name))
