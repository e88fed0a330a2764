"""Training the Mamba regression heads, host side: the fp64 restatement of tests/helpers_reg_mamba_train.py against what the reference
recorded in g_reg_mamba_train*.npz (so that the GPU tests judge the kernels by an oracle that is itself pinned), and what
`python -m video2music_amd.train_regression_mamba` accepts and refuses."""
import pytest

from tests import helpers_reg_mamba_train as T
from video2music_amd import synthetic, train_regression as TR, train_regression_mamba as TRM
from video2music_amd.utilities.argument_reg_funcs import parse_train_args


def state_dict_of(g, name):
    """The procedural weights the generator loaded: the recorded gradient keys carry the reference's key order and shapes."""
    keys = [k[len(name) + 6:] for k in g if k.startswith(name + "_grad_")]
    return synthetic.synthetic_state_dict([(k, g[f"{name}_grad_{k}"].shape) for k in keys], seed=0)


def batch_of(g):
    return g["sem"], g["emo"], g["note_density"], g["loudness"], g["instrument"]


@pytest.mark.parametrize("name", list(T.MODELS))
def test_restatement_equals_the_reference_gradients(golden, name):
    g, g64 = golden("g_reg_mamba_train.npz"), golden("g_reg_mamba_train_64.npz")
    cfg, sd = T.MODELS[name], state_dict_of(g, name)
    r = T.model_grads(sd, cfg["regModel"], cfg["n_layers"], *batch_of(g))
    assert abs(r["loss"] - float(g[f"{name}_loss64"])) <= 1e-12 * abs(r["loss"])
    assert abs(r["loss"] - float(g[f"{name}_loss"])) <= 16 * T.U * abs(r["loss"])         # the reference's fp32 loss: a mean of fp32 terms
    e32 = float(g[f"{name}_e32_grad"])
    assert set(r["grads"]) == set(sd)
    for k in sd:
        assert T.rel_err(g[f"{name}_grad_{k}"], r["grads"][k]) <= 8 * e32, k               # the reference's fp32 figures (its parallel scan)
        if name in T.FULL64:
            assert T.rel_err(r["grads"][k], g64[f"{name}_grad64_{k}"]) <= 1e-11, k         # the recorded fp64 gradients
    assert all(k.startswith(tuple(T.FULL64)) for k in g64)


def test_fixture_holds_what_the_gpu_tests_read(golden):
    g = golden("g_reg_mamba_train.npz")
    for name in T.MODELS:
        assert g[f"{name}_figs_after"][0] < g[f"{name}_figs_before"][0]
        assert 0 < float(g[f"{name}_e32_grad"]) < 1e-4 and 0 < float(g[f"{name}_e32_upd"]) < 1e-1
    assert g["sem"].shape[:2] == (2, 300) and g["emo"].shape == (2, 300, 6)


def test_mask_plan():
    assert T.mask_widths("bimamba+", 2, 32, 64) == [32] + [32, 32, 64, 32] * 2
    assert T.mask_widths("bimamba", 1, 32, 64) == [32, 32, 64, 32, 32, 64, 32]


def _args(*argv):
    return parse_train_args(list(argv))[0]


def test_mamba_entry_accepts_the_bidirectional_heads_and_refuses_the_rest_with_the_reason():
    assert TRM.TRAINABLE == TR.TRAINABLE + ("bimamba+", "bimamba") and TRM.DEFAULT_REGMODEL == "bimamba+"
    for name in TRM.TRAINABLE:
        assert TR.refuse(_args("-regModel", name), trainable=TRM.TRAINABLE) is None
    for name, word in (("mamba", "RMSNorm"), ("mamba+", "RMSNorm"), ("moemamba", "mixture"), ("moe_bimamba+", "mixture"),
                       ("sharedmoe_bimamba+", "mixture"), ("cnngru", "convolution"), ("cnnbigru", "convolution"), ("minGRU", "no such")):
        why = TR.refuse(_args("-regModel", name), trainable=TRM.TRAINABLE)
        assert why and word in why and "bimamba+" in why, (name, why)
        with pytest.raises(SystemExit, match=word):
            TRM.main(["-regModel", name])
    with pytest.raises(SystemExit, match="RAdam"):                           # the other refusals are train_regression's own
        TRM.main(["-regModel", "bimamba", "-optimizer", "RAdam"])


def test_mamba_entry_defaults_to_bimamba_plus(monkeypatch):
    seen = {}

    def fake_main(argv, trainable):
        seen["regModel"], seen["trainable"] = parse_train_args(argv)[0].regModel, trainable
    monkeypatch.setattr(TR, "main", fake_main)
    TRM.main(["-epochs", "1"])
    assert seen == {"regModel": "bimamba+", "trainable": TRM.TRAINABLE}
    TRM.main(["-regModel", "bigru"])
    assert seen["regModel"] == "bigru"


def test_train_regression_itself_still_refuses_the_mamba_heads():
    for name in ("bimamba+", "bimamba", "mamba"):
        why = TR.refuse(_args("-regModel", name))
        assert why and "backward pass is built for the recurrent heads" in why
        with pytest.raises(SystemExit, match="backward pass is built for the recurrent heads"):
            TR.main(["-regModel", name])
    assert TR.refuse(_args("-regModel", "bilstm")) is None
