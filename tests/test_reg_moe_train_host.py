"""Training the mixture regression heads, host side: the fp64 restatement of tests/helpers_moe_train.py against what the reference
recorded in g_reg_moe_train*.npz (so that the GPU tests judge the kernels by an oracle that is itself pinned), what
`python -m video2music_amd.train_regression_moe` accepts and refuses, and the split plan of the grouped weight-gradient product
(ops.moe_wgrad_splits, the launcher's own function) at every case of tests/test_moe_bwd_gpu.py: what each case's comment claims of
its runs is derived here from the fp64 routing before a kernel is judged."""
import numpy as np
import pytest

from tests import helpers_moe_train as T
from tests import test_moe_bwd_gpu as L
from video2music_amd import ops, synthetic, train_regression as TR, train_regression_mamba as TRM, train_regression_moe as TRX
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


# ---- the split plan of the layer cases (tests/test_moe_bwd_gpu.py) ----

def _splits(case, dense=False):
    n_tok, d, raw, n_exp, k = case[:5]
    return ops.moe_wgrad_splits(n_tok, d, (raw + 31) // 32 * 32, n_exp, k, dense)


def _plan(name):
    """(S, [(rows, tiles, tiles per run)] per expert) of a case, from its fp64 routing."""
    case = L.CASES[name]
    o64 = L.oracle(case)[3]
    assert o64["gap"] >= T.GAP, (name, o64["gap"])
    return _splits(case), T.split_plan(o64["idx"], case[3], _splits(case))


def test_cases_from_before_the_split_cases_never_split_the_experts():
    """The gap the split* cases close: every earlier layer case, both masked shapes' elder and the heads' 600-row fixtures run the
    experts' products at S = 1; S > 1 was reached only by the one-group products, at 2."""
    old = [c for name, c in L.CASES.items() if name not in L.SPLIT] + [L.MASKED["tile_plus_one"]]
    assert len(old) == 9
    assert all(_splits(c) == 1 for c in old)
    assert max(_splits(c, dense=True) for c in old) == 2
    for cfg in T.MODELS.values():                                     # (2, 300) clips, top-2 of 6, expert width 2 d + 1
        d = cfg["d_model"]
        assert ops.moe_wgrad_splits(600, d, (2 * d + 1 + 31) // 32 * 32, T.N_EXPERTS, T.TOP_K) == 1
    assert ops.moe_wgrad_splits(32 * 300, 64, 160, T.N_EXPERTS, T.TOP_K) == 25          # tools/bench_reg_train.py's default batch
    with pytest.raises(Exception, match="refuses"):
        ops.moe_wgrad_splits(16, 32, 64, 1, 1)


def test_split_cases_have_the_runs_their_comments_claim():
    assert L.SPLIT == ["split2_even", "split2_empty_group", "split3_empty_run", "split2_head_width", "split3_silu", "split10"]
    assert {name: _plan(name)[0] for name in L.SPLIT} == {"split2_even": 2, "split2_empty_group": 2, "split3_empty_run": 3,
                                                           "split2_head_width": 2, "split3_silu": 3, "split10": 10}
    for name in L.SPLIT:                                             # the runs of a group hold its tiles, in order, none twice
        S, plan = _plan(name)
        assert all(len(runs) == S and sum(runs) == tiles and sorted(runs, reverse=True) == runs for _, tiles, runs in plan), name
    assert _plan("split2_even")[1] == [(256, 2, [1, 1])] * 2                              # full tiles only
    assert _plan("split2_empty_group")[1] == [(520, 5, [3, 2]), (0, 0, [0, 0])]          # a multi-tile run, an 8-row tile, no row at all
    assert _splits(L.CASES["split2_empty_group"], dense=True) == 5
    assert L.MASKED["split2_empty_group"] is L.CASES["split2_empty_group"]
    assert _plan("split3_empty_run")[1] == [(447, 4, [2, 2, 0]), (253, 2, [1, 1, 0])]    # a trailing empty run in every group
    assert sorted({tiles for _, tiles, _ in _plan("split2_head_width")[1]}) == [2, 3]
    assert L.CASES["split2_head_width"][1:5] == (64, 129, T.N_EXPERTS, T.TOP_K)           # the heads' own layer at d_model 64
    silu = _plan("split3_silu")[1]
    assert not L.CASES["split3_silu"][6] and any(runs[-1] == 0 for _, _, runs in silu) and any(runs[-1] == 1 for _, _, runs in silu)
    S, big = _plan("split10")
    n_tok, d, raw, n_exp, k = L.CASES["split10"][:5]
    assert -(-n_tok * k // 256) == 33                                                     # trips of moe_place_stable_kernel
    assert sum(-(-rows // T.TILE) for rows, _, _ in big) * T.TILE > 4096                  # plan rows of the grouped data products
    assert any(max(runs) > 1 for _, _, runs in big) and any(runs[-1] == 0 for _, _, runs in big) and any(min(runs) == 1 for _, _, runs in big)


def test_temperature_of_the_restatement_defaults_to_one():
    case = L.CASES["k3"]
    x, dout, P, o64, _ = L.oracle(case)
    same = T.layer_grads(x, dout, P, case[3], case[4], case[5], temperature=1.0)
    other = T.layer_grads(x, dout, P, case[3], case[4], case[5], temperature=0.7)
    assert all(np.array_equal(same["grads"][k], o64["grads"][k]) for k in o64["grads"]) and np.array_equal(same["out"], o64["out"])
    assert np.array_equal(other["idx"], o64["idx"]) and T.rel_err(other["grads"]["gate.weight"], o64["grads"]["gate.weight"]) > 0.1
