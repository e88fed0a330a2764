"""Training of the V3 chord models and of '2.2' with balancing, without a GPU: the conditions the case table of
tests/helpers_v3_train.py must meet, the restatement against `O.forward_family`, the wrong variants, the opt-in and what is still
refused, the `train_v3` entry point, and the library's new entry points as far as the host can ask."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import amt_oracle as O
from tests import helpers_v3_train as V
from video2music_amd import _lib, ops, train, train_families, train_v3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the case table -------------------------------------------------------------------------------------------------------------------
def test_the_table_is_the_issues():
    got = {c.name: (c.version, c.n_layers, c.d, c.H, c.dff, c.L, c.S, c.B) for c in V.CASES}
    assert got == {"c30": ("3.0", 4, 64, 2, 96, 33, 17, 2), "c31": ("3.1", 4, 64, 2, 96, 33, 17, 2), "c32": ("3.2", 4, 64, 2, 96, 33, 17, 2),
                   "c31_hd128": ("3.1", 3, 128, 1, 96, 129, 40, 3), "c32_hd64": ("3.2", 3, 128, 2, 96, 5, 3, 1),
                   "c31_one": ("3.1", 3, 64, 2, 96, 1, 1, 1), "c31_long": ("3.1", 4, 128, 2, 96, 300, 300, 2),
                   "c30_drop": ("3.0", 4, 64, 2, 96, 33, 17, 2), "c22_bal": ("2.2", 4, 64, 2, 96, 33, 40, 3)}
    assert [V.BY_NAME[n].seed for n in ("c30", "c31", "c32", "c31_hd128", "c32_hd64", "c31_one", "c31_long")] == [21, 22, 23, 24, 25, 26, 27]
    c = V.BY_NAME["c30_drop"]
    assert (c.p, c.droptoken) == (0.2, 0.3) and all(V.BY_NAME[n].p == 0 for n in V.NAMES if n != "c30_drop")


@pytest.mark.parametrize("name", V.NAMES)
def test_every_case_meets_its_conditions(name):
    ref = V.reference(name)
    c = V.BY_NAME[name]
    n_mix = 2 * max(0, V.built_layers(c) - 3)
    assert len(ref["recs"]) == n_mix == len(V.bias_keys(V.state_dict(name)))
    flips = [V.flipped_fraction(r) for r in ref["recs"]]
    gap = V.biased_gap(ref["recs"])
    print(f"{name}: e32 {ref['e32']:.3e}, e32_lambda {ref['e32_lambda']:.3e}, e32_y {ref['e32_y']:.3e}, biased gap {gap:.3e}, flipped {flips}")
    assert all(f >= 0.25 for f in flips), flips
    assert gap >= V.ROUTE_GAP
    assert 0 < V.bound(ref) <= V.CAP and 0 < V.lambda_bound(ref) <= V.CAP and V.LOGIT_FACTOR * ref["e32_y"] <= V.CAP
    lam = [k for k in ref["g64"] if V.is_lambda(k)]
    assert (len(lam) > 0) == (c.version[0] == "3") and all(ref["scales"][k] > 0 or c.L == 1 for k in lam)
    none = {k for k, v in ref["g64"].items() if v is None}
    assert none == {"embedding.weight", "condition_linear.weight", "condition_linear.bias"} | set(V.bias_keys(V.state_dict(name)))
    for rec in ref["recs"]:                                      # the expected bias is the reference's fp32 arithmetic on integer counts
        assert rec["bias_after"].dtype == torch.float32 and float(rec["counts"].sum()) == rec["idx"].numel()


@pytest.mark.parametrize("name", ["c30", "c31", "c32", "c31_hd128", "c22_bal"])
def test_the_restatement_with_zero_bias_is_forward_family(name):
    c, f = V.BY_NAME[name], V.inputs(name)
    sd = {k: (np.zeros_like(v) if k.endswith(".ff.bias") else v) for k, v in V.state_dict(name).items()}
    P = {k: V.cast(v, torch.float64) for k, v in sd.items()}
    t = lambda k: torch.as_tensor(f[k])
    with torch.no_grad():
        want = O.forward_family(P, c.version, c.H, t("root"), t("attr"), t("semantic").double(), t("key").double(), t("scene_offset").double(),
                                t("motion").double(), t("emotion").double())
        for training in (True, False):
            got = V.forward_restated(P, c, f, training=training, table64=True)
            assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (name, training)


VARIANT_CASES = {
    "bias_ignored": ("c31", "c22_bal"),
    "weights_biased": ("c31", "c22_bal"),
    "d_o2_without_lambda": ("c31", "c31_long"),
    "dv_first_map_only": ("c31", "c32"),
    "dw_without_out_scale": ("c31", "c32_hd64"),
    "lambda_init_depth0": ("c31", "c30"),
    "subln_eps_1e-6": ("c31", "c31_one", "c32_hd64"),
}


@pytest.mark.parametrize("variant", V.VARIANTS)
def test_a_wrong_variant_misses_some_bound_by_ten(variant):
    miss = {n: V.variant_miss(n, variant) for n in VARIANT_CASES[variant]}
    print(variant, {n: f"{m:.3g}" for n, m in miss.items()})
    assert max(miss.values()) >= V.MISS, miss


# ---- the opt-in -----------------------------------------------------------------------------------------------------------------------
def _call(m):
    z = torch.zeros(1, 2, dtype=torch.long)
    return m.train()(z, z, z, torch.zeros(1, 2, 8), torch.zeros(1), torch.zeros(1, 2), torch.zeros(1, 2, 1), torch.zeros(1, 2, 6))


@pytest.mark.parametrize("family,kw,message", [
    ("V2", dict(version_name="2.2", balancing=True, n_layers=4), "balancing=True"),
    ("V3", dict(version_name="3.0", n_layers=3), "differential attention"),
    ("V3", dict(version_name="3.1", n_layers=4), "differential attention"),
    ("V3", dict(version_name="3.2", n_layers=3), "differential attention"),
])
def test_a_fresh_model_refuses_and_an_opted_in_one_reaches_the_device_check(family, kw, message):
    from video2music_amd.model import video_music_transformer as M
    from video2music_amd.model.moe import _MoEBase
    m = getattr(M, "VideoMusicTransformer_" + family)(**dict(dict(num_heads=2, d_model=64, dim_feedforward=64, total_vf_dim=16), **kw))
    assert not any(q.train_balancing for q in m.modules() if isinstance(q, _MoEBase))
    with pytest.raises(NotImplementedError, match=message) as info:
        _call(m)
    assert "enable_training()" in str(info.value)
    assert m.enable_training() is m and m._train_refusal() is None
    assert all(q.train_balancing for q in m.modules() if isinstance(q, _MoEBase))
    with pytest.raises(_lib.AmtError, match="no CPU fallback"):
        _call(m)


def test_what_stays_refused_after_the_call(monkeypatch):
    from video2music_amd.model import video_music_transformer as M
    from video2music_amd.utilities import constants
    kw = dict(n_layers=3, d_model=64, dim_feedforward=64, total_vf_dim=16)
    for cls, more, message in ((M.VideoMusicTransformer_V2, dict(version_name="2.0", num_heads=2), "TopKScheduler"),
                               (M.VideoMusicTransformer_V2, dict(version_name="2.1", num_heads=2), "TopKScheduler"),
                               (M.VideoMusicTransformer_V3, dict(version_name="3.1", num_heads=4), "head_dim 16")):
        with pytest.raises(NotImplementedError, match=message):
            _call(cls(**kw, **more).enable_training())
    monkeypatch.setattr(constants, "IS_SEPERATED", True)
    with pytest.raises(NotImplementedError, match="IS_SEPERATED"):
        _call(M.VideoMusicTransformer_V3(version_name="3.1", num_heads=2, **kw).enable_training())


def test_a_bare_layers_switch_is_a_class_attribute_that_defaults_to_off():
    from video2music_amd.model.moe import GLUExpert, MoELayer, SharedMoELayer, _MoEBase
    assert _MoEBase.train_balancing is False
    layer = SharedMoELayer(GLUExpert(32, 64), 32, n_experts=4, balancing=True).train()
    assert "balancing=True" in layer._train_refusal()
    layer.train_balancing = True
    assert layer._train_refusal() is None
    with torch.no_grad():
        assert "balancing=True" in layer._train_refusal()
    assert MoELayer(GLUExpert(32, 64), 32, n_experts=4).train()._train_refusal() is None


# ---- the entry point ------------------------------------------------------------------------------------------------------------------
SYN = ["--synthetic_weights"]


def why(argv):
    return train.refuse(train.parse_args(argv), train_v3.TRAINABLE, balancing=True)


def test_trainable_versions():
    assert train_v3.TRAINABLE == train_families.TRAINABLE + ("3.0", "3.1", "3.2")


@pytest.mark.parametrize("argv", [
    *[["-music_gen_version", v] + SYN for v in train_v3.TRAINABLE],
    ["-music_gen_version", "3.1", "-chord_embed", ""],
    ["-music_gen_version", "2.2", "-balancing", "1"] + SYN,
    ["-music_gen_version", "3.2", "-droptoken", "0.3", "-scene_embed", "1", "-chord_embed", ""],
    ["-music_gen_version", "3.0", "-d_model", "256", "-num_heads", "2"] + SYN,
])
def test_accepted(argv):
    assert why(argv) is None


@pytest.mark.parametrize("argv,reason", [
    (["-music_gen_version", "2.0"] + SYN, r"-music_gen_version 2\.0: .*TopKScheduler"),
    (["-music_gen_version", "2.1"] + SYN, r"-music_gen_version 2\.1: .*TopKScheduler"),
    (["-music_gen_version", "2.3"] + SYN, r"-music_gen_version 2\.3: .*KANLinear.*versions that train are .*3\.0, 3\.1, 3\.2"),
    (["-music_gen_version", "4.0"] + SYN, r"no such model"),
    (["-music_gen_version", "3.1", "-auxiliary_loss", "1"] + SYN, r"-auxiliary_loss"),
    (["-music_gen_version", "3.1", "-drop_loss", "1"] + SYN, r"-drop_loss"),
    (["-music_gen_version", "3.1", "-augmentation", "1"] + SYN, r"-augmentation"),
    (["-music_gen_version", "3.1", "--no_tensorboard", ""] + SYN, r"tensorboard"),
    (["-music_gen_version", "3.1", "-optimizer", "Lion"] + SYN, r"-optimizer Lion: Adam or AdamW"),
    (["-music_gen_version", "3.1", "-num_heads", "32"] + SYN, r"head dims 32 / 64 / 128"),
    (["-music_gen_version", "3.1"], r"-chord_embed: the frozen chord table needs a source"),
])
def test_refused(argv, reason):
    assert re.search(reason, why(argv) or ""), why(argv)
    with pytest.raises(SystemExit, match=reason):
        train_v3.main(argv)


@pytest.mark.parametrize("argv", [["-music_gen_version", "3.0"] + SYN, ["-music_gen_version", "3.2"] + SYN,
                                  ["-music_gen_version", "2.2", "-balancing", "1"] + SYN, SYN, ["-music_gen_version", "None", "-chord_embed", ""]])
def test_the_other_entry_points_answer_as_before(argv):
    args = train.parse_args(argv)
    fam = train.refuse(args, train_families.TRAINABLE)
    assert fam == train.refuse(args, train_families.TRAINABLE, balancing=False)
    v = args.music_gen_version
    if v is not None and v.startswith("3."):
        assert fam == (f"-music_gen_version {v}: the differential attention of the V3 family has no backward; the versions that train are "
                       f"{', '.join(train_families.TRAINABLE)}")
    elif args.balancing:
        assert fam == "-balancing: the routing-bias update of the mixture layers in training is not built"
    else:
        assert fam is None
    base = train.refuse(args)
    assert base == train.refuse(args, ()) == train.refuse(args, (), balancing=True)      # the keyword admits nothing without families
    if v is not None:
        assert base.startswith(f"-music_gen_version {v}: training is built for the base model only")


def test_the_built_class_is_the_reference_s_choice():
    from video2music_amd.model import video_music_transformer as M
    small = ["-n_layers", "3", "-num_heads", "2", "-d_model", "64", "-dim_feedforward", "64", "-chord_embed", ""]
    m = train.build_model(train.parse_args(small + ["-music_gen_version", "3.2", "-droptoken", "0.25"]), 40)
    assert type(m) is M.VideoMusicTransformer_V3 and m.version_name == "3.2" and m.pre_norm and m.dropTokenRate == 0.25 and m.total_vf_dim == 40
    m = train.build_model(train.parse_args(small + ["-music_gen_version", "2.2", "-balancing", "1", "-n_layers", "4"]), 40)
    assert type(m) is M.VideoMusicTransformer_V2 and m.transformer.encoder.layers[3].ff.balancing


# ---- the library ----------------------------------------------------------------------------------------------------------------------
NEW = ("amt_diff_subln_train_fwd", "amt_diff_subln_bwd", "amt_diff_subln_bwd_blocks", "amt_moe_train_fwd_balanced")


def test_library_exports_the_new_entry_points():
    lib = _lib.load()
    header = open(f"{ROOT}/include/amt_hip.h").read()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(rf"\b{name}\(", header), name
    assert _lib.ABI_VERSION >= 13 and lib.amt_abi_version() == _lib.ABI_VERSION
    assert "#define AMT_DIFF_SUBLN_BWD_WS_FLOATS(hd) (4 + 128 * ((hd) + 4))" in header     # ops.diff_subln_bwd allocates this
    assert len(_lib.SIGNATURES["amt_moe_train_fwd_balanced"]) == len(_lib.SIGNATURES["amt_moe_train_fwd"]) + 3


def test_the_workspace_ops_allocates_is_the_headers_macro(monkeypatch):
    from tests.helpers_poison import Poison
    monkeypatch.setattr(ops._lib, "call", lambda *a: 0)
    monkeypatch.setattr(ops, "_st", lambda: None)
    for hd in (32, 64, 128):
        x = torch.zeros(3, hd)
        with Poison("N", modules=["video2music_amd.ops"]) as ps:
            ops.diff_subln_bwd(x, x, x, torch.zeros(hd), torch.zeros(1), 0.5)
        mine = [r.shape[0] for r in ps.registry if len(r.shape) == 1 and r.shape not in ((hd,), (1,))]
        assert mine == [4 + 128 * (hd + 4)]


def test_the_blocks_rule_answers_without_a_device():
    for hd, per in ((32, 128), (64, 64), (128, 32)):
        assert [ops.diff_subln_bwd_blocks(r, hd) for r in (1, per, per + 1, 128 * per, 128 * per + 1, 1 << 22)] == [1, 1, 2, 128, 128, 128]
    for rows, hd in ((0, 32), (-1, 64), (8, 16), (8, 48), (8, 256)):
        with pytest.raises(_lib.AmtError):
            ops.diff_subln_bwd_blocks(rows, hd)


def test_bad_arguments_are_refused_before_any_launch():
    import ctypes as C
    buf = (C.c_float * 4096)()
    addr = (C.addressof(buf) + 15) // 16 * 16
    p = C.c_void_p(addr)
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_diff_subln_train_fwd", None, None, None, None, None, 4, 32, 0.5, 1e-5, None)
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_diff_subln_train_fwd", p, p, p, None, p, 4, 32, 0.5, 1e-5, None)
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_diff_subln_bwd", *[None] * 10, 4, 32, 0.5, 1e-5, None)
    with pytest.raises(_lib.AmtError, match="null pointer"):                    # ws
        _lib.call("amt_diff_subln_bwd", *[p] * 9, None, 4, 32, 0.5, 1e-5, None)
    for hd in (16, 48, 0, 256):
        with pytest.raises(_lib.AmtError, match="must be 32, 64 or 128"):
            _lib.call("amt_diff_subln_bwd", *[p] * 10, 4, hd, 0.5, 1e-5, None)
    with pytest.raises(_lib.AmtError, match="rows"):
        _lib.call("amt_diff_subln_bwd", *[p] * 10, 0, 32, 0.5, 1e-5, None)
    with pytest.raises(_lib.AmtError, match="16-byte aligned"):
        _lib.call("amt_diff_subln_bwd", C.c_void_p(addr + 4), *[p] * 9, 4, 32, 0.5, 1e-5, None)
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_moe_train_fwd_balanced", *[p] * 22, 4, 32, 32, 32, 6, 2, None, None, 0.001, None)
    with pytest.raises(_lib.AmtError, match="amt_moe_train_fwd_balanced: null pointer"):
        _lib.call("amt_moe_train_fwd_balanced", *[None] * 22, 4, 32, 32, 32, 6, 2, None, p, 0.001, p)
