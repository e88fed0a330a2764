"""Host side of the V1 / V2 training tests: the case table of tests/helpers_family_train.py is well conditioned (bounds under the cap,
routes stable), its restatement is `oracle.amt_oracle.forward_family` where no dropout multiplier is given, every wrong variant is told
apart by some case, the models refuse what they do not train, and the library exports the new entry points.  No GPU."""
import re

import numpy as np
import pytest
import torch

from oracle import amt_oracle as O
from tests import helpers_family_train as FT
from tests.conftest import ROOT
from video2music_amd import _lib, ops


@pytest.mark.parametrize("name", FT.NAMES)
def test_case_is_well_conditioned(name):
    ref = FT.reference(name)
    print(f"{name}: e32 {ref['e32']:.3e} e32_y {ref['e32_y']:.3e} route gap {FT.route_gap(ref['gates']):.3e}")
    assert FT.FACTOR * ref["e32"] <= FT.CAP and FT.LOGIT_FACTOR * ref["e32_y"] <= FT.CAP
    assert FT.route_gap(ref["gates"]) >= FT.ROUTE_GAP
    c = FT.BY_NAME[name]
    assert len(ref["gates"]) == 2 * sum(1 for i in range(FT.built_layers(c)) if FT.ff_plan(c, i) != "glu")


@pytest.mark.parametrize("name", [n for n in FT.NAMES if FT.masks(n) == (None, None)])
def test_restatement_is_forward_family(name):
    c, f = FT.BY_NAME[name], FT.inputs(name)
    sd = {k: torch.from_numpy(v).double() for k, v in FT.state_dict(name).items()}
    fl = lambda k: torch.from_numpy(np.asarray(f[k])).double()
    with torch.no_grad():
        want = O.forward_family(sd, c.version, c.H, torch.from_numpy(f["ids"] if c.chord_embed else f["root"]), torch.from_numpy(f["attr"]),
                                fl("semantic"), fl("key"), fl("scene_offset"), fl("motion"), fl("emotion"), mask=c.mask)
        got = FT.forward_restated(sd, c, f, table64=True)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_unused_parameters_are_the_reference_s():
    for name in FT.NAMES:
        c = FT.BY_NAME[name]
        none = {k for k, v in FT.reference(name)["g64"].items() if v is None}
        want = {"embedding.weight", "condition_linear.weight", "condition_linear.bias"}
        if c.chord_embed:
            want |= {"embedding_root.weight", "embedding_attr.weight", "chord_embedding_model.weight"}
        assert none == want, name


def test_masks_cover_every_site_of_the_dropout_case():
    own, mix = FT.masks("v22_drop")
    kinds = [k for k, _ in FT.mask_shapes(FT.BY_NAME["v22_drop"])[0]]
    assert kinds[0] == "rows" and kinds.count("keep") == 4 + 8 and kinds.count("h") == 3 + 3 and len(mix) == 2 and all(len(m) == 3 for m in mix)
    assert own[0].shape == (3, 40) and 0 < own[0].mean() < 1


# variant -> the cases that can see it
VARIANT_CASES = {
    "rope_unconjugated": ("default", "long"),
    "rms_eps_1e-5": ("rms_hd128",),
    "glu_mask_forward_only": ("v22_drop",),
    "shared_without_1_over_k": ("v22", "nomask"),
    "chord_table_gradient": ("default", "v22"),
    "keep_unscaled": ("v22_drop",),
}


@pytest.mark.parametrize("variant", FT.VARIANTS)
def test_a_wrong_variant_misses_some_bound_by_ten(variant):
    miss = {n: FT.variant_miss(n, variant) for n in VARIANT_CASES[variant]}
    print(variant, {n: f"{m:.3g}" for n, m in miss.items()})
    assert max(miss.values()) >= FT.MISS, miss


# ---- refusals ----
def _call(m):
    z = torch.zeros(1, 2, dtype=torch.long)
    return m.train()(z, z, z, torch.zeros(1, 2, 8), torch.zeros(1), torch.zeros(1, 2), torch.zeros(1, 2, 1), torch.zeros(1, 2, 6))


@pytest.mark.parametrize("family,kw,message", [
    ("V2", dict(version_name="2.0"), "TopKScheduler"),
    ("V2", dict(version_name="2.1"), "TopKScheduler"),
    ("V2", dict(version_name="2.2", balancing=True, n_layers=4), "balancing=True"),
    ("V2", dict(version_name="2.2", num_heads=4), "head_dim 16"),
    ("V1", dict(version_name="1.1", num_heads=1, d_model=256), "head_dim 256"),
    ("V3", dict(version_name="3.0", n_layers=3), "differential attention"),
    ("V3", dict(version_name="3.1", n_layers=3), "differential attention"),
    ("V3", dict(version_name="3.2", n_layers=3), "differential attention"),
])
def test_training_forward_refuses(family, kw, message):
    from video2music_amd.model import video_music_transformer as M
    cls = getattr(M, "VideoMusicTransformer_" + family)
    m = cls(**dict(dict(n_layers=1, num_heads=2, d_model=64, dim_feedforward=64, total_vf_dim=16), **kw))
    with pytest.raises(NotImplementedError, match=message):
        _call(m)
    with torch.no_grad(), pytest.raises(_lib.AmtError, match="no CPU fallback"):       # every other state runs the code it ran before
        _call(m)


def test_training_forward_refuses_separate_heads(monkeypatch):
    from video2music_amd.model import video_music_transformer as M
    from video2music_amd.utilities import constants
    monkeypatch.setattr(constants, "IS_SEPERATED", True)
    m = M.VideoMusicTransformer_V1(version_name="1.1", n_layers=1, num_heads=2, d_model=64, dim_feedforward=64, total_vf_dim=16)
    with pytest.raises(NotImplementedError, match="IS_SEPERATED"):
        _call(m)


# ---- the library ----
NEW = ("amt_rope_bwd", "amt_rmsnorm_bwd", "amt_rmsnorm_bwd_blocks", "amt_glu_train_scratch_floats", "amt_glu_train_fwd", "amt_glu_bwd_ws_floats",
       "amt_glu_bwd")


def test_library_exports_the_training_entry_points():
    lib = _lib.load()
    header = open(f"{ROOT}/include/amt_hip.h").read()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(rf"\b{name}\(", header), name
    assert _lib.ABI_VERSION >= 12
    assert "#define AMT_RMSNORM_BWD_WS_FLOATS(dim) (4 + 128 * (dim))" in header          # ops.rmsnorm_bwd allocates this


def test_plan_and_scratch_rules_answer_without_a_device():
    assert [ops.rmsnorm_bwd_blocks(r) for r in (1, 16, 17, 2048, 2049, 100000)] == [1, 1, 2, 128, 128, 128]
    with pytest.raises(_lib.AmtError):
        ops.rmsnorm_bwd_blocks(0)
    assert _lib.call("amt_glu_train_scratch_floats", 129, 128, 1) == 3 * 129 * 128 + 4
    assert _lib.call("amt_glu_train_scratch_floats", 129, 128, 0) == 2 * 129 * 128 + 4
    assert _lib.call("amt_glu_bwd_ws_floats", 129, 32, 128) >= 2 * 129 * 128 + 129 * 32


def test_bad_arguments_are_refused_before_any_launch():
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_rope_bwd", None, None, None, 1, 1, 1, 2, 1, None)
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_rmsnorm_bwd", None, None, None, None, None, None, None, 4, 32, 1e-6, None)
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_glu_train_fwd", *[None] * 10, 4, 32, 32, 32, None)
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_glu_bwd", *[None] * 15, 4, 32, 32, 32, 1, None)
