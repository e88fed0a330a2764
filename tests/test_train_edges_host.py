"""Input conditions of the training edge cases (tests/helpers_train_edges.py), on the CPU, before any GPU run: every case takes the
kernels it is named for (the library is asked, tests/launch_routes.py; each boundary the table is built around is proved through the
same queries, so that a retuned threshold fails here), the fixture of tests/helpers_train.py takes none of the 64-tile GEMMs, each
case's fp32 noise is in the range its bounds assume, and each wrong variant of the restatement misses those bounds by at least 10
times in every case named for it."""
import numpy as np
import pytest
import torch

from tests import helpers_train as T
from tests import helpers_train_edges as E
from tests import launch_routes as R
from video2music_amd.utilities import constants as C

NAMES = list(E.CASES)


def routes_of(name):
    c = E.CASES[name]
    return E.routes(c["cfg"], c["B"], c["S"], c["L"])


def test_launch_boundaries_are_the_librarys():
    """Every entry of R.BOUNDARIES is where the launcher's own rule flips (K moves in steps of 32, the head dims over the four built)."""
    b, g, a = R.BOUNDARIES, R.gemm_route, R.attn_route
    tiles = lambda n: (128 * n, 128)                                             # (M, N) of n 128x128 tiles
    lo, hi = b["split_hd"]
    flips = {            # name: (routes at the boundary and one step past it, what they must be)
        "small_m": ((g(b["small_m"], 32, 32), g(b["small_m"] + 1, 32, 32)), ("skinny", "tile64")),
        "small_mn": ((g(1, b["small_mn"], 32), g(1, b["small_mn"] + 1, 32)), ("skinny", "tile64")),
        "skinny_k": ((g(64, 64, b["skinny_k"]), g(64, 64, b["skinny_k"] + 32)), ("skinny", "tile64")),
        "t64_below": ((g(*tiles(b["t64_below"] - 1), b["big_k"]), g(*tiles(b["t64_below"]), b["big_k"])), ("tile64", "tile128")),
        "big_k": ((g(*tiles(b["t64_below"]), b["big_k"] - 32), g(*tiles(b["t64_below"]), b["big_k"])), ("tile64", "tile128")),
        "attn_row_block": ((a(1, b["split_grid"] - 1, b["attn_row_block"], b["split_lk"], lo),
                            a(1, b["split_grid"] - 1, b["attn_row_block"] + 1, b["split_lk"], lo)), ("splitk", "rows128")),
        "split_grid": ((a(b["split_grid"] - 1, 1, 32, b["split_lk"], hi), a(b["split_grid"], 1, 32, b["split_lk"], hi)), ("splitk", "rows128")),
        "split_lk": ((a(2, 2, 300, b["split_lk"] - 1, lo), a(2, 2, 300, b["split_lk"], lo)), ("rows128", "splitk")),
        "split_hd": ((a(2, 2, 300, 300, lo // 2), a(2, 2, 300, 300, lo), a(2, 2, 300, 300, hi), a(2, 2, 300, 300, 2 * hi)),
                     ("rows128", "splitk", "splitk", "rows128")),
    }
    assert set(flips) == set(b)
    for name, (got, want) in flips.items():
        assert got == want, f"{name} = {b[name]} of tests/launch_routes.py is not where the launcher's route flips: {got} instead of {want}"
    # further edges; a relative position table, a form only the library's own callers set, sigmoid and SiLU keep a shape off the fast route
    assert g(1000, b["small_mn"] // 1000, 64) == "skinny" and g(1000, b["small_mn"] // 1000 + 1, 64) == "tile64"
    assert E.gemm_kernel_and_epilogue(b["small_m"], 32, 32) == ("skinny", "none")
    assert E.gemm_kernel_and_epilogue(64, 65, b["big_k"]) == ("tile64", "none:elementwise")
    assert a(2, 2, 300, 300, 32, True) == "rows128" and g(64, 64, 64, 0, other_forms=True) == "tile64"
    assert [g(64, 64, 64, act) for act in (0, 1, 2, 3)] == ["skinny", "skinny", "tile64", "tile64"]


def test_the_fixture_reaches_no_64_tile_product_and_no_128_row_er_free_attention():
    """The statement the edge cases rest on: tests/test_train_gpu.py trains on the skinny GEMM and the split-key attention only."""
    for cfg in T.MODELS.values():
        g, a = E.routes(cfg, T.B_CLIPS, T.S_VIDEO, T.L_CHORD)
        assert {k for k, _ in g.values()} == {"skinny"}
        assert a["enc.self_attn"] == a["dec.multihead_attn"] == ("splitk", 32, False)     # and so does the plain decoder's self-attention
        assert a["dec.self_attn"] == (("rows128", 32, True) if cfg["rpr"] else ("splitk", 32, False))
        prods = E.products(cfg, T.B_CLIPS, T.S_VIDEO, T.L_CHORD)
        assert max(M * N for _, _, M, N, _, _ in prods) == 600 * 192 and ("bwd", "dec0.self_attn.qkv.dw", 192, 65, 608, 0) in prods
    assert T.CFG["total_vf_dim"] % 32 == 0                                       # its Linear_vis is never padded
    assert T.CFG["max_sequence_chord"] - T.L_CHORD == 1


def test_every_case_takes_the_kernels_it_is_named_for():
    g, a = routes_of("deployed_width")
    assert g["fwd", "enc0.self_attn.qkv"] == g["fwd", "dec0.self_attn.qkv"] == ("tile64", "none:vector")
    assert g["bwd", "enc0.self_attn.qkv.dw"] == g["bwd", "dec0.self_attn.qkv.dw"] == ("tile64", "none:elementwise")
    assert a == {"enc.self_attn": ("rows128", 64, False), "dec.self_attn": ("rows128", 64, True), "dec.multihead_attn": ("rows128", 64, False)}
    assert E.DEPLOYED["total_vf_dim"] % 32 == 8
    g, a = routes_of("deployed_300")
    assert g["fwd", "enc0.self_attn.qkv"][0] == "tile64" and a["enc.self_attn"] == a["dec.multihead_attn"] == ("splitk", 64, False)
    assert a["dec.self_attn"] == ("rows128", 64, True) and -(-299 // 128) == 3 and E.DEPLOYED["max_sequence_chord"] - 299 == 1
    g, a = routes_of("hd128_d1024")
    assert {v[:2] for v in a.values()} == {("rows128", 128)} and g["fwd", "enc0.self_attn.qkv"] == ("skinny", "none")
    assert g["bwd", "enc0.self_attn.qkv.dx"] == ("tile64", "none:vector") and g["bwd", "enc0.self_attn.qkv.dw"] == ("tile64", "none:elementwise")
    assert E.HD128["dim_feedforward"] < E.HD128["d_model"] == 1024 and E.HD128["max_sequence_chord"] - 33 == 7
    for name in ("d96_h3", "one_by_one", "L64", "L65", "all_pad_clip", "plain_noncausal"):
        assert {k for k, _ in routes_of(name)[0].values()} == {"skinny"}, name
    assert E.D96["d_model"] % 64 and E.D96["total_vf_dim"] % 32 == 5 and E.D96["max_sequence_chord"] - 37 == 27
    g, a = routes_of("rows_gt_4096")
    c = E.CASES["rows_gt_4096"]
    assert c["B"] * c["L"] > R.BOUNDARIES["small_m"] and c["B"] * c["L"] * 3 * 32 < R.BOUNDARIES["small_mn"] and c["B"] * c["L"] > 2048
    assert g["fwd", "dec0.linear1"] == ("tile64", "relu:vector") and g["fwd", "Wout"] == ("tile64", "none:elementwise")
    assert g["bwd", "Linear_chord.dx"] == ("tile64", "none:elementwise") and g["bwd", "dec0.linear1.dw"] == ("tile64", "none:elementwise")
    assert g["fwd", "enc0.self_attn.qkv"] == ("skinny", "none")                  # its 560 video rows stay on the skinny GEMM
    g, a = routes_of("k_gt_1536")
    fwd = {v[0] for (ps, _), v in g.items() if ps == "fwd"}
    dw = {v for (ps, n), v in g.items() if n.endswith(".dw")}
    assert fwd == {"skinny"} and dw == {("tile64", "none:elementwise")} and (13 * 129 + 31) // 32 * 32 > R.BOUNDARIES["skinny_k"]
    g, a = routes_of("plain_noncausal")
    assert a == {"enc.self_attn": ("splitk", 32, False), "dec.self_attn": ("rows128", 32, False), "dec.multihead_attn": ("splitk", 32, False)}
    assert not E.CASES["plain_noncausal"]["causal"] and not E.CASES["plain_noncausal"]["cfg"]["rpr"]


def test_route_list_over_the_table():
    """Which (pass, kernel, epilogue) and which attentions the table reaches.  `_forward_train` adds every residual inside its
    LayerNorm call, so no training product has the GEMM's residual epilogue, on either kernel."""
    reached, attn = {}, {}
    for name in NAMES:
        g, a = routes_of(name)
        for (ps, _), v in g.items():
            reached.setdefault((ps,) + v, []).append(name)
        for v in a.values():
            attn.setdefault(v, []).append(name)
    for k in sorted(reached):
        print(k, sorted(set(reached[k])))
    for k in sorted(attn):
        print("attention (kernel, head_dim, Er)", k, sorted(set(attn[k])))
    assert set(reached) == {("fwd", "skinny", "none"), ("fwd", "skinny", "relu"), ("fwd", "tile64", "none:vector"), ("fwd", "tile64", "none:elementwise"),
                            ("fwd", "tile64", "relu:vector"), ("bwd", "skinny", "none"), ("bwd", "tile64", "none:vector"),
                            ("bwd", "tile64", "none:elementwise")}
    assert {("rows128", 64, False), ("rows128", 128, False), ("rows128", 32, False), ("splitk", 32, False), ("splitk", 64, False),
            ("rows128", 32, True), ("rows128", 64, True), ("rows128", 128, True)} == set(attn)
    # the padded Linear_vis and an Er table longer than the sequence
    assert any(c["cfg"]["total_vf_dim"] % 32 for c in E.CASES.values())
    assert any(c["cfg"]["rpr"] and c["cfg"]["max_sequence_chord"] - c["L"] > 1 for c in E.CASES.values())


@pytest.mark.parametrize("name", NAMES)
def test_conditioning(name):
    c, r, bt = E.CASES[name], E.reference(name), E.batch(name)
    print(f"{name}: e32 {r['e32']:.3e} e32_y {r['e32_y']:.3e} loss {r['l64'][0]:.6f} loss bound {E.loss_bound(r):.2e}")
    assert 1e-7 < r["e32"] < 1e-5 and E.GRAD_FACTOR * r["e32"] <= 1e-4
    assert 0 < r["e32_y"] < 1e-5
    zero = tuple(k for k, g in r["g64"].items() if g is not None and not np.abs(g).max() > 0)
    assert zero == E.ZERO_GRADS.get(name, ())
    assert sorted(k for k, g in r["g64"].items() if g is None) == sorted(T.UNUSED)
    assert (bt["tgt"] != C.CHORD_PAD).any() and bt["key"][0] != 0
    assert bt["x_root"].max() == C.CHORD_ROOT_PAD or c["L"] < 16
    if c["L"] >= 4:
        assert bt["tgt"][0, -2] == C.CHORD_END and bt["tgt"][0, -1] == C.CHORD_PAD
    if c["all_pad"] is not None:
        assert (bt["tgt"][c["all_pad"]] == C.CHORD_PAD).all()
    assert sum(E.feature_widths(c["cfg"]["total_vf_dim"])) == c["cfg"]["total_vf_dim"] and min(E.feature_widths(c["cfg"]["total_vf_dim"])) >= 1
    if c["p"] > 0:
        m = E.masks(name)
        assert len(m) == 2 + 10 * c["cfg"]["n_layers"]
        assert all(not a[-1, -1, a.shape[2] // 2].any() for a in m if a.dtype == np.uint8)
    # no ReLU near its kink: the fp32 restatement moves a pre-activation by at most e32_z, the device is allowed 4 e32_z (the factor of
    # the logits), and the nearest unit is at least twice that from 0
    margin, e32_z = E.relu_margin(name)
    print(f"  smallest |pre-activation| {margin:.2e} = {margin / e32_z:.0f} e32_z")
    assert margin >= 8 * e32_z
    sd, plain = E.state_dict(name), T.state_dict(c["cfg"], c["seed"])
    moved = [k for k in sd if not c["small_norms"] and not np.array_equal(sd[k], plain[k])]
    assert set(moved) <= set(E.ffn_bias_keys(c["cfg"])) and all(np.abs(sd[k] - plain[k]).max() <= 16 * E.KINK * 2 for k in moved)
    # the restatement's own fp32 loss sits inside the loss bound
    assert abs(r["l32"][0] - r["l64"][0]) <= E.loss_bound(r)


@pytest.mark.parametrize("variant", list(E.VARIANTS))
def test_wrong_variant_misses_the_bounds(variant):
    _, forward_changes, cases = E.VARIANTS[variant]
    assert cases
    for name in cases:
        grad, logit, errs = E.variant_miss(name, variant)
        print(f"{variant} @ {name}: worst gradient {grad:.0f} bounds, logits {logit:.0f} bounds, "
              f"least-moved tensor {min(errs.values()) / (E.GRAD_FACTOR * E.reference(name)['e32']):.1f} bounds")
        assert grad >= E.MISS, (variant, name, grad)
        if forward_changes:
            assert logit >= E.MISS, (variant, name, logit)
        else:
            assert logit == 0.0


def test_eps_is_invisible_at_the_recipe_weights():
    """Why the small-norms cases exist: with the recipe's norm weights, eps 1e-6 moves no gradient tensor by 2 bounds."""
    for name in E.RECIPE_EPS_CASES:
        grad, logit, _ = E.variant_miss(name, "layernorm_eps_1e-6")
        print(f"{name}: eps 1e-6 moves the worst gradient by {grad:.2f} bounds, the logits by {logit:.2f}")
        assert grad < 2
    for name in E.VARIANTS["layernorm_eps_1e-6"][2]:
        _, _, errs = E.variant_miss(name, "layernorm_eps_1e-6")
        assert min(errs.values()) >= E.MISS * E.GRAD_FACTOR * E.reference(name)["e32"]      # there it moves every tensor


def test_grads_passes_causal_through():
    c = E.CASES["plain_noncausal"]
    bt = E.restated_batch(E.batch("plain_noncausal"), torch.float64)
    sd = E.state_dict("plain_noncausal")
    l, y, g = T.grads(sd, c["cfg"], bt, torch.float64, causal=False)
    r = E.reference("plain_noncausal")
    assert np.array_equal(y, r["y64"]) and np.array_equal(l, r["l64"])
    assert np.abs(T.grads(sd, c["cfg"], bt, torch.float64)[1] - y).max() > 1e-3
