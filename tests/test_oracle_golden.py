"""The CPU oracle (oracle/amt_oracle.py) against goldens produced by the reference itself
(oracle/make_goldens.py).  Runs without a GPU."""
import numpy as np
import pytest
import torch

from oracle import amt_oracle as O
from video2music_amd import synthetic
from video2music_amd.utilities import constants as C
from tests.helpers import CFG1, synthetic_sd, feats_t

TOL = 2e-5   # oracle vs reference logits (same fp32 arithmetic, different op grouping)


def test_kat_skew_pe_tables(golden):
    g = golden("g0_kat.npz")
    assert np.array_equal(O.skew(torch.from_numpy(g["skew_in"])).numpy(), g["skew_out"])
    assert g["skew_out"][0].tolist() == [[3, 0, 0, 0], [6, 7, 0, 0], [9, 10, 11, 0], [12, 13, 14, 15]]
    assert np.array_equal(O.skew(torch.from_numpy(g["skew_rand_in"])).numpy(), g["skew_rand_out"])
    pe = O.positional_encoding(300, 128)
    assert np.array_equal(pe[[0, 1, 2, 3, 150, 299]].numpy(), g["pe128_rows"])
    pe = O.positional_encoding(1024, 512)
    assert np.array_equal(pe[[0, 1, 2, 3, 511, 1023]].numpy(), g["pe512_rows"])
    for i in range(C.CHORD_END):
        assert tuple(g["chord_root_attr"][i]) == C.chord_to_root_attr(i) == O.root_attr_of(i)


def test_skew_equals_closed_form():
    rs = np.random.RandomState(0)
    q = torch.from_numpy(rs.standard_normal((2, 3, 17, 8)).astype(np.float32))
    Er = torch.from_numpy(rs.uniform(size=(40, 8)).astype(np.float32))
    qe = torch.einsum("bhld,md->bhlm", q, Er[40 - 17:])
    a = O.skew(qe)
    b = O.rpr_bias_closed_form(q, Er)
    tri = torch.tril(torch.ones(17, 17, dtype=torch.bool))
    assert torch.allclose(a[..., tri], b[..., tri], atol=1e-6)


@pytest.mark.parametrize("B,L", [(1, 1), (1, 12), (1, 64), (3, 1), (3, 12), (3, 64)])
def test_forward_logits(golden, B, L):
    g = golden("g_fwd_cfg1.npz")
    sd = synthetic_sd(CFG1)
    f = feats_t(synthetic.synthetic_features(3, seed=1234), slice(0, B), key=g["key"])
    logits = O.forward(sd, CFG1["num_heads"], torch.from_numpy(g[f"root_B{B}_L{L}"]), torch.from_numpy(g[f"attr_B{B}_L{L}"]),
                       f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
    assert logits.shape == (B, L, 159)
    assert np.abs(logits.numpy() - g[f"logits_B{B}_L{L}"]).max() < TOL


def test_forward_layer_activations(golden):
    g = golden("g_fwd_cfg1.npz")
    sd = synthetic_sd(CFG1)
    f = feats_t(synthetic.synthetic_features(3, seed=1234), key=g["key"])
    mem = O.encode(sd, 4, f["semantic"], f["scene_offset"], f["motion"], f["emotion"])
    assert np.abs(mem.numpy() - g["memory_B3"]).max() < TOL
    acts = []
    O.forward(sd, 4, torch.from_numpy(g["root_B3_L12"]), torch.from_numpy(g["attr_B3_L12"]),
              f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], collect=acts)
    for i, a in enumerate(acts):
        assert np.abs(a.numpy() - g[f"dec_layer{i}_B3_L12"]).max() < TOL


@pytest.mark.parametrize("clip", [0, 1])
def test_generate_g1_g2(golden, clip):
    g = golden("g_gen_cfg1.npz")
    key = golden("g_fwd_cfg1.npz")["key"]
    sd = synthetic_sd(CFG1)
    f = feats_t(synthetic.synthetic_features(3, seed=1234), slice(clip, clip + 1), key=key)
    pr, prr, pra = (torch.tensor([int(v)]) for v in g[f"primer_clip{clip}"])
    args = (sd, 4, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra)
    g1 = O.generate(*args, target_seq_length=64, beam=1)
    assert np.array_equal(g1.numpy(), g[f"g1_clip{clip}"])
    margins = []
    g2 = O.generate(*args, target_seq_length=64, beam=0, margins=margins)
    assert np.array_equal(g2.numpy(), g[f"g2_clip{clip}"])
    assert np.abs(np.array(margins) - g[f"g2_margins_clip{clip}"]).max() < 1e-4
    assert min(margins) > 1e-2          # the arg-max decisions of the fixture are well conditioned
    g2b = O.generate(*args, target_seq_length=64, beam=0, max_conseq_N=1, max_conseq_chord=3)
    assert np.array_equal(g2b.numpy(), g[f"g2_N1_c3_clip{clip}"])


GQA_SHAPES = [("q_proj.weight", (256, 256)), ("q_proj.bias", (256,)), ("k_proj.weight", (64, 256)), ("k_proj.bias", (64,)),
              ("v_proj.weight", (64, 256)), ("v_proj.bias", (64,)), ("norm.weight", (256,)), ("norm.bias", (256,)),
              ("out_proj.weight", (256, 256)), ("out_proj.bias", (256,))]


@pytest.mark.parametrize("L,B", [(6, 1), (6, 3), (64, 1), (64, 3)])
@pytest.mark.parametrize("causal", [False, True])
def test_gqa(golden, L, B, causal):
    g = golden("g_gqa.npz")
    sd = {k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(GQA_SHAPES, seed=3).items()}
    x = torch.from_numpy(g[f"x_L{L}_B{B}"])
    y = O.gqa_forward(x, x, x, sd, 8, 2, is_causal=causal)
    assert np.abs(y.numpy() - g[f"y_L{L}_B{B}_c{int(causal)}"]).max() < TOL


@pytest.mark.parametrize("name,dim", [("hd", 32), ("full", 256)])
def test_gqa_rope(golden, name, dim):
    """MultiheadGQA(RoPE=...) of the reference (grouped_query_attention.py:316-322): cache built for head_dim and for embed_dim."""
    g = golden("g_gqa_rope.npz")
    sd = {k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(GQA_SHAPES, seed=3).items()}
    cache = O.rope_cache(dim, 80)
    for L, B in ((6, 1), (6, 2), (64, 1), (64, 3)):
        x = torch.from_numpy(g[f"{name}_x_L{L}_B{B}"])
        for causal in (False, True):
            y = O.gqa_forward(x, x, x, sd, 8, 2, is_causal=causal, rope_cache_=cache)
            assert np.abs(y.numpy() - g[f"{name}_y_L{L}_B{B}_c{int(causal)}"]).max() < TOL, (L, B, causal)
    xq, xk = torch.from_numpy(g[f"{name}_xq"]), torch.from_numpy(g[f"{name}_xk"])
    y = O.gqa_forward(xq, xk, xk, sd, 8, 2, rope_cache_=cache)
    assert np.abs(y.numpy() - g[f"{name}_y_cross"]).max() < TOL


def moe_shapes(n_exp, d, dff, shared):
    out = [("gate.weight", (n_exp, d)), ("gate.bias", (n_exp,))]
    names = [f"experts.{e}." for e in range(n_exp)] + (["shared_expert."] if shared else [])
    for p in names:
        out += [(p + "linear1.weight", (dff, d)), (p + "linear1.bias", (dff,)),
                (p + "linear2.weight", (d, dff)), (p + "linear2.bias", (d,)),
                (p + "gate.weight", (dff, d)), (p + "gate.bias", (dff,))]
    return out


@pytest.mark.parametrize("name", ["moe", "shared"])
def test_moe(golden, name):
    g = golden("g_moe.npz")
    shared = name == "shared"
    sd = {k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(moe_shapes(8, 128, 256, shared), seed=5).items()}
    routing = {}
    y = O.moe_forward(torch.from_numpy(g["x"]), sd, 8, k=2, shared=shared, routing=routing)
    assert np.array_equal(routing["idx"].numpy(), g[f"idx_{name}"])
    assert np.abs(routing["weights"].numpy() - g[f"w_{name}"]).max() < 1e-6
    assert np.abs(y.numpy() - g[f"y_{name}"]).max() < TOL


def test_rms_rope(golden):
    g = golden("g_rms_rope.npz")
    y = O.rms_norm(torch.from_numpy(g["rms_x"]), torch.from_numpy(g["rms_w"]))
    assert np.abs(y.numpy() - g["rms_y"]).max() < 1e-6
    cache = O.rope_cache(128, 300)
    for B in (1, 2):
        x = torch.from_numpy(g[f"rope_x_B{B}"])
        L = x.shape[0]
        y = O.rope(x.view(4, L, B, 32), cache).reshape(L, B, 128)
        assert np.abs(y.numpy() - g[f"rope_y_B{B}"]).max() < 1e-6
    y = O.rope(torch.from_numpy(g["rope_hd_x"]), O.rope_cache(32, 64))
    assert np.abs(y.numpy() - g["rope_hd_y"]).max() < 1e-6


@pytest.mark.parametrize("B,L", [(1, 1), (1, 12), (2, 1), (2, 12)])
def test_v2_forward_logits(golden, B, L):
    """VideoMusicTransformer_V2 '2.2' (row f1): RoPE attention, GLU / shared-MoE feed-forwards."""
    from tests.helpers import CFG_V2, synthetic_sd_v2
    g = golden("g_v2_cfg1.npz")
    key = golden("g_fwd_cfg1.npz")["key"]
    sd = synthetic_sd_v2(CFG_V2)
    f = feats_t(synthetic.synthetic_features(3, seed=1234), slice(0, B), key=key)
    logits = O.forward_v2(sd, 4, torch.from_numpy(g[f"root_B{B}_L{L}"]), torch.from_numpy(g[f"attr_B{B}_L{L}"]),
                          f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
    assert np.abs(logits.numpy() - g[f"logits_B{B}_L{L}"]).max() < 5e-5      # 12 layers + MoE, logits of magnitude ~10


def test_v2_generate(golden):
    from tests.helpers import CFG_V2, synthetic_sd_v2
    g = golden("g_v2_cfg1.npz")
    key = golden("g_fwd_cfg1.npz")["key"]
    sd = synthetic_sd_v2(CFG_V2)
    f = feats_t(synthetic.synthetic_features(3, seed=1234), slice(0, 1), key=key)
    args = (sd, 4, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], torch.tensor([1]), torch.tensor([1]), torch.tensor([0]))
    assert np.array_equal(O.generate(*args, target_seq_length=24, beam=1, forward_fn=O.forward_v2).numpy(), g["g1"])
    margins = []
    g2 = O.generate(*args, target_seq_length=24, beam=0, forward_fn=O.forward_v2, margins=margins)
    assert np.array_equal(g2.numpy(), g["g2"])
    assert np.abs(np.array(margins) - g["g2_margins"]).max() < 1e-4


# ---------------- round 2: higher-entropy id fixtures and the reference at config 2 (oracle/make_goldens_cfg2.py) ----------------

def first_ill_conditioned(margins, thr=1e-3):
    """Index of the first decision whose top-1 / top-2 margin is below `thr` (len(margins) if none): ids are compared
    bit-exactly up to and including the token that decision produced only if it is well conditioned."""
    bad = np.nonzero(np.asarray(margins) < thr)[0]
    return int(bad[0]) if len(bad) else len(margins)


@pytest.mark.parametrize("clip", [0, 1])
def test_feedback_recipe_generate_hi_entropy(golden, clip):
    from tests.helpers import CFG1 as cfg
    g = golden("g_gen_hi.npz")
    ids = g[f"g2_clip{clip}"]
    assert len(set(ids.flatten().tolist())) >= 20 and g[f"g2_margins_clip{clip}"].min() >= 1e-2
    sd = synthetic_sd(cfg, recipe="feedback")
    f = feats_t(synthetic.synthetic_features(3, seed=1234), slice(clip, clip + 1), key=g["key"])
    pr, prr, pra = (torch.tensor([int(v)]) for v in g[f"primer_clip{clip}"])
    args = (sd, 4, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra)
    margins = []
    assert np.array_equal(O.generate(*args, target_seq_length=64, beam=0, margins=margins).numpy(), ids)
    assert np.abs(np.array(margins) - g[f"g2_margins_clip{clip}"]).max() < 1e-4
    assert np.array_equal(O.generate(*args, target_seq_length=64, beam=0, max_conseq_N=1, max_conseq_chord=3).numpy(), g[f"g2_N1_c3_clip{clip}"])
    assert np.array_equal(O.generate(*args, target_seq_length=64, beam=1).numpy(), g[f"g1_clip{clip}"])
    if clip == 0:
        lg = O.forward(sd, 4, torch.from_numpy(g["fwd_root"]), torch.from_numpy(g["fwd_attr"]), f["semantic"], f["key"], f["scene_offset"],
                       f["motion"], f["emotion"])
        assert np.abs(lg.numpy() - g["fwd_logits"]).max() < 1e-4


def test_config2_forward_full_length_vs_reference(golden):
    """d=512, 6+6 layers, L = max_sequence_chord = 1024 (er_len = 1024): the oracle against the reference's logits."""
    from tests.helpers import CFG2
    g = golden("g_cfg2.npz")
    sd = synthetic_sd(CFG2)
    f = feats_t(synthetic.synthetic_features(3, seed=1234), slice(0, 2), key=g["key"])
    with torch.no_grad():
        lg = O.forward(sd, 8, torch.from_numpy(g["fwd_root"]), torch.from_numpy(g["fwd_attr"]), f["semantic"], f["key"], f["scene_offset"],
                       f["motion"], f["emotion"]).numpy()
    assert np.abs(lg[0] - g["fwd_logits_clip0"]).max() < 1e-4
    assert np.abs(lg[1][g["fwd_pos_clip1"]] - g["fwd_logits_clip1"]).max() < 1e-4


@pytest.mark.parametrize("which,clip,recipe", [("default", 0, "default"), ("feedback", 1, "feedback")])
def test_config2_generate_prefix_vs_reference(golden, which, clip, recipe):
    """The oracle's feedback-greedy ids at config 2 against the reference's T=1024 run — its first 96 tokens here (a causal
    greedy generate to a shorter target is a prefix of the longer one); the GPU tests compare all 1024."""
    from tests.helpers import CFG2
    g = golden("g_cfg2.npz")
    ids, mg = g[f"g2_{which}_clip{clip}"], g[f"g2_{which}_margins_clip{clip}"]
    assert ids.shape == (1, 1024) and mg.shape == (1023,)
    T = 96
    sd = synthetic_sd(CFG2, recipe=recipe)
    f = feats_t(synthetic.synthetic_features(3, seed=1234), slice(clip, clip + 1), key=g["key"])
    prim = C.primer_from_name("C") if which == "default" else tuple(int(v) for v in g["primer_feedback_clip1"])
    pr, prr, pra = (torch.tensor([v]) for v in prim)
    margins = []
    with torch.no_grad():
        out = O.generate(sd, 8, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra,
                         target_seq_length=T, beam=0, margins=margins).numpy()
    n = min(first_ill_conditioned(mg) + 1, T)
    assert n == T and np.array_equal(out[0, :n], ids[0, :n])
    assert np.abs(np.array(margins) - mg[:T - 1]).max() < 1e-4


@pytest.mark.parametrize("clip", [0, 1])
def test_v2_well_conditioned_fixture(golden, clip):
    """g_v2_hi.npz (reference V2 '2.2', "feedback" recipe): every decision's margin >= 1e-2; the oracle reproduces the ids (the
    oracle's generate has no temperature: the temperature-1.0 run) and the forward logits."""
    from tests.helpers import CFG_V2, synthetic_sd_v2
    g = golden("g_v2_hi.npz")
    assert g[f"g2_t10_margins_clip{clip}"].min() >= 1e-2 and g[f"g2_t08_margins_clip{clip}"].min() >= 1e-2
    assert len(set(g[f"g2_t10_clip{clip}"].flatten().tolist())) >= 12
    sd = synthetic_sd_v2(CFG_V2, seed=int(g["seed"]), recipe="feedback")
    f = feats_t(synthetic.synthetic_features(3, seed=1234), slice(clip, clip + 1), key=g["key"])
    pr, prr, pra = (torch.tensor([int(v)]) for v in g[f"primer_clip{clip}"])
    args = (sd, 4, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra)
    assert np.array_equal(O.generate(*args, target_seq_length=48, beam=0, forward_fn=O.forward_v2).numpy(), g[f"g2_t10_clip{clip}"])
    assert np.array_equal(O.generate(*args, target_seq_length=48, beam=1, forward_fn=O.forward_v2).numpy(), g[f"g1_clip{clip}"])
    if clip == 0:
        lg = O.forward_v2(sd, 4, torch.from_numpy(g["fwd_root"]), torch.from_numpy(g["fwd_attr"]), f["semantic"], f["key"], f["scene_offset"],
                          f["motion"], f["emotion"])
        assert np.abs(lg.numpy() - g["fwd_logits"]).max() < 5e-4          # logits of magnitude ~60 with this recipe: 1e-5 relative


def base_embed_sd(tag):
    """state_dict of the base model with chord_embed / scene_embed as oracle/make_goldens_base_embed.py builds the reference."""
    from tests.helpers import CFG1
    from video2music_amd.utilities.constants import SCENE_OFFSET_MAX
    ce, se = "ce" in tag, "se" in tag
    cfg = dict(CFG1, total_vf_dim=CFG1["total_vf_dim"] - int(se))
    sd = dict(synthetic_sd(cfg))
    if se:
        sd["scene_embedding.weight"] = torch.from_numpy(synthetic.fill_tensor("scene_embedding.weight", (SCENE_OFFSET_MAX, cfg["d_model"]), 0))
    if ce:
        sd["chord_embedding_model.weight"] = torch.from_numpy(synthetic.fill_tensor("chord_embedding_model.weight", (159, cfg["d_model"]), 0))
    return cfg, sd, ce, se


@pytest.mark.parametrize("tag", ["ce", "se", "cese"])
def test_base_model_chord_embed_scene_embed(golden, tag):
    """Reference VideoMusicTransformer with chord_embed / scene_embed (model/video_music_transformer.py:926-937,986-987,1016-1027)."""
    g = golden("g_base_embed.npz")
    cfg, sd, ce, se = base_embed_sd(tag)
    assert len(sd) + 2 == int(g[f"{tag}_n_keys"])            # + the two positional-encoding buffers
    for B in (1, 2):
        f = feats_t(synthetic.synthetic_features(3, seed=1234), slice(0, B), key=g["key"])
        ids, root, attr = (torch.from_numpy(g[f"{tag}_{k}_B{B}"]) for k in ("x", "root", "attr"))
        lg = O.forward(sd, 4, ids if ce else root, attr, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
        assert np.abs(lg.numpy() - g[f"{tag}_logits_B{B}"]).max() < TOL
    f = feats_t(synthetic.synthetic_features(3, seed=1234), slice(0, 1), key=g["key"])
    args = (sd, 4, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], torch.tensor([1]), torch.tensor([1]), torch.tensor([0]))
    assert np.array_equal(O.generate(*args, target_seq_length=32, beam=1).numpy(), g[f"{tag}_g1"])
    margins = []
    assert np.array_equal(O.generate(*args, target_seq_length=32, beam=0, margins=margins).numpy(), g[f"{tag}_g2"])
    assert np.abs(np.array(margins) - g[f"{tag}_g2_margins"]).max() < 1e-4 and min(margins) > 1e-2


# ---------------- rarely used options of the reference classes (oracle/make_goldens_opts.py; VERDICT r1 missing #5) ----------------

@pytest.mark.parametrize("tag", ["beam3", "beam2_c05", "beam1_c03", "beam4_c07"])
def test_beam_and_beam_chance(golden, tag):
    """generate with beam > 1 / beam_chance < 1 as the reference code behaves (model/video_music_transformer.py:1074-1084)."""
    import random
    g = golden("g_opts.npz")
    beam, chance, seed, T = g[f"{tag}_args"]
    assert float(g[f"{tag}_min_gap"]) > 0.05                 # relative gap between neighbouring ranks of every top-k decision
    sd = synthetic_sd(CFG1, recipe="feedback")
    f = feats_t(synthetic.synthetic_features(3, seed=1234), slice(0, 1), key=g["key"])
    rng = random.Random(int(seed))
    ids = O.generate(sd, 4, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], torch.tensor([1, 30]), torch.tensor([1, 3]),
                     torch.tensor([0, 4]), target_seq_length=int(T), beam=int(beam), beam_chance=float(chance), rng=rng)
    assert ids.shape == (int(beam), int(T)) and np.array_equal(ids.numpy(), g[f"{tag}_ids"])


@pytest.mark.parametrize("B,L", [(1, 12), (2, 33), (1, 130)])
def test_forward_without_causal_mask(golden, B, L):
    g = golden("g_opts.npz")
    sd = synthetic_sd(CFG1, recipe="feedback")
    f = feats_t(synthetic.synthetic_features(3, seed=1234), slice(0, B), key=g["key"])
    lg = O.forward(sd, 4, torch.from_numpy(g[f"nomask_root_B{B}_L{L}"]), torch.from_numpy(g[f"nomask_attr_B{B}_L{L}"]), f["semantic"], f["key"],
                   f["scene_offset"], f["motion"], f["emotion"], mask=False)
    assert np.abs(lg.numpy() - g[f"nomask_logits_B{B}_L{L}"]).max() < 5e-4      # logits of magnitude ~130 with this recipe


def test_separated_heads(golden):
    g = golden("g_opts.npz")
    keys = set(g["sep_keys"].tolist())
    assert {"Wout_root.weight", "Wout_attr.bias", "Wout.weight"} <= keys        # the base class always holds the three heads (:973-975)
    sd = synthetic_sd(CFG1)
    f = feats_t(synthetic.synthetic_features(3, seed=1234), slice(0, 2), key=g["key"])
    yr, ya = O.forward(sd, 4, torch.from_numpy(g["sep_root"]), torch.from_numpy(g["sep_attr"]), f["semantic"], f["key"], f["scene_offset"],
                       f["motion"], f["emotion"], separated=True)
    assert np.abs(yr.numpy() - g["sep_y_root"]).max() < TOL and np.abs(ya.numpy() - g["sep_y_attr"]).max() < TOL


def test_v2_drop_token_rate_and_no_mask(golden):
    """VideoMusicTransformer_V2('2.2', 4 layers) with dropTokenRate=0.3 under torch.manual_seed(5), and with mask=False."""
    from tests.helpers import CFG_V2, synthetic_sd_v2
    g = golden("g_opts.npz")
    sd = synthetic_sd_v2(dict(CFG_V2, n_layers=4))
    f = feats_t(synthetic.synthetic_features(3, seed=1234), slice(0, 2), key=g["key"])
    args = (sd, 4, torch.from_numpy(g["fam_root"]), torch.from_numpy(g["fam_attr"]), f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
    torch.manual_seed(5)
    keep = torch.rand(2, f["semantic"].shape[1]) > 0.3
    assert np.array_equal(keep.numpy(), g["v22_drop_mask"])
    assert np.abs(O.forward_v2(*args, drop_keep=keep).numpy() - g["v22_drop_logits"]).max() < 1e-4       # fp32, logits of magnitude ~20
    assert np.abs(O.forward_v2(*args, mask=False).numpy() - g["v22_nomask_logits"]).max() < 1e-4


def test_shared_moe_temperature_scheduler(golden):
    """SharedMoELayer steps its temperature scheduler in eval mode too and divides the routing logits by it (moe.py:238-240, 288)."""
    g = golden("g_opts.npz")
    sd = {k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(moe_shapes(8, 128, 256, True), seed=5).items()}
    ts = [float(g[f"moe_t_t{c}"]) for c in range(3)]
    assert abs(ts[0] - 0.85) < 1e-9 and abs(ts[1] - 0.9) < 1e-9 and abs(ts[2] - 0.9) < 1e-9
    for c in range(3):
        y = O.moe_forward(torch.from_numpy(g["moe_t_x"]), sd, 8, k=2, shared=True, temperature=ts[c])
        assert np.abs(y.numpy() - g[f"moe_t_y{c}"]).max() < TOL
    assert np.abs(g["moe_t_y0"] - g["moe_t_y1"]).max() > 1e-4


def test_v2_bench_width_fixture(golden):
    """oracle/make_goldens_v2_wide.py: the reference V2 class at d_model 512 / 8 heads / d_ff 1024 / 6 layers."""
    from tests.helpers import CFG_V2, synthetic_sd_v2
    g = golden("g_v2_wide.npz")
    assert g["g2_margins"].min() >= 1e-2 and len(set(g["g2"].flatten().tolist())) >= 8
    sd = synthetic_sd_v2(dict(CFG_V2, n_layers=6, num_heads=8, d_model=512, dim_feedforward=1024), seed=int(g["seed"]), recipe="feedback")
    f = feats_t(synthetic.synthetic_features(2, seed=4321), slice(0, 1), key=g["key"])
    lg = O.forward_v2(sd, 8, torch.from_numpy(g["fwd_root"]), torch.from_numpy(g["fwd_attr"]), f["semantic"], f["key"], f["scene_offset"],
                      f["motion"], f["emotion"])
    assert np.abs(lg.numpy() - g["fwd_logits"]).max() < 1e-3           # logits of magnitude ~130: 1e-5 relative
    # the generated ids are the arg-max of the row before them (feedback-greedy, N suppressed, no triple repeats)
    ids = g["g2"][0]
    for cur in range(1, len(ids)):
        p = torch.softmax(lg[0, cur - 1], -1)[:157].clone()
        p[0] = 0.0
        if cur >= 2 and ids[cur - 1] == ids[cur - 2]:
            p[ids[cur - 1]] = 0.0
        assert int(p.argmax()) == int(ids[cur]), cur


def test_rpr_false_forward_and_generate(golden):
    """The oracle without relative-position tables (no `Er` rows in the state_dict) = the reference class built with rpr=False
    (torch's stock decoder layers, model/video_music_transformer.py:956-961): forward logits, G1, G2 of g_norpr.npz."""
    g = golden("g_norpr.npz")
    sd = {k: v for k, v in synthetic_sd(CFG1).items() if not k.endswith(".Er")}
    key = np.array([[0.0], [1.0], [0.0]], dtype=np.float32)
    f = feats_t(synthetic.synthetic_features(3, seed=1234), key=key)
    logits = O.forward(sd, 4, torch.from_numpy(g["root"]), torch.from_numpy(g["attr"]), f["semantic"], f["key"], f["scene_offset"],
                       f["motion"], f["emotion"])
    assert np.abs(logits.numpy() - g["logits"]).max() < TOL
    one = {k: v[:1] for k, v in f.items()}
    args = (sd, 4, one["semantic"], one["key"], one["scene_offset"], one["motion"], one["emotion"], torch.tensor([1]), torch.tensor([1]), torch.tensor([0]))
    assert np.array_equal(O.generate(*args, target_seq_length=48, beam=1).numpy(), g["g1"])
    assert np.array_equal(O.generate(*args, target_seq_length=48, beam=0).numpy(), g["g2"])


# ---------------- the model families: O.forward_family against the reference's V1 / V2 / V3 classes ----------------
# Bound: this file's convention, 5e-5 at logits of magnitude ~10 (test_v2_forward_logits), scaled by max(1, max|golden| / 10).  The
# float64 run's distance to the golden is printed next to it: that is the reference's own fp32 noise.
FAMILY_KEY = np.array([[0.0], [1.0], [0.0]], dtype=np.float32)
FAMILY_CFG = dict(n_layers=4, num_heads=4, d_model=128, dim_feedforward=256, total_vf_dim=synthetic.total_vf_dim(1))


def family_sd(version, seed=0, **over):
    from tests.helpers_family_parity import named_shapes
    cfg = dict(FAMILY_CFG, **over)
    if cfg.get("scene_embed"):
        cfg["total_vf_dim"] -= 1
    return cfg, {k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(named_shapes(version, **cfg), seed=seed).items()}


def check_family_golden(what, cfg, sd, version, want, x_root, x_attr, clips, feats=None, **kw):
    """forward_family in fp32 (asserted) and fp64 (printed) against the reference's logits `want`."""
    feats = synthetic.synthetic_features(3, seed=1234) if feats is None else feats
    dist = {}
    for dtype in (torch.float32, torch.float64):
        f = feats_t(feats, clips, key=FAMILY_KEY[:len(feats["key"])], dtype=dtype)
        with torch.no_grad():
            lg = O.forward_family({k: v.to(dtype) for k, v in sd.items()}, version, cfg["num_heads"], torch.from_numpy(x_root), torch.from_numpy(x_attr),
                                  f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], **kw)
        assert tuple(lg.shape) == want.shape
        dist[dtype] = float(np.abs(lg.numpy() - want).max())
    tol = 5e-5 * max(1.0, float(np.abs(want).max()) / 10.0)
    print(f"\nFAMILY_GOLDEN {what}: fp32 oracle {dist[torch.float32]:.2e}  fp64 oracle {dist[torch.float64]:.2e}  bound {tol:.2e}  "
          f"max|golden| {float(np.abs(want).max()):.1f}")
    assert dist[torch.float32] <= tol, (what, dist[torch.float32], tol)
    return dist


@pytest.mark.parametrize("tag,version,rms", [("v10", "1.0", False), ("v11", "1.1", False), ("v12", "1.2", False), ("v13", "1.3", False),
                                             ("v133", "1.3.3", False), ("v134", "1.3.4", False), ("v11rms", "1.1", True)])
def test_family_v1_vs_reference(golden, tag, version, rms):
    g = golden("g_v1.npz")
    cfg, sd = family_sd(version, rms_norm=rms)
    assert len(sd) == int(g[f"{tag}_n_keys"])
    check_family_golden(f"g_v1 {tag}", cfg, sd, version, g[f"{tag}_logits"], g[f"{tag}_root"], g[f"{tag}_attr"], slice(0, 2))


@pytest.mark.parametrize("tag,version,over", [("v20", "2.0", {}), ("v21", "2.1", {}), ("v22ce", "2.2", dict(chord_embed=True)),
                                              ("v22se", "2.2", dict(scene_embed=True))])
def test_family_v2_variants_vs_reference(golden, tag, version, over):
    g = golden("g_v2_variants.npz")
    cfg, sd = family_sd(version, n_layers=6, **over)
    for B in (1, 2):
        x_root = g[f"{tag}_x_B{B}"] if over.get("chord_embed") else g[f"{tag}_root_B{B}"]
        check_family_golden(f"g_v2_variants {tag} B{B}", cfg, sd, version, g[f"{tag}_logits_B{B}"], x_root, g[f"{tag}_attr_B{B}"], slice(0, B))


@pytest.mark.parametrize("tag,version", [("v30", "3.0"), ("v31", "3.1"), ("v32", "3.2")])
def test_family_v3_vs_reference(golden, tag, version):
    g = golden("g_v3.npz")
    cfg, sd = family_sd(version)
    assert len(sd) == int(g[f"{tag}_n_keys"])
    check_family_golden(f"g_v3 {tag} B2", cfg, sd, version, g[f"{tag}_logits"], g[f"{tag}_root"], g[f"{tag}_attr"], slice(0, 2))
    check_family_golden(f"g_v3 {tag} B1", cfg, sd, version, g[f"{tag}_logits1"], g[f"{tag}_root1"], g[f"{tag}_attr1"], slice(2, 3))


@pytest.mark.parametrize("tag,version", [("v22", "2.2"), ("v20", "2.0"), ("v11", "1.1"), ("v30", "3.0")])
def test_family_options_vs_reference(golden, tag, version):
    """dropTokenRate=0.3 under torch.manual_seed(5) and forward(mask=False) of the family classes (oracle/make_goldens_opts.py)."""
    g = golden("g_opts.npz")
    cfg, sd = family_sd(version)
    keep = torch.from_numpy(g[f"{tag}_drop_mask"])
    torch.manual_seed(5)
    assert torch.equal(torch.rand(2, 300) > 0.3, keep)
    check_family_golden(f"g_opts {tag} drop", cfg, sd, version, g[f"{tag}_drop_logits"], g["fam_root"], g["fam_attr"], slice(0, 2), drop_keep=keep)
    check_family_golden(f"g_opts {tag} nomask", cfg, sd, version, g[f"{tag}_nomask_logits"], g["fam_root"], g["fam_attr"], slice(0, 2), mask=False)


def test_forward_v2_is_the_family_member():
    """`forward_v2` keeps its signature and is version '2.2' of `forward_family`."""
    from tests.helpers import CFG_V2, synthetic_sd_v2
    sd = synthetic_sd_v2(dict(CFG_V2, n_layers=4))
    f = feats_t(synthetic.synthetic_features(2, seed=7, n_frames=40))
    rs = np.random.RandomState(3)
    root, attr = torch.from_numpy(rs.randint(0, 15, size=(2, 9))), torch.from_numpy(rs.randint(0, 16, size=(2, 9)))
    args = (root, attr, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
    ga, gb = [], []
    a = O.forward_v2(sd, 4, *args, collect=ga)
    b = O.forward_family(sd, "2.2", 4, *args, collect=gb)
    assert torch.equal(a, b) and len(ga) == len(gb) == 2 and all(torch.equal(p, q) for p, q in zip(ga, gb))


def test_float64_stays_float64():
    """rms_norm, rope, rope_cache and the mixture weights keep float64 (no rounding to fp32 inside a float64 run) and return for float32
    input what they returned before (test_rms_rope pins that to the reference)."""
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.standard_normal((4, 7, 2, 32)))
    w = torch.from_numpy(rs.uniform(0.5, 1.5, 32))
    y = O.rms_norm(x, w)
    assert y.dtype == torch.float64
    ref = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * w
    assert float((y - ref).abs().max()) < 1e-14 and float((O.rms_norm(x.float(), w.float()).double() - ref).abs().max()) > 1e-9
    c64, c32 = O.rope_cache(64, 300, dtype=torch.float64), O.rope_cache(64, 300)
    assert c64.dtype == torch.float64 and c32.dtype == torch.float32
    ang = torch.arange(300, dtype=torch.float64)[:, None] * (10000.0 ** (-torch.arange(0, 64, 2, dtype=torch.float64) / 64))[None, :]
    assert float((c64 - torch.stack([ang.cos(), ang.sin()], -1)).abs().max()) < 1e-12
    assert float((c32.double() - c64).abs().max()) < 3e-5                  # 299 x an fp32 rounding of theta
    r = O.rope(x, O.rope_cache(128, 300, dtype=torch.float64))            # (n_h, s, b, h_d) = (4, 7, 2, 32) with the d_model-wide cache
    assert r.dtype == torch.float64 and r.shape == x.shape
    assert float((r.pow(2).sum(-1) - x.pow(2).sum(-1)).abs().max()) < 1e-12   # rotations: every vector keeps its norm to float64 accuracy
    r32 = O.rope(x.float(), O.rope_cache(128, 300))
    assert r32.dtype == torch.float32 and 1e-9 < float((r32.double() - r).abs().max()) < 1e-5


@pytest.mark.parametrize("tag,version,rms", [("v12", "1.2", False), ("v10rms", "1.0", True), ("v20", "2.0", False), ("v31", "3.1", False),
                                             ("v32", "3.2", False)])
def test_family_second_configuration_vs_reference(golden, tag, version, rms):
    """oracle/make_goldens_families_alt.py: d_model 256, 2 heads (head_dim 128), 3 layers, dim_feedforward 192, B = 3, L = 40, 64
    frames -- where a wrong generalisation of the raw views no longer coincides with the right one; the V1 models also hold the
    gate logits of their six mixture layers."""
    g = golden("g_families_alt.npz")
    cfg, sd = family_sd(version, n_layers=3, num_heads=2, d_model=256, dim_feedforward=192, rms_norm=rms)
    assert len(sd) == int(g[f"{tag}_n_keys"])
    feats = synthetic.synthetic_features(3, seed=4242, n_frames=64)
    assert np.array_equal(feats["key"], g["key"])
    f = feats_t(feats)
    want = g[f"{tag}_logits"]
    assert want.shape == (3, 40, 159)
    dist = {}
    for dtype in (torch.float32, torch.float64):
        gates = []
        with torch.no_grad():
            lg = O.forward_family({k: v.to(dtype) for k, v in sd.items()}, version, 2, torch.from_numpy(g[f"{tag}_root"]), torch.from_numpy(g[f"{tag}_attr"]),
                                  *(f[k].to(dtype) for k in ("semantic", "key", "scene_offset", "motion", "emotion")), collect=gates)
        dist[dtype] = float(np.abs(lg.numpy() - want).max())
        n_gates = sum(1 for k in g if k.startswith(f"{tag}_gate"))
        assert len(gates) == n_gates == (6 if version[0] == "1" else 0)
        gd = max([float(np.abs(q.numpy() - g[f"{tag}_gate{i}"]).max()) for i, q in enumerate(gates)], default=0.0)
        if dtype == torch.float32:
            assert gd <= 5e-5, (tag, "gate logits", gd)
    tol = 5e-5 * max(1.0, float(np.abs(want).max()) / 10.0)
    print(f"\nFAMILY_GOLDEN g_families_alt {tag}: fp32 oracle {dist[torch.float32]:.2e}  fp64 oracle {dist[torch.float64]:.2e}  bound {tol:.2e}  "
          f"max|golden| {float(np.abs(want).max()):.1f}  gate logits {gd:.2e}")
    assert dist[torch.float32] <= tol, (tag, dist[torch.float32], tol)
