"""Model-level parity of the HIP path: VideoMusicTransformer.forward / generate vs the reference
goldens (tests/golden, produced by the reference itself) and vs the CPU oracle."""
import numpy as np
import pytest
import torch

from oracle import amt_oracle as O
from video2music_amd import synthetic
from video2music_amd.model.video_music_transformer import VideoMusicTransformer
from video2music_amd.utilities import constants as C
from tests.helpers import CFG1, CFG2, synthetic_sd, feats_t
from tests.helpers import check_draws as _check_draws

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-3        # BASELINE.json: logits within 1e-3 fp32


def build(cfg, seed=0):
    m = VideoMusicTransformer(**cfg).eval()
    sd = synthetic_sd(cfg, seed)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing), (missing, unexpected)
    return m.cuda(), sd


@pytest.fixture(scope="module")
def model1():
    return build(CFG1)


def cu(f):
    return {k: v.cuda() for k, v in f.items()}


@pytest.mark.parametrize("B,L", [(1, 1), (1, 12), (1, 64), (3, 1), (3, 12), (3, 64)])
def test_forward_vs_reference_golden(golden, model1, B, L):
    m, _ = model1
    g = golden("g_fwd_cfg1.npz")
    f = cu(feats_t(synthetic.synthetic_features(3, seed=1234), slice(0, B), key=g["key"]))
    root, attr = torch.from_numpy(g[f"root_B{B}_L{L}"]).cuda(), torch.from_numpy(g[f"attr_B{B}_L{L}"]).cuda()
    with torch.no_grad():
        logits = m(torch.zeros_like(root), root, attr, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
    assert logits.shape == (B, L, 159)
    err = np.abs(logits.cpu().numpy() - g[f"logits_B{B}_L{L}"]).max()
    assert err < LOGIT_TOL, err


def test_forward_intermediates_vs_reference_golden(golden, model1):
    m, _ = model1
    g = golden("g_fwd_cfg1.npz")
    f = cu(feats_t(synthetic.synthetic_features(3, seed=1234), key=g["key"]))
    root, attr = torch.from_numpy(g["root_B3_L12"]).cuda(), torch.from_numpy(g["attr_B3_L12"]).cuda()
    for li in (0, 1):
        logits, memory, layer = m.forward_debug(root, attr, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], li)
        assert np.abs(memory.cpu().numpy() - g["memory_B3"]).max() < 1e-4
        assert np.abs(layer.cpu().numpy() - g[f"dec_layer{li}_B3_L12"]).max() < 1e-4
    assert np.abs(logits.cpu().numpy() - g["logits_B3_L12"]).max() < LOGIT_TOL


@pytest.mark.parametrize("clip", [0, 1])
def test_generate_vs_reference_golden(golden, model1, clip):
    """Chord ids bit-exact under greedy decode: G1 (beam=1) and G2 (sampling branch, arg-max sampler)."""
    m, _ = model1
    g = golden("g_gen_cfg1.npz")
    key = golden("g_fwd_cfg1.npz")["key"]
    f = cu(feats_t(synthetic.synthetic_features(3, seed=1234), slice(clip, clip + 1), key=key))
    pr, prr, pra = (torch.tensor([int(v)]) for v in g[f"primer_clip{clip}"])
    kw = dict(feature_semantic_list=f["semantic"], feature_key=f["key"][0], feature_scene_offset=f["scene_offset"],
              feature_motion=f["motion"], feature_emotion=f["emotion"], primer=pr, primer_root=prr, primer_attr=pra,
              target_seq_length=64)
    g1 = m.generate(beam=1, **kw)
    assert g1.shape == (1, 64) and g1.dtype == torch.long
    assert np.array_equal(g1.cpu().numpy(), g[f"g1_clip{clip}"])
    g2 = m.generate(beam=0, sampler="argmax", **kw)
    assert np.array_equal(g2.cpu().numpy(), g[f"g2_clip{clip}"])
    g2b = m.generate(beam=0, sampler="argmax", max_conseq_N=1, max_conseq_chord=3, **kw)
    assert np.array_equal(g2b.cpu().numpy(), g[f"g2_N1_c3_clip{clip}"])


def roots_attrs_of(toks, prr, pra):
    roots = torch.tensor([[C.chord_to_root_attr(int(t))[0] for t in row] for row in toks])
    attrs = torch.tensor([[C.chord_to_root_attr(int(t))[1] for t in row] for row in toks])
    roots[:, 0], attrs[:, 0] = prr, pra
    return roots, attrs


def test_generate_batch_equals_single_and_decode_logits_match_forward(model1):
    """Per clip a batched generate equals the B=1 run, and the KV-cached decode logits equal the
    teacher-forced forward over the generated prefix (prefix invariance)."""
    m, sd = model1
    feats = synthetic.synthetic_features(5, seed=77)
    key = np.array([[0.], [1.], [1.], [0.], [1.]], dtype=np.float32)
    f = cu(feats_t(feats, key=key))
    prim = torch.tensor([[1, 1, 0], [122, 10, 5], [1, 1, 0], [30, 3, 3], [122, 10, 5]])
    pr, prr, pra = prim[:, 0:1], prim[:, 1:2], prim[:, 2:3]
    T = 40
    toks, dec_logits = m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra,
                                        target_seq_length=T, beam=0, sampler="argmax", return_logits=True)
    for b in range(5):
        sl = slice(b, b + 1)
        one = m.generate_batch(f["semantic"][sl], f["key"][sl], f["scene_offset"][sl], f["motion"][sl], f["emotion"][sl],
                               pr[b], prr[b], pra[b], target_seq_length=T, beam=0, sampler="argmax")
        assert torch.equal(one[0], toks[b])
    # oracle (full re-forward, no cache) on clip 1 reproduces the ids
    fc = feats_t(feats, slice(1, 2), key=key)
    ref = O.generate(sd, CFG1["num_heads"], fc["semantic"], fc["key"], fc["scene_offset"], fc["motion"], fc["emotion"],
                     pr[1], prr[1], pra[1], target_seq_length=T, beam=0)
    assert torch.equal(ref[0], toks[1].cpu())
    # teacher-forced forward over the generated sequences
    roots, attrs = roots_attrs_of(toks.cpu(), prr[:, 0], pra[:, 0])
    with torch.no_grad():
        fwd = m(toks, roots.cuda(), attrs.cuda(), f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
    err = (fwd[:, :T - 1].permute(1, 0, 2) - dec_logits[:T - 1]).abs().max().item()
    assert err < 2e-4, err


def test_folded_and_plain_decode_chains_agree(monkeypatch):
    """The shipped decode chain folds every LayerNorm through the next projection (32 launches per step); the plain
    chain (49 launches, `AMT_DECODE_CHAIN=plain`, also the fallback for shapes the fold does not cover) must give
    the same ids and logits up to fp32 rounding."""
    feats = synthetic.synthetic_features(4, seed=99)
    f = cu(feats_t(feats))
    pr, prr, pra = (torch.tensor([v]) for v in C.primer_from_name("A:min"))
    out = {}
    for chain in ("folded", "plain"):
        if chain == "plain":
            monkeypatch.setenv("AMT_DECODE_CHAIN", "plain")     # read when the handle is finalized
        m, sd = build(CFG1, seed=3)
        out[chain] = m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra,
                                      target_seq_length=120, beam=0, sampler="argmax", return_logits=True)
    assert torch.equal(out["folded"][0], out["plain"][0])
    err = (out["folded"][1][:119] - out["plain"][1][:119]).abs().max().item()
    assert 0 < err < 1e-4, err        # > 0: the two chains really are different arithmetic


@pytest.mark.parametrize("mode", ["argmax", "categorical", "top1", "suppress"])
def test_sampling_head_in_the_next_steps_attention_equals_the_separate_launch(mode):
    """Inside a captured graph the sampling head of a step rides in the prologue of the NEXT step's first self-attention
    (attn_decode_sample_kernel: 30 launches per step; `fuse_sampling_head` = 0 keeps the 31-launch chain).  Same decision code, same
    table sums; the new position's own key is added after the cached ones instead of among them (fp32 summation order), so ids must be
    equal on a well-conditioned model and logits equal up to rounding.  Primers of three chords (decided positions start at 3),
    arg-max, the inverse-CDF draw at fixed uniforms, the top-1 branch, and N allowed / three equal chords suppressed."""
    cfg = dict(CFG1, n_layers=3)
    m = VideoMusicTransformer(**cfg).eval()
    m.load_state_dict(synthetic_sd(cfg, 11, recipe="feedback"), strict=False)
    m = m.cuda()
    B, T = 5, 70
    f = cu(feats_t(synthetic.synthetic_features(B, seed=77)))
    prim = torch.tensor([[1, 1, 0], [66, 6, 0], [122, 10, 5]]).t()
    kw = dict(target_seq_length=T, beam=0, sampler="argmax", return_logits=True)
    if mode == "categorical":
        kw.update(sampler="categorical", uniforms=torch.from_numpy(np.random.RandomState(5).rand(T, B).astype(np.float32)))
    elif mode == "top1":
        kw.update(beam=1, one_pass_top1=False)
    elif mode == "suppress":
        kw.update(max_conseq_N=1, max_conseq_chord=3)
    out = {}
    with torch.no_grad():
        for fuse in (1, 0):
            m.set_option("fuse_sampling_head", fuse)
            out[fuse] = m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], prim[0], prim[1], prim[2], **kw)
    assert torch.equal(out[1][0], out[0][0]), (out[1][0], out[0][0])
    assert torch.equal(out[1][0][:, :3].cpu(), prim[0].view(1, 3).expand(B, 3))
    err = (out[1][1][:T - 1] - out[0][1][:T - 1]).abs().max().item()
    assert err < 1e-4, err
    assert len(set(out[1][0][:, 3:].flatten().tolist())) >= (2 if mode == "top1" else 4)      # (top-1 never feeds its ids back)


def test_top1_branch_in_one_pass_equals_the_step_loop(model1):
    """beam=1 (oracle G1) never feeds its ids back, so one teacher-forced forward over (primer, PAD, ...) gives the
    same ids as T-1 decode steps; per-clip primers of length 3."""
    m, _ = model1
    f = cu(feats_t(synthetic.synthetic_features(4, seed=31)))
    prim = torch.tensor([[[1, 1, 0], [66, 6, 0], [122, 10, 5]]] * 4)
    prim[2, 1] = torch.tensor([5, 1, 4])
    a = m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], prim[:, :, 0], prim[:, :, 1], prim[:, :, 2],
                         target_seq_length=80, beam=1)
    b = m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], prim[:, :, 0], prim[:, :, 1], prim[:, :, 2],
                         target_seq_length=80, beam=1, one_pass_top1=False)
    assert a.shape == (4, 80) and torch.equal(a, b) and torch.equal(a[:, :3].cpu(), prim[:, :, 0])


@pytest.mark.parametrize("over", [dict(dim_feedforward=1536), dict(d_model=1024, num_heads=8, dim_feedforward=256, n_layers=1)])
def test_shapes_outside_the_fold_fall_back_to_the_plain_chain(over):
    """dim_feedforward + d_model > 1536, or 2 * d_model > 1536 (the folded G1 / G2 read [o | x]: found by the large-shape sweep, which
    drew d_model 1024 with a narrow feed-forward), does not fit the folded skinny GEMM (K <= 1536): the handle silently uses the
    plain 49-launch chain; ids still equal the oracle's."""
    cfg = dict(CFG1, **over)
    m, sd = build(cfg, seed=4)
    fc = feats_t(synthetic.synthetic_features(1, seed=8))
    f = cu(fc)
    pr, prr, pra = (torch.tensor([v]) for v in C.primer_from_name("C"))
    out = m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra,
                           target_seq_length=20, beam=0, sampler="argmax")
    ref = O.generate(sd, cfg["num_heads"], fc["semantic"], fc["key"], fc["scene_offset"], fc["motion"], fc["emotion"],
                     pr, prr, pra, target_seq_length=20, beam=0)
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("ff", [2048, 2560])
def test_feed_forward_wider_than_the_skinny_gemm_stages(ff):
    """dim_feedforward beyond 1536 (round 3: the cap was 1536): the decode step takes the plain chain and runs linear2 in column ranges
    of 1024 (2560 = 1024 + 1024 + 512), each range adding onto the ones before; forward logits and greedy ids against the oracle."""
    cfg = dict(CFG1, dim_feedforward=ff, n_layers=2)
    m, sd = build(cfg, seed=ff)
    fc = feats_t(synthetic.synthetic_features(2, seed=ff + 1))
    f = cu(fc)
    pr, prr, pra = (torch.tensor([v]) for v in C.primer_from_name("C"))
    T = 24
    with torch.no_grad():
        out = m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra, target_seq_length=T,
                               beam=0, sampler="argmax").cpu()
        rs = np.random.RandomState(ff)
        root = torch.from_numpy(rs.randint(1, 13, size=(2, 12)))
        attr = torch.from_numpy(rs.randint(1, 14, size=(2, 12)))
        y = m(root.cuda(), root.cuda(), attr.cuda(), f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"]).cpu()
    ref_y = O.forward(sd, cfg["num_heads"], root, attr, fc["semantic"], fc["key"], fc["scene_offset"], fc["motion"], fc["emotion"])
    assert (y - ref_y).abs().max().item() < LOGIT_TOL
    for b in range(2):
        one = {k: v[b:b + 1] for k, v in fc.items()}
        margins = []
        ref = O.generate(sd, cfg["num_heads"], one["semantic"], one["key"], one["scene_offset"], one["motion"], one["emotion"], pr, prr, pra,
                         target_seq_length=T, beam=0, margins=margins)
        assert min(margins) > 1e-4, margins
        assert torch.equal(out[b:b + 1], ref), (b, out[b], ref)


@pytest.mark.parametrize("d,H,ff", [(256, 4, 64), (128, 8, 64)])
def test_plain_chain_with_a_feed_forward_narrower_than_the_model(monkeypatch, d, H, ff):
    """The 49-launch chain (AMT_DECODE_CHAIN=plain) publishes LayerNorm(u2) from the prologue of the FFN-up product: with
    dim_feedforward < d_model that launch has fewer column tiles than the row has 16-column blocks (the case the V2 fuzz found);
    also head_dim 16 through both chains."""
    cfg = dict(CFG1, d_model=d, num_heads=H, dim_feedforward=ff, n_layers=2)
    fc = feats_t(synthetic.synthetic_features(2, seed=d + ff))
    f = cu(fc)
    pr, prr, pra = (torch.tensor([v]) for v in C.primer_from_name("C"))
    outs = []
    for chain in ("plain", "folded"):
        if chain == "plain":
            monkeypatch.setenv("AMT_DECODE_CHAIN", "plain")
        else:
            monkeypatch.delenv("AMT_DECODE_CHAIN", raising=False)
        m, sd = build(cfg, seed=d)
        outs.append(m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra,
                                     target_seq_length=18, beam=0, sampler="argmax").cpu())
        del m
    for b in range(2):
        one = {k: v[b:b + 1] for k, v in fc.items()}
        ref = O.generate(sd, H, one["semantic"], one["key"], one["scene_offset"], one["motion"], one["emotion"], pr, prr, pra,
                         target_seq_length=18, beam=0)
        assert torch.equal(outs[0][b:b + 1], ref) and torch.equal(outs[1][b:b + 1], ref)


@pytest.mark.parametrize("d,H,ff", [(256, 2, 512), (256, 8, 256), (192, 3, 320)])
def test_other_head_sizes_through_the_folded_chain(d, H, ff):
    """head_dim 128 / 32 / 64 with d_model not a power of two: greedy ids of the folded decode chain equal the oracle's and
    the decode logits equal the teacher-forced forward."""
    cfg = dict(CFG1, d_model=d, num_heads=H, dim_feedforward=ff, n_layers=3)
    m, sd = build(cfg, seed=d + H)
    fc = feats_t(synthetic.synthetic_features(2, seed=d))
    f = cu(fc)
    pr, prr, pra = (torch.tensor([v]) for v in C.primer_from_name("C"))
    T = 28
    toks, lg = m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra,
                                target_seq_length=T, beam=0, sampler="argmax", return_logits=True)
    one = {k: v[:1] for k, v in fc.items()}
    ref = O.generate(sd, H, one["semantic"], one["key"], one["scene_offset"], one["motion"], one["emotion"], pr, prr, pra,
                     target_seq_length=T, beam=0)
    assert torch.equal(toks[:1].cpu(), ref)
    roots, attrs = roots_attrs_of(toks.cpu(), int(prr[0]), int(pra[0]))
    with torch.no_grad():
        fwd = m(toks, roots.cuda(), attrs.cuda(), f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
    assert (fwd[:, :T - 1].permute(1, 0, 2) - lg[:T - 1]).abs().max().item() < 2e-4


def test_sampled_generate_is_valid_and_seeded(model1):
    m, _ = model1
    f = cu(feats_t(synthetic.synthetic_features(2, seed=5)))
    kw = dict(primer=torch.tensor([1]), primer_root=torch.tensor([1]), primer_attr=torch.tensor([0]), target_seq_length=24)
    torch.manual_seed(3)
    a = m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], **kw)
    torch.manual_seed(3)
    b = m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], **kw)
    assert torch.equal(a, b)
    assert a.shape == (2, 24) and int(a.min()) >= 1 and int(a.max()) < C.CHORD_END     # N suppressed, END/PAD impossible
    assert not bool(((a[:, 2:] == a[:, 1:-1]) & (a[:, 1:-1] == a[:, :-2])).any())      # no 3 equal ids in a row


def test_module_surface(model1):
    m, sd = model1
    ref_keys = set(sd) | {"positional_encoding.pe", "positional_encoding_video.pe"}
    assert set(m.state_dict().keys()) == ref_keys
    m.train()
    with pytest.raises(AssertionError):
        m.generate(primer=torch.tensor([1]), primer_root=torch.tensor([1]), primer_attr=torch.tensor([0]))
    m.eval()
    cpu = VideoMusicTransformer(**CFG1).eval()
    with pytest.raises(Exception, match="no CPU fallback"):
        cpu(torch.zeros(1, 2, dtype=torch.long), torch.zeros(1, 2, dtype=torch.long), torch.zeros(1, 2, dtype=torch.long),
            torch.zeros(1, 300, 768), torch.zeros(1), torch.zeros(1, 300), torch.zeros(1, 300, 512), torch.zeros(1, 300, 6))


def test_full_size_forward_vs_oracle_sample():
    """Config 2 (6 layers, d=512, max_sequence_chord=1024): logits vs the oracle on 2 clips, L=96."""
    m, sd = build(CFG2, seed=1)
    feats = synthetic.synthetic_features(2, seed=9)
    key = np.array([[1.], [0.]], dtype=np.float32)
    rs = np.random.RandomState(2)
    L = 96
    root = torch.from_numpy(rs.randint(0, 13, size=(2, L)))
    attr = torch.from_numpy(rs.randint(0, 14, size=(2, L)))
    fc = feats_t(feats, key=key)
    ref = O.forward(sd, 8, root, attr, fc["semantic"], fc["key"], fc["scene_offset"], fc["motion"], fc["emotion"])
    f = cu(fc)
    with torch.no_grad():
        out = m(root, root.cuda(), attr.cuda(), f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
    err = (out.cpu() - ref).abs().max().item()
    assert err < LOGIT_TOL, err


def test_full_size_generate_properties():
    """Config 2 at full size (B=32, T=1024): per-clip independence of the batch, suppression
    invariants, and decode logits == teacher-forced forward over the whole sequence."""
    m, sd = build(CFG2, seed=1)
    B, T = 32, 1024
    feats = synthetic.synthetic_features(B, seed=4321)
    f = cu(feats_t(feats))
    pr, prr, pra = (torch.tensor([v]) for v in C.primer_from_name("C"))
    toks, dec_logits = m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra,
                                        target_seq_length=T, beam=0, sampler="argmax", return_logits=True)
    assert toks.shape == (B, T) and int(toks.min()) >= 1 and int(toks.max()) < C.CHORD_END
    assert not bool(((toks[:, 2:] == toks[:, 1:-1]) & (toks[:, 1:-1] == toks[:, :-2])).any())
    # clips 3 and 17 alone give the same ids as inside the batch
    for b in (3, 17):
        sl = slice(b, b + 1)
        one = m.generate_batch(f["semantic"][sl], f["key"][sl], f["scene_offset"][sl], f["motion"][sl], f["emotion"][sl],
                               pr, prr, pra, target_seq_length=T, beam=0, sampler="argmax")
        assert torch.equal(one[0], toks[b])
    # teacher-forced forward over the generated ids reproduces the cached decode logits (4 clips)
    sub = slice(0, 4)
    tc = toks[sub].cpu()
    roots, attrs = roots_attrs_of(tc, int(prr[0]), int(pra[0]))
    with torch.no_grad():
        fwd = m(tc, roots.cuda(), attrs.cuda(), f["semantic"][sub], f["key"][sub], f["scene_offset"][sub], f["motion"][sub], f["emotion"][sub])
    err = (fwd[:, :T - 1].permute(1, 0, 2) - dec_logits[:T - 1, sub]).abs().max().item()
    assert err < 5e-4, err


def test_weight_reload_is_picked_up_by_captured_graphs():
    """load_state_dict after a generate: the repacked decode weights must be the ones the (already captured)
    step graph reads."""
    m, _ = build(CFG1, seed=0)
    f = cu(feats_t(synthetic.synthetic_features(2, seed=21)))
    kw = dict(primer=torch.tensor([1]), primer_root=torch.tensor([1]), primer_attr=torch.tensor([0]),
              target_seq_length=32, beam=0, sampler="argmax")
    a0 = m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], **kw)
    sd1 = synthetic_sd(CFG1, seed=5)
    m.load_state_dict(sd1, strict=False)
    a1 = m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], **kw)
    fresh, _ = build(CFG1, seed=5)
    b1 = fresh.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], **kw)
    assert torch.equal(a1, b1)
    assert not torch.equal(a0, a1)


def test_long_primer_short_video_and_batch_slicing(model1):
    """Edge cases: a 4-chord primer (generate.py's custumPrimer path), a clip shorter than max_sequence_video,
    and a batch larger than the 32-clip decode slice."""
    m, sd = model1
    # (1) primer C, A:min, D:min, G with per-chord root/attr as generate.py:286-339 encodes them
    names = ["C", "A:min", "D:min", "G"]
    prim = torch.tensor([C.primer_from_name(n) for n in names])          # (4, 3): id, root, attr
    feats = synthetic.synthetic_features(1, seed=31)
    fc = feats_t(feats)
    f = cu(fc)
    T = 24
    out = m.generate(f["semantic"], f["key"][0], f["scene_offset"], f["motion"], f["emotion"], prim[:, 0], prim[:, 1], prim[:, 2],
                     target_seq_length=T, beam=0, sampler="argmax")
    ref = O.generate(sd, 4, fc["semantic"], fc["key"], fc["scene_offset"], fc["motion"], fc["emotion"],
                     prim[:, 0], prim[:, 1], prim[:, 2], target_seq_length=T, beam=0)
    assert torch.equal(out.cpu(), ref) and out[0, :4].tolist() == prim[:, 0].tolist()
    g1 = m.generate(f["semantic"], f["key"][0], f["scene_offset"], f["motion"], f["emotion"], prim[:, 0], prim[:, 1], prim[:, 2],
                    target_seq_length=T, beam=1)
    ref1 = O.generate(sd, 4, fc["semantic"], fc["key"], fc["scene_offset"], fc["motion"], fc["emotion"],
                      prim[:, 0], prim[:, 1], prim[:, 2], target_seq_length=T, beam=1)
    assert torch.equal(g1.cpu(), ref1)
    # (2) 120-frame clip (the key capacity of the cross-attention stays 300)
    S = 120
    fs = {k: (v[:, :S].contiguous() if v.dim() > 1 and v.shape[1] == 300 else v) for k, v in fc.items()}
    root = torch.tensor([[1, 10, 3, 8, 14, 14]])
    attr = torch.tensor([[0, 5, 5, 0, 15, 15]])
    ref_logits = O.forward(sd, 4, root, attr, fs["semantic"], fs["key"], fs["scene_offset"], fs["motion"], fs["emotion"])
    fsc = cu(fs)
    with torch.no_grad():
        got = m(root, root.cuda(), attr.cuda(), fsc["semantic"], fsc["key"], fsc["scene_offset"], fsc["motion"], fsc["emotion"])
    assert (got.cpu() - ref_logits).abs().max().item() < LOGIT_TOL
    out_s = m.generate(fsc["semantic"], fsc["key"][0], fsc["scene_offset"], fsc["motion"], fsc["emotion"], prim[:1, 0], prim[:1, 1], prim[:1, 2],
                       target_seq_length=12, beam=0, sampler="argmax")
    ref_s = O.generate(sd, 4, fs["semantic"], fs["key"], fs["scene_offset"], fs["motion"], fs["emotion"],
                       prim[:1, 0], prim[:1, 1], prim[:1, 2], target_seq_length=12, beam=0)
    assert torch.equal(out_s.cpu(), ref_s)
    # (3) 35 clips: two decode slices (32 + 3); every clip equals its B=1 run
    f35 = cu(feats_t(synthetic.synthetic_features(35, seed=32)))
    toks = m.generate_batch(f35["semantic"], f35["key"], f35["scene_offset"], f35["motion"], f35["emotion"], prim[:1, 0], prim[:1, 1], prim[:1, 2],
                            target_seq_length=16, beam=0, sampler="argmax")
    assert toks.shape == (35, 16)
    for b in (0, 31, 32, 34):
        sl = slice(b, b + 1)
        one = m.generate_batch(f35["semantic"][sl], f35["key"][sl], f35["scene_offset"][sl], f35["motion"][sl], f35["emotion"][sl],
                               prim[:1, 0], prim[:1, 1], prim[:1, 2], target_seq_length=16, beam=0, sampler="argmax")
        assert torch.equal(one[0], toks[b])
    rs = np.random.RandomState(3)
    root35 = torch.from_numpy(rs.randint(0, 13, size=(35, 5))).cuda()
    attr35 = torch.from_numpy(rs.randint(0, 14, size=(35, 5))).cuda()
    with torch.no_grad():
        lg = m(root35, root35, attr35, f35["semantic"], f35["key"], f35["scene_offset"], f35["motion"], f35["emotion"])
        lg1 = m(root35[33:34], root35[33:34], attr35[33:34], f35["semantic"][33:34], f35["key"][33:34], f35["scene_offset"][33:34],
                f35["motion"][33:34], f35["emotion"][33:34])
    assert (lg[33:34] - lg1).abs().max().item() < 1e-5


@pytest.mark.parametrize("msv,S,B", [(500, 450, 2), (64, 40, 3), (1024, 1000, 1)])
def test_other_max_sequence_video(msv, S, B):
    """max_sequence_video other than the callers' 300 (the cross-attention key capacity and the video positional table follow it): clips of
    40 ... 1000 frames, ids and forward logits against the oracle."""
    cfg = dict(CFG1, max_sequence_video=msv)
    m = VideoMusicTransformer(**cfg).eval()
    sd = synthetic_sd(cfg, seed=msv, recipe="feedback")
    m.load_state_dict(sd, strict=False)
    m = m.cuda()
    fc = feats_t(synthetic.synthetic_features(B, seed=msv, n_frames=S))
    f = cu(fc)
    pr, prr, pra = (torch.tensor([v]) for v in C.primer_from_name("C"))
    T = 14
    out = m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra, target_seq_length=T, beam=0,
                           sampler="argmax").cpu()
    for b in range(B):
        one = {k: v[b:b + 1] for k, v in fc.items()}
        ref = O.generate(sd, 4, one["semantic"], one["key"], one["scene_offset"], one["motion"], one["emotion"], pr, prr, pra, target_seq_length=T, beam=0)
        assert torch.equal(out[b:b + 1], ref), (b, out[b], ref)
    rs = np.random.RandomState(1)
    root, attr = torch.from_numpy(rs.randint(0, 13, size=(B, 9))), torch.from_numpy(rs.randint(0, 14, size=(B, 9)))
    with torch.no_grad():
        lg = m(root, root.cuda(), attr.cuda(), f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"]).cpu()
    ref = O.forward(sd, 4, root, attr, fc["semantic"], fc["key"], fc["scene_offset"], fc["motion"], fc["emotion"])
    assert (lg - ref).abs().max().item() < LOGIT_TOL


def test_scalar_motion_feature_width():
    """motion_type 0: feature_motion is (B,S) and total_vf_dim = 776 (generate.py:146-149, forward :1012-1015)."""
    cfg = dict(CFG1, total_vf_dim=synthetic.total_vf_dim(0))
    m, sd = build(cfg, seed=2)
    fc = feats_t(synthetic.synthetic_features(2, seed=8, motion_type=0))
    assert fc["motion"].shape == (2, 300)
    root = torch.tensor([[1, 2, 3], [4, 5, 6]])
    attr = torch.tensor([[1, 0, 2], [3, 4, 5]])
    ref = O.forward(sd, 4, root, attr, fc["semantic"], fc["key"], fc["scene_offset"], fc["motion"], fc["emotion"])
    f = cu(fc)
    with torch.no_grad():
        got = m(root, root.cuda(), attr.cuda(), f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
    assert (got.cpu() - ref).abs().max().item() < LOGIT_TOL


@pytest.mark.parametrize("cfg,B,T,mcn,mcc", [(CFG1, 3, 48, 0, 2), (CFG1, 2, 40, 1, 3), (CFG2, 5, 96, 0, 2)])
def test_device_categorical_draw(cfg, B, T, mcn, mcc):
    """sampler="categorical": the draw done inside the step graph equals the inverse CDF of the decision distribution at
    the supplied uniforms; the same uniforms give the same ids; a batch row equals the clip alone."""
    m, _ = build(cfg, seed=2)
    f = cu(feats_t(synthetic.synthetic_features(B, seed=99)))
    pr, prr, pra = (torch.tensor(v) for v in zip(*[C.primer_from_name(n) for n in ("C", "G", "A:min")]))
    P = 3
    gen = torch.Generator().manual_seed(5)
    u = torch.rand(T, B, generator=gen)
    kw = dict(target_seq_length=T, beam=0, sampler="categorical", max_conseq_N=mcn, max_conseq_chord=mcc)
    args = (f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra)
    toks, logits = m.generate_batch(*args, uniforms=u, return_logits=True, **kw)
    assert torch.equal(toks[:, :P].cpu(), pr.expand(B, P))
    _check_draws(toks, logits, u, P, mcn, mcc)
    assert torch.equal(m.generate_batch(*args, uniforms=u, **kw), toks)
    one = m.generate_batch(*(a[1:2] for a in args[:5]), pr, prr, pra, uniforms=u[:, 1:2], **kw)
    assert torch.equal(one[0], toks[1])
    # the arg-max decision is back after the next begin (the switch is per generation)
    g2 = m.generate_batch(*args, target_seq_length=T, beam=0, sampler="argmax", max_conseq_N=mcn, max_conseq_chord=mcc)
    g2b = m.generate_batch(*args, target_seq_length=T, beam=0, sampler="argmax", max_conseq_N=mcn, max_conseq_chord=mcc)
    assert torch.equal(g2, g2b)


def test_device_categorical_draw_extremes_and_seed():
    """u = 0 picks the first id with positive mass, u -> 1 one at the top of the CDF; torch.manual_seed repeats a default run; the
    host-side multinomial sampler stays available and respects the suppression rules."""
    m, _ = build(CFG1, seed=2)
    B, T = 2, 24
    f = cu(feats_t(synthetic.synthetic_features(B, seed=7)))
    pr, prr, pra = (torch.tensor([v]) for v in C.primer_from_name("C"))
    args = (f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra)
    lo = m.generate_batch(*args, target_seq_length=T, beam=0, uniforms=torch.zeros(T, B))
    # with token 0 and a doubled previous id suppressed, u = 0 alternates between the two lowest ids
    assert set(lo[:, 1:].flatten().tolist()) <= {1, 2}
    uh = torch.full((T, B), 1.0 - 2.0 ** -24)
    hi, hl = m.generate_batch(*args, target_seq_length=T, beam=0, uniforms=uh, return_logits=True)
    _check_draws(hi, hl, uh, 1, 0, 2)          # the top of the CDF: the last ids that still carry mass above fp32 rounding
    assert int(hi[:, 1:].min()) > 100
    torch.manual_seed(11)
    a = m.generate_batch(*args, target_seq_length=T, beam=0)
    torch.manual_seed(11)
    b = m.generate_batch(*args, target_seq_length=T, beam=0)
    assert torch.equal(a, b) and int(a[:, 1:].min()) >= 1
    mn = m.generate_batch(*args, target_seq_length=T, beam=0, sampler="multinomial")
    assert int(mn[:, 1:].min()) >= 1 and int(mn.max()) < C.CHORD_END
    assert not bool(((mn[:, 2:] == mn[:, 1:-1]) & (mn[:, 1:-1] == mn[:, :-2])).any())


def test_rpr_false_vs_reference_golden(golden):
    """rpr=False (the class default): torch's stock decoder layers, i.e. no relative-position table -- forward, G1, G2 of
    the reference class built that way."""
    g = golden("g_norpr.npz")
    cfg = dict(CFG1, rpr=False)
    m = VideoMusicTransformer(**cfg).eval()
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert len(shapes) == int(g["n_keys"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(shapes, seed=0).items()}, strict=False)
    m = m.cuda()
    key = np.array([[0.0], [1.0], [0.0]], dtype=np.float32)
    f = cu(feats_t(synthetic.synthetic_features(3, seed=1234), key=key))
    root, attr = torch.from_numpy(g["root"]).cuda(), torch.from_numpy(g["attr"]).cuda()
    with torch.no_grad():
        y = m(root, root, attr, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
    err = np.abs(y.cpu().numpy() - g["logits"]).max()
    assert err < LOGIT_TOL, err
    kw = dict(feature_semantic_list=f["semantic"][:1], feature_key=f["key"][0], feature_scene_offset=f["scene_offset"][:1],
              feature_motion=f["motion"][:1], feature_emotion=f["emotion"][:1], primer=torch.tensor([1]), primer_root=torch.tensor([1]),
              primer_attr=torch.tensor([0]), target_seq_length=48)
    assert np.array_equal(m.generate(beam=1, **kw).cpu().numpy(), g["g1"])
    assert np.array_equal(m.generate(beam=0, sampler="argmax", **kw).cpu().numpy(), g["g2"])


# ---------------- round 2: the reference itself at the metric's configuration (tests/golden/g_cfg2.npz) ----------------

def _first_ill_conditioned(margins, thr=1e-3):
    bad = np.nonzero(np.asarray(margins) < thr)[0]
    return int(bad[0]) if len(bad) else len(margins)


@pytest.fixture(scope="module")
def model2():
    return build(CFG2)


def test_config2_forward_L1024_vs_reference_golden(golden, model2):
    """Reference VideoMusicTransformer(6 layers, d=512, H=8, dff=1024, max_sequence_chord=1024, rpr=True).forward at B=2,
    L=1024 (model/video_music_transformer.py:978-1043, rpr.py:391-455 with er_len = L): logits within 1e-3."""
    m, _ = model2
    g = golden("g_cfg2.npz")
    f = cu(feats_t(synthetic.synthetic_features(3, seed=1234), slice(0, 2), key=g["key"]))
    root, attr = torch.from_numpy(g["fwd_root"]).cuda(), torch.from_numpy(g["fwd_attr"]).cuda()
    with torch.no_grad():
        lg = m(torch.zeros_like(root), root, attr, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"]).cpu().numpy()
    assert lg.shape == (2, 1024, 159)
    e0 = np.abs(lg[0] - g["fwd_logits_clip0"]).max()
    e1 = np.abs(lg[1][g["fwd_pos_clip1"]] - g["fwd_logits_clip1"]).max()
    assert e0 < LOGIT_TOL and e1 < LOGIT_TOL, (e0, e1)


@pytest.mark.parametrize("which,clip,recipe", [("default", 0, "default"), ("feedback", 1, "feedback")])
def test_config2_generate_T1024_vs_reference_golden(golden, which, clip, recipe):
    """Feedback-greedy (G2) ids of the reference's own generate (:1046-1132) at T=1024, d=512: bit-exact while the reference's
    top-1 / top-2 margin stays above 1e-3 (the fixtures' minima are 4e-3 / 7e-3, so: all 1024); decode logits of the KV-cached
    folded chain vs the golden margins' scale are checked through the teacher-forced forward test above.  The clip also runs
    inside a batch of 32 (the bench's shape) and must give the same ids there."""
    g = golden("g_cfg2.npz")
    ids, mg = g[f"g2_{which}_clip{clip}"], g[f"g2_{which}_margins_clip{clip}"]
    m = VideoMusicTransformer(**CFG2).eval()
    m.load_state_dict(synthetic_sd(CFG2, recipe=recipe), strict=False)
    m = m.cuda()
    feats = synthetic.synthetic_features(3, seed=1234)
    f = cu(feats_t(feats, slice(clip, clip + 1), key=g["key"]))
    prim = C.primer_from_name("C") if which == "default" else tuple(int(v) for v in g["primer_feedback_clip1"])
    pr, prr, pra = (torch.tensor([v]) for v in prim)
    out = m.generate(feature_semantic_list=f["semantic"], feature_key=f["key"][0], feature_scene_offset=f["scene_offset"],
                     feature_motion=f["motion"], feature_emotion=f["emotion"], primer=pr, primer_root=prr, primer_attr=pra,
                     target_seq_length=1024, beam=0, sampler="argmax").cpu().numpy()
    n = min(_first_ill_conditioned(mg) + 1, 1024)
    assert n == 1024, n
    assert np.array_equal(out[0, :n], ids[0, :n]), int(np.nonzero(out[0] != ids[0])[0][0])
    assert len(set(ids.flatten().tolist())) >= (40 if which == "feedback" else 4)
    # the same clip as row 7 of a 32-clip batch (other rows: other synthetic clips)
    big = synthetic.synthetic_features(32, seed=555)
    for k in big:
        big[k][7] = feats[k][clip]
    key32 = big["key"].copy()
    key32[7] = g["key"][clip]
    fb = cu(feats_t(big, key=key32))
    toks = m.generate_batch(fb["semantic"], fb["key"], fb["scene_offset"], fb["motion"], fb["emotion"], pr, prr, pra,
                            target_seq_length=1024, beam=0, sampler="argmax")
    assert np.array_equal(toks[7].cpu().numpy(), ids[0])


@pytest.mark.parametrize("clip", [0, 1])
def test_feedback_recipe_generate_hi_entropy_vs_reference_golden(golden, clip):
    """Config 1 with the "feedback" weight recipe: >= 20 distinct ids in 64 tokens, margins >= 1e-2 (the round-1 fixtures
    visit 4-6 ids): G2, its suppression variant and G1 bit-exact, forward logits along the generated sequence."""
    g = golden("g_gen_hi.npz")
    m = VideoMusicTransformer(**CFG1).eval()
    m.load_state_dict(synthetic_sd(CFG1, recipe="feedback"), strict=False)
    m = m.cuda()
    f = cu(feats_t(synthetic.synthetic_features(3, seed=1234), slice(clip, clip + 1), key=g["key"]))
    pr, prr, pra = (torch.tensor([int(v)]) for v in g[f"primer_clip{clip}"])
    kw = dict(feature_semantic_list=f["semantic"], feature_key=f["key"][0], feature_scene_offset=f["scene_offset"],
              feature_motion=f["motion"], feature_emotion=f["emotion"], primer=pr, primer_root=prr, primer_attr=pra, target_seq_length=64)
    assert np.array_equal(m.generate(beam=0, sampler="argmax", **kw).cpu().numpy(), g[f"g2_clip{clip}"])
    assert np.array_equal(m.generate(beam=0, sampler="argmax", max_conseq_N=1, max_conseq_chord=3, **kw).cpu().numpy(), g[f"g2_N1_c3_clip{clip}"])
    assert np.array_equal(m.generate(beam=1, **kw).cpu().numpy(), g[f"g1_clip{clip}"])
    if clip == 0:
        root, attr = torch.from_numpy(g["fwd_root"]).cuda(), torch.from_numpy(g["fwd_attr"]).cuda()
        with torch.no_grad():
            lg = m(torch.zeros_like(root), root, attr, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
        assert np.abs(lg.cpu().numpy() - g["fwd_logits"]).max() < LOGIT_TOL


@pytest.mark.parametrize("tag", ["ce", "se", "cese"])
def test_base_model_chord_embed_scene_embed_vs_reference_golden(golden, tag):
    """chord_embed=True (chord ids through a frozen table; the ids feed back in both decision branches) and scene_embed=True
    (scene offsets through an embedding instead of a feature column) of the base class, :926-937,986-987,1016-1027."""
    from tests.test_oracle_golden import base_embed_sd
    g = golden("g_base_embed.npz")
    cfg, sd, ce, se = base_embed_sd(tag)
    m = VideoMusicTransformer(**cfg, chord_embed=ce, scene_embed=se).eval()
    assert len(m.state_dict()) == int(g[f"{tag}_n_keys"])
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing), (missing, unexpected)
    m = m.cuda()
    for B in (1, 2):
        f = cu(feats_t(synthetic.synthetic_features(3, seed=1234), slice(0, B), key=g["key"]))
        ids, root, attr = (torch.from_numpy(g[f"{tag}_{k}_B{B}"]).cuda() for k in ("x", "root", "attr"))
        with torch.no_grad():
            lg = m(ids, root, attr, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
        assert np.abs(lg.cpu().numpy() - g[f"{tag}_logits_B{B}"]).max() < LOGIT_TOL
    f = cu(feats_t(synthetic.synthetic_features(3, seed=1234), slice(0, 1), key=g["key"]))
    kw = dict(feature_semantic_list=f["semantic"], feature_key=f["key"][0], feature_scene_offset=f["scene_offset"], feature_motion=f["motion"],
              feature_emotion=f["emotion"], primer=torch.tensor([1]), primer_root=torch.tensor([1]), primer_attr=torch.tensor([0]),
              target_seq_length=32)
    assert np.array_equal(m.generate(beam=1, **kw).cpu().numpy(), g[f"{tag}_g1"])
    assert np.array_equal(m.generate(beam=0, sampler="argmax", **kw).cpu().numpy(), g[f"{tag}_g2"])
    # inside a batch of three (other clips alongside) the clip keeps its ids
    f3 = cu(feats_t(synthetic.synthetic_features(3, seed=1234), key=g["key"]))
    toks = m.generate_batch(f3["semantic"], f3["key"], f3["scene_offset"], f3["motion"], f3["emotion"], torch.tensor([1]), torch.tensor([1]),
                            torch.tensor([0]), target_seq_length=32, beam=0, sampler="argmax")
    assert np.array_equal(toks[0].cpu().numpy(), g[f"{tag}_g2"][0])


def test_more_than_32_clips_in_one_decode_chain():
    """`model.max_decode_batch` (default 32, the per-GPU batch of BASELINE.json) sizes the handle: with 48, forty clips decode as ONE
    lockstep chain (three 16-row blocks in the skinny GEMMs, 160 attention workgroups) and give the ids of the sliced default."""
    feats = synthetic.synthetic_features(40, seed=61)
    pr, prr, pra = (torch.tensor([v]) for v in C.primer_from_name("C"))
    outs = []
    for mdb in (32, 48):
        m, _ = build(CFG1, seed=6)
        m.max_decode_batch = mdb
        f = cu(feats_t(feats))
        toks, lg = m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra,
                                    target_seq_length=24, beam=0, sampler="argmax", return_logits=True)
        outs.append((toks.cpu(), lg.cpu()))
        root = torch.randint(0, 13, (40, 7), generator=torch.Generator().manual_seed(1))
        with torch.no_grad():
            outs[-1] += (m(root, root.cuda(), root.cuda(), f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"]).cpu(),)
    assert torch.equal(outs[0][0], outs[1][0])
    assert (outs[0][1] - outs[1][1]).abs().max().item() < 1e-5 and (outs[0][2] - outs[1][2]).abs().max().item() < 1e-5


# ---------------- rarely used options of the reference class (tests/golden/g_opts.npz, oracle/make_goldens_opts.py) ----------------

@pytest.fixture(scope="module")
def model1_feedback():
    m = VideoMusicTransformer(**CFG1).eval()
    m.load_state_dict(synthetic_sd(CFG1, recipe="feedback"), strict=False)
    return m.cuda()


@pytest.mark.parametrize("tag", ["beam3", "beam2_c05", "beam1_c03", "beam4_c07"])
def test_beam_and_beam_chance_vs_reference_golden(golden, model1_feedback, tag):
    """beam > 1 / beam_chance < 1 exactly as the reference code behaves (model/video_music_transformer.py:1074-1084): the (beam, T)
    matrix, with python's `random` seeded like the fixture's run and the Categorical draw replaced by arg-max."""
    import random
    g = golden("g_opts.npz")
    beam, chance, seed, T = g[f"{tag}_args"]
    f = cu(feats_t(synthetic.synthetic_features(3, seed=1234), slice(0, 1), key=g["key"]))
    random.seed(int(seed))
    out = model1_feedback.generate(feature_semantic_list=f["semantic"], feature_key=f["key"][0], feature_scene_offset=f["scene_offset"],
                                   feature_motion=f["motion"], feature_emotion=f["emotion"], primer=torch.tensor([1, 30]),
                                   primer_root=torch.tensor([1, 3]), primer_attr=torch.tensor([0, 4]), target_seq_length=int(T),
                                   beam=int(beam), beam_chance=float(chance), sampler="argmax")
    assert out.shape == (int(beam), int(T)) and np.array_equal(out.cpu().numpy(), g[f"{tag}_ids"])
    # generate_batch: row 0 of every clip's matrix
    random.seed(int(seed))
    toks = model1_feedback.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], torch.tensor([1, 30]),
                                          torch.tensor([1, 3]), torch.tensor([0, 4]), target_seq_length=int(T), beam=int(beam),
                                          beam_chance=float(chance), sampler="argmax")
    assert np.array_equal(toks.cpu().numpy(), g[f"{tag}_ids"][:1])


@pytest.mark.parametrize("B,L", [(1, 12), (2, 33), (1, 130)])
def test_forward_without_causal_mask_vs_reference_golden(golden, model1_feedback, B, L):
    g = golden("g_opts.npz")
    f = cu(feats_t(synthetic.synthetic_features(3, seed=1234), slice(0, B), key=g["key"]))
    root, attr = torch.from_numpy(g[f"nomask_root_B{B}_L{L}"]).cuda(), torch.from_numpy(g[f"nomask_attr_B{B}_L{L}"]).cuda()
    args = (root, root, attr, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
    with torch.no_grad():
        lg = model1_feedback(*args, mask=False).cpu().numpy()
        masked = model1_feedback(*args).cpu().numpy()               # the switch does not stick
    assert np.abs(lg - g[f"nomask_logits_B{B}_L{L}"]).max() < LOGIT_TOL
    if L > 1:
        assert np.abs(masked - lg).max() > 1e-2


def test_separated_heads_vs_reference_golden(golden, monkeypatch):
    """IS_SEPERATED = True (utilities/constants.py:11): forward returns (y_root, y_attr) from Wout_root / Wout_attr (:1036-1040);
    generate fails on the pair like the reference's softmax does."""
    import video2music_amd.model.video_music_transformer as vmt
    g = golden("g_opts.npz")
    m, _ = build(CFG1)
    f = cu(feats_t(synthetic.synthetic_features(3, seed=1234), slice(0, 2), key=g["key"]))
    root, attr = torch.from_numpy(g["sep_root"]).cuda(), torch.from_numpy(g["sep_attr"]).cuda()
    args = (root, root, attr, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
    with torch.no_grad():
        plain = m(*args)
        monkeypatch.setattr(vmt, "IS_SEPERATED", True)
        yr, ya = m(*args)
        with pytest.raises(TypeError):
            m.generate(f["semantic"][:1], f["key"][0], f["scene_offset"][:1], f["motion"][:1], f["emotion"][:1], torch.tensor([1]),
                       torch.tensor([1]), torch.tensor([0]), target_seq_length=8)
        monkeypatch.setattr(vmt, "IS_SEPERATED", False)
        again = m(*args)
    assert yr.shape == (2, 12, 15) and ya.shape == (2, 12, 16)
    assert np.abs(yr.cpu().numpy() - g["sep_y_root"]).max() < LOGIT_TOL and np.abs(ya.cpu().numpy() - g["sep_y_attr"]).max() < LOGIT_TOL
    assert torch.equal(plain, again)
