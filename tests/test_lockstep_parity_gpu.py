"""Logits of the lockstep V1 / V2 decode step (`amt_v2_step_batch`, what `generate_batch` and the device-decision `generate` run) and
of the one-clip step (`amt_v2_step`), teacher-forced along random chord sequences, against a high-precision reference of the same
clip, at every width the step accepts; and the ids of the device decision (`amt_v2_step_decide_batch`) against the decision rule
recomputed in fp64 from those logits.

References:
  * '2.2' without chord_embed: `oracle.amt_oracle.forward_v2` in fp64 (state dict and features cast to float64), run one clip at a time
    (for B > 1 the reference's raw RoPE view ties the clips of a batch together); row t of the causal forward is the step's logits at
    position t.  fp64 and fp32 may route a token to different experts at a near-tie of the 2nd and 3rd gate logits, so every row
    of every mixture layer (encoder and decoder) must keep that gap above ROUTE_GAP relative; a seed with such a tie is replaced.
  * Every clip, every family: the model's own teacher-forced fp32 `forward` on that clip alone.  That path shares no kernel with the
    step (dense prefill GEMM and prefill attention instead of the skinny GEMM and decode attention) and is pinned to the reference
    classes at default shapes by goldens (g_v1, g_v2_variants).  It is the only reference of the families the oracle does not hold:
    '2.0' (no rotary), '2.2' + chord_embed, V1 '1.0' / '1.1' / '1.3.3', rms_norm=True.

Error measure per configuration: max |got - ref| / max(1, max |ref|) over the compared clips and positions (logits of magnitude
~25-150).  Observed on an MI355X, max over the parameters of each test, fp64 oracle / fp32 forward; TOL keeps <= ~4x headroom:
  a  E 128, 300 positions           9.3e-7 / 1.8e-6      5e-6
  b  E 256, FFN fold 0 / 1 / 2      9.8e-7 / 1.1e-6      4e-6
  c  E 512, 32 / 33 clips, folds    9.7e-7 / 8.2e-7      3e-6
  d  E 768                          9.2e-7 / 1.1e-6      4e-6
  e  E 1024, 40 clips               9.6e-7 / 7.7e-7      3e-6
  f  E 1536 and 1280                8.9e-7 / 1.2e-6      4e-6
  g  E 256, 256 clips               1.8e-6 / 2.6e-6      8e-6
  h  S = 1, 17                      4.9e-7 / 1.2e-6      4e-6
  i  other families                      - / 9.9e-7      3e-6
  j  one-clip step, E 512 .. 1536   1.0e-6 / 1.3e-6      4e-6
The widths are chosen to reach the step's branches: E <= 768 with the norm folds on, 768 < E <= 1024 with the folds off and the
LayerNorm prologue at K = 1024, E > 1024 with unfused norms and the `settle` head, up to 256 clips (16 row blocks).
"""
import numpy as np
import pytest
import torch

from oracle import amt_oracle as O
from video2music_amd import synthetic
from video2music_amd.model.video_music_transformer import VideoMusicTransformer_V1, VideoMusicTransformer_V2
from video2music_amd.utilities import constants as C
from tests.helpers import (boundary_uniforms, check_argmax, check_draws, decision_inputs, feats_t, lockstep_step_logits,
                           one_clip_step_logits)

pytestmark = pytest.mark.gpu

ROUTE_GAP = 1e-5             # smallest 2nd-vs-3rd gate-logit gap (relative) of a row the fp64 comparison accepts
TOL = dict(a=5e-6, b=4e-6, c=3e-6, d=4e-6, e=3e-6, f=4e-6, g=8e-6, h=4e-6, i=3e-6, j=4e-6)     # see the table above


def build(cls=VideoMusicTransformer_V2, seed=0, recipe="default", **cfg):
    cfg = dict(dict(total_vf_dim=synthetic.total_vf_dim(1)), **cfg)
    m = cls(**cfg).eval()
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    sd = {k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(shapes, seed=seed, recipe=recipe).items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not missing and not unexpected
    return m.cuda(), sd


def chord_inputs(m, B, T, seed):
    """Random teacher-forced inputs (B, T): (root, attr) ids, pads included, or chord ids for chord_embed."""
    rs = np.random.RandomState(seed)
    if m.chord_embed:
        return torch.from_numpy(rs.randint(0, C.CHORD_SIZE, size=(B, T))), torch.zeros(B, T, dtype=torch.long)
    return torch.from_numpy(rs.randint(0, C.CHORD_ROOT_SIZE, size=(B, T))), torch.from_numpy(rs.randint(0, C.CHORD_ATTR_SIZE, size=(B, T)))


def fp64_clips(B):
    """The clips compared with the fp64 oracle: the first, both sides of every 16-row boundary, the last."""
    return sorted({0, B - 1} | {c for k in range(16, B, 16) for c in (k - 1, k)})


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / max(1.0, float(ref.abs().max())))


def forward_fp32(m, f, roots, attrs, c):
    """The model's teacher-forced forward of clip c alone: (T, 159)."""
    one = {k: v[c:c + 1] for k, v in f.items()}
    with torch.no_grad():
        return m(roots[c:c + 1], roots[c:c + 1], attrs[c:c + 1], one["semantic"], one["key"], one["scene_offset"], one["motion"],
                 one["emotion"])[0].cpu()


def oracle_fp64(m, sd64, f64, roots, attrs, c):
    """oracle.forward_v2 of clip c alone in fp64: (T, 159); asserts that no mixture-layer row sits at a routing near-tie."""
    gates = []
    one = {k: v[c:c + 1] for k, v in f64.items()}
    ref = O.forward_v2(sd64, m.nhead, roots[c:c + 1], attrs[c:c + 1], one["semantic"], one["key"], one["scene_offset"], one["motion"],
                       one["emotion"], max_seq_video=m.max_seq_video, collect=gates)[0]
    assert len(gates) == 2 * sum(1 for lyr in m.transformer.decoder.layers if hasattr(lyr.ff, "experts"))
    for li, g in enumerate(gates):
        s = g.sort(dim=-1, descending=True).values
        gap = (s[..., 1] - s[..., 2]) / s.abs().max(dim=-1).values.clamp(min=1.0)
        assert float(gap.min()) > ROUTE_GAP, f"clip {c}: mixture layer {li} has a routing near-tie ({float(gap.min()):.2e}); pick another seed"
    return ref


def check_config(name, m, sd, B, S, T, seed, one_clip=False):
    """Teacher-forces B clips of S frames along T random positions through the lockstep step (or, one_clip, clip 0 through the
    one-call step) and compares every clip with its fp32 forward and, for '2.2' without chord_embed, the fp64_clips with the oracle."""
    fc = feats_t(synthetic.synthetic_features(B, seed=seed, n_frames=S))
    f = {k: v.cuda() for k, v in fc.items()}
    roots, attrs = chord_inputs(m, B, T, seed)
    if one_clip:
        got = one_clip_step_logits(m, f, roots[0], attrs[0]).unsqueeze(1)
        B = 1
    else:
        got = lockstep_step_logits(m, f, roots, attrs)
    assert got.shape == (T, B, C.CHORD_SIZE) and torch.isfinite(got).all()
    e32 = max(rel_err(got[:, c], forward_fp32(m, f, roots, attrs, c)) for c in range(B))
    e64 = None
    if type(m) is VideoMusicTransformer_V2 and m.version_name == "2.2" and not m.chord_embed:
        sd64 = {k: v.double() for k, v in sd.items()}
        f64 = feats_t(synthetic.synthetic_features(B, seed=seed, n_frames=S), dtype=torch.float64)
        e64 = max(rel_err(got[:, c], oracle_fp64(m, sd64, f64, roots, attrs, c)) for c in fp64_clips(B))
    print(f"\nLOCKSTEP_PARITY {name}: fp64 {e64 if e64 is None else f'{e64:.2e}'}  fp32-forward {e32:.2e}  "
          f"|logits| {float(got.abs().max()):.1f}")
    assert e32 <= TOL[name[0]], (name, "fp32 forward", e32)
    if e64 is not None:
        assert e64 <= TOL[name[0]], (name, "fp64 oracle", e64)


def v2cfg(E, H, dff, n_layers, **kw):
    return dict(version_name="2.2", n_layers=n_layers, num_heads=H, d_model=E, dim_feedforward=dff, **kw)


# ---- a: the narrow default through the whole RoPE-capped sequence ----------------------------------------------------------------
@pytest.mark.parametrize("recipe", ["default", "feedback"])
def test_a_narrow_default_to_the_last_cache_row(recipe):
    """CFG_V2 widths (E 128, 4 heads, d_ff 256, 6 layers), 5 clips of 300 frames, T = the cache's 300 rows (the RoPE table caps a V2
    sequence at max_sequence_video): the last cache row is written and attended at pos = cap - 1."""
    m, sd = build(seed=1, recipe=recipe, **v2cfg(128, 4, 256, 6))
    assert m._max_dec == 300
    check_config(f"a/{recipe}", m, sd, B=5, S=300, T=m._max_dec, seed=11)


# ---- b: each fold mode of the plain GLU layers ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", ["0", "1", "2"])
def test_b_ffn_fold_modes(monkeypatch, fold):
    """E 256 / d_ff 256, 17 clips (a one-row second block): AMT_V2_FOLD_FFN off, norm3 folded into the next QKV (1), norm2 folded into
    the stacked gate | up product as well (2) -- each against the same references."""
    monkeypatch.setenv("AMT_V2_FOLD_FFN", fold)
    m, sd = build(seed=2, recipe="feedback", **v2cfg(256, 4, 256, 4))
    check_config(f"b/fold{fold}", m, sd, B=17, S=40, T=20, seed=21)


# ---- c: the bench width ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,fold,g1", [(32, "1", "1"), (33, "1", "1"), (33, "2", "1"), (33, "1", "0")])
def test_c_bench_width(monkeypatch, B, fold, g1):
    """E 512, 8 heads, d_ff 1024, 4 layers (three GLU, one mixture): 32 clips (two full row blocks) and 33 (a one-row tail block), the
    FFN fold modes 1 and 2, the norm1 -> query fold (G1) on and off."""
    monkeypatch.setenv("AMT_V2_FOLD_FFN", fold)
    monkeypatch.setenv("AMT_V2_FOLD_G1", g1)
    m, sd = build(seed=3, recipe="feedback", **v2cfg(512, 8, 1024, 4))
    check_config(f"c/B{B}/fold{fold}/g1{g1}", m, sd, B=B, S=48, T=16, seed=31 + B)


# ---- d, e, f: the width branches ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,H,dff,B,recipe", [
    (768, 12, 768, 16, "default"),          # d: the last width with both folds on (d_ff + E = 1536, 2 E = 1536)
    (1024, 8, 1024, 40, "feedback"),        # e: folds off, LayerNorm prologue at K = 1024, mixture gate | up N = 14336, 3 row blocks
    (1536, 12, 1536, 3, "default"),         # f: E > 1024: unfused norms (settle / norm_rows), the settle -> lin_rows head
    (1280, 10, 64, 3, "feedback"),          # f: 2 d_ff < E with unfused norms
])
def test_def_widths(E, H, dff, B, recipe):
    """Four layers (three GLU, one mixture: n_layers < 3 builds three GLU layers and no mixture), short clips to keep the fp64
    reference cheap."""
    name = {768: "d", 1024: "e"}.get(E, "f")
    m, sd = build(seed=E, recipe=recipe, **v2cfg(E, H, dff, 4))
    check_config(f"{name}/E{E}/dff{dff}", m, sd, B=B, S=24, T=12, seed=E + B)


# ---- g: the clip cap -----------------------------------------------------------------------------------------------------------
def test_g_256_clips():
    """E 256, 256 clips: 16 row blocks of the skinny GEMMs, the attention grid and the decision kernel."""
    m, sd = build(seed=7, recipe="default", **v2cfg(256, 4, 256, 4))
    check_config("g/B256", m, sd, B=256, S=17, T=8, seed=71)


# ---- h: short cross-attention memories -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 17])
def test_h_short_memories(S):
    """A one-frame and a ragged (17-frame) cross-attention memory."""
    m, sd = build(seed=8, recipe="feedback", **v2cfg(128, 4, 256, 6))
    check_config(f"h/S{S}", m, sd, B=5, S=S, T=24, seed=80 + S)


# ---- i: the families the oracle does not hold -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,cls,version,kw", [
    ("v20", VideoMusicTransformer_V2, "2.0", dict(n_layers=4)),                        # learned positional tables, no rotary
    ("v22ce", VideoMusicTransformer_V2, "2.2", dict(n_layers=4, chord_embed=True)),    # chord ids through the frozen table
    ("v10", VideoMusicTransformer_V1, "1.0", dict(n_layers=2)),                        # SiLU-only experts (relu = 2), no shared expert
    ("v11", VideoMusicTransformer_V1, "1.1", dict(n_layers=2)),                        # GLU experts, no shared expert
    ("v133", VideoMusicTransformer_V1, "1.3.3", dict(n_layers=4)),                     # three GLU layers, shared SiLU experts
    ("v11rms", VideoMusicTransformer_V1, "1.1", dict(n_layers=2, rms_norm=True)),      # RMSNorm: the settle launches
])
def test_i_families(tag, cls, version, kw):
    """E 512, 8 heads, d_ff 1024, 32 clips, against the fp32 forward of each clip."""
    m, sd = build(cls, seed=9, recipe="feedback", version_name=version, num_heads=8, d_model=512, dim_feedforward=1024, **kw)
    check_config(f"i/{tag}", m, sd, B=32, S=32, T=16, seed=91)


# ---- j: the one-clip step at the wide widths ------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,H,dff", [(512, 8, 1024), (1024, 8, 1024), (1536, 12, 1536)])
def test_j_one_clip_step(E, H, dff):
    """amt_v2_step (per-clip generate with decision="host"), so far compared at E 128 only."""
    m, sd = build(seed=E + 1, recipe="default", **v2cfg(E, H, dff, 4))
    check_config(f"j/E{E}", m, sd, B=1, S=24, T=12, seed=E + 3, one_clip=True)


# ---- the device decision of the lockstep family ---------------------------------------------------------------------------------
DRAW_CASES = [
    # family, B, sampler / beam, temperature, max_conseq_N, max_conseq_chord, P
    ("v22", 5, "categorical", 1.0, 0, 2, 1),
    ("v22", 33, "categorical", 0.7, 1, 3, 3),
    ("v22", 1, "categorical", 0.7, 0, 1, 3),
    ("v22ce", 5, "categorical", 1.0, 1, 2, 3),
    ("v10", 33, "categorical", 0.7, 0, 3, 1),
    ("v22", 5, "argmax", 0.7, 0, 2, 3),
    ("v11", 5, "argmax", 1.0, 1, 1, 1),
    ("v22ce", 33, "top1", 1.0, 0, 2, 1),
    ("v22", 1, "top1", 0.7, 0, 2, 3),
]


@pytest.mark.parametrize("family,B,sampler,temperature,mcn,mcc,P", DRAW_CASES)
def test_device_decision_draws(family, B, sampler, temperature, mcn, mcc, P):
    """generate_batch with the decision on the device (uniforms given), then the produced ids teacher-forced through the lockstep step:
    each id is the inverse-CDF draw of softmax(logits / temperature)[:157] after the N / repeat suppression at its uniform (1e-5 band), or
    for sampler="argmax" and beam=1 (top-1, no suppression, no root / attr feedback) the arg-max up to a 1e-6 tie band.  Random uniforms
    rarely fall near an interval's edge, so the Categorical draw is then repeated with uniforms placed 2e-5 of the mass inside each
    drawn id's interval (`boundary_uniforms`): the ids must not move.  (Observed on an MI355X: none moves at 3e-6; a temperature off by
    0.1 % moves hundreds at 1e-4.)"""
    cls, version, ce = {"v22": (VideoMusicTransformer_V2, "2.2", False), "v22ce": (VideoMusicTransformer_V2, "2.2", True),
                        "v10": (VideoMusicTransformer_V1, "1.0", False), "v11": (VideoMusicTransformer_V1, "1.1", False)}[family]
    m, _ = build(cls, seed=4, recipe="feedback", version_name=version, n_layers=4, num_heads=4, d_model=128, dim_feedforward=256,
                 chord_embed=ce)
    T = 32
    f = {k: v.cuda() for k, v in feats_t(synthetic.synthetic_features(B, seed=B + P, n_frames=64)).items()}
    names = ("C", "G", "A:min")[:P]
    pr, prr, pra = (torch.tensor(v) for v in zip(*[C.primer_from_name(n) for n in names]))
    u = torch.rand(T, B, generator=torch.Generator().manual_seed(B * 10 + P))
    beam = 1 if sampler == "top1" else 0
    kw = dict(target_seq_length=T, beam=beam, sampler="argmax" if sampler == "top1" else sampler, temperature=temperature,
              max_conseq_N=mcn, max_conseq_chord=mcc)
    args = (f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra)
    with torch.no_grad():
        toks = m.generate_batch(*args, uniforms=u if sampler == "categorical" else None, **kw).cpu()
    assert toks.shape == (B, T) and torch.equal(toks[:, :P], pr.expand(B, P))
    assert len(set(toks[:, P:].flatten().tolist())) >= (2 if sampler == "top1" else 4)
    roots, attrs = decision_inputs(toks, P, prr, pra, beam, ce)
    lg = lockstep_step_logits(m, f, roots, attrs)
    if sampler == "categorical":
        check_draws(toks, lg, u, P, mcn, mcc, temperature)
        u2 = boundary_uniforms(toks, lg, P, mcn, mcc, temperature, margin=2e-5)
        with torch.no_grad():
            again = m.generate_batch(*args, uniforms=u2, **kw).cpu()
        assert torch.equal(again, toks), (again != toks).nonzero()[:8].tolist()
    else:
        check_argmax(toks, lg, P, mcn, mcc, temperature, beam)
