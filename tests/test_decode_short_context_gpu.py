"""The short-context self-attention of the decode step (attn_decode.hip, SHORT instantiations; handle option
`short_context_attn`) and the bound guard of the attention that carries the sampling head.

The short-context kernels change the ORDER OF LOADS only (prologue first, one K/V batch clamped to the length, no second batch);
wave -> key mapping, per-lane online softmax, lane-group merge and the eight-wave combine are the long path's.  So every comparison
between the two is `torch.equal`: a tolerance here would hide a changed summation order."""
import ctypes as C

import numpy as np
import pytest
import torch

from video2music_amd import _lib, synthetic
from video2music_amd.model.video_music_transformer import VideoMusicTransformer
from tests.helpers import CFG2, synthetic_sd, feats_t

pytestmark = pytest.mark.gpu

T_CAP = 320
CFG = dict(CFG2, max_sequence_chord=T_CAP)          # config-2 width: 6 layers, 8 heads of 64, d_model 512


def sp():
    return _lib.stream_ptr()


def dev(t):
    return t.cuda().contiguous()


def rnd(rs, *shape, scale=1.0):
    return torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32))


@pytest.fixture(scope="module")
def model():
    m = VideoMusicTransformer(**CFG).eval()
    m.load_state_dict(synthetic_sd(CFG, 11, recipe="feedback"), strict=False)
    return m.cuda()


@pytest.fixture(scope="module")
def feats():
    return {k: v.cuda() for k, v in feats_t(synthetic.synthetic_features(3, seed=77)).items()}


PRIMER = torch.tensor([[1, 1, 0], [66, 6, 0], [122, 10, 5]]).t()      # (tokens, roots, attrs) of a three-chord primer


def run_generate(m, f, T, chunks=(-1,), short=1, fuse=1, kv_fill=None, total_steps=None):
    """Feedback-greedy generate of B clips driven like `generate_batch`, `amt_generate_run` fed `chunks` steps per call (cycled)
    until `total_steps` (default T - 1) are asked for.  Returns (tokens (B,T), logits (T,B,159), K/V cache or None).  kv_fill: the
    value every element of the self-attention K/V cache holds before the first step."""
    B = f["semantic"].shape[0]
    sem, key, scene, motion, emotion, B, S = m._prep_features(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
    h = m._ensure_handle(sem.shape[2])
    _lib.call("amt_set_option", h, b"short_context_attn", short)
    _lib.call("amt_set_option", h, b"fuse_sampling_head", fuse)
    pr = [p.cuda().long().contiguous() for p in PRIMER]
    lg = torch.zeros(T, B, 159, device="cuda")
    out = torch.empty(B, T, device="cuda", dtype=torch.long)
    kv = None
    with torch.no_grad():
        m._encode(h, sem, scene, motion, emotion, slice(0, B))
        if kv_fill is not None:
            dims = (C.c_int64 * 6)()
            _lib.call("amt_kv_cache_io", h, None, 0, 0, dims, sp())
            kv = torch.full(tuple(dims), kv_fill, device="cuda")
            _lib.call("amt_kv_cache_io", h, _lib.ptr(kv), kv.numel(), 1, None, sp())
        _lib.call("amt_generate_begin", h, B, _lib.ptr(pr[0]), _lib.ptr(pr[1]), _lib.ptr(pr[2]), 3, 0, _lib.ptr(key), T, 0, 0, 2, sp())
        asked, i = 0, 0
        total = T - 1 if total_steps is None else total_steps
        while asked < total:
            n = chunks[i % len(chunks)]
            i += 1
            _lib.call("amt_generate_run", h, n, _lib.ptr(lg), sp())
            asked = total if n < 0 else asked + n
        _lib.call("amt_generate_end", h, _lib.ptr(out), sp())
        if kv is not None:
            _lib.call("amt_kv_cache_io", h, _lib.ptr(kv), kv.numel(), 0, None, sp())
    torch.cuda.synchronize()
    _lib.call("amt_set_option", h, b"short_context_attn", 1)
    _lib.call("amt_set_option", h, b"fuse_sampling_head", 1)
    return out.cpu(), lg.cpu(), (kv.cpu() if kv is not None else None)


@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("chunks", [(-1,), (1,), (3,), (16,), (100,), (1, 3, 16, 100)])
def test_short_context_graphs_are_bit_equal_to_the_long_ones(model, feats, fuse, chunks):
    """B = 3, T = 320, feedback-greedy: logits at every position and the ids with `short_context_attn` 1 equal those with 0 exactly,
    with the sampling head inside the next step's attention and as its own launch, and with `n_steps` per call chosen so that graphs
    of 16 / 8 / 4 / 2 / 1 steps start at every offset: some straddle position 128 (and keep the long kernels), 1-step graphs run at
    both parities of the position."""
    T = T_CAP
    # (the same calls on both sides: where a graph starts decides which steps carry the head in their attention, and those add the
    # position's own key after the cached ones instead of among them -- another rounding, whatever the context length)
    ref_ids, ref_lg, _ = run_generate(model, feats, T, chunks, short=0, fuse=fuse)
    ids, lg, _ = run_generate(model, feats, T, chunks, short=1, fuse=fuse)
    assert torch.equal(ids, ref_ids), (ids != ref_ids).nonzero()[:8]
    assert torch.equal(lg[:T - 1], ref_lg[:T - 1]), (lg[:T - 1] != ref_lg[:T - 1]).any(-1).any(-1).nonzero().flatten()[:8]
    assert torch.equal(ids[:, :3], PRIMER[0].view(1, 3).expand(3, 3))
    assert len(set(ids[:, 3:].flatten().tolist())) >= 4           # the decisions feed back: a degenerate run would compare nothing


N_KEYS = (1, 127, 128, 129, 300)


@pytest.mark.parametrize("B,H,hd", [(3, 8, 64), (2, 4, 32), (2, 2, 128), (2, 8, 16)])
@pytest.mark.parametrize("n_keys", N_KEYS)
def test_short_kernel_plain_query_vs_fp64_and_the_long_kernel(B, H, hd, n_keys):
    """The short-context instantiation forced at 1, 127, 128, 129 and 300 keys (past one batch it loops, correctness does not rest on
    the host's choice): the reference and tolerance of test_ops_gpu.py::test_attention_decode, and bit-equal to the long kernel."""
    cap, pos = 301, n_keys - 1
    rs = np.random.RandomState(n_keys + B + hd)
    q = rnd(rs, B, H * hd, scale=0.5)
    kc, vc = rnd(rs, B, H, cap, hd), rnd(rs, B, H, cap, hd)
    er_len = cap + 5
    Er = torch.from_numpy(rs.uniform(size=(er_len, hd)).astype(np.float32))
    qh = q.view(B, H, 1, hd).double()
    s = qh @ kc[:, :, :pos + 1].double().transpose(-1, -2)
    idx = er_len - 1 - (pos - torch.arange(pos + 1))
    s = s + torch.einsum("bhqd,jd->bhqj", qh, Er[idx].double())
    ref = (torch.softmax(s, -1) @ vc[:, :, :pos + 1].double()).reshape(B, H * hd)
    o_long, o_short = torch.empty(B, H * hd, device="cuda"), torch.empty(B, H * hd, device="cuda")
    dq, dk, dv, de = dev(q), dev(kc), dev(vc), dev(Er)
    _lib.call("amt_attn_decode_fwd", _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(de), _lib.ptr(o_long), B, H, hd, cap, pos, er_len, sp())
    _lib.call("amt_attn_decode_fold_fwd", _lib.ptr(dq), H * hd, _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(de), None, None, None, None, None,
              None, _lib.ptr(o_short), B, H, hd, cap, None, n_keys, er_len, 2, 0.0, 1.0, sp())
    err = (o_short.cpu().double() - ref).abs().max().item()
    print("plain query", (B, H, hd, n_keys), "max |short - fp64| =", err)
    assert err < 2e-5
    assert torch.equal(o_short.cpu(), o_long.cpu())


def _ln64(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


@pytest.mark.parametrize("B,H,hd", [(3, 8, 64), (32, 8, 64), (2, 4, 32), (2, 8, 128), (2, 8, 16)])
@pytest.mark.parametrize("n_keys", N_KEYS)
def test_short_kernel_folded_prologue_vs_fp64_and_the_long_kernel(B, H, hd, n_keys):
    """The same for the folded-LayerNorm self-attention that brings the position's own key / value (layers > 0 of the decode step):
    n_keys counts the own key (position t = n_keys - 1, the cache holds t keys).  Reference and tolerances of
    test_ops_gpu.py::test_folded_decode_attention_random_sweep; output, LayerNorm row and the written cache rows bit-equal to the long
    kernel's."""
    d = H * hd
    cap, t = 301, n_keys - 1
    rs = np.random.RandomState(1000 + n_keys + B + hd)
    u = rnd(rs, B, d) + float(rs.uniform(-2, 2))
    gam, bet = 1 + rnd(rs, d, scale=0.2), rnd(rs, d, scale=0.1)
    W, bW = rnd(rs, 3 * d, d, scale=d ** -0.5), rnd(rs, 3 * d, scale=0.1)
    kc, vc = rnd(rs, B, H, cap, hd), rnd(rs, B, H, cap, hd)
    er_len = cap + 3
    Er = torch.from_numpy(rs.uniform(size=(er_len, hd)).astype(np.float32))
    scale = hd ** -0.5
    Wp = W.double() * gam.double()
    raw = (u.double() @ Wp.t()).float()
    g, c = Wp.sum(1).float(), (W.double() @ bet.double() + bW.double()).float()
    xn = _ln64(u.double(), gam.double(), bet.double())
    proj = xn @ W.double().t() + bW.double()
    q = (proj[:, :d] * scale).view(B, H, 1, hd)
    K, V = kc.double().clone(), vc.double().clone()
    K[:, :, t], V[:, :, t] = proj[:, d:2 * d].view(B, H, hd), proj[:, 2 * d:].view(B, H, hd)
    s = q @ K[:, :, :n_keys].transpose(-1, -2)
    idx = er_len - 1 - (t - torch.arange(n_keys))
    s = s + torch.einsum("bhqd,jd->bhqj", q, Er[idx].double())
    ref = (torch.softmax(s, -1) @ V[:, :, :n_keys]).reshape(B, d)
    pos = torch.tensor([t], dtype=torch.int32, device="cuda")
    d_raw, d_er, d_u, d_g, d_c, d_gam, d_bet = (dev(v) for v in (raw, Er, u, g, c, gam, bet))
    got = {}
    for flag in (1, 3):                                # new_kv, and new_kv with the short-context instantiation
        dk, dv = dev(kc), dev(vc)
        o, xo = torch.empty(B, d, device="cuda"), torch.empty(B, d, device="cuda")
        _lib.call("amt_attn_decode_fold_fwd", _lib.ptr(d_raw), 3 * d, _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(d_er),
                  _lib.ptr(d_u), _lib.ptr(d_g), _lib.ptr(d_c), _lib.ptr(d_gam), _lib.ptr(d_bet), _lib.ptr(xo), _lib.ptr(o),
                  B, H, hd, cap, _lib.ptr(pos), n_keys, er_len, flag, 1e-5, scale, sp())
        got[flag] = tuple(x.cpu() for x in (o, xo, dk, dv))
    o, xo, dk, dv = got[3]
    err = (o.double() - ref).abs().max().item()
    print("folded prologue", (B, H, hd, n_keys), "max |short - fp64| =", err)
    assert err < 5e-5
    assert (xo.double() - xn).abs().max().item() < 2e-5
    assert (dk.double()[:, :, t] - K[:, :, t]).abs().max().item() < 3e-5
    assert (dv.double()[:, :, t] - V[:, :, t]).abs().max().item() < 3e-5
    keep = torch.ones(cap, dtype=torch.bool)
    keep[t] = False
    assert torch.equal(dk[:, :, keep], kc[:, :, keep]) and torch.equal(dv[:, :, keep], vc[:, :, keep])     # only row t is touched
    for a, b in zip(got[3], got[1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("ask", ["exact", "more"])
def test_a_run_to_the_end_fills_the_last_position_and_leaves_the_padding_rows(model, feats, fuse, ask):
    """The attention that carries the sampling head writes its rows and advances the position only while the position lies inside
    the sequence and the cache (`t < T && t < cap`, read from the source: the case it exists for needs a failed launch and is not
    provoked).  Here: the guard does not bite a legal step.  A generate to exactly T = max_sequence_chord, asked for in steps that
    end exactly at T - 1, or for more steps than remain (clamped by amt_generate_run), writes tokens[:, T-1]; row T of every
    (layer, clip, head) slice of the K/V cache -- the padding row behind the T rows of keys -- still holds the test's fill value,
    rows 0 .. T-2 of the clips in use do not (row T-1's key would belong to a step the generate does not take)."""
    T = T_CAP
    FILL = 12345.0
    # 11 calls of 29 steps are the 319 steps exactly; 4 calls of 100 ask for 400, the last one with 19 remaining
    chunks, total = ((29,), T - 1) if ask == "exact" else ((100,), 400)
    ids, lg, kv = run_generate(model, feats, T, chunks, short=1, fuse=fuse, kv_fill=FILL, total_steps=total)
    ref_ids, ref_lg, _ = run_generate(model, feats, T, chunks, short=0, fuse=fuse, total_steps=total)
    assert torch.equal(ids, ref_ids) and torch.equal(lg[:T - 1], ref_lg[:T - 1])
    assert (ids[:, T - 1] >= 0).all() and (ids[:, T - 1] < 157).all(), ids[:, T - 1]       # a decided chord, not the PAD the rows start with
    assert kv.shape[4] == T + 1, kv.shape                       # an even max_sequence_chord gets one padding row per slice
    assert (kv[..., T, :] == FILL).all()
    B = ids.shape[0]
    assert (kv[:, :, :B, :, :T - 1, :] != FILL).all()
    assert (kv[:, :, B:] == FILL).all()
