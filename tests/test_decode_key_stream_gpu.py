"""The scalar-controlled key stream of the decode attentions (attn_decode.hip, the SCAL instantiations; handle option
`scalar_key_stream`, bit 2 of `amt_attn_decode_fold_fwd`'s new_kv, `amt_set_option` without a handle for the process-wide default).

The scalar stream changes WHICH LOADS are issued and how the loop is controlled (per wave: a scalar batch count, interior batches
without clamp or guard, the last batch clamped and guarded lane by lane with nothing requested behind it).  Wave -> key mapping,
the order in which a lane group consumes its keys, both merges and the own key's place are those of the previous stream, so every
comparison between the two is `torch.equal`: a tolerance would hide a changed summation order.  Against fp64 the restatements and
tolerances are those of tests/test_decode_short_context_gpu.py (2e-5 plain query, 5e-5 folded prologue)."""
import numpy as np
import pytest
import torch

from video2music_amd import _lib, synthetic
from video2music_amd.model.video_music_transformer import VideoMusicTransformer, VideoMusicTransformer_V2
from tests.helpers import CFG2, synthetic_sd, feats_t

pytestmark = pytest.mark.gpu

OLD = 4              # bit 2 of new_kv: the previous (per-lane controlled) key stream
B, H = 2, 2


def sp():
    return _lib.stream_ptr()


def dev(t):
    return t.cuda().contiguous()


def rnd(rs, *shape, scale=1.0):
    return torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32))


def key_counts(hd):
    """hd = 64 (a batch of S = 128 keys, G = 32 keys per key group of the workgroup, K = 4 keys per wave instruction): 1, 4, 5, 32, 33,
    127, 128, 129, 132, 133, 160, 161, 255, 256, 257, 288, 300, 383, 384, 385, 1023 -- every live-group count 1..4 of the last batch,
    waves with no keys, exactly full batches, an odd and an even number of batches per wave.  Other widths: the same set in their S, G, K."""
    K = 64 // (hd // 4)
    G, S = 8 * K, 32 * K
    return [1, K, K + 1, G, G + 1, S - 1, S, S + 1, S + K, S + K + 1, S + G, S + G + 1, 2 * S - 1, 2 * S, 2 * S + 1, 2 * S + G,
            2 * S + G + 3 * K, 3 * S - 1, 3 * S, 3 * S + 1, 8 * S - 1]


def test_the_key_counts_of_head_width_64():
    assert key_counts(64) == [1, 4, 5, 32, 33, 127, 128, 129, 132, 133, 160, 161, 255, 256, 257, 288, 300, 383, 384, 385, 1023]


COUNTS = {16: [512, 513], 32: key_counts(32), 64: key_counts(64), 128: key_counts(128)}


def _ln64(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


@pytest.mark.parametrize("hd", [64, 32, 128, 16])
def test_plain_self_attention_both_streams_and_fp64(hd):
    """FOLD 0 with the relative-position table: amt_attn_decode_fwd (scalar stream) against the same kernel on the previous stream
    (finished query through amt_attn_decode_fold_fwd, new_kv = 4) and the fp64 restatement, at every key count of the width."""
    counts = COUNTS[hd]
    cap = max(counts) + 2
    rs = np.random.RandomState(7 + hd)
    q = rnd(rs, B, H * hd, scale=0.5)
    kc, vc = rnd(rs, B, H, cap, hd), rnd(rs, B, H, cap, hd)
    er_len = cap + 5
    Er = torch.from_numpy(rs.uniform(size=(er_len, hd)).astype(np.float32))
    dq, dk, dv, de = dev(q), dev(kc), dev(vc), dev(Er)
    qh = q.view(B, H, 1, hd).double()
    for n_keys in counts:
        pos = n_keys - 1
        s = qh @ kc[:, :, :n_keys].double().transpose(-1, -2)
        idx = er_len - 1 - (pos - torch.arange(n_keys))
        s = s + torch.einsum("bhqd,jd->bhqj", qh, Er[idx].double())
        ref = (torch.softmax(s, -1) @ vc[:, :, :n_keys].double()).reshape(B, H * hd)
        o_new, o_old = torch.full((B, H * hd), 7.0, device="cuda"), torch.full((B, H * hd), 9.0, device="cuda")
        _lib.call("amt_attn_decode_fwd", _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(de), _lib.ptr(o_new), B, H, hd, cap, pos, er_len, sp())
        _lib.call("amt_attn_decode_fold_fwd", _lib.ptr(dq), H * hd, _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(de), None, None, None, None, None,
                  None, _lib.ptr(o_old), B, H, hd, cap, None, n_keys, er_len, OLD, 0.0, 1.0, sp())
        err = (o_new.cpu().double() - ref).abs().max().item()
        print("plain self-attention", (hd, n_keys), "max |scalar stream - fp64| =", err)
        assert err < 2e-5, (hd, n_keys, err)
        assert torch.equal(o_new.cpu(), o_old.cpu()), (hd, n_keys)


@pytest.mark.parametrize("hd", [64, 32, 128, 16])
def test_folded_self_attention_both_streams_and_fp64(hd):
    """FOLD 2 (folded LayerNorm, the position's own key / value from the prologue; n_keys counts the own key): output, LayerNorm row
    and the cache after the call equal on both streams, and the fp64 restatement of test_decode_short_context_gpu.py."""
    counts = COUNTS[hd]
    d = H * hd
    cap = max(counts) + 2
    rs = np.random.RandomState(1000 + hd)
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
    d_raw, d_er, d_u, d_g, d_c, d_gam, d_bet = (dev(v) for v in (raw, Er, u, g, c, gam, bet))
    for n_keys in counts:
        t = n_keys - 1
        K, V = kc.double().clone(), vc.double().clone()
        K[:, :, t], V[:, :, t] = proj[:, d:2 * d].view(B, H, hd), proj[:, 2 * d:].view(B, H, hd)
        s = q @ K[:, :, :n_keys].transpose(-1, -2)
        idx = er_len - 1 - (t - torch.arange(n_keys))
        s = s + torch.einsum("bhqd,jd->bhqj", q, Er[idx].double())
        ref = (torch.softmax(s, -1) @ V[:, :, :n_keys]).reshape(B, d)
        pos = torch.tensor([t], dtype=torch.int32, device="cuda")
        got = {}
        for flag in (1, 1 | OLD):
            dk, dv = dev(kc), dev(vc)
            o, xo = torch.empty(B, d, device="cuda"), torch.empty(B, d, device="cuda")
            _lib.call("amt_attn_decode_fold_fwd", _lib.ptr(d_raw), 3 * d, _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(d_er),
                      _lib.ptr(d_u), _lib.ptr(d_g), _lib.ptr(d_c), _lib.ptr(d_gam), _lib.ptr(d_bet), _lib.ptr(xo), _lib.ptr(o),
                      B, H, hd, cap, _lib.ptr(pos), n_keys, er_len, flag, 1e-5, scale, sp())
            got[flag] = tuple(x.cpu() for x in (o, xo, dk, dv))
        o, xo, dk, dv = got[1]
        err = (o.double() - ref).abs().max().item()
        print("folded self-attention", (hd, n_keys), "max |scalar stream - fp64| =", err)
        assert err < 5e-5, (hd, n_keys, err)
        assert (xo.double() - xn).abs().max().item() < 2e-5
        assert (dk.double()[:, :, t] - K[:, :, t]).abs().max().item() < 3e-5
        assert (dv.double()[:, :, t] - V[:, :, t]).abs().max().item() < 3e-5
        keep = torch.ones(cap, dtype=torch.bool)
        keep[t] = False
        assert torch.equal(dk[:, :, keep], kc[:, :, keep]) and torch.equal(dv[:, :, keep], vc[:, :, keep])     # only row t is touched
        for a, b in zip(got[1], got[1 | OLD]):
            assert torch.equal(a, b), (hd, n_keys)


@pytest.mark.parametrize("hd", [64, 32, 128, 16])
@pytest.mark.parametrize("n_keys", [300, 301])
def test_cross_attention_both_streams_and_fp64(hd, n_keys):
    """No relative-position table, a fixed key count: the plain query (FOLD 0) and the folded-LayerNorm query (FOLD 1) at 300 and 301
    keys, each on both streams and against fp64."""
    d = H * hd
    cap = n_keys
    rs = np.random.RandomState(50 + hd + n_keys)
    kc, vc = rnd(rs, B, H, cap, hd), rnd(rs, B, H, cap, hd)
    dk, dv = dev(kc), dev(vc)
    # plain query
    q = rnd(rs, B, d, scale=0.5)
    dq = dev(q)
    s = q.view(B, H, 1, hd).double() @ kc.double().transpose(-1, -2)
    ref = (torch.softmax(s, -1) @ vc.double()).reshape(B, d)
    o_new, o_old = torch.full((B, d), 7.0, device="cuda"), torch.full((B, d), 9.0, device="cuda")
    _lib.call("amt_attn_decode_fwd", _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), None, _lib.ptr(o_new), B, H, hd, cap, n_keys - 1, 0, sp())
    _lib.call("amt_attn_decode_fold_fwd", _lib.ptr(dq), d, _lib.ptr(dk), _lib.ptr(dv), None, None, None, None, None, None,
              None, _lib.ptr(o_old), B, H, hd, cap, None, n_keys, 0, OLD, 0.0, 1.0, sp())
    err = (o_new.cpu().double() - ref).abs().max().item()
    print("plain cross-attention", (hd, n_keys), "max |scalar stream - fp64| =", err)
    assert err < 2e-5
    assert torch.equal(o_new.cpu(), o_old.cpu())
    # folded query
    u = rnd(rs, B, d) + float(rs.uniform(-2, 2))
    gam, bet = 1 + rnd(rs, d, scale=0.2), rnd(rs, d, scale=0.1)
    W, bW = rnd(rs, d, d, scale=d ** -0.5), rnd(rs, d, scale=0.1)
    scale = hd ** -0.5
    Wp = W.double() * gam.double()
    raw = (u.double() @ Wp.t()).float()
    g, c = Wp.sum(1).float(), (W.double() @ bet.double() + bW.double()).float()
    xn = _ln64(u.double(), gam.double(), bet.double())
    qf = ((xn @ W.double().t() + bW.double()) * scale).view(B, H, 1, hd)
    ref = (torch.softmax(qf @ kc.double().transpose(-1, -2), -1) @ vc.double()).reshape(B, d)
    d_raw, d_u, d_g, d_c, d_gam, d_bet = (dev(v) for v in (raw, u, g, c, gam, bet))
    got = {}
    for flag in (0, OLD):
        o, xo = torch.empty(B, d, device="cuda"), torch.empty(B, d, device="cuda")
        _lib.call("amt_attn_decode_fold_fwd", _lib.ptr(d_raw), d, _lib.ptr(dk), _lib.ptr(dv), None,
                  _lib.ptr(d_u), _lib.ptr(d_g), _lib.ptr(d_c), _lib.ptr(d_gam), _lib.ptr(d_bet), _lib.ptr(xo), _lib.ptr(o),
                  B, H, hd, cap, None, n_keys, 0, flag, 1e-5, scale, sp())
        got[flag] = (o.cpu(), xo.cpu())
    err = (got[0][0].double() - ref).abs().max().item()
    print("folded cross-attention", (hd, n_keys), "max |scalar stream - fp64| =", err)
    assert err < 5e-5
    assert (got[0][1].double() - xn).abs().max().item() < 2e-5
    assert torch.equal(got[0][0], got[OLD][0]) and torch.equal(got[0][1], got[OLD][1])
    assert torch.equal(dk.cpu(), kc) and torch.equal(dv.cpu(), vc)


# ---------------- generate level ----------------

T_CAP = 320
CFG = dict(CFG2, max_sequence_chord=T_CAP)          # config-2 width: 6 layers, 8 heads of 64, d_model 512
PRIMER = torch.tensor([[1, 1, 0], [66, 6, 0], [122, 10, 5]]).t()      # (tokens, roots, attrs) of a three-chord primer


@pytest.fixture(scope="module")
def model():
    m = VideoMusicTransformer(**CFG).eval()
    m.load_state_dict(synthetic_sd(CFG, 11, recipe="feedback"), strict=False)
    return m.cuda()


@pytest.fixture(scope="module")
def feats():
    return {k: v.cuda() for k, v in feats_t(synthetic.synthetic_features(3, seed=77)).items()}


def run_generate(m, f, T, scalar, tables, fuse):
    """Feedback-greedy generate of B clips driven like `generate_batch` (the driver of tests/test_decode_short_context_gpu.py), 16
    steps per call.  Returns (tokens (B,T), logits (T,B,159))."""
    sem, key, scene, motion, emotion, nb, S = m._prep_features(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
    h = m._ensure_handle(sem.shape[2])
    opts = {b"scalar_key_stream": scalar, b"layer0_kv_from_tables": tables, b"fuse_sampling_head": fuse}
    for name, v in opts.items():
        _lib.call("amt_set_option", h, name, v)
    try:
        pr = [p.cuda().long().contiguous() for p in PRIMER]
        lg = torch.zeros(T, nb, 159, device="cuda")
        out = torch.empty(nb, T, device="cuda", dtype=torch.long)
        with torch.no_grad():
            m._encode(h, sem, scene, motion, emotion, slice(0, nb))
            _lib.call("amt_generate_begin", h, nb, _lib.ptr(pr[0]), _lib.ptr(pr[1]), _lib.ptr(pr[2]), 3, 0, _lib.ptr(key), T, 0, 0, 2, sp())
            for _ in range((T - 1 + 15) // 16):
                _lib.call("amt_generate_run", h, 16, _lib.ptr(lg), sp())
            _lib.call("amt_generate_end", h, _lib.ptr(out), sp())
        torch.cuda.synchronize()
    finally:
        for name in opts:
            _lib.call("amt_set_option", h, name, 1)
    return out.cpu(), lg.cpu()


@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("tables", [1, 0])
def test_generate_is_bit_equal_on_both_streams(model, feats, tables, fuse):
    """B = 3, T = 320: ids and the logits of every step under `scalar_key_stream` 0 and 1, with layer 0's keys from the tables and
    from the cache and with the sampling head inside the next step's attention (FOLD 5 and its table-sourced form) and on its own."""
    T = T_CAP
    ref_ids, ref_lg = run_generate(model, feats, T, 0, tables, fuse)
    ids, lg = run_generate(model, feats, T, 1, tables, fuse)
    assert torch.equal(ids, ref_ids), (ids != ref_ids).nonzero()[:8]
    assert torch.equal(lg[:T - 1], ref_lg[:T - 1]), (lg[:T - 1] != ref_lg[:T - 1]).any(-1).any(-1).nonzero().flatten()[:8]
    assert torch.equal(ids[:, :3], PRIMER[0].view(1, 3).expand(3, 3))
    assert len(set(ids[:, 3:].flatten().tolist())) >= 4           # the decisions feed back: a degenerate run would compare nothing


def test_lockstep_v2_generate_has_equal_ids_on_both_streams():
    """Lockstep V2 '2.2' (rotary self- and cross-attention behind folded norms, FOLD 3 / 4), heads of 64, 3 clips, 40 tokens: the
    process-wide switch picks the stream of every attention launch the step makes."""
    T = 40
    cfg = dict(version_name="2.2", n_layers=2, num_heads=8, d_model=512, dim_feedforward=1024, max_sequence_chord=T,
               total_vf_dim=synthetic.total_vf_dim(1))
    m = VideoMusicTransformer_V2(**cfg).eval()
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(shapes, seed=4, recipe="feedback").items()})
    m = m.cuda()
    f = {k: v.cuda() for k, v in feats_t(synthetic.synthetic_features(3, seed=5)).items()}
    pr = [torch.tensor([v]) for v in (1, 1, 0)]
    args = (f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], *pr)
    out = {}
    try:
        for scalar in (0, 1):
            _lib.call("amt_set_option", None, b"scalar_key_stream", scalar)
            with torch.no_grad():
                out[scalar] = m.generate_batch(*args, target_seq_length=T, beam=0, sampler="argmax").cpu()
    finally:
        _lib.call("amt_set_option", None, b"scalar_key_stream", 1)
    assert out[1].shape == (3, T) and torch.equal(out[0], out[1]), (out[0] != out[1]).nonzero()[:8]
    assert len(set(out[1][:, 1:].flatten().tolist())) >= 4
