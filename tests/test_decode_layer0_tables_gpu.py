"""Layer 0's self-attention keys from the shared input tables (attn_decode.hip, the TAB instantiation of attn_decode_sample_kernel;
handle option `layer0_kv_from_tables`).

Inside a captured graph of more than one K/V batch per step, the attention that carries the sampling head re-sums the keys / values
of positions 0 .. t-1 from the head-sliced position table (shared by every clip) and the clip's ids, instead of streaming the rows
the same sum was stored into.  One function (table_sum4, sample_device.h) spells the sum at every site, the wave -> key mapping, the
consumption order and both merges are unchanged: every comparison between the two settings is `torch.equal`.  A tolerance here would
hide a changed summation."""
import ctypes as C

import pytest
import torch

from video2music_amd import _lib, synthetic
from video2music_amd.model.video_music_transformer import VideoMusicTransformer
from tests.helpers import CFG2, synthetic_sd, feats_t

pytestmark = pytest.mark.gpu

T_CAP = 320
CFG = dict(CFG2, max_sequence_chord=T_CAP)          # config-2 width: 6 layers, 8 heads of 64, d_model 512
PRIMER = torch.tensor([[1, 1, 0], [66, 6, 0], [122, 10, 5]]).t()      # (tokens, roots, attrs) of a three-chord primer
KEYS = (0.0, 7.0, 3.0, 11.0, 5.0)                   # one key value per clip, all different
CHUNKS = [(-1,), (1,), (3,), (16,), (100,), (1, 3, 16, 100)]


def sp():
    return _lib.stream_ptr()


def build(cfg, seed):
    m = VideoMusicTransformer(**cfg).eval()
    m.load_state_dict(synthetic_sd(cfg, seed, recipe="feedback"), strict=False)
    return m.cuda()


def features(B, seed=77):
    f = {k: v.cuda() for k, v in feats_t(synthetic.synthetic_features(B, seed=seed)).items()}
    f["key"] = torch.tensor(KEYS[:B], device="cuda")
    return f


def run_generate(m, f, T, chunks=(-1,), tables=1, fuse=1, total_steps=None):
    """Feedback-greedy generate of B clips driven like `generate_batch` (the driver of tests/test_decode_short_context_gpu.py):
    `amt_generate_run` fed `chunks` steps per call (cycled) until `total_steps` (default T - 1) are asked for.  The self-attention
    K/V cache starts from zeros and is read back whole.  Returns (tokens (B,T), logits (T,B,159), K/V cache)."""
    sem, key, scene, motion, emotion, B, S = m._prep_features(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
    h = m._ensure_handle(sem.shape[2])
    _lib.call("amt_set_option", h, b"layer0_kv_from_tables", tables)
    _lib.call("amt_set_option", h, b"fuse_sampling_head", fuse)
    try:
        pr = [p.cuda().long().contiguous() for p in PRIMER]
        lg = torch.zeros(T, B, 159, device="cuda")
        out = torch.empty(B, T, device="cuda", dtype=torch.long)
        with torch.no_grad():
            m._encode(h, sem, scene, motion, emotion, slice(0, B))
            dims = (C.c_int64 * 6)()
            _lib.call("amt_kv_cache_io", h, None, 0, 0, dims, sp())
            kv = torch.zeros(tuple(dims), device="cuda")
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
            _lib.call("amt_kv_cache_io", h, _lib.ptr(kv), kv.numel(), 0, None, sp())
        torch.cuda.synchronize()
    finally:
        _lib.call("amt_set_option", h, b"layer0_kv_from_tables", 1)
        _lib.call("amt_set_option", h, b"fuse_sampling_head", 1)
    return out.cpu(), lg.cpu(), kv.cpu()


def assert_same(got, ref, T):
    ids, lg, kv = got
    ref_ids, ref_lg, ref_kv = ref
    assert torch.equal(ids, ref_ids), (ids != ref_ids).nonzero()[:8]
    assert torch.equal(lg[:T - 1], ref_lg[:T - 1]), (lg[:T - 1] != ref_lg[:T - 1]).any(-1).any(-1).nonzero().flatten()[:8]
    assert torch.equal(kv, ref_kv), (kv != ref_kv).nonzero()[:8]


@pytest.fixture(scope="module")
def model():
    return build(CFG, 11)


@pytest.mark.parametrize("chunks", CHUNKS)
def test_tables_equal_the_cache_at_every_key_count(model, chunks):
    """B = 3 clips of different keys, T = 320: graphs of 16 / 8 / 4 / 2 / 1 steps start at every offset and both parities, so the
    table-sourced kernel runs at every key count from one batch + 1 to 319 (129, 255, 256, 257, a ragged tail).  Ids, logits at
    every position and the whole K/V cache equal those of option 0."""
    T, f = T_CAP, features(3)
    ref = run_generate(model, f, T, chunks, tables=0)
    got = run_generate(model, f, T, chunks, tables=1)
    assert_same(got, ref, T)
    ids = got[0]
    assert torch.equal(ids[:, :3], PRIMER[0].view(1, 3).expand(3, 3))
    assert len(set(ids[:, 3:].flatten().tolist())) >= 4           # the decisions feed back: a degenerate run would compare nothing
    assert (got[2][:, 0, :3, :, 3:T - 1] != 0).any()              # layer 0's rows are still written


@pytest.mark.parametrize("hd,H,d,dff", [(32, 4, 128, 256), (128, 4, 512, 1024)])
def test_other_head_widths(hd, H, d, dff):
    """256 keys per batch at hd = 32, 64 at hd = 128; two layers, B = 2, T = 2 batches + 45.  Both widths take the table-sourced kernel
    (amt_attn_decode_tables_fit holds for every head width at these lengths), there is no fall-back to assert."""
    stride = 8 * (64 // (hd // 4)) * 4
    T = 2 * stride + 45
    cfg = dict(CFG2, n_layers=2, num_heads=H, d_model=d, dim_feedforward=dff, max_sequence_chord=T)
    m, f = build(cfg, 3), features(2)
    ref = run_generate(m, f, T, (16,), tables=0)
    got = run_generate(m, f, T, (16,), tables=1)
    assert_same(got, ref, T)


def test_five_clips(model):
    """B = 5 (no multiple of anything), T = 200, 16 steps per call."""
    T, f = 200, features(5)
    ref = run_generate(model, f, T, (16,), tables=0)
    got = run_generate(model, f, T, (16,), tables=1)
    assert_same(got, ref, T)


def test_more_steps_asked_than_remain(model):
    """4 calls of 100 steps ask for 400 at T = 320 (the last one with 19 remaining): equal to option 0, and the last position holds a
    decided chord."""
    T, f = T_CAP, features(3)
    ref = run_generate(model, f, T, (100,), tables=0, total_steps=400)
    got = run_generate(model, f, T, (100,), tables=1, total_steps=400)
    assert_same(got, ref, T)
    ids = got[0]
    assert (ids[:, T - 1] >= 0).all() and (ids[:, T - 1] < 157).all(), ids[:, T - 1]


def test_weight_reload_rebuilds_the_head_slices():
    """Another state dict into the same handle, option on: the head-sliced tables follow the reload (ids and logits equal option 0's,
    which reads the cache rows written from the reloaded tables) and the graphs captured before it keep working."""
    T, f = T_CAP, features(3)
    m = build(CFG, 11)
    before = run_generate(m, f, T, (16,), tables=1)
    m.load_state_dict(synthetic_sd(CFG, 5, recipe="feedback"), strict=False)
    got = run_generate(m, f, T, (16,), tables=1)
    ref = run_generate(m, f, T, (16,), tables=0)
    assert_same(got, ref, T)
    assert not torch.equal(got[1][:T - 1], before[1][:T - 1])


def test_option_is_inert_without_the_fused_head(model):
    """fuse_sampling_head 0: no attention launch carries the head, both settings capture and give equal results."""
    T, f = T_CAP, features(3)
    ref = run_generate(model, f, T, (16,), tables=0, fuse=0)
    got = run_generate(model, f, T, (16,), tables=1, fuse=0)
    assert_same(got, ref, T)
