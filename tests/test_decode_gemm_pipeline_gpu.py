"""The pipelined tile loop of the skinny decode GEMM (decode_gemm.hip, `decode_gemm_kernel<.., PIPE = true>`; handle option
`gemm_tile_pipeline`) against the serial loop it replaces (`AMT_GEMM_PRO_SERIAL_LOOP` in `amt_decode_gemm_args.pro`).

The pipelined loop changes WHEN a k-tile's LDS reads and its folded-FFN fix are issued, not what is computed: one accumulator chain
per wave, tiles and .x .y .z .w in the serial order, the fix with the same operands and nesting.  So every comparison between the two
loops is `torch.equal`; the 3e-5 bound against the fp64 product (that of test_ops_gpu.py's skinny-GEMM test, same data recipe) only
guards against both being wrong together.

The shapes are the smallest that reach each way the loop can go: a wave that owns all KCH tiles of its instantiation walks them
branch-free (raw side, LayerNorm side, or -- the one wave whose range straddles K1 -- both with a select), any other wave takes a
scalar branch per tile, a wave past the last tile none."""
import ctypes

import numpy as np
import pytest
import torch

from video2music_amd import _lib, synthetic
from video2music_amd.model.video_music_transformer import VideoMusicTransformer
from tests.helpers import synthetic_sd, feats_t

pytestmark = pytest.mark.gpu

SERIAL = 0x100          # AMT_GEMM_PRO_SERIAL_LOOP (include/amt_hip.h)


def rnd(rs, *shape, scale=1.0):
    return torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32))


def _ln64(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mu) * rstd * w + b, mu, rstd


# (B, K1, K2, n_low, n_high, pro)
CASES = [
    # one tile per wave with idle waves: K = 96 is 6 tiles, waves 6-15 own none
    (5, 48, 48, 16, 24, 0),
    (5, 32, 64, 16, 24, 1),
    # ragged last wave: K = 416 is 26 tiles, 2 per wave, wave 12 holds the last pair, waves 13-15 own none; second row block and
    # last column tile ragged (K1 = 208: 13 low tiles, one per wave, and the K1 boundary inside wave 6's pair)
    (19, 208, 208, 32, 40, 0),
    (19, 208, 208, 32, 40, 1),
    # K1 boundary inside one wave's tile range (tiles 16 | 17 are wave 8's pair), and exactly between two waves
    (19, 272, 112, 32, 40, 1),
    (19, 256, 128, 32, 40, 1),
    # the same inside the branch-free walk: K = 768 is 3 tiles per wave at KCH = 3, K1 = 400 puts tiles 24 | 25 into wave 8's three
    (3, 400, 368, 16, 40, 1),
    (3, 400, 368, 16, 40, 0),
    # low-column tiles with fewer tiles than the high ones (K1 = K / 2: one tile per wave below the split, two above), and no high part
    (19, 256, 256, 32, 48, 0),
    (19, 256, 256, 32, 48, 1),
    (19, 256, 256, 32, 0, 0),
    (19, 256, 256, 32, 0, 1),
    # the decode chain's own forms (G1 / G2, G3 with the next layer's QKV, G3 with the output head), one launch each
    (32, 512, 512, 512, 512, 0),
    (32, 1024, 512, 512, 1536, 1),
    (32, 1024, 512, 512, 160, 1),
]


@pytest.mark.parametrize("B,K1,K2,n_low,n_high,pro", CASES)
def test_pipelined_tile_loop_is_bit_equal_to_the_serial_one(B, K1, K2, n_low, n_high, pro):
    K = K1 + K2
    rs = np.random.RandomState(1000 * pro + K + B + n_high)
    x, x2 = rnd(rs, B, K1), rnd(rs, B, K2) + (0.7 if pro else 0.0)
    wl, bl = rnd(rs, n_low, K1, scale=K1 ** -0.5), rnd(rs, n_low, scale=0.1)
    wh, bh = (rnd(rs, n_high, K, scale=K ** -0.5), rnd(rs, n_high, scale=0.1)) if n_high else (None, None)
    fg, fc = rnd(rs, K1), rnd(rs, K1, scale=0.3)
    gam, bet = 1 + rnd(rs, K2, scale=0.2), rnd(rs, K2, scale=0.1)
    if pro:
        ln, mu, rstd = _ln64(x2.double(), gam.double(), bet.double())
        a = torch.relu((x.double() - mu * fg.double()) * rstd + fc.double())
        rows = torch.cat([a, ln], 1)
        ref_low = a @ wl.double().t() + bl.double() + ln[:, :n_low]
        resid = None
    else:
        rows = torch.cat([x.double(), x2.double()], 1)
        resid = x2[:, :n_low].contiguous() if K2 >= n_low else None
        ref_low = x.double() @ wl.double().t() + bl.double() + (resid.double() if resid is not None else 0)
    ref_high = rows @ wh.double().t() + bh.double() if n_high else None
    D = {k: v.cuda().contiguous() for k, v in dict(x=x, x2=x2, wl=wl, bl=bl, fg=fg, fc=fc, gam=gam, bet=bet).items()}
    for k, v in dict(resid=resid, wh=wh, bh=bh).items():
        D[k] = v.cuda().contiguous() if v is not None else None
    A = lambda k, on=True: _lib.addr(D[k]) if on and D[k] is not None else None
    sl = torch.empty((n_low + 15) // 16 * 16 * K1, device="cuda")
    sh = torch.empty(max((n_high + 15) // 16 * 16 * K, 1), device="cuda")
    got = {}
    for loop in (SERIAL, 0):
        yl = torch.full((B, n_low), float("nan"), device="cuda")
        yh = torch.full((B, max(n_high, 1)), float("nan"), device="cuda")
        args = _lib.DecodeGemmArgs(x=A("x"), ldx=K1, x2=A("x2"), ldx2=K2, K1=K1, K=K, w_low=A("wl"), bias_low=A("bl"), resid=A("resid"), relu=0,
                                   w_high=A("wh"), bias_high=A("bh"), n_low=n_low, n_high=n_high, pro=pro | loop, fold_g=A("fg", pro),
                                   fold_c=A("fc", pro), ln_w=A("gam", pro), ln_b=A("bet", pro), y_low=_lib.addr(yl),
                                   y_high=_lib.addr(yh) if n_high else None, scratch_low=_lib.addr(sl),
                                   scratch_high=_lib.addr(sh) if n_high else None, B=B, eps=1e-5)
        _lib.call("amt_decode_gemm_ex_fwd", ctypes.byref(args), _lib.stream_ptr())
        got[loop] = (yl.cpu(), yh.cpu())
    tag = (B, K1, K2, n_low, n_high, pro)
    yl, yh = got[0]
    err_low = (yl.double() - ref_low).abs().max().item()
    err_high = (yh.double() - ref_high).abs().max().item() if n_high else 0.0
    print(tag, "max |pipelined - fp64| low", err_low, "high", err_high)
    assert torch.equal(yl, got[SERIAL][0]), tag
    if n_high:
        assert torch.equal(yh, got[SERIAL][1]), tag
    assert err_low < 3e-5, tag
    assert err_high < 3e-5, tag


def test_a_bad_prologue_value_is_refused():
    """The loop bit is the only one `pro` takes besides the prologue's 0 / 1."""
    y = torch.zeros(16, 16, device="cuda")
    args = _lib.DecodeGemmArgs(x=_lib.addr(y), ldx=16, K1=32, K=32, w_low=_lib.addr(y), n_low=16, n_high=0, pro=2, y_low=_lib.addr(y),
                               scratch_low=_lib.addr(y), B=1, eps=1e-5)
    with pytest.raises(RuntimeError):
        _lib.call("amt_decode_gemm_ex_fwd", ctypes.byref(args), _lib.stream_ptr())


CHAIN_CFG = dict(n_layers=2, num_heads=2, d_model=128, dim_feedforward=256, max_sequence_chord=40,
                 total_vf_dim=synthetic.total_vf_dim(1), rpr=True)


def test_decode_chain_ids_and_logits_do_not_depend_on_the_tile_loop():
    """A small folded-chain model (2 layers, d_model 128, 2 heads, dff 256), 3 clips, T = 40, a primer of 4: `generate_batch` under
    `gemm_tile_pipeline` 1, then 0, then 1 again on the same handle gives the same ids and the same logits at every step.  Without
    logits the captured graphs of the two settings differ in nothing but the option, which is therefore part of their key."""
    m = VideoMusicTransformer(**CHAIN_CFG).eval()
    m.load_state_dict(synthetic_sd(CHAIN_CFG, 5, recipe="feedback"), strict=False)
    m = m.cuda()
    f = {k: v.cuda() for k, v in feats_t(synthetic.synthetic_features(3, seed=31)).items()}
    pr = [torch.tensor(v) for v in ([1, 66, 122, 7], [1, 6, 10, 1], [0, 0, 5, 3])]
    T = 40
    h = m._ensure_handle()
    runs = []
    with torch.no_grad():
        for opt in (1, 0, 1):
            _lib.call("amt_set_option", h, b"gemm_tile_pipeline", opt)
            ids, lg = m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], *pr, target_seq_length=T,
                                       beam=0, sampler="argmax", return_logits=True)
            ids2 = m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], *pr, target_seq_length=T,
                                    beam=0, sampler="argmax")
            runs.append((ids.cpu(), lg.cpu(), ids2.cpu()))
    _lib.call("amt_set_option", h, b"gemm_tile_pipeline", 1)
    ids, lg, _ = runs[0]
    assert len(set(ids[:, 4:].flatten().tolist())) >= 3           # the decisions feed back: a degenerate run would compare nothing
    assert lg[:T - 1].abs().sum().item() > 0
    for o_ids, o_lg, o_ids2 in runs:
        assert torch.equal(o_ids, ids), (o_ids != ids).nonzero()[:8]
        assert torch.equal(o_lg[:T - 1], lg[:T - 1]), (o_lg[:T - 1] != lg[:T - 1]).any(-1).any(-1).nonzero().flatten()[:8]
        assert torch.equal(o_ids2, ids)
