"""The lean front of the skinny decode GEMM (decode_gemm.hip, `decode_gemm_kernel<.., LEAN = true>`; handle option
`gemm_scalar_front`) against the generic front it replaces (`AMT_GEMM_PRO_GENERIC_FRONT` in `amt_decode_gemm_args.pro`).

The lean front changes WHERE the addresses of the row, prologue-vector and weight-tile loads are computed (on the scalar unit, from a
block of kernel arguments the launcher works out), not what is loaded or summed.  So every comparison between the two fronts is
`torch.equal`; the 3e-5 bound against the fp64 product (data recipe and bound of test_decode_gemm_pipeline_gpu.py) only guards
against both being wrong together.

Which front a launch takes is the launcher's rule (`amt_decode_gemm_lean_ok`, asked through `amt_decode_gemm_ex_lean`); the test
does not restate it, it only requires that the shapes built to reach the lean front's addresses are accepted."""
import ctypes

import numpy as np
import pytest
import torch

from video2music_amd import _lib, synthetic
from video2music_amd.model.video_music_transformer import VideoMusicTransformer
from tests.helpers import synthetic_sd, feats_t

pytestmark = pytest.mark.gpu

SERIAL = 0x100          # AMT_GEMM_PRO_SERIAL_LOOP (include/amt_hip.h)
GENERIC = 0x200         # AMT_GEMM_PRO_GENERIC_FRONT


def rnd(rs, *shape, scale=1.0):
    return torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32))


def _ln64(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mu) * rstd * w + b, mu, rstd


# (B, K1, K2, n_low, n_high): the smallest shapes where an address of the lean front can go wrong; each runs with pro 0 and 1
ACCEPTED = [
    # row clamp: rows past B - 1 repeat row B - 1; fifteen rows in a sixteen-row block; one full block; one row in the second; two full
    (1, 256, 256, 32, 48),
    (15, 256, 256, 32, 48),
    (16, 256, 256, 32, 48),
    (17, 256, 256, 32, 48),
    (32, 256, 256, 32, 48),
    # one chunk per source; low tiles with half the k-tiles of the high ones
    (19, 256, 256, 32, 48),
    # three chunks; tile clamp on the low tiles: 16 k-tiles, one per wave, none idle
    (19, 256, 512, 32, 48),
    # no high column part
    (19, 256, 256, 32, 0),
    # six chunks (two behind the immediate offset's range); the high weight's base past one low tile
    (19, 1024, 512, 16, 16),
    # low tiles at K1 = 512 give waves 8-15 no tile: clamped tile index
    (3, 512, 256, 16, 32),
    # the decode chain's own forms: G1 / G2, G3 with the next layer's QKV, G3 with the output head
    (32, 512, 512, 512, 512),
    (32, 1024, 512, 512, 1536),
    (32, 1024, 512, 512, 160),
]
# launches the rule must refuse: (B, K1, K2, n_low, n_high, pro, extra bits of pro); K2 == 0 stands for a null x2
REFUSED = [
    (19, 208, 208, 32, 40, 0, 0),          # K1 is no multiple of 256
    (19, 208, 208, 32, 40, 1, 0),
    (19, 512, 0, 32, 0, 0, 0),             # single-source rows (the folded prologue needs the second source)
    (19, 256, 256, 32, 48, 0, SERIAL),     # the serial tile loop keeps the generic front
    (19, 256, 256, 32, 48, 1, SERIAL),
]


def _both_fronts(B, K1, K2, n_low, n_high, pro, bits=0):
    """Runs one launch with and without the generic-front bit.  Returns {0: (y_low, y_high), GENERIC: ...}, whether the launcher takes
    the lean front without the bit (and never with it), and the fp64 results."""
    K = K1 + K2
    two = K2 > 0
    rs = np.random.RandomState(1000 * pro + K + B + n_high)
    x, x2 = rnd(rs, B, K1), (rnd(rs, B, K2) + (0.7 if pro else 0.0)) if two else None
    wl, bl = rnd(rs, n_low, K1, scale=K1 ** -0.5), rnd(rs, n_low, scale=0.1)
    wh, bh = (rnd(rs, n_high, K, scale=K ** -0.5), rnd(rs, n_high, scale=0.1)) if n_high else (None, None)
    fg, fc = rnd(rs, K1), rnd(rs, K1, scale=0.3)
    gam, bet = (1 + rnd(rs, K2, scale=0.2), rnd(rs, K2, scale=0.1)) if two else (None, None)
    if pro:
        ln, mu, rstd = _ln64(x2.double(), gam.double(), bet.double())
        a = torch.relu((x.double() - mu * fg.double()) * rstd + fc.double())
        rows = torch.cat([a, ln], 1)
        ref_low = a @ wl.double().t() + bl.double() + ln[:, :n_low]
        resid = None
    else:
        rows = torch.cat([x.double(), x2.double()], 1) if two else x.double()
        resid = x2[:, :n_low].contiguous() if two and K2 >= n_low else None
        ref_low = x.double() @ wl.double().t() + bl.double() + (resid.double() if resid is not None else 0)
    ref_high = rows @ wh.double().t() + bh.double() if n_high else None
    D = {k: (v.cuda().contiguous() if v is not None else None)
         for k, v in dict(x=x, x2=x2, wl=wl, bl=bl, fg=fg, fc=fc, gam=gam, bet=bet, resid=resid, wh=wh, bh=bh).items()}
    A = lambda k, on=True: _lib.addr(D[k]) if on and D[k] is not None else None
    sl = torch.empty((n_low + 15) // 16 * 16 * K1, device="cuda")
    sh = torch.empty(max((n_high + 15) // 16 * 16 * K, 1), device="cuda")
    got, lean = {}, {}
    for front in (GENERIC, 0):
        yl = torch.full((B, n_low), float("nan"), device="cuda")
        yh = torch.full((B, max(n_high, 1)), float("nan"), device="cuda")
        args = _lib.DecodeGemmArgs(x=A("x"), ldx=K1, x2=A("x2"), ldx2=K2, K1=K1, K=K, w_low=A("wl"), bias_low=A("bl"), resid=A("resid"), relu=0,
                                   w_high=A("wh"), bias_high=A("bh"), n_low=n_low, n_high=n_high, pro=pro | bits | front, fold_g=A("fg", pro),
                                   fold_c=A("fc", pro), ln_w=A("gam", pro), ln_b=A("bet", pro), y_low=_lib.addr(yl),
                                   y_high=_lib.addr(yh) if n_high else None, scratch_low=_lib.addr(sl),
                                   scratch_high=_lib.addr(sh) if n_high else None, B=B, eps=1e-5)
        lean[front] = _lib.call("amt_decode_gemm_ex_lean", ctypes.byref(args))
        _lib.call("amt_decode_gemm_ex_fwd", ctypes.byref(args), _lib.stream_ptr())
        got[front] = (yl.cpu(), yh.cpu())
    assert lean[GENERIC] == 0                        # the bit always keeps the generic front
    return got, lean[0], ref_low, ref_high


def _check(tag, got, ref_low, ref_high):
    yl, yh = got[0]
    err_low = (yl.double() - ref_low).abs().max().item()
    err_high = (yh.double() - ref_high).abs().max().item() if ref_high is not None else 0.0
    print(tag, "max |lean - fp64| low", err_low, "high", err_high)
    assert torch.equal(yl, got[GENERIC][0]), tag
    if ref_high is not None:
        assert torch.equal(yh, got[GENERIC][1]), tag
    assert err_low < 3e-5, tag
    assert err_high < 3e-5, tag


@pytest.mark.parametrize("pro", [0, 1])
@pytest.mark.parametrize("B,K1,K2,n_low,n_high", ACCEPTED)
def test_lean_front_is_bit_equal_to_the_generic_one(B, K1, K2, n_low, n_high, pro):
    got, lean, ref_low, ref_high = _both_fronts(B, K1, K2, n_low, n_high, pro)
    assert lean == 1, "the launcher keeps this shape on the generic front: the comparison would be of the generic front with itself"
    _check((B, K1, K2, n_low, n_high, pro), got, ref_low, ref_high)


@pytest.mark.parametrize("B,K1,K2,n_low,n_high,pro,bits", REFUSED)
def test_refused_launches_keep_the_generic_front(B, K1, K2, n_low, n_high, pro, bits):
    """A launch outside the rule goes through the same call and gives the generic result (trivially: it is the generic kernel)."""
    got, lean, ref_low, ref_high = _both_fronts(B, K1, K2, n_low, n_high, pro, bits)
    assert lean == 0
    _check((B, K1, K2, n_low, n_high, pro, bits), got, ref_low, ref_high)


def test_the_front_bit_is_not_a_prologue():
    """`pro` still takes 0 or 1 besides its two loop / front bits."""
    y = torch.zeros(16, 16, device="cuda")
    args = _lib.DecodeGemmArgs(x=_lib.addr(y), ldx=16, K1=32, K=32, w_low=_lib.addr(y), n_low=16, n_high=0, pro=2 | GENERIC, y_low=_lib.addr(y),
                               scratch_low=_lib.addr(y), B=1, eps=1e-5)
    assert _lib.call("amt_decode_gemm_ex_lean", ctypes.byref(args)) < 0
    with pytest.raises(RuntimeError):
        _lib.call("amt_decode_gemm_ex_fwd", ctypes.byref(args), _lib.stream_ptr())


# d_model 128: K1 = 128, every skinny GEMM of the step keeps the generic front whatever the option says (3 clips: one row block);
# d_model 512: the folded chain's own launches, all on the lean front (17 clips: a second row block with one row)
CHAINS = [
    (dict(n_layers=2, num_heads=2, d_model=128, dim_feedforward=256, max_sequence_chord=40, total_vf_dim=synthetic.total_vf_dim(1), rpr=True), 40, 3),
    (dict(n_layers=1, num_heads=8, d_model=512, dim_feedforward=1024, max_sequence_chord=24, total_vf_dim=synthetic.total_vf_dim(1), rpr=True), 24, 17),
]
PRIMER = ([1, 66, 122, 7], [1, 6, 10, 1], [0, 0, 5, 3])


def _model(cfg, B):
    m = VideoMusicTransformer(**cfg).eval()
    m.load_state_dict(synthetic_sd(cfg, 5, recipe="feedback"), strict=False)
    m = m.cuda()
    f = {k: v.cuda() for k, v in feats_t(synthetic.synthetic_features(B, seed=31)).items()}
    return m, (f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], *[torch.tensor(v) for v in PRIMER])


@pytest.fixture(scope="module", params=range(len(CHAINS)), ids=["d128", "d512"])
def chain(request):
    """(model, inputs, T, {option value: (ids, per-step logits)}): one generate with logits per setting, shared by the two tests below."""
    cfg, T, B = CHAINS[request.param]
    m, inp = _model(cfg, B)
    h = m._ensure_handle()
    ref = {}
    with torch.no_grad():
        for opt in (0, 1):
            _lib.call("amt_set_option", h, b"gemm_scalar_front", opt)
            ids, lg = m.generate_batch(*inp, target_seq_length=T, beam=0, sampler="argmax", return_logits=True)
            ref[opt] = (ids.cpu(), lg.cpu())
    _lib.call("amt_set_option", h, b"gemm_scalar_front", 1)
    return m, inp, T, ref


def test_decode_chain_ids_and_logits_do_not_depend_on_the_front(chain):
    m, inp, T, ref = chain
    ids, lg = ref[0]
    assert len(set(ids[:, 4:].flatten().tolist())) >= 3           # the decisions feed back: a degenerate run would compare nothing
    assert lg[:T - 1].abs().sum().item() > 0
    assert torch.equal(ref[1][0], ids), (ref[1][0] != ids).nonzero()[:8]
    assert torch.equal(ref[1][1][:T - 1], lg[:T - 1]), (ref[1][1][:T - 1] != lg[:T - 1]).any(-1).any(-1).nonzero().flatten()[:8]


def test_the_front_is_part_of_the_graph_key(chain):
    """Without logits the captured graphs of the two settings differ in nothing but the option: toggled on one handle, every generate
    gives its own setting's ids."""
    m, inp, T, ref = chain
    h = m._ensure_handle()
    with torch.no_grad():
        for opt in (1, 0, 1, 0):
            _lib.call("amt_set_option", h, b"gemm_scalar_front", opt)
            ids = m.generate_batch(*inp, target_seq_length=T, beam=0, sampler="argmax")
            assert torch.equal(ids.cpu(), ref[opt][0]), opt
    _lib.call("amt_set_option", h, b"gemm_scalar_front", 1)
