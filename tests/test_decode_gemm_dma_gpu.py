"""Rows of the skinny decode GEMM staged by LDS-DMA (decode_gemm.hip, `decode_gemm_kernel<.., LEAN = true, DMA = true>`; option
`gemm_rows_dma`) against the register staging they replace (`AMT_GEMM_PRO_REG_ROWS` in `amt_decode_gemm_args.pro`).

The DMA form changes the PATH a row chunk takes into LDS (memory -> LDS, instead of memory -> registers -> ds_write_b128), the wait in
front of the staging barrier and the barrier's spelling; not one arithmetic instruction.  So every comparison is `torch.equal`.  The
3e-5 bound against the fp64 product (data recipe and bound of test_decode_gemm_lean_gpu.py) only guards against both being wrong together.

What can go wrong is a chunk at the wrong LDS or global offset (the row clamp, the two sources' bases, chunks past the immediate's
range), a barrier passed before another wave's chunk has landed, or, behind the folded-FFN prologue, the u half's own ds_write.  Hence:
B in {1, 15, 16, 17, 32} (clamped rows, one and two row blocks), (K1, K) with 2 / 3 / 4 / 6 chunks, 32 and 48 low columns without and
with the high column part, and the folded-FFN prologue at the two shapes the DMA form serves (K1 = 2 (K - K1)) with the u half drawn
from N(0, 1) and from N(3, 5).  Every launch runs on poisoned allocations: outputs and packing scratch inside a backing that is NaN
throughout, with guards in front and behind (the layout of tests/helpers_poison.py); no NaN may be left in an output and no guard
may change.

The operator entry point carries no handle, so the module sets the process-wide `gemm_rows_dma` to 1 for its launches (the library's
default, set all the same: another module may have left 0); which shapes take the DMA form is the launcher's rule, of which the
test only requires the lean front (`amt_decode_gemm_ex_lean`), a precondition."""
import ctypes

import numpy as np
import pytest
import torch

from video2music_amd import _lib, synthetic
from video2music_amd.model.video_music_transformer import VideoMusicTransformer
from tests.helpers import synthetic_sd, feats_t
from tests.helpers_poison import GUARD_BYTES
from tests.test_decode_gemm_pipeline_gpu import CHAIN_CFG

pytestmark = pytest.mark.gpu

REG_ROWS = 0x400        # AMT_GEMM_PRO_REG_ROWS (include/amt_hip.h)
GUARD = GUARD_BYTES // 4


@pytest.fixture(scope="module", autouse=True)
def rows_dma_on():
    assert _lib.CONST["AMT_GEMM_PRO_REG_ROWS"] == REG_ROWS
    _lib.call("amt_set_option", None, b"gemm_rows_dma", 1)


def rnd(rs, *shape, scale=1.0, mean=0.0):
    return torch.from_numpy((rs.standard_normal(shape) * scale + mean).astype(np.float32))


def _ln64(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mu) * rstd * w + b, mu, rstd


class Poisoned:
    """NaN-filled device allocations between two NaN guards."""

    def __init__(self):
        self.backings = []

    def empty(self, *shape):
        n = int(np.prod(shape))
        backing = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
        self.backings.append(backing)
        return backing[GUARD:GUARD + n].view(*shape)

    def guards_hold(self):
        torch.cuda.synchronize()
        return all(bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[-GUARD:]).all()) for b in self.backings)


_DATA = {}


def _data(B, K1, K2, n_low, n_high, pro, u_mean, u_std):
    """Inputs on the device and the fp64 results of one case: built once, left unchanged."""
    key = (B, K1, K2, n_low, n_high, pro, u_mean, u_std)
    if key in _DATA:
        return _DATA[key]
    K = K1 + K2
    rs = np.random.RandomState(1000 * pro + K + B + n_high + 7 * n_low + int(u_mean))
    x, x2 = rnd(rs, B, K1), rnd(rs, B, K2, scale=u_std, mean=u_mean)
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
        resid = x2[:, :n_low].contiguous()
        ref_low = torch.relu(x.double() @ wl.double().t() + bl.double() + resid.double())
    ref_high = rows @ wh.double().t() + bh.double() if n_high else None
    D = {k: (v.cuda().contiguous() if v is not None else None)
         for k, v in dict(x=x, x2=x2, wl=wl, bl=bl, fg=fg, fc=fc, gam=gam, bet=bet, resid=resid, wh=wh, bh=bh).items()}
    _DATA[key] = (D, ref_low, ref_high, max(1.0, float(rows.abs().max())))
    return _DATA[key]


def _both_paths(B, K1, K2, n_low, n_high, pro, u_mean=0.0, u_std=1.0):
    K = K1 + K2
    D, ref_low, ref_high, _ = _data(B, K1, K2, n_low, n_high, pro, u_mean, u_std)
    A = lambda k, on=True: _lib.addr(D[k]) if on and D[k] is not None else None
    got = {}
    for bit in (REG_ROWS, 0):
        ps = Poisoned()
        yl, yh = ps.empty(B, n_low), ps.empty(B, max(n_high, 1))
        sl, sh = ps.empty((n_low + 15) // 16 * 16 * K1), ps.empty(max((n_high + 15) // 16 * 16 * K, 1))
        args = _lib.DecodeGemmArgs(x=A("x"), ldx=K1, x2=A("x2"), ldx2=K2, K1=K1, K=K, w_low=A("wl"), bias_low=A("bl"), resid=A("resid"),
                                   relu=0 if pro else 1, w_high=A("wh"), bias_high=A("bh"), n_low=n_low, n_high=n_high, pro=pro | bit,
                                   fold_g=A("fg", pro), fold_c=A("fc", pro), ln_w=A("gam", pro), ln_b=A("bet", pro), y_low=_lib.addr(yl),
                                   y_high=_lib.addr(yh) if n_high else None, scratch_low=_lib.addr(sl),
                                   scratch_high=_lib.addr(sh) if n_high else None, B=B, eps=1e-5)
        assert _lib.call("amt_decode_gemm_ex_lean", ctypes.byref(args)) == 1, "not a lean-front launch: both runs would stage through registers"
        _lib.call("amt_decode_gemm_ex_fwd", ctypes.byref(args), _lib.stream_ptr())
        assert ps.guards_hold(), ("a guard changed", bit)
        got[bit] = (yl.cpu(), yh.cpu() if n_high else None)
    return got, ref_low, ref_high


def _check(tag, got, ref_low, ref_high, bound=3e-5):
    yl, yh = got[0]
    assert not torch.isnan(yl).any() and not torch.isnan(got[REG_ROWS][0]).any(), tag
    err_low = (yl.double() - ref_low).abs().max().item()
    err_high = 0.0
    assert torch.equal(yl, got[REG_ROWS][0]), tag
    if ref_high is not None:
        assert not torch.isnan(yh).any() and not torch.isnan(got[REG_ROWS][1]).any(), tag
        err_high = (yh.double() - ref_high).abs().max().item()
        assert torch.equal(yh, got[REG_ROWS][1]), tag
    print(tag, "max |dma - fp64| low", err_low, "high", err_high, "bound", bound)
    assert err_low < bound and err_high < bound, tag


ROWS = [1, 15, 16, 17, 32]
PLAIN_K = [(256, 512), (512, 768), (512, 1024), (1024, 1536)]
COLUMNS = [(32, 0), (48, 0), (32, 48)]          # 32 and 48 low columns alone, and the column split
FFN_K = [(1024, 1536), (512, 768)]


@pytest.mark.parametrize("n_low,n_high", COLUMNS)
@pytest.mark.parametrize("K1,K", PLAIN_K)
@pytest.mark.parametrize("B", ROWS)
def test_plain_rows_by_dma_are_bit_equal_to_register_staging(B, K1, K, n_low, n_high):
    """`Pro::Plain` with bias, residual and ReLU on the low columns: every chunk of every row goes by DMA."""
    got, ref_low, ref_high = _both_paths(B, K1, K - K1, n_low, n_high, 0)
    _check((B, K1, K, n_low, n_high), got, ref_low, ref_high)


@pytest.mark.parametrize("u_mean,u_std", [(0.0, 1.0), (3.0, 5.0)])
@pytest.mark.parametrize("K1,K", FFN_K)
@pytest.mark.parametrize("B", ROWS)
def test_folded_ffn_raw_columns_by_dma_are_bit_equal_to_register_staging(B, K1, K, u_mean, u_std):
    """`Pro::FoldedFfn`: the raw columns by DMA, the u half through registers (its statistics: mean 3, deviation 5 in the second
    draw, so neither is the trivial 0 / 1).  The fp64 bound is the lean test's 3e-5 for rows of magnitude <= ~5 scaled by the largest
    staged value otherwise (the error of an fp32 dot product is relative to its terms)."""
    got, ref_low, ref_high = _both_paths(B, K1, K - K1, 32, 48, 1, u_mean, u_std)
    scale = _data(B, K1, K - K1, 32, 48, 1, u_mean, u_std)[3]
    _check((B, K1, K, u_mean, u_std), got, ref_low, ref_high, bound=3e-5 * max(1.0, scale / 5.0))


# the issue's chain (d_model 128: no launch of it reaches the lean front, the option must change nothing and be part of the graph key), and
# a one-layer d_model 512 chain whose G1 / G2 / G3 all take the DMA form (17 clips: a second row block with one row)
CHAINS = [
    (CHAIN_CFG, 40, 3),
    (dict(n_layers=1, num_heads=8, d_model=512, dim_feedforward=1024, max_sequence_chord=24, total_vf_dim=synthetic.total_vf_dim(1), rpr=True), 24, 17),
]
PRIMER = ([1, 66, 122, 7], [1, 6, 10, 1], [0, 0, 5, 3])


@pytest.mark.parametrize("which", range(len(CHAINS)), ids=["d128", "d512"])
def test_decode_chain_ids_and_logits_do_not_depend_on_the_row_staging(which):
    cfg, T, B = CHAINS[which]
    m = VideoMusicTransformer(**cfg).eval()
    m.load_state_dict(synthetic_sd(cfg, 5, recipe="feedback"), strict=False)
    m = m.cuda()
    f = {k: v.cuda() for k, v in feats_t(synthetic.synthetic_features(B, seed=31)).items()}
    inp = (f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], *[torch.tensor(v) for v in PRIMER])
    h = m._ensure_handle()
    ref = {}
    with torch.no_grad():
        for opt in (0, 1):
            _lib.call("amt_set_option", h, b"gemm_rows_dma", opt)
            ids, lg = m.generate_batch(*inp, target_seq_length=T, beam=0, sampler="argmax", return_logits=True)
            ref[opt] = (ids.cpu(), lg.cpu())
        ids, lg = ref[0]
        assert len(set(ids[:, 4:].flatten().tolist())) >= 3           # the decisions feed back: a degenerate run would compare nothing
        assert lg[:T - 1].abs().sum().item() > 0 and not torch.isnan(lg[:T - 1]).any()
        assert torch.equal(ref[1][0], ids), (ref[1][0] != ids).nonzero()[:8]
        assert torch.equal(ref[1][1][:T - 1], lg[:T - 1]), (ref[1][1][:T - 1] != lg[:T - 1]).any(-1).any(-1).nonzero().flatten()[:8]
        # without logits the captured graphs of the two settings differ in nothing but the option: it is part of their key
        for opt in (1, 0, 1):
            _lib.call("amt_set_option", h, b"gemm_rows_dma", opt)
            assert torch.equal(m.generate_batch(*inp, target_seq_length=T, beam=0, sampler="argmax").cpu(), ref[opt][0]), opt
