"""amt_chord_metrics_fwd (csrc/metrics.hip) against the fp64 restatement of tests/helpers_eval.py and, on the golden logits,
against the figures the reference's own metric functions returned (g_eval.npz)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import helpers_eval as H
from video2music_amd import _lib, metrics
from video2music_amd.utilities import constants as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THR = 0.8
N_FIELDS = len(H.FIELDS)
I = {k: i for i, k in enumerate(H.FIELDS)}
COUNTS = [i for k, i in I.items() if k not in ("ce_sum", "bce_sum")]


def call(y, tgt, emo, prob, thr=THR, rows=True, ld=None, B=None, L=None):
    """y: (B, L, ld) fp32 device tensor (columns >= 159 are padding).  -> clip (B, 10), pred, rank, ce as numpy."""
    Bv, Lv = tgt.shape
    B, L, ld = Bv if B is None else B, Lv if L is None else L, y.shape[2] if ld is None else ld
    t = torch.as_tensor(tgt, dtype=torch.long, device=DEV).contiguous()
    e = torch.as_tensor(emo, dtype=torch.int32, device=DEV).contiguous()
    p = torch.as_tensor(prob, dtype=torch.float32, device=DEV).contiguous()
    clip = torch.full((Bv, N_FIELDS), -7.0, device=DEV)
    pred = torch.full((Bv, Lv), -7, dtype=torch.int32, device=DEV) if rows else None
    rank = torch.full((Bv, Lv), -7, dtype=torch.int32, device=DEV) if rows else None
    ce = torch.full((Bv, Lv), -7.0, device=DEV) if rows else None
    _lib.call("amt_chord_metrics_fwd", _lib.ptr(y), ld, _lib.ptr(t), _lib.ptr(e), _lib.ptr(p), ctypes.c_float(thr), B, L,
              _lib.ptr(clip), _lib.ptr(pred), _lib.ptr(rank), _lib.ptr(ce), _lib.stream_ptr())
    torch.cuda.synchronize()
    return clip, pred, rank, ce


def make_case(B, L, seed):
    """Logits 3 * N(0,1) with a third of the targets boosted into the top; targets over the whole vocabulary with id 0, 156, END and
    PAD planted; clip 1 (when there is one) all PAD, clip 2 with nothing counted; one probability exactly at the threshold."""
    rng = np.random.default_rng(seed)
    y = (3 * rng.standard_normal((B, L, C.CHORD_SIZE))).astype(np.float32)
    tgt = rng.integers(0, C.CHORD_END, size=(B, L))
    for pos, v in enumerate((0, 156, C.CHORD_END, C.CHORD_PAD)):
        if L > pos + 1:
            tgt[0, L - 1 - pos] = v
    boost = rng.random((B, L)) < 0.4
    np.put_along_axis(y, tgt[..., None], np.take_along_axis(y, tgt[..., None], -1) + np.where(boost, 7, 0)[..., None].astype(np.float32), -1)
    y[:, ::7, 0] += np.float32(9)                        # "N" predicted now and then: the one-part chord of the correspondence
    if L >= 5:                                           # clip 0 has a sure hit (row 0) and a sure miss (its last row, target "N")
        y[0, 0, tgt[0, 0]], y[0, L - 1, 0] = 30.0, -30.0
    emo = rng.integers(0, 6, size=(B, L))
    prob = np.where(rng.random((B, L)) < 0.5, 0.9, 0.5).astype(np.float32)
    prob[0, 0] = np.float32(THR)                          # exactly at the threshold: counted
    emo[0, 0] = 0
    if B > 1:
        tgt[1] = C.CHORD_PAD
    if B > 2:
        emo[2, ::2], prob[2, 1::2] = 5, 0.79
    return y, tgt, emo, prob


def check(clip, pred, rank, ce, want, L):
    got = clip.cpu().numpy().astype(np.float64)
    assert np.array_equal(got[:, COUNTS], want["clip"][:, COUNTS]), (got, want["clip"])
    for k in ("ce_sum", "bce_sum"):
        err, bound = np.abs(got[:, I[k]] - want["clip"][:, I[k]]), H.loss_bound(L, want["clip"][:, I[k]])
        print(k, "L", L, "max error / bound", float((err / bound).max()))
        assert (err <= bound).all(), (k, got[:, I[k]], want["clip"][:, I[k]])
    if pred is not None:
        assert np.array_equal(pred.cpu().numpy(), want["pred"]) and np.array_equal(rank.cpu().numpy(), want["rank"])
        err = np.abs(ce.cpu().numpy().astype(np.float64) - want["ce"])
        assert (err <= H.loss_bound(L, want["ce"])).all(), float(err.max())


@pytest.mark.parametrize("ld", [159, 160])
@pytest.mark.parametrize("L", [1, 5, 63, 64, 65, 299])
@pytest.mark.parametrize("B", [1, 3])
def test_kernel_equals_fp64_restatement(B, L, ld):
    y, tgt, emo, prob = make_case(B, L, seed=1000 * B + 10 * L + ld)
    want = H.restate(y, tgt, emo, prob, THR)
    if L >= 5:
        assert want["clip"][0, I["n_counted"]] > 0 and want["counted"][0, 0]
        assert 0 < want["clip"][0, I["n_hit5"]] < want["clip"][0, I["n_valid"]]
    if B == 3:
        assert want["clip"][1, I["n_valid"]] == 0 and want["clip"][2, I["n_counted"]] == 0
    yp = torch.full((B, L, ld), 1.0e4, device=DEV)       # a padding column read as a class would win every arg-max
    yp[:, :, :C.CHORD_SIZE] = torch.from_numpy(y).to(DEV)
    check(*call(yp, tgt, emo, prob), want, L)


def test_more_rows_than_one_ordered_pass_holds():
    """L = 1030: the per-row sums of a clip wait in LDS 1024 rows at a time."""
    y, tgt, emo, prob = make_case(2, 1030, seed=5)
    check(*call(torch.from_numpy(y).to(DEV), tgt, emo, prob), H.restate(y, tgt, emo, prob, THR), 1030)


def test_equal_maxima_take_the_lowest_index():
    y = np.zeros((1, 6, C.CHORD_SIZE), dtype=np.float32)
    y[0, 0, [3, 70, 140]] = 5.0                  # one maximum per lane group
    y[0, 1, [64, 128]] = 2.0
    y[0, 2, [157, 158]] = 1.0
    y[0, 3, :] = -3.0                            # all equal: pred 0
    y[0, 4, [10, 11]] = 4.0                      # the target ties with an earlier and a later class
    y[0, 4, 12] = 4.0
    y[0, 5, 158] = 9.0
    tgt = np.array([[70, 128, 158, 100, 11, 5]])
    emo, prob = np.zeros((1, 6), dtype=np.int64), np.full((1, 6), 0.9, dtype=np.float32)
    want = H.restate(y, tgt, emo, prob, THR)
    assert want["pred"].tolist() == [[3, 64, 157, 0, 10, 158]] and want["rank"].tolist() == [[1, 1, 1, 100, 1, 6]]
    clip, pred, rank, ce = call(torch.from_numpy(y).to(DEV), tgt, emo, prob)
    assert pred.cpu().tolist() == want["pred"].tolist() and rank.cpu().tolist() == want["rank"].tolist()
    check(clip, pred, rank, ce, want, 6)


def test_calls_are_deterministic_and_optional_outputs_do_not_change_the_sums():
    y, tgt, emo, prob = make_case(3, 299, seed=9)
    yd = torch.from_numpy(y).to(DEV)
    a, b, c = call(yd, tgt, emo, prob), call(yd, tgt, emo, prob), call(yd, tgt, emo, prob, rows=False)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert c[1] is None and torch.equal(a[0], c[0])


def test_golden_logits_reproduce_the_reference_figures(golden, tmp_path):
    from tests.helpers_features import write_mini_dataset
    from video2music_amd.dataset import vevo_features as V
    g = golden("g_eval.npz")
    content = {k[3:]: g[k] for k in g if k.startswith("in_")}
    content["ids"] = [str(i) for i in g["ids"]]
    write_mini_dataset(str(tmp_path), content)
    f = V.load_clips(str(tmp_path), content["ids"], motion_type=1)
    names = ("acc", "h1", "h3", "h5", "cor", "loss_chord", "loss_emotion", "total_loss")
    for n, (fid, L) in enumerate(H.CASES):
        b = content["ids"].index(fid)
        m = metrics.chord_metrics(torch.from_numpy(g[f"case{n}_logits"]).to(DEV)[None], f["tgt"][b:b + 1, :L], f["emo_class"][b:b + 1, :L],
                                  f["emo_prob"][b:b + 1, :L])
        got, want = metrics.clip_ratios(m), dict(zip(names, g[f"case{n}_results"]))
        for k in names[:5]:
            assert got[k][0] == want[k], (fid, L, k, got[k][0], want[k])
        for k in names[5:]:
            assert abs(got[k][0] - want[k]) <= 2 * H.loss_bound(L, want[k]), (fid, L, k, got[k][0], want[k])   # two fp32 computations
    assert want["cor"] == -1.0


def test_wrapper_takes_strided_rows_and_returns_rows():
    y, tgt, emo, prob = make_case(2, 37, seed=3)
    wide = torch.zeros(2, 37, 192, device=DEV)
    wide[:, :, :C.CHORD_SIZE] = torch.from_numpy(y).to(DEV)
    m = metrics.chord_metrics(wide[:, :, :C.CHORD_SIZE], tgt, emo, prob, return_rows=True)
    want = H.restate(y, tgt, emo, prob, THR)
    clip = torch.stack([m[k] for k in metrics.FIELDS], dim=1)
    check(clip, m["pred"], m["rank"], m["ce"], want, 37)


def test_bad_arguments_raise():
    y, tgt, emo, prob = make_case(1, 5, seed=1)
    yd = torch.from_numpy(y).to(DEV)
    with pytest.raises(_lib.AmtError, match="row stride"):
        call(yd, tgt, emo, prob, ld=158)
    with pytest.raises(_lib.AmtError, match="positive"):
        call(yd, tgt, emo, prob, B=0)
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_chord_metrics_fwd", _lib.ptr(yd), 159, None, None, None, ctypes.c_float(THR), 1, 5, None, None, None, None,
                  _lib.stream_ptr())
