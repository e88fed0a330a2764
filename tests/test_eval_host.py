"""Evaluation metrics, host side (no GPU): the fp64 restatement of the metrics kernel against the reference's own figures
(g_eval.npz, tools/make_goldens_eval.py), the target reader against the reference's dataset class, `metrics.summarize` and the
evaluation flags."""
import json

import numpy as np
import pytest

from tests import helpers_eval as H
from tests.helpers_features import write_mini_dataset
from video2music_amd import metrics
from video2music_amd.dataset import vevo_features as V
from video2music_amd.utilities import constants as C
from video2music_amd.utilities.argument_eval_funcs import parse_eval_args

RESULTS = ("acc", "h1", "h3", "h5", "cor", "loss_chord", "loss_emotion", "total_loss")


@pytest.fixture(scope="module")
def g(golden):
    return golden("g_eval.npz")


@pytest.fixture(scope="module")
def clips(g, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("vevo_eval"))
    content = {k[3:]: g[k] for k in g if k.startswith("in_")}
    content["ids"] = [str(i) for i in g["ids"]]
    write_mini_dataset(root, content)
    return {fid: V.load_clip(root, fid, motion_type=1, max_seq_video=300, max_seq_chord=300) for fid in content["ids"]}


def test_fixture_content_is_reproducible(g):
    c = H.eval_dataset_content()
    for fid in c["ids"]:
        assert np.array_equal(c[f"{fid}_emotion"], g[f"in_{fid}_emotion"])
        top = c[f"{fid}_emotion"].max(1)
        assert np.abs(top - C.EMOTION_THRESHOLD).min() > 0.01 and 0.2 < (top >= C.EMOTION_THRESHOLD).mean() < 0.45


def test_eval_targets_equal_the_reference_dataset_class(g, clips):
    for fid in ("003", "017"):            # "003": END right after its last chord; "017": cut at 300 s
        t = V.eval_targets(clips[fid], 300)
        assert all(v.shape == (299,) for v in t.values())
        for k in ("tgt", "tgt_root", "tgt_attr"):
            assert np.array_equal(t[k], g[f"ref_{fid}_{k}"]), (fid, k)
        assert np.array_equal(t["emo_prob"], g[f"ref_{fid}_tgt_emotion_prob"])
        assert np.array_equal(H.emotion_rows(t["tgt"], t["emo_class"]), g[f"ref_{fid}_tgt_emotion"])
    t = V.eval_targets(clips["003"], 300)
    assert t["tgt"][38] < C.CHORD_END and t["tgt"][39] == C.CHORD_END and (t["tgt"][40:] == C.CHORD_PAD).all()
    assert (V.eval_targets(clips["017"], 300)["tgt"] < C.CHORD_END).all()


def test_load_clips_stacks_the_targets_and_keeps_its_keys(g, tmp_path):
    content = {k[3:]: g[k] for k in g if k.startswith("in_")}
    content["ids"] = [str(i) for i in g["ids"]]
    write_mini_dataset(str(tmp_path), content)
    f = V.load_clips(str(tmp_path), content["ids"], motion_type=1)
    assert {"semantic", "key", "scene_offset", "motion", "emotion", "chord", "chord_root", "chord_attr"} <= set(f)
    for k in ("tgt", "tgt_root", "tgt_attr", "emo_class", "emo_prob"):
        assert f[k].shape == (2, 299)
    assert np.array_equal(f["tgt"][1], g["ref_017_tgt"]) and np.array_equal(f["chord"][:, 1:], f["tgt"])


def test_restatement_reproduces_every_recorded_reference_figure(g, clips):
    for n, (fid, L) in enumerate(H.CASES):
        t = V.eval_targets(clips[fid], 300)
        y = g[f"case{n}_logits"]
        assert y.shape == (L, C.CHORD_SIZE)
        r = H.restate(y[None], t["tgt"][None, :L], t["emo_class"][None, :L], t["emo_prob"][None, :L], C.EMOTION_THRESHOLD)
        got = metrics.clip_ratios({k: r["clip"][:, i] for i, k in enumerate(metrics.FIELDS)})
        want = dict(zip(RESULTS, g[f"case{n}_results"]))
        for k in ("acc", "h1", "h3", "h5", "cor"):
            assert got[k][0] == want[k], (fid, L, k, got[k][0], want[k])
        for k in ("loss_chord", "loss_emotion", "total_loss"):
            assert abs(got[k][0] - want[k]) <= H.loss_bound(L, want[k]), (fid, L, k, got[k][0], want[k])
    assert want["cor"] == -1.0                          # the L = 5 case counts nothing


def test_restatement_counts_N_as_maj_and_honours_the_threshold():
    y = np.full((1, 4, C.CHORD_SIZE), -1.0, dtype=np.float32)
    y[0, :, 0] = 2.0                                     # every row predicts "N"
    tgt = np.array([[5, 5, 5, C.CHORD_END]])
    emo = np.array([[0, 3, 0, 0]])                       # exciting accepts maj, sad does not
    prob = np.array([[0.9, 0.9, np.nextafter(np.float32(0.8), np.float32(0)), 0.9]], dtype=np.float32)
    r = H.restate(y, tgt, emo, prob, 0.8)
    assert r["counted"].tolist() == [[True, True, False, False]] and r["right"].tolist() == [[True, False, False, False]]
    prob[0, 2] = np.float32(0.8)                         # exactly at the threshold: counted
    assert H.restate(y, tgt, emo, prob, 0.8)["counted"].tolist() == [[True, True, True, False]]


def test_summarize_follows_eval_model():
    rows = np.array([[10, 4, 4, 6, 8, 20.0, 318.0, 4, 1, 10],          # cor 1/4
                     [5, 5, 5, 5, 5, 2.5, 159.0, 0, 0, 20],            # nothing counted: cor -1, left out of avg_cor
                     [8, 2, 2, 4, 4, 16.0, 636.0, 2, 2, 8]])           # cor 1
    per_clip = {k: rows[:, i] for i, k in enumerate(metrics.FIELDS)}
    r = metrics.clip_ratios(per_clip)
    assert r["cor"].tolist() == [0.25, -1.0, 1.0]
    assert r["acc"].tolist() == [float(np.float32(4) / np.float32(10)), 1.0, 0.25]
    assert r["loss_chord"].tolist() == [2.0, 0.5, 2.0]
    assert np.allclose(r["loss_emotion"], [318 / 1590, 159 / 3180, 636 / 1272], rtol=0, atol=1e-15)
    s = metrics.summarize(per_clip)
    assert set(s) == {"avg_total_loss", "avg_loss_chord", "avg_loss_emotion", "avg_acc", "avg_cor", "avg_acc_cor", "avg_h1", "avg_h3", "avg_h5"}
    assert s["avg_cor"] == (0.25 + 1.0) / 2                           # two clips in the denominator, not three
    assert s["avg_acc"] == sum(r["acc"].tolist()) / 3 and s["avg_acc_cor"] == (s["avg_acc"] + s["avg_cor"]) / 2
    assert s["avg_loss_chord"] == 1.5 and s["avg_h5"] == sum(r["h5"].tolist()) / 3
    want_total = sum(C.LOSS_LAMBDA * a + (1 - C.LOSS_LAMBDA) * b for a, b in zip(r["loss_chord"], r["loss_emotion"])) / 3
    assert abs(s["avg_total_loss"] - want_total) < 1e-15
    assert (C.LOSS_LAMBDA, C.EMOTION_THRESHOLD) == (0.4, 0.8)
    empty = metrics.clip_ratios({k: np.array([v]) for k, v in zip(metrics.FIELDS, (0, 0, 0, 0, 0, 0.0, 100.0, 0, 0, 4))})
    assert empty["acc"][0] == 1.0 and empty["cor"][0] == -1.0 and np.isnan(empty["h1"][0])     # a clip of PAD targets only


def test_confusion_counts():
    pred = np.array([0, 1, 14, 27, C.CHORD_END, C.CHORD_PAD, 156])
    root, attr = metrics.pred_root_attr(pred)
    assert root.tolist() == [0, 1, 2, 3, C.CHORD_ROOT_END, C.CHORD_ROOT_PAD, 12]
    assert attr.tolist() == [0, 1, 1, 1, C.CHORD_ATTR_END, C.CHORD_ATTR_PAD, 13]
    m = metrics.confusion_matrix([1, 1, 2, 14, 3], [1, 2, 2, 1, 0], np.arange(1, 13))
    assert m.shape == (12, 12) and m.sum() == 3 and m[0, 0] == 1 and m[0, 1] == 1 and m[1, 1] == 1


def test_separated_heads_are_refused(monkeypatch):
    monkeypatch.setattr(C, "IS_SEPERATED", True)
    with pytest.raises(TypeError, match="IS_SEPERATED heads"):
        metrics.chord_metrics(None, None, None, None)


def test_eval_flag_defaults_equal_the_reference(g):
    want = json.loads(str(g["eval_arg_defaults"]))
    got = vars(parse_eval_args([])[0])
    assert {k: got[k] for k in want} == want
    assert set(got) - set(want) == {"save_conf_matrix", "save_expert_emotion_plot", "output_dir", "test_ids", "synthetic_weights"}
    assert (got["save_conf_matrix"], got["test_ids"], got["synthetic_weights"], got["batch_size"]) == (False, "split:test", False, 1)
    assert parse_eval_args(["-save_conf_matrix"])[0].save_conf_matrix is True
