"""Regression evaluation, host side (no GPU): the target reader against the reference's dataset class, the fp64 restatement of the
metrics kernel against the reference's own figures (g_reg_eval.npz, tools/make_goldens_reg_eval.py), `metrics.summarize_regression`,
the evaluation flags, and the condition check of the kernel tests' bounds."""
import json

import numpy as np
import pytest
import torch

from tests import helpers_reg_eval as H
from video2music_amd import metrics
from video2music_amd.dataset import vevo_features as V
from video2music_amd.utilities import constants as C
from video2music_amd.utilities.argument_reg_funcs import parse_eval_args


@pytest.fixture(scope="module")
def g(golden):
    return golden("g_reg_eval.npz")


@pytest.fixture(scope="module")
def root(g, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("vevo_reg_eval"))
    H.write_reg_dataset(path, H.content_of(g))
    return path


def test_fixture_content_is_reproducible(g):
    c = H.reg_dataset_content()
    for fid, n in (("003", 40), ("017", 320)):
        for k in ("note_density", "loudness", "instrument", "semantic", "emotion"):
            assert np.array_equal(c[f"{fid}_{k}"], g[f"in_{fid}_{k}"]), (fid, k)
        assert c[f"{fid}_instrument"].shape == (n, 40) and 0.15 < c[f"{fid}_instrument"].mean() < 0.35
        assert c[f"{fid}_note_density"].max() > 4 and c[f"{fid}_loudness"].max() > 2
    assert float(g["classifier_scale"]) == 1.0


@pytest.mark.parametrize("Tc,Sv", H.LENGTHS)
def test_reader_equals_the_reference_dataset_class(g, root, Tc, Sv):
    for fid, n in (("003", 40), ("017", 320)):
        t = V.read_regression_targets(root, fid, max_seq_video=Sv, max_seq_chord=Tc)
        assert set(t) == {"note_density", "loudness", "instrument"}
        for k, v in t.items():
            want = g[f"ref_{fid}_{k}_{Tc}_{Sv}"]
            assert v.dtype == np.float32 and v.shape == want.shape == ((Sv, 40) if k == "instrument" else (Sv,))
            assert np.array_equal(v, want), (fid, k)
        filled = min(n, Tc)                   # both the text streams and the csv rows stop at max_seq_chord; the rest is PAD
        assert (t["note_density"][:filled] != 0).all() and (t["note_density"][filled:] == C.NOTE_DENSITY_PAD).all()
        assert (t["loudness"][filled:] == C.LOUDNESS_PAD).all() and (t["instrument"][filled:] == C.INSTRUMENT_PAD).all()
        assert t["instrument"][:filled].any(axis=1).mean() > 0.9
    assert (C.NOTE_DENSITY_PAD, C.LOUDNESS_PAD, C.INSTRUMENT_PAD, C.INSTRUMENT_SIZE) == (0.0, 0.0, 0, 40)


def test_load_clips_reads_the_targets_only_on_request(g, root):
    ids = [str(i) for i in g["ids"]]
    f = V.load_clips(root, ids, motion_type=0)
    assert set(f) == {"semantic", "scene_offset", "motion", "emotion", "chord", "chord_root", "chord_attr", "key", "tgt", "tgt_root",
                      "tgt_attr", "emo_class", "emo_prob"}
    t = V.load_clips(root, ids, motion_type=0, regression_targets=True)
    assert set(t) - set(f) == {"note_density", "loudness", "instrument"}
    assert t["note_density"].shape == (2, 300) and t["instrument"].shape == (2, 300, 40)
    assert np.array_equal(t["instrument"][1], g["ref_017_instrument_300_300"])
    assert all(np.array_equal(f[k], t[k]) for k in f)


def tolerance(fig):
    """(total_loss, rmse_note_density, rmse_loudness, bce_instrument) -> the fp32 allowance of each (see the test below)."""
    total, rmse_nd, rmse_l, bce = np.abs(fig)
    tol_bce = 12004 * H.U * bce
    return np.array([604 * H.U * (total - bce) + tol_bce, 304 * H.U * rmse_nd, 304 * H.U * rmse_l, tol_bce])


@pytest.mark.parametrize("name", list(H.MODELS))
def test_restatement_reproduces_every_recorded_reference_figure(g, root, name):
    """Fed the reference model's own outputs, the restatement's sums give the figures eval_model returned.  The reference forms them
    in fp32: a mean over n rounded terms (n = 300 per RMSE, 600 under the total's root, 12000 for the BCE) and a square root or a
    division, so it is within (n + 4) 2^-24 relative of the fp64 value whatever order torch adds in."""
    ids = [str(i) for i in g["ids"]]
    clips = []
    for fid in ids:
        t = V.read_regression_targets(root, fid)
        r = H.sums(g[f"{name}_{fid}_ln_nd"], g[f"{name}_{fid}_inst"], t["note_density"], t["loudness"], t["instrument"])
        got, want = H.figures(r["clip"][None])[0], g[f"{name}_{fid}_figures"]
        tol = tolerance(want)
        print(name, fid, "error / tolerance", np.abs(got - want) / tol)
        assert (np.abs(got - want) <= tol).all(), (name, fid, got, want)
        clips.append(r["clip"])
        assert float(g[f"{name}_{fid}_mean_inv_sharp"]) < 5 and np.minimum(g[f"{name}_{fid}_inst"], 1 - g[f"{name}_{fid}_inst"]).min() >= 0.01
    s = metrics.summarize_regression({k: np.array(clips)[:, i] for i, k in enumerate(metrics.REG_FIELDS)})
    want = dict(zip(H.FIGURES, g[f"{name}_avg_figures"]))
    tol = tolerance(g[f"{name}_avg_figures"])
    for i, k in enumerate(H.FIGURES):
        assert abs(s["avg_" + k] - want[k]) <= tol[i], (k, s["avg_" + k], want[k])


def test_summarize_follows_eval_model():
    rows = np.array([[300.0, 1200.0, 6000.0, 300], [2700.0, 0.0, 24000.0, 300], [4.0, 4.0, 160.0, 4]])
    per_clip = {k: rows[:, i] for i, k in enumerate(metrics.REG_FIELDS)}
    assert metrics.REG_FIELDS == H.FIELDS
    r = metrics.regression_clip_figures(per_clip)
    assert r["rmse_note_density"].tolist() == [1.0, 3.0, 1.0] and r["rmse_loudness"].tolist() == [2.0, 0.0, 1.0]
    assert r["bce_instrument"].tolist() == [0.5, 2.0, 1.0]
    assert np.allclose(r["total_loss"], [np.sqrt(2.5) + 0.5, np.sqrt(4.5) + 2.0, 2.0], rtol=0, atol=1e-15)
    assert np.array_equal(H.figures(rows), np.stack([r[k] for k in H.FIGURES], axis=1))
    s = metrics.summarize_regression(per_clip)
    assert set(s) == {"avg_total_loss", "avg_rmse_note_density", "avg_rmse_loudness", "avg_bce_instrument"}
    assert s["avg_rmse_note_density"] == 5.0 / 3              # the mean of the clips' roots ...
    assert abs(s["avg_rmse_note_density"] - np.sqrt((300 + 2700 + 4) / 604)) > 0.1        # ... not the root of the pooled mean
    assert s["avg_rmse_loudness"] == 1.0 and s["avg_bce_instrument"] == 3.5 / 3
    assert s["avg_total_loss"] == sum(r["total_loss"].tolist()) / 3


def test_eval_flag_defaults_equal_the_reference(g):
    want = json.loads(str(g["eval_arg_defaults"]))
    got = vars(parse_eval_args([])[0])
    assert {k: got[k] for k in want} == want
    assert set(got) - set(want) == {"output_dir", "test_ids", "synthetic_weights"}
    assert (got["regModel"], got["d_model"], got["dim_feedforward"], got["n_layers"], got["motion_type"], got["batch_size"]) == \
        ("bilstm", 64, 256, 2, 0, 1)
    assert (got["test_ids"], got["synthetic_weights"], got["output_dir"]) == ("split:test", False, "./log")


def test_refusals_come_before_any_device_work():
    from video2music_amd import evaluate_regression as E
    for flag, reason in ((["--force_cpu", "1"], "no CPU path"), (["-is_video", ""], "is_video False"), (["-use_KAN", "1"], "use_KAN"),
                         (["-augmentation", "1"], "augmentation")):
        with pytest.raises(SystemExit, match=reason):
            E.main(flag)


def torch_fp32_clip_rows(c):
    """The reference's expressions (video_regression.py:240-245, run_model_regression.py:104-118) in torch's fp32 on the CPU, as
    per-clip sums."""
    t = {k: torch.from_numpy(v) for k, v in c.items()}
    ln_nd = torch.nn.functional.linear(t["feat"], t["reg_w"], t["reg_b"])
    inst = torch.sigmoid(torch.nn.functional.linear(t["feat"], t["cls_w"], t["cls_b"]))
    rows = []
    for b in range(ln_nd.shape[0]):
        mse = torch.nn.functional.mse_loss
        rows.append([float(mse(ln_nd[b, :, 0], t["note_density"][b], reduction="sum")),
                     float(mse(ln_nd[b, :, 1], t["loudness"][b], reduction="sum")),
                     float(torch.nn.functional.binary_cross_entropy(inst[b], t["instrument"][b], reduction="sum")), ln_nd.shape[1]])
    return np.array(rows, dtype=np.float64), ln_nd.numpy(), inst.numpy()


@pytest.mark.parametrize("B,S,W", H.KERNEL_CASES + [(1, 1030, 40)])
def test_the_reference_expressions_stay_within_the_bounds(B, S, W):
    """Condition check: on the inputs of the GPU test, torch's own fp32 computation is within the stated bounds of the restatement,
    so the inputs are ones for which the reference alone passes."""
    c = H.make_case(B, S, W)
    want = H.restate(**c)
    assert np.abs(want["z"]).max() <= H.Z_MAX
    got, ln_nd, inst = torch_fp32_clip_rows(c)
    err = np.abs(got - want["clip"])
    print("B S W", B, S, W, "max error / bound", (err[:, :3] / want["bound"][:, :3]).max(axis=0))
    assert (err <= want["bound"]).all(), (got, want["clip"], want["bound"])
    assert (np.abs(ln_nd - want["ln_nd"]) <= want["d_ln_nd"]).all()
    assert (np.abs(inst.astype(np.float64) - want["p32"]) <= want["d_z"] / 4 + 4 * H.U).all()
