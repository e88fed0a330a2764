"""python -m video2music_amd.evaluate_regression on the miniature dataset of g_reg_eval.npz with procedural weights, against the
figures the reference's eval_model returned for the same files and weights on the CPU."""
import json
import os

import numpy as np
import pytest

from tests import helpers_reg_eval as H
from video2music_amd import evaluate_regression

pytestmark = pytest.mark.gpu
TOL = 5e-5              # what g_reg.npz pins for these heads' outputs; an RMSE moves by at most the largest element error
LABELS = ["Avg Total loss", "Avg RMSE (Note Density)", "Avg RMSE (Loudness)", "Avg BCE (Instrument)"]


@pytest.fixture(scope="module")
def g(golden):
    return golden("g_reg_eval.npz")


@pytest.fixture(scope="module")
def root(g, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("vevo_reg_eval"))
    H.write_reg_dataset(path, H.content_of(g))
    return path


def argv(root, out, name, batch, ids=None):
    cfg = H.MODELS[name]
    a = ["-dataset_dir", root, "-output_dir", out, "-regModel", cfg["regModel"], "-d_model", str(cfg["d_model"]), "-n_layers",
         str(cfg["n_layers"]), "-dim_feedforward", str(cfg["dim_feedforward"]), "-batch_size", str(batch), "--synthetic_weights"]
    return a + (["--test_ids", ids] if ids else [])


def tolerances(inv_sharp):
    """(total_loss, rmse_note_density, rmse_loudness, bce_instrument): a BCE term moves by the probability's error over min(p, 1 - p)."""
    bce = TOL * inv_sharp
    return np.array([TOL + bce, TOL, TOL, bce])


@pytest.mark.parametrize("name", list(H.MODELS))
def test_evaluate_regression_cli(g, root, tmp_path, capsys, name):
    ids = [str(i) for i in g["ids"]]
    out = str(tmp_path / "split")
    summary = evaluate_regression.main(argv(root, out, name, 2))
    lines = capsys.readouterr().out.strip().splitlines()[-4:]
    assert [ln.rsplit(":", 1)[0] for ln in lines] == LABELS
    assert lines[0] == f"Avg Total loss: {summary['avg_total_loss']}" and lines[3] == f"Avg BCE (Instrument): {summary['avg_bce_instrument']}"
    got = json.load(open(os.path.join(out, "metrics.json")))
    assert got["summary"] == summary and [c["id"] for c in got["clips"]] == ids
    inv = [float(g[f"{name}_{fid}_mean_inv_sharp"]) for fid in ids]
    for clip, fid, s in zip(got["clips"], ids, inv):
        err = np.abs(np.array([clip[k] for k in H.FIGURES]) - g[f"{name}_{fid}_figures"])
        print(name, fid, "error / tolerance", err / tolerances(s))
        assert (err <= tolerances(s)).all(), (name, fid, clip, g[f"{name}_{fid}_figures"])
        assert clip["n_rows"] == 300
    err = np.abs(np.array([summary["avg_" + k] for k in H.FIGURES]) - g[f"{name}_avg_figures"])
    assert (err <= tolerances(max(inv))).all(), (summary, g[f"{name}_avg_figures"])

    # the per-clip figures do not depend on -batch_size
    by_batch = {}
    for b in (1, 3):
        evaluate_regression.main(argv(root, str(tmp_path / f"b{b}"), name, b, ids="003,017,003"))
        by_batch[b] = json.load(open(os.path.join(str(tmp_path / f"b{b}"), "metrics.json")))["clips"]
    capsys.readouterr()
    assert [c["id"] for c in by_batch[1]] == [c["id"] for c in by_batch[3]] == ["003", "017", "003"]
    for c1, c3 in zip(by_batch[1], by_batch[3]):
        s = float(g[f"{name}_{c1['id']}_mean_inv_sharp"])
        d = np.abs(np.array([c1[k] - c3[k] for k in H.FIGURES]))
        assert (d <= tolerances(s)).all(), (name, c1, c3)
        assert (np.abs(np.array([c3[k] for k in H.FIGURES]) - g[f"{name}_{c3['id']}_figures"]) <= tolerances(s)).all()
