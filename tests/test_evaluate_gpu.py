"""python -m video2music_amd.evaluate on the miniature dataset of g_eval.npz with procedural weights: metrics.json against the fp64
restatement applied to the logits the same model's forward returns, independence of -batch_size, and the confusion matrices."""
import json
import os

import numpy as np
import pytest
import torch

from tests import helpers_eval as H
from tests.helpers_features import write_mini_dataset
from video2music_amd import evaluate, metrics
from video2music_amd.dataset import vevo_features as V
from video2music_amd.utilities import constants as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOP = [1, 122, 66, 92, 57, 14, 27, 40, 0, 156]        # ten leading chords of the test's vevo_meta/top_chord.txt


@pytest.fixture(scope="module")
def dataset(golden, tmp_path_factory):
    g = golden("g_eval.npz")
    root = str(tmp_path_factory.mktemp("vevo_eval"))
    content = {k[3:]: g[k] for k in g if k.startswith("in_")}
    content["ids"] = [str(i) for i in g["ids"]]
    write_mini_dataset(root, content)
    with open(os.path.join(root, "vevo_meta", "top_chord.txt"), "w") as fh:
        fh.write("".join(f"{C.chord_name(cid)} {cid} {1000 - i}\n" for i, cid in enumerate(TOP + [5, 6])) + "\n")
    return root, content["ids"]


def argv(root, out, version, batch):
    return ["-dataset_dir", root, "-output_dir", out, "-music_gen_version", version, "-motion_type", "1", "-n_layers", "2", "-num_heads", "4",
            "-d_model", "64", "-dim_feedforward", "128", "-batch_size", str(batch), "--synthetic_weights", "-save_conf_matrix"]


def count(true, pred, labels):
    m = np.zeros((len(labels), len(labels)), dtype=np.int64)
    for t, p in zip(true.reshape(-1).tolist(), pred.reshape(-1).tolist()):
        if t in labels and p in labels:
            m[labels.index(t), labels.index(p)] += 1
    return m


@pytest.mark.parametrize("version", ["None", "2.2"])
def test_evaluate_cli(dataset, tmp_path, capsys, version):
    root, ids = dataset
    out = {b: str(tmp_path / f"b{b}") for b in (1, 2)}
    summary = evaluate.main(argv(root, out[2], version, 2))
    lines = capsys.readouterr().out.strip().splitlines()[-6:]
    assert [ln.rsplit(":", 1)[0] for ln in lines] == ["Avg test loss (total)", "Avg test loss (chord)", "Avg test loss (emotion)",
                                                      "Avg test h1", "Avg test h3", "Avg test h5"]
    assert lines[0] == f"Avg test loss (total): {summary['avg_total_loss']:.4f}" and lines[5] == f"Avg test h5: {summary['avg_h5']:.4f}"
    evaluate.main(argv(root, out[1], version, 1))
    got = {b: json.load(open(os.path.join(out[b], "metrics.json"))) for b in (1, 2)}
    assert got[1] == got[2]                                  # per-clip rows and summary do not depend on -batch_size
    assert got[2]["summary"] == summary and [c["id"] for c in got[2]["clips"]] == ids

    # the same model's forward, the restatement on its logits
    args = evaluate.parse_args(argv(root, out[2], version, 2))
    f = V.load_clips(root, ids, motion_type=1)
    model = evaluate.load_model(args, f["semantic"].shape[-1], torch.device(DEV))
    t = {k: torch.from_numpy(v).to(DEV) for k, v in f.items()}
    with torch.no_grad():           # clip by clip, as the reference evaluates (batch_size 1)
        y = torch.cat([model(t["chord"][b:b + 1, :299].contiguous(), t["chord_root"][b:b + 1, :299].contiguous(),
                             t["chord_attr"][b:b + 1, :299].contiguous(), t["semantic"][b:b + 1], t["key"][b:b + 1],
                             t["scene_offset"][b:b + 1], t["motion"][b:b + 1], t["emotion"][b:b + 1]) for b in range(len(ids))])
    want = H.restate(y.cpu().numpy(), f["tgt"], f["emo_class"], f["emo_prob"], C.EMOTION_THRESHOLD)
    assert len(np.unique(want["pred"])) > 3                  # the procedural model does not predict one chord everywhere
    want_ratios = metrics.clip_ratios({k: want["clip"][:, i] for i, k in enumerate(metrics.FIELDS)})
    for b, clip in enumerate(got[2]["clips"]):
        for i, k in enumerate(metrics.FIELDS):
            if k in ("ce_sum", "bce_sum"):
                assert abs(clip[k] - want["clip"][b, i]) <= H.loss_bound(299, want["clip"][b, i]), (k, clip[k], want["clip"][b, i])
            else:
                assert clip[k] == want["clip"][b, i], (k, clip[k], want["clip"][b, i])
        for k in ("acc", "h1", "h3", "h5", "cor"):
            assert clip[k] == want_ratios[k][b], k
        for k in ("loss_chord", "loss_emotion", "total_loss"):
            assert abs(clip[k] - want_ratios[k][b]) <= H.loss_bound(299, want_ratios[k][b]), k
    want_summary = metrics.summarize({k: want["clip"][:, i] for i, k in enumerate(metrics.FIELDS)})
    for k, v in want_summary.items():
        if "loss" in k:
            assert abs(summary[k] - v) <= H.loss_bound(299, v), k
        else:
            assert summary[k] == v, k

    # confusion matrices: plain counts over all positions
    root_ids, attr_ids = metrics.pred_root_attr(want["pred"])
    assert np.array_equal(np.load(os.path.join(out[2], "chord_root.npy")), count(f["tgt_root"], root_ids, list(range(1, 13))))
    assert np.array_equal(np.load(os.path.join(out[2], "chord_attr.npy")), count(f["tgt_attr"], attr_ids, list(range(1, 14))))
    chord = np.load(os.path.join(out[2], "chord.npy"))
    assert chord.shape == (10, 10) and np.array_equal(chord, count(f["tgt"], want["pred"], TOP))
