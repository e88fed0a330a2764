"""Training of the V3 chord models against the REFERENCE's own run (tests/golden/g_train_v3.npz, written by
tools/make_goldens_train_v3.py from the reference's classes, dataset, train_epoch and eval_model) with the rules of
tests/test_train_families_gpu.py: the first batch's loss and every gradient against fp64 within 8 e32 (e32: the reference's fp32
gradients against the fp64 restatement, recorded; the lambda vectors at their own scale), the recorded logits rows within 1e-4, the
recorded fp32 gradients within 9 e32 (ours 8, theirs 1), both routing-bias buffers after the step within 1e-7 of the reference's (the
counts are integers: anything larger is another selection), three Adam passes within 2 % of the recorded decrease, and the command line."""
import numpy as np
import pytest
import torch

from tests import helpers_train as T
from tests import helpers_v3_train as V
from video2music_amd import losses
from video2music_amd.model import video_music_transformer as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = "g_train_v3.npz"


def build(tag):
    m = M.VideoMusicTransformer_V3(**V.golden_kwargs(tag))
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in V.golden_state_dict(tag).items()}, strict=False)
    assert not missing and not unexpected
    return m.to(DEV).enable_training()


def train_loss(m, bt):
    d = lambda k: torch.from_numpy(np.ascontiguousarray(bt[k])).to(DEV)
    y = m(d("x"), d("x_root"), d("x_attr"), d("semantic"), d("key"), d("scene_offset"), d("motion"), d("emotion"))
    return y, losses.chord_train_loss(y, torch.from_numpy(bt["tgt"]), torch.from_numpy(bt["emo_class"]), T.LAM, T.SMOOTHING)


@pytest.fixture(scope="module")
def bt():
    return T.batch()


@pytest.mark.parametrize("tag", list(V.GOLDEN))
def test_first_loss_logits_gradients_and_bias_buffers(golden, tag, bt):
    g = golden(G)
    e32, e32_lam, e32_y = float(g[f"{tag}_e32_grad"]), float(g[f"{tag}_e32_lambda"]), float(g[f"{tag}_e32_y"])
    l64, y64, g64, recs, scales = V.golden_fp64(tag)
    assert V.biased_gap(recs) >= V.ROUTE_GAP
    m = build(tag).train()
    y, loss = train_loss(m, bt)
    loss.backward()
    got = {k: None if p.grad is None else p.grad.cpu().numpy() for k, p in m.named_parameters()}
    y = y.detach().cpu().numpy()
    yl = torch.from_numpy(y64).requires_grad_(True)
    T.loss(yl, bt)[0].backward()
    bound = 1e-4 * float(yl.grad.abs().sum()) + 159 * T.U * abs(l64[0])
    d_ref = np.abs(y[:, T.LOGIT_ROWS] - g[f"{tag}_logits_rows"]).max()
    lossv = float(loss.detach())
    print(f"{tag}: loss {lossv:.7f} fp64 {l64[0]:.7f} recorded {g[f'{tag}_loss'][0]:.7f} bound {bound:.2e}; logits - recorded {d_ref:.3e}, "
          f"logit error {V.logit_err(y, y64):.3e} (recorded e32_y {e32_y:.3e})")
    assert abs(lossv - l64[0]) <= bound and abs(lossv - g[f"{tag}_loss"][0]) <= bound + abs(g[f"{tag}_loss"][0] - l64[0])
    assert d_ref <= 1e-4 and V.logit_err(y, y64) <= V.LOGIT_FACTOR * e32_y
    unrouted = set(g[f"{tag}_unrouted"].tolist())
    assert {k for k, v in got.items() if v is None} == set(g[f"{tag}_unused"].tolist()) - unrouted
    assert all(not got[k].any() for k in unrouted)
    params = {k: v for k, v in g64.items() if not k.endswith(".ff.bias")}
    plain, lam = V.grad_errors(got, params, scales)
    worst = max(plain, key=plain.get)
    print(f"  worst gradient {worst}: {plain[worst]:.3e} = {plain[worst] / e32:.2f} e32_grad; worst lambda vector {max(lam.values()):.3e} "
          f"(recorded e32_lambda {e32_lam:.3e})")
    bad = {k: e for k, e in plain.items() if not e <= V.FACTOR * e32}
    assert not bad, (e32, bad)
    lam_bound = max(V.FACTOR * e32_lam, V.FACTOR * V.U)
    bad = {k: e for k, e in lam.items() if not e <= lam_bound}
    assert not bad, (lam_bound, bad)
    for k in V.GOLDEN_KEYS[tag]:
        want = g[f"{tag}_grad_{k}"]
        if V.is_lambda(k):
            assert V.rel_err(got[k], want, scales[k]) <= lam_bound + e32_lam, k
        else:
            assert V.rel_err(got[k], want, V.grad_scale(g64, k)) <= (V.FACTOR + 1) * e32, k
    keys = V.bias_keys(V.golden_state_dict(tag))
    assert len(keys) == 2
    for k in keys:
        after = dict(m.named_buffers())[k].cpu().numpy()
        assert np.abs(after - g[f"{tag}_bias_{k}"]).max() <= 1e-7, k
        assert not np.array_equal(after, V.golden_state_dict(tag)[k])


@pytest.mark.parametrize("tag", list(V.GOLDEN))
def test_three_adam_steps_lower_the_total_loss_as_the_recorded_reference_run_does(golden, tag, bt):
    from tests.helpers_eval import loss_bound
    from video2music_amd import train
    g = golden(G)
    want_before, want_after, want_traj = g[f"{tag}_figs_before"], g[f"{tag}_figs_after"], g[f"{tag}_adam_losses"]
    m = build(tag)
    data = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in
            dict(bt, chord=np.pad(bt["x"], ((0, 0), (0, 1))), chord_root=np.pad(bt["x_root"], ((0, 0), (0, 1))),
                 chord_attr=np.pad(bt["x_attr"], ((0, 0), (0, 1)))).items()}
    figs = lambda: np.array([train.evaluate(m, data, 2, T.S_VIDEO, T.SMOOTHING)[k] for k in T.FIGURES])
    before = figs()
    tol = np.array([2e-4, 2e-4, 1e-4]) + loss_bound(T.L_CHORD, want_before[:3] * T.L_CHORD) / T.L_CHORD
    print(f"{tag}: before {before} recorded {want_before}")
    assert (np.abs(before[:3] - want_before[:3]) <= tol).all() and np.array_equal(before[3:], want_before[3:])

    class Args:
        optimizer = "Adam"
    opt = train.make_optimizer(Args, m.parameters(), T.ADAM_LR)
    traj = []
    for _ in range(T.ADAM_STEPS):
        opt.zero_grad()
        loss = train_loss(m.train(), bt)[1]
        loss.backward()
        opt.step()
        traj.append(float(loss.detach()))
    after = figs()
    print(f"  losses {traj} recorded {want_traj}\n  after {after} recorded {want_after}")
    assert (np.diff(traj) < 0).all() and (np.diff(want_traj) < 0).all() and after[0] < before[0] and want_after[0] < want_before[0]
    assert (np.abs(np.array(traj) - want_traj) <= 0.02 * (want_traj[0] - want_traj[-1])).all()
    assert (np.abs(after[:3] - want_after[:3]) <= 0.02 * np.abs(want_before[:3] - want_after[:3])).all()


def _dataset(golden, tmp_path):
    import os
    from tests.helpers_features import write_mini_dataset
    g = golden("g_eval.npz")
    root = str(tmp_path / "vevo")
    os.makedirs(root)
    content = {k[3:]: g[k] for k in g if k.startswith("in_")}
    content["ids"] = [str(i) for i in g["ids"]]
    write_mini_dataset(root, content)
    return root, ",".join(content["ids"])


def _run(golden, tmp_path, epochs, extra):
    from video2music_amd import train_v3
    root, ids = _dataset(golden, tmp_path)
    out = str(tmp_path / "out")
    res = train_v3.main(["-dataset_dir", root, "-output_dir", out, "-epochs", str(epochs), "-batch_size", "2", "-weight_modulus", "1",
                         "-print_modulus", "1", "-lr", "1e-3", "--train_ids", ids, "--val_ids", ids, "--seed", "3", "--synthetic_weights",
                         "-n_layers", "4", "-num_heads", "2", "-d_model", "64", "-dim_feedforward", "128", "-motion_type", "1"] + extra)
    return out, res


def test_cli_trains_a_v3_model_two_epochs_and_writes_the_reference_s_files(golden, tmp_path, capsys):
    import csv
    import os
    from video2music_amd import train
    out, res = _run(golden, tmp_path, 2, ["-music_gen_version", "3.1", "-chord_embed", ""])
    amt = os.path.join(out, "AMT")
    for name in ("model_params.txt", "results.csv", "best_loss_weights.pickle", "best_epochs.txt", "weights/epoch_0000.pickle",
                 "weights/epoch_0001.pickle", "weights/epoch_0002.pickle"):
        assert os.path.isfile(os.path.join(amt, name)), name
    assert open(os.path.join(out, "model_architecture.txt")).read().startswith("VideoMusicTransformer_V3")
    assert "music_gen_version: 3.1" in open(os.path.join(amt, "model_params.txt")).read()
    rows = list(csv.reader(open(os.path.join(amt, "results.csv"))))
    assert rows[0] == train.CSV_HEADER and [r[0] for r in rows[1:]] == ["0", "1", "2"] and all(len(r) == 14 for r in rows)
    fig = np.array([[float(v) for v in r[2:]] for r in rows[1:]])
    assert np.isfinite(fig).all() and np.array_equal(fig[:, :6], fig[:, 6:])
    assert fig[2, 0] < fig[0, 0]                                 # two epochs of Adam lower the total loss
    assert res["best_epoch"] in (1, 2, 3) and "Train loss (total):" in capsys.readouterr().out
    best, first = (torch.load(os.path.join(amt, n)) for n in ("best_loss_weights.pickle", "weights/epoch_0000.pickle"))
    M.VideoMusicTransformer_V3(version_name="3.1", n_layers=4, num_heads=2, d_model=64, dim_feedforward=128,
                               total_vf_dim=best["Linear_vis.weight"].shape[1]).load_state_dict(best, strict=True)
    k = "transformer.decoder.layers.3.ff.bias"
    assert not torch.equal(best["Wout.weight"], first["Wout.weight"]) and not torch.equal(best[k], first[k])
    assert not torch.equal(best["transformer.decoder.layers.0.self_attn.lambda_q1"], first["transformer.decoder.layers.0.self_attn.lambda_q1"])


def test_cli_trains_2_2_with_balancing_one_epoch(golden, tmp_path):
    import os
    out, _ = _run(golden, tmp_path, 1, ["-music_gen_version", "2.2", "-balancing", "1"])
    first, last = (torch.load(os.path.join(out, "AMT", "weights", n)) for n in ("epoch_0000.pickle", "epoch_0001.pickle"))
    k = "transformer.encoder.layers.3.ff.bias"
    assert k in last and not torch.equal(first[k], last[k]) and not torch.equal(first["Wout.weight"], last["Wout.weight"])
