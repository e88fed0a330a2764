"""Training with -auxiliary_loss / -drop_loss against the REFERENCE's own run (tests/golden/g_train_aux.npz, written by
tools/make_goldens_train_aux.py from the reference's classes, CombinedLoss, dataset, train_epoch and eval_model), with the rules of
tests/test_train_gpu.py and tests/test_train_families_gpu.py: the first batch's loss against fp64 within what a logit error of 1e-4
can move it, and within that plus the reference's own distance from fp64 of the recorded fp32 figure; every gradient against fp64
within 8 e32 (e32: the reference's fp32 gradients against fp64 under this loss, recorded), the recorded fp32 gradients within 9 e32
(ours 8, theirs 1); and `python -m video2music_amd.train_losses` on the miniature dataset.

Epoch figures.  A logit error of at most 1e-4 moves a probability by at most 2e-4 of itself, a hinge by at most 2e-4 (mean top-k +
p_t) <= 4e-4, A_k by w_k times that, the cross-entropy by 2e-4, the BCE mean by 1e-4; the chord figure (CE + A_3 + A_5) / count by at
most 2e-4 + 8 x 4e-4 at any count >= 1, plus the loss kernel's own bound."""
import csv
import os
import random

import numpy as np
import pytest
import torch

from tests import helpers_chord_aux as H
from tests import helpers_family_train as FT
from tests import helpers_train as T
from tests.helpers_eval import loss_bound
from video2music_amd import losses, train, train_losses

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = "g_train_aux.npz"
W = (T.LAM, 1 - T.LAM)
CHORD_TOL = 2e-4 + (3.0 + 5.0) * 4e-4


@pytest.fixture(scope="module")
def bt():
    return T.batch()


def step(m, bt):
    d = lambda k: torch.from_numpy(np.ascontiguousarray(bt[k])).to(DEV)
    y = m(d("x"), d("x_root"), d("x_attr"), d("semantic"), d("key"), d("scene_offset"), d("motion"), d("emotion"))
    loss = losses.chord_train_loss(y, torch.from_numpy(bt["tgt"]), torch.from_numpy(bt["emo_class"]), T.LAM, T.SMOOTHING, auxiliary=True)
    loss.backward()
    return float(loss.detach()), {k: None if p.grad is None else p.grad.cpu().numpy() for k, p in m.named_parameters()}


def fp64_of(logits_fn, sd, bt):
    """(losses (3,), sum |dL/dy|, gradients) of a restated forward with the restated auxiliary loss (view layout), in double."""
    P = {k: torch.as_tensor(np.asarray(v)).to(torch.float64).requires_grad_(True) for k, v in sd.items()}
    y = logits_fn(P)
    y.retain_grad()
    r = H.loss_terms(y, bt["tgt"], bt["emo_class"], T.SMOOTHING, W, "view")
    r["total"].backward()
    return (np.array([float(r[k].detach()) for k in ("total", "chord", "emotion")]), float(y.grad.abs().sum()),
            {k: None if p.grad is None else p.grad.numpy() for k, p in P.items()})


def check_loss(tag, g, lossv, l64, dl_dy):
    bound = 1e-4 * dl_dy + 159 * T.U * abs(l64[0])
    rec, rec64 = g[f"{tag}_loss"], g[f"{tag}_loss64"]
    print(f"{tag}: loss {lossv:.7f} fp64 {l64[0]:.7f} recorded {rec[0]:.7f} (its fp64 {rec64[0]:.7f}) bound {bound:.2e}")
    assert g[f"{tag}_parts"][3] == 3                                             # all three terms live in the recorded batch
    # the restatement is the reference's arithmetic in double, up to the fp32 positional table both read: its sin / cos come from the
    # host's libm, and a last-bit difference there is 6e-8 of an entry
    assert np.abs(l64 - rec64).max() <= 1e-6 * np.abs(rec64).max()
    assert abs(lossv - l64[0]) <= bound and abs(lossv - rec[0]) <= bound + abs(rec[0] - rec64[0])


def test_one_step_of_the_base_model(golden, bt):
    from tests.test_train_gpu import build
    g = golden(G)
    cfg, e32 = T.MODELS["rpr"], float(g["rpr_e32_grad"])
    sd = T.state_dict(cfg)
    l64, dl_dy, g64 = fp64_of(lambda P: T.forward(P, cfg, bt), sd, bt)
    lossv, got = step(build(cfg).train(), bt)
    check_loss("rpr", g, lossv, l64, dl_dy)
    worst = 0.0
    for k, v in g64.items():
        if v is None:
            assert got[k] is None, k
            continue
        err = T.rel_err(got[k], v)
        worst = max(worst, err / e32)
        assert err <= 8 * e32, (k, err, e32)
    print(f"  worst gradient error / e32_grad = {worst:.2f}")
    keys = [k[len("rpr_grad_"):] for k in g if k.startswith("rpr_grad_")]
    assert len(keys) == 14
    for k in keys:
        assert T.rel_err(got[k], g[f"rpr_grad_{k}"]) <= 9 * e32, k
    # the auxiliary terms are in the gradient: the plain loss's differs by far more than the bound
    m = build(cfg).train()
    d = lambda k: torch.from_numpy(np.ascontiguousarray(bt[k])).to(DEV)
    y = m(d("x"), d("x_root"), d("x_attr"), d("semantic"), d("key"), d("scene_offset"), d("motion"), d("emotion"))
    losses.chord_train_loss(y, torch.from_numpy(bt["tgt"]), torch.from_numpy(bt["emo_class"]), T.LAM, T.SMOOTHING).backward()
    assert T.rel_err(m.get_parameter("Wout.weight").grad.cpu().numpy(), g64["Wout.weight"]) > 100 * 8 * e32


def test_one_step_of_a_family_model(golden, bt):
    from tests.test_train_families_gpu import build
    g = golden(G)
    tag, e32 = "v22", float(g["v22_e32_grad"])
    l64, dl_dy, g64 = fp64_of(lambda P: FT.forward_restated(P, FT.GOLDEN[tag], FT.golden_inputs(), None, None, (), [], True),
                              FT.golden_state_dict(tag), bt)
    lossv, got = step(build(tag).train(), bt)
    check_loss(tag, g, lossv, l64, dl_dy)
    errs = FT.grad_errors(got, g64)
    worst = max(errs, key=errs.get)
    print(f"  worst gradient {worst}: {errs[worst]:.3e} = {errs[worst] / e32:.2f} e32_grad")
    bad = {k: e for k, e in errs.items() if not e <= FT.FACTOR * e32}
    assert not bad, (e32, bad)
    keys = [k[len("v22_grad_"):] for k in g if k.startswith("v22_grad_")]
    assert len(keys) == 8
    for k in keys:
        assert FT.rel_err(got[k], g[f"v22_grad_{k}"], FT.grad_scale(g64, k)) <= (FT.FACTOR + 1) * e32, k


def test_three_adam_steps_follow_the_recorded_reference_run(golden, bt):
    """The rule of tests/test_train_gpu.py's test of the same name, with the combined loss in the steps (view layout) and in
    `evaluate` (rows layout, per clip): the training loss before each step and the figures after within 2 % of the recorded decrease."""
    from tests.test_train_gpu import build
    g = golden(G)
    want_before, want_after, want_traj = g["rpr_figs_before"], g["rpr_figs_after"], g["rpr_adam_losses"]
    m = build(T.MODELS["rpr"])
    data = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in
            dict(bt, chord=np.pad(bt["x"], ((0, 0), (0, 1))), chord_root=np.pad(bt["x_root"], ((0, 0), (0, 1))),
                 chord_attr=np.pad(bt["x_attr"], ((0, 0), (0, 1)))).items()}
    figs = lambda: np.array([train.evaluate(m, data, 1, T.S_VIDEO, T.SMOOTHING, auxiliary=True)[k] for k in T.FIGURES])
    before = figs()
    tol = np.array([T.LAM * CHORD_TOL + (1 - T.LAM) * 1e-4, CHORD_TOL, 1e-4]) + loss_bound(T.L_CHORD, want_before[:3] * T.L_CHORD) / T.L_CHORD
    assert (np.abs(before[:3] - want_before[:3]) <= tol).all() and np.array_equal(before[3:], want_before[3:])

    class Args:
        optimizer = "Adam"
    opt = train.make_optimizer(Args, m.parameters(), T.ADAM_LR)
    traj = []
    for _ in range(T.ADAM_STEPS):
        opt.zero_grad()
        m.train()
        d = lambda k: torch.from_numpy(np.ascontiguousarray(bt[k])).to(DEV)
        y = m(d("x"), d("x_root"), d("x_attr"), d("semantic"), d("key"), d("scene_offset"), d("motion"), d("emotion"))
        loss = losses.chord_train_loss(y, torch.from_numpy(bt["tgt"]), torch.from_numpy(bt["emo_class"]), T.LAM, T.SMOOTHING, auxiliary=True)
        loss.backward()
        opt.step()
        traj.append(float(loss.detach()))
    after = figs()
    print(f"losses {traj} recorded {want_traj}\n  after {after} recorded {want_after}")
    assert (np.diff(traj) < 0).all() and (np.diff(want_traj) < 0).all() and after[0] < before[0] and want_after[0] < want_before[0]
    assert (np.abs(np.array(traj) - want_traj) <= 0.02 * (want_traj[0] - want_traj[-1])).all()
    assert (np.abs(after[:3] - want_after[:3]) <= 0.02 * np.abs(want_before[:3] - want_after[:3])).all()


# ---- python -m video2music_amd.train_losses on the miniature dataset ----
MODEL = ["-n_layers", "2", "-num_heads", "2", "-d_model", "64", "-dim_feedforward", "128", "-motion_type", "0"]


def run_cli(tmp_path, name, extra, epochs=2, batch_size=2, seed=0):
    root, out = str(tmp_path / name / "vevo"), str(tmp_path / name / "out")
    os.makedirs(root)
    ids = ",".join(T.write_dataset(root))
    argv = ["-dataset_dir", root, "-output_dir", out, "-music_gen_version", "None", "-chord_embed", "", "-epochs", str(epochs), "-batch_size",
            str(batch_size), "-weight_modulus", "1", "-print_modulus", "1", "-lr", "1e-3", "--train_ids", ids, "--val_ids", ids, "--seed",
            str(seed), "--synthetic_weights"] + MODEL + extra
    res = train_losses.main(argv)
    rows = list(csv.reader(open(os.path.join(out, "AMT", "results.csv"))))
    return argv, out, res, rows


def test_cli_with_auxiliary_loss_two_epochs(golden, tmp_path, capsys):
    g = golden(G)
    argv, out, res, rows = run_cli(tmp_path, "aux", ["-auxiliary_loss", "1"])
    assert "loss_weights" not in res and "Train loss (total):" in capsys.readouterr().out
    assert rows[0] == train.CSV_HEADER and [r[0] for r in rows[1:]] == ["0", "1", "2"] and all(len(r) == 14 for r in rows)
    fig = np.array([[float(v) for v in r[2:]] for r in rows[1:]])
    assert np.isfinite(fig).all() and np.array_equal(fig[:, :6], fig[:, 6:])          # the same clips train and validate here
    assert "auxiliary_loss: True" in open(os.path.join(out, "AMT", "model_params.txt")).read()
    # epoch 0 is the synthetic model of the fixture before any step: eval_model's recorded figures with the combined loss
    want = g["rpr_figs_before"]
    tol = np.array([T.LAM * CHORD_TOL + (1 - T.LAM) * 1e-4, CHORD_TOL, 1e-4]) + loss_bound(T.L_CHORD, want[:3] * T.L_CHORD) / T.L_CHORD
    print(f"epoch 0 {fig[0, :6]} recorded {want}, |diff| / tol {np.abs(fig[0, :3] - want[:3]) / tol}")
    assert (np.abs(fig[0, :3] - want[:3]) <= tol).all() and np.array_equal(fig[0, 3:6], want[3:])
    assert fig[2, 0] < fig[0, 0]                                                       # two epochs of Adam lower the total loss
    # every row is what evaluate() gives on that epoch's saved weights, with the auxiliary chord figure
    args = train.parse_args(argv)
    data = train.load(args, train.names_of(args, args.train_ids), torch.device(DEV))
    from video2music_amd.generate import total_vf_dim_of
    for e in (0, 1, 2):
        m = train.build_model(args, total_vf_dim_of(args, sem_dim=data["semantic"].shape[-1]))
        m.load_state_dict(torch.load(train.epoch_weights_path(os.path.join(out, "AMT", "weights"), e)))
        figs = train.evaluate(m.to(DEV), data, 2, args.max_sequence_chord, 0.1, auxiliary=True)
        assert [figs[k] for k in train.FIGURE_KEYS] == fig[e, :6].tolist(), e
        plain = train.evaluate(m, data, 2, args.max_sequence_chord, 0.1)
        assert plain["avg_loss_chord"] != figs["avg_loss_chord"] and plain["avg_loss_emotion"] == figs["avg_loss_emotion"]


def test_cli_with_drop_loss_repeats_from_its_seed_and_follows_the_draws(tmp_path):
    runs = [run_cli(tmp_path, f"drop{i}", ["-drop_loss", "1", "-auxiliary_loss", "1"], epochs=2, batch_size=1, seed=0) for i in range(2)]
    (_, _, res_a, rows_a), (_, _, res_b, rows_b) = runs
    assert rows_a == rows_b and len(rows_a) == 4
    rng = random.Random(0)
    want = [train.drop_loss_weights(rng.random()) for _ in range(4)]                   # two epochs of two steps
    assert res_a["loss_weights"] == res_b["loss_weights"] == want
    assert set(want) == {(0.4, 0.6), (1.0, 0.0), (0.0, 1.0)}                           # seed 0 draws all three in its first four
    _, _, res_c, rows_c = run_cli(tmp_path, "drop_other", ["-drop_loss", "1", "-auxiliary_loss", "1"], epochs=2, batch_size=1, seed=1)
    assert res_c["loss_weights"] != want and rows_c[1][2:] == rows_a[1][2:] and rows_c[3] != rows_a[3]
