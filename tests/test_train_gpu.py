"""`loss.backward()` on the base `VideoMusicTransformer` in the training state (model/video_music_transformer.py `_forward_train`,
video2music_amd/autograd.py) on the fixture's two models (tests/helpers_train.py, tests/golden/g_train.npz).

Bounds.  e32_grad / e32_upd are the recorded noise levels of the reference's own fp32 training arithmetic against fp64; our fp32
figures are held to 8 times them, the factor of tests/test_rnn_train_gpu.py (another summation order, device exp / log a few ulps
wide).  The loss: |dL| <= sum |dL/dy| |dy| with |dy| <= 1e-4, the forward's golden tolerance, and sum |dL/dy| taken from the fp64
gradient of the logits."""
import numpy as np
import pytest
import torch

from tests import helpers_train as T
from video2music_amd import losses
from video2music_amd.model.video_music_transformer import VideoMusicTransformer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def build(cfg, dropout=0.0, sd=None):
    m = VideoMusicTransformer(dropout=dropout, **cfg)
    sd = T.state_dict(cfg) if sd is None else sd
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing)
    return m.to(DEV)


def logits_of(m, bt):
    d = lambda k, dt=None: torch.from_numpy(np.ascontiguousarray(bt[k])).to(DEV) if dt is None else torch.from_numpy(np.ascontiguousarray(bt[k])).to(DEV, dt)
    return m(d("x"), d("x_root"), d("x_attr"), d("semantic"), d("key"), d("scene_offset"), d("motion"), d("emotion"))


def train_loss(m, bt, fused=True, smoothing=T.SMOOTHING):
    y = logits_of(m, bt)
    if fused:
        return y, losses.chord_train_loss(y, torch.from_numpy(bt["tgt"]), torch.from_numpy(bt["emo_class"]), T.LAM, smoothing)
    dev_bt = {"tgt": bt["tgt"], "emo_class": bt["emo_class"]}
    tgt = torch.from_numpy(bt["tgt"]).to(DEV).reshape(-1)
    from tests import helpers_eval as HE
    from video2music_amd.utilities import constants as C
    rows = torch.from_numpy(HE.emotion_rows(dev_bt["tgt"], dev_bt["emo_class"])).float().to(DEV)
    chord = torch.nn.CrossEntropyLoss(ignore_index=C.CHORD_PAD, label_smoothing=smoothing)(y.reshape(-1, C.CHORD_SIZE), tgt)
    return y, T.LAM * chord + (1 - T.LAM) * torch.nn.BCEWithLogitsLoss()(y, rows)


def grads_of(m):
    return {k: None if p.grad is None else p.grad.detach().cpu().numpy() for k, p in m.named_parameters()}


@pytest.fixture(scope="module")
def bt():
    return T.batch()


@pytest.fixture(scope="module", params=list(T.MODELS))
def case(request, bt):
    cfg = T.MODELS[request.param]
    sd = T.state_dict(cfg)
    return request.param, cfg, sd, T.grads(sd, cfg, bt, torch.float64)


def test_training_state_logits_equal_the_eval_state_and_the_reference(golden, case, bt):
    name, cfg, sd, (l64, y64, g64) = case
    m = build(cfg).train()
    y = logits_of(m, bt)
    assert y.requires_grad and y.shape == (T.B_CLIPS, T.L_CHORD, 159)
    with torch.no_grad():
        y_eval = logits_of(m.eval(), bt)
    assert not y_eval.requires_grad
    d_eval = float((y - y_eval).abs().max())
    d_ref = np.abs(y.detach().cpu().numpy()[:, T.LOGIT_ROWS] - golden("g_train.npz")[f"{name}_logits_rows"]).max()
    print(f"{name}: train - eval {d_eval:.3e}, train - reference {d_ref:.3e}")
    assert d_eval <= 1e-4 and d_ref <= 1e-4
    m.train()
    with torch.no_grad():                                              # gradients off: the handle path, bit for bit
        assert torch.equal(logits_of(m, bt), y_eval)


@pytest.mark.parametrize("fused", [True, False])
def test_first_loss_and_every_gradient(golden, case, bt, fused):
    name, cfg, sd, (l64, y64, g64) = case
    e32 = float(golden("g_train.npz")[f"{name}_e32_grad"])
    m = build(cfg).train()
    y, loss = train_loss(m, bt, fused)
    loss.backward()
    got = grads_of(m)
    yl = torch.from_numpy(y64).requires_grad_(True)
    T.loss(yl, bt)[0].backward()
    bound = 1e-4 * float(yl.grad.abs().sum()) + 159 * T.U * abs(l64[0])
    print(f"{name} fused {fused}: loss {float(loss):.7f} fp64 {l64[0]:.7f} bound {bound:.2e}")
    assert abs(float(loss) - l64[0]) <= bound
    worst = 0.0
    for k, g in g64.items():
        if g is None:
            assert got[k] is None, k                                   # embedding, condition_linear, Wout_root, Wout_attr
            continue
        err = T.rel_err(got[k], g)
        worst = max(worst, err / e32)
        assert err <= 8 * e32, (k, err, e32)
    print(f"  worst gradient error / e32_grad = {worst:.2f}")
    m.zero_grad(set_to_none=True)
    train_loss(m, bt, fused)[1].backward()
    again = grads_of(m)
    assert all((got[k] is None and again[k] is None) or np.array_equal(got[k], again[k]) for k in got)     # same bits twice


def test_three_sgd_steps_and_the_next_eval_forward(golden, case, bt):
    name, cfg, sd, _ = case
    e32u = float(golden("g_train.npz")[f"{name}_e32_upd"])
    m = build(cfg).train()
    with torch.no_grad():
        y0 = logits_of(m.eval(), bt).clone()
    m.train()
    opt = torch.optim.SGD(m.parameters(), lr=T.SGD_LR)
    P64 = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    for _ in range(T.SGD_STEPS):
        opt.zero_grad()
        loss = train_loss(m, bt)[1]
        loss.backward()
        opt.step()
        l64, _, g = T.grads(P64, cfg, bt, torch.float64)
        # the loss before each step follows the fp64 run (at this rate it overshoots on the third): logits within 1e-4 move the
        # cross-entropy by at most 2e-4 and the BCE mean by 1e-4, so the total by (2 lambda + 1 - lambda) 1e-4 <= 2e-4
        assert abs(float(loss) - l64[0]) <= 2e-4 + 159 * T.U * l64[0], (float(loss), l64[0])
        P64 = {k: (v if g[k] is None else v - T.SGD_LR * g[k]) for k, v in P64.items()}
    for k, p in m.named_parameters():
        if k in T.UNUSED:
            continue
        want = P64[k] - np.asarray(sd[k], dtype=np.float64)
        assert T.rel_err(p.detach().cpu().numpy().astype(np.float64) - np.asarray(sd[k], dtype=np.float64), want) <= 8 * e32u, k
    with torch.no_grad():                                              # the handle re-reads the stepped weights
        y1 = logits_of(m.eval(), bt)
    y1_64 = T.forward({k: torch.from_numpy(v) for k, v in P64.items()}, cfg, bt).numpy()
    assert float((y1 - y0).abs().max()) > 1e-3 and np.abs(y1.cpu().numpy() - y1_64).max() <= 1e-3


def test_three_adam_steps_lower_the_total_loss_as_the_recorded_reference_run_does(golden, case, bt):
    """The reference's train_epoch with its Adam settings at lr 1e-3, three passes over the one batch, eval_model's figures (training
    loss function, per clip) on either side: recorded in g_train.npz.  Ours starts from the same figures -- losses within the change
    a logit error of 1e-4 (the forward's tolerance) can make, 2e-4 for the cross-entropy and 1e-4 for the BCE mean, plus the loss kernels'
    own bound; hits exactly 0 at the start, as recorded -- and Adam's first steps are sign-like (lr g / (|g| + eps)), so a gradient
    within 8 e32_grad moves each weight by the same 1e-3 except where |g| is within that noise of 0: the training loss before each step
    and the figures after are held to 2 % of the recorded DECREASE, two orders above what such weights can contribute and far below
    the decrease itself."""
    from tests.helpers_eval import loss_bound
    from video2music_amd import train
    name, cfg, sd, _ = case
    g = golden("g_train.npz")
    want_before, want_after, want_traj = g[f"{name}_figs_before"], g[f"{name}_figs_after"], g[f"{name}_adam_losses"]
    from video2music_amd import train_regression as TR
    assert tuple(g["adam"]) == (TR.ADAM_BETA_1, TR.ADAM_BETA_2, TR.ADAM_EPSILON)        # what make_optimizer hands to Adam
    m = build(cfg)
    data = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in
            dict(bt, chord=np.pad(bt["x"], ((0, 0), (0, 1))), chord_root=np.pad(bt["x_root"], ((0, 0), (0, 1))),
                 chord_attr=np.pad(bt["x_attr"], ((0, 0), (0, 1)))).items()}
    figs = lambda: np.array([train.evaluate(m, data, 1, T.S_VIDEO, T.SMOOTHING)[k] for k in T.FIGURES])
    before = figs()
    tol = np.array([2e-4, 2e-4, 1e-4]) + loss_bound(T.L_CHORD, want_before[:3] * T.L_CHORD) / T.L_CHORD
    print(f"{name}: before {before} recorded {want_before}")
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
        traj.append(float(loss))
    after = figs()
    print(f"  losses {traj} recorded {want_traj}\n  after {after} recorded {want_after}")
    assert (np.diff(traj) < 0).all() and (np.diff(want_traj) < 0).all() and after[0] < before[0] and want_after[0] < want_before[0]
    assert (np.abs(np.array(traj) - want_traj) <= 0.02 * (want_traj[0] - want_traj[-1])).all()
    assert (np.abs(after[:3] - want_after[:3]) <= 0.02 * np.abs(want_before[:3] - want_after[:3])).all()


def test_injected_masks_match_the_restatement(golden, case, bt):
    name, cfg, sd, _ = case
    e32 = float(golden("g_train.npz")[f"{name}_e32_grad"])
    p = 0.2
    masks = T.draw_masks(cfg, p, seed=11)
    l64, y64, g64 = T.grads(sd, cfg, bt, torch.float64, masks=T.Masks(masks, p))
    m = build(cfg, dropout=p).train()
    m.dropout_masks = [torch.from_numpy(a).to(DEV) for a in masks]
    y, loss = train_loss(m, bt)
    loss.backward()
    assert len(m.last_dropout_masks) == len(masks) == 2 + 10 * cfg["n_layers"]
    assert np.abs(y.detach().cpu().numpy() - y64).max() <= 1e-4
    for k, g in g64.items():
        if g is not None:
            assert T.rel_err(m.get_parameter(k).grad.cpu().numpy(), g) <= 8 * e32, k


def test_drawn_masks_are_repeatable_and_keep_at_the_right_rate(bt):
    cfg, p = T.MODELS["rpr"], 0.2
    m = build(cfg, dropout=p).train()
    torch.manual_seed(4)
    y1 = logits_of(m, bt)
    used = m.last_dropout_masks
    torch.manual_seed(4)
    y2 = logits_of(m, bt)
    assert torch.equal(y1, y2) and all(torch.equal(a, b) for a, b in zip(used, m.last_dropout_masks))
    want = T.draw_masks(cfg, p, seed=0)
    assert [tuple(a.shape) for a in used] == [a.shape for a in want] and [a.dtype == torch.uint8 for a in used] == [a.dtype == np.uint8 for a in want]
    for a in used:
        kept = float((a != 0).float().mean())
        assert abs(kept - (1 - p)) <= 4 * np.sqrt(p * (1 - p) / a.numel())
        assert a.dtype == torch.uint8 or set(torch.unique(a).tolist()) <= {0.0, float(np.float32(1.0) / np.float32(1 - p))}
    torch.manual_seed(5)
    assert not torch.equal(logits_of(m, bt), y1)


# ---- python -m video2music_amd.train on the miniature dataset ----

def test_cli_trains_two_epochs_and_its_last_row_is_what_evaluate_reports(golden, tmp_path, capsys):
    import csv
    import os
    from tests.helpers_features import write_mini_dataset
    from video2music_amd import evaluate, train
    g = golden("g_eval.npz")
    root = str(tmp_path / "vevo")
    os.makedirs(root)
    content = {k[3:]: g[k] for k in g if k.startswith("in_")}
    content["ids"] = [str(i) for i in g["ids"]]
    write_mini_dataset(root, content)
    ids = ",".join(content["ids"])
    model = ["-n_layers", "2", "-num_heads", "2", "-d_model", "64", "-dim_feedforward", "128", "-motion_type", "1"]
    out = str(tmp_path / "out")
    res = train.main(["-dataset_dir", root, "-output_dir", out, "-music_gen_version", "None", "-chord_embed", "", "-epochs", "2", "-batch_size", "2",
                      "-weight_modulus", "1", "-print_modulus", "1", "-ce_smoothing", "0", "-lr", "1e-3", "--train_ids", ids, "--val_ids", ids,
                      "--seed", "3"] + model)
    amt = os.path.join(out, "AMT")
    for name in ("model_params.txt", "results.csv", "best_loss_weights.pickle", "best_epochs.txt", "weights/epoch_0000.pickle",
                 "weights/epoch_0001.pickle", "weights/epoch_0002.pickle"):
        assert os.path.isfile(os.path.join(amt, name)), name
    rows = list(csv.reader(open(os.path.join(amt, "results.csv"))))
    assert rows[0] == train.CSV_HEADER and [r[0] for r in rows[1:]] == ["0", "1", "2"] and all(len(r) == 14 for r in rows)
    fig = np.array([[float(v) for v in r[2:]] for r in rows[1:]])
    assert np.isfinite(fig).all() and np.array_equal(fig[:, :6], fig[:, 6:])          # the same clips train and validate here
    assert fig[2, 0] < fig[0, 0]                                                       # two epochs of Adam lower the total loss
    assert res["best_epoch"] in (1, 2, 3) and "Train loss (total):" in capsys.readouterr().out
    best = torch.load(os.path.join(amt, "best_loss_weights.pickle"))
    cfg = dict(n_layers=2, num_heads=2, d_model=64, dim_feedforward=128, max_sequence_chord=300, total_vf_dim=best["Linear_vis.weight"].shape[1],
               rpr=True)
    VideoMusicTransformer(**cfg).load_state_dict(best, strict=True)

    # the last row's evaluation columns against `evaluate` on the saved epoch weights (ce_smoothing off: the definitions coincide)
    summary = evaluate.main(["-dataset_dir", root, "-output_dir", str(tmp_path / "ev"), "-music_gen_version", "None", "-batch_size", "2",
                             "--test_ids", ids, "-model_weights", os.path.join(amt, "weights", "epoch_0002.pickle")] + model)
    last = dict(zip(train.CSV_HEADER[8:], fig[2, 6:]))
    for col, key in (("Avg Eval h1", "avg_h1"), ("Avg Eval h3", "avg_h3"), ("Avg Eval h5", "avg_h5"), ("Avg Eval loss (emotion)", "avg_loss_emotion")):
        assert last[col] == summary[key], col
    from tests.helpers_eval import loss_bound
    assert abs(last["Avg Eval loss (chord)"] - summary["avg_loss_chord"]) <= loss_bound(299, summary["avg_loss_chord"])
