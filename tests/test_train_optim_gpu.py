"""Training under RAdam, RAdamW and RAdanW: the reference's recorded 8-step runs (tests/golden/g_train_optim.npz,
tools/make_goldens_train_optim.py) reproduced directly and through `python -m video2music_amd.train_optim`, and one epoch of
`train_regression_optim -optimizer RAdamW` on 'bimamba+'.

Bounds.  The losses: the rule tests/test_train_gpu.py applies to its recorded Adam run -- the training loss before each step within
2 % of the recorded decrease (first loss minus last).  RAdanW's recorded trajectory is not monotone (its difference term divides by
sqrt(exp_diff_sq), which is tiny when the term first acts at step 3: the loss jumps at step 4 and then falls below RAdamW's), so
monotony is asked of the two RAdam runs only, as recorded.  The final weights: theta_8 - theta_0 against the recorded fp32 run within
twice `<o>_spread`, the distance the reference's own fp32 run keeps from its fp64 run of the same 8 steps in the same measure
(max |difference| over max |update|, per tensor; rectified steps are sign-like where exp_avg_sq is small, so gradient noise around 0
becomes whole steps -- each fp32 run can sit one spread from fp64)."""
import csv
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import helpers_train as T
from tests.test_train_gpu import build, train_loss
from video2music_amd import optim, train, train_optim

pytestmark = pytest.mark.gpu
G = "g_train_optim.npz"
OPTIMIZERS = {"radam": "RAdam", "radamw": "RAdamW", "radanw": "RAdanW"}
MODEL = ["-n_layers", "2", "-num_heads", "2", "-d_model", "64", "-dim_feedforward", "128", "-motion_type", "0", "-dropout", "0"]


def check_run(g, name, losses, weights, sd):
    want = g[f"{name}_losses"]
    steps, spread = int(g["steps"]), float(g[f"{name}_spread"])
    drop = want[0] - want[-1]
    print(f"{name}: losses {losses}\n  recorded {want.tolist()}\n  |diff| / (0.02 decrease) {(np.abs(np.array(losses) - want) / (0.02 * drop)).tolist()}")
    assert len(losses) == steps and drop > 0
    assert (np.abs(np.array(losses) - want) <= 0.02 * drop).all()
    if name != "radanw":
        assert (np.diff(losses) < 0).all() and (np.diff(want) < 0).all()
    worst = 0.0
    for k in g["keys"]:
        k = str(k)
        rec = g[f"{name}_w_{k}"]
        part = (lambda a: a if a.size <= 4096 else a[:4])
        w0 = part(np.asarray(sd[k], dtype=np.float64))
        got = part(weights[k].detach().cpu().numpy().astype(np.float64))
        assert got.shape == rec.shape, k
        err = T.rel_err(got - w0, rec.astype(np.float64) - w0)
        worst = max(worst, err / spread)
        assert err <= 2 * spread, (name, k, err, spread)
    print(f"  worst update error / recorded fp32-vs-fp64 spread = {worst:.3f} (allowed 2)")


@pytest.mark.parametrize("name", list(OPTIMIZERS))
def test_eight_steps_follow_the_recorded_reference_run(golden, name):
    g = golden(G)
    cfg = T.MODELS["rpr"]
    sd, bt = T.state_dict(cfg), T.batch()
    m = build(cfg)
    opt = train.make_chord_optimizer(SimpleNamespace(optimizer=OPTIMIZERS[name]), m.parameters(), float(g["lr"]))
    assert isinstance(opt, (optim.RAdam, optim.RAdanW))
    assert tuple(g["settings"][:3]) == opt.defaults["betas"][:2] + (opt.defaults["eps"],)
    losses = []
    for _ in range(int(g["steps"])):
        opt.zero_grad()
        loss = train_loss(m.train(), bt)[1]
        loss.backward()
        opt.step()
        assert opt.last_step_launches >= 1
        losses.append(float(loss.detach()))
    check_run(g, name, losses, dict(m.named_parameters()), sd)


@pytest.mark.parametrize("name", list(OPTIMIZERS))
def test_cli_follows_the_recorded_reference_run(golden, tmp_path, capsys, name):
    g = golden(G)
    root, out = str(tmp_path / "vevo"), str(tmp_path / "out")
    os.makedirs(root)
    ids = ",".join(T.write_dataset(root))
    steps = int(g["steps"])
    res = train_optim.main(["-dataset_dir", root, "-output_dir", out, "-music_gen_version", "None", "-chord_embed", "", "-epochs", str(steps),
                            "-batch_size", "2", "-weight_modulus", str(steps), "-print_modulus", "1", "-lr", str(float(g["lr"])), "--train_ids", ids,
                            "--val_ids", ids, "--seed", "0", "--synthetic_weights", "-optimizer", OPTIMIZERS[name]] + MODEL)
    printed = capsys.readouterr().out
    losses = [float(x) for x in re.findall(r"Train loss \(total\): (\S+)", printed)]
    amt = os.path.join(out, "AMT")
    assert f"optimizer: {OPTIMIZERS[name]}" in open(os.path.join(amt, "model_params.txt")).read()
    rows = list(csv.reader(open(os.path.join(amt, "results.csv"))))
    assert rows[0] == train.CSV_HEADER and [r[0] for r in rows[1:]] == [str(e) for e in range(steps + 1)] and res["best_epoch"] >= 1
    weights = torch.load(train.epoch_weights_path(os.path.join(amt, "weights"), steps))
    check_run(g, name, losses, weights, T.state_dict(T.MODELS["rpr"]))


def test_train_regression_optim_radamw_one_epoch_of_bimamba_plus(tmp_path, capsys):
    from tests import helpers_reg_eval as HE
    from video2music_amd import train_regression as TR, train_regression_optim
    from video2music_amd.model.video_regression import VideoRegression
    root, out = str(tmp_path / "data"), str(tmp_path / "out")
    c = HE.reg_dataset_content()
    HE.write_reg_dataset(root, c)
    for split in ("train", "val"):
        with open(os.path.join(root, "vevo_meta", "split", "v1", split + ".txt"), "w") as f:
            f.write("\n".join(c["ids"]) + "\n")
    res = train_regression_optim.main(["-dataset_dir", root, "-output_dir", out, "-epochs", "1", "-weight_modulus", "1", "-print_modulus", "1",
                                       "--seed", "5", "-regModel", "bimamba+", "-optimizer", "RAdamW", "-lr", "1e-3"])
    assert "Train loss:" in capsys.readouterr().out
    d = os.path.join(out, "AMT")
    for f in ("results_regression.csv", "best_rmse_weights.pickle", "best_epochs_regression.txt", "model_params_regression.txt",
              os.path.join("weights_regression_bimamba+", "epoch_0000.pickle"), os.path.join("weights_regression_bimamba+", "epoch_0001.pickle")):
        assert os.path.isfile(os.path.join(d, f)), f
    rows = list(csv.reader(open(os.path.join(d, "results_regression.csv"), newline="")))
    assert rows[0] == TR.CSV_HEADER and [r[0] for r in rows[1:]] == ["0", "1"] and res["best_epoch"] in (0, 1)
    fig = np.array([[float(v) for v in r[2:]] for r in rows[1:]])
    assert np.isfinite(fig).all() and not np.array_equal(fig[0], fig[1])                # the step moved the weights the next evaluation read
    m = VideoRegression(n_layers=2, d_model=64, d_hidden=256, dropout=0.2, total_vf_dim=30, regModel="bimamba+")
    m.load_state_dict(torch.load(os.path.join(d, "weights_regression_bimamba+", "epoch_0001.pickle"), map_location="cpu"), strict=True)
