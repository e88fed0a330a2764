"""Regression training, host side: the fp64 numpy restatement of tests/helpers_reg_train.py against what the reference recorded in
g_reg_train.npz (so that the GPU tests judge the kernels by an oracle that is itself pinned), the parser's defaults, the learn-rate
schedule, the refusals and the file names of `python -m video2music_amd.train_regression`."""
import json

import numpy as np
import pytest

from tests import helpers_reg_train as T
from video2music_amd import synthetic, train_regression as TR
from video2music_amd.utilities.argument_reg_funcs import parse_train_args

FULL64 = ("lstm", "gru")          # the models whose fp64 gradients and updates are recorded in full


def state_dict_of(g, name):
    """The procedural weights the generator loaded: the recorded gradient keys carry the reference's key order and shapes."""
    keys = [k[len(name) + 6:] for k in g if k.startswith(name + "_grad_")]
    return {k: v for k, v in synthetic.synthetic_state_dict([(k, g[f"{name}_grad_{k}"].shape) for k in keys], seed=0).items()}


def batch_of(g):
    return g["sem"], g["emo"], g["note_density"], g["loudness"], g["instrument"]


@pytest.mark.parametrize("name", list(T.MODELS))
def test_restatement_equals_the_reference_gradients(golden, name):
    g = golden("g_reg_train.npz")
    cfg, sd = T.MODELS[name], state_dict_of(g, name)
    r = T.model_grads64(sd, cfg["regModel"], cfg["n_layers"], *batch_of(g))
    assert abs(r["loss"] - float(g[f"{name}_loss64"])) <= 1e-12 * abs(r["loss"])
    assert abs(r["loss"] - float(g[f"{name}_loss"])) <= 16 * T.U * abs(r["loss"])         # the reference's fp32 loss: a mean of fp32 terms
    e32 = float(g[f"{name}_e32_grad"])
    assert set(r["grads"]) == set(sd)
    for k in sd:
        assert T.rel_err(g[f"{name}_grad_{k}"], r["grads"][k]) <= e32 * (1 + 1e-6), k       # the reference's fp32 figures, at their noise level
        if name in FULL64:
            assert T.rel_err(r["grads"][k], g[f"{name}_grad64_{k}"]) <= 1e-11, k           # torch's fp64 autograd on the same stack


@pytest.mark.parametrize("name", FULL64)
def test_restatement_equals_the_reference_updates(golden, name):
    g = golden("g_reg_train.npz")
    cfg, sd = T.MODELS[name], state_dict_of(g, name)
    upd = T.sgd_updates64(sd, T.SGD_STEPS, T.SGD_LR, cfg["regModel"], cfg["n_layers"], *batch_of(g))
    e32 = float(g[f"{name}_e32_upd"])
    for k in sd:
        assert T.rel_err(upd[k], g[f"{name}_upd64_{k}"]) <= 1e-10, k
        assert T.rel_err(g[f"{name}_upd_{k}"], upd[k]) <= e32 * (1 + 1e-6), k


def test_loss_restatement_saturated_probabilities_and_the_smooth_l1_knee():
    """p = 0 / 1 (in fp32) against either target: the term is exactly 100 or 0 and the logit gradient exactly 0; |e| on both sides of
    1 and at it."""
    p = np.full((2, 40), 0.5)
    t = np.zeros((2, 40))
    p[0, :4], t[0, :4] = (0.0, 0.0, 1.0, 1.0), (0.0, 1.0, 0.0, 1.0)
    r = T.loss64(np.array([[1.5, -2.0], [0.75, 1.0]]), p, np.zeros(2), np.zeros(2), t)
    assert r["bce"][0, :4].tolist() == [0.0, 100.0, 100.0, 0.0] and not r["d_logit"][0, :4].any()
    assert np.allclose(r["bce"][1], np.log(2.0)) and np.allclose(r["d_logit"][1], 0.5 / 80)
    assert r["sl1"].tolist() == [[1.0, 1.5], [0.5 * 0.75 ** 2, 0.5]]
    assert (r["d_ln_nd"] * 4).tolist() == [[1.0, -1.0], [0.75, 1.0]]


def test_parser_defaults_equal_the_reference(golden):
    ref = json.loads(str(golden("g_reg_train.npz")["train_arg_defaults"]))
    mine = vars(parse_train_args([])[0])
    assert set(ref) <= set(mine)
    assert {k: mine[k] for k in ref} == ref
    assert (mine["regModel"], mine["d_model"], mine["dim_feedforward"], mine["n_layers"], mine["dropout"], mine["batch_size"], mine["epochs"],
            mine["lr"], mine["optimizer"], mine["weight_modulus"]) == ("bilstm", 64, 256, 2, 0.2, 32, 50, None, "Adam", 10)


def test_schedule_equals_the_reference(golden):
    g = golden("g_reg_train.npz")
    d, warm = int(g["schedule_d_model"]), int(g["schedule_warmup"])
    assert (TR.LR_DEFAULT_START, TR.SCHEDULER_WARMUP_STEPS) == (1.0, warm)
    assert [TR.ADAM_BETA_1, TR.ADAM_BETA_2, TR.ADAM_EPSILON] == g["adam"].tolist()
    plain, cont = TR.LrStepTracker(d, warm, 0), TR.LrStepTracker(d, warm, T.SCHEDULE_CONTINUE[0] * T.SCHEDULE_CONTINUE[1])
    for i, s in enumerate(T.SCHEDULE_STEPS):
        assert plain.step(s) == g["schedule"][i] and cont.step(s) == g["schedule_continued"][i]
        assert abs(T.schedule(s, d, warm) - g["schedule"][i]) <= 1e-15 * g["schedule"][i]
    assert np.argmax(g["schedule"]) == T.SCHEDULE_STEPS.index(4000)


@pytest.mark.parametrize("argv,reason", [
    (["--force_cpu", "1"], "no CPU path"), (["-is_video", ""], "-is_video False is not built"), (["-use_KAN", "1"], "KANLinear"),
    (["-augmentation", "1"], "-augmentation is not built"), (["--no_tensorboard", ""], "tensorboard reporting is not built"),
    (["-optimizer", "RAdam"], "RAdam file is not ported"), (["-optimizer", "RAdamW"], "RAdam file is not ported"),
    (["-continue_epoch", "3"], "go together")] +
    [(["-regModel", rm], "backward pass is built for the recurrent heads")
     for rm in ("mamba", "mamba+", "bimamba", "bimamba+", "moemamba", "moe_bimamba+", "sharedmoe_bimamba+", "cnngru", "cnnbigru")])
def test_cli_refuses_what_is_not_built(argv, reason):
    with pytest.raises(SystemExit) as e:
        TR.main(argv)
    assert reason in str(e.value)


def test_file_names_and_csv_header(tmp_path):
    assert TR.CSV_HEADER == ["Epoch", "Learn rate", "Avg Train Total loss", "Avg Train RMSE (Note Density)", "Avg Train RMSE (Loudness)",
                             "Avg Train BCE (Instrument)", "Avg Eval Total loss", "Avg Eval RMSE (Note Density)", "Avg Eval RMSE (Loudness)",
                             "Avg Eval BCE (Instrument)"]
    args = parse_train_args([])[0]
    TR.write_model_params(args, tmp_path / "model_params_regression.txt")
    lines = (tmp_path / "model_params_regression.txt").read_text().splitlines()
    assert lines[0] == "lr: None" and "regModel: bilstm" in lines and "dropout: 0.2" in lines and "n_epochs: 50" in lines
