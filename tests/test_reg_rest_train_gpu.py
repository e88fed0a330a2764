"""Training of VideoRegression(mamba / mamba+ / moemamba / cnngru / cnnbigru) after `enable_training()` on the device against
g_reg_rest_train*.npz (the reference's own train_epoch on the CPU, every Dropout at p = 0) and the fp64 restatement of
tests/helpers_reg_rest_train.py, which tests/test_reg_rest_train_host.py holds to that fixture; then
`python -m video2music_amd.train_regression_all` end to end on the miniature dataset.  The plan is tests/test_reg_mamba_train_gpu.py's.

Bound of every gradient and of every update: rel_err(got, g64) <= 8 e32 with e32 the fixture's recorded noise level of fp32 training
arithmetic (`_e32_grad`, `_e32_upd`), as in tests/test_reg_mamba_train_gpu.py; no floor."""
import csv
import os

import numpy as np
import pytest
import torch

from tests import helpers_reg_eval as HE
from tests import helpers_reg_rest_train as T
from video2music_amd import evaluate_regression, synthetic, train_regression as TR, train_regression_all as TRA
from video2music_amd.losses import regression_train_loss
from video2music_amd.model.video_regression import VideoRegression

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 5e-5              # what g_reg.npz pins for these heads' outputs (tests/test_evaluate_regression_gpu.py)
NAMES = list(T.MODELS)
ROWS = 600


@pytest.fixture(scope="module")
def g(golden):
    return {**golden("g_reg_rest_train.npz"), **golden("g_reg_rest_train_b.npz"), **golden("g_reg_rest_train_64.npz")}


def state_dict_of(g, name):
    keys = [k[len(name) + 6:] for k in g if k.startswith(name + "_grad_")]
    return synthetic.synthetic_state_dict([(k, g[f"{name}_grad_{k}"].shape) for k in keys], seed=T.SEEDS[name])


def moe_layers(m):
    return [lyr[1].moe_layer for lyr in m.model.layers] if m.regModel == "moemamba" else []


def build(g, name, dropout=0.0, inner=0.0, opt_in=True):
    """inner: the rate of the experts' own Dropout (the class default 0.1 when None)."""
    cfg = T.MODELS[name]
    m = VideoRegression(n_layers=cfg["n_layers"], d_model=cfg["d_model"], d_hidden=cfg["dim_feedforward"], dropout=dropout,
                        total_vf_dim=g["sem"].shape[2] + 6, regModel=cfg["regModel"])
    if inner is not None:
        for layer in moe_layers(m):
            for e in list(layer.experts) + [layer.shared_expert]:
                e.dropout.p = inner
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state_dict_of(g, name).items()}, strict=True)
    m = m.to(DEV)
    if opt_in:
        assert m.enable_training() is m and m._training_enabled
    return m


def batch(g):
    return {k: torch.from_numpy(g[k]).to(DEV) for k in ("sem", "emo", "note_density", "loudness", "instrument")}


def data_of(g):
    return g["sem"], g["emo"], g["note_density"], g["loudness"], g["instrument"]


def step_loss(m, b):
    ln_nd, inst = m(b["sem"], None, None, b["emo"])
    return regression_train_loss(ln_nd, inst, b["note_density"], b["loudness"], b["instrument"])


_ORACLE = {}


def oracle(g, name):
    """fp64 loss / gradients of the restatement with every dropout rate 0 (computed once per model)."""
    if name not in _ORACLE:
        cfg = T.MODELS[name]
        _ORACLE[name] = T.model_grads(state_dict_of(g, name), cfg["regModel"], cfg["n_layers"], *data_of(g))
    return _ORACLE[name]


def grads_of(m):
    return {k: p.grad.detach().cpu().numpy().astype(np.float64) for k, p in m.named_parameters()}


def routing_of(m):
    return [layer.last_routing[0].reshape(ROWS, T.TOP_K).cpu().numpy() for layer in moe_layers(m)]


def same_routing(m, routing):
    return all(np.array_equal(a, r["idx"].numpy()) for a, r in zip(routing_of(m), routing)) and len(routing) == len(moe_layers(m))


def bound(e32):
    return 8 * e32


@pytest.mark.parametrize("name", NAMES)
def test_train_forward_equals_eval_forward_and_first_loss_and_gradients(g, name):
    m, b = build(g, name), batch(g)
    with torch.no_grad():
        e_ln, e_inst = m.eval()(b["sem"], None, None, b["emo"])
    m.train()
    ln_nd, inst = m(b["sem"], None, None, b["emo"])
    assert ln_nd.requires_grad and inst.requires_grad and m.last_dropout_masks == []
    assert torch.equal(ln_nd.detach(), e_ln) and torch.equal(inst.detach(), e_inst)               # every rate 0: bit for bit
    o = oracle(g, name)
    assert same_routing(m, o["routing"]) and T.min_gap([o["routing"]]) >= T.GAP
    loss = regression_train_loss(ln_nd, inst, b["note_density"], b["loudness"], b["instrument"])
    inv_sharp = float((1.0 / np.minimum(o["p"], 1 - o["p"])).mean())
    print(name, "loss", float(loss.detach()), "reference", float(g[f"{name}_loss"]), "tolerance", TOL * (1 + inv_sharp))
    assert abs(float(loss.detach()) - float(g[f"{name}_loss"])) <= TOL * (1 + inv_sharp)        # SmoothL1's slope <= 1; a BCE term moves by dp / min(p, 1 - p)
    loss.backward()
    e32 = float(g[f"{name}_e32_grad"])
    got = grads_of(m)
    assert set(got) == set(o["grads"])
    errs = {}
    for k, v in got.items():
        want = g[f"{name}_grad64_{k}"] if f"{name}_grad64_{k}" in g else o["grads"][k]
        errs[k] = T.rel_err(v, want) / bound(e32)
        assert T.rel_err(v, g[f"{name}_grad_{k}"]) <= 1.01 * (bound(e32) + e32), ("reference fp32", k)     # the reference's own figures: its e32 further
    worst = max(errs, key=errs.get)
    print(name, "worst gradient err / bound =", round(errs[worst], 3), "at", worst, "bound", bound(e32))
    assert errs[worst] <= 1, {k: round(v, 2) for k, v in errs.items() if v > 1}
    # and the same bits twice
    m.zero_grad()
    step_loss(m, b).backward()
    assert all(np.array_equal(v, got[k]) for k, v in grads_of(m).items())


@pytest.mark.parametrize("name", NAMES)
def test_three_sgd_steps(g, name):
    cfg, m, b = T.MODELS[name], build(g, name).train(), batch(g)
    sd0 = state_dict_of(g, name)
    routings = []
    want = T.sgd_updates(sd0, T.SGD_STEPS, T.SGD_LR, cfg["regModel"], cfg["n_layers"], *data_of(g), routings=routings)
    assert T.min_gap(routings) >= T.GAP
    opt = torch.optim.SGD(m.parameters(), lr=T.SGD_LR)
    for step in range(T.SGD_STEPS):
        opt.zero_grad()
        step_loss(m, b).backward()
        opt.step()
        assert same_routing(m, routings[step]), step
    e32 = float(g[f"{name}_e32_upd"])
    worst = 0.0
    for k, p in m.named_parameters():
        err = T.rel_err(p.detach().cpu().numpy().astype(np.float64) - sd0[k].astype(np.float64), want[k])
        worst = max(worst, err / bound(e32))
        assert err <= bound(e32), (k, err, e32)
    print(name, "worst update err / bound =", round(worst, 3))


@pytest.mark.parametrize("name", NAMES)
def test_three_adam_steps_lower_the_validation_loss_as_the_reference_does(g, name):
    m, b = build(g, name), batch(g)
    data = {"semantic": b["sem"], "scene_offset": b["sem"][..., 0], "motion": b["sem"][..., 0], "emotion": b["emo"],
            "note_density": b["note_density"], "loudness": b["loudness"], "instrument": b["instrument"]}
    before = TR.evaluate(m, data, 1)
    o = oracle(g, name)                                                               # the same starting point, at the evaluation tests' bound
    bce = TOL * float((1.0 / np.minimum(o["p"], 1 - o["p"])).mean(axis=(1, 2)).max())
    assert (np.abs(np.array(before) - g[f"{name}_figs_before"]) <= np.array([TOL + bce, TOL, TOL, bce])).all()
    opt = torch.optim.Adam(m.parameters(), lr=T.ADAM_LR, betas=(TR.ADAM_BETA_1, TR.ADAM_BETA_2), eps=TR.ADAM_EPSILON)
    m.train()
    for _ in range(T.ADAM_STEPS):
        opt.zero_grad()
        step_loss(m, b).backward()
        opt.step()
    after = TR.evaluate(m, data, 1)
    print(name, "total loss", before[0], "->", after[0], "reference", g[f"{name}_figs_before"][0], "->", g[f"{name}_figs_after"][0])
    assert g[f"{name}_figs_after"][0] < g[f"{name}_figs_before"][0] and after[0] < before[0]


MASK_SEEDS = {name: 10 for name in NAMES}       # picked on the CPU: the masked forward's fp64 gate gaps hold (asserted below)


@pytest.mark.parametrize("name", NAMES)
def test_injected_dropout_masks(g, name):
    """Model rate 0.2 and the experts' own 0.1, the sites of `helpers_reg_rest_train.mask_shapes`: the given multipliers on the device
    and in the restatement."""
    p, p_inner = 0.2, 0.1
    cfg = T.MODELS[name]
    L = cfg["n_layers"]
    shapes = T.mask_shapes(cfg["regModel"], L, ROWS, cfg["d_model"], p, p_inner)
    assert len(shapes) == {"mamba": 1, "mamba+": 1, "moemamba": 1 + 3 * L, "cnngru": 1 + L, "cnnbigru": 1 + L}[cfg["regModel"]]
    m, b = build(g, name, dropout=p, inner=None).train(), batch(g)
    rng = np.random.default_rng(MASK_SEEDS[name])
    rate = lambda s: p_inner if s[1] == 2 * cfg["d_model"] + 1 else p
    masks = [((rng.random(s) >= rate(s)) / (1 - rate(s))).astype(np.float32) for s in shapes]
    m.dropout_masks = [torch.from_numpy(k).to(DEV) for k in masks]
    step_loss(m, b).backward()
    assert len(m.last_dropout_masks) == len(shapes) and all(torch.equal(a, c) for a, c in zip(m.last_dropout_masks, m.dropout_masks))
    o = T.model_grads(state_dict_of(g, name), cfg["regModel"], L, *data_of(g), masks=masks)
    assert T.min_gap([o["routing"]]) >= T.GAP and same_routing(m, o["routing"])
    e32 = float(g[f"{name}_e32_grad"])
    for k, v in grads_of(m).items():
        assert T.rel_err(v, o["grads"][k]) <= bound(e32), k
    assert abs(o["loss"] - oracle(g, name)["loss"]) > 1e-3          # the masks did something


@pytest.mark.parametrize("name", ["mamba+", "moemamba", "cnngru"])
def test_drawn_dropout_masks(g, name):
    p, p_inner = 0.2, 0.1
    cfg = T.MODELS[name]
    m, b = build(g, name, dropout=p, inner=None).train(), batch(g)
    runs = []
    for _ in range(2):
        torch.manual_seed(11)
        m.zero_grad()
        step_loss(m, b).backward()
        runs.append((grads_of(m), [k.clone() for k in m.last_dropout_masks]))
    assert all(np.array_equal(runs[0][0][k], runs[1][0][k]) for k in runs[0][0])
    shapes = T.mask_shapes(cfg["regModel"], cfg["n_layers"], ROWS, cfg["d_model"], p, p_inner)
    assert len(runs[0][1]) == len(shapes) and all(torch.equal(a, c) for a, c in zip(runs[0][1], runs[1][1]))
    for mask, shape in zip(runs[0][1], shapes):
        assert tuple(mask.shape) == shape
        q = p_inner if shape[1] == 65 else p
        n = mask.numel()
        zeros = int((mask == 0).sum())
        assert abs(zeros - q * n) <= 5 * np.sqrt(n * q * (1 - q))                      # the kept share within the binomial 5 sigma
        assert torch.equal(mask[mask != 0], torch.full((n - zeros,), 1.0, device=DEV) / (1.0 - q))


@pytest.mark.parametrize("name", NAMES)
def test_an_optimiser_step_reaches_the_next_forward(g, name):
    m, b = build(g, name).train(), batch(g)
    opt = torch.optim.SGD(m.parameters(), lr=0.5)
    with torch.no_grad():
        old = m.eval()(b["sem"], None, None, b["emo"])[0].clone()          # fills the caches
    m.train()
    step_loss(m, b).backward()
    opt.step()
    fresh = build(g, name)
    fresh.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()})
    with torch.no_grad():
        want = fresh.eval()(b["sem"], None, None, b["emo"])
        got_eval = m.eval()(b["sem"], None, None, b["emo"])
    got_train = m.train()(b["sem"], None, None, b["emo"])
    assert not torch.equal(want[0], old)
    for a, c, t in zip(want, got_eval, got_train):
        assert torch.equal(a, c) and torch.equal(a, t.detach())


@pytest.mark.parametrize("name", ["mamba", "mamba+", "moemamba", "cnngru", "cnnbigru"])
def test_without_the_opt_in_the_training_state_builds_no_graph(g, name):
    """The default of before: a module that never called enable_training() runs the inference kernels in every state."""
    m, b = build(g, name, opt_in=False), batch(g)
    assert not m._training_enabled and not m.train()._train_path()
    ln_nd, inst = m(b["sem"], None, None, b["emo"])
    assert not ln_nd.requires_grad and not inst.requires_grad
    with torch.no_grad():
        e_ln, e_inst = m.eval()(b["sem"], None, None, b["emo"])
    assert torch.equal(ln_nd, e_ln) and torch.equal(inst, e_inst)
    on = build(g, name)
    assert on.train()._train_path() and not on.eval()._train_path()
    with torch.no_grad():
        assert not on.train()._train_path()


@pytest.mark.parametrize("rm", ["moemamba", "cnnbigru"])
def test_train_regression_all_cli(tmp_path, capsys, rm):
    """Two epochs at the parser's defaults (moemamba: d 64, 256 states per channel, S = 300) on the miniature dataset; the split files
    are written here."""
    root, out = str(tmp_path / "data"), str(tmp_path / "out")
    c = HE.reg_dataset_content()
    HE.write_reg_dataset(root, c)
    for split in ("train", "val"):
        with open(os.path.join(root, "vevo_meta", "split", "v1", split + ".txt"), "w") as f:
            f.write("\n".join(c["ids"]) + "\n")
    res = TRA.main(["-dataset_dir", root, "-output_dir", out, "-epochs", "2", "-weight_modulus", "2", "-print_modulus", "1", "--seed", "5",
                    "-regModel", rm])
    capsys.readouterr()
    d = os.path.join(out, "AMT")
    for f in ("results_regression.csv", "best_rmse_weights.pickle", "best_epochs_regression.txt", "model_params_regression.txt",
              os.path.join("weights_regression_" + rm, "epoch_0002.pickle")):
        assert os.path.isfile(os.path.join(d, f)), f
    assert "regModel: " + rm in open(os.path.join(d, "model_params_regression.txt")).read()
    rows = list(csv.reader(open(os.path.join(d, "results_regression.csv"), newline="")))
    assert rows[0] == TR.CSV_HEADER and [r[0] for r in rows[1:]] == ["0", "1", "2"]
    assert res["best_epoch"] in (0, 1, 2) and min(float(r[6]) for r in rows[1:]) == res["best_val_total_loss"]
    assert rows[1][2:] != rows[3][2:]                                       # two epochs of training moved the figures
    weights = os.path.join(d, "weights_regression_" + rm, "epoch_0002.pickle")
    # the last epoch's weights through evaluate_regression: the validation figures of the last CSV row
    s = evaluate_regression.main(["-dataset_dir", root, "-output_dir", str(tmp_path / "eval_val"), "-batch_size", "32", "-regModel", rm,
                                  "-model_weights", weights, "--test_ids", "split:val"])
    printed = [float(ln.rsplit(":", 1)[1]) for ln in capsys.readouterr().out.strip().splitlines()[-4:]]
    assert printed == [s[k] for k in TR.FIGURE_KEYS] == [float(v) for v in rows[-1][6:10]]
