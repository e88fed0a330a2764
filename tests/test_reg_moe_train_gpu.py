"""Training of VideoRegression(moe_bimamba+ / sharedmoe_bimamba+) on the device against g_reg_moe_train*.npz (the reference's own
train_epoch on the CPU, every Dropout at p = 0) and the fp64 restatement of tests/helpers_moe_train.py, which
tests/test_reg_moe_train_host.py holds to that fixture; then `python -m video2music_amd.train_regression_moe` end to end on the
miniature dataset.  The plan is tests/test_reg_mamba_train_gpu.py's.

Bound of every gradient: rel_err(got, g64) <= max(8 e32, n U) with e32 the fixture's recorded noise level of fp32 training arithmetic,
U = 2^-24 and n = 600, the rows (both clips' frames) a weight gradient adds up -- the longest sum behind any of the values."""
import csv
import os

import numpy as np
import pytest
import torch

from tests import helpers_moe_train as T
from tests import helpers_reg_eval as HE
from video2music_amd import evaluate_regression, synthetic, train_regression as TR, train_regression_moe as TRX
from video2music_amd.losses import regression_train_loss
from video2music_amd.model.video_regression import VideoRegression

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 5e-5              # what g_reg.npz pins for these heads' outputs (tests/test_evaluate_regression_gpu.py)
NAMES = list(T.MODELS)
ROWS = 600


@pytest.fixture(scope="module")
def g(golden):
    return {**golden("g_reg_moe_train.npz"), **golden("g_reg_moe_train_64.npz")}


def state_dict_of(g, name):
    keys = [k[len(name) + 6:] for k in g if k.startswith(name + "_grad_")]
    return synthetic.synthetic_state_dict([(k, g[f"{name}_grad_{k}"].shape) for k in keys], seed=T.SEED)


def build(g, name, dropout=0.0, inner=0.0):
    """inner: the rate of the experts' own Dropout (the class default 0.1 when None)."""
    cfg = T.MODELS[name]
    m = VideoRegression(n_layers=cfg["n_layers"], d_model=cfg["d_model"], d_hidden=cfg["dim_feedforward"], dropout=dropout,
                        total_vf_dim=g["sem"].shape[2] + 6, regModel=cfg["regModel"])
    if inner is not None:
        for lyr in m.model.layers:
            for e in list(lyr.ffn.experts) + ([lyr.ffn.shared_expert] if lyr.ffn.shared else []):
                e.dropout.p = inner
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state_dict_of(g, name).items()}, strict=True)
    return m.to(DEV)


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
    return m.model.layers[0].ffn.last_routing[0].reshape(ROWS, T.TOP_K).cpu().numpy()


def bound(e32):
    return max(8 * e32, ROWS * T.U)


@pytest.mark.parametrize("name", NAMES)
def test_train_forward_equals_eval_forward_and_first_loss_and_gradients(g, name):
    m, b = build(g, name), batch(g)
    with torch.no_grad():
        e_ln, e_inst = m.eval()(b["sem"], None, None, b["emo"])
    m.train()
    ln_nd, inst = m(b["sem"], None, None, b["emo"])
    assert ln_nd.requires_grad and inst.requires_grad and m.last_dropout_masks == []
    assert torch.equal(ln_nd.detach(), e_ln) and torch.equal(inst.detach(), e_inst)               # every rate 0: bit for bit
    assert np.array_equal(routing_of(m), g[f"{name}_routing"])                                   # the reference's choices, every token
    o = oracle(g, name)
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
    opt = torch.optim.SGD(m.parameters(), lr=T.SGD_LR)
    for step in range(T.SGD_STEPS):
        opt.zero_grad()
        step_loss(m, b).backward()
        opt.step()
        assert np.array_equal(routing_of(m), routings[step][0]["idx"].numpy()), step           # the fixture tool pinned these to the reference's
        if step == 0:
            assert np.array_equal(routing_of(m), g[f"{name}_routing"])
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


@pytest.mark.parametrize("name", NAMES)
def test_injected_dropout_masks(g, name):
    """Model rate 0.2 and the experts' own 0.1: after in_proj, after the forward block, after the backward block, then the mixture
    layer's [inside the experts, on their outputs, inside the shared expert], then after the layer -- the given multipliers on the
    device and in the restatement."""
    p, p_inner = 0.2, 0.1
    cfg = T.MODELS[name]
    shapes = T.mask_shapes(name, cfg["n_layers"], ROWS, cfg["d_model"], p, p_inner)
    assert len(shapes) == (7 if name.startswith("shared") else 6)
    m, b = build(g, name, dropout=p, inner=None).train(), batch(g)
    assert m.model.layers[0].ffn.dropout_rates() == (p_inner, p, p_inner if name.startswith("shared") else 0.0)
    rng = np.random.default_rng(10)         # picked on the CPU: the masked forward's fp64 gate gap is 8e-4 (asserted below)
    rate = lambda s: p_inner if s[1] == 2 * cfg["d_model"] + 1 else p
    masks = [((rng.random(s) >= rate(s)) / (1 - rate(s))).astype(np.float32) for s in shapes]
    m.dropout_masks = [torch.from_numpy(k).to(DEV) for k in masks]
    step_loss(m, b).backward()
    assert len(m.last_dropout_masks) == len(shapes) and all(torch.equal(a, c) for a, c in zip(m.last_dropout_masks, m.dropout_masks))
    o = T.model_grads(state_dict_of(g, name), cfg["regModel"], cfg["n_layers"], *data_of(g), masks=masks)
    assert np.array_equal(routing_of(m), o["routing"][0]["idx"].numpy()) and T.gate_gap(o["routing"][0]["logits"], T.TOP_K) >= T.GAP
    e32 = float(g[f"{name}_e32_grad"])
    for k, v in grads_of(m).items():
        assert T.rel_err(v, o["grads"][k]) <= bound(e32), k
    assert abs(o["loss"] - oracle(g, name)["loss"]) > 1e-3          # the masks did something


def test_drawn_dropout_masks(g):
    """The reference's default construction: the experts keep their own 0.1 whatever the model's rate is."""
    name, p, p_inner = "sharedmoe_bimamba+", 0.2, 0.1
    cfg = T.MODELS[name]
    m, b = build(g, name, dropout=p, inner=None).train(), batch(g)
    runs = []
    for _ in range(2):
        torch.manual_seed(11)
        m.zero_grad()
        step_loss(m, b).backward()
        runs.append((grads_of(m), [k.clone() for k in m.last_dropout_masks]))
    assert all(np.array_equal(runs[0][0][k], runs[1][0][k]) for k in runs[0][0])
    shapes = T.mask_shapes(name, cfg["n_layers"], ROWS, cfg["d_model"], p, p_inner)
    assert len(runs[0][1]) == len(shapes) and all(torch.equal(a, c) for a, c in zip(runs[0][1], runs[1][1]))
    for mask, shape in zip(runs[0][1], shapes):
        assert tuple(mask.shape) == shape
        q = p_inner if shape[1] == 65 else p
        n = mask.numel()
        zeros = int((mask == 0).sum())
        assert abs(zeros - q * n) <= 5 * np.sqrt(n * q * (1 - q))                      # the kept share within the binomial 5 sigma
        assert torch.equal(mask[mask != 0], torch.full((n - zeros,), 1.0, device=DEV) / (1.0 - q))
    # the model's rate at 0: the experts' own sites alone
    m0 = build(g, name, dropout=0.0, inner=None).train()
    step_loss(m0, b).backward()
    assert [tuple(k.shape) for k in m0.last_dropout_masks] == [(2 * ROWS, 65), (ROWS, 65)]


@pytest.mark.parametrize("name", NAMES)
def test_an_optimiser_step_reaches_the_next_forward(g, name):
    """The stacked expert weights are keyed on the parameters' versions: after opt.step() the training and the inference forward both
    equal those of a fresh module that loaded the stepped state dict."""
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


def test_train_regression_moe_cli(tmp_path, capsys):
    """Two epochs of the default head ('sharedmoe_bimamba+') at the reference's default configuration on the miniature dataset; the
    split files are written here."""
    root, out = str(tmp_path / "data"), str(tmp_path / "out")
    c = HE.reg_dataset_content()
    HE.write_reg_dataset(root, c)
    for split in ("train", "val"):
        with open(os.path.join(root, "vevo_meta", "split", "v1", split + ".txt"), "w") as f:
            f.write("\n".join(c["ids"]) + "\n")
    res = TRX.main(["-dataset_dir", root, "-output_dir", out, "-epochs", "2", "-weight_modulus", "2", "-print_modulus", "1", "--seed", "5"])
    capsys.readouterr()
    d = os.path.join(out, "AMT")
    rm = "sharedmoe_bimamba+"
    for f in ("results_regression.csv", "best_rmse_weights.pickle", "best_epochs_regression.txt", "model_params_regression.txt",
              os.path.join("weights_regression_" + rm, "epoch_0002.pickle")):
        assert os.path.isfile(os.path.join(d, f)), f
    assert "regModel: " + rm in open(os.path.join(d, "model_params_regression.txt")).read()
    rows = list(csv.reader(open(os.path.join(d, "results_regression.csv"), newline="")))
    assert rows[0] == TR.CSV_HEADER and [r[0] for r in rows[1:]] == ["0", "1", "2"]
    assert res["best_epoch"] in (0, 1, 2) and min(float(r[6]) for r in rows[1:]) == res["best_val_total_loss"]
    m = VideoRegression(n_layers=2, d_model=64, d_hidden=256, dropout=0.2, total_vf_dim=30, regModel=rm)
    weights = os.path.join(d, "weights_regression_" + rm, "epoch_0002.pickle")
    m.load_state_dict(torch.load(weights, map_location="cpu"), strict=True)
    # the last epoch's weights through evaluate_regression: the validation figures of the last CSV row
    s = evaluate_regression.main(["-dataset_dir", root, "-output_dir", str(tmp_path / "eval_val"), "-batch_size", "32", "-regModel", rm,
                                  "-model_weights", weights, "--test_ids", "split:val"])
    printed = [float(ln.rsplit(":", 1)[1]) for ln in capsys.readouterr().out.strip().splitlines()[-4:]]
    assert printed == [s[k] for k in TR.FIGURE_KEYS] == [float(v) for v in rows[-1][6:10]]
