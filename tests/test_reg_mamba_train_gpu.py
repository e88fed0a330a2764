"""Training of VideoRegression(bimamba+ / bimamba) on the device against g_reg_mamba_train*.npz (the reference's own train_epoch on
the CPU) and the fp64 restatement of tests/helpers_reg_mamba_train.py, which tests/test_reg_mamba_train_host.py holds to that
fixture; then `python -m video2music_amd.train_regression_mamba` end to end on the miniature dataset."""
import csv
import os

import numpy as np
import pytest
import torch

from tests import helpers_reg_eval as HE
from tests import helpers_reg_mamba_train as T
from video2music_amd import evaluate_regression, synthetic, train_regression as TR, train_regression_mamba as TRM
from video2music_amd.losses import regression_train_loss
from video2music_amd.model.video_regression import VideoRegression

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 5e-5              # what g_reg.npz pins for these heads' outputs (tests/test_evaluate_regression_gpu.py)
NAMES = list(T.MODELS)


@pytest.fixture(scope="module")
def g(golden):
    return {**golden("g_reg_mamba_train.npz"), **golden("g_reg_mamba_train_64.npz")}


def state_dict_of(g, name):
    keys = [k[len(name) + 6:] for k in g if k.startswith(name + "_grad_")]
    return synthetic.synthetic_state_dict([(k, g[f"{name}_grad_{k}"].shape) for k in keys], seed=0)


def build(g, name, dropout=0.0):
    cfg = T.MODELS[name]
    m = VideoRegression(n_layers=cfg["n_layers"], d_model=cfg["d_model"], d_hidden=cfg["dim_feedforward"], dropout=dropout,
                        total_vf_dim=g["sem"].shape[2] + 6, regModel=cfg["regModel"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state_dict_of(g, name).items()}, strict=True)
    return m.to(DEV)


def batch(g):
    return {k: torch.from_numpy(g[k]).to(DEV) for k in ("sem", "emo", "note_density", "loudness", "instrument")}


def data_of(g):
    return g["sem"], g["emo"], g["note_density"], g["loudness"], g["instrument"]


def step_loss(m, b, fused=True):
    ln_nd, inst = m(b["sem"], None, None, b["emo"])
    if fused:
        return regression_train_loss(ln_nd, inst, b["note_density"], b["loudness"], b["instrument"])
    tgt = torch.stack([b["note_density"].reshape(-1), b["loudness"].reshape(-1)], dim=1)          # train_epoch's own lines
    return torch.nn.SmoothL1Loss()(ln_nd.reshape(-1, 2), tgt) + torch.nn.functional.binary_cross_entropy(inst, b["instrument"])


_ORACLE = {}


def oracle(g, name):
    """fp64 loss / gradients of the restatement at dropout 0 (computed once per model)."""
    if name not in _ORACLE:
        cfg = T.MODELS[name]
        _ORACLE[name] = T.model_grads(state_dict_of(g, name), cfg["regModel"], cfg["n_layers"], *data_of(g))
    return _ORACLE[name]


def grads_of(m):
    return {k: p.grad.detach().cpu().numpy().astype(np.float64) for k, p in m.named_parameters()}


@pytest.mark.parametrize("name", NAMES)
def test_train_forward_equals_eval_forward_and_first_loss_and_gradients(g, name):
    m, b = build(g, name), batch(g)
    with torch.no_grad():
        e_ln, e_inst = m.eval()(b["sem"], None, None, b["emo"])
    m.train()
    ln_nd, inst = m(b["sem"], None, None, b["emo"])
    assert ln_nd.requires_grad and inst.requires_grad
    assert torch.equal(ln_nd.detach(), e_ln) and torch.equal(inst.detach(), e_inst)               # dropout 0: bit for bit
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
        errs[k] = T.rel_err(v, want) / e32
    worst = max(errs, key=errs.get)
    print(name, "worst gradient err / e32_grad =", round(errs[worst], 3), "at", worst)
    assert errs[worst] <= 8, {k: round(v, 2) for k, v in errs.items() if v > 8}
    # the reference's unchanged pattern: torch's own loss expressions on the model's outputs
    m.zero_grad()
    step_loss(m, b, fused=False).backward()
    for k, v in grads_of(m).items():
        assert T.rel_err(v, o["grads"][k]) <= 8 * e32, ("torch loss", k)
    # and the same bits twice
    m.zero_grad()
    step_loss(m, b).backward()
    assert all(np.array_equal(v, got[k]) for k, v in grads_of(m).items())


@pytest.mark.parametrize("name", NAMES)
def test_three_sgd_steps(g, name):
    cfg, m, b = T.MODELS[name], build(g, name).train(), batch(g)
    sd0 = state_dict_of(g, name)
    opt = torch.optim.SGD(m.parameters(), lr=T.SGD_LR)
    for _ in range(T.SGD_STEPS):
        opt.zero_grad()
        step_loss(m, b).backward()
        opt.step()
    want = T.sgd_updates(sd0, T.SGD_STEPS, T.SGD_LR, cfg["regModel"], cfg["n_layers"], *data_of(g))
    e32 = float(g[f"{name}_e32_upd"])
    worst = 0.0
    for k, p in m.named_parameters():
        err = T.rel_err(p.detach().cpu().numpy().astype(np.float64) - sd0[k].astype(np.float64), want[k])
        worst = max(worst, err / e32)
        assert err <= 8 * e32, (k, err, e32)
    print(name, "worst update err / e32_upd =", round(worst, 3))


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


def test_injected_dropout_masks(g):
    """p = 0.2 on 'bimamba+': after in_proj, then per layer after the forward block, after the backward block, inside the FFN and
    after it -- the given multipliers on the device and in the restatement."""
    name, p = "bimamba+", 0.2
    cfg = T.MODELS[name]
    widths = T.mask_widths(name, cfg["n_layers"], cfg["d_model"], cfg["dim_feedforward"])
    assert widths == [32, 32, 32, 64, 32, 32, 32, 64, 32]
    m, b = build(g, name, dropout=p).train(), batch(g)
    rng = np.random.default_rng(3)
    masks = [((rng.random((600, w)) >= p) / (1 - p)).astype(np.float32) for w in widths]
    m.dropout_masks = [torch.from_numpy(k).to(DEV) for k in masks]
    step_loss(m, b).backward()
    assert len(m.last_dropout_masks) == 9 and all(torch.equal(a, c) for a, c in zip(m.last_dropout_masks, m.dropout_masks))
    o = T.model_grads(state_dict_of(g, name), cfg["regModel"], cfg["n_layers"], *data_of(g), masks=masks)
    e32 = float(g[f"{name}_e32_grad"])
    for k, v in grads_of(m).items():
        assert T.rel_err(v, o["grads"][k]) <= 8 * e32, k
    assert abs(o["loss"] - oracle(g, name)["loss"]) > 1e-3          # the masks did something


def test_injected_dropout_masks_original_gate_layer(g):
    """The six masks of a BiMambaEncoderLayer ('bimamba'): forward block, ffn1 inner / output, backward block, ffn2 inner / output."""
    name, p = "bimamba", 0.2
    cfg = T.MODELS[name]
    widths = T.mask_widths(name, cfg["n_layers"], cfg["d_model"], cfg["dim_feedforward"])
    m, b = build(g, name, dropout=p).train(), batch(g)
    rng = np.random.default_rng(4)
    masks = [((rng.random((600, w)) >= p) / (1 - p)).astype(np.float32) for w in widths]
    m.dropout_masks = [torch.from_numpy(k).to(DEV) for k in masks]
    step_loss(m, b).backward()
    assert [tuple(k.shape) for k in m.last_dropout_masks] == [(600, w) for w in widths]
    o = T.model_grads(state_dict_of(g, name), cfg["regModel"], cfg["n_layers"], *data_of(g), masks=masks)
    e32 = float(g[f"{name}_e32_grad"])
    for k, v in grads_of(m).items():
        assert T.rel_err(v, o["grads"][k]) <= 8 * e32, k


def test_drawn_dropout_masks_and_seeded_repeatability(g):
    name, p = "bimamba+", 0.2
    m, b = build(g, name, dropout=p).train(), batch(g)
    runs = []
    for _ in range(2):
        torch.manual_seed(11)
        m.zero_grad()
        step_loss(m, b).backward()
        runs.append((grads_of(m), [k.clone() for k in m.last_dropout_masks]))
    assert all(np.array_equal(runs[0][0][k], runs[1][0][k]) for k in runs[0][0])
    assert len(runs[0][1]) == 9 and all(torch.equal(a, c) for a, c in zip(runs[0][1], runs[1][1]))
    for mask, width in zip(runs[0][1], (32, 32, 32, 64, 32, 32, 32, 64, 32)):
        assert mask.shape == (600, width)
        n = mask.numel()
        zeros = int((mask == 0).sum())
        assert abs(zeros - p * n) <= 4 * np.sqrt(n * p * (1 - p))
        assert torch.equal(mask[mask != 0], torch.full((n - zeros,), 1.0, device=DEV) / (1.0 - p))
    torch.manual_seed(12)
    m.zero_grad()
    step_loss(m, b).backward()
    assert not torch.equal(m.last_dropout_masks[0], runs[0][1][0])


@pytest.mark.parametrize("name", NAMES)
def test_an_optimiser_step_reaches_the_next_forward(g, name):
    """The padded copies of dt_proj / x_proj weights are keyed on the parameters' versions: after opt.step() the training and the
    inference forward both equal those of a fresh module that loaded the stepped state dict."""
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


def test_unbuilt_heads_keep_their_forward_in_the_training_state(g):
    b = batch(g)
    for name in ("mamba+", "mamba"):                 # no RMSNorm backward: the inference kernels, no graph
        m = VideoRegression(n_layers=1, d_model=32, d_hidden=64, dropout=0.0, total_vf_dim=30, regModel=name).to(DEV).train()
        ln_nd, inst = m(b["sem"], None, None, b["emo"])
        assert not ln_nd.requires_grad and not inst.requires_grad


def test_train_regression_mamba_cli(tmp_path, capsys):
    """Two epochs of the default head ('bimamba+') at the reference's default configuration on the miniature dataset; the split files
    are written here."""
    root, out = str(tmp_path / "data"), str(tmp_path / "out")
    c = HE.reg_dataset_content()
    HE.write_reg_dataset(root, c)
    for split in ("train", "val"):
        with open(os.path.join(root, "vevo_meta", "split", "v1", split + ".txt"), "w") as f:
            f.write("\n".join(c["ids"]) + "\n")
    res = TRM.main(["-dataset_dir", root, "-output_dir", out, "-epochs", "2", "-weight_modulus", "2", "-print_modulus", "1", "--seed", "5"])
    capsys.readouterr()
    d = os.path.join(out, "AMT")
    for f in ("results_regression.csv", "best_rmse_weights.pickle", "best_epochs_regression.txt", "model_params_regression.txt",
              os.path.join("weights_regression_bimamba+", "epoch_0002.pickle")):
        assert os.path.isfile(os.path.join(d, f)), f
    assert "regModel: bimamba+" in open(os.path.join(d, "model_params_regression.txt")).read()
    rows = list(csv.reader(open(os.path.join(d, "results_regression.csv"), newline="")))
    assert rows[0] == TR.CSV_HEADER and [r[0] for r in rows[1:]] == ["0", "1", "2"]
    assert res["best_epoch"] in (0, 1, 2) and min(float(r[6]) for r in rows[1:]) == res["best_val_total_loss"]
    m = VideoRegression(n_layers=2, d_model=64, d_hidden=256, dropout=0.2, total_vf_dim=30, regModel="bimamba+")
    m.load_state_dict(torch.load(os.path.join(d, "weights_regression_bimamba+", "epoch_0002.pickle"), map_location="cpu"), strict=True)
    # the last epoch's weights through evaluate_regression: the figures of the last CSV row for that split
    for split, cols in (("val", slice(6, 10)), ("train", slice(2, 6))):
        s = evaluate_regression.main(["-dataset_dir", root, "-output_dir", str(tmp_path / ("eval_" + split)), "-batch_size", "32", "-regModel", "bimamba+", "-model_weights",
                                      os.path.join(d, "weights_regression_bimamba+", "epoch_0002.pickle"), "--test_ids", "split:" + split])
        printed = [float(ln.rsplit(":", 1)[1]) for ln in capsys.readouterr().out.strip().splitlines()[-4:]]
        assert printed == [s[k] for k in TR.FIGURE_KEYS] == [float(v) for v in rows[-1][cols]]
