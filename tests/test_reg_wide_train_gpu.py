"""Training of the wide recurrent heads (`VideoRegression(..., wide_recurrent=True)` at d_model 160: autograd.RnnLayerFn on the
amt_rnn_wide_seq_train_fwd / amt_rnn_wide_seq_bwd pair) against the fp64 restatements, and the command line end to end.

One training step of 'bilstm', 'gru' (tests/helpers_reg_train.model_grads64) and 'cnnbigru' (tests/helpers_reg_rest_train.model_grads,
after `enable_training()`), two layers, model dropout 0.2 with the multipliers given to both sides.  Bounds, the forms of
tests/helpers_reg_train_edges.py with e32 the same restatement in fp32 on one CPU thread: every gradient rel_err <= max(8 e32, rows U),
an exact fp64 zero exact; ln_nd and p max(8 e32, W U) of their largest value; the loss what those two move it by plus the roundings of
the fused loss's sums (`loss_adds`) and 8 for the logarithms.

Then `python -m video2music_amd.train_regression -regModel bilstm -d_model 160` for one epoch on the miniature dataset and
`python -m video2music_amd.evaluate_regression` on the weights it wrote, each a fresh child process."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import helpers_reg_eval as HE
from tests import helpers_reg_parity as P
from tests import helpers_reg_rest_train as T
from tests import helpers_reg_train as R
from tests import helpers_reg_train_edges as E
from video2music_amd import synthetic
from video2music_amd.losses import regression_train_loss
from video2music_amd.model.video_regression import VideoRegression

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = R.U
D, D_HIDDEN, VF, B, S, LAYERS, P_DROP = 160, 64, 13, 2, 5, 2, 0.2
HEADS = {"bilstm": 4101, "gru": 4102, "cnnbigru": 4103}            # seed of the weights; seed + 1000: inputs, targets and masks
ROWS = B * S


def kwargs(rm):
    return dict(n_layers=LAYERS, d_model=D, d_hidden=D_HIDDEN, total_vf_dim=VF, regModel=rm)


@functools.lru_cache(maxsize=None)
def case(rm):
    """(state dict, (sem, emo, note_density, loudness, instrument), masks), numpy fp32."""
    sd = synthetic.synthetic_state_dict(P.named_shapes(**kwargs(rm)), seed=HEADS[rm])
    data = E._draw(E.Case(rm, rm, D, D_HIDDEN, VF, B, S, LAYERS, HEADS[rm], "d_model 160 on the wide kernels"))
    dirs = 2 if "bi" in rm else 1
    if rm.startswith("cnn"):
        shapes = T.mask_shapes(rm, LAYERS, ROWS, D, P_DROP)
        assert shapes == [(ROWS, D), (ROWS, D)] + [(ROWS, dirs * D)] * (LAYERS - 1)
    else:                                                           # after in_proj, then between the recurrent layers (model_grads64)
        shapes = [(ROWS, D)] + [(ROWS, dirs * D)] * (LAYERS - 1)
    rng = np.random.default_rng(HEADS[rm] + 1000)
    masks = [((rng.random(s) >= P_DROP) / (1 - P_DROP)).astype(np.float32) for s in shapes]
    return sd, data, masks


def restatement(rm, fp64):
    sd, data, masks = case(rm)
    if rm.startswith("cnn"):
        return T.model_grads(sd, rm, LAYERS, *data, masks=masks, dtype=torch.float64 if fp64 else torch.float32)
    return R.model_grads64(sd, rm, LAYERS, *data, masks=masks, dtype=np.float64 if fp64 else np.float32)


@functools.lru_cache(maxsize=None)
def reference(rm):
    o64 = restatement(rm, True)
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        o32 = restatement(rm, False)
    finally:
        torch.set_num_threads(n)
    e32 = {k: R.rel_err(o32["grads"][k], g) for k, g in o64["grads"].items()}
    return {"o64": o64, "e32": e32, "e32_ln": R.rel_err(o32["ln_nd"], o64["ln_nd"]), "e32_p": R.rel_err(o32["p"], o64["p"])}


@pytest.mark.parametrize("rm", list(HEADS))
def test_one_training_step_against_fp64(rm):
    sd, data, masks = case(rm)
    ref = reference(rm)
    o = ref["o64"]
    # the conditions a bound made of rounding needs (helpers_reg_train_edges): no SmoothL1 residual at its kink, no saturated probability
    for j, tgt in enumerate(data[2:4]):
        assert (np.abs(np.abs(o["ln_nd"].reshape(B, S, 2)[..., j] - tgt.astype(np.float64)) - 1.0) >= E.SL1_MARGIN).all()
    assert E.P_MARGIN < o["p"].min() and o["p"].max() < 1 - E.P_MARGIN
    m = VideoRegression(**kwargs(rm), dropout=P_DROP, wide_recurrent=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).train()
    if rm.startswith("cnn"):
        m.enable_training()
    m.dropout_masks = [torch.from_numpy(k).to(DEV) for k in masks]
    sem, emo, nd, loud, inst = (torch.from_numpy(a).to(DEV) for a in data)
    ln_nd, p = m(sem, None, None, emo)
    assert ln_nd.requires_grad and len(m.last_dropout_masks) == len(masks)
    loss = regression_train_loss(ln_nd, p, nd, loud, inst)
    loss.backward()
    got = {k: q.grad.detach().cpu().numpy().astype(np.float64) for k, q in m.named_parameters()}
    assert set(got) == set(o["grads"])

    W = D * (2 if "bi" in rm else 1)
    b_ln, b_p = max(E.GRAD_FACTOR * ref["e32_ln"], W * U), max(E.GRAD_FACTOR * ref["e32_p"], W * U)
    e_ln = R.rel_err(ln_nd.detach().cpu().numpy().reshape(o["ln_nd"].shape), o["ln_nd"])
    e_p = R.rel_err(p.detach().cpu().numpy().reshape(o["p"].shape), o["p"])
    l_bound = (b_ln * np.abs(o["ln_nd"]).max() + b_p * o["p"].max() * float((1.0 / np.minimum(o["p"], 1 - o["p"])).mean())
               + (E.loss_adds(ROWS) + 8) * U * abs(o["loss"]))
    l_err = abs(float(loss.detach()) - float(o["loss"]))
    ratios = {}
    for k, want in o["grads"].items():
        want = np.asarray(want, dtype=np.float64)
        assert got[k].shape == want.shape and not (got[k][want == 0.0] != 0.0).any(), k
        ratios[k] = R.rel_err(got[k], want) / max(E.GRAD_FACTOR * ref["e32"][k], ROWS * U)
    worst = max(ratios, key=ratios.get)
    print(f"{rm} d {D}: worst gradient err / bound = {ratios[worst]:.3f} ({worst}); ln_nd {e_ln / b_ln:.3f} p {e_p / b_p:.3f} of their bounds; "
          f"loss {float(loss.detach()):.7f} fp64 {float(o['loss']):.7f} err / bound = {l_err / l_bound:.3f}")
    assert e_ln <= b_ln and e_p <= b_p, (e_ln, b_ln, e_p, b_p)
    assert l_err <= l_bound, (float(loss.detach()), o["loss"], l_bound)
    assert ratios[worst] <= 1, {k: round(v, 2) for k, v in ratios.items() if v > 1}


def test_train_then_evaluate_from_the_command_line_at_160(tmp_path):
    root, out, ev = str(tmp_path / "data"), str(tmp_path / "out"), str(tmp_path / "eval")
    c = HE.reg_dataset_content()
    HE.write_reg_dataset(root, c)
    for split in ("train", "val"):
        with open(os.path.join(root, "vevo_meta", "split", "v1", split + ".txt"), "w") as f:
            f.write("\n".join(c["ids"]) + "\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    model = ["-regModel", "bilstm", "-d_model", "160"]
    r = subprocess.run([sys.executable, "-m", "video2music_amd.train_regression", "-dataset_dir", root, "-output_dir", out, "-epochs", "1",
                        "-weight_modulus", "1", "-print_modulus", "1", "--seed", "5"] + model, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = os.path.join(out, "AMT")
    weights = os.path.join(d, "weights_regression_bilstm", "epoch_0001.pickle")
    for f in ("results_regression.csv", "best_rmse_weights.pickle", "best_epochs_regression.txt", "model_params_regression.txt", weights):
        assert os.path.isfile(os.path.join(d, f)), f
    assert "d_model: 160" in open(os.path.join(d, "model_params_regression.txt")).read()
    sd = torch.load(weights, map_location="cpu")
    assert tuple(sd["model.weight_hh_l1_reverse"].shape) == (4 * 160, 160)
    r = subprocess.run([sys.executable, "-m", "video2music_amd.evaluate_regression", "-dataset_dir", root, "-output_dir", ev, "-batch_size", "32",
                        "-model_weights", weights, "--test_ids", "split:val"] + model, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.path.isfile(os.path.join(ev, "metrics.json"))
