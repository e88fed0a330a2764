"""One training step of `VideoRegression` after `enable_training()` -- `regression_train_loss(...).backward()` -- for 'mamba' /
'mamba+' / 'moemamba' / 'cnngru' at the shapes where a step's launch plan changes, against the fp64 restatement of
tests/helpers_reg_rest_train.py on the case's own inputs.  Weights, inputs, conditioning and bounds are those of
tests/helpers_reg_train_edges.py: `video2music_amd.synthetic` over `helpers_reg_parity.named_shapes`, its `_draw`, a target whose fp64
residual lies within SL1_MARGIN of +-1 moved by 4 SL1_MARGIN, every dropout rate 0;

    every gradient   rel_err(got, g64) <= max(8 e32, rows U), e32 the same restatement in fp32 on one CPU thread against the same
                     fp64, per case and tensor; an fp64 gradient that is exactly zero is exactly zero on the device
    ln_nd, p         max(8 e32, W U) of their largest value, W the feature width
    the loss         what those two move it by plus `loss_adds(rows) + 8` roundings of its own

At the listed seeds every mixture layer's fp64 gate gap is at least GAP and no probability lies within P_MARGIN of 0 or 1 (picked on
the CPU; a seed that fails is replaced in the table, never skipped at run time); the test asserts both and the routing of every token."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import helpers_reg_parity as P
from tests import helpers_reg_rest_train as T
from tests import helpers_reg_train_edges as E
from video2music_amd import synthetic
from video2music_amd.losses import regression_train_loss
from video2music_amd.model.video_regression import VideoRegression

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Case = namedtuple("Case", "name rm d dh vf B S n_layers seed edge")
_TABLE = [
    Case("moemamba_cli_width", "moemamba", 64, 256, 37, 2, 33, 2, 4101, "the CLI's width: 256 states (16 slices), d_conv 8, ldbc 516, one step past a checkpoint"),
    Case("moemamba_one_token", "moemamba", 32, 128, 37, 1, 1, 1, 4102, "128 states, one token: dA_log exactly zero, four experts without a row"),
    Case("mambap_dt6_below_conv", "mamba+", 96, 64, 37, 1, 3, 1, 4103, "dt_rank 6, ldbc 38 -> 40; S = 3 below d_conv"),
    Case("mamba_one_row", "mamba", 32, 64, 37, 1, 1, 2, 4104, "one row: every weight-gradient K is 1 padded to 32"),
    Case("mamba_rows4097", "mamba", 32, 64, 37, 1, 4097, 1, 4105, "4097 rows in one clip: 129 checkpoints, the data products leave the skinny GEMM"),
    Case("cnngru_one_step", "cnngru", 32, 64, 37, 2, 1, 1, 4106, "S = 1: six of the seven taps read padding"),
    Case("cnngru_rows1540", "cnngru", 64, 64, 37, 1, 1540, 2, 4107, "1540 rows in one clip: weight-gradient K above skinny_k"),
]
CASES = {c.name: c for c in _TABLE}
NAMES = list(CASES)


def rows(c):
    return c.B * c.S


def model_kwargs(c):
    return dict(n_layers=c.n_layers, d_model=c.d, d_hidden=c.dh, total_vf_dim=c.vf, regModel=c.rm, dropout=0.0)


@functools.lru_cache(maxsize=None)
def state_dict(name):
    c = CASES[name]
    return synthetic.synthetic_state_dict(P.named_shapes(**model_kwargs(c)), seed=c.seed)


def _grads(c, sd, data, dtype):
    return T.model_grads(sd, c.rm, c.n_layers, *data, dtype=dtype)


@functools.lru_cache(maxsize=None)
def batch(name):
    c = CASES[name]
    sem, emo, nd, loud, inst = E._draw(c)
    ln = _grads(c, state_dict(name), (sem, emo, nd, loud, inst), torch.float64)["ln_nd"].reshape(c.B, c.S, 2)
    for j, tgt in enumerate((nd, loud)):
        close = np.abs(np.abs(ln[..., j] - tgt.astype(np.float64)) - 1.0) < E.SL1_MARGIN
        tgt[close] += np.float32(4 * E.SL1_MARGIN)
    return sem, emo, nd, loud, inst


@functools.lru_cache(maxsize=None)
def reference(name):
    """fp64 and fp32 (one CPU thread) runs of the restatement, computed once and never written to."""
    c, sd, data = CASES[name], state_dict(name), batch(name)
    o64 = _grads(c, sd, data, torch.float64)
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        o32 = _grads(c, sd, data, torch.float32)
    finally:
        torch.set_num_threads(n)
    e32 = {k: (T.rel_err(o32["grads"][k], g) if np.abs(g).max() > 0 else float(np.abs(o32["grads"][k]).max())) for k, g in o64["grads"].items()}
    return {"o64": o64, "e32": e32, "e32_ln": T.rel_err(o32["ln_nd"], o64["ln_nd"]), "e32_p": T.rel_err(o32["p"], o64["p"])}


def grad_bound(name, key):
    return max(E.GRAD_FACTOR * reference(name)["e32"][key], rows(CASES[name]) * T.U)


def output_bounds(name):
    r, W = reference(name), CASES[name].d
    return max(E.GRAD_FACTOR * r["e32_ln"], W * T.U), max(E.GRAD_FACTOR * r["e32_p"], W * T.U)


def loss_bound(name):
    c, o = CASES[name], reference(name)["o64"]
    b_ln, b_p = output_bounds(name)
    p = o["p"]
    return (b_ln * np.abs(o["ln_nd"]).max() + b_p * p.max() * float((1.0 / np.minimum(p, 1 - p)).mean())
            + (E.loss_adds(rows(c)) + 8) * T.U * abs(o["loss"]))


def grad_errors(got, name):
    out = {}
    for k, want in reference(name)["o64"]["grads"].items():
        g = np.asarray(got[k], dtype=np.float64)
        assert g.shape == want.shape, (k, g.shape, want.shape)
        if (g[want == 0.0] != 0.0).any():
            out[k] = float("inf")
        elif np.abs(want).max() == 0.0:
            out[k] = 0.0
        else:
            out[k] = T.rel_err(g, want) / grad_bound(name, k)
    return out


def moe_layers(m):
    return [lyr[1].moe_layer for lyr in m.model.layers] if m.regModel == "moemamba" else []


def build(name):
    m = VideoRegression(**model_kwargs(CASES[name]))
    for layer in moe_layers(m):                                          # the experts' own Dropout (GLUExpert's default 0.1)
        for e in list(layer.experts) + [layer.shared_expert]:
            e.dropout.p = 0.0
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state_dict(name).items()}, strict=True)
    return m.to(DEV).enable_training().train()


def step(m, data):
    sem, emo, nd, loud, inst = data
    m.zero_grad(set_to_none=True)
    ln_nd, p = m(sem, None, None, emo)
    loss = regression_train_loss(ln_nd, p, nd, loud, inst)
    loss.backward()
    return ln_nd.detach(), p.detach(), float(loss.detach()), {k: q.grad.detach().cpu().numpy() for k, q in m.named_parameters()}


@pytest.mark.parametrize("name", NAMES)
def test_loss_outputs_and_every_gradient_against_fp64(name):
    c, ref = CASES[name], reference(name)
    o64 = ref["o64"]
    assert T.min_gap([o64["routing"]]) >= T.GAP and len(o64["routing"]) == (c.n_layers if c.rm == "moemamba" else 0)
    p64 = o64["p"]
    assert p64.min() >= E.P_MARGIN and p64.max() <= 1 - E.P_MARGIN
    m, data = build(name), [torch.from_numpy(a).to(DEV) for a in batch(name)]
    ln_nd, p, loss, got = step(m, data)
    b_ln, b_p = output_bounds(name)
    e_ln, e_p = T.rel_err(ln_nd.cpu().numpy(), o64["ln_nd"]), T.rel_err(p.cpu().numpy(), o64["p"])
    l_err, l_bound = abs(loss - o64["loss"]), loss_bound(name)
    assert set(got) == set(o64["grads"])
    errs = grad_errors(got, name)
    worst = max(errs, key=errs.get)
    print(f"{name}: worst gradient err / bound = {errs[worst]:.3f} ({worst}, bound {grad_bound(name, worst):.2e}); ln_nd {e_ln / b_ln:.3f} "
          f"p {e_p / b_p:.3f} of their bounds; loss {loss:.7f} fp64 {o64['loss']:.7f} err / bound = {l_err / l_bound:.3f}")
    assert ln_nd.shape == (c.B, c.S, 2) and p.shape == (c.B, c.S, 40)
    assert e_ln <= b_ln and e_p <= b_p, (e_ln, b_ln, e_p, b_p)
    assert l_err <= l_bound, (loss, o64["loss"], l_bound)
    assert errs[worst] <= 1, {k: round(v, 2) for k, v in errs.items() if v > 1}
    for layer, r in zip(moe_layers(m), o64["routing"]):                  # the fp64 top-2 of every layer, every token
        assert np.array_equal(layer.last_routing[0].reshape(rows(c), T.TOP_K).cpu().numpy(), r["idx"].reshape(rows(c), T.TOP_K).numpy())
    again = step(m, data)                                                # the same bits from a second backward
    assert again[2] == loss and all(np.array_equal(again[3][k], v) for k, v in got.items())
