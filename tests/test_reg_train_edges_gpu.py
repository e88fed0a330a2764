"""One training step of `VideoRegression` on the device -- `regression_train_loss(...).backward()` -- for the eight heads that train,
at the shapes where a step's launch plan changes (tests/helpers_reg_train_edges.py; tests/test_reg_train_edges_host.py checks every
case's claim, its conditioning and that it can see the errors it exists for), against the fp64 restatements on the case's own inputs.

Held per case: the loss (within `loss_bound`), ln_nd and p of the training state (max(8 e32, W U)), every parameter's gradient
(rel_err <= max(8 e32, rows U), exact zeros where fp64 has them), the fp64 top-2 routing of every mixture layer on every token, and
the same bits from a second backward.  For one case per family the (M, N, K) of every `ops.linear_ex` call of the step is compared
with the product list the host test derives the routes from."""
import collections

import numpy as np
import pytest
import torch

from tests import helpers_moe_train as M
from tests import helpers_reg_train as R
from tests import helpers_reg_train_edges as E
from video2music_amd import ops
from video2music_amd.losses import regression_train_loss
from video2music_amd.model.video_regression import VideoRegression

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RECORDED = ("bilstm_half48", "bimamba_dt6", "shared_two_layers")        # one case per family


def build(name):
    c = E.CASES[name]
    m = VideoRegression(**E.model_kwargs(c))
    if E.family(c) == "mixture":                                         # the experts' own Dropout (GLUExpert's default 0.1)
        for lyr in m.model.layers:
            for e in list(lyr.ffn.experts) + ([lyr.ffn.shared_expert] if lyr.ffn.shared else []):
                e.dropout.p = 0.0
    m.load_state_dict({k: torch.from_numpy(v) for k, v in E.state_dict(name).items()}, strict=True)
    return m.to(DEV).train()


def step(m, data):
    """One forward + backward from cleared gradients: ln_nd, p, loss, {key: gradient}."""
    sem, emo, nd, loud, inst = data
    m.zero_grad(set_to_none=True)
    ln_nd, p = m(sem, None, None, emo)
    loss = regression_train_loss(ln_nd, p, nd, loud, inst)
    loss.backward()
    return ln_nd.detach(), p.detach(), float(loss.detach()), {k: q.grad.detach().cpu().numpy() for k, q in m.named_parameters()}


@pytest.mark.parametrize("name", E.NAMES)
def test_loss_outputs_and_every_gradient_against_fp64(name, monkeypatch):
    c, ref = E.CASES[name], E.reference(name)
    o64 = ref["o64"]
    m, data = build(name), [torch.from_numpy(a).to(DEV) for a in E.batch(name)]
    calls = []
    if name in RECORDED:
        plain = ops.linear_ex

        def recording(x, w, *args, **kw):
            K = kw.get("K", args[4] if len(args) > 4 else None)
            calls.append((x.shape[0], w.shape[0], w.shape[1] if K is None else K))
            return plain(x, w, *args, **kw)
        monkeypatch.setattr(ops, "linear_ex", recording)
    ln_nd, p, loss, got = step(m, data)
    monkeypatch.undo()

    b_ln, b_p = E.output_bounds(name)
    e_ln, e_p = R.rel_err(ln_nd.cpu().numpy(), o64["ln_nd"]), R.rel_err(p.cpu().numpy(), o64["p"])
    l_err, l_bound = abs(loss - o64["loss"]), E.loss_bound(name)
    assert set(got) == set(o64["grads"])
    errs = E.grad_errors(got, name)
    worst = max(errs, key=errs.get)
    print(f"{name}: worst gradient err / bound = {errs[worst]:.3f} ({worst}, bound {E.grad_bound(name, worst):.2e}); ln_nd {e_ln / b_ln:.3f} "
          f"p {e_p / b_p:.3f} of their bounds; loss {loss:.7f} fp64 {o64['loss']:.7f} err / bound = {l_err / l_bound:.3f}")
    assert ln_nd.shape == (c.B, c.S, 2) and p.shape == (c.B, c.S, 40)
    assert e_ln <= b_ln and e_p <= b_p, (e_ln, b_ln, e_p, b_p)
    assert l_err <= l_bound, (loss, o64["loss"], l_bound)
    assert errs[worst] <= 1, {k: round(v, 2) for k, v in errs.items() if v > 1}
    if E.family(c) == "mixture":                                         # the fp64 top-2 of every layer, every token
        for lyr, r in zip(m.model.layers, o64["routing"]):
            assert np.array_equal(lyr.ffn.last_routing[0].reshape(E.rows(c), M.TOP_K).cpu().numpy(), r["idx"].reshape(E.rows(c), M.TOP_K).numpy())
    if name in RECORDED:
        want = collections.Counter((q.M, q.N, q.K) for q in E.case_products(c))
        assert collections.Counter(calls) == want, (sorted((collections.Counter(calls) - want).items()), sorted((want - collections.Counter(calls)).items()))

    ln2, p2, loss2, again = step(m, data)                                # the same bits twice
    assert torch.equal(ln_nd, ln2) and torch.equal(p, p2) and loss == loss2
    assert all(np.array_equal(got[k], again[k]) for k in got)
