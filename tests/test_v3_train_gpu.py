"""One training step of the V3 chord models, and of '2.2' with balancing, on the device against the fp64 restatement of
tests/helpers_v3_train.py, by the rules of tests/test_family_train_gpu.py: the routing as a set per token, the set of parameters whose
.grad stays None, the loss within `loss_bound`, the logits within LOGIT_FACTOR x e32_y, every gradient within FACTOR x e32 (the lambda
vectors at their own scale, `lambda_bound`), and every `ff.bias` after the step equal to the restatement's fp32 arithmetic."""
import numpy as np
import pytest
import torch

from tests import helpers_train as T
from tests import helpers_v3_train as V
from video2music_amd import losses
from video2music_amd.model import video_music_transformer as M
from video2music_amd.model.moe import _MoEBase

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def build(name, enable=True):
    c = V.BY_NAME[name]
    cls = M.VideoMusicTransformer_V3 if c.version[0] == "3" else M.VideoMusicTransformer_V2
    m = cls(**V.model_kwargs(c))
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in V.state_dict(name).items()}, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    m = m.to(DEV).train()
    return m.enable_training() if enable else m


def _args(name):
    f = V.inputs(name)
    t = lambda k: torch.from_numpy(np.asarray(f[k])).to(DEV)
    return (t("ids"), t("root"), t("attr"), t("semantic"), t("key"), t("scene_offset"), t("motion"), t("emotion"))


def mixtures(m):
    return [q for q in m.modules() if isinstance(q, _MoEBase)]


def step(name, m):
    f = V.inputs(name)
    own, mix = V.masks(name)
    m.zero_grad(set_to_none=True)
    if own is not None:
        m.dropout_masks = [torch.from_numpy(a).to(DEV) for a in own]
        assert len(mixtures(m)) == len(mix)
        for q, lm in zip(mixtures(m), mix):
            q.dropout_masks = [torch.from_numpy(a).to(DEV) for a in lm]
    t = lambda k: torch.from_numpy(np.asarray(f[k])).to(DEV)
    logits = m(*_args(name))
    loss = losses.chord_train_loss(logits, t("tgt"), t("emo_class"), T.LAM, T.SMOOTHING)
    loss.backward()
    torch.cuda.synchronize()
    routes = [q.last_routing[0].reshape(-1, V.TOP_K).cpu() for q in mixtures(m)]
    biases = {k: b.cpu() for k, b in m.named_buffers() if k.endswith(".ff.bias")}
    return (float(loss.detach()), logits.detach().cpu().numpy(), {k: None if q.grad is None else q.grad.cpu().numpy() for k, q in m.named_parameters()},
            routes, biases)


@pytest.mark.parametrize("name", V.NAMES)
def test_one_step_against_fp64(name):
    ref = V.reference(name)
    m = build(name)
    assert m._train_path() and m._train_refusal() is None
    loss, y, g, routes, biases = step(name, m)
    assert len(routes) == len(ref["recs"])
    for got, rec in zip(routes, ref["recs"]):
        assert torch.equal(got.long().sort(-1).values, rec["idx"].sort(-1).values)
    params = {k: v for k, v in ref["g64"].items() if not k.endswith(".ff.bias")}
    assert set(g) == set(params)
    assert {k for k, v in g.items() if v is None} == {k for k, v in params.items() if v is None}
    e_y = V.logit_err(y, ref["y64"])
    plain, lam = V.grad_errors(g, params, ref["scales"])
    worst = max(plain, key=plain.get)
    print(f"{name}: loss {loss:.9g} (fp64 {ref['l64'][0]:.9g}, bound {V.loss_bound(ref):.3e}); logits {e_y:.3e} (e32 {ref['e32_y']:.3e}); "
          f"worst gradient {worst} {plain[worst]:.3e} (e32 {ref['e32']:.3e}); worst lambda vector {max(lam.values()) if lam else 0.0:.3e} "
          f"(e32 {ref['e32_lambda']:.3e}, bound {V.lambda_bound(ref):.3e})")
    assert abs(loss - ref["l64"][0]) <= V.loss_bound(ref)
    assert e_y <= V.LOGIT_FACTOR * ref["e32_y"]
    bad = {k: e for k, e in plain.items() if not e <= V.bound(ref)}
    assert not bad, (V.bound(ref), bad)
    bad = {k: e for k, e in lam.items() if not e <= V.lambda_bound(ref)}
    assert not bad, (V.lambda_bound(ref), bad)
    keys = V.bias_keys(V.state_dict(name))
    assert sorted(biases) == sorted(keys) and len(keys) == len(ref["recs"])
    for k, rec in zip(keys, ref["recs"]):
        assert torch.equal(biases[k], rec["bias_after"]), k
        assert not torch.equal(biases[k], torch.from_numpy(V.state_dict(name)[k]))


@pytest.mark.parametrize("name", ["c30_drop", "c32"])
def test_the_same_step_twice_gives_the_same_bits_and_the_next_one_starts_from_the_updated_bias(name):
    m = build(name)
    start = {k: b.clone() for k, b in m.named_buffers() if k.endswith(".ff.bias")}
    a = step(name, m)
    after = {k: b.clone() for k, b in m.named_buffers() if k.endswith(".ff.bias")}
    with torch.no_grad():
        for k, b in m.named_buffers():
            if k in start:
                b.copy_(start[k])
    b = step(name, m)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    for k in a[2]:
        assert (a[2][k] is None and b[2][k] is None) or np.array_equal(a[2][k], b[2][k]), k
    for k in a[4]:
        assert torch.equal(a[4][k], b[4][k])
    # a step that is not reset routes on the bias the last one left: the update_rate (mean(c) - c) of its own counts lands on top
    c = step(name, m)
    for q, k in zip(mixtures(m), V.bias_keys(V.state_dict(name))):
        cnt = torch.bincount(q.last_routing[0].reshape(-1).cpu().long(), minlength=V.N_EXPERTS).to(torch.float32)
        assert torch.equal(c[4][k], after[k].cpu() + (V.UPDATE_RATE * (torch.mean(cnt) - cnt)).unsqueeze(1)), k


@pytest.mark.parametrize("name", ["c31", "c22_bal"])
def test_without_gradients_or_in_eval_mode_the_forward_is_the_code_it_was(name):
    plain, opted = build(name, enable=False), build(name, enable=True)
    y = [m.eval()(*_args(name)) for m in (plain, opted)]
    assert not y[0].requires_grad and torch.equal(y[0], y[1])
    with torch.no_grad():
        y2 = [m.eval()(*_args(name)) for m in (plain, opted)]
    assert torch.equal(y2[0], y[0]) and torch.equal(y2[1], y[0])
    for m in (plain, opted):                                       # training mode without gradients: the mixtures answer as before
        with torch.no_grad(), pytest.raises(NotImplementedError, match="balancing=True"):
            m.train()(*_args(name))
    for k, b in opted.named_buffers():                             # none of this moved a bias
        if k.endswith(".ff.bias"):
            assert torch.equal(b.cpu(), torch.from_numpy(V.state_dict(name)[k]))
    ref = V.reference(name)
    with torch.no_grad():
        P = {k: V.cast(v, torch.float64) for k, v in V.state_dict(name).items()}
        want = V.forward_restated(P, V.BY_NAME[name], V.inputs(name), training=False).numpy()
    assert V.logit_err(y[0].cpu().numpy(), want) <= V.LOGIT_FACTOR * max(ref["e32_y"], V.U)


@pytest.mark.parametrize("name,pattern", [("c31", "differential attention"), ("c22_bal", "balancing=True")])
def test_a_model_without_enable_training_still_refuses(name, pattern):
    m = build(name, enable=False)
    with pytest.raises(NotImplementedError, match=pattern):
        m(*_args(name))
    assert m.enable_training() is m and m._train_refusal() is None
    assert all(q.train_balancing for q in mixtures(m)) and m(*_args(name)).requires_grad


def test_head_dims_other_than_32_64_128_stay_refused_after_the_call():
    m = M.VideoMusicTransformer_V3(version_name="3.1", n_layers=3, num_heads=4, d_model=64, dim_feedforward=96, total_vf_dim=32).to(DEV).train()
    m.enable_training()
    assert "head_dim 16" in m._train_refusal()
    m = M.VideoMusicTransformer_V2(version_name="2.1", n_layers=3, num_heads=2, d_model=64, dim_feedforward=96, total_vf_dim=32).train()
    assert "TopKScheduler" in m.enable_training()._train_refusal()
