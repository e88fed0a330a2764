"""One training step of the V1 / V2 chord models on the device against the fp64 restatement of tests/helpers_family_train.py: the loss
(`losses.chord_train_loss`), the logits and every parameter gradient, per case of its table.  Gradients and logits are held to 8 x e32
(e32: the restatement in float32 on the CPU, by `rel_err` at `grad_scale`), the loss to the bound that follows from the logits'; the
set of parameters whose .grad stays None must be the fp64 side's.  The mixture layers' routing is checked against the fp64 choice, so a
flipped route shows as itself and not as a gradient error (the host test holds every case's gate-logit gap above ROUTE_GAP)."""
import numpy as np
import pytest
import torch

from tests import helpers_family_train as FT
from tests import helpers_train as T
from video2music_amd import losses
from video2music_amd.model import video_music_transformer as M
from video2music_amd.model.moe import _MoEBase

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def build(name):
    c = FT.BY_NAME[name]
    cls = M.VideoMusicTransformer_V1 if c.version[0] == "1" else M.VideoMusicTransformer_V2
    m = cls(**FT.model_kwargs(c))
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in FT.state_dict(name).items()}, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    return m.to(DEV).train()


def step(name, m):
    c, f = FT.BY_NAME[name], FT.inputs(name)
    own, mix = FT.masks(name)
    m.zero_grad(set_to_none=True)
    if own is not None:
        m.dropout_masks = [torch.from_numpy(a).to(DEV) for a in own]
        layers = [q for q in m.modules() if isinstance(q, _MoEBase)]
        assert len(layers) == len(mix)
        for q, lm in zip(layers, mix):
            q.dropout_masks = [torch.from_numpy(a).to(DEV) for a in lm]
    t = lambda k: torch.from_numpy(np.asarray(f[k])).to(DEV)
    logits = m(t("ids"), t("root"), t("attr"), t("semantic"), t("key"), t("scene_offset"), t("motion"), t("emotion"), mask=c.mask)
    loss = losses.chord_train_loss(logits, t("tgt"), t("emo_class"), T.LAM, T.SMOOTHING)
    loss.backward()
    torch.cuda.synchronize()
    routes = [q.last_routing[0].reshape(-1, FT.TOP_K).cpu() for q in m.modules() if isinstance(q, _MoEBase)]
    return float(loss.detach()), logits.detach().cpu().numpy(), {k: None if q.grad is None else q.grad.cpu().numpy() for k, q in m.named_parameters()}, routes


@pytest.mark.parametrize("name", FT.NAMES)
def test_one_step_against_fp64(name):
    ref = FT.reference(name)
    m = build(name)
    assert m._train_path()
    loss, y, g, routes = step(name, m)
    # routing: the fp64 choice, as a set per token (the module lists the mixtures encoder first, as the restatement meets them)
    assert len(routes) == len(ref["gates"])
    for got, gate in zip(routes, ref["gates"]):
        want = gate.topk(FT.TOP_K, dim=-1).indices
        assert torch.equal(got.long().sort(-1).values, want.sort(-1).values)
    assert set(g) == set(ref["g64"])
    assert {k for k, v in g.items() if v is None} == {k for k, v in ref["g64"].items() if v is None}
    e_y = FT.logit_err(y, ref["y64"])
    errs = FT.grad_errors(g, ref["g64"])
    worst = max(errs, key=errs.get)
    print(f"{name}: loss {loss:.9g} (fp64 {ref['l64'][0]:.9g}, bound {FT.loss_bound(ref):.3e}); logits {e_y:.3e} (e32 {ref['e32_y']:.3e}); "
          f"worst gradient {worst} {errs[worst]:.3e} (e32 {ref['e32']:.3e})")
    assert abs(loss - ref["l64"][0]) <= FT.loss_bound(ref)
    assert e_y <= FT.LOGIT_FACTOR * ref["e32_y"]
    bad = {k: e for k, e in errs.items() if not e <= FT.FACTOR * ref["e32"]}
    assert not bad, (FT.FACTOR * ref["e32"], bad)


def test_the_same_step_twice_gives_the_same_bits():
    m = build("v22_drop")
    a, b = step("v22_drop", m), step("v22_drop", m)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    for k in a[2]:
        assert (a[2][k] is None and b[2][k] is None) or np.array_equal(a[2][k], b[2][k]), k


def _args(name):
    f = FT.inputs(name)
    t = lambda k: torch.from_numpy(np.asarray(f[k])).to(DEV)
    return (t("ids"), t("root"), t("attr"), t("semantic"), t("key"), t("scene_offset"), t("motion"), t("emotion"))


def test_drawn_masks_are_kept_in_the_documented_order():
    name = "v22_drop"
    m = build(name)
    torch.manual_seed(0)
    y = m(*_args(name))
    own, _ = FT.mask_shapes(FT.BY_NAME[name])
    assert y.requires_grad and [tuple(q.shape) for q in m.last_dropout_masks] == [s for _, s in own]
    rows = m.last_dropout_masks[0]
    assert set(rows.unique().tolist()) <= {0.0, 1.0} and 0 < float(rows.mean()) < 1


def test_without_gradients_the_forward_is_the_code_it_was():
    """Training mode under no_grad takes the operator composition, not the autograd path: with dropout 0 its logits are eval's bits."""
    name = "v22"
    m = build(name)
    with torch.no_grad():
        y0 = m(*_args(name))
    y1 = m.eval()(*_args(name))
    assert not y0.requires_grad and not y1.requires_grad and torch.equal(y0, y1)
    y2 = m.train()(*_args(name))
    assert y2.requires_grad and FT.logit_err(y2.detach().cpu().numpy(), y1.cpu().numpy().astype(np.float64)) <= 1e-5
