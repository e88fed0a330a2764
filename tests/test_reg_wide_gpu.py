"""`VideoRegression(..., wide_recurrent=True)`: the six recurrent heads at d_model above 128, where `get_feature` / `forward` run the wide
recurrence kernels (csrc/rnn_wide.hip).

On the GPU: eval forward against the float64 oracle (`oracle.reg_oracle.forward`) at the cases of tests/helpers_reg_wide.py, measured and
bounded as tests/test_reg_forward_parity_gpu.py does (max |got - ref64| / max(1, max |ref64|) <= 8 x e32 per output); the flag changes
nothing at d_model 64 (equal bits); the state dict is torch's nn.LSTM / nn.GRU of that width; the reference class's own outputs
(tests/golden/g_reg_wide.npz, tools/make_goldens_reg_wide.py) within the 5e-5 that tests/test_reg_gpu.py allows against g_reg.npz.
On the CPU (not marked): the constructor's rules, and the conditions of the parity cases."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import helpers_reg_parity as HR
from tests import helpers_reg_wide as W
from video2music_amd.model.video_regression import VideoRegression

gpu = pytest.mark.gpu


def build(c, **kw):
    m = VideoRegression(**HR.model_kwargs(c), **kw).eval()
    sd = HR.state_dict(c.name)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}, \
        "the key list of helpers_reg_parity.named_shapes is not the class's state dict"
    m.load_state_dict(sd, strict=True)
    return m


# ---- CPU ----

def test_default_constructor_still_refuses_256():
    for rm in W.HEADS:
        with pytest.raises(ValueError, match="at most 128"):
            VideoRegression(n_layers=1, d_model=256, d_hidden=64, total_vf_dim=13, regModel=rm)
        with pytest.raises(ValueError, match="at most 128"):
            VideoRegression(n_layers=1, d_model=256, d_hidden=64, total_vf_dim=13, regModel=rm, wide_recurrent=False)


@pytest.mark.parametrize("d", [136, 544, 520])
def test_flag_refuses_other_widths_with_the_rule(d):
    for rm in W.HEADS:
        with pytest.raises(ValueError, match=f"multiple of 32, at most 512 .got {d}"):
            VideoRegression(n_layers=1, d_model=d, d_hidden=64, total_vf_dim=13, regModel=rm, wide_recurrent=True)


def test_flag_is_keyword_only_and_accepts_the_wide_widths():
    with pytest.raises(TypeError):
        VideoRegression(1, 256, 64, 0.1, False, 300, 13, "bilstm", False, False, True)
    for d in (32, 128, 160, 512):
        m = VideoRegression(n_layers=1, d_model=d, d_hidden=64, total_vf_dim=13, regModel="bigru", wide_recurrent=True)
        assert m.regressor.in_features == 2 * d
    m = VideoRegression(n_layers=1, d_model=256, d_hidden=64, total_vf_dim=13, regModel="bimamba+", wide_recurrent=True)     # no recurrent head: no effect
    assert m.regressor.in_features == 256


@pytest.mark.parametrize("name", W.NAMES)
def test_case_conditions(name):
    """test_reg_parity_host.py's conditions on a case's bounds: in (0, CAP], and no luckier than four float32 roundings of the output."""
    bounds, floor = HR.bounds(name), HR.bound_floor(name)
    for k in HR.OUTPUTS:
        assert 0.0 < bounds[k] <= HR.CAP, f"{name} {k}: bound {bounds[k]:.2e} outside (0, cap]; change its seed"
        assert bounds[k] >= floor[k], f"{name} {k}: bound {bounds[k]:.2e} under four float32 roundings ({floor[k]:.2e}); change its seed"


def test_table_covers_every_head_width_and_length():
    assert {(c.rm, c.d, c.S) for c in W.CASES} == {(rm, d, S) for rm in W.HEADS for d in (160, 256) for S in (1, 5)}
    assert all(c.n_layers == 2 and c.B == 2 for c in W.CASES) and len({c.seed for c in W.CASES}) == len(W.CASES)
    assert not set(W.NAMES) & set(HR.NAMES)


# ---- GPU ----

@gpu
@pytest.mark.parametrize("name", W.NAMES)
def test_wide_heads_vs_fp64_oracle(name):
    c = HR.BY_NAME[name]
    q = HR.derived(c)
    m = build(c, wide_recurrent=True).cuda()
    f = HR.inputs(name)
    sem, emo = f["semantic"].cuda(), f["emotion"].cuda()
    with torch.no_grad():
        feat = m.get_feature(sem, None, None, emo)
        ln_nd, inst = m(sem, None, None, emo)
    got = dict(feature=feat.cpu(), lnnd=ln_nd.cpu(), inst=inst.cpu())
    ref, _ = HR.ref64(name)
    assert got["feature"].shape == (c.B, c.S, q["feature_width"]) and got["lnnd"].shape == (c.B, c.S, 2) and got["inst"].shape == (c.B, c.S, HR.INSTRUMENTS)
    assert all(torch.isfinite(got[k]).all() for k in HR.OUTPUTS)
    err, bounds = HR.errors(got, ref), HR.bounds(name)
    print(f"\nREG_WIDE_PARITY {name}: " + "  ".join(f"{k} error {err[k]:.2e} bound {bounds[k]:.2e} ratio {err[k] / bounds[k]:.2f}" for k in HR.OUTPUTS))
    for k in HR.OUTPUTS:
        assert 0.0 < bounds[k] <= HR.CAP
    for k in HR.OUTPUTS:
        assert err[k] <= bounds[k], f"{name} {k}: max |got - ref64| / max(1, max |ref64|) = {err[k]:.3e} over the bound {bounds[k]:.3e}"


@gpu
@pytest.mark.parametrize("rm", W.HEADS)
def test_flag_changes_nothing_at_64(rm):
    c = HR.RegCase(f"wide_flag_{rm}_64", rm, 64, 64, W.VF, 2, 5, 2, 3100, frozenset(), "d_model 64 with and without the flag")
    HR.BY_NAME.setdefault(c.name, c)
    f = HR.inputs(c.name)
    sem, emo = f["semantic"].cuda(), f["emotion"].cuda()
    outs = []
    for kw in ({}, dict(wide_recurrent=True)):
        m = build(c, **kw).cuda()
        with torch.no_grad():
            outs.append((m.get_feature(sem, None, None, emo).cpu(), *[t.cpu() for t in m(sem, None, None, emo)]))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("rm", W.HEADS)
@pytest.mark.parametrize("d", [160, 512])
def test_state_dict_is_torchs_module_of_that_width(rm, d):
    m = VideoRegression(n_layers=2, d_model=d, d_hidden=64, total_vf_dim=13, regModel=rm, wide_recurrent=True)
    t = (nn.LSTM if "lstm" in rm else nn.GRU)(d, d, 2, bidirectional="bi" in rm, batch_first=True)
    pre = "model.gru." if rm.startswith("cnn") else "model."
    mine = {k[len(pre):]: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith(pre)}
    assert mine == {k: tuple(v.shape) for k, v in t.state_dict().items()}
    assert set(mine) == {f"{n}_l{l}{s}" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh") for l in range(2) for s in ("", "_reverse")[:2 if "bi" in rm else 1]}


@gpu
@pytest.mark.parametrize("name", list(W.GOLDEN_MODELS))
def test_wide_heads_vs_reference_golden(golden, name):
    g = golden("g_reg_wide.npz")
    cfg = W.GOLDEN_MODELS[name]
    m = VideoRegression(**cfg, **W.GOLDEN_COMMON, wide_recurrent=True).eval()
    assert list(m.state_dict()) == [str(k) for k in g[f"{name}_keys"]]
    m.load_state_dict(W.golden_state_dict(m), strict=True)
    m = m.cuda()
    sem, emo = (t.cuda() for t in W.golden_inputs())
    with torch.no_grad():
        feat = m.get_feature(sem, None, None, emo)
        ln_nd, inst = m(sem, None, None, emo)
    B, S = W.GOLDEN_BS
    assert feat.shape == (B, S, cfg["d_model"] * (2 if name == "bilstm" else 1))
    for got, k in ((feat, "feat"), (ln_nd, "lnnd"), (inst, "inst")):
        err = float(np.abs(got.cpu().numpy() - g[f"{name}_{k}"]).max())
        assert err < 5e-5, (name, k, err)
