"""Eval forward of `VideoRegression` for all thirteen regModels on the HIP kernels against the float64 oracle (`oracle.reg_oracle.forward`,
pinned to the reference class by tests/test_reg_oracle.py), at the kernel-edge shapes of tests/helpers_reg_parity.py: dt ranks 2 .. 32
against the padded dt projection, padded `dbc` row strides, every d_state of 'moemamba', sequence lengths around the scan chunks and
below d_conv, conv7 over clips shorter than its kernel, half rows of 32 and 48 recurrent weights, odd expert widths, one token.

Measure: max |got - ref64| / max(1, max |ref64|), separately over `get_feature`, the (note density, loudness) pair and the instrument
probabilities.  Bound per case and output: 8 x e32, e32 being the same measure of the oracle's float32 run on the CPU (the conditions
are checked by tests/test_reg_parity_host.py; no bound may exceed 1e-4).  The bounds are computed when the test runs: 1.3e-8 .. 1.9e-5
on the MI355X machine's CPU, errors observed there 3.3e-9 .. 1.7e-6, the largest error / bound ratio 0.43 ('bigru' at S = 1, on the
two numbers of the (note density, loudness) pair); apart from that pair in the S = 1 cases no ratio is above 0.2.
"""
import pytest
import torch

from tests import helpers_reg_parity as HR
from video2music_amd.model.video_regression import VideoRegression

pytestmark = pytest.mark.gpu


def build(c):
    m = VideoRegression(**HR.model_kwargs(c)).eval()
    sd = HR.state_dict(c.name)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}, \
        "the key list of helpers_reg_parity.named_shapes is not the class's state dict"
    m.load_state_dict(sd, strict=True)
    return m.cuda()


@pytest.mark.parametrize("name", HR.NAMES)
def test_reg_forward_vs_fp64_oracle(name):
    c = HR.BY_NAME[name]
    q = HR.derived(c)
    m = build(c)
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
    print(f"\nREG_PARITY {name}: " + "  ".join(f"{k} error {err[k]:.2e} bound {bounds[k]:.2e} ratio {err[k] / bounds[k]:.2f}" for k in HR.OUTPUTS))
    for k in HR.OUTPUTS:
        assert 0.0 < bounds[k] <= HR.CAP
    for k in HR.OUTPUTS:
        i = int((got[k].double() - ref[k]).abs().argmax())
        assert err[k] <= bounds[k], (f"{name} [{c.edge}] {k}: max |got - ref64| / max(1, max |ref64|) = {err[k]:.3e} over the bound {bounds[k]:.3e}; worst at flat "
                                     f"index {i} of {tuple(ref[k].shape)}: got {float(got[k].flatten()[i]):.8f}, fp64 {float(ref[k].flatten()[i]):.8f}")
