"""Teacher-forced eval forward of every member of the V1 / V2 / V3 families on the HIP kernels against the float64 oracle
(`oracle.amt_oracle.forward_family`, pinned to the reference classes by tests/test_oracle_golden.py), at the route-edge shapes of
tests/helpers_family_parity.py.  The whole batch is compared: for B > 1 the raw views of the rotary and differential attentions
tie the clips together, in the model and in the oracle alike.

Measure: max |got - ref64| / max(1, max |ref64|) over the logits (B, L, 159).  Bound per case: 8 x e32, e32 being the same measure of
the oracle's float32 run on the CPU (the conditions are checked by tests/test_family_parity_host.py; no bound may exceed 1e-4).
Bounds as computed on the CPU of a build machine / of the MI355X machine (the fp32 run's summation order follows the BLAS
threading, which moves e32 by up to 2x) and the errors observed on the MI355X; the largest error / bound ratio is 0.13 (s2_v21):

  case          bound (two machines)  observed      case          bound (two machines)  observed
  s1_v30        5.1e-06 / 5.2e-06   5.1e-07      s3_v134       9.4e-06 / 7.3e-06   7.3e-07
  s1_v31        5.6e-06 / 5.9e-06   4.5e-07      s4_v30        4.3e-06 / 5.5e-06   3.2e-07
  s1_v32        4.6e-06 / 5.4e-06   3.2e-07      s4_v31        5.3e-06 / 5.6e-06   3.8e-07
  s1_v12        1.1e-05 / 1.0e-05   1.3e-06      s4_v32        4.0e-06 / 5.5e-06   3.0e-07
  s1_v11rms     5.4e-06 / 5.5e-06   2.9e-07      s4_v133       4.7e-06 / 5.6e-06   4.4e-07
  s1_v22drop    7.7e-06 / 7.1e-06   8.6e-07      s4_v22ce      5.6e-06 / 5.9e-06   4.8e-07
  s2_v31        5.9e-06 / 4.9e-06   5.3e-07      s4_v13        6.8e-06 / 5.7e-06   6.6e-07
  s2_v12        1.8e-05 / 1.5e-05   1.6e-06      s5_v32        1.5e-06 / 2.4e-06   2.2e-07
  s2_v133       7.0e-06 / 5.7e-06   4.8e-07      s5_v13        4.4e-06 / 7.4e-06   9.3e-07
  s2_v21        9.7e-06 / 6.9e-06   9.0e-07      s5_v20        5.4e-06 / 6.9e-06   6.4e-07
  s3_v30        8.1e-06 / 4.4e-06   4.6e-07      s6_v21nomask  5.5e-06 / 5.3e-06   5.3e-07
  s3_v31        7.0e-06 / 5.7e-06   5.7e-07      s6_v11        7.7e-06 / 5.9e-06   7.5e-07
  s3_v32        5.5e-06 / 3.9e-06   3.2e-07      s6_v10        6.7e-06 / 5.2e-06   5.7e-07
  s3_v20se      8.6e-06 / 8.3e-06   7.3e-07      s6_v134       5.6e-06 / 4.6e-06   5.2e-07
  s3_v10rms     5.3e-06 / 3.7e-06   3.8e-07
"""
import pytest
import torch

from tests import helpers_family_parity as HF
from video2music_amd.model.video_music_transformer import VideoMusicTransformer_V1, VideoMusicTransformer_V2, VideoMusicTransformer_V3

pytestmark = pytest.mark.gpu
CLASSES = {"V1": VideoMusicTransformer_V1, "V2": VideoMusicTransformer_V2, "V3": VideoMusicTransformer_V3}


def build(c):
    m = CLASSES[HF.family_of(c.version)](**HF.model_kwargs(c)).eval()
    sd = HF.state_dict(c.name)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}, \
        "the key list of helpers_family_parity.named_shapes is not the class's state dict"
    m.load_state_dict(sd)
    return m.cuda()


@pytest.mark.parametrize("name", HF.NAMES)
def test_family_forward_vs_fp64_oracle(name):
    c = HF.BY_NAME[name]
    s = HF.SHAPES[c.shape]
    m = build(c)
    f = HF.inputs(name)
    if c.drop:
        m.dropTokenRate = HF.DROP_RATE
        torch.manual_seed(HF.drop_seed(c))                 # the model draws `torch.rand(B, S) > rate` from the default generator
    with torch.no_grad():
        got = m(f["ids"], f["root"], f["attr"], f["semantic"].cuda(), f["key"].cuda(), f["scene_offset"].cuda(), f["motion"].cuda(),
                f["emotion"].cuda(), mask=c.mask).cpu()
    ref, _ = HF.ref64(name)
    assert got.shape == (s.B, s.L, 159) and torch.isfinite(got).all()
    err, bound = HF.rel_err(got, ref), HF.bound(name)
    b, l, j = HF.worst(got, ref)
    print(f"\nFAMILY_PARITY {name}: error {err:.2e}  bound {bound:.2e}  ratio {err / bound:.2f}  max|logit| {float(ref.abs().max()):.1f}")
    assert 0.0 < bound <= HF.CAP
    assert err <= bound, (f"{name} [{c.edge}]: max |got - ref64| / max(1, max |ref64|) = {err:.3e} over the bound {bound:.3e}; worst logit at "
                          f"clip {b}, position {l}, chord {j}: got {float(got[b, l, j]):.6f}, fp64 {float(ref[b, l, j]):.6f}")
