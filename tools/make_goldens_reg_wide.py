"""Golden fixture of the wide recurrent regression heads (tests/golden/g_reg_wide.npz), produced by the REFERENCE's own
`VideoRegression` run on the CPU in the build container: regModel 'bilstm' and 'cnngru' at d_model 160, one layer, on the 2 x 5 input and
with the procedural weights of tests/helpers_reg_wide.py.  The file holds the reference's outputs only (get_feature, the (note density,
loudness) pair, the instrument probabilities, and the key list of its state dict); the test rebuilds weights and inputs from their seeds.

TEST INFRASTRUCTURE.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_reg_wide.py
"""
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_goldens as G                                                        # noqa: E402
from tests import helpers_reg_wide as W                                                     # noqa: E402


def main():
    import torch
    G.import_reference()                                    # chdirs into the reference tree, stubs off-path modules

    class _Absent:                      # off-path third-party module of model/minGRULM.py, never executed for these regModels
        def __init__(self, *a, **k):
            raise RuntimeError("off-path third-party module is stubbed")
    pkg, sub = types.ModuleType("minGRU_pytorch"), types.ModuleType("minGRU_pytorch.minGRU")
    sub.minGRU, pkg.minGRU = _Absent, sub
    sys.modules["minGRU_pytorch"], sys.modules["minGRU_pytorch.minGRU"] = pkg, sub
    from model.video_regression import VideoRegression

    sem, emo = W.golden_inputs()
    out = {}
    for name, cfg in W.GOLDEN_MODELS.items():
        torch.manual_seed(0)
        m = VideoRegression(n_layers=cfg["n_layers"], d_model=cfg["d_model"], d_hidden=W.GOLDEN_COMMON["d_hidden"], use_KAN=False,
                            max_sequence_video=300, total_vf_dim=W.GOLDEN_COMMON["total_vf_dim"], regModel=cfg["regModel"]).eval()
        m.load_state_dict(W.golden_state_dict(m), strict=True)
        with torch.no_grad():
            feat = m.get_feature(sem, None, None, emo)
            ln_nd, inst = m(sem, None, None, emo)
        out[f"{name}_keys"] = np.array(list(m.state_dict()))
        out[f"{name}_feat"], out[f"{name}_lnnd"], out[f"{name}_inst"] = feat.numpy(), ln_nd.numpy(), inst.numpy()
        print(name, {k: tuple(out[f"{name}_{k}"].shape) for k in ("feat", "lnnd", "inst")})
    path = os.path.join(REPO, "tests", "golden", "g_reg_wide.npz")
    np.savez_compressed(path, **out)
    print("wrote g_reg_wide.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
