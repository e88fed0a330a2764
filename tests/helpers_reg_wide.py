"""Cases and fixtures of the wide recurrent regression heads (`VideoRegression(..., wide_recurrent=True)`, d_model above 128 on
csrc/rnn_wide.hip), shared by tests/test_reg_wide_gpu.py and tools/make_goldens_reg_wide.py.  Nothing here imports the HIP library.

Parity cases: all six recurrent heads at d_model 160 (the first width above the register kernels' cap, no multiple of 64) and 256, two
layers (layer 1 of a bidirectional head reads 2 d_model columns), B = 2 clips, S = 1 (no recurrent term: the first step's predicate) and
S = 5, thirteen features.  They are entered into helpers_reg_parity's name table, so that its state dicts, inputs, float64 / float32
oracle runs, error measure and bounds (8 x e32) serve them unchanged; the seeds are the first from 3001 on -- all of them, as it turned
out -- whose bounds lie in (0, CAP] and above four float32 roundings of the output (test_reg_parity_host.py's conditions, which
test_reg_wide_gpu.py repeats on the CPU)."""
import numpy as np
import torch

from tests import helpers_reg_parity as HR
from video2music_amd import synthetic

HEADS = ("lstm", "bilstm", "gru", "bigru", "cnngru", "cnnbigru")
WIDTHS = (160, 256)
FRAMES = (1, 5)
D_HIDDEN, VF, CLIPS, LAYERS = 64, 13, 2, 2


def _cases():
    out, seed = [], 3001
    for rm in HEADS:
        for d in WIDTHS:
            for S in FRAMES:
                name = f"wide_{rm}_{d}_{CLIPS}x{S}_L{LAYERS}"
                out.append(HR.RegCase(name, rm, d, D_HIDDEN, VF, CLIPS, S, LAYERS, seed, frozenset({"skinny", "tile64"}),
                                      f"d_model {d} on the wide recurrence kernels, S = {S}"))
                seed += 1
    return out


CASES = _cases()
NAMES = [c.name for c in CASES]
for _c in CASES:                        # helpers_reg_parity looks its cases up by name; CASES / NAMES there (the other suites' table) stay as they are
    assert HR.BY_NAME.setdefault(_c.name, _c) is _c

# ---- the fixture from the reference's own class (tests/golden/g_reg_wide.npz holds its outputs only) ----
GOLDEN_MODELS = {"bilstm": dict(regModel="bilstm", d_model=160, n_layers=1), "cnngru": dict(regModel="cnngru", d_model=160, n_layers=1)}
GOLDEN_COMMON = dict(d_hidden=64, total_vf_dim=VF)
GOLDEN_SEED = 5
GOLDEN_BS = (2, 5)


def golden_state_dict(module):
    """The procedural weights of video2music_amd.synthetic for `module`'s own key list, as the other make_goldens_* tools fix them."""
    shapes = [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
    return {k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(shapes, seed=GOLDEN_SEED).items()}


def golden_inputs():
    """semantic (2, 5, 7) ~ N(0, 1), emotion (2, 5, 6) softmax rows."""
    B, S = GOLDEN_BS
    rs = np.random.RandomState(77)
    sem = rs.standard_normal((B, S, VF - HR.EMO_DIM)).astype(np.float32)
    z = rs.standard_normal((B, S, HR.EMO_DIM))
    e = np.exp(z - z.max(-1, keepdims=True))
    return torch.from_numpy(sem), torch.from_numpy((e / e.sum(-1, keepdims=True)).astype(np.float32))
