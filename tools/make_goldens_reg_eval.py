"""Golden fixture for the regression evaluation (tests/golden/g_reg_eval.npz), produced by the REFERENCE's own `VevoDataset`,
`VideoRegression` and `utilities/run_model_regression.eval_model` run on the CPU in the build container, over a miniature dataset
written to a temp dir, with `video2music_amd.synthetic` weights.

TEST INFRASTRUCTURE.  The npz holds the content of the miniature dataset (so a test can rebuild the files anywhere), the target
arrays the reference's `createSample` returned at two (max_seq_chord, max_seq_video) pairs, per model ('bilstm' at the reference's
evaluation defaults, 'bimamba+' at d_model 128) the reference model's outputs per clip, its per-clip and average figures and the
per-clip mean of 1 / min(p, 1 - p) over the instrument probabilities, and the defaults of the reference's `parse_eval_args`.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_reg_eval.py
"""
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_goldens as G                                                        # noqa: E402
from tests.helpers_reg_eval import FIGURES, LENGTHS, MODELS, reg_dataset_content, write_reg_dataset   # noqa: E402
from video2music_amd import synthetic                                                       # noqa: E402

CLASSIFIER_SCALE = 1.0      # factor on classifier.0.weight / bias, should the procedural weights give min(p, 1 - p) < 0.01
P_MIN = 0.01


def main():
    import torch
    content = reg_dataset_content()
    tmp = tempfile.mkdtemp(prefix="vevo_reg_eval_")
    write_reg_dataset(tmp, content)
    G.import_reference()                                    # chdirs into the reference tree, stubs off-path modules

    class _Absent:                      # off-path third-party module of model/minGRULM.py, never executed for these regModels
        def __init__(self, *a, **k):
            raise RuntimeError("off-path third-party module is stubbed")
    pkg, sub = types.ModuleType("minGRU_pytorch"), types.ModuleType("minGRU_pytorch.minGRU")
    sub.minGRU, pkg.minGRU = _Absent, sub
    sys.modules["minGRU_pytorch"], sys.modules["minGRU_pytorch.minGRU"] = pkg, sub
    from torch.utils.data import DataLoader, Subset
    from dataset import vevo_dataset as D
    from model.video_regression import VideoRegression
    from utilities.argument_reg_funcs import parse_eval_args
    from utilities.run_model_regression import eval_model

    ids = content["ids"]
    out = {"ids": np.array(ids), "eval_arg_defaults": np.array(json.dumps(vars(parse_eval_args()[0]), sort_keys=True)),
           "classifier_scale": np.array(CLASSIFIER_SCALE)}
    for k, v in content.items():
        if k != "ids":
            out["in_" + k] = v

    class _ShortArgmax:
        """`torch` as dataset/vevo_dataset.py sees it, with arg-max results cut to n entries.  With max_seq_chord < max_seq_video the
        reference's createSample fails in its emotion -> chord-quality table (:491-492 index the max_seq_chord chords with the
        max_seq_video emotion rows), after it has read the regression targets (:381-413,453-459); cutting that loop's iterator lets
        it finish without touching the lines this fixture records."""
        def __init__(self, n):
            self.n = n

        def __getattr__(self, k):
            return getattr(torch, k)

        def argmax(self, t, dim=None):
            return torch.argmax(t, dim=dim)[:self.n]

    def dataset(Tc, Sv):
        D.torch = _ShortArgmax(Tc) if Tc < Sv else torch
        try:
            return D.VevoDataset(dataset_root=tmp + "/", split="test", split_ver="v1", vis_models="2d/clip_l14p", emo_model="6c_l14p",
                                 motion_type=0, max_seq_chord=Tc, max_seq_video=Sv, random_seq=True, is_video=True)
        finally:
            D.torch = torch
    for Tc, Sv in LENGTHS:
        ds = dataset(Tc, Sv)
        for i, fid in enumerate(ids):
            s = ds[i]
            out[f"ref_{fid}_note_density_{Tc}_{Sv}"] = s["note_density"].numpy()
            out[f"ref_{fid}_loudness_{Tc}_{Sv}"] = s["loudness"].numpy()
            out[f"ref_{fid}_instrument_{Tc}_{Sv}"] = np.asarray(s["instrument"]).astype(np.float32)

    ds = dataset(300, 300)
    sem_dim = ds[0]["semanticList"].shape[1]
    for name, cfg in MODELS.items():
        torch.manual_seed(0)
        m = VideoRegression(n_layers=cfg["n_layers"], d_model=cfg["d_model"], d_hidden=cfg["dim_feedforward"], use_KAN=False,
                            max_sequence_video=300, total_vf_dim=sem_dim + 6, regModel=cfg["regModel"]).eval()
        shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
        sd = {k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(shapes, seed=0).items()}
        for k in ("classifier.0.weight", "classifier.0.bias"):
            sd[k] = sd[k] * CLASSIFIER_SCALE
        m.load_state_dict(sd, strict=True)
        for i, fid in enumerate(ids):
            s = ds[i]
            with torch.no_grad():
                ln_nd, inst = m(s["semanticList"][None], s["scene_offset"][None], s["motion"][None], s["emotion"][None])
            p = inst[0].numpy().astype(np.float64)
            sharp = np.minimum(p, 1 - p)
            assert sharp.min() >= P_MIN, (name, fid, float(sharp.min()), "raise CLASSIFIER_SCALE's divisor")
            out[f"{name}_{fid}_ln_nd"], out[f"{name}_{fid}_inst"] = ln_nd[0].numpy(), inst[0].numpy()
            out[f"{name}_{fid}_mean_inv_sharp"] = np.array((1.0 / sharp).mean())
            res = eval_model(m, DataLoader(Subset(ds, [i]), batch_size=1, num_workers=0))        # one clip: its own figures
            out[f"{name}_{fid}_figures"] = np.array([float(v) for v in res])
            print(name, fid, dict(zip(FIGURES, res)), "min sharp", float(sharp.min()), "mean 1/sharp", float((1.0 / sharp).mean()))
        res = eval_model(m, DataLoader(ds, batch_size=1, num_workers=0))
        out[f"{name}_avg_figures"] = np.array([float(v) for v in res])
        print(name, "avg", dict(zip(FIGURES, res)))
    np.savez_compressed(os.path.join(REPO, "tests", "golden", "g_reg_eval.npz"), **out)
    print("wrote g_reg_eval.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
