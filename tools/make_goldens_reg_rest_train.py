"""Golden fixture for training the five regression heads behind `VideoRegression.enable_training()` -- 'mamba', 'mamba+', 'moemamba',
'cnngru', 'cnnbigru' -- (tests/golden/g_reg_rest_train.npz, g_reg_rest_train_b.npz, g_reg_rest_train_64.npz), produced by the REFERENCE's own
`VideoRegression`, `VevoDataset`, `train_epoch` and `eval_model` run on the CPU in the build container: the recipe of
tools/make_goldens_reg_mamba_train.py -- the miniature dataset of tests/helpers_reg_eval.py (both clips in one batch, S = 300),
`video2music_amd.synthetic` weights, dropout 0.0 and, as tools/make_goldens_reg_moe_train.py does, every nn.Dropout of the constructed
reference model set to p = 0 (the experts bring their own 0.1) -- for the models of tests/helpers_reg_rest_train.MODELS.

TEST INFRASTRUCTURE.  Only arrays go in.  Per model:

    <m>_loss               the first batch's training loss (the lines of train_epoch up to backward, through the reference's objects)
    <m>_grad_<key>         every parameter's gradient after that backward (fp32; the reference's parallel scan)
    <m>_e32_grad           max over parameters of max|g_ref32 - g64| / max|g64|: the noise level of fp32 training arithmetic
    <m>_e32_upd            the same for the update theta_3 - theta_0 after three train_epoch passes with torch.optim.SGD(lr = 0.05)
    <m>_figs_before/after  eval_model's four figures before and after three train_epoch passes with the reference's Adam settings
                           at lr = 1e-3
    <m>_loss64             the first batch's loss of the fp64 restatement

    <m>_min_gap            the smallest gate gap of the fp64 restatement at the first batch and the three SGD steps (inf: no mixture)

g64 is the restatement of tests/helpers_reg_rest_train.py in double (the scan as the plain sequential recurrence, torch's own
autograd) sharing the state dict; the reference casts to float, so fp64 cannot pass through it.  The full fp64 gradients of the
one-layer models 'moemamba' and 'cnnbigru' (<m>_grad64_<key>) go to the second file, so that each stays under the size a fixture may
have.  The weights' seed per model is tests/helpers_reg_rest_train.SEEDS: the first at which every gate gap above is >= GAP (asserted).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_reg_rest_train.py
"""
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_goldens as G                                                        # noqa: E402
from tests.helpers_reg_eval import FIGURES, reg_dataset_content, write_reg_dataset           # noqa: E402
from tests import helpers_reg_rest_train as T                                              # noqa: E402
from video2music_amd import synthetic                                                       # noqa: E402

MAX_BYTES = 1 << 20
SECOND_FILE = ("moemamba_64", "cnngru", "cnnbigru")      # their arrays go to g_reg_rest_train_b.npz: each file stays under MAX_BYTES


def main():
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    torch.set_num_threads(1)                                # one summation order, whatever the machine
    content = reg_dataset_content()
    tmp = tempfile.mkdtemp(prefix="vevo_reg_rest_train_")
    write_reg_dataset(tmp, content)
    G.import_reference()                                    # chdirs into the reference tree, stubs off-path modules

    class _Absent:                      # off-path third-party module of model/minGRULM.py, never executed for these regModels
        def __init__(self, *a, **k):
            raise RuntimeError("off-path third-party module is stubbed")
    pkg, sub = types.ModuleType("minGRU_pytorch"), types.ModuleType("minGRU_pytorch.minGRU")
    sub.minGRU, pkg.minGRU = _Absent, sub
    sys.modules["minGRU_pytorch"], sys.modules["minGRU_pytorch.minGRU"] = pkg, sub
    from torch.utils.data import DataLoader
    from dataset import vevo_dataset as D
    from model.video_regression import VideoRegression
    from utilities.constants import ADAM_BETA_1, ADAM_BETA_2, ADAM_EPSILON
    from utilities.run_model_regression import eval_model, train_epoch

    ds = D.VevoDataset(dataset_root=tmp + "/", split="test", split_ver="v1", vis_models="2d/clip_l14p", emo_model="6c_l14p",
                       motion_type=0, max_seq_chord=300, max_seq_video=300, random_seq=True, is_video=True)
    train_loader = DataLoader(ds, batch_size=len(ds), num_workers=0, shuffle=False)         # both clips: one batch per epoch
    eval_loader = DataLoader(ds, batch_size=1, num_workers=0)
    batch = next(iter(train_loader))
    sem_dim = batch["semanticList"].shape[2]
    inputs = {"sem": batch["semanticList"].numpy().astype(np.float32), "emo": batch["emotion"].numpy().astype(np.float32),
              "note_density": batch["note_density"].numpy().astype(np.float32), "loudness": batch["loudness"].numpy().astype(np.float32),
              "instrument": batch["instrument"].numpy().astype(np.float32)}
    out, out64 = {"ids": np.array(content["ids"]), **inputs}, {}
    data = [inputs[k] for k in ("sem", "emo", "note_density", "loudness", "instrument")]

    def loss_of(ln_nd, inst, b):
        tgt = torch.cat((b["note_density"].float().flatten().reshape(-1, 1), b["loudness"].float().flatten().reshape(-1, 1)), dim=1)
        return nn.SmoothL1Loss()(ln_nd.reshape(-1, 2), tgt) + F.binary_cross_entropy(inst, b["instrument"].float())

    for name, cfg in T.MODELS.items():
        def ref_model():
            m = VideoRegression(n_layers=cfg["n_layers"], d_model=cfg["d_model"], d_hidden=cfg["dim_feedforward"], dropout=0.0,
                                use_KAN=False, max_sequence_video=300, total_vf_dim=sem_dim + 6, regModel=cfg["regModel"])
            for mod in m.modules():                         # the experts of 'moemamba' are built with a Dropout(0.1) of their own
                if isinstance(mod, nn.Dropout):
                    mod.p = 0.0
            if sd is not None:
                m.load_state_dict(sd, strict=True)
            return m
        sd = None
        shapes = [(k, tuple(v.shape)) for k, v in ref_model().state_dict().items()]
        for seed in range(16):                             # the first seed whose gate gaps hold must be the recorded one
            sd_np = synthetic.synthetic_state_dict(shapes, seed=seed)
            routings = []
            o64 = T.model_grads(sd_np, cfg["regModel"], cfg["n_layers"], *data)
            upd64 = T.sgd_updates(sd_np, T.SGD_STEPS, T.SGD_LR, cfg["regModel"], cfg["n_layers"], *data, routings=routings)
            gap = T.min_gap([o64["routing"]] + routings)
            print(name, "seed", seed, "min gate gap", gap)
            if gap >= T.GAP:
                break
        assert gap >= T.GAP and seed == T.SEEDS[name], (name, seed, gap, "set tests/helpers_reg_rest_train.SEEDS to the first seed that holds")
        out[f"{name}_min_gap"] = np.array(gap)
        sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}

        # first batch: the lines of train_epoch up to backward, through the reference's objects
        m = ref_model().train()
        ln_nd, inst = m(batch["semanticList"], batch["scene_offset"], batch["motion"], batch["emotion"])
        loss = loss_of(ln_nd, inst, batch)
        loss.backward()
        g32 = {k: p.grad.numpy().copy() for k, p in m.named_parameters()}
        g64 = o64["grads"]
        assert list(g32) == list(sd) and set(g64) == set(sd)
        out[f"{name}_loss"], out[f"{name}_loss64"] = np.array(float(loss)), np.array(o64["loss"])

        # three SGD passes: the reference's train_epoch; the restatement's own loop
        m = ref_model()
        opt = torch.optim.SGD(m.parameters(), lr=T.SGD_LR)
        for e in range(T.SGD_STEPS):
            train_epoch(e + 1, m, train_loader, nn.SmoothL1Loss(), opt, None, print_modulus=10 ** 9)
        upd32 = {k: (p.detach() - sd[k]).numpy() for k, p in m.named_parameters()}

        out[f"{name}_e32_grad"] = np.array(max(T.rel_err(g32[k], g64[k]) for k in g64))
        out[f"{name}_e32_upd"] = np.array(max(T.rel_err(upd32[k], upd64[k]) for k in g64))
        assert float(out[f"{name}_e32_grad"]) < 1e-3, (name, "fp32 and fp64 disagree: a routing decision differs or the restatement is wrong")
        for k in g64:
            out[f"{name}_grad_{k}"] = g32[k].astype(np.float32)
            if name in T.FULL64:
                out64[f"{name}_grad64_{k}"] = g64[k]

        # three Adam passes at the reference's settings, eval_model's figures on either side
        m = ref_model()
        out[f"{name}_figs_before"] = np.array([float(v) for v in eval_model(m, eval_loader)])
        opt = torch.optim.Adam(m.parameters(), lr=T.ADAM_LR, betas=(ADAM_BETA_1, ADAM_BETA_2), eps=ADAM_EPSILON)
        for e in range(T.ADAM_STEPS):
            train_epoch(e + 1, m, train_loader, nn.SmoothL1Loss(), opt, None, print_modulus=10 ** 9)
        out[f"{name}_figs_after"] = np.array([float(v) for v in eval_model(m, eval_loader)])
        print(name, "loss", float(loss), o64["loss"], "e32_grad", float(out[f"{name}_e32_grad"]), "e32_upd", float(out[f"{name}_e32_upd"]),
              dict(zip(FIGURES, out[f"{name}_figs_before"])), "->", dict(zip(FIGURES, out[f"{name}_figs_after"])))
    second = {k: out.pop(k) for k in list(out) if k.startswith(tuple(n + "_" for n in SECOND_FILE))}
    for fname, arrays in (("g_reg_rest_train.npz", out), ("g_reg_rest_train_b.npz", second), ("g_reg_rest_train_64.npz", out64)):
        path = os.path.join(REPO, "tests", "golden", fname)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        print("wrote", fname + ":", len(arrays), "arrays,", size, "bytes")
        assert size <= MAX_BYTES, (fname, size)


if __name__ == "__main__":
    main()
