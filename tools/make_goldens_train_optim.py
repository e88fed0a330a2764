"""Golden fixture for training the base model under RAdam, RAdamW and RAdanW: the recipe of tools/make_goldens_train.py for its Adam
run (the REFERENCE's own `VideoMusicTransformer`, `VevoDataset` and `train_epoch` on the CPU over the miniature dataset of
tests/helpers_eval.py, both clips in one batch, the rpr model of tests/helpers_train.py, dropout 0, lr 1e-3), eight passes per
optimiser with the settings of the reference's train.py:241-248:

    radam    torch.optim.RAdam(betas=(ADAM_BETA_1, ADAM_BETA_2), eps=ADAM_EPSILON)
    radamw   the same with weight_decay=0.01, decoupled_weight_decay=True
    radanw   the reference's model/RAdanW.py, betas (ADAM_BETA_1, ADAM_BETA_2, 0.92, 0.99), weight_decay=0.01, foreach=True passed
             explicitly: the variant its default picks on a GPU (on the CPU the default would pick the other optimiser)

TEST INFRASTRUCTURE.  Only arrays go in.  `model/RAdanW.py` needs `torch.optim.optimizer._dispatch_sqrt`, gone from newer torch
releases: tools/make_goldens_optim.py's stand-in is put there first.

tests/golden/g_train_optim.npz -- per optimiser <o>:
    <o>_losses        (8,) the training loss before each pass, fp32 run (train_epoch itself)
    <o>_losses64      the same of the fp64 run: the reference's modules cast to double, the lines of train_epoch, the same optimiser
    <o>_spread        max over the trained tensors of max|d32 - d64| / max|d64|, d = theta_8 - theta_0: how far the reference's own
                      fp32 arithmetic carries this run from its fp64 one (rectified, sign-like steps turn gradient noise around 0
                      into whole steps)
    <o>_w_<key>       theta_8 of the fp32 run: the whole tensor up to 4096 values, its first 4 rows beyond
  and once: steps, lr, keys (the trained tensors), settings (the constants above).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_train_optim.py
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from oracle import make_goldens as G                                    # noqa: E402
from tests import helpers_train as T                                    # noqa: E402
from video2music_amd.utilities import constants as C                    # noqa: E402

STEPS, WHOLE, ROWS = 8, 4096, 4


def recorded_part(a):
    return a if a.size <= WHOLE else a[:ROWS]


def main():
    import torch
    torch.set_num_threads(1)
    tmp = tempfile.mkdtemp(prefix="vevo_train_")
    T.write_dataset(tmp)
    import make_goldens_optim
    make_goldens_optim.import_radanw()                      # the stand-in, before anything imports model.RAdanW
    ref = G.import_reference()
    from model.RAdanW import RAdanW
    from torch.utils.data import DataLoader
    from dataset import vevo_dataset as D
    from utilities.constants import ADAM_BETA_1, ADAM_BETA_2, ADAM_EPSILON, LOSS_LAMBDA
    from utilities.run_model_vevo import train_epoch
    assert LOSS_LAMBDA == T.LAM == C.LOSS_LAMBDA

    ds = D.VevoDataset(dataset_root=tmp + "/", split="test", split_ver="v1", vis_models="2d/clip_l14p", emo_model="6c_l14p", motion_type=0,
                       max_seq_chord=T.S_VIDEO, max_seq_video=T.S_VIDEO, random_seq=True, is_video=True)
    loader = DataLoader(ds, batch_size=len(ds), num_workers=0, shuffle=False)
    b = next(iter(loader))
    cfg = T.MODELS["rpr"]
    sd = {k: torch.from_numpy(v) for k, v in T.state_dict(cfg).items()}
    b12 = (ADAM_BETA_1, ADAM_BETA_2)
    optimisers = {"radam": lambda ps: torch.optim.RAdam(ps, lr=T.ADAM_LR, betas=b12, eps=ADAM_EPSILON),
                  "radamw": lambda ps: torch.optim.RAdam(ps, lr=T.ADAM_LR, betas=b12, eps=ADAM_EPSILON, weight_decay=0.01,
                                                         decoupled_weight_decay=True),
                  "radanw": lambda ps: RAdanW(ps, lr=T.ADAM_LR, betas=b12 + (0.92, 0.99), eps=ADAM_EPSILON, weight_decay=0.01, foreach=True)}

    def loss_funcs():
        return torch.nn.CrossEntropyLoss(ignore_index=C.CHORD_PAD, label_smoothing=T.SMOOTHING), torch.nn.BCEWithLogitsLoss()

    def total_loss(y):
        ce, bce = loss_funcs()
        chord = ce.forward(y.permute(0, 2, 1), b["tgt"])
        emotion = bce.forward(y.permute(0, 2, 1), b["tgt_emotion"].to(y.dtype).permute(0, 2, 1))
        return LOSS_LAMBDA * chord + (1 - LOSS_LAMBDA) * emotion

    def ref_model():
        m = ref.vmt.VideoMusicTransformer(dropout=0.0, **cfg)
        res = m.load_state_dict(sd, strict=False)
        assert all(k.endswith(".pe") for k in res.missing_keys) and not res.unexpected_keys, res
        return m

    def forward32(m):
        return m(b["x"], b["x_root"], b["x_attr"], b["semanticList"], b["key"], b["scene_offset"], b["motion"], b["emotion"])

    def forward64(m):
        """The reference's forward on its own modules in double (its text casts the features to float)."""
        mask = m.transformer.generate_square_subsequent_mask(b["x"].shape[1]).double()
        x = m.embedding_root(b["x_root"]) + m.embedding_attr(b["x_attr"])
        key = torch.cat([torch.full((1, x.shape[1], 1), b["key"][i, 0].item()) for i in range(x.shape[0])], dim=0).double()
        xf = m.Linear_chord(torch.cat([x, key], dim=-1))
        vfc = torch.cat([b["semanticList"].double(), b["scene_offset"].unsqueeze(-1).double(), b["motion"].unsqueeze(-1).double(),
                         b["emotion"].double()], dim=-1)
        vf = m.Linear_vis(vfc)
        xf, vf = m.positional_encoding(xf.permute(1, 0, 2)), m.positional_encoding_video(vf.permute(1, 0, 2))
        return m.Wout(m.transformer(src=vf, tgt=xf, tgt_mask=mask).permute(1, 0, 2))

    out = {"steps": np.array(STEPS), "lr": np.array(T.ADAM_LR), "settings": np.array([ADAM_BETA_1, ADAM_BETA_2, ADAM_EPSILON, 0.92, 0.99, 0.01])}
    for name, make in optimisers.items():
        m = ref_model()
        opt = make(m.parameters())
        losses = []
        for e in range(STEPS):
            with torch.no_grad():
                losses.append(float(total_loss(forward32(m.train()))))
            train_epoch(e + 1, m, loader, *loss_funcs(), opt, None, print_modulus=10 ** 9)
        m64 = ref_model().double().train()
        opt = make(m64.parameters())
        losses64 = []
        for _ in range(STEPS):
            opt.zero_grad()
            loss = total_loss(forward64(m64))
            losses64.append(float(loss))
            loss.backward()
            opt.step()
        p32, p64 = dict(m.named_parameters()), dict(m64.named_parameters())
        used = [k for k in p64 if k not in T.UNUSED]
        out["keys"] = np.array(used)
        out[f"{name}_losses"], out[f"{name}_losses64"] = np.array(losses), np.array(losses64)
        out[f"{name}_spread"] = np.array(max(T.rel_err(p32[k].detach().double().numpy() - sd[k].double().numpy(),
                                                       p64[k].detach().numpy() - sd[k].double().numpy()) for k in used))
        for k in used:
            out[f"{name}_w_{k}"] = recorded_part(p32[k].detach().numpy().astype(np.float32))
        print(name, "losses", losses, "\n  fp64", losses64, "\n  spread of theta_8 - theta_0:", float(out[f"{name}_spread"]))
    path = os.path.join(REPO, "tests", "golden", "g_train_optim.npz")
    np.savez_compressed(path, **out)
    print("wrote g_train_optim.npz", len(out), "arrays,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 2 ** 20


if __name__ == "__main__":
    main()
