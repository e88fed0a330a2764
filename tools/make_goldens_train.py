"""Golden fixtures for chord-model training, produced by the REFERENCE's own `VideoMusicTransformer`, `VevoDataset`, `train_epoch`
and `eval_model` run on the CPU over the miniature dataset of tests/helpers_eval.py (both clips in one batch, 300 seconds, 299 chord
positions, motion_type 0), on the two small models of tests/helpers_train.py (rpr=True and rpr=False: 2 layers, 2 heads, d_model 64,
dim_feedforward 128, dropout 0, `video2music_amd.synthetic` weights).

TEST INFRASTRUCTURE.  Only arrays go in.  A committed file may not exceed 1 MiB, so there are three:

tests/golden/g_train.npz -- per model <m> in helpers_train.MODELS:
    <m>_loss / <m>_loss0     {total, chord, emotion} of the first batch with ce_smoothing 0.1 / without: the lines of train_epoch up to
                             backward, through the reference's objects, fp32
    <m>_loss64               the same three with ce_smoothing 0.1 in fp64
    <m>_logits_rows          rows 0, 1, 38, 39, 40, 298 of both clips of the reference's training-state logits, fp32
    <m>_e32_grad             max over ALL parameters of max|g_ref32 - g64| / max|g64|: the noise level of fp32 training arithmetic
    <m>_e32_upd              the same for theta_3 - theta_0 after three SGD steps (lr 0.05)
    <m>_unused               the keys whose .grad stays None on the reference class
    <m>_adam_losses          the training loss before each of three train_epoch passes with the reference's Adam settings at lr 1e-3
    <m>_figs_before/after    eval_model's figures (helpers_train.FIGURES) with the training loss function before and after them
    <m>_grad64_<key>         fp64 gradients of the tensors with at most 5000 values
    plain_grad_<key>         the reference's fp32 gradient of the keys of RECORDED for the model without relative positions
  and once: train_arg_defaults (the reference's `parse_train_args` defaults as a JSON string), csv_header (the CSV_HEADER list of its
  train.py, read from the file's syntax tree: importing train.py would pull in optimisers the tree does not ship), adam (its three
  constants).
tests/golden/g_train_rpr32.npz -- grad_<key>: the reference's fp32 gradient of EVERY parameter of the rpr model.
tests/golden/g_train_rpr64.npz -- grad64_<key>: the fp64 gradient of the keys of helpers_train.FULL64 of the rpr model (Er, one whole
  decoder layer, one encoder layer, Linear_chord, both embeddings, Wout).

The fp64 side is the REFERENCE's own modules cast to double (`model.double()`: embeddings, Linear_chord, Linear_vis, both positional
encodings, `transformer`, Wout), called in the order of its `forward`, whose own text casts the features to float and so cannot run
in double itself.  The restatement of tests/helpers_train.py takes no part in what is recorded; the tests hold it to these arrays.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_train.py
"""
import ast
import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True
import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_goldens as G                                    # noqa: E402
from tests import helpers_eval as HE                                    # noqa: E402
from tests import helpers_train as T                                    # noqa: E402
from video2music_amd.utilities import constants as C                    # noqa: E402

RECORDED = ("transformer.decoder.layers.1.self_attn.in_proj_weight", "transformer.decoder.layers.1.multihead_attn.in_proj_weight",
            "transformer.decoder.layers.1.norm2.weight", "transformer.decoder.layers.1.linear1.weight",
            "transformer.encoder.layers.0.self_attn.in_proj_weight", "transformer.encoder.layers.0.norm1.bias",
            "transformer.encoder.norm.weight", "Linear_chord.weight", "Linear_chord.bias", "Linear_vis.weight", "embedding_root.weight",
            "embedding_attr.weight", "Wout.weight", "Wout.bias")


def main():
    import torch
    torch.set_num_threads(1)                                # one summation order, whatever the machine
    bt = T.batch()
    tmp = tempfile.mkdtemp(prefix="vevo_train_")
    ids = T.write_dataset(tmp)
    ref = G.import_reference()
    from torch.utils.data import DataLoader
    from dataset import vevo_dataset as D
    from utilities.argument_funcs import parse_train_args
    from utilities.constants import ADAM_BETA_1, ADAM_BETA_2, ADAM_EPSILON, LOSS_LAMBDA
    from utilities.run_model_vevo import eval_model, train_epoch
    assert LOSS_LAMBDA == T.LAM == C.LOSS_LAMBDA

    ds = D.VevoDataset(dataset_root=tmp + "/", split="test", split_ver="v1", vis_models="2d/clip_l14p", emo_model="6c_l14p", motion_type=0,
                       max_seq_chord=T.S_VIDEO, max_seq_video=T.S_VIDEO, random_seq=True, is_video=True)
    train_loader = DataLoader(ds, batch_size=len(ds), num_workers=0, shuffle=False)          # both clips: one batch per epoch
    eval_loader = DataLoader(ds, batch_size=1, num_workers=0)
    b = next(iter(train_loader))
    # the project's reader and the reference's dataset agree on every input of this fixture, and on the emotion rows
    for ours, theirs in (("x", "x"), ("x_root", "x_root"), ("x_attr", "x_attr"), ("tgt", "tgt"), ("semantic", "semanticList"), ("key", "key"),
                         ("scene_offset", "scene_offset"), ("motion", "motion"), ("emotion", "emotion")):
        assert np.array_equal(bt[ours], b[theirs].numpy()), ours
    assert np.array_equal(HE.emotion_rows(bt["tgt"], bt["emo_class"]), b["tgt_emotion"].numpy().astype(np.int64))

    out = {"ids": np.array(ids), "train_arg_defaults": np.array(json.dumps(vars(parse_train_args()[0]), sort_keys=True)),
           "adam": np.array([ADAM_BETA_1, ADAM_BETA_2, ADAM_EPSILON])}
    for node in ast.parse(open(os.path.join(G.REF, "train.py")).read()).body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "CSV_HEADER":
            out["csv_header"] = np.array(ast.literal_eval(node.value))
    rpr32, rpr64 = {}, {}

    def loss_funcs(smoothing):
        return torch.nn.CrossEntropyLoss(ignore_index=C.CHORD_PAD, label_smoothing=smoothing), torch.nn.BCEWithLogitsLoss()

    def losses_of(y, smoothing):
        """train_epoch's three lines (utilities/run_model_vevo.py:101-119)."""
        ce, bce = loss_funcs(smoothing)
        chord = ce.forward(y.permute(0, 2, 1), b["tgt"])
        emotion = bce.forward(y.permute(0, 2, 1), b["tgt_emotion"].to(y.dtype).permute(0, 2, 1))
        return LOSS_LAMBDA * chord + (1 - LOSS_LAMBDA) * emotion, chord, emotion

    def forward64(m):
        """The reference's forward (model/video_music_transformer.py:978-1044) on its own modules in double."""
        mask = m.transformer.generate_square_subsequent_mask(b["x"].shape[1]).double()
        x = m.embedding_root(b["x_root"]) + m.embedding_attr(b["x_attr"])
        key = torch.cat([torch.full((1, x.shape[1], 1), b["key"][i, 0].item()) for i in range(x.shape[0])], dim=0).double()
        xf = m.Linear_chord(torch.cat([x, key], dim=-1))
        vfc = torch.cat([b["semanticList"].double(), b["scene_offset"].unsqueeze(-1).double(), b["motion"].unsqueeze(-1).double(),
                         b["emotion"].double()], dim=-1)
        vf = m.Linear_vis(vfc)
        xf, vf = m.positional_encoding(xf.permute(1, 0, 2)), m.positional_encoding_video(vf.permute(1, 0, 2))
        return m.Wout(m.transformer(src=vf, tgt=xf, tgt_mask=mask).permute(1, 0, 2))

    for name, cfg in T.MODELS.items():
        sd = {k: torch.from_numpy(v) for k, v in T.state_dict(cfg).items()}

        def ref_model():
            m = ref.vmt.VideoMusicTransformer(dropout=0.0, **cfg)
            res = m.load_state_dict(sd, strict=False)
            assert all(k.endswith(".pe") for k in res.missing_keys) and not res.unexpected_keys, res
            return m

        def ref_forward(m):
            return m(b["x"], b["x_root"], b["x_attr"], b["semanticList"], b["key"], b["scene_offset"], b["motion"], b["emotion"])

        m = ref_model().train()
        y = ref_forward(m)
        total, chord, emotion = losses_of(y, T.SMOOTHING)
        total.backward()
        g32 = {k: (None if p.grad is None else p.grad.numpy().copy()) for k, p in m.named_parameters()}
        m64 = ref_model().double().train()
        l64 = losses_of(forward64(m64), T.SMOOTHING)
        l64[0].backward()
        g64 = {k: (None if p.grad is None else p.grad.numpy().copy()) for k, p in m64.named_parameters()}
        unused = sorted(k for k, g in g32.items() if g is None)
        assert unused == sorted(T.UNUSED) and unused == sorted(k for k, g in g64.items() if g is None)
        used = [k for k in g64 if g64[k] is not None]
        out[f"{name}_loss"] = np.array([float(total), float(chord), float(emotion)])
        out[f"{name}_loss64"] = np.array([float(v) for v in l64])
        out[f"{name}_loss0"] = np.array([float(v) for v in losses_of(ref_forward(ref_model().train()), 0.0)])
        out[f"{name}_logits_rows"] = y.detach().numpy()[:, T.LOGIT_ROWS].astype(np.float32)
        out[f"{name}_unused"] = np.array(unused)
        out[f"{name}_e32_grad"] = np.array(max(T.rel_err(g32[k], g64[k]) for k in used))
        for k in used:
            if g64[k].size <= 5000:
                out[f"{name}_grad64_{k}"] = g64[k]
            if name == "rpr":
                rpr32[f"grad_{k}"] = g32[k].astype(np.float32)
                if k.startswith(T.FULL64):
                    rpr64[f"grad64_{k}"] = g64[k]
            elif k in RECORDED:
                out[f"{name}_grad_{k}"] = g32[k].astype(np.float32)

        # three SGD steps: the reference's train_epoch in fp32; its modules in double, the same lines
        m = ref_model()
        opt = torch.optim.SGD(m.parameters(), lr=T.SGD_LR)
        for e in range(T.SGD_STEPS):
            train_epoch(e + 1, m, train_loader, *loss_funcs(T.SMOOTHING), opt, None, print_modulus=10 ** 9)
        m64 = ref_model().double().train()
        opt = torch.optim.SGD(m64.parameters(), lr=T.SGD_LR)
        for _ in range(T.SGD_STEPS):
            opt.zero_grad()
            losses_of(forward64(m64), T.SMOOTHING)[0].backward()
            opt.step()
        p32, p64 = dict(m.named_parameters()), dict(m64.named_parameters())
        out[f"{name}_e32_upd"] = np.array(max(T.rel_err(p32[k].detach().double().numpy() - sd[k].double().numpy(),
                                                        p64[k].detach().numpy() - sd[k].double().numpy()) for k in used))

        # three Adam passes at the reference's settings, eval_model's figures (training loss function) on either side
        m = ref_model()
        figs = lambda: np.array([float(eval_model(m, eval_loader, *loss_funcs(T.SMOOTHING))[k]) for k in T.FIGURES])
        out[f"{name}_figs_before"] = figs()
        opt = torch.optim.Adam(m.parameters(), lr=T.ADAM_LR, betas=(ADAM_BETA_1, ADAM_BETA_2), eps=ADAM_EPSILON)
        traj = []
        for e in range(T.ADAM_STEPS):
            with torch.no_grad():
                traj.append(float(losses_of(ref_forward(m.train()), T.SMOOTHING)[0]))
            train_epoch(e + 1, m, train_loader, *loss_funcs(T.SMOOTHING), opt, None, print_modulus=10 ** 9)
        out[f"{name}_adam_losses"] = np.array(traj)
        out[f"{name}_figs_after"] = figs()
        assert abs(traj[0] - float(total)) <= 1e-6 * float(total)
        print(name, "loss", out[f"{name}_loss"], "fp64", out[f"{name}_loss64"], "e32_grad", float(out[f"{name}_e32_grad"]), "e32_upd",
              float(out[f"{name}_e32_upd"]), "adam", traj, dict(zip(T.FIGURES, out[f"{name}_figs_before"])), "->",
              dict(zip(T.FIGURES, out[f"{name}_figs_after"])))
    for fname, arrays in (("g_train.npz", out), ("g_train_rpr32.npz", rpr32), ("g_train_rpr64.npz", rpr64)):
        path = os.path.join(REPO, "tests", "golden", fname)
        np.savez_compressed(path, **arrays)
        print("wrote", fname, len(arrays), "arrays,", os.path.getsize(path), "bytes")
        assert os.path.getsize(path) <= 2 ** 20, fname


if __name__ == "__main__":
    main()
