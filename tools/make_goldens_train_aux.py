"""Golden fixture for the auxiliary chord loss (-auxiliary_loss), produced by the REFERENCE's own `TopKAuxiliaryLoss` / `CombinedLoss`
(model/loss.py:85-141, built as train.py:224-229 builds them), `VideoMusicTransformer`, `VideoMusicTransformer_V2`, `VevoDataset`,
`train_epoch` and `eval_model`, run on the CPU.

TEST INFRASTRUCTURE.  Only arrays go in: tests/golden/g_train_aux.npz, at most 1 MiB.

Seeded logits (the inputs of tests/test_chord_aux_loss_gpu.py, tests/helpers_chord_aux.py), for every shape BxL of SHAPES, both call
forms -- "view": `loss(y.permute(0, 2, 1), tgt)` as train_epoch calls it, "rows": `loss(y.reshape(B * L, -1), tgt.flatten())` as
eval_model does -- and smoothing s in (0, 0.1):
    seed_<B>x<L>_<form>_s<s>_f32 / _f64   {CE, A_3, A_5, combined, count}: each loss object on its own, then the CombinedLoss, on the
                                          fp32 logits / on the logits cast to double (the combined value of the double run is the sum
                                          of its three components over its count: CombinedLoss itself accumulates in fp32)
    regime<c>_<form>_f32 / _f64           the same five on the count-2 and count-1 inputs of `regime_case` (s = 0.1)
    dlogits64_2x39_<form>                 d combined / d logits in double (s = 0.1)
  The view form of (2, 1) is left out: with L = 1 and B > 1 `mask.squeeze()` broadcasts the (B,) mask against the (B, 1) loss, a
  quirk the library does not reproduce.
Training run, on the miniature dataset and the models of tools/make_goldens_train.py (rpr) and tools/make_goldens_train_families.py
(v22), ce_smoothing 0.1, the combined loss in the chord part:
    <m>_loss / <m>_loss64    {total, chord, emotion} of the first batch of train_epoch's lines, fp32 / in double (rpr: the reference's
                             modules cast to double; v22: the fp64 restatement of tests/helpers_family_train.py)
    <m>_parts                {CE, A_3, A_5, count} of that batch, fp32
    <m>_e32_grad             max over all parameters of max|g_ref32 - g64| / max|g64| (v22: at `helpers_family_train.grad_scale`)
    <m>_grad_<key>           the reference's fp32 gradient of RECORDED (rpr) / V22_KEYS (v22)
    rpr_figs_before / _after, rpr_adam_losses
                             eval_model's figures with eval_loss_func = the combined loss before and after three train_epoch passes
                             with the reference's Adam settings at lr 1e-3, and the training loss before each pass

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_train_aux.py
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_goldens as G                                    # noqa: E402
from tests import helpers_chord_aux as H                                # noqa: E402
from tests import helpers_family_train as FT                            # noqa: E402
from tests import helpers_train as T                                    # noqa: E402
from tools.make_goldens_train import RECORDED                           # noqa: E402
from video2music_amd.utilities import constants as C                    # noqa: E402

V22_KEYS = ("Wout.weight", "Linear_chord.weight", "transformer.decoder.layers.3.norm3.weight", "transformer.decoder.norm.bias",
            "transformer.decoder.layers.0.ff.gate.weight", "transformer.decoder.layers.3.ff.gate.bias",
            "transformer.decoder.layers.2.cross_attn.out_proj.bias", "transformer.encoder.layers.3.ff.shared_expert.linear2.bias")


def main():
    import torch
    torch.set_num_threads(1)                                # one summation order, whatever the machine
    bt = T.batch()
    tmp = tempfile.mkdtemp(prefix="vevo_train_")
    ids = T.write_dataset(tmp)

    def v22_fp64():
        """`FT.run_case` with the combined loss in the chord part (before the reference is imported: it changes the directory)."""
        P = {k: FT.cast(v, torch.float64, True) for k, v in FT.golden_state_dict("v22").items()}
        logits = FT.forward_restated(P, FT.GOLDEN["v22"], FT.golden_inputs(), None, None, (), [], True)
        r = H.loss_terms(logits, bt["tgt"], bt["emo_class"], T.SMOOTHING, (T.LAM, 1 - T.LAM), "view")
        r["total"].backward()
        return (np.array([float(r[k].detach()) for k in ("total", "chord", "emotion")]),
                {k: None if q.grad is None else q.grad.numpy() for k, q in P.items()})
    v22_l64, v22_g64 = v22_fp64()

    ref = G.import_reference()
    from torch.utils.data import DataLoader
    from dataset import vevo_dataset as D
    from model.loss import CombinedLoss, TopKAuxiliaryLoss
    from utilities.constants import ADAM_BETA_1, ADAM_BETA_2, ADAM_EPSILON, LOSS_LAMBDA
    from utilities.run_model_vevo import eval_model, train_epoch
    assert LOSS_LAMBDA == T.LAM == C.LOSS_LAMBDA

    def parts(smoothing):
        return [torch.nn.CrossEntropyLoss(ignore_index=C.CHORD_PAD, label_smoothing=smoothing),
                TopKAuxiliaryLoss(k=3, weight=3.0, vocab_size=C.CHORD_SIZE, ignore_index=C.CHORD_PAD),
                TopKAuxiliaryLoss(k=5, weight=5.0, vocab_size=C.CHORD_SIZE, ignore_index=C.CHORD_PAD)]

    def combined(smoothing):
        return CombinedLoss(parts(smoothing), type="avg")                                   # train.py:224-229

    def call_form(y, tgt, form):
        B, L = tgt.shape
        return (y.permute(0, 2, 1), tgt) if form == "view" else (y.reshape(B * L, -1), tgt.flatten())

    def five(y, tgt, emo, form, smoothing, dtype):
        """{CE, A_3, A_5, combined, count} through the reference's objects on y cast to dtype; with grad: + d combined / dy."""
        yt = torch.from_numpy(np.ascontiguousarray(y[..., :H.NC])).to(dtype).requires_grad_(True)
        t = torch.from_numpy(H.clean_targets(tgt, emo)[0])                                  # an id outside the vocabulary reads as PAD
        args = call_form(yt, t, form)
        vals = [f(*args) for f in parts(smoothing)]
        count = sum(int(v > 1e-10) for v in vals)
        if dtype == torch.float32:
            comb = combined(smoothing)(*args)
        else:
            comb = ((vals[0] + vals[1]) + vals[2]) / count
        comb.backward()
        return np.array([float(v.detach()) for v in vals] + [float(comb.detach()), float(count)]), yt.grad.numpy()

    out = {"ids": np.array(ids)}
    for B, L in H.SHAPES:
        y, tgt, emo = H.make_case(B, L)
        for form in H.LAYOUTS:
            if form == "view" and L == 1 and B > 1:
                continue
            for s in (0.0, 0.1):
                for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
                    vals, grad = five(y, tgt, emo, form, s, dtype)
                    out[f"seed_{B}x{L}_{form}_s{s}_{tag}"] = vals
                    if (B, L) == (2, 39) and s == 0.1 and tag == "f64":
                        out[f"dlogits64_{B}x{L}_{form}"] = grad
    for count in (2, 1):
        for form in H.LAYOUTS:
            y, tgt, emo = H.regime_case(count, form)
            for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
                out[f"regime{count}_{form}_{tag}"] = five(y, tgt, emo, form, 0.1, dtype)[0]
            assert out[f"regime{count}_{form}_f32"][4] == count, (count, form, out[f"regime{count}_{form}_f32"])

    # ---- the training run ----
    ds = D.VevoDataset(dataset_root=tmp + "/", split="test", split_ver="v1", vis_models="2d/clip_l14p", emo_model="6c_l14p", motion_type=0,
                       max_seq_chord=T.S_VIDEO, max_seq_video=T.S_VIDEO, random_seq=True, is_video=True)
    train_loader = DataLoader(ds, batch_size=len(ds), num_workers=0, shuffle=False)          # both clips: one batch per epoch
    eval_loader = DataLoader(ds, batch_size=1, num_workers=0)
    b = next(iter(train_loader))
    for ours, theirs in (("x", "x"), ("x_root", "x_root"), ("x_attr", "x_attr"), ("tgt", "tgt"), ("semantic", "semanticList"), ("key", "key"),
                         ("scene_offset", "scene_offset"), ("motion", "motion"), ("emotion", "emotion")):
        assert np.array_equal(bt[ours], b[theirs].numpy()), ours
    bce = torch.nn.BCEWithLogitsLoss()

    def losses_of(y, double=False):
        """train_epoch's three lines (utilities/run_model_vevo.py:101-119) with the combined loss; double: its components summed in
        double (CombinedLoss accumulates into an fp32 scalar)."""
        args = (y.permute(0, 2, 1), b["tgt"])
        if double:
            vals = [f(*args) for f in parts(T.SMOOTHING)]
            chord = ((vals[0] + vals[1]) + vals[2]) / sum(int(v > 1e-10) for v in vals)
        else:
            chord = combined(T.SMOOTHING).forward(*args)
        emotion = bce.forward(y.permute(0, 2, 1), b["tgt_emotion"].to(y.dtype).permute(0, 2, 1))
        return LOSS_LAMBDA * chord + (1 - LOSS_LAMBDA) * emotion, chord, emotion

    def part_values(y):
        vals = [float(f(y.permute(0, 2, 1), b["tgt"])) for f in parts(T.SMOOTHING)]
        return np.array(vals + [sum(v > 1e-10 for v in vals)])

    def ref_forward(m):
        return m(b["x"], b["x_root"], b["x_attr"], b["semanticList"], b["key"], b["scene_offset"], b["motion"], b["emotion"])

    def first_batch(name, make, keys, fp64, errors):
        m = make().train()
        y = ref_forward(m)
        total, chord, emotion = losses_of(y)
        total.backward()
        g32 = {k: (None if p.grad is None else p.grad.numpy().copy()) for k, p in m.named_parameters()}
        l64, g64 = fp64()
        used = [k for k in g64 if g64[k] is not None and g32.get(k) is not None]
        out[f"{name}_loss"] = np.array([float(v.detach()) for v in (total, chord, emotion)])
        out[f"{name}_loss64"] = np.asarray(l64, dtype=np.float64)
        out[f"{name}_parts"] = part_values(y.detach())
        out[f"{name}_e32_grad"] = np.array(max(errors(g32, {k: g64[k] for k in used}).values()))
        for k in keys:
            out[f"{name}_grad_{k}"] = g32[k].astype(np.float32)
        print(name, "loss", out[f"{name}_loss"], "fp64", out[f"{name}_loss64"], "parts", out[f"{name}_parts"], "e32_grad",
              float(out[f"{name}_e32_grad"]))
        return float(total.detach())

    # rpr: the base model of tools/make_goldens_train.py
    cfg = T.MODELS["rpr"]
    sd = {k: torch.from_numpy(v) for k, v in T.state_dict(cfg).items()}

    def rpr_model():
        m = ref.vmt.VideoMusicTransformer(dropout=0.0, **cfg)
        res = m.load_state_dict(sd, strict=False)
        assert all(k.endswith(".pe") for k in res.missing_keys) and not res.unexpected_keys, res
        return m

    def rpr_fp64():
        """The reference's forward (model/video_music_transformer.py:978-1044) on its own modules in double."""
        m = rpr_model().double().train()
        mask = m.transformer.generate_square_subsequent_mask(b["x"].shape[1]).double()
        x = m.embedding_root(b["x_root"]) + m.embedding_attr(b["x_attr"])
        key = torch.cat([torch.full((1, x.shape[1], 1), b["key"][i, 0].item()) for i in range(x.shape[0])], dim=0).double()
        xf = m.Linear_chord(torch.cat([x, key], dim=-1))
        vfc = torch.cat([b["semanticList"].double(), b["scene_offset"].unsqueeze(-1).double(), b["motion"].unsqueeze(-1).double(),
                         b["emotion"].double()], dim=-1)
        vf = m.Linear_vis(vfc)
        xf, vf = m.positional_encoding(xf.permute(1, 0, 2)), m.positional_encoding_video(vf.permute(1, 0, 2))
        l64 = losses_of(m.Wout(m.transformer(src=vf, tgt=xf, tgt_mask=mask).permute(1, 0, 2)), double=True)
        l64[0].backward()
        return [float(v.detach()) for v in l64], {k: (None if p.grad is None else p.grad.numpy().copy()) for k, p in m.named_parameters()}

    first = first_batch("rpr", rpr_model, RECORDED, rpr_fp64, lambda g32, g64: {k: T.rel_err(g32[k], g) for k, g in g64.items()})
    m = rpr_model()
    figs = lambda: np.array([float(eval_model(m, eval_loader, combined(T.SMOOTHING), bce)[k]) for k in T.FIGURES])
    out["rpr_figs_before"] = figs()
    opt = torch.optim.Adam(m.parameters(), lr=T.ADAM_LR, betas=(ADAM_BETA_1, ADAM_BETA_2), eps=ADAM_EPSILON)
    traj = []
    for e in range(T.ADAM_STEPS):
        with torch.no_grad():
            traj.append(float(losses_of(ref_forward(m.train()))[0]))
        train_epoch(e + 1, m, train_loader, combined(T.SMOOTHING), bce, opt, None, print_modulus=10 ** 9)
    out["rpr_adam_losses"] = np.array(traj)
    out["rpr_figs_after"] = figs()
    assert abs(traj[0] - first) <= 1e-6 * first
    print("rpr adam", traj, dict(zip(T.FIGURES, out["rpr_figs_before"])), "->", dict(zip(T.FIGURES, out["rpr_figs_after"])))

    # v22: the '2.2' model of tools/make_goldens_train_families.py
    sd2 = {k: torch.from_numpy(v) for k, v in FT.golden_state_dict("v22").items()}

    def v22_model():
        m = ref.vmt.VideoMusicTransformer_V2(**dict(FT.golden_kwargs("v22"), chord_embed=False))
        res = m.load_state_dict({k: v for k, v in sd2.items() if k != "chord_embedding_model.weight"}, strict=False)
        assert not res.missing_keys and not res.unexpected_keys, res
        m.chord_embed = True
        m.chord_embedding_model = torch.nn.Embedding.from_pretrained(sd2["chord_embedding_model.weight"].clone(), freeze=True)
        return m

    first_batch("v22", v22_model, V22_KEYS, lambda: (v22_l64, v22_g64), FT.grad_errors)

    path = os.path.join(REPO, "tests", "golden", "g_train_aux.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 2 ** 20


if __name__ == "__main__":
    main()
