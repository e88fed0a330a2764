"""`loss.backward()` on the base `VideoMusicTransformer` at the shapes where the training path changes kernels
(tests/helpers_train_edges.py; tests/test_train_edges_host.py derives the routes and shows that each case can see the errors it exists
for), against the fp64 restatement of tests/helpers_train.py on the case's own inputs.

Bounds, all computed per case from the restatement's own fp32 run (one CPU thread) against fp64: every gradient within 8 e32 of its
tensor's fp64 maximum (the factor of tests/test_train_gpu.py; a gradient that is identically zero in fp64 is held to the same figure
relative to its attention's in_proj_weight gradient), the training-state logits within 4 e32_y (the decode parity's factor), the loss
within D sum |dL/dy| + 159 U |loss| with D that logits bound in absolute terms."""
import numpy as np
import pytest
import torch

from tests import helpers_eval as HE
from tests import helpers_train as T
from tests import helpers_train_edges as E
from video2music_amd import losses, ops
from video2music_amd.model.video_music_transformer import VideoMusicTransformer
from video2music_amd.utilities import constants as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def build(cfg, sd, dropout=0.0, **kw):
    m = VideoMusicTransformer(dropout=dropout, **dict(cfg, **kw))
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith(".pe") or k.startswith(("scene_embedding", "chord_embedding_model")) for k in missing)
    return m.to(DEV).train()


def logits_of(m, bt, F, causal=True):
    """The module call on the case's feature rows cut into (semantic, scene, motion, emotion), so that ops.concat_features runs."""
    ws = E.feature_widths(F)[0]
    vfc = torch.from_numpy(bt["vfc"]).to(DEV)
    d = lambda k: torch.from_numpy(np.ascontiguousarray(bt[k])).to(DEV)
    return m(d("x"), d("x_root"), d("x_attr"), vfc[..., :ws].contiguous(), d("key"), vfc[..., ws].contiguous(), vfc[..., ws + 1].contiguous(),
             vfc[..., ws + 2:].contiguous(), mask=causal)


def loss_of(y, bt, fused=True):
    if fused:
        return losses.chord_train_loss(y, torch.from_numpy(bt["tgt"]), torch.from_numpy(bt["emo_class"]), T.LAM, T.SMOOTHING)
    rows = torch.from_numpy(HE.emotion_rows(bt["tgt"], bt["emo_class"])).float().to(DEV)
    chord = torch.nn.CrossEntropyLoss(ignore_index=C.CHORD_PAD, label_smoothing=T.SMOOTHING)(y.reshape(-1, C.CHORD_SIZE),
                                                                                               torch.from_numpy(bt["tgt"]).to(DEV).reshape(-1))
    return T.LAM * chord + (1 - T.LAM) * torch.nn.BCEWithLogitsLoss()(y, rows)


def step(m, name, bt, fused=True):
    """One forward + backward from cleared gradients: (logits, loss, {key: gradient or None})."""
    c = E.CASES[name]
    masks = E.masks(name)
    m.dropout_masks = None if masks is None else [torch.from_numpy(a).to(DEV) for a in masks]
    m.zero_grad(set_to_none=True)
    y = logits_of(m, bt, c["cfg"]["total_vf_dim"], c["causal"])
    loss = loss_of(y, bt, fused)
    loss.backward()
    return y.detach(), float(loss.detach()), {k: None if p.grad is None else p.grad.detach().cpu().numpy() for k, p in m.named_parameters()}


@pytest.mark.parametrize("name", list(E.CASES))
def test_loss_logits_and_every_gradient_against_fp64(name):
    c, ref, bt = E.CASES[name], E.reference(name), E.batch(name)
    cfg, B, L = c["cfg"], c["B"], c["L"]
    e32, g64 = ref["e32"], ref["g64"]
    m = build(cfg, E.state_dict(name), dropout=c["p"])
    y, loss, got = step(m, name, bt)
    assert y.shape == (B, L, C.CHORD_SIZE)

    y_err, l_err, l_bound = E.logit_err(y.cpu().numpy(), ref["y64"]), abs(loss - ref["l64"][0]), E.loss_bound(ref)
    errs = E.grad_errors({k: g for k, g in got.items() if g is not None}, g64)
    worst = max(errs, key=errs.get)
    print(f"{name}: e32 {e32:.3e} worst gradient err / e32 = {errs[worst] / e32:.2f} ({worst}); logits err / e32_y = {y_err / ref['e32_y']:.2f}; "
          f"loss {loss:.7f} fp64 {ref['l64'][0]:.7f} err / bound = {l_err / l_bound:.3f}")
    assert y_err <= E.LOGIT_FACTOR * ref["e32_y"], (y_err, ref["e32_y"])
    assert l_err <= l_bound, (loss, ref["l64"][0], l_bound)
    for k, g in g64.items():
        if g is None:
            assert got[k] is None, k                                   # embedding, condition_linear, Wout_root, Wout_attr
        else:
            assert got[k].shape == g.shape and errs[k] <= E.GRAD_FACTOR * e32, (k, errs[k], e32)
    assert sorted(k for k, g in got.items() if g is None) == sorted(T.UNUSED)

    # exact statements
    if cfg["rpr"]:
        for i in range(cfg["n_layers"]):
            dEr = got[f"transformer.decoder.layers.{i}.self_attn.Er"]
            assert not dEr[:cfg["max_sequence_chord"] - L].any()              # the rows of a longer table that the sequence never reads
    if c["p"] > 0:
        assert len(m.last_dropout_masks) == len(E.masks(name)) == 2 + 10 * cfg["n_layers"]
    if c["all_pad"] is not None:
        _, clip, _ = ops.chord_loss(y, torch.from_numpy(bt["tgt"]).to(DEV), torch.from_numpy(bt["emo_class"]).to(DEV), T.LAM, T.SMOOTHING,
                                    backward=False)
        clip = dict(zip(ops.CHORD_LOSS_CLIP_FIELDS, clip[c["all_pad"]].tolist()))
        assert clip["n_valid"] == 0 and clip["ce_sum"] == 0.0 and clip["bce_sum"] > 0 and clip["n_rows"] == L
    y2, loss2, again = step(m, name, bt)
    assert torch.equal(y, y2) and loss == loss2
    assert all((got[k] is None and again[k] is None) or np.array_equal(got[k], again[k]) for k in got)     # same bits twice

    if c["unfused"]:                                                    # torch's loss modules on the same logits
        y3, loss3, got3 = step(m, name, bt, fused=False)
        print(f"  unfused loss {loss3:.7f} err / bound = {abs(loss3 - ref['l64'][0]) / l_bound:.3f}")
        assert torch.equal(y, y3) and abs(loss3 - ref["l64"][0]) <= l_bound
        errs3 = E.grad_errors({k: g for k, g in got3.items() if g is not None}, g64)
        assert max(errs3.values()) <= E.GRAD_FACTOR * e32, max(errs3, key=errs3.get)


@pytest.mark.parametrize("kw,causal,reason", [
    (dict(rpr=True), False, r"training with relative positions is built for the causal mask \(mask=True\) only"),
    (dict(chord_embed=True), True, r"training is built for scene_embed=False, chord_embed=False and the single 159-way head"),
    (dict(scene_embed=True), True, r"training is built for scene_embed=False, chord_embed=False and the single 159-way head")])
def test_what_the_training_path_refuses(kw, causal, reason):
    name = "L64"
    m = build(E.CASES[name]["cfg"], E.state_dict(name), **kw)
    with pytest.raises(NotImplementedError, match=reason):
        logits_of(m, E.batch(name), E.CASES[name]["cfg"]["total_vf_dim"], causal)
