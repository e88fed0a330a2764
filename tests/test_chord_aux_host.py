"""The auxiliary chord loss without a GPU: the restatement of tests/helpers_chord_aux.py against the reference's own outputs
(tests/golden/g_train_aux.npz, tools/make_goldens_train_aux.py), wrong readings of the reference that must miss those outputs, the
conditions the inputs of tests/test_chord_aux_loss_gpu.py meet, the three regimes of `count`, the host side of the epoch figures and of
-drop_loss, and the command lines.

Bounds.  The restatement in fp64 and the reference's objects on the logits cast to double are the same expressions: 1e-12 relative.
The reference's fp32 figure of a mean over the valid rows of B clips: `helpers_eval.loss_bound(B L, value)`, a 159-term tree inside a
row followed by a sum over at most B L rows (torch sums the whole batch at once); an auxiliary term times its weight, the combined
value the three bounds over count, plus 4 U of the value for the divisions."""
import random
import re

import numpy as np
import pytest
import torch

from tests import helpers_chord_aux as H
from tests import helpers_eval as HE
from video2music_amd import ops, train, train_families, train_losses, train_v3

G = "g_train_aux.npz"
U = H.U
W = (0.4, 0.6)
RECORDED = [(B, L, form) for (B, L) in H.SHAPES for form in H.LAYOUTS if not (form == "view" and L == 1 and B > 1)]


def bounds32(B, L, want):
    """Bounds of {CE, A_3, A_5, combined} in fp32 from their fp64 values `want` (5,) = those four and count."""
    b = [HE.loss_bound(B * L, want[0]), 3.0 * HE.loss_bound(B * L, want[1] / 3.0), 5.0 * HE.loss_bound(B * L, want[2] / 5.0)]
    b = [v + 4 * U * abs(w) for v, w in zip(b, want)]
    return np.array(b + [sum(b) / want[4] + 4 * U * abs(want[3])])


def restated(y, tgt, emo, s, form, variant=None, grad=False):
    r = H.chord_aux(y, tgt, emo, s, W, form, grad=grad, variant=variant)
    return np.array([r["loss"][3], r["loss"][4], r["loss"][5], r["loss"][1], r["loss"][6]]), r


@pytest.mark.parametrize("B,L,form", RECORDED)
@pytest.mark.parametrize("s", [0.0, 0.1])
def test_restatement_equals_the_reference(golden, B, L, form, s):
    g = golden(G)
    y, tgt, emo = H.make_case(B, L)
    got, _ = restated(y, tgt, emo, s, form)
    w64, w32 = g[f"seed_{B}x{L}_{form}_s{s}_f64"], g[f"seed_{B}x{L}_{form}_s{s}_f32"]
    assert got[4] == w64[4] == w32[4]
    assert (np.abs(got[:4] - w64[:4]) <= 1e-12 * np.abs(w64[:4])).all(), (got, w64)
    assert (np.abs(got[:4] - w32[:4]) <= bounds32(B, L, w64)).all(), (got, w32, bounds32(B, L, w64))


@pytest.mark.parametrize("form", H.LAYOUTS)
def test_restatement_gradient_equals_the_reference(golden, form):
    y, tgt, emo = H.make_case(2, 39)
    yt = torch.from_numpy(y[..., :H.NC].copy()).double().requires_grad_(True)
    H.loss_terms(yt, tgt, emo, 0.1, W, form)["chord"].backward()
    want = golden(G)[f"dlogits64_2x39_{form}"]
    assert H.rel_err(yt.grad.numpy(), want) <= 1e-12


@pytest.mark.parametrize("variant", H.WRONG)
def test_wrong_readings_miss_the_recorded_values(golden, variant):
    """Each by at least 100 times the bound of the recorded fp32 figure, on the view form of (3, 299) -- the training call; `count`
    fixed at 3 shows where the count is not 3."""
    g = golden(G)
    if variant == "count3":
        B, L = H.REGIME_SHAPE
        y, tgt, emo = H.regime_case(2, "view")
        w64, w32 = g["regime2_view_f64"], g["regime2_view_f32"]
    else:
        B, L = 3, 299
        y, tgt, emo = H.make_case(B, L)
        w64, w32 = g[f"seed_{B}x{L}_view_s0.1_f64"], g[f"seed_{B}x{L}_view_s0.1_f32"]
    right, _ = restated(y, tgt, emo, 0.1, "view")
    wrong, _ = restated(y, tgt, emo, 0.1, "view", variant)
    b = bounds32(B, L, w64)[3]
    assert abs(right[3] - w32[3]) <= b
    print(f"{variant}: combined {wrong[3]:.6f} recorded {w32[3]:.6f}, miss / bound {abs(wrong[3] - w32[3]) / b:.0f}")
    assert abs(wrong[3] - w32[3]) >= 100 * b and abs(wrong[3] - w64[3]) >= 100 * b


def test_unview_inverts_the_view():
    rng = np.random.default_rng(0)
    for B, L in ((1, 1), (3, 2), (2, 65), (2, 159)):
        z = rng.standard_normal((B, L, H.NC))
        assert np.array_equal(H.aux_rows(H.unview(z), "view"), z)
        zt = torch.from_numpy(z)
        assert torch.equal(H.aux_rows(H.unview(zt), "view"), zt)
        f = 159 * (L - 1) + 7                             # element j = 7 of the last view row is logits[b, f % L, f // L]
        assert H.aux_rows(z, "view")[0, L - 1, 7] == z[0, f % L, f // L]


@pytest.mark.parametrize("B,L", H.SHAPES)
@pytest.mark.parametrize("layout", H.LAYOUTS)
def test_gpu_cases_stay_away_from_ties_and_from_the_kink(B, L, layout):
    gap, margin = H.conditions(*H.make_case(B, L)[:2], layout)
    print(f"B {B} L {L} {layout}: gap {gap:.3e} margin {margin:.3e}")
    assert gap >= H.MIN_GAP and margin >= H.MIN_MARGIN


def test_a_shape_that_does_not_hold_the_conditions_is_not_among_the_cases():
    assert (4, 159) not in H.SHAPES
    gap = min(H.conditions(*H.make_case(4, 159)[:2], layout)[0] for layout in H.LAYOUTS)
    assert gap < H.MIN_GAP


@pytest.mark.parametrize("layout", H.LAYOUTS)
@pytest.mark.parametrize("count", [3, 2, 1])
def test_count_regimes_are_reached(golden, count, layout):
    g = golden(G)
    y, tgt, emo = H.regime_case(count, layout)
    gap, margin = H.conditions(y, tgt, layout)
    assert gap >= H.MIN_GAP and margin >= H.MIN_MARGIN
    got, _ = restated(y, tgt, emo, 0.1, layout)
    assert got[4] == count
    if count < 3:
        w64 = g[f"regime{count}_{layout}_f64"]
        assert w64[4] == g[f"regime{count}_{layout}_f32"][4] == count
        assert (np.abs(got[:4] - w64[:4]) <= 1e-12 * np.abs(w64[:4])).all()
        assert got[2] == 0.0 and (abs(got[1] - 0.2105) < 1e-4 if count == 2 else got[1] == 0.0)


def test_epoch_figures_are_eval_model_s_per_clip_combination():
    """`train.clip_chord_losses` on the per-clip sums of the rows layout equals the restatement run on every clip alone, as eval_model's
    loader of batch size 1 runs the loss; a clip without a valid target gives NaN; without the switch, the plain quotient."""
    y, tgt, emo = H.make_case(3, 64)
    clip = H.chord_aux(y, tgt, emo, 0.1, W, "rows", grad=False)["clip"]
    got = train.clip_chord_losses(clip, auxiliary=True)
    for b in (0, 2):
        want = H.chord_aux(y[b:b + 1], tgt[b:b + 1], emo[b:b + 1], 0.1, W, "rows", grad=False)["loss"][1]
        assert abs(got[b] - want) <= 1e-12 * abs(want)
    assert np.isnan(got[1]) and np.isnan(train.clip_chord_losses(clip)[1])
    assert np.array_equal(train.clip_chord_losses(clip)[[0, 2]], (clip[:, 1] / clip[:, 0])[[0, 2]])
    # a clip whose hinges are all inactive divides by 1
    y1, t1, e1 = H.regime_case(1, "rows")
    c1 = H.chord_aux(y1, t1, e1, 0.1, W, "rows", grad=False)["clip"]
    assert train.clip_chord_losses(c1, auxiliary=True)[0] == c1[0, 1] / c1[0, 0]
    assert ops.CHORD_AUX_TERMS == H.TERMS and ops.CHORD_AUX_CLIP_FIELDS[:4] == ops.CHORD_LOSS_CLIP_FIELDS


def test_drop_loss_weights_follow_the_draws():
    assert train.drop_loss_weights(0.0) == train.drop_loss_weights(0.5999) == (train.LOSS_LAMBDA, 1 - train.LOSS_LAMBDA)
    assert train.drop_loss_weights(0.6) == train.drop_loss_weights(0.7999) == (1.0, 0.0)
    assert train.drop_loss_weights(0.8) == train.drop_loss_weights(0.9999) == (0.0, 1.0)
    rng = random.Random(3)
    kinds = {train.drop_loss_weights(rng.random()) for _ in range(200)}
    assert len(kinds) == 3


# ---- the command lines ----
BASE = ["-music_gen_version", "None", "-chord_embed", ""]
SYN = ["-chord_embed", "", "--synthetic_weights"]


@pytest.mark.parametrize("flag,reason", [("-auxiliary_loss", "-auxiliary_loss: the top-k auxiliary losses are not built"),
                                         ("-drop_loss", "-drop_loss is not built: every step uses the weighted sum of both losses")])
def test_the_three_old_entries_still_refuse(flag, reason):
    for entry, argv in ((train, BASE), (train_families, ["-music_gen_version", "2.2"] + SYN), (train_v3, ["-music_gen_version", "3.1"] + SYN)):
        with pytest.raises(SystemExit, match=re.escape(reason)):
            entry.main(argv + [flag, "1"])
    args = train.parse_args(BASE + [flag, "1"])
    assert train.refuse(args) == train.refuse(args, ()) == train.refuse(args, (), losses=False) == reason
    assert train.refuse(args, train_v3.TRAINABLE, balancing=True) == reason


@pytest.mark.parametrize("argv", [BASE, ["-music_gen_version", "2.2"] + SYN, ["-music_gen_version", "3.1"] + SYN,
                                  ["-music_gen_version", "2.2", "-balancing", "1"] + SYN])
def test_train_losses_admits_both_switches(argv):
    assert train_losses.TRAINABLE == train_v3.TRAINABLE
    for extra in (["-auxiliary_loss", "1"], ["-drop_loss", "1"], ["-auxiliary_loss", "1", "-drop_loss", "1"], []):
        args = train.parse_args(argv + extra)
        assert args.auxiliary_loss == ("-auxiliary_loss" in extra) and args.drop_loss == ("-drop_loss" in extra)
        assert train.refuse(args, train_losses.TRAINABLE, balancing=True, losses=True) is None


@pytest.mark.parametrize("argv,reason", [
    (BASE + ["-auxiliary_loss", "1", "-augmentation", "1"], r"-augmentation"),
    (BASE + ["-auxiliary_loss", "1", "-optimizer", "Lion"], r"-optimizer Lion"),
    (["-music_gen_version", "2.0", "-drop_loss", "1"] + SYN, r"-music_gen_version 2\.0: .*TopKScheduler"),
    (BASE + ["-drop_loss", "1", "--no_tensorboard", ""], r"tensorboard"),
])
def test_train_losses_refuses_what_is_still_not_built(argv, reason):
    with pytest.raises(SystemExit, match=reason):
        train_losses.main(argv)


def test_chord_train_loss_keeps_its_old_call():
    import inspect
    from video2music_amd import losses
    sig = inspect.signature(losses.chord_train_loss)
    assert list(sig.parameters)[:5] == ["logits", "tgt", "emo_class", "lam", "smoothing"]
    kw = {k: p.default for k, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY}
    assert kw == {"auxiliary": False, "layout": "view", "weights": None}
