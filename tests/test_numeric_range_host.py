"""The numeric-range recipes of tests/helpers_numeric_range.py judged on the CPU, before any kernel is: every recipe reaches the regime
it names (in fp64), its bound max(8 e32, n U) from the fp32 reference alone stays under CAP = 1e-3 with everything finite, and a
deliberately wrong fp32 variant misses the bound on the recipe that exists for it."""
import numpy as np
import pytest
import torch

from tests import helpers_numeric_range as R


def under_cap(w64, w32, n_of, tag, vanish=0.0):
    for k in w64:
        assert np.isfinite(w64[k]).all() and np.isfinite(w32[k]).all(), (tag, k)
    c = R.caps(w64, w32, n_of, vanish)
    print(tag, " ".join(f"{k} {v:.1e}" for k, v in c.items()))
    assert max(c.values()) <= R.CAP, (tag, c)
    return c


# ---- A. softmax-shaped ----------------------------------------------------------------------------------------------------------

def head_scores(recipe, Lq=77, Lk=300, hd=64):
    a, _ = R.attn_recipe(recipe, 1, 2, Lq, Lk, hd)
    return a, R.attn_scores64(a, 2, 1, hd)


@pytest.mark.parametrize("recipe", R.ATTN_RECIPES)
def test_attention_recipe_reaches_its_regime(recipe):
    a, s = head_scores(recipe)
    tiles = np.stack([s[..., j0:j0 + R.KEY_TILE].max(-1) for j0 in range(0, s.shape[-1], R.KEY_TILE)], -1)      # (B, H, Lq, tiles)
    if recipe == "ramp_up":
        assert np.diff(tiles, axis=-1).min() >= 4.0                   # every key tile raises the running maximum: alpha <= e^-4
    elif recipe == "ramp_down":
        assert np.diff(tiles, axis=-1).max() <= -4.0 and np.exp(tiles[..., -1] - tiles[..., 0]).max() < R.U
    elif recipe == "offset60":
        assert 55.0 < s.min() and s.max() < 65.0 and s.std() > 0.8
    elif recipe == "neg90":
        assert np.exp(s).max() < 1e-38                                # exp(s) itself underflows
    elif recipe == "onehot":
        j = 2 * 77 // 3
        assert s[..., j].min() > 95.0 and np.abs(np.delete(s, j, axis=-1)).max() < 1.0 and j >= R.KEY_TILE


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("shape", R.ATTN_FWD_SHAPES)
@pytest.mark.parametrize("recipe", R.ATTN_RECIPES)
def test_attention_forward_bound_is_under_the_cap(recipe, shape, causal):
    Lq, Lk, hd, kernel = shape
    w64, w32 = R.attn_fwd_refs(recipe, Lq, Lk, hd, kernel, causal)
    under_cap(w64, w32, lambda k: Lk + hd, f"{recipe} {shape} causal {causal}")


@pytest.mark.parametrize("case", R.ATTN_TRAIN_CASES)
@pytest.mark.parametrize("recipe", R.ATTN_RECIPES)
def test_attention_training_bound_is_under_the_cap(recipe, case):
    H, Lq, Lk, hd, g, causal, rpr, mask = case
    w64, w32 = R.attn_train_refs(recipe, *case)
    under_cap(w64, w32, R.attn_train_n(H, Lq, Lk, hd, g), f"{recipe} {case}", R.VANISH)


@pytest.mark.parametrize("recipe", R.ATTN_RECIPES)
def test_rpr_prefill_bound_is_under_the_cap(recipe):
    """The forward alone keeps `onehot` at 100: from the key on, every other probability of a row is e^-100, 0 in fp32."""
    H, L, hd = R.RPR_PREFILL
    under_cap(*R.rpr_prefill_refs(recipe), lambda k: L + hd, f"rpr prefill {recipe}")
    if recipe == "onehot":
        a, _ = R.attn_recipe(recipe, 1, H, L, L, hd, 1, 1, 0)
        s = R.attn_scores64(a, H, 1, hd)
        j = 2 * L // 3
        gap = np.delete(s, j, axis=-1).max() + 5.0 - s[..., j].min()           # 5: the most the N(0,1) relative-position term moves a pair
        assert s[..., j].min() > 95.0 and np.exp(gap) < R.FLT_MIN               # below the smallest normal number: __expf returns 0


PLAIN_TRAIN_SHAPES = [(2, 77, 130, 32), (2, 130, 300, 64), (2, 77, 77, 32)]          # the training cases' (H, Lq, Lk, hd)


def flash_dq_over_bound(onehot, H, Lq, Lk, hd):
    a, _ = R.attn_recipe("onehot", 1, H, Lq, Lk, hd, onehot=onehot)
    w64, w32 = (R.attn_train_torch_cpu(a, None, H, 1, 1, dt)["q"] for dt in (torch.float64, torch.float32))
    return R.rel_err(R.attn_bwd_flash_f32(a, H, 1), w64) / R.bound(R.rel_err(w32, w64), Lk + hd)


def test_onehot_of_the_training_cases_is_the_largest_the_flash_backward_holds():
    """dq of the documented formulation (D = rowsum(dO o O)) against max(8 e32, n U) down the ladder: it holds at ONEHOT_TRAIN on every
    shape and misses on some shape at every rung above.  Measured err / bound at (77, 130, 32), (130, 300, 64), (77, 77, 32):
    100: 3.1, 1.9, 7.2;  50: 1.6, 0.9, 3.6;  35: 1.1, 0.7, 2.6;  25: 0.8, 0.5, 1.9;  17.5: 0.4, 0.8, 0.4."""
    table = {m: [flash_dq_over_bound(m, *s) for s in PLAIN_TRAIN_SHAPES] for m in R.ONEHOT_LADDER}
    print({m: [round(v, 2) for v in row] for m, row in table.items()})
    assert R.ONEHOT_TRAIN == R.ONEHOT_LADDER[-1] and max(table[R.ONEHOT_TRAIN]) < 1.0
    assert all(max(table[m]) > 1.0 for m in R.ONEHOT_LADDER[:-1])
    a, _ = R.attn_recipe("onehot", 1, 2, 77, 130, 32, onehot=R.ONEHOT_TRAIN)
    s = R.attn_scores64(a, 2, 1, 32)
    assert np.exp(s - s.max(-1, keepdims=True)).sum(-1).max() < 1 + 1e-5            # still one-hot: the other keys sum to under 1e-5


def softmax_variant(recipe, variant):
    """-> ({o, lse, p} errors of the fp32 variant, of the right fp32 online softmax, both against fp64) on head 0."""
    a, s = head_scores(recipe)
    s, v = s[0, 0], a["v"].reshape(1, 300, 2, 64)[0, :, 0]
    want = dict(zip(("o", "lse", "p"), R.softmax_rows_f64(s, v)))
    err = lambda got: {k: R.rel_err(g, want[k]) for k, g in zip(("o", "lse", "p"), got)}
    return err(R.softmax_rows_f32(s, v, variant)), err(R.softmax_rows_f32(s, v))


@pytest.mark.parametrize("recipe", R.ATTN_RECIPES)
def test_the_online_softmax_restatement_holds_the_bound(recipe):
    _, ok = softmax_variant(recipe, "ok")
    print(recipe, ok)
    assert max(ok.values()) <= 364 * R.U                              # n U alone, n = Lk + hd


def test_softmax_without_the_maximum_is_not_finite_on_neg90():
    wrong, _ = softmax_variant("neg90", "no_max")
    assert wrong["o"] == float("inf")                                 # every exp(s) is flushed to 0: 0 / 0


def test_softmax_without_the_maximum_survives_offset60():
    """exp(64) = 6e27 is far below the largest fp32 number (3.4e38): without the maximum subtracted `offset60` stays finite and as exact as
    with it, so it cannot be the recipe that shows this error (an offset of 89 would be, and is outside the fp32 reference's own
    range).  `neg90` above and the chord loss's `offset1000` below do show it."""
    wrong, ok = softmax_variant("offset60", "no_max")
    print("offset60 without the maximum:", wrong, "with:", ok)
    assert np.isfinite(wrong["o"]) and wrong["o"] <= R.bound(ok["o"], 364)


def test_rescaling_o_but_not_l_misses_ramp_up():
    wrong, ok = softmax_variant("ramp_up", "l_not_rescaled")
    assert wrong["o"] > 100 * R.bound(ok["o"], 364), (wrong, ok)


def test_lse_without_the_maximum_misses_offset60():
    wrong, ok = softmax_variant("offset60", "lse_log_l")
    assert wrong["lse"] > 100 * R.bound(ok["lse"], 364) and wrong["p"] > 100 * R.bound(ok["p"], 364), (wrong, ok)


@pytest.mark.parametrize("treatment", R.LOGIT_TREATMENTS)
def test_chord_logit_treatments(treatment):
    y, tgt, emo, _ = R.chord_logits(treatment)
    top = y.max(-1)
    if treatment == "offset1000":
        assert y.min() > 900
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(y, dtype=np.float32)
            assert np.isnan(e / e.sum(-1, keepdims=True)).all()       # softmax without the maximum: inf / inf
    elif treatment == "spread30":
        assert y.std() > 25 and top.min() - y.min() > 88.7            # the far classes underflow
    elif treatment == "target_minus80":
        valid = (tgt >= 0) & (tgt < 157)
        assert np.allclose((top - np.take_along_axis(y, np.where(valid, tgt, 0)[..., None], -1)[..., 0])[valid], 80.0, atol=1e-4)
    elif treatment == "emotion100":
        assert (y > 88.7).any() and (y < -88.7).any()
    for smoothing in (0.0, 0.1):
        w64, w32 = R.chord_refs(treatment, smoothing)
        under_cap(w64, w32, R.chord_n(2, 5), f"{treatment} smoothing {smoothing}")


AUX_CASES = [(r, layout) for r in R.AUX_RECIPES for layout in ("rows", "view")]


def aux_rows_of(recipe, layout):
    """The valid auxiliary rows z (rows, 159) of the case and their targets."""
    from tests import helpers_chord_aux as HA
    y, tgt, emo = R.chord_aux_case(recipe, layout)
    t, _ = HA.clean_targets(tgt, emo)
    valid = t != HA.C.CHORD_PAD
    return HA.aux_rows(y, layout)[valid], t[valid]


@pytest.mark.parametrize("recipe,layout", AUX_CASES)
def test_chord_aux_recipe(recipe, layout):
    """Every case stays away from a tie at the top-k border and from the hinge's kink by floors derived from the fp32 spacing at its
    logits' magnitude, reaches what it is named for, and `count` is the same in both precisions."""
    from tests import helpers_chord_aux as HA
    assert HA.LAYOUTS == ("rows", "view")
    y, tgt, emo = R.chord_aux_case(recipe, layout)
    assert y.shape == HA.REGIME_SHAPE + (HA.NC,) and y.dtype == np.float32
    gap, margin = HA.conditions(y, tgt, layout)
    gap_floor, margin_floor = R.chord_aux_floors(y)
    print(recipe, layout, f"gap {gap:.2e} (floor {gap_floor:.1e}) margin {margin:.2e} (floor {margin_floor:.1e})")
    assert gap >= gap_floor and margin >= margin_floor
    z, t = aux_rows_of(recipe, layout)
    s = -np.sort(-z.astype(np.float64), axis=-1)
    if recipe == "ties_inside":
        assert (s[:, 0] == s[:, 1]).all() and (s[:, 3] == s[:, 4]).all() and (s[:, 1] > s[:, 2]).all() and len(z) > 40
    elif recipe.startswith("count_flip_guard"):
        assert y.min() > 980
    for smoothing in (0.0, 0.1):
        w64, w32 = R.chord_aux_refs(recipe, layout, smoothing)
        want = {"count_flip_guard2": 2, "count_flip_guard1": 1}.get(recipe, 3)
        assert w64["count"][0] == w32["count"][0] == want
        if want < 3:                                                  # the inactive hinges: exactly 0 in both precisions
            for k in ("loss_aux5", "clip_a5") + (("loss_aux3", "clip_a3") if want == 1 else ()):
                assert not w64[k].any() and not w32[k].any(), k
        under_cap(w64, w32, R.chord_aux_n(*HA.REGIME_SHAPE), f"chord_aux {recipe} {layout} smoothing {smoothing}")


@pytest.mark.parametrize("layout", ["rows", "view"])
def test_second_softmax_without_its_maximum_is_not_finite_on_offset1000(layout):
    z, t = aux_rows_of("offset1000", layout)
    for i, k in ((4, 3), (5, 5)):
        want = R.chord_aux_refs("offset1000", layout, 0.0)[0]["clip_" + R.AUX_CLIP[i]].sum()
        ok, wrong = R.aux_hinge_sum_f32(z, t, k), R.aux_hinge_sum_f32(z, t, k, "no_max")
        assert abs(ok - want) <= R.bound(0.0, 159 + len(z)) * want and not np.isfinite(wrong)        # inf / inf


@pytest.mark.parametrize("layout", ["rows", "view"])
def test_top_k_chosen_on_the_underflowed_probabilities_cannot_miss(layout):
    """The second wrong variant the auxiliary loss was to be shown against, and why it is dropped: on `spread30` most of a row's
    probabilities underflow to 0 and tie there, yet choosing the k largest on the rounded p gives the sums choosing on the logits gives,
    bit for bit.  p is a non-decreasing function of the logit, so the k largest p are the p of the k largest logits as a multiset, ties
    included: the hinge's value cannot tell the two apart on any input."""
    z, t = aux_rows_of("spread30", layout)
    with np.errstate(under="ignore"):
        p = np.exp((z - z.max(-1, keepdims=True)).astype(np.float32))
    assert ((p < R.FLT_MIN).sum(-1) >= 20).all()                      # 20 or more of a row's 159 classes are flushed to 0 and tie there
    for k in (3, 5):
        assert R.aux_hinge_sum_f32(z, t, k, "topk_of_p") == R.aux_hinge_sum_f32(z, t, k) > 0


# ---- B. selective scan ----------------------------------------------------------------------------------------------------------

def scan_facts(recipe, B, L, ED, N=16):
    c = R.scan_recipe(recipe, B, L, ED, N)
    v = (c["draw"] + c["dt_bias"]).double()
    delta = torch.nn.functional.softplus(v)
    return c, v, delta


@pytest.mark.parametrize("shape", R.SCAN_SHAPES)
@pytest.mark.parametrize("recipe", R.SCAN_RECIPES)
def test_scan_recipe_reaches_its_regime(recipe, shape):
    scan_regime(recipe, shape, 16)


def scan_regime(recipe, shape, N):
    B, L, ED = shape
    c, v, delta = scan_facts(recipe, B, L, ED, N)
    A = -torch.exp(c["A_log"].double())
    if recipe == "slow_decay":
        assert float(torch.exp(delta.max() * A.min()) ** 32) > 0.9
    elif recipe == "fast_decay":
        a32 = torch.exp(torch.nn.functional.softplus(c["draw"] + c["dt_bias"])[:, :, None] * -torch.exp(c["A_log"]))
        assert not a32.any() and 0.5 < float(delta.min()) and float(delta.max()) < 1.5
    elif recipe == "threshold":
        assert ((v > 20) & (v < 20.001 + 1e-6)).any() and ((v < 20) & (v > 19.999 - 1e-6)).any() and (v == 20).any() and (v == 88).any()
        assert sorted(set(np.round(v.numpy().reshape(-1), 3))) == sorted(np.round(R.SOFTPLUS_GRID, 3))
    elif recipe == "tiny_delta":
        assert (v[:, 1::2] == -30).all() and float(delta[:, 1::2].max()) < 1e-12
        assert not np.log(np.float32(1) + np.exp(np.float32(-30), dtype=np.float32))      # 0 in fp32 without log1p
    elif recipe == "gate_saturated":
        z = c["xz"][:, ED:]
        assert (z > 59).any() and (z < -59).any() and float(z.abs().min()) > 59


@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("shape", R.SCAN_SHAPES)
@pytest.mark.parametrize("recipe", R.SCAN_RECIPES)
def test_scan_bound_is_under_the_cap(recipe, shape, reverse, version):
    B, L, ED = shape
    w64, w32 = R.scan_refs(recipe, B, L, ED, 16, version, reverse)
    under_cap(w64, w32, R.scan_n(B, L, 16), f"{recipe} {shape} reverse {reverse} version {version}", R.SCAN_VANISH)


def test_scan_wide_state_bound_is_under_the_cap():
    w64, w32 = R.scan_refs("slow_decay", 1, 70, 40, 64, 1, 0, False)
    under_cap(w64, w32, R.scan_n(1, 70, 64), "slow_decay N = 64")


@pytest.mark.parametrize("shape", R.SCAN_SHAPES)
@pytest.mark.parametrize("carry", ["zero", "neighbour"])
def test_a_wrong_carried_state_misses_slow_decay(carry, shape):
    B, L, ED = shape
    c = R.scan_recipe("slow_decay", B, L, ED)
    y64 = R.scan_state_np(c, B, L, ED, 16, np.float64)
    b = R.bound(R.rel_err(R.scan_state_np(c, B, L, ED, 16, np.float32), y64), L * 16)
    assert R.rel_err(R.scan_state_np(c, B, L, ED, 16, np.float64, carry), y64) > 100 * b        # the carried state is O(1) of the result
    assert R.rel_err(R.scan_state_np(c, B, L, ED, 16, np.float32, carry), y64) > 100 * b


def test_softplus_variants():
    f = np.float32
    assert np.isinf(R.softplus_f32(f(88 + 1), "no_threshold")) and R.softplus_f32(f(89)) == f(89)
    c = R.scan_recipe("tiny_delta", 2, 33, 24)
    y64 = R.scan_state_np(c, 2, 33, 24, 16, np.float64)
    ok, wrong = (R.scan_state_np(c, 2, 33, 24, 16, np.float32, softplus=s) for s in ("ok", "no_log1p"))
    odd = lambda y: y[:, 1::2]
    b = R.bound(R.rel_err(odd(ok), odd(y64)), 33 * 16)
    assert b <= R.CAP and R.rel_err(odd(wrong), odd(y64)) > 100 * b and R.rel_err(odd(wrong), odd(y64)) == 1.0     # the state stays 0
    assert R.rel_err(wrong, y64) <= R.bound(R.rel_err(ok, y64), 33 * 16)              # judged as one tensor it would go unseen


@pytest.mark.parametrize("N", R.SCAN_WIDE_N)
@pytest.mark.parametrize("shape", R.SCAN_SHAPES)
@pytest.mark.parametrize("recipe", R.SCAN_RECIPES)
def test_scan_wide_recipe_reaches_its_regime(recipe, shape, N):
    scan_regime(recipe, shape, N)


@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("N", R.SCAN_WIDE_N)
@pytest.mark.parametrize("shape", R.SCAN_SHAPES)
@pytest.mark.parametrize("recipe", R.SCAN_RECIPES)
def test_scan_wide_training_bound_is_under_the_cap(recipe, shape, N, reverse, version):
    """The largest bounds are the n U floor of the state chains at N = 256, n = L N: 5.0e-4 at L = 33; at L = 70 it would be 1.07e-3,
    over the cap, and `scan_n` holds n at CAP / U there: the case runs, against the cap itself."""
    B, L, ED = shape
    assert R.scan_n(B, L, N)("y") == min(L * N, int(R.CAP / R.U)) and R.scan_n(B, L, N)("dD") == B * L
    w64, w32 = R.scan_refs(recipe, B, L, ED, N, version, reverse)
    under_cap(w64, w32, R.scan_n(B, L, N), f"{recipe} {shape} N {N} reverse {reverse} version {version}", R.SCAN_VANISH)


@pytest.mark.parametrize("shape", R.SCAN_SHAPES)
@pytest.mark.parametrize("carry", ["zero", "neighbour"])
def test_a_wrong_carried_state_misses_slow_decay_at_32_states(carry, shape):
    B, L, ED = shape
    c = R.scan_recipe("slow_decay", B, L, ED, 32)
    y64 = R.scan_state_np(c, B, L, ED, 32, np.float64)
    b = R.bound(R.rel_err(R.scan_state_np(c, B, L, ED, 32, np.float32), y64), L * 32)
    assert b <= R.CAP and R.rel_err(R.scan_state_np(c, B, L, ED, 32, np.float32, carry), y64) > 100 * b


@pytest.mark.parametrize("N", R.SCAN_WIDE_N)
@pytest.mark.parametrize("shape", R.SCAN_SHAPES)
def test_a_state_slice_left_out_of_the_sum_misses(shape, N):
    """y's state sum over the first N - 16 states only, what a lost partial of the wide kernels' slice sum leaves."""
    B, L, ED = shape
    for recipe in ("slow_decay", "fast_decay"):
        c = R.scan_recipe(recipe, B, L, ED, N)
        y64 = R.scan_state_np(c, B, L, ED, N, np.float64)
        b = R.bound(R.rel_err(R.scan_state_np(c, B, L, ED, N, np.float32), y64), R.scan_n(B, L, N)("y"))
        miss = R.rel_err(R.scan_state_np(c, B, L, ED, N, np.float32, slices_left_out=1), y64) / b
        print(f"{recipe} {shape} N {N}: one slice left out, err / bound = {miss:.1f}")
        assert b <= R.CAP and miss > (100 if recipe == "slow_decay" else 1)


# ---- C. gates --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("recipe,G,n_dirs", R.RNN_CASES)
def test_rnn_recipe(recipe, G, n_dirs):
    rnn_regime(recipe, G, n_dirs, R.RNN_SHAPE[2])


@pytest.mark.parametrize("recipe,G,n_dirs,d", R.RNN_WIDE_CASES)
def test_rnn_wide_recipe(recipe, G, n_dirs, d):
    """The recipes at the wide kernels' widths.  Largest bounds: `xproj30` and `cell_ramp` 6.5e-5; `whh2` 6.8e-4 at d = 160 and 9.1e-4 at
    256 (GRU, two directions), under the cap."""
    assert d > 128 and d % 32 == 0                                    # past ops.RNN_NARROW_MAX, whole 32-column tiles
    rnn_regime(recipe, G, n_dirs, d)                                  # xproj30: exp(v) / (1 + exp(v)) is NaN at every width


def rnn_regime(recipe, G, n_dirs, d):
    xproj, w_hh, b_hh, dy = R.rnn_recipe(recipe, G, n_dirs, R.RNN_SHAPE[0], d)
    w64, w32 = R.rnn_refs(recipe, G, n_dirs, d)
    if recipe == "xproj30":
        assert xproj.max() > R.EXP_OVERFLOW and xproj.min() < -R.EXP_OVERFLOW
        assert np.isnan(R.sigmoid_f32(xproj, "exp_over")).any() and np.isfinite(R.sigmoid_f32(xproj)).all()       # inf / inf
    elif recipe == "whh2":                                # W_hh h alone saturates the gates, on both sides
        h = w64["y"].reshape(-1, n_dirs, d)
        pre = np.einsum("rgd,mrd->mrg", w_hh.astype(np.float64), h)
        assert pre.max() > R.SATURATED and pre.min() < -R.SATURATED
    elif recipe == "cell_ramp":
        L = R.rnn_len(recipe)
        xp = xproj.reshape(2, L, n_dirs, G, d).astype(np.float64)
        low = 30.0 - (np.abs(w_hh).sum(-1).max() + np.abs(b_hh).max())         # |h| < 1: the least an i, f or g pre-activation can be
        assert (xp[:, :, :, :3] == 30.0).all() and 1 / (1 + np.exp(-low)) > 1 - 1e-6 and np.tanh(low) > 1 - 1e-6
        # so c_t >= t (1 - 1e-5): the cell grows like t, and from t = 10 on tanh(c) is 1 to 1e-8 and y_t = sigmoid(o_t)
        step = lambda t, r: t if r == 0 else L - 1 - t                        # the direction's t-th step
        y = w64["y"].reshape(2, L, n_dirs, d)
        for r in range(n_dirs):
            for t in (10, L - 1):
                o_pre = xp[:, step(t, r), r, 3]
                slack = np.abs(w_hh[r, 3 * d:]).sum(-1) + np.abs(b_hh[r, 3 * d:])
                lo, hi = 1 / (1 + np.exp(-(o_pre - slack))), 1 / (1 + np.exp(-(o_pre + slack)))
                assert ((y[:, step(t, r), r] >= lo * (1 - 1e-7)) & (y[:, step(t, r), r] <= hi)).all()
            assert np.abs(y[:, step(0, r), r]).max() < np.tanh(1.0) + 1e-6    # while at the first step c = 1
        assert np.abs(w64["dxproj"]).max() > 1e-2
    return under_cap(w64, w32, R.rnn_n(recipe, G, d=d), f"{recipe} G {G} dirs {n_dirs} d {d}")


@pytest.mark.parametrize("M,N,K,act,resid", R.ACT_CASES)
def test_activation_epilogue_inputs(M, N, K, act, resid):
    x, w, b, r = R.act_inputs(M, N, K, act, resid)
    w64, w32 = R.act_run(x, w, b, r, act, torch.float64), R.act_run(x, w, b, r, act, torch.float32)
    pre = w64.pop("pre")
    w32.pop("pre")
    assert pre.max() > 100 and pre.min() < -100
    assert np.isnan(R.sigmoid_f32(pre, "exp_over")).any()
    under_cap(w64, w32, lambda k: K, f"act {act} N {N} resid {resid}")


# ---- D. row statistics -----------------------------------------------------------------------------------------------------------

NORM_CASES = [(kind, recipe, shape, resid) for kind in R.NORM_KINDS for recipe in R.norm_recipes_for(kind) for shape in R.NORM_SHAPES
              for resid in (False, True) if resid or recipe != "cancel"]


@pytest.mark.parametrize("kind,recipe,shape,resid", NORM_CASES)
def test_norm_recipe(kind, recipe, shape, resid):
    rows, dim = shape
    a = R.norm_recipe(recipe, rows, dim, resid)
    u = a["x"].astype(np.float64) + (a["resid"].astype(np.float64) if resid else 0.0)
    if recipe.startswith("ladder"):
        m = float(recipe[6:])
        assert np.allclose(np.abs(u.mean(1)) / u.std(1), m, rtol=2e-2)
    elif recipe == "constant":
        assert not u.std(1).any()
    elif recipe == "tiny":
        assert u.var(1).max() < 1e-30
    elif recipe.startswith("huge"):
        assert u.std(1).min() > (5e11 if recipe == "huge12" else 5e14)
    elif recipe == "spike":
        assert np.allclose(np.abs(u).max(1), 1e4, rtol=1e-6) and np.median(np.abs(u)) < 1.0
    elif recipe == "cancel":
        assert np.abs(a["x"]).min() > 0.5 * R.BIG and np.allclose(u.std(1), 1.0, atol=1e-2) and np.abs(u.mean(1)).max() < 1e-2
        assert np.array_equal((a["x"] + a["resid"]).astype(np.float64), u)            # the fp32 sum is exact
    w64, w32 = R.norm_refs(kind, recipe, rows, dim, resid)
    under_cap(w64, w32, R.norm_n(rows, dim), f"{kind} {recipe} {shape} resid {resid}")


@pytest.mark.parametrize("shape", R.NORM_SHAPES)
def test_one_pass_variance_misses_ladder512(shape):
    rows, dim = shape
    a = R.norm_recipe("ladder512", rows, dim, False)
    w64, w32 = R.norm_refs("layernorm", "ladder512", rows, dim, False)
    b = R.bound(R.rel_err(w32["y"], w64["y"]), max(rows, dim))
    assert R.rel_err(R.layernorm_one_pass_f32(a["x"], a["w"], a["b"]), w64["y"]) > 4 * b
    a = R.norm_recipe("ladder8", rows, dim, False)                    # and goes unseen near unit scale
    w64, w32 = R.norm_refs("layernorm", "ladder8", rows, dim, False)
    assert R.rel_err(R.layernorm_one_pass_f32(a["x"], a["w"], a["b"]), w64["y"]) < 1e-4


@pytest.mark.parametrize("shape", R.NORM_SHAPES)
def test_statistics_of_x_alone_miss_the_cancelling_pair(shape):
    rows, dim = shape
    a = R.norm_recipe("cancel", rows, dim, True)
    w64, w32 = R.norm_refs("layernorm", "cancel", rows, dim, True)
    wrong = R.norm_run("layernorm", a, torch.float32, stats_of_x_alone=True)
    for k in ("y", "dx"):
        assert R.rel_err(wrong[k], w64[k]) > 100 * R.bound(R.rel_err(w32[k], w64[k]), max(rows, dim)), k


@pytest.mark.parametrize("shape", R.SUBLN_SHAPES)
@pytest.mark.parametrize("recipe", R.SUBLN_RECIPES)
def test_subln_bound_is_under_the_cap(recipe, shape):
    o1, o2, w = R.subln_inputs(recipe, *shape)
    under_cap(R.subln_run(o1, o2, w, torch.float64), R.subln_run(o1, o2, w, torch.float32), lambda k: shape[1], f"diff_subln {recipe} {shape}")


@pytest.mark.parametrize("shape", R.SUBLN_BWD_SHAPES)
@pytest.mark.parametrize("recipe", R.SUBLN_BWD_RECIPES)
def test_subln_backward_recipe(recipe, shape):
    """o1 - lam o2 is the recipe's row; every bound of y, d_o1, d_o2, dw and dlambda is under the cap (the largest, 7.9e-5, is the 8 n U
    of `constant`'s exactly-zero dlambda; 9.8e-6 at 1e12)."""
    rows, hd = shape
    o1, o2, w, dy = R.subln_bwd_inputs(recipe, rows, hd)
    a = R.norm_recipe(recipe, rows, hd, True)
    u = o1.astype(np.float64) - R.SUBLN_LAM * o2.astype(np.float64)
    assert np.array_equal(u, a["x"].astype(np.float64) + a["resid"].astype(np.float64)) and hd in (32, 64, 128)
    w64, w32 = R.subln_bwd_refs(recipe, rows, hd)
    assert w64["dlambda"].shape == (1,)
    if recipe == "constant":                                          # o2 = 0: dlambda = -sum du o2 is exactly 0
        assert not o2.any() and not u.std(1).any() and w64["dlambda"][0] == 0.0 and w32["dlambda"][0] == 0.0
    elif recipe == "cancel":                                          # o1 and lam o2 at 1e4, their difference a unit row; dlambda at 1e5 .. 1e6
        assert np.abs(o1).min() > 0.5 * R.BIG and np.allclose(u.std(1), 1.0, atol=5e-2) and 1e4 < abs(w64["dlambda"][0]) < 1e7
    elif recipe == "huge12":
        assert u.std(1).min() > 5e11
    under_cap(w64, w32, R.subln_bwd_n(rows, hd), f"diff_subln backward {recipe} {shape}")


def test_subln_backward_at_1e15_is_past_the_fp32_reference():
    """Why `huge` is `huge12` here: at rows of 1e15 torch's own fp32 autograd of the written-out sub-norm is percents to tenths off fp64
    in d_o1, d_o2 and dlambda (ms^-3/2 underflows, as in the RMSNorm), and 8 e32 is far over the cap."""
    for rows, hd in R.SUBLN_BWD_SHAPES:
        o1, o2, w = R.subln_inputs("huge", rows, hd)
        dy = R.norm_recipe("huge", rows, hd, True)["dy"]
        w64, w32 = (R.subln_run(o1, o2, w, dt, grads=True, dy=dy) for dt in (torch.float64, torch.float32))
        e = {k: R.rel_err(w32[k], w64[k]) for k in ("d_o1", "d_o2", "dlambda")}
        print((rows, hd), e)
        assert 8 * min(e.values()) > 10 * R.CAP


@pytest.mark.parametrize("shape", R.SUBLN_BWD_SHAPES)
def test_statistics_of_o1_alone_miss_the_cancelling_pair_of_the_subln(shape):
    rows, hd = shape
    o1, o2, w, dy = R.subln_bwd_inputs("cancel", rows, hd)
    w64, w32 = R.subln_bwd_refs("cancel", rows, hd)
    wrong = R.subln_run(o1, o2, w, torch.float32, grads=True, dy=dy, stats_of_o1_alone=True)
    n = R.subln_bwd_n(rows, hd)
    for k in ("y", "d_o1", "d_o2", "dw"):
        assert R.rel_err(wrong[k], w64[k]) > 100 * R.bound(R.rel_err(w32[k], w64[k]), n(k)), k


@pytest.mark.parametrize("m", R.FOLD_LADDER)
def test_fold_bounds_are_under_the_cap(m):
    """The folded forms' bound is 8 x the fp32 evaluation of (raw - mu g) rstd + c; the fused LayerNorm's 8 x the unfolded fp32.  At
    mean / std = 4096 the first is 2.6e-4 and 8 x it over the cap: the ladder ends at 512."""
    f = R.fold_inputs(m, 5, 64)
    assert m == 0 or np.allclose(np.abs(f["u"].mean(1)) / f["u"].std(1), m, rtol=2e-2)
    for fn, how in ((R.fold_decode_outputs, "folded32"), (R.fold_ffn_outputs, "folded32"), (R.fold_linear_outputs, "unfolded32")):
        under_cap(fn(m, "ref64"), fn(m, how), lambda k: R.FOLD_K, f"{fn.__name__} mean/std {m}")


@pytest.mark.parametrize("case", R.MOE_CASES)
def test_moe_gate_times_100(case):
    from tests import helpers_moe_train as TMoe
    n_tok, d, raw, n_exp, k = case
    x, dout, P, o64, o32 = R.moe_recipe(*case)
    assert o64["gap"] >= TMoe.GAP and np.array_equal(o64["idx"], o32["idx"])
    assert (o64["weights"].max(1) > 1 - 1e-6).mean() > 0.8            # (1, 0, ..) on most tokens
    t64 = lambda a: torch.from_numpy(a).double()
    for pre, rows in [(f"experts.{e}.", (o64["idx"] == e).any(1)) for e in range(n_exp)] + [("shared_expert.", np.ones(n_tok, dtype=bool))]:
        if rows.any():                                                # the gate branch on the rows the expert is given
            g = t64(x[rows]) @ t64(P[pre + "gate.weight"]).T + t64(P[pre + "gate.bias"])
            assert float(g.abs().max()) > R.EXP_OVERFLOW, pre
            if pre == "shared_expert.":
                assert float(g.max()) > R.EXP_OVERFLOW and float(g.min()) < -R.EXP_OVERFLOW
                assert np.isnan(R.sigmoid_f32(g.numpy(), "exp_over")).any()
    under_cap(R.moe_tensors(o64), R.moe_tensors(o32), R.moe_n(n_tok, d, raw, k), f"moe {case}")


@pytest.mark.parametrize("case", R.MOE_CASES)
def test_moe_gate_times_100_with_a_selection_bias(case):
    """The bias moves at least a quarter of the rows to another expert set, the biased k-th versus (k+1)-th gap stays above the floor
    (relative to the largest selection value: helpers_moe_train.GAP, and never under 8 d U, eight times what an fp32 dot product of
    length d loses at that magnitude), fp32 picks fp64's experts in fp64's order, and weights from logits + bias miss."""
    from tests import helpers_moe_train as TMoe
    from tests import helpers_v3_train as V
    n_tok, d, raw, n_exp, k = case
    x, dout, P, bias, o64, o32 = R.moe_biased_recipe(*case)
    assert sorted(R.MOE_BIAS_ORDER) == list(range(n_exp)) and sorted(V.BIAS_ORDER) == list(range(6)) and bias.dtype == np.float32
    assert np.array_equal(np.sort(bias), np.sort(bias)[::-1] * -1)                   # a ramp, permuted
    print(f"moe bias {case}: flipped {o64['flipped']:.2f} gap {o64['gap']:.2e}")
    assert o64["flipped"] >= 0.25 and o64["gap"] >= max(TMoe.GAP, 8 * d * R.U)
    assert np.array_equal(o64["idx"], o32["idx"])
    n_of = R.moe_n(n_tok, d, raw, k)
    c = under_cap(R.moe_tensors(o64), R.moe_tensors(o32), n_of, f"moe biased {case}")
    wrong = R.moe_tensors(R.moe_biased_grads(x, dout, P, bias, n_exp, k, torch.float32, weights_biased=True))
    for name in ("weights", "out"):
        assert R.rel_err(wrong[name], R.moe_tensors(o64)[name]) > 100 * c[name], name


@pytest.mark.parametrize("case", R.GLU_CASES)
def test_glu_gate_times_40(case):
    n, d, dff, silu = case
    sd, a = R.glu_recipe(*case)
    w, b = (sd["0.weight"], sd["0.bias"]) if silu else (sd["gate.weight"], sd["gate.bias"])
    pre = a["x"].astype(np.float64) @ w.astype(np.float64).T + b
    assert pre.max() > R.EXP_OVERFLOW and pre.min() < -R.EXP_OVERFLOW and np.isnan(R.sigmoid_f32(pre, "exp_over")).any()
    under_cap(*R.glu_refs(*case), lambda k: max(n, dff), f"glu {case}")


def test_regression_head_on_slow_decay_weights():
    sd, sem, emo = R.reg_slow_case()
    assert R.REG_SLOW_BS[1] == 2 * 64 + 1                             # three 64-row blocks of the forward scan
    under_cap(*R.reg_slow_refs(), lambda k: R.REG_SLOW_BS[1] * 16, "VideoRegression bimamba+ slow_decay")
