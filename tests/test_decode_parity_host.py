"""Input conditions of the base decode step's parity cases (tests/helpers_decode_parity.py), on the CPU: the case table reaches every
edge it is there for, the teacher-forced sequences hold every id, each case can see the errors it exists for (a wrong root id, an Er
row off by one -- in fp64, at a reduced length for the two long cases), the fp32 restatement that sets the bound is sound, and row t
of the causal forward is what the step computes at position t."""
import pytest
import torch

from oracle import amt_oracle as O
from tests import helpers_decode_parity as P
from tests.helpers import CFG1, feats_t, synthetic_sd
from video2music_amd import synthetic
from video2music_amd.utilities import constants as K

ALL = P.CASES + [P.HOST_STEP]
DISTINCT = list({c.ref_key(): c for c in reversed(ALL)}.values())[::-1]     # the first case of each distinct model and inputs (group b shares a/default's)


def by_prefix(p):
    return [c for c in P.CASES if c.name.startswith(p)]


def test_case_table_reaches_every_edge():
    # the chains: 5 launches per layer folded, 8 plain, + the head (the six-layer step of DESIGN.md §5: 31 and 49)
    assert P.launches_per_step(6, 512, 1024) == 31 and P.launches_per_step(6, 512, 1024, plain_option=True) == 49
    assert P.launches_per_step(2, 512, 2560) == 2 * (8 + 2) + 1
    folded = {c.name for c in P.CASES if c.folded}
    assert {c.name for c in P.CASES} - folded == {"b/plain_chain", "d/1024x8x512", "d/512x8x2560", "i/small_norms_plain"}
    # the fold conditions, from the shapes: the last folded width on both conditions, and one case past each
    dims = {c.name: (c.config["d_model"], c.config["dim_feedforward"]) for c in P.CASES}
    assert any(d + ff == 1536 and 2 * d == 1536 and n in folded for n, (d, ff) in dims.items())
    assert any(2 * d > 1536 and d + ff <= 1536 for d, ff in dims.values())
    assert any(ff > 1536 and 2 * d <= 1536 for d, ff in dims.values())
    assert any(d % 64 == 32 and n in folded for n, (d, ff) in dims.items())
    assert any(ff < d for d, ff in dims.values())
    # the key batches of the self-attention: every head_dim has a case whose positions lie on both sides of its batch size, and
    # head_dim 128 crosses two batches
    assert {hd: P.key_batch(hd) for hd in (16, 32, 64, 128)} == {16: 512, 32: 256, 64: 128, 128: 64}
    for hd in (16, 32, 64, 128):
        assert any(c.hd == hd and c.T - 1 > P.key_batch(hd) + 1 for c in P.CASES), hd
    assert any(c.hd == 128 and c.T - 1 > 2 * P.key_batch(128) for c in P.CASES)
    # the last cache row (T = max_sequence_chord) at config 1 and config 2; more than one graph of 16 steps and a remainder everywhere
    assert any(c.T == c.config["max_sequence_chord"] == 300 for c in by_prefix("a/"))
    assert all(c.T == c.config["max_sequence_chord"] == 1024 and c.config["n_layers"] == 6 and c.B == 32 for c in by_prefix("e/"))
    assert all(c.T <= c.config["max_sequence_chord"] and c.T - 1 > 16 and (c.T - 1) % 16 for c in ALL)
    # the 16-row blocks: full, full + 1, two full, two + 1, two + 8 -- the last two as ONE chain
    assert [c.B for c in by_prefix("c/")] == [16, 17, 32, 33, 40]
    assert all(c.B <= c.max_decode_batch for c in ALL) and all(c.fp64_clips is None for c in by_prefix("c/"))
    # the video memory: one frame, a ragged count, the cap, and a smaller cap
    assert [(c.S, c.config.get("max_sequence_video", 300)) for c in by_prefix("f/")] == [(1, 300), (17, 300), (300, 300), (40, 64)]
    assert [c.config["rpr"] for c in by_prefix("g/")] == [False]
    # group b: a/default's model and inputs, one case per option named in include/amt_hip.h
    opts = {n for c in by_prefix("b/") for n, _ in c.options}
    assert opts == {"decode_chain_plain", "fuse_sampling_head", "short_context_attn", "layer0_kv_from_tables", "gemm_tile_pipeline"}
    assert all(c.ref_key() == P.BY_NAME["a/default"].ref_key() for c in by_prefix("b/"))
    assert {c.recipe for c in by_prefix("a/")} == {"default", "feedback"}
    assert all(P.FACTOR <= c.factor <= P.FACTOR_CAP for c in ALL)


@pytest.mark.parametrize("name", [c.name for c in DISTINCT])
def test_sequences_hold_every_id(name):
    """Every root id and every attr id, both pads among them, in every case (and in clip 0, the clip of the sensitivity run); keys 0, 1
    and 0.5; ids that repeat and ids that do not, for the repeat suppression of the host-driven step."""
    c = P.BY_NAME.get(name, P.HOST_STEP)
    f, toks, roots, attrs = P.inputs(c)
    assert toks.shape == roots.shape == attrs.shape == (c.B, c.T) and f["semantic"].shape[:2] == (c.B, c.S)
    assert set(roots.flatten().tolist()) == set(range(K.CHORD_ROOT_SIZE)) and K.CHORD_ROOT_PAD in roots
    assert set(attrs.flatten().tolist()) == set(range(K.CHORD_ATTR_SIZE)) and K.CHORD_ATTR_PAD in attrs
    if c.T >= 140:
        assert set(roots[0].tolist()) == set(range(K.CHORD_ROOT_SIZE)) and set(attrs[0].tolist()) == set(range(K.CHORD_ATTR_SIZE))
    keys = f["key"].flatten().tolist()
    assert keys.count(0.5) == 1 and set(keys) <= {0.0, 0.5, 1.0} and len(set(keys)) == min(3, c.B)
    assert int(toks.min()) >= 0 and int(toks.max()) < K.CHORD_END
    rep = toks[:, 1:] == toks[:, :-1]
    assert rep.any() and not rep.all()


@pytest.mark.parametrize("name", [c.name for c in DISTINCT])
def test_reference_and_sensitivity(name):
    """e32 (the fp32 oracle against the fp64 one, the unit of the bound) is finite and positive and of fp32's size; a root id off by one
    at the middle position, and layer 0's Er shifted by one row, each move the rows behind it by at least 100 bounds."""
    c = P.BY_NAME.get(name, P.HOST_STEP)
    y64, y32, e32 = P.reference(c)
    assert y64.shape == y32.shape == (len(c.clips64), c.T - 1, K.CHORD_SIZE)
    assert torch.isfinite(y64).all() and torch.isfinite(y32).all()
    # fp32 has 6e-8 per rounding; a model of 2 .. 6 layers and sums of up to 2560 terms stays below a few hundred of them
    assert 0.0 < e32 < 2e-5, e32
    by_root, by_er = P.sensitivity(c)
    b = P.bound(c)
    print(f"\nDECODE_PARITY_HOST {name}: e32 {e32:.2e}  bound {b:.2e}  wrong root {by_root / b:.0f} bounds  "
          f"Er off by one {'-' if by_er is None else f'{by_er / b:.0f} bounds'}  |logits| {float(y64.abs().max()):.1f}")
    assert by_root >= P.SENSITIVITY * b, (by_root, b)
    assert (by_er is None) == (not c.config["rpr"])
    if by_er is not None:
        assert by_er >= P.SENSITIVITY * b, (by_er, b)
    # one LayerNorm (norm1 of the last layer) with 1e-6 for 1e-5: below one bound at the recipes' unit-variance rows, which is what
    # group i is there for
    by_eps = P.eps_sensitivity(c)
    print(f"DECODE_PARITY_HOST {name}: epsilon 1e-6 in one LayerNorm {by_eps / b:.1f} bounds")
    if c.norm_scale is not None:
        assert by_eps >= P.SENSITIVITY * b, (by_eps, b)


def test_row_convention_against_generate():
    """`O.generate` re-runs the forward over positions 0 .. cur-1 and decides id `cur` from its LAST row: along the ids it produced, that
    row is row cur-1 of ONE causal forward over the whole sequence (what `oracle_rows` returns, and what `teacher_forced_logits`
    reads at input position cur-1), and `decision_rows` of it restates the decision: the suppressions and the arg-max give the id."""
    T, P0, H = 14, 2, CFG1["num_heads"]
    sd = synthetic_sd(CFG1, seed=1, dtype=torch.float64, recipe="feedback")
    f = feats_t(synthetic.synthetic_features(1, seed=3, n_frames=20), dtype=torch.float64)
    steps = []

    def recording(sd_, H_, r, a, *feats):
        y = O.forward(sd_, H_, r, a, *feats)
        steps.append((r.shape[1], y[0, -1].clone()))
        return y

    pr, prr, pra = torch.tensor([1, 66]), torch.tensor([1, 6]), torch.tensor([0, 0])
    for mcn, mcc in P.HOST_STEP_VARIANTS:
        steps.clear()
        gen = O.generate(sd, H, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra,
                         target_seq_length=T, beam=0, max_conseq_N=mcn, max_conseq_chord=mcc, forward_fn=recording)
        assert gen.shape == (1, T) and [n for n, _ in steps] == list(range(P0, T))
        roots, attrs = prr.tolist(), pra.tolist()
        for tok in gen[0, P0:].tolist():
            r, a = O.root_attr_of(tok)
            roots.append(r)
            attrs.append(a)
        roots, attrs = torch.tensor([roots]), torch.tensor([attrs])
        rows = P.oracle_rows(sd, H, f, roots, attrs, (0,), T)
        assert rows.shape == (1, T - 1, K.CHORD_SIZE)
        for cur, last in steps:
            # the same fp64 arithmetic over a longer sequence: sums in another blocking, 1e-16 x |logits| 150 x a few thousand terms
            assert float((rows[0, cur - 1] - last).abs().max()) < 1e-9, cur
        dec = P.decision_rows(rows, gen, mcn, mcc)
        assert dec.shape == (1, T - 1, K.CHORD_END)
        assert dec[0, P0 - 1:].argmax(-1).tolist() == gen[0, P0:].tolist()
        if mcn == 0:
            assert float(dec[..., 0].abs().max()) == 0.0
