"""Input conditions of the free-running decode cases (tests/helpers_decode_free.py), on the CPU, before any GPU run: every scheduled
draw is reachable and its uniform sits a derived margin inside its interval, plain fp32 is itself inside that margin, each case can see
the errors it exists for (a wrong feedback pair, a missing repeat / N suppression, a CDF scan that loses the carry between its 64-id
blocks), and over the table every head decides every id.  The last test restates why the suite's earlier categorical tests barely drew:
the entropy of their decision distribution against the flat head's."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import helpers_decode_free as F
from tests import helpers_decode_parity as P
from tests.helpers import CFG1, CFG2, feats_t, synthetic_sd
from video2music_amd import synthetic
from video2music_amd.utilities import constants as K

DISTINCT = list({c.ref_key(): c for c in reversed(F.CASES)}.values())[::-1]      # the first case of each distinct model, inputs and schedule
DEVICE = [c for c in DISTINCT if not c.host]


def decided(fc):
    return [(b, cur) for b in range(fc.case.B) for cur in range(fc.P, fc.case.T)]


def test_steps_per_graph_is_the_library_default():
    """`head_of` classifies positions by 16 steps per graph: `AmtTuning::steps_per_graph`, immutable in a release build (tuning.hip)."""
    src = os.path.join(os.path.dirname(os.path.abspath(synthetic.__file__)), "csrc", "amt_common.h")
    with open(src) as fh:
        found = re.findall(r"int\s+steps_per_graph\s*=\s*(\d+)\s*;", fh.read())
    assert found == [str(F.STEPS_PER_GRAPH)]
    assert F.graph_sizes(299) == [16] * 18 + [8, 2, 1] and F.graph_sizes(47) == [16, 16, 8, 4, 2, 1] and F.graph_sizes(39) == [16, 16, 4, 2, 1]


def test_case_table():
    by = F.BY_NAME
    cfgs = {n: (c.case.config["d_model"], c.case.config["dim_feedforward"], c.case.config["n_layers"]) for n, c in by.items()}
    # chains and head instantiations (sample.hip: (d + 255) / 256 float4 chunks per lane)
    plain = {n for n, c in by.items() if not c.case.folded}
    assert plain == {"a/plain_chain", "d/320x5x512_plain", "d/768x12x768_plain", "d/1024x8x512"}
    assert sorted((cfgs[n][0] + 255) // 256 for n in plain) == [1, 2, 3, 4]
    assert {(cfgs[n][0] + 255) // 256 for n in set(by) - plain} == {1, 2, 3}
    assert P.takes_folded_chain(320, 512) and P.takes_folded_chain(768, 768) and not P.takes_folded_chain(1024, 512)
    # group a: one model, inputs and schedule under the options of the step
    a = [c for c in F.CASES if c.name.startswith("a/")]
    assert len({c.ref_key() for c in a}) == 1 and len(a) == 5
    assert {n for c in a for n, _ in c.case.options} == {"decode_chain_plain", "fuse_sampling_head", "short_context_attn",
                                                         "layer0_kv_from_tables", "gemm_tile_pipeline"}
    assert all(c.case.B == 3 and c.case.T == 300 and (c.mcn, c.mcc, c.P) == (0, 2, 1) for c in a)
    assert sum(len(decided(c)) for c in a[:1]) == 897
    # the key batches of the self-attention are crossed where the issue says so
    assert a[0].case.hd == 32 and a[0].case.T - 1 > P.key_batch(32) + 1
    c2 = by["c/config2"]
    assert c2.case.config == dict(CFG2) and c2.case.hd == 64 and c2.case.T - 1 > P.key_batch(64) + 1 and c2.case.B == 17
    assert [(by[n].case.B, by[n].mcn, by[n].mcc, by[n].P, by[n].case.T) for n in ("b/N1_rep3_B17", "b/N1_rep3_B33", "b/rep1")] == \
        [(17, 1, 3, 3, 48), (33, 1, 3, 3, 48), (2, 0, 1, 1, 40)]
    assert by["b/N1_rep3_B33"].case.max_decode_batch == 40 and all(c.case.B <= c.case.max_decode_batch for c in F.CASES)
    assert not by["e/no_rpr"].case.config["rpr"] and by["f/chord_embed"].chord_embed
    assert [(c.case.B, c.case.T, c.mcn, c.mcc, c.P) for c in F.HOST_CASES] == [(3, 40, 0, 2, 1), (3, 40, 1, 2, 1)]
    assert all(c.case.S == 24 and c.case.T <= c.case.config["max_sequence_chord"] for c in F.CASES)
    # steps per graph: each size occurs
    assert {ns for c in F.DEVICE_CASES for ns in F.graph_sizes(c.case.T - 1)} == {16, 8, 4, 2, 1}


@pytest.mark.parametrize("name", [c.name for c in DISTINCT])
def test_schedule(name):
    fc = F.BY_NAME[name]
    toks, roots, attrs = F.schedule(fc)
    B, T = fc.case.B, fc.case.T
    assert toks.shape == roots.shape == attrs.shape == (B, T)
    assert int(toks.min()) >= (0 if fc.mcn == 1 else 1) and int(toks.max()) < K.CHORD_END
    assert (0 in toks[:, fc.P:]) == (fc.mcn == 1)
    tk = toks.numpy()
    for b in range(B):
        for t in range(fc.mcc, T):
            assert not all(tk[b, t] == tk[b, t - 1 - k] for k in range(fc.mcc)), (b, t)       # no run longer than max_conseq_chord
    rep = float((tk[:, 1:] == tk[:, :-1]).mean())
    assert (rep == 0.0) if fc.mcc == 1 else (0.2 < rep < 0.45), rep
    # the host's feedback rule, not the kernel's
    for b, cur in decided(fc):
        if fc.chord_embed:
            want = (int(tk[b, cur]), 0)
        elif fc.host and F.host_branch(cur):
            want = (K.CHORD_ROOT_PAD, K.CHORD_ATTR_PAD)
        else:
            want = K.chord_to_root_attr(int(tk[b, cur]))
        assert (int(roots[b, cur]), int(attrs[b, cur])) == want
    if fc.mcn == 1 and not fc.chord_embed:
        fed = {(int(r), int(a)) for r, a, t in zip(roots.flatten(), attrs.flatten(), toks.flatten()) if t == 0}
        assert (0, 1) in fed
    if fc.host:
        br = [F.host_branch(cur) for cur in range(fc.P, T)]
        assert abs(sum(br) / len(br) - 1 / 3) < 0.02


@pytest.mark.parametrize("name", [c.name for c in DEVICE])
def test_draw_conditions(name):
    fc = F.BY_NAME[name]
    ref = F.reference(fc)
    case, tk = fc.case, ref.toks.numpy()
    B, T = tk.shape
    ymax = float(ref.y64.abs().max())
    # the flat head and the reference's own error
    assert math.frexp(ref.head_scale)[0] == 0.5 and 2.0 <= ymax < 4.0
    assert torch.isfinite(ref.y64).all() and torch.isfinite(ref.y32).all() and ref.y64.shape == (B, T - 1, K.CHORD_SIZE)
    assert 0.0 < ref.e32 < 2e-5 and P.FACTOR <= case.factor <= P.FACTOR_CAP          # fp32's size, as tests/test_decode_parity_host.py
    bnd = F.bound(fc)
    margin = ref.margin
    assert margin == 2.0 * math.expm1(2.0 * bnd * max(1.0, ymax)) + F.DRAW_BAND and margin < 1e-3
    # reachability and placement, in fp64
    mass, ent = [], []
    for b, cur in decided(fc):
        lo, hi, p = F.edge_distances(fc, ref, b, cur)
        mass.append(p)
        assert p >= 2 * margin, (b, cur, int(tk[b, cur]), p, margin)
        assert lo >= margin and hi >= margin, (b, cur, lo, hi, margin)
        assert (lo < hi) == (cur % 2 == 0)                                           # lower edge at even positions, upper at odd
        ent.append(F.entropy_bits(F.decision(fc, ref.y64[b, cur - 1], tk, b, cur)))
    assert np.array_equal(F.replay(fc, ref, ref.y64), tk)
    assert float(ref.u.min()) > 0.0 and float(ref.u.max()) < 1.0 and ref.u.dtype == torch.float32 and ref.u.shape == (T, B)
    # plain fp32 (probabilities and cumulative sums) is itself inside the margin
    assert ref.y32.dtype == torch.float32 and np.array_equal(F.replay(fc, ref, ref.y32), tk)
    # (a) one wrong feedback pair
    by_fb = F.feedback_sensitivity(fc)
    assert by_fb >= P.SENSITIVITY * bnd, (by_fb, bnd)
    # (b) the repeat suppression left out: another id at every position behind a full run
    behind = [(b, cur) for b, cur in decided(fc) if F.full_run(tk, b, cur, fc.mcc)]
    no_rep = F.replay(fc, ref, ref.y64, rep=False)
    assert len(behind) >= 10 and all(no_rep[b, cur] != tk[b, cur] for b, cur in behind), \
        [(b, cur) for b, cur in behind if no_rep[b, cur] == tk[b, cur]]
    assert all(no_rep[b, cur] == tk[b, cur] for b, cur in decided(fc) if (b, cur) not in set(behind))
    # (c) the N suppression left out
    n_share = None
    if fc.mcn == 0:
        no_n = F.replay(fc, ref, ref.y64, n=False)
        n_share = float(np.mean([no_n[b, cur] != tk[b, cur] for b, cur in decided(fc)]))
        assert n_share >= 0.5, n_share
    # (d) the carry between the 64-id blocks dropped
    no_carry = F.replay(fc, ref, ref.y64, carry=False)
    # (every draw of an id >= 64 but those of 156: a scan without the carry never reaches a target in the last block, and `pick_token`
    # then returns the last id with positive mass -- 156 itself; every other id of that block comes back as 156)
    high = [(b, cur) for b, cur in decided(fc) if 64 <= tk[b, cur] < K.CHORD_END - 1]
    assert len(high) >= 10 and all(no_carry[b, cur] != tk[b, cur] for b, cur in high), \
        [(b, cur, tk[b, cur], no_carry[b, cur]) for b, cur in high if no_carry[b, cur] == tk[b, cur]]
    assert all(no_carry[b, cur] == tk[b, cur] for b, cur in decided(fc) if tk[b, cur] < 64 or tk[b, cur] == K.CHORD_END - 1)
    print(f"\nDECODE_FREE_HOST {name}: head x{ref.head_scale:g}  |logits| {ymax:.2f}  e32 {ref.e32:.2e}  bound {bnd:.2e}  margin {margin:.2e}  "
          f"min mass {min(mass):.2e} ({min(mass) / margin:.1f} margins)  draws {len(mass)}  distinct ids {len(set(tk[:, fc.P:].flatten().tolist()))}  "
          f"median entropy {np.median(ent):.2f} bits  wrong feedback {by_fb / bnd:.0f} bounds  behind a full run {len(behind)}  "
          f"N left out moves {'-' if n_share is None else f'{n_share:.0%}'}")


@pytest.mark.parametrize("name", [c.name for c in F.HOST_CASES])
def test_host_leg_conditions(name):
    fc = F.BY_NAME[name]
    ref = F.reference(fc)
    tk = ref.toks.numpy()
    assert ref.u is None and 2.0 <= float(ref.y64.abs().max()) < 4.0 and 0.0 < ref.e32 < 2e-5
    by_fb = F.feedback_sensitivity(fc)
    assert by_fb >= P.SENSITIVITY * F.bound(fc), (by_fb, F.bound(fc))
    rows, r32 = F.host_decision_rows(fc, ref.y64, ref.toks), F.host_decision_rows(fc, ref.y32, ref.toks)
    assert rows.dtype == torch.float64 and r32.dtype == torch.float32 and rows.shape == (fc.case.B, fc.case.T - 1, K.CHORD_END)
    zeros = (rows == 0.0).sum(-1)
    for b, cur in decided(fc):
        want = 0 if F.host_branch(cur) else int(fc.mcn == 0) + int(F.full_run(tk, b, cur, fc.mcc))
        assert int(zeros[b, cur - 1]) == want, (b, cur)
    assert sum(F.full_run(tk, b, cur, fc.mcc) and not F.host_branch(cur) for b, cur in decided(fc)) >= 10
    e32p = max(P.prob_err(r32[b], rows[b]) for b in range(fc.case.B))
    assert 0.0 < e32p < 1e-4
    print(f"\nDECODE_FREE_HOST {name}: head x{ref.head_scale:g}  e32 {ref.e32:.2e}  distribution e32 {e32p:.2e}  wrong feedback {by_fb / F.bound(fc):.0f} bounds")


def test_head_scale_is_exact():
    """The power-of-two head scale commutes with the forward bit for bit, in fp64 and in fp32: the reference multiplies the rows of ONE
    forward, the device runs the scaled weights."""
    fc = F.BY_NAME["b/rep1"]
    ref = F.reference(fc)
    assert ref.head_scale != 1.0
    H, clips = fc.case.config["num_heads"], tuple(range(fc.case.B))
    for dtype, y in ((torch.float64, ref.y64), (torch.float32, ref.y32)):
        again = P.oracle_rows(F.state_dict(fc, dtype, ref.head_scale), H, F.features(fc, dtype), ref.roots, ref.attrs, clips, fc.case.T)
        assert torch.equal(again, y)


def test_coverage_over_the_table():
    """Every id 1 .. 156 is decided at least once by each head (and committed by the host); id 0 in every max_conseq_N = 1 case."""
    seen = {h: set() for h in F.HEADS}
    for fc in F.CASES:
        tk = F.schedule(fc)[0].numpy()
        mine = {h: set() for h in F.HEADS}
        for b, cur in decided(fc):
            mine[F.head_of(fc, cur)].add(int(tk[b, cur]))
        for h in F.HEADS:
            seen[h] |= mine[h]
        if fc.mcn == 1:
            assert 0 in set().union(*mine.values()), fc.name
    for h in F.HEADS:
        missing = set(range(1, K.CHORD_END)) - seen[h]
        assert not missing, (h, sorted(missing))
    assert 0 in seen["fused"] and 0 in seen["sample_fold_kernel"] and 0 in seen["host commit"]
    a = F.BY_NAME["a/config1"]
    heads = [F.head_of(a, cur) for cur in range(1, a.case.T)]
    assert heads.count("sample_fold_kernel") == 21 and heads.count("fused") == 278
    print("\nDECODE_FREE_HOST coverage: " + "  ".join(f"{h}: {len(seen[h])} ids" for h in F.HEADS))


def test_entropy_of_the_earlier_categorical_tests():
    """`test_device_categorical_draw` (tests/test_model_gpu.py) draws from the synthetic recipe's own head along the path it samples
    itself.  Restated here in fp64 for its first case (config 1, 3 clips, T 48, the same weights, features, primers and uniforms): the
    decision distribution holds a fraction of a bit at the median position, so one or two ids carry all the mass above rounding and a
    scan that lost its carry, or a suppression missing from one head, passes.  The flat head's holds most of the 7.3 bits of 156 ids."""
    from oracle import amt_oracle as O
    B, T, Pn, mcn, mcc = 3, 48, 3, 0, 2
    fc = F.FreeCase("entropy", P.Case("entropy", P._cfg(), B=B, T=T, S=300), mcn=mcn, mcc=mcc, P=Pn)
    sd = synthetic_sd(CFG1, 2, dtype=torch.float64)
    f = feats_t(synthetic.synthetic_features(B, seed=99), dtype=torch.float64)
    prim = [torch.tensor(v) for v in zip(*[K.primer_from_name(n) for n in ("C", "G", "A:min")])]
    u = torch.rand(T, B, generator=torch.Generator().manual_seed(5)).numpy()
    toks, roots, attrs = (p.expand(B, Pn).clone() for p in prim)
    ent = []
    with torch.no_grad():
        memory = O.encode(sd, CFG1["num_heads"], f["semantic"], f["scene_offset"], f["motion"], f["emotion"])
        for cur in range(Pn, T):
            y = O.linear(O.decode(sd, CFG1["num_heads"], O.chord_stream(sd, roots, attrs, f["key"]), memory), sd["Wout.weight"], sd["Wout.bias"])
            new = []
            for b in range(B):
                pr = F.decision(fc, y[b, -1], toks, b, cur)
                ent.append(F.entropy_bits(pr))
                new.append(F.inverse_cdf(pr, float(u[cur - 1, b])))
            ra = [K.chord_to_root_attr(t) for t in new]
            toks = torch.cat([toks, torch.tensor(new)[:, None]], 1)
            roots = torch.cat([roots, torch.tensor([r for r, _ in ra])[:, None]], 1)
            attrs = torch.cat([attrs, torch.tensor([a for _, a in ra])[:, None]], 1)
    peaked, distinct = float(np.median(ent)), len(set(toks[:, Pn:].flatten().tolist()))
    flat_fc = F.BY_NAME["a/config1"]
    ref = F.reference(flat_fc)
    flat = float(np.median([F.entropy_bits(F.decision(flat_fc, ref.y64[b, cur - 1], ref.toks, b, cur)) for b, cur in decided(flat_fc)]))
    print(f"\nDECODE_FREE_HOST median entropy of the decision distribution: test_device_categorical_draw (config 1, its own path) "
          f"{peaked:.3f} bits, {distinct} distinct ids in {B * (T - Pn)} draws; flat head (a/config1) {flat:.2f} bits of {math.log2(156):.2f}")
    # the two thresholds only name the sides of the gap: under two bits (the mass of fewer than four ids) against over half of the table's bits
    assert peaked < 2.0 and flat > 0.5 * math.log2(156)
