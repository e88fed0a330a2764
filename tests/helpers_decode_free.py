"""Cases, schedules, references and uniforms of the free-running base decode (tests/test_decode_free_gpu.py; the input conditions are
checked on the CPU by tests/test_decode_free_host.py).

What this holds.  The teacher-forced parity (tests/helpers_decode_parity.py) runs every step inside a primer, where both sampling heads
and the host commit take the next token / root / attr from the primer and drop their decision.  The code that turns logits into a token
and a token into the next input -- the suppressions and `pick_token`, `feedback_of`, `write_next_input`, the q / k / v the fused head forms
from the token it has just decided, the stores to tokens / roots / attrs that the table-sourced key stream re-reads -- runs only when the
model generates freely, and there the suite compared the run with itself.

Mechanism.  Logits at position t depend only on ids up to t, so an id sequence (the schedule) is chosen in advance, ONE fp64 forward along
it gives every decision distribution, and the uniforms are placed so that the free-running device must reproduce that very sequence, draw
by draw, through the real captured graphs -- while its logits, computed from what IT fed back, are held against an oracle that never saw
the device.

1. Schedule: ids dealt from reshuffled decks of the allowed ids (1 .. 156, and 0 where max_conseq_N is 1), so every id comes up once per
   deck; about a third of the positions repeat their predecessor; a run never exceeds max_conseq_chord.  The id BEHIND a full run (the
   one position where the repeat suppression acts) lies above the run's id at even positions and below it at odd ones, away from the
   ends of the table (`GUARD`): with the placement of (5) that is where a missing suppression moves the draw (condition (b) of the host
   file).  (root, attr) follow by the HOST's rule (`chord_to_root_attr` through `tests.helpers.decision_inputs`), not the kernel's.
2. Flat head: Wout.weight / Wout.bias times a power of two (exact in fp32 and fp64, so both see the same weights and the logits scale
   exactly), chosen so that max |y64| along the schedule lies in [2, 4): every id keeps a mass far above the margin.
3. Reference: `oracle_rows` in fp64 for EVERY clip, the same in fp32; `e32` and the bound `FACTOR * e32` as in the parity helper.
4. Margin (derived): a logit error of at most D = bound * max(1, max |y64|) in the sup norm multiplies every un-normalised probability
   by a factor in [exp(-D), exp(D)], so it moves any normalised CDF value by at most exp(2 D) - 1 of the total mass;
   margin = 2 * (exp(2 D) - 1) + 1e-5, the 1e-5 being `check_draws`' band for the device's fp32 cumulative sums.
5. Uniforms (T, B) fp32: the draw of toks[b, cur] reads row cur - 1; u puts the target `margin` inside the id's interval
   (cdf[tok] - pr[tok], cdf[tok]] of the fp64 decision distribution, at the lower edge for even cur and the upper for odd
   (`boundary_uniforms`' rule), rounded to fp32 towards the inside.  Unused rows are 0.5.
6. Run: `generate_batch(primer, target_seq_length=T, beam=0, sampler="categorical", uniforms=u, ..., return_logits=True)`.

Host-driven leg: `amt_generate_step_probs`, then `amt_generate_commit` of the SCHEDULED id (so `commit_tokens_kernel` stores it and
`embed_step_kernel` applies `feedback_of`), with `amt_generate_set_branch` at 1 for a fixed third of the steps (the committed position
keeps the PAD pair, the distribution is the plain softmax[:157]).

Which head decides position cur (`head_of`): the step at position cur - 1 ends with it.  `amt_generate_run` issues whole graphs of
`STEPS_PER_GRAPH` steps and then the remainder in halves (amt_api.hip; the 16 is `AmtTuning::steps_per_graph` of amt_common.h, which the
host file reads from the source); on the folded chain the head between two steps of ONE graph rides in the next step's self-attention
(attn_decode.hip, FOLD 5) unless `fuse_sampling_head` is 0, the last step of a graph ends with `sample_fold_kernel`; the plain chain
ends every step with `sample_kernel`.
"""
import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

from tests import helpers_decode_parity as P
from tests.helpers import CFG2, _decision_probs, decision_inputs
from video2music_amd import synthetic
from video2music_amd.utilities import constants as K

STEPS_PER_GRAPH = 16           # AmtTuning::steps_per_graph (video2music_amd/csrc/amt_common.h)
DRAW_BAND = 1e-5               # `tests.helpers.check_draws`: the device's fp32 cumulative sums
GUARD = 40                     # ids behind a full run keep this many ids between themselves and either end of the table
REPEAT = 0.5                   # a position tries to repeat its predecessor this often; with the refusals (a run at its length,
                               # no room behind a full run) about a third do
HEADS = ("fused", "sample_fold_kernel", "sample_kernel", "host commit")


@dataclass(frozen=True)
class FreeCase:
    name: str
    case: P.Case                # model, clips, length, features, options (tests/helpers_decode_parity.py)
    mcn: int = 0                # max_conseq_N
    mcc: int = 2                # max_conseq_chord
    P: int = 1                  # primer positions
    chord_embed: bool = False
    host: bool = False          # the host-driven leg
    sched_seed: int = 0
    repeat: float = REPEAT      # how often a position tries to repeat its predecessor
    after: str = None           # the case whose deck this one's continues: its first deck opens with the ids that case did not reach
    note: str = ""

    def ref_key(self):
        """Cases with the same model, inputs and schedule share one reference."""
        return (self.case.ref_key(), self.mcn, self.mcc, self.P, self.chord_embed, self.host, self.sched_seed)


def _c(name, cfg, B, T, seed, recipe="default", options=(), mdb=32):
    return P.Case(name, cfg, B=B, T=T, S=24, seed=seed, recipe=recipe, options=options, max_decode_batch=mdb)


_PLAIN = (("decode_chain_plain", 1),)
# The seeds (of the weights and features; the schedule follows them) are ones at which every condition of the host file holds: no
# repair pass touches a schedule, a case that misses a condition on the CPU gets another seed
CASES = [
    # config 1 across head_dim 32's 256-key batch: 299 steps = 18 graphs of 16, then 8 + 2 + 1; 897 draws
    FreeCase("a/config1", _c("a", P._cfg(), 3, 300, 11), note="fused head inside the graphs, sample_fold_kernel at their ends"),
    FreeCase("a/separate_head", _c("a", P._cfg(), 3, 300, 11, options=(("fuse_sampling_head", 0),)), note="sample_fold_kernel at every step"),
    FreeCase("a/long_attn_cache_keys", _c("a", P._cfg(), 3, 300, 11, options=(("short_context_attn", 0), ("layer0_kv_from_tables", 0)))),
    FreeCase("a/serial_tile_loop", _c("a", P._cfg(), 3, 300, 11, options=(("gemm_tile_pipeline", 0),))),
    FreeCase("a/plain_chain", _c("a", P._cfg(), 3, 300, 11, options=_PLAIN), note="sample_kernel<1>"),
    # id 0 drawn and fed back as (0, 1), runs of three, a primer of three, row blocks of 16 + 1 and 16 + 16 + 1 clips
    FreeCase("b/N1_rep3_B17", _c("b17", P._cfg(), 17, 48, 12, "feedback"), mcn=1, mcc=3, P=3),
    FreeCase("b/N1_rep3_B33", _c("b33", P._cfg(), 33, 48, 12, "feedback", mdb=40), mcn=1, mcc=3, P=3),
    FreeCase("b/rep1", _c("b", P._cfg(), 2, 40, 13), mcc=1, note="the previous id is always suppressed"),
    # config 2 across head_dim 64's 128-key batch: six layers, KCH 2 in the folded head
    FreeCase("c/config2", _c("c", P._cfg(CFG2), 17, 140, 22)),
    # widths: the stand-alone head's instantiations on the plain chain, the folded head at KCH 3
    FreeCase("d/320x5x512_plain", _c("d", P._wide(320, 5, 512), 2, 40, 24, options=_PLAIN), note="sample_kernel<2>"),
    FreeCase("d/768x12x768_plain", _c("d", P._wide(768, 12, 768), 2, 40, 24, options=_PLAIN),
             note="sample_kernel<3>: five rows per wave, a second pass over Wout with the reload"),
    FreeCase("d/1024x8x512", _c("d", P._wide(1024, 8, 512), 2, 40, 24), note="sample_kernel<4>: a third pass"),
    FreeCase("d/768x12x768", _c("d", P._wide(768, 12, 768), 2, 40, 24), note="folded head, KCH 3"),
    FreeCase("e/no_rpr", _c("e", P._cfg(rpr=False), 2, 140, 16)),
    FreeCase("f/chord_embed", _c("f", P._cfg(), 3, 48, 17), chord_embed=True,
             note="the id itself feeds back with attr 0; a 159-row table in the root table's place"),
    # the host-driven leg: 2 x 117 commits have to hold all 157 ids, so these try to repeat a little less often and the second deck
    # opens with what the first left
    FreeCase("h/host_N0", _c("h", P._cfg(), 3, 40, 18), mcn=0, mcc=2, host=True, repeat=0.4),
    FreeCase("h/host_N1", _c("h", P._cfg(), 3, 40, 18), mcn=1, mcc=2, host=True, sched_seed=1, repeat=0.4, after="h/host_N0"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
DEVICE_CASES = [c for c in CASES if not c.host]
HOST_CASES = [c for c in CASES if c.host]


# ---- which head decides a position -------------------------------------------------------------------------------------------------
def graph_sizes(n_steps, spg=STEPS_PER_GRAPH):
    """Steps per captured graph of `amt_generate_run` over n_steps: whole graphs, then the remainder in halves."""
    out, left = [], n_steps
    while left > 0:
        ns = spg
        while ns > left:
            ns >>= 1
        out.append(max(ns, 1))
        left -= out[-1]
    return out


def head_of(fc, cur):
    """The head that decides position cur (>= P): it ends the step at position cur - 1."""
    if fc.host:
        return "host commit"
    if not fc.case.folded:
        return "sample_kernel"
    if dict(fc.case.options).get("fuse_sampling_head", 1) == 0:
        return "sample_fold_kernel"
    first = 0
    for ns in graph_sizes(fc.case.T - 1):
        if first <= cur - 1 < first + ns:
            return "sample_fold_kernel" if cur - 1 == first + ns - 1 else "fused"
        first += ns
    raise ValueError(cur)


def host_branch(cur):
    """Branch of the host-driven step that produces position cur: the top-k branch (1: raw distribution, no feedback) at a fixed third."""
    return 1 if cur % 3 == 2 else 0


# ---- schedule ----------------------------------------------------------------------------------------------------------------------
def _room(tok, t):
    """Can a full run of `tok` be followed at position t?  (even t: an id above it, odd t: one below, `GUARD` ids from the ends)"""
    return tok < K.CHORD_END - 1 - GUARD if t % 2 == 0 else tok > GUARD


def _behind_full_run(tok, prev, t):
    return prev < tok <= K.CHORD_END - 1 - GUARD if t % 2 == 0 else GUARD <= tok < prev


@functools.lru_cache(maxsize=None)
def _schedule(B, T, P_, mcn, mcc, seed, repeat, lead=()):
    rs = np.random.RandomState(2000 + seed)
    allowed = list(range(0 if mcn == 1 else 1, K.CHORD_END))
    deck = rs.permutation(list(lead)).tolist() if lead else []

    def deal(ok, primer=False):
        while primer:                         # the primer is given, not decided: its ids do not come off the deck
            c = allowed[rs.randint(len(allowed))]
            if ok(c):
                return c
        while True:
            for i, c in enumerate(deck):
                if ok(c):
                    return deck.pop(i)
            deck.extend(rs.permutation(allowed).tolist())

    toks = np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        run = 0
        for t in range(T):
            prev = int(toks[b, t - 1]) if t else -1
            last = t + 1 >= T

            def fits(c, new_run):             # an id that completes a full run must leave room for the position behind it
                return new_run < mcc or last or _room(c, t + 1)

            if t and run >= mcc:
                tok = deal(lambda c: _behind_full_run(c, prev, t) and fits(c, 1), t < P_)
                run = 1
            elif t and rs.uniform() < repeat and fits(prev, run + 1):
                tok, run = prev, run + 1
            else:
                tok = deal(lambda c: c != prev and fits(c, 1), t < P_)
                run = 1
            toks[b, t] = tok
    return torch.from_numpy(toks)


def schedule(fc):
    """(toks, roots, attrs), each (B, T) int64: the ids the run must produce and the (root, attr) the host's rule feeds back for them
    (positions the host-driven leg commits on the top-k branch keep the PAD pair)."""
    lead = ()
    if fc.after:
        first = BY_NAME[fc.after]
        reached = set(schedule(first)[0][:, first.P:].flatten().tolist())
        lead = tuple(i for i in range(0 if fc.mcn == 1 else 1, K.CHORD_END) if i not in reached)
    toks = _schedule(fc.case.B, fc.case.T, fc.P, fc.mcn, fc.mcc, 10 * fc.case.seed + fc.sched_seed, fc.repeat, lead)
    pr = torch.tensor([[K.chord_to_root_attr(int(v)) for v in row[:fc.P]] for row in toks])
    roots, attrs = decision_inputs(toks, fc.P, pr[..., 0], pr[..., 1], 0, fc.chord_embed)
    if fc.host:
        for cur in range(fc.P, fc.case.T):
            if host_branch(cur):
                roots[:, cur], attrs[:, cur] = K.CHORD_ROOT_PAD, K.CHORD_ATTR_PAD
    return toks, roots, attrs


def full_run(toks, b, cur, mcc):
    """Do the last mcc ids in front of position cur form a run (the repeat suppression acts on the decision of cur)?"""
    return cur >= mcc and all(toks[b, cur - 1] == toks[b, cur - 1 - k] for k in range(1, mcc))


# ---- model and reference -----------------------------------------------------------------------------------------------------------
def state_dict(fc, dtype=torch.float32, head_scale=1.0):
    """The parity helper's state dict with the output head times `head_scale` (a power of two) and, for chord_embed, the frozen chord
    table of `tests.test_oracle_golden.base_embed_sd`."""
    sd = P.state_dict(fc.case, dtype)
    assert math.frexp(head_scale)[0] == 0.5, "the head scale must be a power of two"
    for k in ("Wout.weight", "Wout.bias"):
        sd[k] = sd[k] * head_scale
    if fc.chord_embed:
        name = "chord_embedding_model.weight"
        sd[name] = torch.from_numpy(synthetic.fill_tensor(name, (K.CHORD_SIZE, fc.case.config["d_model"]), fc.case.seed)).to(dtype)
    return sd


def features(fc, dtype=torch.float32):
    return P.inputs(fc.case, dtype)[0]


def head_scale_for(ymax):
    """The power of two that brings max |logit| `ymax` into [2, 4)."""
    return 2.0 ** (1 - math.frexp(ymax)[1] + 1)


@dataclass(frozen=True)
class Reference:
    toks: torch.Tensor
    roots: torch.Tensor
    attrs: torch.Tensor
    y64: torch.Tensor            # (B, T-1, 159) fp64, flat head
    y32: torch.Tensor            # the same oracle in fp32
    e32: float
    head_scale: float
    margin: float
    u: torch.Tensor              # (T, B) fp32; None for the host-driven leg


_REFERENCES = {}


def reference(fc):
    if fc.ref_key() not in _REFERENCES:
        _REFERENCES[fc.ref_key()] = _compute_reference(fc)
    return _REFERENCES[fc.ref_key()]


def _compute_reference(fc):
    case = fc.case
    H, clips = case.config["num_heads"], tuple(range(case.B))
    toks, roots, attrs = schedule(fc)
    # the head only scales the logits, and by a power of two exactly: one forward with the recipe's head gives the scale and the rows
    y64 = P.oracle_rows(state_dict(fc, torch.float64), H, features(fc, torch.float64), roots, attrs, clips, case.T)
    y32 = P.oracle_rows(state_dict(fc), H, features(fc), roots, attrs, clips, case.T)
    assert y64.dtype == torch.float64 and y32.dtype == torch.float32
    s = head_scale_for(float(y64.abs().max()))
    y64, y32 = y64 * s, y32 * s
    e32 = max(P.rel_err(y32[b], y64[b]) for b in clips)
    m = margin_of(case.factor * e32, float(y64.abs().max()))
    u = None if fc.host else uniforms(fc, toks, y64, m)
    return Reference(toks, roots, attrs, y64, y32, e32, s, m, u)


def bound(fc):
    assert P.FACTOR <= fc.case.factor <= P.FACTOR_CAP
    return fc.case.factor * reference(fc).e32


def margin_of(bound_, ymax):
    delta = bound_ * max(1.0, ymax)
    return 2.0 * math.expm1(2.0 * delta) + DRAW_BAND


# ---- the decision, restated ----------------------------------------------------------------------------------------------------------
def decision(fc, y_row, toks, b, cur, rep=True, n=True):
    """Masked, un-normalised decision distribution (157,) of position cur from the logits row of position cur - 1, in the row's dtype;
    `rep` / `n` = False leave that suppression out."""
    tk = toks.numpy() if isinstance(toks, torch.Tensor) else toks
    return _decision_probs(y_row, tk, b, cur, fc.mcn if n else 1, fc.mcc if rep else cur + 1, 1.0)


def inverse_cdf(pr, u, carry=True):
    """`pick_token` with uniforms (sample_device.h): the first id with positive mass whose cumulative mass reaches u * sum, the scan
    running over three blocks of 64 ids whose totals carry into the next block (`carry=False`: the carry dropped); the last id with
    positive mass when none does.  Sums in the dtype of `pr`."""
    target = pr.dtype.type(u) * pr.sum(dtype=pr.dtype)
    base = pr.dtype.type(0)
    for k in range(0, len(pr), 64):
        c = np.cumsum(pr[k:k + 64], dtype=pr.dtype)
        hit = np.flatnonzero((pr[k:k + 64] > 0) & (base + c >= target))
        if len(hit):
            return k + int(hit[0])
        if carry:
            base = base + c[-1]
    return int(np.flatnonzero(pr > 0)[-1])


def uniforms(fc, toks, y64, margin):
    """(T, B) fp32 (see the module docstring, 5)."""
    B, T = toks.shape
    tk = toks.numpy()
    u = np.full((T, B), 0.5, dtype=np.float32)
    for b in range(B):
        for cur in range(fc.P, T):
            pr = decision(fc, y64[b, cur - 1], tk, b, cur)
            pr /= pr.sum()
            tok = int(tk[b, cur])
            lo = pr[:tok].sum()
            if pr[tok] < 2 * margin:
                want = lo + pr[tok] / 2
                u[cur - 1, b] = want
                continue
            want = lo + margin if cur % 2 == 0 else lo + pr[tok] - margin
            v = np.float32(want)
            if cur % 2 == 0 and float(v) < want:                 # fp32 rounding goes towards the inside of the interval
                v = np.nextafter(v, np.float32(1))
            elif cur % 2 == 1 and float(v) > want:
                v = np.nextafter(v, np.float32(0))
            u[cur - 1, b] = v
    return torch.from_numpy(u)


def edge_distances(fc, ref, b, cur):
    """(u - lower edge, upper edge - u, mass of the id) of the scheduled draw of position cur in the normalised fp64 CDF."""
    pr = decision(fc, ref.y64[b, cur - 1], ref.toks, b, cur)
    pr /= pr.sum()
    tok = int(ref.toks[b, cur])
    lo, u = pr[:tok].sum(), float(ref.u[cur - 1, b])
    return u - lo, lo + pr[tok] - u, float(pr[tok])


def replay(fc, ref, y, carry=True, rep=True, n=True):
    """Ids (B, T) that the decision restated above draws from logits `y` (B, T-1, 159) under the reference's uniforms, the history
    being the SCHEDULE's (each position is judged on its own)."""
    B, T = ref.toks.shape
    tk = ref.toks.numpy()
    out = tk.copy()
    for b in range(B):
        for cur in range(fc.P, T):
            out[b, cur] = inverse_cdf(decision(fc, y[b, cur - 1], tk, b, cur, rep=rep, n=n), float(ref.u[cur - 1, b]), carry)
    return out


def entropy_bits(pr):
    p = pr[pr > 0] / pr.sum()
    return float(-(p * np.log2(p)).sum())


def feedback_sensitivity(fc):
    """Move (the parity error measure, clip 0, the rows behind the middle position) of ONE wrong feedback: the host's pair of id % 156 + 1
    for the middle position's id (the id itself for chord_embed), in fp64."""
    ref, case = reference(fc), fc.case
    mid = case.T // 2
    while fc.host and host_branch(mid):
        mid += 1
    wrong = int(ref.toks[0, mid]) % 156 + 1
    roots, attrs = ref.roots.clone(), ref.attrs.clone()
    roots[0, mid], attrs[0, mid] = (wrong, 0) if fc.chord_embed else K.chord_to_root_attr(wrong)
    sd = state_dict(fc, torch.float64, ref.head_scale)
    moved = P.oracle_rows(sd, case.config["num_heads"], features(fc, torch.float64), roots, attrs, (0,), case.T)[0]
    return P.rel_err(moved[mid + 1:], ref.y64[0][mid + 1:])


# ---- the device side -----------------------------------------------------------------------------------------------------------------
def build_model(fc):
    ref = reference(fc)
    return P.build_model(fc.case, state_dict(fc, head_scale=ref.head_scale), **({"chord_embed": True} if fc.chord_embed else {}))


def free_run(m, f, fc, ref):
    """(ids (B, T), logits (B, T-1, 159)) of the free-running device under the reference's uniforms."""
    Pn, T = fc.P, fc.case.T
    with torch.no_grad():
        ids, lg = m.generate_batch(*P.feature_args(f), ref.toks[:, :Pn], ref.roots[:, :Pn], ref.attrs[:, :Pn], target_seq_length=T, beam=0,
                                   sampler="categorical", uniforms=ref.u, max_conseq_N=fc.mcn, max_conseq_chord=fc.mcc, return_logits=True)
    torch.cuda.synchronize()
    lg = lg[:T - 1].permute(1, 0, 2).contiguous().cpu()
    assert lg.shape == (fc.case.B, T - 1, K.CHORD_SIZE)
    return ids.cpu(), lg


def host_free_probs(m, f, fc, ref):
    """(ids (B, T) of `amt_generate_end`, distributions (B, T-1, 157)) of the host-driven step with a primer of P positions: every step's
    distribution is read, then the SCHEDULED id is committed, on the branch `host_branch` names."""
    from video2music_amd import _lib
    B, T = ref.toks.shape
    sem, key, scene, motion, emotion, Bf, S = m._prep_features(*P.feature_args(f))
    assert Bf == B <= m.max_decode_batch
    h = m._ensure_handle(sem.shape[2])
    st = _lib.stream_ptr()
    pr = [p[:, :fc.P].cuda().long().contiguous() for p in (ref.toks, ref.roots, ref.attrs)]
    sched = ref.toks.t().contiguous().cuda()                        # (T, B): row cur is what the host commits at position cur
    out = torch.empty(T - 1, B, K.CHORD_END, device="cuda")
    ids = torch.empty(B, T, device="cuda", dtype=torch.long)
    with torch.no_grad():
        m._encode(h, sem, scene, motion, emotion, slice(0, B))
        _lib.call("amt_generate_begin", h, B, _lib.ptr(pr[0]), _lib.ptr(pr[1]), _lib.ptr(pr[2]), fc.P, 1, _lib.ptr(key), T, 0,
                  int(fc.mcn), int(fc.mcc), st)
        for cur in range(1, T):
            _lib.call("amt_generate_set_branch", h, host_branch(cur) if cur >= fc.P else 0)
            _lib.call("amt_generate_step_probs", h, _lib.ptr(out[cur - 1]), st)
            _lib.call("amt_generate_commit", h, _lib.ptr(sched[cur]), st)
        _lib.call("amt_generate_end", h, _lib.ptr(ids), st)
    torch.cuda.synchronize()
    return ids.cpu(), out.permute(1, 0, 2).contiguous().cpu()


def host_decision_rows(fc, y, toks):
    """What `host_free_probs` must return for logits `y` (B, T-1, 159): `decision_rows` (the suppressions of sample.hip) on the sampling
    branch, the plain softmax[:157] on the top-k branch; in the dtype of `y`."""
    rows = P.decision_rows(y, toks, fc.mcn, fc.mcc)
    for cur in range(fc.P, toks.shape[1]):
        if host_branch(cur):
            rows[:, cur - 1] = torch.softmax(y[:, cur - 1], -1)[:, :K.CHORD_END]
    return rows
