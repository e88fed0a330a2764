"""Cases, inputs, references and bounds of the base decode step's logit parity (tests/test_decode_parity_gpu.py; the input conditions
are checked on the CPU by tests/test_decode_parity_host.py).

Mechanism.  `amt_generate_begin` takes a primer of 1 .. T positions per clip.  A position inside the primer is stepped like any other and
its decision is discarded: the stand-alone head (sample.hip, `sample_kernel` / `sample_fold_kernel`) and the head that rides in the next
step's first self-attention (attn_decode.hip, FOLD 5) both branch on `cur < n_primer` and then read token, root and attr of the next
position from the sequences `init_sequences_kernel` filled from the primer; `commit_tokens_kernel` / `embed_step_kernel` of the
host-driven step do the same (`cur >= n_primer`).  So a primer as long as the sequence teacher-forces every clip along arbitrary
(root, attr) ids through the real captured graphs, and `return_logits` gives the step's logits at every position.

Reference: `oracle.amt_oracle.forward` with the state dict and the features cast to float64; row t of the causal forward is the step's
logits at input position t (held against `O.generate`'s own steps by the host file).

Error measure of clip c: max |got - y64| / max(1, max |y64|) over rows 0 .. T-2.  Bound: `e32` is that measure of the SAME oracle run in
fp32 on the CPU on the same inputs, maximised over the case's fp64 clips, and a case asserts err <= factor * e32 with factor 4 -- what
tests/test_gemm_routes_gpu.py gives a device sum in another order over its fp32 restatement.  No case needed 8, the training tests' factor.
Clips without an fp64 row (config 2 only) are compared with the model's own teacher-forced fp32 `forward` (the prefill path: dense GEMM
and prefill attention, no kernel shared with the step) at 2 * factor * e32: each side is within factor * e32 of fp64.
"""
import functools
from dataclasses import dataclass

import numpy as np
import torch

from oracle import amt_oracle as O
from tests.helpers import CFG1, CFG2, _decision_probs, feats_t, synthetic_sd
from video2music_amd import synthetic
from video2music_amd.utilities import constants as K

FACTOR = 4                     # device sum in another order over the fp32 restatement (tests/helpers_ops_edges.py)
FACTOR_CAP = 8                 # the training tests' factor: nothing may take more
SENSITIVITY = 100              # a one-id / one-Er-row error must move the logits by this many bounds


def key_batch(hd):
    """Keys per K/V batch of the decode self-attention (attn_decode.hip: 8 waves x (64 / (hd / 4)) keys x 4 sub-batches)."""
    return 8 * (64 // (hd // 4)) * 4


def takes_folded_chain(d, dff, plain_option=False):
    """amt_finalize's choice of the folded decode chain (amt_api.hip): G1 / G2 read [o | x] (K = 2 d), G3 reads [h | x] (K = dff + d)."""
    return (not plain_option) and d % 32 == 0 and 2 * d <= 1536 and (dff + d) % 64 == 0 and dff + d <= 1536 and dff % 16 == 0


def launches_per_step(n_layers, d, dff, plain_option=False):
    """Kernel launches of one eagerly issued decode step, sampling head included (`generate_profile`): 5 per layer folded, 8 plain, and
    one more per further 1024-column range of linear2 when dim_feedforward > 1536."""
    if takes_folded_chain(d, dff, plain_option):
        return 5 * n_layers + 1
    extra = (-(-dff // 1024) - 1) if dff > 1536 else 0
    return (8 + extra) * n_layers + 1


@dataclass(frozen=True)
class Case:
    name: str
    cfg: tuple                   # sorted (key, value) pairs over CFG1 / CFG2
    B: int
    T: int
    S: int
    recipe: str = "default"
    seed: int = 0
    options: tuple = ()          # ((handle option, value), ...); "decode_chain_plain" is set before the handle exists
    fp64_clips: tuple = None     # None: every clip
    max_decode_batch: int = 32
    factor: int = FACTOR
    sens_T: int = None           # length of the fp64 sensitivity run (default: T)
    norm_scale: tuple = None     # (factor on the weights, factor on the biases) of norm1 / norm2 / norm3 of every decoder layer
    note: str = ""

    @property
    def config(self):
        return dict(self.cfg)

    @property
    def plain_option(self):
        return dict(self.options).get("decode_chain_plain", 0) == 1

    @property
    def folded(self):
        c = self.config
        return takes_folded_chain(c["d_model"], c["dim_feedforward"], self.plain_option)

    @property
    def hd(self):
        c = self.config
        return c["d_model"] // c["num_heads"]

    @property
    def clips64(self):
        return tuple(range(self.B)) if self.fp64_clips is None else self.fp64_clips

    def ref_key(self):
        """Cases with the same model and inputs (group b) share one reference."""
        return (self.cfg, self.B, self.T, self.S, self.recipe, self.seed, self.clips64, self.norm_scale)


def _cfg(base=CFG1, **kw):
    return tuple(sorted(dict(base, **kw).items()))


def _wide(d, H, dff, **kw):
    return _cfg(CFG1, d_model=d, num_heads=H, dim_feedforward=dff, **kw)


CASES = [
    # a: config 1 to the last cache row and across the 256-key batch of head_dim 32; 299 steps = 18 graphs of 16 + 8 + 2 + 1
    Case("a/default", _cfg(), B=3, T=300, S=64, seed=1),
    Case("a/feedback", _cfg(), B=3, T=300, S=64, seed=1, recipe="feedback"),
    # b: the same model and inputs under the other spellings of the step
    Case("b/plain_chain", _cfg(), B=3, T=300, S=64, seed=1, options=(("decode_chain_plain", 1),)),
    Case("b/separate_head", _cfg(), B=3, T=300, S=64, seed=1, options=(("fuse_sampling_head", 0),)),
    Case("b/long_attn_cache_keys", _cfg(), B=3, T=300, S=64, seed=1, options=(("short_context_attn", 0), ("layer0_kv_from_tables", 0))),
    Case("b/serial_tile_loop", _cfg(), B=3, T=300, S=64, seed=1, options=(("gemm_tile_pipeline", 0),)),
    # c: 16-row blocks of the skinny GEMMs: one full, one + a one-row tail, two full, two + one row, two + half (one chain of 40)
    Case("c/B16", _cfg(), B=16, T=48, S=24, seed=2, recipe="feedback"),
    Case("c/B17", _cfg(), B=17, T=48, S=24, seed=2, recipe="feedback"),
    Case("c/B32", _cfg(), B=32, T=48, S=24, seed=2, recipe="feedback"),
    Case("c/B33", _cfg(), B=33, T=48, S=24, seed=2, recipe="feedback", max_decode_batch=40),
    Case("c/B40", _cfg(), B=40, T=48, S=24, seed=2, recipe="feedback", max_decode_batch=40),
    # d: widths and head sizes
    Case("d/64x2x128", _wide(64, 2, 128), B=2, T=40, S=24, seed=3),
    Case("d/96x3x160", _wide(96, 3, 160), B=2, T=40, S=24, seed=3, note="d_model a multiple of 32, not of 64"),
    Case("d/256x2x512", _wide(256, 2, 512), B=2, T=140, S=24, seed=3, note="head_dim 128: crosses the 64- and 128-key batches"),
    Case("d/192x3x320", _wide(192, 3, 320), B=2, T=140, S=24, seed=3, note="head_dim 64: crosses the 128-key batch"),
    Case("d/128x8x64", _wide(128, 8, 64, max_sequence_chord=640), B=2, T=530, S=24, seed=3, sens_T=160,
         note="head_dim 16, dff < d: crosses the 512-key batch"),
    Case("d/768x12x768", _wide(768, 12, 768), B=2, T=40, S=24, seed=3, note="d + dff = 1536: the last folded width"),
    Case("d/1024x8x512", _wide(1024, 8, 512), B=2, T=40, S=24, seed=3, note="2 d > 1536: plain chain"),
    Case("d/512x8x2560", _wide(512, 8, 2560), B=2, T=40, S=24, seed=3, note="dff > 1536: plain chain, linear2 in column ranges"),
    # e: config 2 as benchmarked
    Case("e/config2", _cfg(CFG2), B=32, T=1024, S=300, seed=0, fp64_clips=(0, 31), sens_T=256),
    # f: video memory edges
    Case("f/S1", _cfg(), B=2, T=20, S=1, seed=5, recipe="feedback"),
    Case("f/S17", _cfg(), B=2, T=20, S=17, seed=5, recipe="feedback"),
    Case("f/S300", _cfg(), B=2, T=20, S=300, seed=5, recipe="feedback"),
    Case("f/S40_cap64", _cfg(max_sequence_video=64), B=2, T=20, S=40, seed=5, recipe="feedback"),
    # g: stock decoder layers (no relative-position table)
    Case("g/no_rpr", _cfg(rpr=False), B=2, T=140, S=24, seed=6),
    # i (added to the issue's list): LayerNorm rows of small variance.  At the synthetic recipes every normalised row has a variance near
    # 1, where an epsilon of 1e-6 for 1e-5 in one LayerNorm moves the logits by less than one bound (`eps_sensitivity`: 0.0 .. 0.8):
    # no case above can see it.  With the decoder layers' norm weights at 0.02 and their biases at 0.3 of the recipe's, the rows that
    # enter the next LayerNorm have a small variance and the epsilon moves the logits by 44 .. 2100 bounds (every LayerNorm but layer
    # 0's norm1, whose input holds the chord embedding), while a wrong id or Er row still moves them by ~1000
    Case("i/small_norms", _cfg(), B=17, T=40, S=24, seed=8, recipe="feedback", norm_scale=(0.02, 0.3)),
    Case("i/small_norms_plain", _cfg(), B=17, T=40, S=24, seed=8, recipe="feedback", norm_scale=(0.02, 0.3),
         options=(("decode_chain_plain", 1),)),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# h: the host-driven step (amt_generate_step_probs / amt_generate_commit): the eager kernels and the stand-alone head
HOST_STEP = Case("h/host_step", _cfg(), B=3, T=40, S=24, seed=7, recipe="feedback")
HOST_STEP_VARIANTS = [(0, 2), (1, 2)]          # (max_conseq_N, max_conseq_chord)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def model_cfg(case):
    """Constructor keywords of the case's VideoMusicTransformer."""
    return case.config


def state_dict(case, dtype=torch.float32):
    cfg = case.config
    sd = synthetic_sd(cfg, seed=case.seed, dtype=dtype, recipe=case.recipe)
    if not cfg["rpr"]:
        sd = {k: v for k, v in sd.items() if not k.endswith(".Er")}
    if case.norm_scale is not None:
        for k in sd:
            if k.startswith("transformer.decoder.layers.") and ".norm" in k:
                sd[k] = (sd[k].double() * case.norm_scale[k.endswith(".bias")]).to(dtype)
    return sd


def clip_keys(B, seed):
    """Keys 0 and 1 alternating (which comes first depends on the seed) and 0.5 for one clip (the last of two, else clip 2)."""
    k = np.array([(c + seed) % 2 for c in range(B)], dtype=np.float32)
    k[min(2, B - 1)] = 0.5
    return k.reshape(B, 1)


def chord_ids(B, T, seed):
    """(toks, roots, attrs), each (B, T) int64.  Roots uniform over all CHORD_ROOT_SIZE ids and attrs over all CHORD_ATTR_SIZE ids, both
    pads included, drawn independently per clip and position (most pairs are no chord of chord.json: the step only sums table rows).
    The ids in `toks` are what the run returns and what the repeat suppression looks at; half of them repeat their predecessor."""
    rs = np.random.RandomState(1000 + seed)
    roots = rs.randint(0, K.CHORD_ROOT_SIZE, size=(B, T))
    attrs = rs.randint(0, K.CHORD_ATTR_SIZE, size=(B, T))
    for ids, n in ((roots, K.CHORD_ROOT_SIZE), (attrs, K.CHORD_ATTR_SIZE)):
        # a short case (2 clips of 20) can miss an id: each missing one takes a place of the most frequent one
        for i in sorted(set(range(n)) - set(ids.flatten().tolist())):
            common = np.bincount(ids.flatten(), minlength=n).argmax()
            where = np.flatnonzero(ids.flatten() == common)
            ids.reshape(-1)[where[rs.randint(len(where))]] = i
    toks = rs.randint(0, K.CHORD_END, size=(B, T))
    rep = rs.uniform(size=(B, T)) < 0.5
    for t in range(1, T):
        toks[:, t] = np.where(rep[:, t], toks[:, t - 1], toks[:, t])
    return tuple(torch.from_numpy(a.astype(np.int64)) for a in (toks, roots, attrs))


@functools.lru_cache(maxsize=None)
def _inputs(B, T, S, seed):
    feats = synthetic.synthetic_features(B, seed=100 + seed, n_frames=S)
    return feats, clip_keys(B, seed), chord_ids(B, T, seed)


def inputs(case, dtype=torch.float32):
    """(features dict of CPU tensors in `dtype`, toks, roots, attrs)."""
    feats, key, ids = _inputs(case.B, case.T, case.S, case.seed)
    return (feats_t(feats, key=key, dtype=dtype),) + ids


# ---- references --------------------------------------------------------------------------------------------------------------------
def oracle_rows(sd, H, f, roots, attrs, clips, T):
    """Rows 0 .. T-2 of the oracle's causal teacher-forced forward for `clips`: (len(clips), T-1, 159) in the dtype of `sd`."""
    idx = torch.as_tensor(list(clips))
    with torch.no_grad():
        return O.forward(sd, H, roots[idx, :T - 1], attrs[idx, :T - 1], f["semantic"][idx], f["key"][idx], f["scene_offset"][idx],
                         f["motion"][idx], f["emotion"][idx])


def rel_err(got, ref):
    """max |got - ref| / max(1, max |ref|): the measure of tests/test_lockstep_parity_gpu.py."""
    return float((got.double() - ref.double()).abs().max() / max(1.0, float(ref.abs().max())))


_REFERENCES = {}


def reference(case):
    """(y64 (n fp64 clips, T-1, 159), the fp32 oracle's rows, e32); computed once per distinct model and inputs and left unchanged."""
    if case.ref_key() not in _REFERENCES:
        _REFERENCES[case.ref_key()] = _compute_reference(case)
    return _REFERENCES[case.ref_key()]


def _compute_reference(case):
    H = case.config["num_heads"]
    f64, _, roots, attrs = inputs(case, torch.float64)
    y64 = oracle_rows(state_dict(case, torch.float64), H, f64, roots, attrs, case.clips64, case.T)
    f32 = inputs(case)[0]
    y32 = oracle_rows(state_dict(case), H, f32, roots, attrs, case.clips64, case.T)
    assert y32.dtype == torch.float32 and y64.dtype == torch.float64
    e32 = max(rel_err(y32[i], y64[i]) for i in range(len(case.clips64)))
    return y64, y32, e32


def bound(case):
    assert FACTOR <= case.factor <= FACTOR_CAP
    return case.factor * reference(case)[2]


# ---- sensitivity (CPU, fp64) ---------------------------------------------------------------------------------------------------
def sensitivity(case):
    """(move of a wrong root id, move of layer 0's Er shifted by one row or None without rpr), each the error measure of clip 0's rows
    BEHIND the middle position (those that see the position only through the self-attention's keys and values), in fp64 at length
    `sens_T`: what the case's comparison would read if the step made that error."""
    T = case.sens_T or case.T
    H = case.config["num_heads"]
    sd = state_dict(case, torch.float64)
    f64, _, roots, attrs = inputs(case, torch.float64)
    mid = T // 2
    base = oracle_rows(sd, H, f64, roots, attrs, (0,), T)[0]
    wrong = roots.clone()
    wrong[0, mid] = (wrong[0, mid] + 1) % K.CHORD_ROOT_SIZE
    by_root = rel_err(oracle_rows(sd, H, f64, wrong, attrs, (0,), T)[0][mid + 1:], base[mid + 1:])
    by_er = None
    er = "transformer.decoder.layers.0.self_attn.Er"
    if er in sd:
        sd_er = dict(sd)
        sd_er[er] = torch.roll(sd[er], 1, dims=0)
        by_er = rel_err(oracle_rows(sd_er, H, f64, roots, attrs, (0,), T)[0][mid + 1:], base[mid + 1:])
    return by_root, by_er


def eps_sensitivity(case, eps=1e-6):
    """Move (the error measure, clip 0, all rows) of ONE LayerNorm taking `eps` for 1e-5: norm1 of the last decoder layer."""
    from unittest import mock
    T = case.sens_T or case.T
    cfg = case.config
    sd = state_dict(case, torch.float64)
    f64, _, roots, attrs = inputs(case, torch.float64)
    base = oracle_rows(sd, cfg["num_heads"], f64, roots, attrs, (0,), T)[0]
    target = (2 * cfg["n_layers"] + 1) + 3 * (cfg["n_layers"] - 1)          # calls before it: the encoder's, the earlier decoder layers'
    calls = []
    plain = O.layer_norm

    def one_wrong(x, w, b, eps_=O.LN_EPS):
        calls.append(1)
        return plain(x, w, b, eps if len(calls) - 1 == target else eps_)

    with mock.patch.object(O, "layer_norm", one_wrong):
        moved = oracle_rows(sd, cfg["num_heads"], f64, roots, attrs, (0,), T)[0]
    assert len(calls) == 5 * cfg["n_layers"] + 2
    return rel_err(moved, base)


# ---- the device side -----------------------------------------------------------------------------------------------------------
def build_model(case, sd=None, **ctor):
    """The case's model on the device with its options set; `sd` (default: the case's own state dict) and further constructor
    keywords are for tests/helpers_decode_free.py (a scaled output head, `chord_embed`)."""
    from video2music_amd.model.video_music_transformer import VideoMusicTransformer
    m = VideoMusicTransformer(**model_cfg(case), **ctor).eval()
    missing, unexpected = m.load_state_dict(state_dict(case) if sd is None else sd, strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing), (missing, unexpected)
    m.max_decode_batch = case.max_decode_batch
    if case.plain_option:
        m.decode_chain = "plain"                 # read when the handle is created: the option precedes the first amt_finalize
    m = m.cuda()
    for name, value in case.options:
        if name != "decode_chain_plain":
            m.set_option(name, value)
    return m


def feature_args(f):
    return f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"]


def teacher_forced_logits(m, f, toks, roots, attrs):
    """Logits (B, T-1, 159) of the decode step at input positions 0 .. T-2 of every clip, teacher-forced along (root, attr) ids (B, T)
    by a primer as long as the sequence: `generate_batch` with per-clip primers of T positions runs the real captured graphs (16 steps
    per graph plus the remainder) and returns row t = logits computed from input position t.

    Inside the primer the next position's root / attr come from the primer, not from the discarded decision: `sample_kernel` and
    `sample_fold_kernel` (sample.hip) read tokens / roots / attrs [b][cur] when cur < n_primer, the head fused into the next step's
    self-attention (attn_decode.hip, FOLD 5) reads roots / attrs [b][t] when t < n_primer and still writes the previous position's
    logits for a caller who asked.  The returned ids must therefore be `toks` untouched."""
    B, T = toks.shape
    with torch.no_grad():
        ids, lg = m.generate_batch(*feature_args(f), toks, roots, attrs, target_seq_length=T, beam=0, sampler="argmax", return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(ids.cpu(), toks), "a decision inside the primer was kept"
    lg = lg[:T - 1].permute(1, 0, 2).contiguous().cpu()
    assert lg.shape == (B, T - 1, K.CHORD_SIZE) and torch.isfinite(lg).all()
    return lg


def measured_launches_per_step(m, f):
    """Launches of one eagerly issued step (attention, skinny GEMMs and the sampling head) from `generate_profile` over 2 steps."""
    one = torch.tensor([1]), torch.tensor([1]), torch.tensor([0])
    _, stats = m.generate_profile(*feature_args(f), *one, target_seq_length=3)
    n = sum(stats[k]["launches"] for k in ("self_attn_decode", "cross_attn_decode", "decode_gemm", "sample"))
    assert n % 2 == 0
    return n // 2


def host_step_probs(m, f, toks, roots, attrs, max_conseq_N, max_conseq_chord):
    """Decision distributions (B, T-1, 157) of the host-driven step (`amt_generate_step_probs` / `amt_generate_commit`: the eager
    kernels and the stand-alone head), teacher-forced by the same full-length primer; the commit inside the primer keeps the given ids."""
    from video2music_amd import _lib
    B, T = toks.shape
    sem, key, scene, motion, emotion, Bf, S = m._prep_features(*feature_args(f))
    assert Bf == B <= m.max_decode_batch
    h = m._ensure_handle(sem.shape[2])
    st = _lib.stream_ptr()
    pr = [p.cuda().long().contiguous() for p in (toks, roots, attrs)]
    out = torch.empty(T - 1, B, K.CHORD_END, device="cuda")
    ids = torch.empty(B, T, device="cuda", dtype=torch.long)
    chosen = torch.zeros(B, device="cuda", dtype=torch.long)
    with torch.no_grad():
        m._encode(h, sem, scene, motion, emotion, slice(0, B))
        _lib.call("amt_generate_begin", h, B, _lib.ptr(pr[0]), _lib.ptr(pr[1]), _lib.ptr(pr[2]), T, 1, _lib.ptr(key), T, 0,
                  int(max_conseq_N), int(max_conseq_chord), st)
        for cur in range(1, T):
            _lib.call("amt_generate_step_probs", h, _lib.ptr(out[cur - 1]), st)
            _lib.call("amt_generate_commit", h, _lib.ptr(chosen), st)
        _lib.call("amt_generate_end", h, _lib.ptr(ids), st)
    torch.cuda.synchronize()
    assert torch.equal(ids.cpu(), toks), "a commit inside the primer replaced a given id"
    out = out.permute(1, 0, 2).contiguous().cpu()
    assert torch.isfinite(out).all()
    return out


def decision_rows(y, toks, max_conseq_N, max_conseq_chord):
    """softmax(y)[:157] of every row of `y` (B, T-1, 159) with the suppressions sample.hip applies at that position (id 0 when
    max_conseq_N == 0; the previous id when the last max_conseq_chord ids of `toks` are equal), not renormalised: the rule of
    `tests.helpers._decision_probs`, in the dtype of `y`."""
    B, L, _ = y.shape
    tk = toks.numpy()
    return torch.stack([torch.stack([torch.from_numpy(_decision_probs(y[b, t], tk, b, t + 1, max_conseq_N, max_conseq_chord, 1.0))
                                     for t in range(L)]) for b in range(B)])


def prob_err(got, ref):
    """max |got - ref| relative to the reference distribution's maximum."""
    return float((got.double() - ref.double()).abs().max() / float(ref.max()))
