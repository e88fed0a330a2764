"""Training of the V1 / V2 chord models: the restatements, case tables and bounds of tests/test_family_train_ops_gpu.py (operators),
tests/test_family_train_host.py and tests/test_family_train_gpu.py (models).

The fp64 truth is `oracle.amt_oracle`: `rope`, `rms_norm`, `glu_expert`, `forward_family` -- all torch, so fp64 leaves with
requires_grad give the gradients.  Where dropout multipliers are given the oracle has no argument for them; the restatements below are
then built from the oracle's own pieces (`linear`, `rope`, `rms_norm`, `layer_norm`, the mixture's routing rule) with the multipliers
put where the reference's nn.Dropout modules sit, and the host test holds them to `forward_family` where no multiplier is given.

Error measures are the project's: `rel_err` / `grad_scale` of tests/helpers_train_edges.py.  Bound per case: 8 x e32, e32 being the same
restatement run in float32 on the CPU at test time (8: another summation order plus a device exp); CAP = 1e-4 is the most a bound may be.
"""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import amt_oracle as O
from tests import helpers_family_parity as FP
from tests import helpers_train as T
from tests.helpers_train_edges import grad_scale, logit_err, rel_err
from video2music_amd import synthetic
from video2music_amd.utilities import constants as C

FACTOR = 8
CAP = 1e-4
MISS = 10
ROUTE_GAP = 1e-5
U = 2.0 ** -24


def cast(a, dtype, grad=False):
    return torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(grad)


def one_thread(fn, *args, **kw):
    """fn on one CPU thread, so that an fp32 run repeats."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn(*args, **kw)
    finally:
        torch.set_num_threads(n)


# ---- operators ------------------------------------------------------------------------------------------------------------------------
# RopeFn: (n0, seq, n2, hd), the d_model the cache is built for, its max_seq, what the shape exists for
ROPE_CASES = {
    "reinterpreted": ((4, 5, 3, 32), 128, 300, "n0 * hd equals the cache width: the [seq][64][2] cache read as [4][seq][16][2]"),
    "broadcast": ((1, 7, 1, 128), 128, 300, "hd equals the cache width: one slab for every leading index"),
    "last_row": ((2, 300, 2, 64), 128, 300, "position 299: the last cache row"),
    "hd2": ((3, 9, 2, 2), 6, 16, "one pair per head"),
}


def rope_inputs(name):
    shape, dim, max_seq, _ = ROPE_CASES[name]
    rng = np.random.default_rng(sum(shape) + dim)
    cache = O.rope_cache(dim, max_seq)                       # fp32, as the model builds it
    return rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32), cache


def rope_restated(x, dy, cache, dtype, conjugate=True):
    """(y, dx) of O.rope in `dtype` on the fp32 cache cast to it.  conjugate=False: the wrong adjoint that rotates dy forward again."""
    xt = cast(x, dtype, True)
    y = O.rope(xt, cache.to(dtype))
    if not conjugate:
        return y.detach().numpy(), O.rope(cast(dy, dtype), cache.to(dtype)).numpy()
    y.backward(cast(dy, dtype))
    return y.detach().numpy(), xt.grad.numpy()


def norm_bwd_plan_boundaries(limit=4096):
    """Row counts one below / at every change of the plan kind of the norm backward launchers (csrc/norm_bwd.hip, LayerNorm and RMSNorm
    alike): from one workgroup to several, and from 16 rows per workgroup to the even spread over all of them.  Asked from the launcher's
    own rule."""
    from video2music_amd import ops
    kind = lambda r: (ops.norm_bwd_blocks(r) > 1, -(-r // ops.norm_bwd_blocks(r)) > 16)
    return [r for edge in range(2, limit) if kind(edge) != kind(edge - 1) for r in (edge - 1, edge)]


RMS_EPS = 1e-6
RMS_GAIN = 0.1                      # gains and rows of this scale: mean squares of 1e-2, where eps 1e-6 vs 1e-5 shows


def rms_inputs(rows, dim, resid, zero_row=None):
    rng = np.random.default_rng(7 * rows + dim + int(resid))
    a = {"x": RMS_GAIN * rng.standard_normal((rows, dim)), "w": RMS_GAIN * (1.0 + 0.3 * rng.standard_normal(dim)),
         "dy": rng.standard_normal((rows, dim))}
    if resid:
        a["resid"] = 0.5 * RMS_GAIN * rng.standard_normal((rows, dim))
    if zero_row is not None:
        a["x"][zero_row] = 0.0
        if resid:
            a["resid"][zero_row] = 0.0
    return {k: v.astype(np.float32) for k, v in a.items()}


def rms_restated(a, dtype, eps=RMS_EPS):
    t = {k: cast(v, dtype, k != "dy") for k, v in a.items()}
    u = t["x"] + t["resid"] if "resid" in t else t["x"]
    y = O.rms_norm(u, t["w"], eps=eps)
    y.backward(t["dy"])
    out = {k: t[k].grad.numpy() for k in t if k != "dy"}
    out["y"] = y.detach().numpy()
    return out


def glu_inputs(n, d, dff, silu, masked, p=0.2):
    rng = np.random.default_rng(1000 * n + dff + 2 * int(silu) + int(masked))
    w = lambda *s: (rng.standard_normal(s) / np.sqrt(s[-1])).astype(np.float32)
    b = lambda m: (0.1 * rng.standard_normal(m)).astype(np.float32)
    if silu:
        sd = {"0.weight": w(dff, d), "0.bias": b(dff), "3.weight": w(d, dff), "3.bias": b(d)}
    else:
        sd = {"linear1.weight": w(dff, d), "linear1.bias": b(dff), "gate.weight": w(dff, d), "gate.bias": b(dff),
              "linear2.weight": w(d, dff), "linear2.bias": b(d)}
    a = {"x": rng.standard_normal((n, d)).astype(np.float32), "dy": rng.standard_normal((n, d)).astype(np.float32)}
    mask = ((rng.random((n, dff)) >= p) / (1.0 - p)).astype(np.float32) if masked else None
    return sd, a, mask


def expert_restated(x, sd, p, mask_h=None, mask_in_backward=True):
    """O.expert with the hidden Dropout's multipliers (model/moe.py:44-49: dropout(linear1(x) * silu(gate(x))); index 2 of a SiLU expert).
    mask_in_backward=False: the wrong variant whose backward forgets the mask."""
    if p + "linear1.weight" in sd:
        h = O.linear(x, sd[p + "linear1.weight"], sd[p + "linear1.bias"]) * F.silu(O.linear(x, sd[p + "gate.weight"], sd[p + "gate.bias"]))
        w2, b2 = sd[p + "linear2.weight"], sd[p + "linear2.bias"]
    else:
        h = F.silu(O.linear(x, sd[p + "0.weight"], sd[p + "0.bias"]))
        w2, b2 = sd[p + "3.weight"], sd[p + "3.bias"]
    if mask_h is not None:
        m = mask_h.to(h.dtype)
        h = h * m if mask_in_backward else h + (h * (m - 1.0)).detach()
    return O.linear(h, w2, b2)


def glu_restated(sd, a, mask, dtype):
    P = {k: cast(v, dtype, True) for k, v in sd.items()}
    x = cast(a["x"], dtype, True)
    y = expert_restated(x, P, "", None if mask is None else cast(mask, dtype))
    y.backward(cast(a["dy"], dtype))
    out = {k: v.grad.numpy() for k, v in P.items()}
    out["x"], out["y"] = x.grad.numpy(), y.detach().numpy()
    return out


def op_errors(got, r64, r32):
    """{key: (err, e32)} by `rel_err` against the fp64 run."""
    return {k: (rel_err(got[k], r64[k]), rel_err(r32[k], r64[k])) for k in r64}


# ---- models ---------------------------------------------------------------------------------------------------------------------------
LOGIT_FACTOR = FACTOR
N_EXPERTS, TOP_K = 6, 2
Case = namedtuple("Case", "name version n_layers d H dff L S B seed rms_norm chord_embed scene_embed mask p droptoken edge")


def _case(name, version, n_layers, L, S, B, seed, edge, d=64, H=2, dff=192, rms_norm=False, chord_embed=False, scene_embed=False, mask=True,
          p=0.0, droptoken=0.0):
    return Case(name, version, n_layers, d, H, dff, L, S, B, seed, rms_norm, chord_embed, scene_embed, mask, p, droptoken, edge)


# seed: of the weights (seed), the video features (seed + 1000), the ids and targets (seed + 2000) and the dropout multipliers
# (seed + 3000).  The seeds listed keep every mixture row's 2nd-vs-3rd gate-logit gap above ROUTE_GAP in fp64 and the bound under CAP
# (tests/test_family_train_host.py); a seed that fails either is replaced here, never skipped at run time.
CASES = [
    _case("default", "1.2.3", 2, 33, 17, 2, 11, "the reference default; raw rotary view with B = 2; learned tables; frozen chord table", chord_embed=True),
    _case("v22", "2.2", 4, 33, 40, 3, 32, "three GLU layers, then a shared GLU mixture; B = 3", dff=96, chord_embed=True),     # 12: a bound of 1.1e-4
    _case("v22_drop", "2.2", 4, 33, 40, 3, 13, "every dropout site and the row mask, multipliers given", dff=96, chord_embed=True, p=0.2,
          droptoken=0.3),
    _case("rms_hd128", "1.1", 1, 5, 3, 1, 14, "RMSNormFn in the model; head_dim 128; MoELayer without a shared expert", d=128, H=1, rms_norm=True),
    _case("shallow_se", "1.3.4", 4, 129, 17, 2, 15, "plain GLU layers, then a SiLU mixture; one row past a 128-query block", scene_embed=True),
    _case("one", "1.0", 1, 1, 1, 1, 16, "one token"),
    _case("nomask", "1.3", 1, 33, 17, 2, 17, "non-causal decoder self-attention", mask=False),
    _case("long", "1.2", 1, 300, 300, 2, 18, "last row of both tables and of the rotary cache; 600 tokens per mixture", d=128, H=2),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


def model_kwargs(c):
    kw = dict(version_name=c.version, n_layers=c.n_layers, num_heads=c.H, d_model=c.d, dim_feedforward=c.dff, dropout=c.p,
              max_sequence_chord=300, max_sequence_video=300, total_vf_dim=synthetic.total_vf_dim(1) - int(c.scene_embed),
              scene_embed=c.scene_embed, chord_embed=c.chord_embed, dropTokenRate=c.droptoken)
    if c.rms_norm:
        kw["rms_norm"] = True
    return kw


def built_layers(c):
    """Layers per stack the class builds: '1.3.3' / '1.3.4' and every V2 hold at least their three shallow ones."""
    return max(3, c.n_layers) if c.version in ("1.3.3", "1.3.4") or c.version[0] == "2" else c.n_layers


@functools.lru_cache(maxsize=None)
def state_dict(name):
    """Seeded fp32 state dict of case `name` ({key: numpy array}), norm gains of the rms_norm cases scaled as in helpers_family_parity."""
    c = BY_NAME[name]
    kw = model_kwargs(c)
    shapes = FP.named_shapes(c.version, built_layers(c), c.H, c.d, c.dff, kw["total_vf_dim"], rms_norm=c.rms_norm, chord_embed=c.chord_embed,
                             scene_embed=c.scene_embed)
    sd = synthetic.synthetic_state_dict(shapes, seed=c.seed)
    if c.rms_norm:
        sd = {k: (v * FP.RMS_GAIN).astype(v.dtype) if "norm" in k and k.endswith(".weight") else v for k, v in sd.items()}
    return sd


@functools.lru_cache(maxsize=None)
def inputs(name):
    c = BY_NAME[name]
    f = dict(synthetic.synthetic_features(c.B, seed=c.seed + 1000, n_frames=c.S))
    rs = np.random.RandomState(c.seed + 2000)
    f["ids"], f["root"], f["attr"] = rs.randint(0, 157, size=(c.B, c.L)), rs.randint(0, 15, size=(c.B, c.L)), rs.randint(0, 16, size=(c.B, c.L))
    f["tgt"] = rs.randint(0, C.CHORD_END, size=(c.B, c.L))
    f["emo_class"] = rs.randint(0, 6, size=(c.B, c.L)).astype(np.int32)
    if c.L >= 4:
        f["tgt"][0, -2], f["tgt"][0, -1] = C.CHORD_END, C.CHORD_PAD
    return f


def ff_plan(c, i):
    return FP._layer_plan(c.version, i)[2]                      # "glu" or (expert kind, shared, balancing)


def mask_shapes(c):
    """[(kind, shape)] of the multipliers one step takes, in the order of `VideoMusicTransformer_V2._forward_train`: "rows" the
    dropTokenRate mask, "keep" an attention's uint8 mask, "h" a plain GLU layer's hidden multipliers; then, per mixture layer in forward
    order, its own triple ("moe": [inside the experts, on their outputs, inside the shared expert])."""
    own, mix = [], []
    if c.droptoken:
        own.append(("rows", (c.B, c.S)))
    if c.p > 0:
        for stack, n, att in (("enc", c.S, [(c.S, c.S)]), ("dec", c.L, [(c.L, c.L), (c.L, c.S)])):
            for i in range(built_layers(c)):
                own += [("keep", (c.B, c.H, lq, lk)) for lq, lk in att]
                plan = ff_plan(c, i)
                raw = c.dff if plan == "glu" or plan[0] == "glu" else 2 * c.d
                if plan == "glu":
                    own.append(("h", (n * c.B, raw)))
                else:
                    mix.append([(n * c.B * TOP_K, raw), (n * c.B * TOP_K, c.d)] + ([(n * c.B, raw)] if plan[1] else []))
    return own, mix


@functools.lru_cache(maxsize=None)
def masks(name):
    """(the model's list, the mixture layers' lists) of numpy multipliers, or (None, None) for a case without dropout."""
    c = BY_NAME[name]
    own, mix = mask_shapes(c)
    if not own and not mix:
        return None, None
    rng = np.random.default_rng(c.seed + 3000)
    el = lambda s: ((rng.random(s) >= c.p) / (1.0 - c.p)).astype(np.float32)
    draw = {"rows": lambda s: (rng.random(s) > c.droptoken).astype(np.float32), "keep": lambda s: (rng.random(s) >= c.p).astype(np.uint8), "h": el}
    return [draw[k](s) for k, s in own], [[el(s) for s in layer] for layer in mix]


def grad_errors(got, g64):
    """{key: rel_err against the fp64 gradient at `grad_scale`}.  A gradient that is identically zero in fp64 (an expert no token was
    routed to) has nothing to be relative to: it must be zero in `got` too, bit for bit (error 0, else inf)."""
    out = {}
    for k, g in g64.items():
        if g is None:
            continue
        if np.abs(g).max() > 0:
            out[k] = rel_err(got[k], g, grad_scale(g64, k))
        else:
            out[k] = 0.0 if not np.asarray(got[k]).any() else float("inf")
    return out


VARIANTS = ("rope_unconjugated", "rms_eps_1e-5", "glu_mask_forward_only", "shared_without_1_over_k", "chord_table_gradient", "keep_unscaled")


class _RopeWrongAdjoint(torch.autograd.Function):
    """O.rope whose backward rotates the gradient forward again instead of back."""

    @staticmethod
    def forward(ctx, x, cache):
        ctx.save_for_backward(cache)
        return O.rope(x, cache)

    @staticmethod
    def backward(ctx, dy):
        return O.rope(dy, ctx.saved_tensors[0]), None


def forward_restated(P, c, f, own=None, mix=None, wrong=(), collect=None, table64=False):
    """`O.forward_family` for the V1 / V2 members, from the oracle's pieces, with the multipliers of `mask_shapes` where the reference's
    Dropout modules sit: on the attention probabilities (scaled by 1 / (1 - p)), on a plain expert's hidden, inside the mixtures (rows by
    seq-first token), and the dropTokenRate rows.  P: {key: tensor}, leaves that may require grad.  wrong: names of VARIANTS.
    The rotary table is the model's own fp32 one cast to P's dtype, as every device path reads it (`O.forward_v2` does the same);
    table64: built in P's dtype instead, as `O.forward_family` builds it, for the comparison with that function."""
    assert all(w in VARIANTS for w in wrong)
    dt = P["Wout.weight"].dtype
    d, H = c.d, c.H
    hd = d // H
    own = None if own is None else [torch.as_tensor(m) for m in own]
    mix = None if mix is None else [[torch.as_tensor(m).to(dt) for m in layer] for layer in mix]
    learned_pos, rope_mult, _ = O.family_plan(c.version)
    cache = None if rope_mult is None else O.rope_cache(d, 300, dtype=dt) if table64 else O.rope_cache(d, 300).to(dt)
    rms_eps = 1e-5 if "rms_eps_1e-5" in wrong else 1e-6
    fl = lambda k: torch.as_tensor(f[k]).to(dt)
    take = lambda: own.pop(0)

    def norm(x, p):
        if p + "bias" in P:
            return O.layer_norm(x, P[p + "weight"], P[p + "bias"])
        return O.rms_norm(x, P[p + "weight"], eps=rms_eps)

    def rot(x):
        return _RopeWrongAdjoint.apply(x, cache) if "rope_unconjugated" in wrong else O.rope(x, cache)

    def attention(xq, xkv, p, causal):                          # O.v2_attention with the keep mask on the probabilities
        L, B, E = xq.shape
        S = xkv.shape[0]
        W, b = P[p + "in_proj_weight"], P[p + "in_proj_bias"]
        q = O.linear(xq, W[:E], b[:E]).contiguous()
        k = O.linear(xkv, W[E:2 * E], b[E:2 * E]).contiguous()
        v = O.linear(xkv, W[2 * E:], b[2 * E:]).contiguous()
        if cache is not None:
            q = rot(q.view(H, L, B, hd)).reshape(L, B, E)
            k = rot(k.view(H, S, B, hd)).reshape(S, B, E)
        qh = q.reshape(L, B * H, hd).transpose(0, 1) * (1.0 / float(hd)) ** 0.5
        kh = k.reshape(S, B * H, hd).transpose(0, 1)
        vh = v.reshape(S, B * H, hd).transpose(0, 1)
        s = qh @ kh.transpose(-1, -2)
        if causal:
            s = s + torch.triu(torch.full((L, S), float("-inf"), dtype=s.dtype), diagonal=1)
        a = torch.softmax(s, dim=-1)
        if own is not None and c.p > 0:
            a = a * take().to(dt).reshape(B * H, L, S) / (1.0 if "keep_unscaled" in wrong else 1.0 - c.p)
        o = (a @ vh).transpose(0, 1).contiguous().view(L * B, E)
        return O.linear(o, P[p + "out_proj.weight"], P[p + "out_proj.bias"]).view(L, B, E)

    fwd_only = "glu_mask_forward_only" in wrong

    def ff(x, p):
        n, B, _ = x.shape
        rows = x.reshape(n * B, d)
        if p + "linear1.weight" in P:
            m = take().to(dt) if own is not None and c.p > 0 else None
            return expert_restated(rows, P, p, m, not fwd_only).view(n, B, d)
        logits = O.linear(rows, P[p + "gate.weight"], P[p + "gate.bias"])
        if collect is not None:
            collect.append(logits.detach())
        shared = p + "shared_expert.linear2.weight" in P or p + "shared_expert.3.weight" in P
        lm = mix.pop(0) if mix is not None and c.p > 0 else []
        mh, my, mhs = (lm + [None] * 3)[:3]
        top, idx = torch.topk(logits, TOP_K, dim=-1)
        w = torch.softmax(top, dim=-1)
        out = torch.zeros_like(rows)
        for e in range(N_EXPERTS):                              # an expert without a token still runs, on zero rows: its gradients are zeros
            tok, j = torch.where(idx == e)
            a = tok * TOP_K + j
            y = expert_restated(rows[tok], P, f"{p}experts.{e}.", None if mh is None else mh[a])
            if my is not None:
                y = y * my[a]
            out = out.index_add(0, tok, w[tok, j].unsqueeze(1) * y)
        if shared:
            out = out + (1.0 if "shared_without_1_over_k" in wrong else 1.0 / TOP_K) * expert_restated(rows, P, p + "shared_expert.", mhs)
        return out.view(n, B, d)

    ids = torch.as_tensor(f["ids"] if c.chord_embed else f["root"])
    if c.chord_embed:
        x = P["chord_embedding_model.weight"][ids]
        if "chord_table_gradient" not in wrong:
            x = x.detach()
    else:
        x = P["embedding_root.weight"][ids] + P["embedding_attr.weight"][torch.as_tensor(f["attr"])]
    B, L, _ = x.shape
    kk = fl("key").reshape(-1)
    kk = kk.expand(B) if kk.numel() == 1 else kk
    x = O.linear(torch.cat([x, kk.view(B, 1, 1).expand(B, L, 1)], dim=-1), P["Linear_chord.weight"], P["Linear_chord.bias"])
    motion = fl("motion")
    cols = [fl("semantic")] + ([] if c.scene_embed else [fl("scene_offset").unsqueeze(-1)]) + [motion.unsqueeze(-1) if motion.dim() == 2 else motion,
                                                                                                fl("emotion")]
    vf = O.linear(torch.cat(cols, dim=-1), P["Linear_vis.weight"], P["Linear_vis.bias"])
    if c.scene_embed:
        vf = vf + P["scene_embedding.weight"][torch.as_tensor(f["scene_offset"]).to(torch.int32).long()]
    if own is not None and c.droptoken:
        vf = vf * take().to(dt).unsqueeze(-1)
    S = vf.shape[1]
    t, src = x.permute(1, 0, 2).contiguous(), vf.permute(1, 0, 2).contiguous()
    if learned_pos:
        t = t + P["positional_embedding.weight"][:L].unsqueeze(1)
        src = src + P["positional_embedding_video.weight"][:S].unsqueeze(1)
    for i in range(O.n_layers_of(P, "encoder")):
        p = f"transformer.encoder.layers.{i}."
        src = norm(src + attention(src, src, p + "self_attn.", False), p + "norm1.")
        src = norm(src + ff(src, p + "ff."), p + "norm2.")
    memory = norm(src, "transformer.encoder.norm.")
    for i in range(O.n_layers_of(P, "decoder")):
        p = f"transformer.decoder.layers.{i}."
        t = norm(t + attention(t, t, p + "self_attn.", c.mask is True), p + "norm1.")
        t = norm(t + attention(t, memory, p + "cross_attn.", False), p + "norm2.")
        t = norm(t + ff(t, p + "ff."), p + "norm3.")
    t = norm(t, "transformer.decoder.norm.")
    assert not own and not mix
    return O.linear(t.permute(1, 0, 2), P["Wout.weight"], P["Wout.bias"])


def run_case(c, sd, f, own, mix, dtype, wrong=(), table64=False):
    """(losses (3,), logits, {key: gradient or None}, gate logits of the mixture layers) of the restatement of case `c` on state dict `sd`
    and inputs `f` (numpy arrays)."""
    P = {k: cast(v, dtype, True) for k, v in sd.items()}
    gates = []
    logits = forward_restated(P, c, f, own, mix, wrong, gates, table64)
    total, chord, emotion = T.loss(logits, f)
    total.backward()
    return (np.array([float(total.detach()), float(chord.detach()), float(emotion.detach())]), logits.detach().numpy(),
            {k: None if q.grad is None else q.grad.numpy() for k, q in P.items()}, gates)


def run(name, dtype, wrong=()):
    """`run_case` on the inputs, weights and multipliers of case `name` of the table."""
    return run_case(BY_NAME[name], state_dict(name), inputs(name), *masks(name), dtype, wrong)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's fp64 and fp32 restatement (fp32 on one CPU thread) and its noise levels; shared by the tests of a process, read-only."""
    r64 = run(name, torch.float64)
    r32 = one_thread(run, name, torch.float32)
    yl = torch.from_numpy(r64[1]).requires_grad_(True)
    T.loss(yl, inputs(name))[0].backward()
    return dict(l64=r64[0], y64=r64[1], g64=r64[2], gates=r64[3], l32=r32[0], y32=r32[1], g32=r32[2],
                e32=max(grad_errors(r32[2], r64[2]).values()), e32_y=logit_err(r32[1], r64[1]), dl_dy_sum=float(yl.grad.abs().sum()))


def loss_bound(ref):
    """|loss - l64| <= D sum |dL/dy| + 159 U |l64|, D the logits bound in absolute terms (tests/helpers_train_edges.py)."""
    D = LOGIT_FACTOR * ref["e32_y"] * max(1.0, float(np.abs(ref["y64"]).max()))
    return D * ref["dl_dy_sum"] + 159 * U * abs(ref["l64"][0])


def route_gap(gates):
    return FP.route_gap(gates)


def variant_miss(name, variant):
    """Worst gradient error / (8 e32) of a wrong variant in fp64 against the case's fp64 reference (a gradient that is None on one side
    only counts as an infinite miss)."""
    ref = reference(name)
    _, y, g, _ = run(name, torch.float64, (variant,))
    if {k for k, v in g.items() if v is None} != {k for k, v in ref["g64"].items() if v is None}:
        return float("inf")
    return max(max(grad_errors(g, ref["g64"]).values()) / (FACTOR * ref["e32"]), logit_err(y, ref["y64"]) / (LOGIT_FACTOR * ref["e32_y"]))


# ---- against the reference's own run (tools/make_goldens_train_families.py, tests/test_train_families_gpu.py) --------------------------
# the two models g_train_families.npz records, on the miniature dataset of tests/helpers_eval.py (both clips in one batch, 299 chord
# positions, 300 frames, 24 semantic features + scene offset + scalar motion + 6 emotions), dropout 0, synthetic weights of seed 0
GOLDEN_VF = 24 + 1 + 1 + 6
GOLDEN = {"v123": _case("v123", "1.2.3", 2, T.L_CHORD, T.S_VIDEO, T.B_CLIPS, 0, "the reference default", dff=128, chord_embed=True),
          "v22": _case("v22", "2.2", 4, T.L_CHORD, T.S_VIDEO, T.B_CLIPS, 0, "three GLU layers and a shared mixture", dff=128, chord_embed=True)}
# the keys whose fp32 gradient is recorded: every parameter kind of the two models
GOLDEN_KEYS = {
    "v123": ("Linear_vis.weight", "Linear_vis.bias", "Linear_chord.weight", "Linear_chord.bias", "positional_embedding.weight",
             "positional_embedding_video.weight", "Wout.weight", "Wout.bias", "transformer.encoder.layers.0.self_attn.in_proj_weight",
             "transformer.encoder.layers.0.self_attn.in_proj_bias", "transformer.decoder.layers.1.self_attn.out_proj.weight",
             "transformer.decoder.layers.1.cross_attn.in_proj_weight", "transformer.decoder.layers.1.norm2.weight",
             "transformer.decoder.layers.1.norm3.bias", "transformer.encoder.norm.weight", "transformer.decoder.layers.0.ff.gate.weight",
             "transformer.decoder.layers.0.ff.gate.bias", "transformer.decoder.layers.0.ff.experts.2.0.weight",
             "transformer.decoder.layers.0.ff.experts.2.0.bias", "transformer.decoder.layers.0.ff.experts.2.3.weight",
             "transformer.encoder.layers.1.ff.shared_expert.0.weight", "transformer.encoder.layers.1.ff.shared_expert.3.bias"),
    "v22": ("Linear_vis.weight", "Linear_chord.weight", "Wout.weight", "transformer.encoder.layers.0.self_attn.in_proj_weight",
            "transformer.decoder.layers.2.cross_attn.in_proj_weight", "transformer.decoder.layers.2.cross_attn.out_proj.bias",
            "transformer.decoder.layers.3.norm3.weight", "transformer.decoder.norm.bias", "transformer.encoder.layers.1.ff.linear1.weight",
            "transformer.encoder.layers.1.ff.linear1.bias", "transformer.decoder.layers.0.ff.gate.weight", "transformer.decoder.layers.0.ff.gate.bias",
            "transformer.decoder.layers.2.ff.linear2.weight", "transformer.decoder.layers.2.ff.linear2.bias",
            "transformer.decoder.layers.3.ff.gate.weight", "transformer.decoder.layers.3.ff.gate.bias",
            "transformer.decoder.layers.3.ff.experts.4.linear1.weight", "transformer.decoder.layers.3.ff.experts.4.gate.bias",
            "transformer.encoder.layers.3.ff.experts.0.linear2.weight", "transformer.encoder.layers.3.ff.shared_expert.gate.weight",
            "transformer.encoder.layers.3.ff.shared_expert.linear2.bias"),
}


def golden_kwargs(tag):
    return dict(model_kwargs(GOLDEN[tag]), total_vf_dim=GOLDEN_VF)


@functools.lru_cache(maxsize=None)
def golden_state_dict(tag):
    c = GOLDEN[tag]
    return synthetic.synthetic_state_dict(FP.named_shapes(c.version, built_layers(c), c.H, c.d, c.dff, GOLDEN_VF, chord_embed=True), seed=0)


def golden_inputs():
    bt = T.batch()
    return dict(bt, ids=bt["x"], root=bt["x_root"], attr=bt["x_attr"])


@functools.lru_cache(maxsize=None)
def golden_fp64(tag):
    """(losses, logits, gradients, gates) of `O.forward_family`'s arithmetic in fp64 (the restatement with the rotary table built in
    double, which the host test holds equal to that function) on the recorded models."""
    return run_case(GOLDEN[tag], golden_state_dict(tag), golden_inputs(), None, None, torch.float64, table64=True)
