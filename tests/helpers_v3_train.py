"""Training of the V3 chord models and of '2.2' with balancing: the case table, state dicts, inputs, restatement and bounds of
tests/test_v3_train_host.py, tests/test_v3_train_ops_gpu.py and tests/test_v3_train_gpu.py.

The fp64 truth is `oracle.amt_oracle`'s arithmetic (`diff_attention`, `forward_family`: torch, so fp64 leaves give gradients).  The
oracle is an eval forward: it has no argument for dropout multipliers and ignores the routing bias.  `forward_restated` below is built
from the oracle's pieces (`linear`, `rope`, `rms_norm`, `layer_norm`) with, in training mode, the selection on `logits + bias`, the
weights from the raw logits (reference model/moe.py:257-268), the multipliers where tests/helpers_family_train.py places them, and the
per-layer counts and expected bias after the step in fp32 torch arithmetic (moe.py:270-279).  The host test holds it equal to
`O.forward_family` with zero bias.

Error measures, FACTOR, CAP, MISS, ROUTE_GAP and U are those of tests/helpers_family_train.py.  Two things have a measure of their own:

The lambda vectors.  dlambda = -sum du o2 is a sum with heavy cancellation (the norm is scale-invariant; with one key both maps are
[1] and dlambda is 0 analytically), so the gradient of each lambda vector is compared at the scale A max|dlambda / dvector| with
A = sum over rows and columns of |du o2|, collected in fp64 from the restatement.  Bound: max(FACTOR e32_lambda, FACTOR U), e32_lambda
the maximum over the case's attentions (one scalar is too noisy a sample), the floor one fp32 rounding times the project's factor.

The routing bias.  Zero or synthetic buffers never change a selection; each `ff.bias` is set to std(gate logits of that layer in the
zero-bias fp64 forward) x linspace(-1, 1, 6)[3, 0, 5, 1, 4, 2].
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle import amt_oracle as O
from tests import helpers_family_parity as FP
from tests import helpers_family_train as FT
from tests import helpers_train as T
from tests.helpers_family_train import CAP, FACTOR, MISS, ROUTE_GAP, U, cast, expert_restated, one_thread
from tests.helpers_train_edges import grad_scale, logit_err, rel_err
from video2music_amd import synthetic
from video2music_amd.utilities import constants as C

LOGIT_FACTOR = FACTOR
N_EXPERTS, TOP_K = 6, 2
UPDATE_RATE = 0.001
BIAS_ORDER = (3, 0, 5, 1, 4, 2)
LAMBDA_NAMES = ("lambda_q1", "lambda_k1", "lambda_q2", "lambda_k2")
Case = namedtuple("Case", "name version n_layers d H dff L S B seed balancing p droptoken edge")


def _case(name, version, n_layers, d, H, L, S, B, seed, edge, balancing=True, p=0.0, droptoken=0.0):
    return Case(name, version, n_layers, d, H, 96, L, S, B, seed, balancing, p, droptoken, edge)


# seed: of the weights (seed), the video features (seed + 1000), the ids and targets (seed + 2000) and the multipliers (seed + 3000).
# The seeds listed keep, for every balancing layer, >= 25 % of the rows on another expert pair than without the bias and the biased
# 2nd-vs-3rd gap above ROUTE_GAP in fp64, and every bound under CAP (tests/test_v3_train_host.py); a seed that fails is replaced here.
CASES = [
    _case("c30", "3.0", 4, 64, 2, 33, 17, 2, 21, "V2 attention with the 2d rotary cache in the encoder, differential decoder, one balancing mixture per stack"),
    _case("c31", "3.1", 4, 64, 2, 33, 17, 2, 22, "differential attention in both stacks"),
    _case("c32", "3.2", 4, 64, 2, 33, 17, 2, 23, "pre-norm"),
    _case("c31_hd128", "3.1", 3, 128, 1, 129, 40, 3, 24, "head_dim 128, one row past a 128-query block, B = 3 through the raw views"),
    _case("c32_hd64", "3.2", 3, 128, 2, 5, 3, 1, 25, "head_dim 64, S below one key tile"),
    _case("c31_one", "3.1", 3, 64, 2, 1, 1, 1, 26, "one query, one key: dlambda is 0 in exact arithmetic"),
    _case("c31_long", "3.1", 4, 128, 2, 300, 300, 2, 27, "last rotary row, split-key forward, 600 tokens per mixture"),
    _case("c30_drop", "3.0", 4, 64, 2, 33, 17, 2, 28, "p = 0.2 at every dropout site and dropTokenRate 0.3, multipliers given", p=0.2, droptoken=0.3),
    _case("c22_bal", "2.2", 4, 64, 2, 33, 40, 3, 29, "-balancing on the V2 class"),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


def model_kwargs(c):
    kw = dict(version_name=c.version, n_layers=c.n_layers, num_heads=c.H, d_model=c.d, dim_feedforward=c.dff, dropout=c.p,
              max_sequence_chord=300, max_sequence_video=300, total_vf_dim=synthetic.total_vf_dim(1), scene_embed=False, chord_embed=False,
              dropTokenRate=c.droptoken)
    if c.version[0] == "2":
        kw["balancing"] = c.balancing
    return kw


def built_layers(c):
    return max(3, c.n_layers)


def bias_keys(sd):
    return sorted((k for k in sd if k.endswith(".ff.bias")), key=lambda k: (k.split(".")[1] != "encoder", k))


def _features(c):
    f = dict(synthetic.synthetic_features(c.B, seed=c.seed + 1000, n_frames=c.S))
    rs = np.random.RandomState(c.seed + 2000)
    f["ids"], f["root"], f["attr"] = rs.randint(0, 157, size=(c.B, c.L)), rs.randint(0, 15, size=(c.B, c.L)), rs.randint(0, 16, size=(c.B, c.L))
    f["tgt"] = rs.randint(0, C.CHORD_END, size=(c.B, c.L))
    f["emo_class"] = rs.randint(0, 6, size=(c.B, c.L)).astype(np.int32)
    if c.L >= 4:
        f["tgt"][0, -2], f["tgt"][0, -1] = C.CHORD_END, C.CHORD_PAD
    return f


@functools.lru_cache(maxsize=None)
def inputs(name):
    return _features(BY_NAME[name])


@functools.lru_cache(maxsize=None)
def state_dict(name):
    """Seeded fp32 state dict of case `name` ({key: numpy array}) with the case bias in every `ff.bias` buffer."""
    c = BY_NAME[name]
    shapes = FP.named_shapes(c.version, built_layers(c), c.H, c.d, c.dff, synthetic.total_vf_dim(1))
    if c.version[0] == "2" and c.balancing:
        shapes = list(shapes) + [(f"transformer.{s}.layers.{i}.ff.bias", (N_EXPERTS, 1)) for s in ("encoder", "decoder")
                                 for i in range(3, built_layers(c))]
    sd = synthetic.synthetic_state_dict(shapes, seed=c.seed)
    keys = bias_keys(sd)
    for k in keys:
        sd[k] = np.zeros((N_EXPERTS, 1), dtype=np.float32)
    gates = []
    with torch.no_grad():
        forward_restated({k: cast(v, torch.float64) for k, v in sd.items()}, c, inputs(name), collect=gates, training=False)
    assert len(gates) == len(keys)
    pattern = np.linspace(-1.0, 1.0, N_EXPERTS)[list(BIAS_ORDER)]
    for k, g in zip(keys, gates):
        sd[k] = (float(g["logits"].std()) * pattern).astype(np.float32).reshape(N_EXPERTS, 1)
    return sd


def mask_shapes(c):
    """[(kind, shape)] of the multipliers one step takes, in the order of `VideoMusicTransformer_V2._forward_train` (a differential
    attention contributes none), then per mixture layer in forward order its own triple."""
    own, mix = [], []
    if c.droptoken:
        own.append(("rows", (c.B, c.S)))
    if c.p > 0:
        for stack, n, att in (("enc", c.S, [(c.S, c.S)]), ("dec", c.L, [(c.L, c.L), (c.L, c.S)])):
            for i in range(built_layers(c)):
                enc_kind, dec_kind, plan = FP._layer_plan(c.version, i)
                if (enc_kind if stack == "enc" else dec_kind) == "mha":
                    own += [("keep", (c.B, c.H, lq, lk)) for lq, lk in att]
                if plan == "glu":
                    own.append(("h", (n * c.B, c.dff)))
                else:
                    mix.append([(n * c.B * TOP_K, c.dff), (n * c.B * TOP_K, c.d), (n * c.B, c.dff)])
    return own, mix


@functools.lru_cache(maxsize=None)
def masks(name):
    c = BY_NAME[name]
    own, mix = mask_shapes(c)
    if not own and not mix:
        return None, None
    rng = np.random.default_rng(c.seed + 3000)
    el = lambda s: ((rng.random(s) >= c.p) / (1.0 - c.p)).astype(np.float32)
    draw = {"rows": lambda s: (rng.random(s) > c.droptoken).astype(np.float32), "keep": lambda s: (rng.random(s) >= c.p).astype(np.uint8), "h": el}
    return [draw[k](s) for k, s in own], [[el(s) for s in layer] for layer in mix]


# ---- the differential attention ---------------------------------------------------------------------------------------------------------
VARIANTS = ("bias_ignored", "weights_biased", "d_o2_without_lambda", "dv_first_map_only", "dw_without_out_scale", "lambda_init_depth0",
            "subln_eps_1e-6")


def _grad_as(x, factor_value, factor_grad):
    """x * factor_value in the forward, x's gradient scaled by factor_grad instead (factor_value's own gradient is kept)."""
    return factor_value * x.detach() + factor_grad * (x - x.detach())


def diff_maps(q, k, v, B, H, Lq, Lk, hd, causal):
    """(o1, o2) (B, H, Lq, hd): the two softmax maps' outputs from the rotated q (Lq B 2E values), k and v (Lk B E values) read through
    the raw (B, L, 2H, hd) / (B, S, H, hd) views (`O.diff_attention`, custom_transformer.py:787-821), v given per map."""
    qh = q.reshape(B, Lq, 2 * H, hd).transpose(1, 2) * (float(hd) ** -0.5)
    kh = k.reshape(B, Lk, 2 * H, hd).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2)
    if causal:
        s = s + torch.triu(torch.full((Lq, Lk), float("-inf"), dtype=s.dtype), diagonal=1 + Lk - Lq)
    a = torch.softmax(s, dim=-1).view(B, H, 2, Lq, Lk)
    v1, v2 = v
    return a[:, :, 0] @ v1.reshape(B, Lk, H, hd).transpose(1, 2), a[:, :, 1] @ v2.reshape(B, Lk, H, hd).transpose(1, 2)


def diff_tail(o1, o2, lam, w, out_scale, eps, wrong=(), collect=None, tag=None):
    """RMSNorm_hd(o1 - lam o2) w out_scale; collect gets (tag, u, o2) with u's gradient retained."""
    t2 = _grad_as(o2, lam, 1.0) if "d_o2_without_lambda" in wrong else lam * o2
    u = o1 - t2
    if collect is not None and u.requires_grad:
        u.retain_grad()
        collect.append((tag, u, o2))
    we = _grad_as(w, out_scale, 1.0) if "dw_without_out_scale" in wrong else w * out_scale
    return u * torch.rsqrt(u.pow(2).mean(-1, keepdim=True) + eps) * we


def lambda_of(P, p, depth, wrong=()):
    lam_init = O.lambda_init_of(0 if "lambda_init_depth0" in wrong else depth)
    return torch.exp(torch.sum(P[p + "lambda_q1"] * P[p + "lambda_k1"])) - torch.exp(torch.sum(P[p + "lambda_q2"] * P[p + "lambda_k2"])) + lam_init, lam_init


def forward_restated(P, c, f, own=None, mix=None, wrong=(), collect=None, training=True, tails=None, table64=False):
    """`O.forward_family` for the V3 members and '2.2' with balancing, from the oracle's pieces.  training: the mixtures select on
    logits + bias and weigh with the raw logits, and the multipliers of `mask_shapes` sit where the reference's Dropout modules do;
    otherwise the eval forward (bias ignored).  collect: per mixture layer, encoder first, a dict of its gate logits, selection values,
    chosen experts, counts and the bias after the step.  tails: per differential attention (prefix, u, o2)."""
    assert all(w in VARIANTS for w in wrong)
    dt = P["Wout.weight"].dtype
    d, H = c.d, c.H
    hd = d // H
    own = None if own is None else [torch.as_tensor(m) for m in own]
    mix = None if mix is None else [[torch.as_tensor(m).to(dt) for m in layer] for layer in mix]
    _, rope_mult, pre_norm = O.family_plan(c.version)
    cache = O.rope_cache(rope_mult * d, 300, dtype=dt) if table64 else O.rope_cache(rope_mult * d, 300).to(dt)
    fl = lambda k: torch.as_tensor(f[k]).to(dt)
    take = lambda: own.pop(0)
    subln_eps = 1e-6 if "subln_eps_1e-6" in wrong else 1e-5

    def norm(x, p):
        if p + "bias" in P:
            return O.layer_norm(x, P[p + "weight"], P[p + "bias"])
        return O.rms_norm(x, P[p + "weight"], eps=1e-6)

    def mha(xq, xkv, p, causal):                                # tests/helpers_family_train.py's, the rotary table the model's own
        L, B, E = xq.shape
        S = xkv.shape[0]
        W, b = P[p + "in_proj_weight"], P[p + "in_proj_bias"]
        q = O.linear(xq, W[:E], b[:E]).contiguous()
        k = O.linear(xkv, W[E:2 * E], b[E:2 * E]).contiguous()
        v = O.linear(xkv, W[2 * E:], b[2 * E:]).contiguous()
        q = O.rope(q.view(H, L, B, hd), cache).reshape(L, B, E)
        k = O.rope(k.view(H, S, B, hd), cache).reshape(S, B, E)
        qh = q.reshape(L, B * H, hd).transpose(0, 1) * (1.0 / float(hd)) ** 0.5
        kh = k.reshape(S, B * H, hd).transpose(0, 1)
        vh = v.reshape(S, B * H, hd).transpose(0, 1)
        s = qh @ kh.transpose(-1, -2)
        if causal:
            s = s + torch.triu(torch.full((L, S), float("-inf"), dtype=s.dtype), diagonal=1)
        a = torch.softmax(s, dim=-1)
        if own is not None and c.p > 0:
            a = a * take().to(dt).reshape(B * H, L, S) / (1.0 - c.p)
        o = (a @ vh).transpose(0, 1).contiguous().view(L * B, E)
        return O.linear(o, P[p + "out_proj.weight"], P[p + "out_proj.bias"]).view(L, B, E)

    def attention(xq, xkv, p, causal, depth):
        if p + "q_proj.weight" not in P:
            return mha(xq, xkv, p, causal)
        L, B, E = xq.shape
        S = xkv.shape[0]
        q = O.linear(xq, P[p + "q_proj.weight"]).contiguous()
        k = O.linear(xkv, P[p + "k_proj.weight"]).contiguous()
        v = O.linear(xkv, P[p + "v_proj.weight"]).contiguous()
        q = O.rope(q.view(2 * H, L, B, hd), cache).contiguous()
        k = O.rope(k.view(2 * H, S, B, hd), cache).contiguous()
        o1, o2 = diff_maps(q, k, (v, v.detach() if "dv_first_map_only" in wrong else v), B, H, L, S, hd, causal)
        lam, lam_init = lambda_of(P, p, depth, wrong)
        o = diff_tail(o1, o2, lam, P[p + "subln.weight"], 1.0 - lam_init, subln_eps, wrong, tails, p)
        return O.linear(o.contiguous().view(L, B, E), P[p + "out_proj.weight"])

    def ff(x, p):
        n, B, _ = x.shape
        rows = x.reshape(n * B, d)
        if p + "linear1.weight" in P:
            m = take().to(dt) if own is not None and c.p > 0 else None
            return expert_restated(rows, P, p, m).view(n, B, d)
        logits = O.linear(rows, P[p + "gate.weight"], P[p + "gate.bias"])
        lm = mix.pop(0) if mix is not None and c.p > 0 else []
        mh, my, mhs = (lm + [None] * 3)[:3]
        biased = training and p + "bias" in P
        sel = logits + P[p + "bias"].detach().reshape(1, N_EXPERTS) if biased and "bias_ignored" not in wrong else logits
        _, idx = torch.topk(sel, TOP_K, dim=-1)
        raw = torch.gather(sel if "weights_biased" in wrong else logits, -1, idx)
        w = torch.softmax(raw, dim=-1)
        if collect is not None:
            rec = {"logits": logits.detach(), "sel": sel.detach(), "idx": idx}
            if biased:
                cnt = torch.bincount(idx.flatten(), minlength=N_EXPERTS).to(torch.float32)
                b32 = P[p + "bias"].detach().to(torch.float32)
                rec["counts"], rec["bias_after"] = cnt, b32 + UPDATE_RATE * (torch.mean(cnt) - cnt).unsqueeze(1)
            collect.append(rec)
        out = torch.zeros_like(rows)
        for e in range(N_EXPERTS):
            tok, j = torch.where(idx == e)
            a = tok * TOP_K + j
            y = expert_restated(rows[tok], P, f"{p}experts.{e}.", None if mh is None else mh[a])
            if my is not None:
                y = y * my[a]
            out = out.index_add(0, tok, w[tok, j].unsqueeze(1) * y)
        out = out + (1.0 / TOP_K) * expert_restated(rows, P, p + "shared_expert.", mhs)
        return out.view(n, B, d)

    x = P["embedding_root.weight"][torch.as_tensor(f["root"])] + P["embedding_attr.weight"][torch.as_tensor(f["attr"])]
    B, L, _ = x.shape
    kk = fl("key").reshape(-1)
    kk = kk.expand(B) if kk.numel() == 1 else kk
    x = O.linear(torch.cat([x, kk.view(B, 1, 1).expand(B, L, 1)], dim=-1), P["Linear_chord.weight"], P["Linear_chord.bias"])
    motion = fl("motion")
    cols = [fl("semantic"), fl("scene_offset").unsqueeze(-1), motion.unsqueeze(-1) if motion.dim() == 2 else motion, fl("emotion")]
    vf = O.linear(torch.cat(cols, dim=-1), P["Linear_vis.weight"], P["Linear_vis.bias"])
    if own is not None and c.droptoken:
        vf = vf * take().to(dt).unsqueeze(-1)
    t, src = x.permute(1, 0, 2).contiguous(), vf.permute(1, 0, 2).contiguous()
    causal = True
    for i in range(O.n_layers_of(P, "encoder")):
        p = f"transformer.encoder.layers.{i}."
        if pre_norm:
            h = norm(src, p + "norm1.")
            src = src + attention(h, h, p + "self_attn.", False, i)
            src = src + ff(norm(src, p + "norm2."), p + "ff.")
        else:
            src = norm(src + attention(src, src, p + "self_attn.", False, i), p + "norm1.")
            src = norm(src + ff(src, p + "ff."), p + "norm2.")
    memory = norm(src, "transformer.encoder.norm.")
    for i in range(O.n_layers_of(P, "decoder")):
        p = f"transformer.decoder.layers.{i}."
        if pre_norm:
            h = norm(t, p + "norm1.")
            t = t + attention(h, h, p + "self_attn.", causal, i)
            t = t + attention(norm(t, p + "norm2."), memory, p + "cross_attn.", False, i)
            t = t + ff(norm(t, p + "norm3."), p + "ff.")
        else:
            t = norm(t + attention(t, t, p + "self_attn.", causal, i), p + "norm1.")
            t = norm(t + attention(t, memory, p + "cross_attn.", False, i), p + "norm2.")
            t = norm(t + ff(t, p + "ff."), p + "norm3.")
    t = norm(t, "transformer.decoder.norm.")
    assert not own and not mix
    return O.linear(t.permute(1, 0, 2), P["Wout.weight"], P["Wout.bias"])


def lambda_scales(P, tails):
    """{lambda vector key: A max|dlambda / dvector|} after the backward: A = sum |du o2| of that attention, in P's dtype."""
    out = {}
    for p, u, o2 in tails:
        A = float((u.grad * o2.detach()).abs().sum())
        e1 = float(torch.exp(torch.sum(P[p + "lambda_q1"] * P[p + "lambda_k1"])).detach())
        e2 = float(torch.exp(torch.sum(P[p + "lambda_q2"] * P[p + "lambda_k2"])).detach())
        m = lambda k: float(P[p + k].detach().abs().max())
        out[p + "lambda_q1"], out[p + "lambda_k1"] = A * e1 * m("lambda_k1"), A * e1 * m("lambda_q1")
        out[p + "lambda_q2"], out[p + "lambda_k2"] = A * e2 * m("lambda_k2"), A * e2 * m("lambda_q2")
    return out


def run_case(c, sd, f, own, mix, dtype, wrong=(), table64=False):
    """(losses (3,), logits, {key: gradient or None}, the mixture layers' records, {lambda key: scale}) of the restatement."""
    P = {k: cast(v, dtype, True) for k, v in sd.items()}
    recs, tails = [], []
    logits = forward_restated(P, c, f, own, mix, wrong, recs, True, tails, table64)
    total, chord, emotion = T.loss(logits, f)
    total.backward()
    return (np.array([float(total.detach()), float(chord.detach()), float(emotion.detach())]), logits.detach().numpy(),
            {k: None if q.grad is None else q.grad.numpy() for k, q in P.items()}, recs, lambda_scales(P, tails))


def run(name, dtype, wrong=()):
    return run_case(BY_NAME[name], state_dict(name), inputs(name), *masks(name), dtype, wrong)


def is_lambda(k):
    return k.rsplit(".", 1)[-1] in LAMBDA_NAMES


def grad_errors(got, g64, scales):
    """({key: error} of every gradient but the lambda vectors' at `grad_scale` -- one that is identically zero in fp64 must be zero
    bit for bit --, {key: error} of the lambda vectors at their own scale)."""
    plain, lam = {}, {}
    for k, g in g64.items():
        if g is None:
            continue
        if k.endswith(("q_proj.weight", "k_proj.weight")) and not np.abs(g).max() > 0:
            # one key: both maps are [1] and the scores have no gradient in exact arithmetic; fp32 leaves the rounding of dP - sum dO O,
            # whose terms are the products the same attention's v_proj gradient is made of: that gradient is the scale (the rule of
            # `grad_scale` for Er with one key)
            plain[k] = rel_err(got[k], g, float(np.abs(g64[k.rsplit(".", 2)[0] + ".v_proj.weight"]).max()))
        elif is_lambda(k):
            lam[k] = rel_err(got[k], g, scales[k]) if scales[k] > 0 else (0.0 if not np.asarray(got[k]).any() else float("inf"))
        elif np.abs(g).max() > 0:
            plain[k] = rel_err(got[k], g, grad_scale(g64, k))
        else:
            plain[k] = 0.0 if not np.asarray(got[k]).any() else float("inf")
    return plain, lam


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's fp64 and fp32 restatement (fp32 on one CPU thread) and its noise levels; shared by the tests of a process, read-only."""
    r64 = run(name, torch.float64)
    r32 = one_thread(run, name, torch.float32)
    yl = torch.from_numpy(r64[1]).requires_grad_(True)
    T.loss(yl, inputs(name))[0].backward()
    plain, lam = grad_errors(r32[2], r64[2], r64[4])
    return dict(l64=r64[0], y64=r64[1], g64=r64[2], recs=r64[3], scales=r64[4], l32=r32[0], y32=r32[1], g32=r32[2],
                e32=max(plain.values()), e32_lambda=max(lam.values()) if lam else 0.0, e32_y=logit_err(r32[1], r64[1]),
                dl_dy_sum=float(yl.grad.abs().sum()))


def bound(ref):
    return FACTOR * ref["e32"]


def lambda_bound(ref):
    return max(FACTOR * ref["e32_lambda"], FACTOR * U)


def loss_bound(ref):
    D = LOGIT_FACTOR * ref["e32_y"] * max(1.0, float(np.abs(ref["y64"]).max()))
    return D * ref["dl_dy_sum"] + 159 * U * abs(ref["l64"][0])


def biased_gap(recs):
    """Smallest relative gap between the 2nd and 3rd selection value over the rows of every mixture layer."""
    return FP.route_gap([r["sel"] for r in recs])


def flipped_fraction(rec):
    """Share of the rows whose expert pair differs from the one the raw logits give."""
    a = rec["idx"].sort(-1).values
    b = rec["logits"].topk(TOP_K, dim=-1).indices.sort(-1).values
    return float((a != b).any(-1).double().mean())


def variant_miss(name, variant):
    """Worst error / bound of a wrong variant in fp64 against the case's fp64 reference (gradients at their measures, logits, the
    routing; a gradient that is None on one side only, or another routing, counts as an infinite miss)."""
    ref = reference(name)
    _, y, g, recs, _ = run(name, torch.float64, (variant,))
    if {k for k, v in g.items() if v is None} != {k for k, v in ref["g64"].items() if v is None}:
        return float("inf")
    if any(not torch.equal(a["idx"].sort(-1).values, b["idx"].sort(-1).values) for a, b in zip(recs, ref["recs"])):
        return float("inf")
    plain, lam = grad_errors(g, ref["g64"], ref["scales"])
    return max(max(plain.values()) / bound(ref), max(lam.values()) / lambda_bound(ref) if lam else 0.0,
               logit_err(y, ref["y64"]) / (LOGIT_FACTOR * ref["e32_y"]))


# ---- the operators alone ---------------------------------------------------------------------------------------------------------------
def subln_inputs(rows, hd, zero_row=None, seed=0):
    rng = np.random.default_rng(seed + 13 * rows + hd)
    a = {"o1": rng.standard_normal((rows, hd)), "o2": rng.standard_normal((rows, hd)), "w": 1.0 + 0.3 * rng.standard_normal(hd),
         "dy": rng.standard_normal((rows, hd)), "lam": np.array([0.35 + 0.1 * rng.standard_normal()])}
    if zero_row is not None:
        a["o1"][zero_row] = 0.0
        a["o2"][zero_row] = 0.0
    return {k: v.astype(np.float32) for k, v in a.items()}


SUBLN_SCALE, SUBLN_EPS = 0.644, 1e-5


def subln_restated(a, dtype):
    """{y, o1, o2, w, lam gradients, A} of the tail alone."""
    t = {k: cast(v, dtype, k != "dy") for k, v in a.items()}
    tails = []
    y = diff_tail(t["o1"], t["o2"], t["lam"], t["w"], SUBLN_SCALE, SUBLN_EPS, collect=tails, tag="")
    y.backward(t["dy"])
    out = {k: t[k].grad.numpy() for k in ("o1", "o2", "w", "lam")}
    out["y"], out["A"] = y.detach().numpy(), float((tails[0][1].grad * t["o2"].detach()).abs().sum())
    return out


def diff_attention_inputs(B, H, Lq, Lk, hd, seed=0):
    rng = np.random.default_rng(seed + B + 7 * H + 11 * Lq + 13 * Lk + hd)
    n = lambda *s: rng.standard_normal(s).astype(np.float32)
    return {"q": n(B * Lq * 2 * H * hd), "k": n(B * Lk * 2 * H * hd), "v": n(B * Lk * H * hd), "w": (1.0 + 0.3 * n(hd)).astype(np.float32),
            "lam": np.array([0.3], dtype=np.float32), "dy": n(B, H, Lq, hd)}


def diff_attention_restated(a, B, H, Lq, Lk, hd, causal, dtype):
    """{y, gradients of q, k, v, lam, w, A} of `DiffAttentionFn`'s arithmetic (`O.diff_attention` between the rotation and the out
    projection)."""
    t = {k: cast(v, dtype, k != "dy") for k, v in a.items()}
    tails = []
    o1, o2 = diff_maps(t["q"], t["k"], (t["v"], t["v"]), B, H, Lq, Lk, hd, causal)
    y = diff_tail(o1, o2, t["lam"], t["w"], SUBLN_SCALE, SUBLN_EPS, collect=tails, tag="")
    y.backward(t["dy"])
    out = {k: t[k].grad.numpy() for k in ("q", "k", "v", "lam", "w")}
    out["y"], out["A"] = y.detach().numpy(), float((tails[0][1].grad * tails[0][2].detach()).abs().sum())
    return out


# ---- against the reference's own run (tools/make_goldens_train_v3.py, tests/test_train_v3_gpu.py) -------------------------------------
# the two models g_train_v3.npz records, on the miniature dataset of tests/helpers_eval.py (both clips in one batch, 299 chord positions,
# 300 frames), 4 layers, 2 heads, d_model 64, dim_feedforward 128, dropout 0, synthetic weights of seed 0 (the bias buffers included)
GOLDEN = {"v31": Case("v31", "3.1", 4, 64, 2, 128, T.L_CHORD, T.S_VIDEO, T.B_CLIPS, 0, True, 0.0, 0.0, "differential attention in both stacks"),
          "v30": Case("v30", "3.0", 4, 64, 2, 128, T.L_CHORD, T.S_VIDEO, T.B_CLIPS, 0, True, 0.0, 0.0, "the V2 attention in the encoder")}
_DEC1, _ENC1 = "transformer.decoder.layers.1.", "transformer.encoder.layers.1."
_MIX = "transformer.decoder.layers.3.ff."
GOLDEN_KEYS = {
    "v31": tuple(_DEC1 + "self_attn." + n for n in LAMBDA_NAMES + ("subln.weight", "q_proj.weight", "k_proj.weight", "v_proj.weight", "out_proj.weight"))
    + tuple(_DEC1 + "cross_attn." + n for n in LAMBDA_NAMES + ("subln.weight", "q_proj.weight", "k_proj.weight", "v_proj.weight", "out_proj.weight"))
    + tuple(_ENC1 + "self_attn." + n for n in LAMBDA_NAMES + ("subln.weight", "q_proj.weight", "k_proj.weight", "v_proj.weight", "out_proj.weight"))
    + (_MIX + "gate.weight", _MIX + "gate.bias", _MIX + "experts.2.linear1.weight", _MIX + "experts.2.gate.bias", _MIX + "experts.2.linear2.weight",
       "transformer.encoder.layers.3.ff.gate.weight", "transformer.decoder.norm.weight", "Wout.weight", "Linear_vis.weight"),
    "v30": tuple(_DEC1 + "self_attn." + n for n in LAMBDA_NAMES + ("subln.weight", "q_proj.weight", "out_proj.weight"))
    + tuple(_DEC1 + "cross_attn." + n for n in LAMBDA_NAMES + ("k_proj.weight", "v_proj.weight"))
    + (_ENC1 + "self_attn.in_proj_weight", _ENC1 + "self_attn.out_proj.bias", _MIX + "gate.weight", _MIX + "gate.bias",
       _MIX + "experts.2.linear1.weight", "transformer.encoder.layers.3.ff.gate.bias", "Linear_chord.weight"),
}


def golden_kwargs(tag):
    return dict(model_kwargs(GOLDEN[tag]), total_vf_dim=FT.GOLDEN_VF)


@functools.lru_cache(maxsize=None)
def golden_state_dict(tag):
    c = GOLDEN[tag]
    return synthetic.synthetic_state_dict(FP.named_shapes(c.version, c.n_layers, c.H, c.d, c.dff, FT.GOLDEN_VF), seed=0)


@functools.lru_cache(maxsize=None)
def golden_fp64(tag):
    """(losses, logits, gradients, the mixtures' records, lambda scales) of the restatement in fp64 with the rotary table built in
    double (`O.forward_family`'s arithmetic) on the recorded models."""
    return run_case(GOLDEN[tag], golden_state_dict(tag), FT.golden_inputs(), None, None, torch.float64, table64=True)
