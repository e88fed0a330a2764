"""Numeric-range recipes: inputs away from N(0,1) for the softmax-shaped, scan, gate and row-statistics kernels, their references
and the bound (tests/test_numeric_range_host.py on the CPU, tests/test_numeric_range_gpu.py on the GPU).

Every other parity test draws at unit scale, where the running-max rescale of the online softmax, `m + log l`, `__expf` at large
arguments, softplus's threshold branch, `1 / (1 + exp(-v))` past overflow and the two-pass row statistics give the answer a wrong
version gives too.  A recipe names the regime it reaches; the host test proves it reaches it, that the fp32 reference alone stays
under the cap, and that a deliberately wrong fp32 variant misses the bound on it.

References are the restatements the suite already has (`helpers_ops_edges._attn_restate`, `attn_train_torch_cpu` -- the formula of
tests/test_attn_train_gpu.py, which imports it from here --, `helpers_reg_mamba_train.scan_gate`, `rnn_torch_cpu` -- torch's nn.LSTM /
nn.GRU as tests/test_rnn_train_gpu.py drives them --, torch's layer_norm), run in fp64 and in fp32 on the CPU.

Bound, the project's rule (tests/test_mamba_bwd_gpu.py): rel_err(got, ref64) <= max(8 e32, n U), e32 the fp32 CPU run of the same
restatement on the same inputs, n the longest sum behind a value, U = 2^-24; rel_err is relative to the tensor's max norm, and a
tensor that is identically zero in fp64 is held to zero absolutely.  No bound may exceed CAP = 1e-3 (a condition on the recipe, not a
measurement), and everything is finite on both sides."""
import functools

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import helpers_ops_edges as HO
from tests import helpers_reg_mamba_train as TM
from tests.helpers_reg_train import U

CAP = 1e-3
FLT_MIN = np.float32(1.17549435e-38)      # below it the device's __expf returns 0 (denormals are flushed)


def rel_err(got, want):
    """`helpers_reg_train.rel_err`, max |got - want| / max |want|, made total: where `want` is identically zero the absolute maximum
    of `got` (the zero-gradient convention of tests/test_mamba_bwd_gpu.py), and inf for non-finite values (a miss, not a NaN that
    compares false)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if not (np.isfinite(got).all() and np.isfinite(want).all()):
        return float("inf")
    top = np.abs(want).max()
    return float(np.abs(got).max()) if not top else float(np.abs(got - want).max() / top)


def bound(e32, n):
    return max(8.0 * e32, n * U)


def judge(got, w64, w32, n_of, tag="", vanish=0.0, only=None):
    """-> (report line, names that miss, worst err / bound).  got / w64 / w32: {name: array}; n_of: name -> longest sum.  `got` must
    hold every output of the reference, or exactly those named in `only`.  vanish: a tensor whose fp64 values all lie within it is
    held to 8 n U absolute (tests/test_attn_train_gpu.py: dS = P (dP - D) with P = 1 cancels to zero, and dP and D are the same sum
    in two orders)."""
    names = list(w64) if only is None else list(only)
    assert set(got) == set(names) and set(names) <= set(w64), (tag, sorted(set(got) ^ set(names)))
    report, bad, worst = [], [], 0.0
    for k in names:
        want = w64[k]
        if np.abs(want).max() <= vanish:
            b, e = 8 * n_of(k) * U, float(np.abs(np.asarray(got[k], dtype=np.float64)).max())
        else:
            b, e = bound(rel_err(w32[k], want), n_of(k)), rel_err(got[k], want)
        report.append(f"{k} {e:.2e}/{b:.2e}")
        worst = max(worst, e / b)
        if not (e <= b and np.isfinite(np.asarray(got[k], dtype=np.float64)).all()):
            bad.append(k)
    return f"{tag}: err/bound " + " ".join(report), bad, worst


def caps(w64, w32, n_of, vanish=0.0):
    """{name: bound} from the fp32 reference alone; the host test holds every one of them to CAP."""
    out = {}
    for k, want in w64.items():
        if np.abs(want).max() <= vanish:
            assert np.abs(w32[k]).max() <= 8 * n_of(k) * U, k
            out[k] = 8 * n_of(k) * U
        else:
            out[k] = bound(rel_err(w32[k], want), n_of(k))
    return out


VANISH = 1e-12                  # attention: gradients of rows whose softmax is one-hot
SCAN_VANISH = 1e-100            # the scan's dA_log where exp(delta A) underflows: 1e-170 in fp64, 0 in fp32


# =====================================================================================================================
# A. softmax-shaped kernels
# =====================================================================================================================
ATTN_RECIPES = ("ramp_up", "ramp_down", "offset60", "neg90", "onehot")
KEY_TILE = 32
# ops.attention: (Lq, Lk, hd, kernel)
ATTN_FWD_SHAPES = [(77, 300, 64, "splitk"), (40, 300, 32, "splitk"), (130, 77, 128, "rows128"), (33, 31, 16, "rows128")]
# ops.attention_train + ops.attention_bwd: (H, Lq, Lk, hd, kv_group, causal, rpr, mask)
ATTN_TRAIN_CASES = [(2, 77, 130, 32, 1, 0, 0, 0), (2, 77, 130, 32, 1, 1, 0, 0), (2, 130, 300, 64, 2, 0, 0, 0), (2, 130, 300, 64, 2, 1, 0, 0),
                    (2, 77, 130, 64, 2, 1, 0, 0), (2, 130, 300, 32, 1, 1, 0, 1),
                    (2, 130, 130, 64, 1, 1, 1, 0), (2, 77, 77, 32, 1, 1, 1, 0)]       # relative positions need causal self-attention, kv_group 1
P_DROP = 0.2


# `onehot` in the training cases.  amt_attn_bwd is the flash-style backward: dS = P (dP - D) with D = rowsum(dO o O) read from the
# rounded output, where torch's softmax backward forms sum_j P dP itself.  On a one-hot row dP_j - D is then rounding noise of about
# sqrt(hd) U instead of 0, and dq = dS k multiplies it by |k_j| = the key's score: at 100 the fp32 restatement of that formulation
# (`attn_bwd_flash_f32`) misses max(8 e32, n U) for dq by 1.9 to 7.2 times, and so does the kernel, by 1.6 to 3.2 times.  The ladder is
# walked down to the largest magnitude at which the restatement holds the bound at every training shape (the host test shows both
# sides); the forward kernels, amt_rpr_attn_fwd among them (`rpr_prefill_refs`), keep 100.  At 17.5 the other keys of a row still sum
# to under 1e-5.
# Without the causal mask every row is one-hot and dq, dk vanish: there the magnitude stays 100 and the tensors are held to 8 n U
# absolute (at 17.5 they would be 1e-6 of cancellation residue, which fp32 itself gets 5 % wrong).
ONEHOT_LADDER = (100.0, 50.0, 35.0, 25.0, 17.5)
ONEHOT_TRAIN = 17.5


def onehot_train(causal):
    return ONEHOT_TRAIN if causal else 100.0


def key_scores(recipe, Lq, Lk, rs, onehot=100.0):
    """t_j, the score every query gives key j."""
    j = np.arange(Lk)
    if recipe == "ramp_up":
        return 8.0 * (j // KEY_TILE) + 0.3 * rs.standard_normal(Lk)
    if recipe == "ramp_down":
        return -8.0 * (j // KEY_TILE) + 0.3 * rs.standard_normal(Lk)
    if recipe == "offset60":
        return 60.0 + rs.standard_normal(Lk)
    if recipe == "neg90":           # the draw is cut at +-2, so that every exp(s) is below the smallest normal fp32 number
        return -90.0 + np.clip(rs.standard_normal(Lk), -2.0, 2.0)
    if recipe == "onehot":          # at two thirds of the shorter side: a causal row sees it from there on, after a tile without it
        t = np.zeros(Lk)
        t[2 * min(Lq, Lk) // 3] = onehot
        return t
    raise ValueError(recipe)


@functools.lru_cache(maxsize=None)
def attn_recipe(recipe, B, H, Lq, Lk, hd, g=1, rpr=0, mask=0, onehot=100.0):
    """Controlled scores: q_i = a u + 0.05 noise, k_j = t_j u + 0.3 noise with u a fixed unit vector, a = sqrt(hd) and the noise
    orthogonal to u, so that with q_scale = hd^-0.5 the score of key j is t_j + 0.015 hd^-0.5 (noise . noise).  v, dO ~ N(0,1); Er
    stays N(0,1) (qs . Er is then N(0,1): the skewed term does not undo the recipe).  -> ({q, k, v, dO (, Er)} as (B, L, heads hd)
    fp32, keep or None)."""
    rs = np.random.RandomState((ATTN_RECIPES.index(recipe) * 1009 + Lq * 7 + Lk * 13 + hd * 3 + g + 2 * rpr + 5 * mask) % 2 ** 31)
    u = rs.standard_normal(hd)
    u /= np.linalg.norm(u)

    def noise(*shape):
        n = rs.standard_normal(shape + (hd,))
        return n - (n @ u)[..., None] * u

    t = np.stack([np.stack([key_scores(recipe, Lq, Lk, rs, onehot) for _ in range(H // g)]) for _ in range(B)])         # (B, Hk, Lk)
    q = np.sqrt(hd) * u + 0.05 * noise(B, Lq, H)
    k = t.transpose(0, 2, 1)[..., None] * u + 0.3 * noise(B, Lk, H // g)
    a = {"q": q.reshape(B, Lq, H * hd), "k": k.reshape(B, Lk, H // g * hd), "v": rs.standard_normal((B, Lk, H // g * hd)),
         "dO": rs.standard_normal((B, Lq, H * hd))}
    if rpr:
        a["Er"] = rs.standard_normal((Lq, hd))
    a = {n: v.astype(np.float32) for n, v in a.items()}
    keep = None
    if mask:
        keep = (rs.random_sample((B, H, Lq, Lk)) >= P_DROP).astype(np.uint8)
    return a, keep


def attn_scores64(a, H, g, hd):
    """(B, H, Lq, Lk) scores in fp64, no mask."""
    B, Lq, _ = a["q"].shape
    Lk = a["k"].shape[1]
    q = a["q"].astype(np.float64).reshape(B, Lq, H, hd).transpose(0, 2, 1, 3) * np.float64(np.float32(hd ** -0.5))
    k = np.repeat(a["k"].astype(np.float64).reshape(B, Lk, H // g, hd).transpose(0, 2, 1, 3), g, axis=1)
    return q @ k.transpose(0, 1, 3, 2)


def attn_fwd_case(recipe, Lq, Lk, hd, kernel, causal):
    """The recipe as a case of helpers_ops_edges (clip-major layout, q_scale = hd^-0.5), for `_attn_restate` and amt_attn_fwd."""
    B, H = 1, 2
    c = HO.AttnCase(f"{recipe}_{Lq}x{Lk}_hd{hd}{'c' if causal else ''}", B, H, Lq, Lk, hd, causal, 1, "clip", 1, kernel, False, recipe)
    a, _ = attn_recipe(recipe, B, H, Lq, Lk, hd)
    lay = HO.attn_layout(c)
    inp = dict(bufs={n: a[n].reshape(-1) for n in ("q", "k", "v")}, lay=lay, q_scale=float(hd) ** -0.5,
               strides=[lay[t][i] for t in ("q", "k", "v", "o") for i in (1, 2, 3)])
    return c, inp


@functools.lru_cache(maxsize=None)
def attn_fwd_refs(recipe, Lq, Lk, hd, kernel, causal):
    c, inp = attn_fwd_case(recipe, Lq, Lk, hd, kernel, causal)
    return {"o": HO._attn_restate(c, inp, torch.float64)}, {"o": HO._attn_restate(c, inp, torch.float32)}


def attn_train_torch_cpu(a, keep, H, causal, g, dtype, p_drop=P_DROP):
    """The written-out training attention of tests/test_attn_train_gpu.py on the CPU in `dtype`, differentiated by torch:
    S_ij = qs_i . k_j (+ qs_i . Er[er_len-1-(i-j)] for j <= i), P = softmax_j(S) under the mask, O = (P o keep / (1 - p)) V."""
    t = {k: torch.from_numpy(v).to(dtype).requires_grad_(k != "dO") for k, v in a.items()}
    B, Lq, E = t["q"].shape
    Lk, hd = t["k"].shape[1], E // H
    qh = (t["q"] * hd ** -0.5).view(B, Lq, H, hd).transpose(1, 2)
    kh = t["k"].view(B, Lk, H // g, hd).transpose(1, 2).repeat_interleave(g, dim=1)
    vh = t["v"].view(B, Lk, H // g, hd).transpose(1, 2).repeat_interleave(g, dim=1)
    S = qh @ kh.transpose(2, 3)
    i, j = torch.arange(Lq)[:, None], torch.arange(Lk)[None, :]
    if "Er" in t:
        er_len = t["Er"].shape[0]
        rel = qh @ t["Er"].t()                                                   # (B, H, L, er_len)
        idx = (er_len - 1 - (i - j)).clamp(0, er_len - 1)
        S = S + torch.where(j <= i, torch.gather(rel, 3, idx.expand(B, H, Lq, Lk)), torch.zeros((), dtype=dtype))
    if causal:
        S = S.masked_fill(j > i, float("-inf"))
    lse = torch.logsumexp(S, dim=-1)
    Pd = torch.softmax(S, dim=-1)
    if keep is not None:
        Pd = Pd * torch.from_numpy(keep).to(dtype) / (1.0 - p_drop)
    O = (Pd @ vh).transpose(1, 2).reshape(B, Lq, E)
    O.backward(t["dO"])
    out = {"O": O.detach().numpy(), "lse": lse.detach().numpy()}
    out.update({k: t[k].grad.numpy() for k in t if k != "dO"})
    return out


def attn_train_n(H, Lq, Lk, hd, g, B=1):
    n = {"O": Lk + hd, "lse": Lk + hd, "q": Lk + hd, "k": g * Lq, "v": g * Lq, "Er": B * H * Lq}
    return n.__getitem__


@functools.lru_cache(maxsize=None)
def attn_train_refs(recipe, H, Lq, Lk, hd, g, causal, rpr, mask):
    a, keep = attn_recipe(recipe, 1, H, Lq, Lk, hd, g, rpr, mask, onehot_train(causal))
    return attn_train_torch_cpu(a, keep, H, causal, g, torch.float64), attn_train_torch_cpu(a, keep, H, causal, g, torch.float32)


RPR_PREFILL = (2, 130, 64)              # H, L, head_dim of the amt_rpr_attn_fwd case


@functools.lru_cache(maxsize=None)
def rpr_prefill_refs(recipe):
    """The forward alone of causal self-attention with relative positions, `onehot` at the full 100: O of `attn_train_torch_cpu`
    (its gradients, which 100 makes ill-conditioned, are not read)."""
    H, L, hd = RPR_PREFILL
    a, _ = attn_recipe(recipe, 1, H, L, L, hd, 1, 1, 0)
    return tuple({"O": attn_train_torch_cpu(a, None, H, 1, 1, dt)["O"]} for dt in (torch.float64, torch.float32))


def attn_bwd_flash_f32(a, H, causal):
    """dq of the flash-style backward as csrc/attn_bwd.hip's header states it, in fp32 numpy with every sum taken term by term in index
    order (no BLAS: the same figures on every machine): P = exp(S - lse), D = rowsum(dO o O), dS = P o (dP - D), dq = q_scale dS k.
    kv_group 1, no relative positions, no keep mask."""
    f = np.float32
    B, Lq, E = a["q"].shape
    Lk, hd = a["k"].shape[1], E // H
    heads = lambda t, L: t.reshape(B, L, H, hd).transpose(0, 2, 1, 3)
    q, k, v, dO = heads(a["q"], Lq) * f(hd ** -0.5), heads(a["k"], Lk), heads(a["v"], Lk), heads(a["dO"], Lq)

    def mm(x, y):                   # x (.., m, n) y (.., n, p): one fp32 accumulator per output, n ascending
        acc = np.zeros(x.shape[:-1] + (y.shape[-1],), dtype=f)
        for i in range(x.shape[-1]):
            acc += x[..., :, i, None] * y[..., i, None, :]
        return acc

    kT, vT = k.transpose(0, 1, 3, 2), v.transpose(0, 1, 3, 2)
    s = mm(q, kT)
    if causal:
        s = np.where(np.arange(Lk)[None, :] > np.arange(Lq)[:, None], f(-np.inf), s)
    m = s.max(-1, keepdims=True)
    lse = m + np.log(np.exp(s - m).sum(-1, keepdims=True, dtype=f))
    p = np.exp(s - lse)
    D = (dO * mm(p, v)).sum(-1, keepdims=True, dtype=f)
    dq = mm(p * (mm(dO, vT) - D), k) * f(hd ** -0.5)
    return dq.transpose(0, 2, 1, 3).reshape(B, Lq, E)


def softmax_rows_f32(s, v, variant="ok", tile=KEY_TILE):
    """The online softmax of the attention kernels in fp32 numpy on one head: s (Lq, Lk) scores, v (Lk, hd).  -> (o, lse, p) with
    p = exp(s - lse), what the backward re-exponentiates.  exp flushes results below the smallest normal number, as __expf does.
    variant: "ok" | "no_max" (exp(s) without the maximum) | "l_not_rescaled" (alpha = exp(m_old - m_new) applied to o, not to l) |
    "lse_log_l" (lse = log l without m)."""
    f = np.float32
    s, v = s.astype(f), v.astype(f)

    def ex(x):
        with np.errstate(over="ignore", under="ignore"):
            e = np.exp(x, dtype=f)
        return np.where(e < FLT_MIN, f(0), e)

    Lq, Lk = s.shape
    m = np.full(Lq, -np.inf, dtype=f)
    l = np.zeros(Lq, dtype=f)
    o = np.zeros((Lq, v.shape[1]), dtype=f)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j0 in range(0, Lk, tile):
            st = s[:, j0:j0 + tile]
            m_new = np.maximum(m, st.max(1)) if variant != "no_max" else np.zeros(Lq, dtype=f)
            alpha = ex(m - m_new) if variant != "no_max" else np.ones(Lq, dtype=f)
            p = ex(st - m_new[:, None])
            l = (l if variant == "l_not_rescaled" else l * alpha) + p.sum(1, dtype=f)
            o = o * alpha[:, None] + p @ v[j0:j0 + tile]
            m = m_new
        lse = (np.log(l) if variant == "lse_log_l" else m + np.log(l)).astype(f)
        return (o / l[:, None]).astype(f), lse, ex(s - lse[:, None])


def softmax_rows_f64(s, v):
    s, v = s.astype(np.float64), v.astype(np.float64)
    m = s.max(1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(1, keepdims=True)
    return (e / l) @ v, (m + np.log(l))[:, 0], e / l


# ---- row-softmax reductions: the chord loss and the chord metrics ----
LOGIT_TREATMENTS = ("offset1000", "spread30", "target_minus80", "emotion100")


@functools.lru_cache(maxsize=None)
def chord_logits(treatment, B=2, L=5):
    """The case of tests/test_chord_loss_gpu.py (3 N(0,1) logits, every kind of target) with the logits treated.  -> y (B, L, 159),
    tgt, emo, prob."""
    from tests.test_chord_loss_gpu import NC, make_case
    y, tgt, emo = make_case(B, L, NC)
    y = y.copy()
    rs = np.random.RandomState(LOGIT_TREATMENTS.index(treatment))
    safe = np.where((tgt >= 0) & (tgt < NC), tgt, 0)
    if treatment == "offset1000":
        y += np.float32(1000.0)
    elif treatment == "spread30":
        y = (30.0 * rs.standard_normal(y.shape)).astype(np.float32)
    elif treatment == "target_minus80":
        np.put_along_axis(y, safe[..., None], (y.max(-1) - np.float32(80.0))[..., None], -1)
    elif treatment == "emotion100":
        y = np.where(rs.random_sample(y.shape) < 0.5, np.float32(100.0), np.float32(-100.0)) + y
    prob = np.where(rs.random_sample((B, L)) < 0.5, 0.9, 0.5).astype(np.float32)
    return y.astype(np.float32), tgt, emo, prob


def chord_split(res):
    """The outputs of tests/test_chord_loss_gpu.torch_cpu as tensors of one scale each."""
    return {"loss_total": res["loss"][0:1], "loss_chord": res["loss"][1:2], "loss_emotion": res["loss"][2:3], "clip_ce": res["clip"][:, 1],
            "clip_bce": res["clip"][:, 2], "dlogits": res["dlogits"]}


def chord_n(B, L):
    return lambda k: B * L * 159 if k.startswith("loss") else 159 + L if k.startswith("clip") else 159


@functools.lru_cache(maxsize=None)
def chord_refs(treatment, smoothing):
    from tests.test_chord_loss_gpu import torch_cpu
    y, tgt, emo, _ = chord_logits(treatment)
    return tuple(chord_split(torch_cpu(y, tgt, emo, smoothing, dt)) for dt in (torch.float64, torch.float32))


# ---- the auxiliary chord loss (csrc/chord_aux_loss.hip): a second softmax per row, five selected maxima, two hinges, `count` ----
AUX_W = (0.4, 0.6)              # the weighting of tests/test_chord_aux_loss_gpu.py
# the treatments above at helpers_chord_aux.REGIME_SHAPE and three recipes of the auxiliary terms' own.  ties_inside: in every auxiliary
# row the two largest logits are equal and so are the 4th and 5th (the top-3 and top-5 means do not depend on the order among equals;
# the 3rd / 4th and 5th / 6th gaps are `make_case`'s or wider).  count_flip_guard2 / 1: `regime_case(2)` / `(1)` with + 1000 on every
# logit -- an inactive hinge must stay exactly inactive, or `count` and with it every chord gradient changes by a factor
AUX_RECIPES = LOGIT_TREATMENTS + ("ties_inside", "count_flip_guard2", "count_flip_guard1")
AUX_LOSSES = ("total", "chord", "emotion", "ce", "aux3", "aux5")
AUX_CLIP = ("n_valid", "ce", "bce", "L", "a3", "a5")


@functools.lru_cache(maxsize=None)
def chord_aux_case(recipe, layout):
    """-> y (B, L, 159) fp32, tgt, emo at REGIME_SHAPE.  The recipes of the auxiliary terms' own are built on the auxiliary rows and,
    for "view", carried to y by `unview`; a treatment's y is the same for both layouts."""
    from tests import helpers_chord_aux as HA
    B, L = HA.REGIME_SHAPE
    if recipe in LOGIT_TREATMENTS:
        return chord_logits(recipe, B, L)[:3]
    if recipe == "ties_inside":
        y, tgt, emo = HA.make_case(B, L)
        z = np.ascontiguousarray(HA.aux_rows(y, layout)).copy()
        order = np.argsort(-z, axis=-1, kind="stable")
        for dst, src in ((1, 0), (4, 3)):                   # the 2nd takes the 1st's value, the 5th the 4th's
            np.put_along_axis(z, order[..., dst:dst + 1], np.take_along_axis(z, order[..., src:src + 1], -1), -1)
        return np.ascontiguousarray(z if layout == "rows" else HA.unview(z), dtype=np.float32), tgt, emo
    y, tgt, emo = HA.regime_case({"count_flip_guard2": 2, "count_flip_guard1": 1}[recipe], layout)
    return y + np.float32(1000.0), tgt, emo


def chord_aux_split(res):
    """The outputs of `helpers_chord_aux.chord_aux` (and of the kernel) as tensors of one scale each."""
    out = {"loss_" + k: res["loss"][i:i + 1] for i, k in enumerate(AUX_LOSSES)}
    out["count"] = res["loss"][6:7]
    out.update({"clip_" + k: res["clip"][:, i] for i, k in enumerate(AUX_CLIP)})
    out["dlogits"] = res["dlogits"]
    return out


@functools.lru_cache(maxsize=None)
def chord_aux_refs(recipe, layout, smoothing):
    from tests import helpers_chord_aux as HA
    y, tgt, emo = chord_aux_case(recipe, layout)
    return tuple(chord_aux_split(HA.chord_aux(y, tgt, emo, smoothing, AUX_W, layout, dt)) for dt in (torch.float64, torch.float32))


def chord_aux_n(B, L):
    """The sums of tests/test_chord_aux_loss_gpu.py's bounds: a 159-term tree inside a row and a sum over the clip's L rows for a
    per-clip sum (`helpers_eval.loss_bound`); for a loss those carried through the B clips, and 4 for the quotients and the
    combination; 159 for dlogits."""
    return lambda k: 159 + L + B + 4 if k.startswith("loss") else 159 + L if k.startswith("clip") else 159


def chord_aux_floors(y):
    """(gap, margin) a case must keep from the two places where the gradient jumps, from the fp32 spacing s at the logits' magnitude
    (6e-5 at 1000).  The logits are fp32 numbers, so two of them that differ differ by s or more: a top-k border is decided by
    a comparison of inputs and any gap of 2 s is unambiguous.  z - m is rounded to s / 2, so a probability carries up to s of relative
    error on top of the 159-term sum's; a hinge 4 (s + 159 U) from its kink cannot change sides.  Never under helpers_chord_aux's own."""
    from tests import helpers_chord_aux as HA
    s = float(np.spacing(np.float32(np.abs(y).max())))
    return max(2 * s, HA.MIN_GAP), max(4 * (s + HA.NC * U), HA.MIN_MARGIN)


def aux_hinge_sum_f32(z, t, k, variant="ok"):
    """sum over the rows of relu(mean(top-k of softmax(z)) - softmax(z)_t) in fp32 numpy as the kernel's header states it: the k
    largest are chosen on the logits, p = exp(z - m) / se with results below the smallest normal number flushed.  z (rows, 159), t (rows).
    variant: "no_max" (the softmax without its maximum) | "topk_of_p" (the k largest chosen on the rounded p, lowest index first)."""
    f = np.float32
    z = z.astype(f)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        e = np.exp(z if variant == "no_max" else z - z.max(-1, keepdims=True), dtype=f)
        e = np.where(e < FLT_MIN, f(0), e)
        p = e / e.sum(-1, keepdims=True, dtype=f)
        order = np.argsort(-(p if variant == "topk_of_p" else z), axis=-1, kind="stable")[:, :k]
        top = np.take_along_axis(p, order, -1).sum(-1, dtype=f) / f(k)
        return np.maximum(top - np.take_along_axis(p, t[:, None], -1)[:, 0], f(0)).sum(dtype=f)


# =====================================================================================================================
# B. selective scan
# =====================================================================================================================
SCAN_RECIPES = ("slow_decay", "fast_decay", "threshold", "tiny_delta", "gate_saturated")
SCAN_SHAPES = [(2, 33, 24), (1, 70, 40)]
SOFTPLUS_GRID = (19.0, 19.999, 20.0, 20.001, 21.0, 40.0, 88.0)
SCAN_CHUNK = 32
# amt_selective_scan_wide_train_fwd / _bwd (csrc/mamba.hip, csrc/mamba_bwd.hip): the narrowest and the widest state, every recipe, both
# shapes; the backward recomputes from checkpoints every 32 steps and adds the partial state sums of N / 16 slices in a second launch
SCAN_WIDE_N = (32, 256)
SCAN_SLICE = 16


@functools.lru_cache(maxsize=None)
def scan_recipe(recipe, B, L, ED, N=16):
    """The inputs of tests/test_mamba_bwd_gpu.scan_case moved into the recipe's regime.  A read-only dict of torch tensors and R."""
    g = torch.Generator().manual_seed(SCAN_RECIPES.index(recipe) * 7919 + B * 1000 + L + N)
    R = -(-(ED // 2) // 16)
    ld = (R + 2 * N + 3) // 4 * 4
    M = B * L
    r = lambda *s: torch.randn(*s, generator=g)
    c = {"xc": r(M, ED), "draw": 0.5 * r(M, ED), "dt_bias": r(ED) - 1.0,
         "A_log": torch.log(torch.arange(1, N + 1, dtype=torch.float32)).repeat(ED, 1) + 0.1 * r(ED, N),
         "dbc": 0.5 * r(M, ld), "D": 1.0 + 0.1 * r(ED), "xz": r(M, 2 * ED), "dout": r(M, ED), "R": R}
    if recipe == "slow_decay":      # delta = 1e-3, A = -1: a = 0.999 per step; D small, so that the state is the output
        c["draw"], c["dt_bias"] = 0.05 * r(M, ED), torch.full((ED,), -6.9)
        c["A_log"] = torch.zeros(ED, N)
        c["D"] = 1e-3 * r(ED)
    elif recipe == "fast_decay":    # delta = 1, A = -403: exp(delta A) underflows to exactly 0
        c["draw"], c["dt_bias"] = 0.05 * r(M, ED), 0.55 + 0.05 * r(ED)
        c["A_log"] = torch.full((ED, N), 6.0)
    elif recipe == "threshold":     # draw + dt_bias on the grid, laid over steps and channels; dt_bias = 0 keeps the sum exact
        grid = torch.tensor(SOFTPLUS_GRID, dtype=torch.float32)
        c["draw"] = grid[(torch.arange(M)[:, None] + torch.arange(ED)[None, :]) % len(SOFTPLUS_GRID)].contiguous()
        c["dt_bias"] = torch.zeros(ED)
    elif recipe == "tiny_delta":    # the odd channels: draw + dt_bias = -30 and D = 0 (their output is the state alone)
        c["draw"][:, 1::2] = 0.0
        c["dt_bias"][1::2] = -30.0
        c["D"][1::2] = 0.0
    elif recipe == "gate_saturated":
        sign = torch.where(torch.rand(M, ED, generator=g) < 0.5, -1.0, 1.0)
        c["xz"][:, ED:] = 60.0 * sign + 0.1 * r(M, ED)
    return c


def scan_run(c, B, L, ED, N, version, reverse, dtype, grads=True):
    """`helpers_reg_mamba_train.scan_gate` on the recipe and, with `grads`, torch's autograd of sum(out dout).  float64 arrays."""
    R = c["R"]
    leaf = lambda t: t.to(dtype).clone().requires_grad_(grads)
    x, draw, z = (leaf(t.view(B, L, -1)) for t in (c["xc"], c["draw"], c["xz"][:, ED:]))
    Bm, Cm = leaf(c["dbc"][:, R:R + N].reshape(B, L, N)), leaf(c["dbc"][:, R + N:R + 2 * N].reshape(B, L, N))
    dt_bias, A_log, D = leaf(c["dt_bias"]), leaf(c["A_log"]), leaf(c["D"])
    with torch.set_grad_enabled(grads):
        out = TM.scan_gate(x, draw, dt_bias, A_log, Bm, Cm, D, z, version, reverse)
    res = {"y": out.detach().reshape(B * L, ED).numpy().astype(np.float64)}
    if grads:
        (out * c["dout"].view(B, L, ED).to(dtype)).sum().backward()
        flat = lambda t: t.grad.reshape(B * L, -1).numpy().astype(np.float64)
        res.update({"dx": flat(x), "ddraw": flat(draw), "dz": flat(z), "dB": flat(Bm), "dC": flat(Cm),
                    "d_dt_bias": dt_bias.grad.numpy().astype(np.float64), "dA_log": A_log.grad.numpy().astype(np.float64),
                    "dD": D.grad.numpy().astype(np.float64)})
    return res


PER_CHANNEL = ("y", "dx", "ddraw", "dz", "d_dt_bias", "dA_log", "dD")


def scan_split(recipe, res):
    """`tiny_delta` judges its two channel halves as tensors of their own: relative to the other half's O(1) values a state of 1e-13
    is nothing, and log1p would go unseen.  The channel axis is the last one but for dA_log (ED, N)."""
    if recipe != "tiny_delta":
        return res
    out = {}
    for k, v in res.items():
        if k in PER_CHANNEL:
            out[k + "[even]"], out[k + "[odd]"] = (v[0::2], v[1::2]) if k == "dA_log" else (v[..., 0::2], v[..., 1::2])
        else:
            out[k] = v
    return out


def scan_n(B, L, N):
    """B L for a parameter's gradient, L N for a value at the end of a state chain (tests/test_scan_wide_bwd_gpu.py) -- but never more
    than CAP / U: at (L, N) = (70, 256) L N U is 1.07e-3, and the case is held to the cap instead of being left out."""
    return lambda k: B * L if k.split("[")[0] in ("dA_log", "dD", "d_dt_bias") else min(L * N, int(CAP / U))


@functools.lru_cache(maxsize=None)
def scan_refs(recipe, B, L, ED, N, version, reverse, grads=True):
    c = scan_recipe(recipe, B, L, ED, N)
    return tuple(scan_split(recipe, scan_run(c, B, L, ED, N, version, reverse, dt, grads)) for dt in (torch.float64, torch.float32))


def softplus_f32(v, variant="ok"):
    """mamba.hip's `v > 20 ? v : log1pf(expf(v))` in fp32 numpy.  variant: "no_threshold" | "no_log1p"."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore"):
        e = np.exp(np.minimum(v, np.float32(20.0)) if variant == "ok" else v, dtype=np.float32)
        soft = np.log(np.float32(1.0) + e, dtype=np.float32) if variant == "no_log1p" else np.log1p(e, dtype=np.float32)
    return soft if variant != "ok" else np.where(v > 20, v, soft)


def scan_state_np(c, B, L, ED, N, dtype, carry="ok", softplus="ok", slices_left_out=0):
    """The un-gated scan output y_t = h_t . C_t + D x_t, forward in time, in numpy at `dtype`, walking in chunks of SCAN_CHUNK steps as
    the training kernels do.  carry: "ok" | "zero" (a chunk starts from h = 0) | "neighbour" (from the state of channel n + 1).
    slices_left_out: the state sum of y runs over the first N - 16 slices_left_out states only (the wide kernels sum N / 16 slices of
    16 states each and add the partials afterwards)."""
    R = c["R"]
    f = lambda t: t.numpy().astype(dtype)
    x, v = f(c["xc"]).reshape(B, L, ED), (f(c["draw"]) + f(c["dt_bias"])).reshape(B, L, ED)
    Bm, Cm = f(c["dbc"][:, R:R + N]).reshape(B, L, N), f(c["dbc"][:, R + N:R + 2 * N]).reshape(B, L, N)
    delta = softplus_f32(v, softplus).astype(dtype) if dtype == np.float32 else np.where(v > 20, v, np.log1p(np.exp(np.minimum(v, 20))))
    A = -np.exp(f(c["A_log"]))
    h = np.zeros((B, ED, N), dtype=dtype)
    y = np.zeros((B, L, ED), dtype=dtype)
    for t in range(L):
        if t and t % SCAN_CHUNK == 0 and carry != "ok":
            h = np.zeros_like(h) if carry == "zero" else np.roll(h, -1, axis=2)
        with np.errstate(under="ignore"):
            h = np.exp(delta[:, t, :, None] * A) * h + (delta[:, t, :, None] * Bm[:, t, None, :]) * x[:, t, :, None]
        y[:, t] = (h * Cm[:, t, None, :])[..., :N - SCAN_SLICE * slices_left_out].sum(-1) + f(c["D"]) * x[:, t]
    return y.reshape(B * L, ED)


# =====================================================================================================================
# C. recurrent gates and the GLU / SiLU epilogues
# =====================================================================================================================
RNN_RECIPES = ("xproj30", "whh2", "cell_ramp")
# cell_ramp is an LSTM recipe.  whh2 runs 5 steps, not 33: a recurrence with W_hh = +-2 is chaotic, and over 33 steps torch's fp32 run
# ends 0.9 (LSTM) to 1.9 (GRU) relative away from its own fp64 run in y (1e-5 at 5 steps, up to 2e-3 at 9, 1e-2 at 17): past a few
# steps no bound under the cap exists
RNN_CASES = [(r, G, n) for r in ("xproj30", "whh2") for G in (4, 3) for n in (1, 2)] + [("cell_ramp", 4, n) for n in (1, 2)]
SATURATED = 8.0                 # a gate is within 3.4e-4 of 0 or 1 past it
RNN_SHAPE = (2, 33, 32)
RNN_NAMES = ("weight_ih", "bias_ih", "weight_hh", "bias_hh")
EXP_OVERFLOW = 88.7             # expf overflows past it


def rnn_len(recipe):
    return 5 if recipe == "whh2" else RNN_SHAPE[1]


def rnn_torch_cpu(G, n_dirs, d, par, x, dy, dtype, reverse=False, d_in=None):
    """torch's CPU autograd on nn.LSTM / nn.GRU (input width d_in, default d); a single reversed direction is the forward module on
    the time-flipped sequence.  The restatement of tests/test_rnn_train_gpu.py, which imports it from here."""
    m = (nn.LSTM if G == 4 else nn.GRU)(d if d_in is None else d_in, d, 1, bidirectional=n_dirs == 2, batch_first=True).to(dtype)
    m.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in par.items()})
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    y = m(xt.flip(1) if reverse else xt)[0]
    y = y.flip(1) if reverse else y
    y.backward(torch.from_numpy(dy).to(dtype))
    out = {"y": y.detach().numpy(), "x": xt.grad.numpy()}
    out.update({k: getattr(m, k).grad.numpy() for k in par})
    return out


@functools.lru_cache(maxsize=None)
def rnn_recipe(recipe, G, n_dirs, B=RNN_SHAPE[0], d=RNN_SHAPE[2]):
    """-> xproj (B, L, n_dirs G d), w_hh (n_dirs, G d, d), b_hh (n_dirs, G d), dy (B, L, n_dirs d), fp32.  The kernels take projected
    inputs, so the recipe sets them directly."""
    rs = np.random.RandomState(RNN_RECIPES.index(recipe) * 100 + 10 * G + n_dirs)
    L = rnn_len(recipe)
    k = 1.0 / np.sqrt(d)
    xproj = rs.standard_normal((B, L, n_dirs * G * d))
    w_hh, b_hh = rs.uniform(-k, k, (n_dirs, G * d, d)), rs.uniform(-k, k, (n_dirs, G * d))
    if recipe == "xproj30":         # gates at +-90: the exponential overflows on one side
        xproj *= 30.0
    elif recipe == "whh2":          # the hidden path saturates on its own: up to 2 d = 64 behind a gate
        w_hh = np.where(rs.random_sample(w_hh.shape) < 0.5, -2.0, 2.0)
    elif recipe == "cell_ramp":     # LSTM: i = f = 1 and g = 1, so c_t = t; o ~ N(0,1) carries the gradient through tanh(c)
        assert G == 4
        xproj = xproj.reshape(B, L, n_dirs, G, d)
        xproj[:, :, :, :3] = 30.0
        xproj = xproj.reshape(B, L, n_dirs * G * d)
        w_hh, b_hh = 0.01 * w_hh, 0.01 * b_hh
    dy = rs.standard_normal((B, L, n_dirs * d))
    return tuple(a.astype(np.float32) for a in (xproj, w_hh, b_hh, dy))


def rnn_run(G, n_dirs, d, xproj, w_hh, b_hh, dy, dtype):
    """nn.LSTM / nn.GRU fed the projected inputs: weight_ih picks a direction's G d columns (a product with 0 / 1 is exact) and
    bias_ih = 0.  -> y, dxproj, db_hh (n_dirs, G d)."""
    W = n_dirs * G * d
    par = {}
    for r, sfx in enumerate(("", "_reverse")[:n_dirs]):
        w_ih = np.zeros((G * d, W), dtype=np.float32)
        w_ih[np.arange(G * d), r * G * d + np.arange(G * d)] = 1.0
        par.update({"weight_ih_l0" + sfx: w_ih, "bias_ih_l0" + sfx: np.zeros(G * d, dtype=np.float32),
                    "weight_hh_l0" + sfx: w_hh[r], "bias_hh_l0" + sfx: b_hh[r]})
    res = rnn_torch_cpu(G, n_dirs, d, par, xproj, dy, dtype, d_in=W)
    B, L = xproj.shape[:2]
    return {"y": res["y"].reshape(B * L, -1).astype(np.float64), "dxproj": res["x"].reshape(B * L, -1).astype(np.float64),
            "db_hh": np.stack([res["bias_hh_l0" + sfx] for sfx in ("", "_reverse")[:n_dirs]]).astype(np.float64)}


@functools.lru_cache(maxsize=None)
def rnn_refs(recipe, G, n_dirs, d=RNN_SHAPE[2]):
    a = rnn_recipe(recipe, G, n_dirs, RNN_SHAPE[0], d)
    return rnn_run(G, n_dirs, d, *a, torch.float64), rnn_run(G, n_dirs, d, *a, torch.float32)


# csrc/rnn_wide.hip (amt_rnn_wide_seq_fwd / _train_fwd / _bwd: its own sigm and tanhf, W_hh h on fp32 MFMA tiles): every case at
# d = 160 (five 32-column tiles, an odd count) and the bidirectional ones at 256, the first width the CLI uses.  whh2 puts up to
# 2 d = 512 behind a gate; its bound at 256 is the largest of the suite and still under the cap (the host test holds it there)
RNN_WIDE_CASES = [(r, G, n, 160) for r, G, n in RNN_CASES] + [(r, G, n, 256) for r, G, n in RNN_CASES if n == 2]


def rnn_n(recipe, G, B=RNN_SHAPE[0], d=RNN_SHAPE[2]):
    return lambda k: B * rnn_len(recipe) + G * d              # the bound of tests/test_rnn_train_gpu.py


def sigmoid_f32(v, variant="ok"):
    """rnn.hip's 1 / (1 + exp(-v)) in fp32 numpy; variant "exp_over": exp(v) / (1 + exp(v))."""
    v = np.asarray(v, dtype=np.float32)
    one = np.float32(1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        if variant == "exp_over":
            e = np.exp(v, dtype=np.float32)
            return e / (one + e)
        return one / (one + np.exp(-v, dtype=np.float32))


# ops.linear_ex with act 2 (sigmoid) / 3 (SiLU): pre-activations spread over +-100.  N = 64: the vector epilogue; 66: element-wise
ACT_CASES = [(129, N, 64, act, resid) for N in (64, 66) for act in (2, 3) for resid in (False, True)]


@functools.lru_cache(maxsize=None)
def act_inputs(M, N, K, act, resid):
    rs = np.random.RandomState(M + 3 * N + 5 * K + 7 * act + int(resid))
    x = rs.standard_normal((M, K)).astype(np.float32)
    w = (40.0 * K ** -0.5 * rs.standard_normal((N, K))).astype(np.float32)
    b = rs.standard_normal(N).astype(np.float32)
    r = rs.standard_normal((M, N)).astype(np.float32) if resid else None
    return x, w, b, r


def act_run(x, w, b, r, act, dtype):
    t = lambda a: torch.from_numpy(a).to(dtype)
    v = t(x) @ t(w).t() + t(b)
    if r is not None:
        v = v + t(r)
    return {"pre": v.numpy().astype(np.float64), "y": (torch.sigmoid(v) if act == 2 else F.silu(v)).numpy().astype(np.float64)}


# =====================================================================================================================
# D. row statistics
# =====================================================================================================================
NORM_SHAPES = [(37, 512), (5, 36)]
# mean / std of a row.  The rung 4096 is left out: there torch's own fp32 layer_norm is 1.8e-4 (y) and 2.7e-4 (dw) off fp64 at
# (37, 512), so the bound 8 e32 would pass the cap of 1e-3
LADDER = (8, 64, 512)
NORM_RECIPES = tuple(f"ladder{m}" for m in LADDER) + ("constant", "tiny", "huge", "spike", "cancel")
NORM_KINDS = ("layernorm", "layernorm_post", "rmsnorm")
BIG = 1.0e4                               # the cancelling pair: x = BIG + r, resid = -BIG


def norm_recipes_for(kind):
    """RMSNorm takes `huge12` (rows of 1e12) for `huge` (1e15): torch's fp32 autograd of the written-out RMSNorm forms ms^-3/2 = 1e-45,
    which underflows, and its dx is then 3e-2 off fp64 -- the reference's own limit, not the kernel's."""
    return tuple("huge12" if (r == "huge" and kind == "rmsnorm") else r for r in NORM_RECIPES)


@functools.lru_cache(maxsize=None)
def norm_recipe(recipe, rows, dim, resid):
    """-> {x, w, b, dy, post (, resid)} fp32.  With `resid` the row of the recipe is x + resid (resid ~ 0.5 N(0,1) at the row's
    scale); `cancel` exists with resid only."""
    rs = np.random.RandomState(sum(map(ord, recipe)) * 1000 + rows + dim + int(resid))
    z = rs.standard_normal((rows, dim))
    z = (z - z.mean(1, keepdims=True)) / z.std(1, keepdims=True)
    a = {"w": 1.0 + 0.3 * rs.standard_normal(dim), "b": 0.1 * rs.standard_normal(dim), "dy": rs.standard_normal((rows, dim)),
         "post": rs.standard_normal((rows, dim))}
    scale = 1.0
    if recipe.startswith("ladder"):
        x = z + float(recipe[6:]) * np.where(np.arange(rows) % 2, -1.0, 1.0)[:, None]
    elif recipe == "constant":      # variance 0: rstd = eps^-1/2.  Small integers: a row's sum is exact in fp32 in any order, so the
        x = np.tile(rs.randint(1, 4, (rows, 1)) * np.where(np.arange(rows) % 2, -1.0, 1.0)[:, None], (1, dim))      # mean's rounding (the ladder's subject) stays out
    elif recipe == "tiny":          # var << eps
        x, scale = 1e-20 * z, 1e-20
    elif recipe.startswith("huge"):
        scale = 1e12 if recipe == "huge12" else 1e15
        x = scale * z
    elif recipe == "spike":         # one coordinate at 1e4 times the rest
        x = z.copy()
        x[np.arange(rows), rs.randint(0, dim, rows)] = 1e4
    elif recipe == "cancel":
        assert resid
        big = BIG * (1.0 + 0.1 * rs.standard_normal((rows, dim)))
        a["resid"] = -big.astype(np.float32)
        x = big.astype(np.float32).astype(np.float64) + z                 # rounds to the grid of BIG: x + resid is then exact in fp32
    if resid and recipe != "cancel":
        a["resid"] = 0.5 * scale * rs.standard_normal((rows, dim)) if recipe != "constant" else np.zeros((rows, dim))
        x = x - a["resid"].astype(np.float32).astype(np.float64)
    a["x"] = x
    return {k: v.astype(np.float32) for k, v in a.items()}


def norm_run(kind, a, dtype, stats_of_x_alone=False):
    """torch's autograd on F.layer_norm (eps 1e-5) / the RMSNorm of custom_transformer.py (eps 1e-6) of x (+ resid) at `dtype`."""
    t = {k: torch.from_numpy(v).to(dtype).requires_grad_(k in ("x", "w", "b")) for k, v in a.items()}
    u = t["x"] + t["resid"] if "resid" in t else t["x"]
    if kind == "rmsnorm":
        y = u * torch.rsqrt((u * u).mean(-1, keepdim=True) + 1e-6) * t["w"]
    elif stats_of_x_alone:
        mu, var = t["x"].mean(-1, keepdim=True), t["x"].var(-1, unbiased=False, keepdim=True)
        y = (u - mu) * torch.rsqrt(var + 1e-5) * t["w"] + t["b"]
    else:
        y = F.layer_norm(u, (u.shape[1],), t["w"], t["b"], 1e-5)
    if kind == "layernorm_post":
        y = y + t["post"]
    y.backward(t["dy"])
    out = {"y": y.detach().numpy(), "dx": t["x"].grad.numpy(), "dw": t["w"].grad.numpy()}
    if kind != "rmsnorm":
        out["db"] = t["b"].grad.numpy()
    return {k: v.astype(np.float64) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def norm_refs(kind, recipe, rows, dim, resid):
    a = norm_recipe(recipe, rows, dim, resid)
    return norm_run(kind, a, torch.float64), norm_run(kind, a, torch.float32)


def norm_n(rows, dim):
    return lambda k: max(rows, dim)             # the bound of tests/test_layernorm_bwd_gpu.py


def layernorm_one_pass_f32(x, w, b, eps=1e-5):
    """The wrong variant: var = E[x^2] - E[x]^2 in fp32."""
    x = x.astype(np.float32)
    mu = x.mean(1, keepdims=True, dtype=np.float32)
    var = (x * x).mean(1, keepdims=True, dtype=np.float32) - mu * mu
    with np.errstate(invalid="ignore"):
        return (x - mu) / np.sqrt(var + np.float32(eps)) * w + b


# diff_subln: RMSNorm_hd(o1 - lam o2) w out_scale, hd <= 128
SUBLN_SHAPES = [(37, 128), (5, 36)]
SUBLN_RECIPES = tuple(f"ladder{m}" for m in LADDER) + ("constant", "tiny", "huge", "spike", "cancel")
SUBLN_LAM, SUBLN_SCALE = 0.5, 0.8


@functools.lru_cache(maxsize=None)
def subln_inputs(recipe, rows, hd):
    """o1 = the recipe's x, lam o2 = -resid (a division by 0.5 is exact): o1 - lam o2 is the recipe's row; `cancel`: o1 = BIG + r,
    lam o2 = BIG, the difference the well-conditioned row."""
    a = norm_recipe(recipe, rows, hd, True)
    return a["x"], (-a["resid"] / np.float32(SUBLN_LAM)).astype(np.float32), a["w"]


def subln_run(o1, o2, w, dtype, eps=1e-5, grads=False, dy=None, stats_of_o1_alone=False):
    """grads: torch's autograd of y against `dy` with lambda a leaf -> y, d_o1, d_o2, dw, dlambda (1,).  stats_of_o1_alone: the wrong
    variant, the mean square taken of o1 instead of o1 - lam o2."""
    t = lambda v: torch.from_numpy(v).to(dtype).requires_grad_(grads)
    o1, o2, w = t(o1), t(o2), t(w)
    lam = torch.tensor([SUBLN_LAM], dtype=dtype, requires_grad=grads)
    u = o1 - lam * o2
    s = o1 if stats_of_o1_alone else u
    y = u * torch.rsqrt((s * s).mean(-1, keepdim=True) + eps) * w * torch.tensor(SUBLN_SCALE, dtype=dtype)
    out = {"y": y.detach().numpy().astype(np.float64)}
    if grads:
        y.backward(torch.from_numpy(dy).to(dtype))
        out.update({"d_o1": o1.grad, "d_o2": o2.grad, "dw": w.grad, "dlambda": lam.grad})
        out = {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}
    return out


# amt_diff_subln_train_fwd / amt_diff_subln_bwd (csrc/diff_subln_train.hip): the backward takes head_dim 32 / 64 / 128 only.  `huge12`
# for `huge`, as `norm_recipes_for("rmsnorm")` and for its reason: at 1e15 torch's own fp32 autograd is 3 % to 11 % off fp64 in d_o1,
# d_o2 and dlambda (the host test shows it)
SUBLN_BWD_SHAPES = [(37, 128), (70, 32), (5, 64)]
SUBLN_BWD_RECIPES = tuple("huge12" if r == "huge" else r for r in SUBLN_RECIPES)


@functools.lru_cache(maxsize=None)
def subln_bwd_inputs(recipe, rows, hd):
    """`subln_inputs` and the recipe's dy."""
    return subln_inputs(recipe, rows, hd) + (norm_recipe(recipe, rows, hd, True)["dy"],)


@functools.lru_cache(maxsize=None)
def subln_bwd_refs(recipe, rows, hd):
    o1, o2, w, dy = subln_bwd_inputs(recipe, rows, hd)
    return tuple(subln_run(o1, o2, w, dt, grads=True, dy=dy) for dt in (torch.float64, torch.float32))


def subln_bwd_n(rows, hd):
    """The longest sum behind a value: a row's mean square for y, d_o1 and d_o2 (hd, as `test_diff_subln`); for dw and
    dlambda = -sum du o2 the sum over the rows on top of it (a row's share of dlambda is a sum of hd terms, the rows' shares are added)."""
    return lambda k: rows + hd if k in ("dw", "dlambda") else hd


# ---- the folded LayerNorm: y = (raw - mu g) rstd + c (csrc/fold.hip) ----
FOLD_K = 512
FOLD_LADDER = (0, 8, 64, 512)             # mean / std of u; the host test holds every rung's bound to the cap


@functools.lru_cache(maxsize=None)
def fold_inputs(m, B, n_out, seed=0):
    """u (B, K) with mean / std = m, a LayerNorm (gam, bet) and the projection (W, bW) behind it, and the producer's side as
    tests/test_ops_gpu.py forms it (in fp64, rounded once): W' = W o gam, raw = u W'^T, g = rowsum(W'), c = W bet + bW."""
    rs = np.random.RandomState(7 * int(m) + B + n_out + seed)
    z = rs.standard_normal((B, FOLD_K))
    z = (z - z.mean(1, keepdims=True)) / z.std(1, keepdims=True)
    u = (z + m * np.where(np.arange(B) % 2, -1.0, 1.0)[:, None]).astype(np.float32)
    f = dict(u=u, gam=1 + 0.2 * rs.standard_normal(FOLD_K), bet=0.1 * rs.standard_normal(FOLD_K),
             W=rs.standard_normal((n_out, FOLD_K)) * FOLD_K ** -0.5, bW=0.1 * rs.standard_normal(n_out))
    f = {k: v.astype(np.float32) for k, v in f.items()}
    Wp = f["W"].astype(np.float64) * f["gam"].astype(np.float64)
    f["raw"] = (u.astype(np.float64) @ Wp.T).astype(np.float32)
    f["g"] = Wp.sum(1).astype(np.float32)
    f["c"] = (f["W"].astype(np.float64) @ f["bet"].astype(np.float64) + f["bW"]).astype(np.float32)
    return f


def ln_rows(u, gam, bet, dtype, eps=1e-5):
    """Two-pass LayerNorm in numpy at `dtype` -> (LN(u), mu, rstd)."""
    u, gam, bet = (a.astype(dtype) for a in (u, gam, bet))
    mu = u.mean(1, keepdims=True, dtype=dtype)
    var = ((u - mu) ** 2).mean(1, keepdims=True, dtype=dtype)
    rstd = (1.0 / np.sqrt(var + dtype(eps))).astype(dtype)
    return (u - mu) * rstd * gam + bet, mu, rstd


def fold_proj(f, how):
    """LayerNorm(u) W^T + bW: "ref64"; "folded32": (raw - mu g) rstd + c in fp32, as fold.hip's header states it; "unfolded32": the
    LayerNorm, then the product, both in fp32."""
    if how == "ref64":
        return ln_rows(f["u"], f["gam"], f["bet"], np.float64)[0] @ f["W"].astype(np.float64).T + f["bW"].astype(np.float64)
    ln, mu, rstd = ln_rows(f["u"], f["gam"], f["bet"], np.float32)
    if how == "folded32":
        return (f["raw"] - mu * f["g"]) * rstd + f["c"]
    return ln @ f["W"].T + f["bW"]


FOLD_DECODE = dict(B=5, H=8, hd=64, cap=40)          # d = H hd = FOLD_K


@functools.lru_cache(maxsize=None)
def fold_decode_case(m):
    """amt_attn_decode_fold_fwd with the new key / value row, no relative positions: the fold's inputs at n_out = 3 d and a cache."""
    B, H, hd, cap = (FOLD_DECODE[k] for k in ("B", "H", "hd", "cap"))
    f = fold_inputs(m, B, 3 * H * hd)
    rs = np.random.RandomState(int(m) + 1)
    return f, rs.standard_normal((B, H, cap, hd)).astype(np.float32), rs.standard_normal((B, H, cap, hd)).astype(np.float32)


def fold_decode_outputs(m, how):
    """{xo, k_new, v_new, o} of the decode attention at position cap - 1 from the projection formed as `how` says."""
    f, kc, vc = fold_decode_case(m)
    B, H, hd, cap = (FOLD_DECODE[k] for k in ("B", "H", "hd", "cap"))
    d, dt = H * hd, np.float64 if how == "ref64" else np.float32
    proj = fold_proj(f, how).astype(dt)
    q = (proj[:, :d] * dt(hd ** -0.5)).reshape(B, H, 1, hd)
    K, V = kc.astype(dt).copy(), vc.astype(dt).copy()
    K[:, :, cap - 1], V[:, :, cap - 1] = proj[:, d:2 * d].reshape(B, H, hd), proj[:, 2 * d:].reshape(B, H, hd)
    s = q @ K.transpose(0, 1, 3, 2)
    p = np.exp(s - s.max(-1, keepdims=True))
    o = (p / p.sum(-1, keepdims=True, dtype=dt)) @ V
    out = {"xo": ln_rows(f["u"], f["gam"], f["bet"], dt)[0], "k_new": K[:, :, cap - 1], "v_new": V[:, :, cap - 1], "o": o.reshape(B, d)}
    return {k: v.astype(np.float64) for k, v in out.items()}


FOLD_FFN = dict(B=32, K1=1024, n_low=512, n_high=160)        # the shape of tests/test_ops_gpu.py's folded-FFN case; K2 = FOLD_K


@functools.lru_cache(maxsize=None)
def fold_ffn_case(m):
    B, K1, n_low, n_high = (FOLD_FFN[k] for k in ("B", "K1", "n_low", "n_high"))
    f = fold_inputs(m, B, K1, seed=1)
    rs = np.random.RandomState(int(m) + 2)
    r = lambda *s, scale=1.0: (rs.standard_normal(s) * scale).astype(np.float32)
    return f, dict(wl=r(n_low, K1, scale=K1 ** -0.5), bl=r(n_low, scale=0.1), wh=r(n_high, K1 + FOLD_K, scale=(K1 + FOLD_K) ** -0.5),
                   bh=r(n_high, scale=0.1))


def fold_ffn_outputs(m, how):
    """{y_low, y_high} of the folded-FFN prologue: rows = [relu(proj) | LayerNorm(u)], y_low = relu(proj) wl^T + bl + LN(u)[:, :n_low],
    y_high = rows wh^T + bh."""
    f, w = fold_ffn_case(m)
    dt = np.float64 if how == "ref64" else np.float32
    a = np.maximum(fold_proj(f, how).astype(dt), 0)
    ln = ln_rows(f["u"], f["gam"], f["bet"], dt)[0]
    t = lambda k: w[k].astype(dt)
    out = {"y_low": a @ t("wl").T + t("bl") + ln[:, :FOLD_FFN["n_low"]], "y_high": np.concatenate([a, ln], 1) @ t("wh").T + t("bh")}
    return {k: v.astype(np.float64) for k, v in out.items()}


FOLD_LINEAR = dict(B=7, N=512)


def fold_linear_outputs(m, how):
    """amt_decode_linear_fwd with its fused LayerNorm: {y, xn}; the kernel normalises and multiplies, so its fp32 yardstick is "unfolded32"."""
    f = fold_inputs(m, FOLD_LINEAR["B"], FOLD_LINEAR["N"], seed=2)
    dt = np.float64 if how == "ref64" else np.float32
    return {"y": fold_proj(f, how).astype(np.float64), "xn": ln_rows(f["u"], f["gam"], f["bet"], dt)[0].astype(np.float64)}


# ---- mixture layer and gated experts with saturated gates ----
MOE_CASES = [(37, 64, 65, 8, 2), (37, 64, 65, 8, 3)]          # n_tok, d, dff_raw (padded to 96), n_exp, k; GLU experts and a shared one
GATE_SCALE = 100.0              # the router
EXPERT_GATE_SCALE = 40.0        # the gate branch of every expert and of the shared one, as GLU_SCALE


@functools.lru_cache(maxsize=None)
def moe_recipe(n_tok, d, raw, n_exp, k):
    """The layer of tests/helpers_moe_train.py with the router's weights and bias times 100 -- the top-k weights go to (1, 0, ..) and the
    router's gradient is what is left of it -- and the gate branch of every expert times 40: silu and its derivative in the grouped
    kernels of csrc/moe_train_kernels.h see pre-activations over +-100.  -> x, dout, P, fp64 and fp32 results of `layer_grads`."""
    from tests import helpers_moe_train as TMoe
    x, dout, P = TMoe.layer_params(n_tok, d, raw, n_exp, k, True, True, seed=3)
    P = dict(P)
    P["gate.weight"], P["gate.bias"] = P["gate.weight"] * np.float32(GATE_SCALE), P["gate.bias"] * np.float32(GATE_SCALE)
    for key in P:
        if key.endswith((".gate.weight", ".gate.bias")):                 # experts.N.gate.*, shared_expert.gate.*
            P[key] = P[key] * np.float32(EXPERT_GATE_SCALE)
    o64 = TMoe.layer_grads(x, dout, P, n_exp, k, True)
    o32 = TMoe.layer_grads(x, dout, P, n_exp, k, True, dtype=torch.float32)
    return x, dout, P, o64, o32


def moe_tensors(o):
    return {"out": o["out"], "weights": o["weights"], **o["grads"]}


def moe_n(n_tok, d, raw, k):
    return lambda name: max(raw, d) + k if name in ("x", "out") else k if name == "weights" else max(n_tok, raw, d)      # tests/test_moe_bwd_gpu.py


# amt_moe_train_fwd_balanced (csrc/moe.hip): the V3 selection bias on the saturated router -- the experts are chosen on logits + bias and
# weighed by the softmax of their raw logits.  The bias is a permuted ramp (helpers_v3_train.BIAS_ORDER's analogue for 8 experts) of
# the logits' own standard deviation, as `case_bias` of tests/test_v3_train_ops_gpu.py scales it
MOE_BIAS_ORDER = (3, 0, 5, 1, 7, 4, 2, 6)


def moe_biased_grads(x, dout, P, bias, n_exp, k, dtype, weights_biased=False):
    """`helpers_moe_train.layer_grads` of the shared GLU layer with the routing of helpers_v3_train.forward_restated's `ff`: top-k of
    logits + bias, softmax over the chosen experts' raw logits.  weights_biased: the wrong variant, the softmax over logits + bias.
    Also: gap, the smallest k-th versus (k+1)-th selection value relative to the largest, and the share of rows whose expert set is not
    the raw logits'."""
    from tests import helpers_moe_train as TMoe
    with torch.enable_grad():
        t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
        Pt = {key: t(v).requires_grad_(True) for key, v in P.items()}
        xt = t(x).requires_grad_(True)
        logits = TMoe.gate_logits(Pt, "", xt)
        sel = logits + t(bias)
        idx = torch.topk(sel, k, dim=-1).indices
        w = torch.softmax(torch.gather(sel if weights_biased else logits, -1, idx), dim=-1)
        out = torch.zeros_like(xt)
        for e in range(n_exp):
            tok, j = torch.where(idx == e)
            if tok.numel():
                out = out.index_add(0, tok, w[tok, j].unsqueeze(1) * TMoe.expert(Pt, f"experts.{e}.", xt[tok]))
        out = out + (1.0 / k) * TMoe.expert(Pt, "shared_expert.", xt)
        (out * t(dout)).sum().backward()
    g = {key: (torch.zeros_like(v) if v.grad is None else v.grad).numpy().astype(np.float64) for key, v in Pt.items()}
    g["x"] = xt.grad.numpy().astype(np.float64)
    plain = torch.topk(logits.detach(), k, dim=-1).indices.sort(-1).values
    return {"out": out.detach().numpy().astype(np.float64), "grads": g, "idx": idx.numpy(), "weights": w.detach().numpy().astype(np.float64),
            "gap": TMoe.gate_gap(sel, k), "flipped": float((idx.sort(-1).values != plain).any(-1).double().mean())}


@functools.lru_cache(maxsize=None)
def moe_biased_recipe(n_tok, d, raw, n_exp, k):
    """`moe_recipe` and a selection bias -> x, dout, P, bias (n_exp,) fp32, fp64 and fp32 results of `moe_biased_grads`."""
    x, dout, P, _, _ = moe_recipe(n_tok, d, raw, n_exp, k)
    logits = x.astype(np.float64) @ P["gate.weight"].astype(np.float64).T + P["gate.bias"]
    assert n_exp == len(MOE_BIAS_ORDER)
    bias = (logits.std() * np.linspace(-1.0, 1.0, n_exp)[list(MOE_BIAS_ORDER)]).astype(np.float32)
    return x, dout, P, bias, moe_biased_grads(x, dout, P, bias, n_exp, k, torch.float64), moe_biased_grads(x, dout, P, bias, n_exp, k, torch.float32)


GLU_CASES = [(129, 32, 100, False), (129, 32, 100, True)]       # n, d, dff (padded to 128), SiLU expert
GLU_SCALE = 40.0


@functools.lru_cache(maxsize=None)
def glu_recipe(n, d, dff, silu):
    """tests/helpers_family_train.glu_inputs with the gate branch's weights and bias times 40: pre-activations over +-100."""
    from tests import helpers_family_train as FT
    sd, a, _ = FT.glu_inputs(n, d, dff, silu, False)
    sd = dict(sd)
    for key in (("0.weight", "0.bias") if silu else ("gate.weight", "gate.bias")):
        sd[key] = sd[key] * np.float32(GLU_SCALE)
    return sd, a


@functools.lru_cache(maxsize=None)
def glu_refs(n, d, dff, silu):
    from tests import helpers_family_train as FT
    sd, a = glu_recipe(n, d, dff, silu)
    return FT.glu_restated(sd, a, None, torch.float64), FT.one_thread(FT.glu_restated, sd, a, None, torch.float32)


# ---- VideoRegression('bimamba+') on slow_decay weights: three 64-row blocks of the forward scan ----
REG_SLOW = dict(n_layers=1, d_model=32, d_hidden=64, total_vf_dim=7, regModel="bimamba+")
REG_SLOW_BS = (1, 129)


@functools.lru_cache(maxsize=None)
def reg_slow_case():
    from tests import helpers_reg_parity as HR
    from video2music_amd import synthetic
    sd = {k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(HR.named_shapes(**REG_SLOW), seed=77).items()}
    for k in sd:
        if k.endswith("dt_proj.bias"):
            sd[k] = torch.full_like(sd[k], -6.9)
        elif k.endswith("dt_proj.weight"):
            sd[k] = sd[k] * 0.05
        elif k.endswith("A_log"):
            sd[k] = torch.zeros_like(sd[k])
        elif k.endswith(".D"):
            sd[k] = sd[k] * 1e-3
    rs = np.random.RandomState(78)
    B, S = REG_SLOW_BS
    z = rs.standard_normal((B, S, 6))
    e = np.exp(z - z.max(-1, keepdims=True))
    return sd, torch.from_numpy(rs.standard_normal((B, S, 1)).astype(np.float32)), torch.from_numpy((e / e.sum(-1, keepdims=True)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def reg_slow_refs():
    from oracle import reg_oracle
    sd, sem, emo = reg_slow_case()
    out = []
    for dt in (torch.float64, torch.float32):
        col = {}
        with torch.no_grad():
            reg_oracle.forward(sd, sem, emo, collect=col, reg_model="bimamba+", dtype=dt)
        out.append({"feature": col["feature"].numpy().astype(np.float64)})
    return tuple(out)


# ---- profiles/numeric_range_fold.json ----
FOLD_JSON_ENV = "NUMERIC_RANGE_FOLD_JSON"     # a path: the fold tests of tests/test_numeric_range_gpu.py then write their rows there
FOLD_WHAT = ("tests/test_numeric_range_gpu.py on one MI355X, written by its fold tests when " + FOLD_JSON_ENV + " names this file: per form and "
             "mean / std of the LayerNorm's input row (K = 512), max |y - fp64| / max |fp64| of the kernel, of the fp32 evaluation of "
             "(raw - mu g) rstd + c and of LayerNorm then product in fp32; kernel_over_unfolded32 is the worst ratio over the outputs behind "
             "the fold (xo / xn, the LayerNorm itself, left out).  raw = u W'^T is formed in fp64 and rounded once, as tests/test_ops_gpu.py "
             "forms it: the kernel and folded32 are handed an exact product while unfolded32 runs its own fp32 product, so the figures are "
             "those of the consumer kernels alone, not of a chain whose producer GEMM runs in fp32 on the device (an fp32 raw of magnitude "
             "|mu g| adds about |mu g| 2^-24 sqrt(K) rstd).")
FOLD_DIRECT = ("xo", "xn")              # the LayerNorm itself, not behind the fold


def fold_row(form, m, got, fn):
    """One row of the file: the kernel's error per output beside the folded and the unfolded fp32 evaluation's."""
    w64 = fn(m, "ref64")
    sig = lambda v: float(f"{v:.3e}")
    row = {"form": form, "mean_over_std": m}
    for how in ("folded32", "unfolded32"):
        w = fn(m, how)
        row[how] = {k: sig(rel_err(w[k], w64[k])) for k in w64}
    row["kernel"] = {k: sig(rel_err(got[k], w64[k])) for k in w64}
    row["kernel_over_unfolded32"] = round(max(row["kernel"][k] / row["unfolded32"][k] for k in w64 if k not in FOLD_DIRECT), 2)
    return row


def fold_write(path, row):
    """Puts `row` into the JSON at `path` in the place of the row of the same form and mean / std, rows kept in (form, mean / std) order."""
    import json
    import os
    rows = json.load(open(path))["rows"] if os.path.exists(path) else []
    key = lambda r: (r["form"], r["mean_over_std"])
    rows = sorted([r for r in rows if key(r) != key(row)] + [row], key=key)
    with open(path, "w") as f:
        json.dump({"what": FOLD_WHAT, "rows": rows}, f, indent=1)
        f.write("\n")
