"""Chord-model training at the shapes where its kernels change route: the case table, the per-case batch, the bounds and the wrong
variants of tests/test_train_edges_host.py and tests/test_train_edges_gpu.py.  Everything is computed from the restatement of
tests/helpers_train.py (pinned to the reference's own fp64 gradients by tests/test_train_host.py); nothing is recorded.

A case is named for the edge it exists for; its sizes are the smallest at which that route is taken (the host test derives the routes
from the shapes by asking the library, tests/launch_routes.py)."""
import functools
import re

import numpy as np
import torch

from tests import helpers_eval as HE
from tests import helpers_train as T
from tests import launch_routes as R
from video2music_amd.utilities import constants as C

P_DROP = 0.2
GRAD_FACTOR, LOGIT_FACTOR = 8, 4            # of test_train_gpu.py (gradients) and of the decode parity (logits)
MISS = 10                                   # a wrong variant misses its bound by at least this factor
KINK = 2.0 ** -14                           # no ReLU pre-activation within KINK x its layer's rms of 0 (see `clear_kinks`)
KEYS = (1.0, 0.5, 0.0)                      # clip b gets KEYS[b % 3]: clip 0's key column is never silent


def cfg_of(n_layers, H, d, d_ff, er_len, F, rpr=True):
    return dict(n_layers=n_layers, num_heads=H, d_model=d, dim_feedforward=d_ff, max_sequence_chord=er_len, max_sequence_video=300,
                total_vf_dim=F, rpr=rpr)


DEPLOYED = cfg_of(1, 8, 512, 1024, 300, 776)
HD128 = cfg_of(1, 8, 1024, 32, 40, 37)
D96 = cfg_of(2, 3, 96, 160, 64, 37)
L6X = cfg_of(1, 2, 64, 128, 65, 32)


def _case(cfg, B, S, L, seed, causal=True, small_norms=False, p=0.0, all_pad=None, unfused=False):
    return dict(cfg=cfg, B=B, S=S, L=L, seed=seed, causal=causal, small_norms=small_norms, p=p, all_pad=all_pad, unfused=unfused)


CASES = {
    # 64-tile GEMM forward (450 x 1536 > 650k) and in the weight gradients (1536 x 513: odd N, element-wise stores), ReLU epilogue;
    # head_dim 64 with Er; Er-free attention on the 128-row kernel (Lk < 256); F = 776 = 24 * 32 + 8: the padded Linear_vis
    "deployed_width": _case(DEPLOYED, 3, 150, 150, 1, unfused=True),
    # the deployed layer at the deployed lengths: split-key encoder and cross attention at head_dim 64, three query blocks, L = er_len - 1
    "deployed_300": _case(DEPLOYED, 2, 300, 299, 2),
    # head_dim 128 (never split-key), LayerNorm backward at its widest, d_ff < d_model, K = 1024 on the skinny GEMM, Er 7 rows longer
    # than L, one query row past a 32-row wave
    "hd128_d1024": _case(HD128, 2, 20, 33, 3),
    # width no multiple of 64, three heads, three clips, two layers, F = 37, Er 27 rows longer than L
    "d96_h3": _case(D96, 3, 17, 37, 4),
    # one key everywhere: dS cancels, dEr is identically zero, the chord loss sees one row
    "one_by_one": _case(cfg_of(1, 1, 32, 32, 1, 7), 1, 1, 1, 5),
    # M = 4200 rows: past the skinny GEMM's row limit, M N far below its output limit; weight gradients with K = 4224; LayerNorm
    # backward above its 2048-row spread; dEr summed over 14 slabs
    "rows_gt_4096": _case(cfg_of(1, 1, 32, 32, 300, 32), 14, 40, 300, 6),
    # B L = 1677: weight-gradient K = 1696 > 1536 leaves the skinny GEMM while M N is small; L = 129: one row in the second query
    # block and in the fifth key tile
    "k_gt_1536": _case(cfg_of(1, 2, 64, 128, 129, 32), 13, 129, 129, 7),
    # mask=False decoder; split-key encoder at Lk = 257 (one key in the ninth tile); cross-attention Lq 70 / Lk 257; L = 70 in the
    # chord loss (second workgroup of 6 rows)
    "plain_noncausal": _case(cfg_of(1, 2, 64, 32, 70, 64, rpr=False), 2, 257, 70, 8, causal=False),
    # the chord loss's workgroup boundary, exactly and plus one; Er of L + 1 rows and of L rows
    "L64": _case(L6X, 2, 33, 64, 9),
    "L65": _case(L6X, 2, 33, 65, 10, unfused=True),
    # clip 1 has only PAD targets: its cross-entropy rows are all ignored, its BCE rows still count
    "all_pad_clip": _case(dict(D96, n_layers=1), 3, 17, 37, 11, all_pad=1),
    # the only cases that can see a LayerNorm epsilon, forward or backward
    "small_norms/deployed_width": _case(DEPLOYED, 3, 150, 150, 12, small_norms=True),
    "small_norms/hd128_d1024": _case(HD128, 2, 20, 33, 13, small_norms=True),
    "small_norms/d96_h3": _case(D96, 3, 17, 37, 14, small_norms=True),
    # injected masks, every attention mask with one fully dropped row: keep_scale and the element-wise multipliers at three heads and at
    # head_dim 64
    "dropout/d96_h3": _case(D96, 3, 17, 37, 15, p=P_DROP),
    "dropout/deployed_width": _case(DEPLOYED, 3, 150, 150, 16, p=P_DROP),
}
ZERO_GRADS = {"one_by_one": ("transformer.decoder.layers.0.self_attn.Er",)}       # the fp64 gradients that are identically zero


def feature_widths(F):
    """(semantic, scene, motion, emotion) widths that `_vfc` of width F is cut into for the module call."""
    emo = 6 if F >= 9 else F - 3
    return F - 2 - emo, 1, 1, emo


def batch(name):
    """The case's inputs as numpy arrays, deterministic per case.  `vfc` (B, S, F) holds the concatenated feature rows."""
    c = CASES[name]
    B, S, L, F = c["B"], c["S"], c["L"], c["cfg"]["total_vf_dim"]
    rng = np.random.default_rng(c["seed"])
    bt = {"x_root": rng.integers(0, C.CHORD_ROOT_SIZE, size=(B, L)), "x_attr": rng.integers(0, C.CHORD_ATTR_SIZE, size=(B, L)),
          "tgt": rng.integers(0, C.CHORD_END, size=(B, L)), "emo_class": rng.integers(0, 6, size=(B, L)).astype(np.int32),
          "key": np.array([KEYS[b % 3] for b in range(B)], dtype=np.float32), "vfc": rng.standard_normal((B, S, F)).astype(np.float32)}
    if L >= 4:
        bt["tgt"][0, -2], bt["tgt"][0, -1] = C.CHORD_END, C.CHORD_PAD
    if c["all_pad"] is not None:
        bt["tgt"][c["all_pad"]] = C.CHORD_PAD
    bt["x"] = bt["x_root"]                                      # the module reads its shape only
    return bt


@functools.lru_cache(maxsize=None)
def state_dict(name):
    """The case's weights (numpy fp32; shared, read-only): the synthetic recipe, the norms scaled down in the small-norms cases, and
    the feed-forward biases nudged by `clear_kinks`."""
    c = CASES[name]
    sd = T.state_dict(c["cfg"], c["seed"])
    if c["small_norms"]:
        sd = {k: (v * 0.02 if re.search(r"\.norm\d*\.weight$", k) else v * 0.3 if re.search(r"\.norm\d*\.bias$", k) else v).astype(v.dtype)
              for k, v in sd.items()}
    return clear_kinks(dict(sd), name)


def ffn_bias_keys(cfg):
    """The linear1 biases in the order the forward reaches their ReLUs."""
    return [f"transformer.{part}.layers.{i}.linear1.bias" for part in ("encoder", "decoder") for i in range(cfg["n_layers"])]


def pre_relu(sd, name, dtype):
    """The feed-forward pre-activations of the restatement's forward, one (rows, d_ff) array per ReLU in forward order."""
    c, m = CASES[name], masks(name)
    tap = []
    with torch.no_grad():
        T.forward({k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items()}, c["cfg"], restated_batch(batch(name), dtype),
                  None if m is None else T.Masks(m, c["p"]), c["causal"], pre_relu=tap)
    return [z.reshape(-1, z.shape[-1]).to(torch.float64).numpy() for z in tap]


def clear_kinks(sd, name):
    """A ReLU whose pre-activation is within rounding of 0 is open in one arithmetic and shut in another, and its whole term of the
    weight gradients comes or goes with it: no bound derived from rounding holds such a unit, in the fp32 restatement (it shows as an
    e32 of 1e-4) or on the device.  With a million units of unit scale (d_ff 1024 over 900 rows) a few always lie within 4e-6 of 0,
    whatever the seed, so the case is conditioned instead: going through the feed-forwards in forward order, the bias of every hidden
    column that has a pre-activation within KINK x the layer's rms of 0 (fp64) is moved by the smallest multiple of twice that margin
    which leaves the whole column clear.  About one column in fifty moves, by 1e-4 of the pre-activations' scale.  The host test
    asserts the outcome against the measured fp32 error of the pre-activations."""
    for j, k in enumerate(ffn_bias_keys(CASES[name]["cfg"])):
        z = pre_relu(sd, name, torch.float64)[j]                 # the biases moved so far are upstream of this layer
        delta = KINK * float(np.sqrt((z * z).mean()))
        b = sd[k].copy()
        for col in np.nonzero(np.abs(z).min(axis=0) < delta)[0]:
            for step in (s * n * 2 * delta for n in range(1, 9) for s in (1, -1)):
                moved = float(np.float32(b[col] + step)) - float(b[col])
                if np.abs(z[:, col] + moved).min() >= delta:
                    b[col] = np.float32(b[col] + step)
                    break
            else:
                raise AssertionError(f"{name}: no clear position for column {col} of {k}")
        sd[k] = b
    return sd


def relu_margin(name):
    """(the smallest |pre-activation| of the case in fp64, the largest fp32 error of a pre-activation) over all feed-forwards."""
    z64, z32 = pre_relu(state_dict(name), name, torch.float64), pre_relu(state_dict(name), name, torch.float32)
    return min(float(np.abs(z).min()) for z in z64), max(float(np.abs(a - b).max()) for a, b in zip(z64, z32))


def masks(name):
    """The injected dropout masks of a dropout case (None elsewhere); every attention keep mask has one fully dropped row."""
    c = CASES[name]
    if c["p"] <= 0:
        return None
    m = T.draw_masks(c["cfg"], c["p"], c["seed"], c["B"], c["L"], c["S"])
    for a in m:
        if a.dtype == np.uint8:
            a[-1, -1, a.shape[2] // 2, :] = 0
    return m


def restated_batch(bt, dtype):
    return dict(bt, _vfc=torch.from_numpy(bt["vfc"]).to(dtype))


def rel_err(got, want, scale=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / (np.abs(want).max() if scale is None else scale))


def grad_scale(g64, k):
    """What a gradient's error is taken relative to: its own fp64 maximum, or, where that is identically zero (Er with one key), the
    maximum of the same attention's in_proj_weight gradient."""
    m = float(np.abs(g64[k]).max())
    return m if m > 0 else float(np.abs(g64[k.rsplit(".", 1)[0] + ".in_proj_weight"]).max())


def grad_errors(got, g64):
    return {k: rel_err(got[k], g, grad_scale(g64, k)) for k, g in g64.items() if g is not None}


def logit_err(y, y64):
    return float(np.abs(np.asarray(y, dtype=np.float64) - y64).max() / max(1.0, np.abs(y64).max()))


def run(name, dtype, variant=None):
    """(losses (3,), logits, {key: gradient or None}) of the restatement on the case's inputs, or of one of its wrong VARIANTS."""
    c = CASES[name]
    bt, sd, m = batch(name), state_dict(name), masks(name)
    P = {k: torch.as_tensor(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in sd.items()}
    v = dict(P=P, bt=bt, masks=m, p=c["p"], causal=c["causal"], fwd={}, smoothing=T.SMOOTHING, loss=T.loss, L=c["L"])
    if variant is not None:
        VARIANTS[variant][0](v)
    mk = None if v["masks"] is None else T.Masks(v["masks"], v["p"])
    logits = T.forward(v["P"], c["cfg"], restated_batch(v["bt"], dtype), mk, v["causal"], **v["fwd"])
    total, chord, emotion = v["loss"](logits, bt, v["smoothing"])
    total.backward()
    return (np.array([float(total.detach()), float(chord.detach()), float(emotion.detach())]), logits.detach().numpy(),
            {k: None if p.grad is None else p.grad.numpy() for k, p in P.items()})


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's fp64 and fp32 restatement (the fp32 one on one CPU thread, so that e32 repeats) and its noise levels: e32 the largest
    relative gradient error of fp32 (`<m>_e32_grad` of tools/make_goldens_train.py on the case's own inputs), e32_y the same measure of
    the logits.  Shared by every test of a process; treat it as read-only."""
    r64 = run(name, torch.float64)
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        r32 = run(name, torch.float32)
    finally:
        torch.set_num_threads(n)
    e32 = max(grad_errors(r32[2], r64[2]).values())
    yl = torch.from_numpy(r64[1]).requires_grad_(True)
    T.loss(yl, batch(name))[0].backward()
    return dict(l64=r64[0], y64=r64[1], g64=r64[2], l32=r32[0], y32=r32[1], g32=r32[2], e32=e32, e32_y=logit_err(r32[1], r64[1]),
                dl_dy_sum=float(yl.grad.abs().sum()))


def loss_bound(ref):
    """|loss - l64| <= D sum |dL/dy| + 159 U |l64| with D the logits bound in absolute terms: the form of test_train_gpu.py with the
    measured D in place of 1e-4."""
    D = LOGIT_FACTOR * ref["e32_y"] * max(1.0, float(np.abs(ref["y64"]).max()))
    return D * ref["dl_dy_sum"] + 159 * T.U * abs(ref["l64"][0])


# ---- wrong variants of the restatement: each edits the run's description `v` before the forward ----

def _er_keys(v):
    return [k for k in v["P"] if k.endswith(".Er")]


def _v_eps(v):
    v["fwd"]["eps"] = 1e-6


def _v_er_first_rows(v):
    """The first L rows of the table where the last L belong (the gradient still lands on the rows that were read)."""
    L = v["L"]
    v["P"] = dict(v["P"], **{k: torch.cat([v["P"][k][L:], v["P"][k][:L]]) for k in _er_keys(v)})


def _v_er_shifted(v):
    v["P"] = dict(v["P"], **{k: torch.roll(v["P"][k], 1, 0) for k in _er_keys(v)})


def _v_keep_unscaled(v):
    v["p"] = 0.0                                                # T.mha divides the kept probabilities by 1 - p


def _v_mask_one_site_late(v):
    """Every element-wise mask is used at the next site of its shape (the last one at the first)."""
    m = list(v["masks"])
    by_shape = {}
    for i, a in enumerate(m):
        if a.dtype != np.uint8:
            by_shape.setdefault(a.shape, []).append(i)
    out = list(m)
    for idx in by_shape.values():
        assert len(idx) >= 2
        for j, i in enumerate(idx):
            out[i] = m[idx[j - 1]]
    v["masks"] = out


def _v_no_key(v):
    v["bt"] = dict(v["bt"], key=np.zeros_like(v["bt"]["key"]))


def _v_tail_features_dropped(v):
    vfc = v["bt"]["vfc"].copy()
    assert vfc.shape[2] % 32
    vfc[:, :, vfc.shape[2] // 32 * 32:] = 0
    v["bt"] = dict(v["bt"], vfc=vfc)


def _v_pe_off_by_one(v):
    v["fwd"]["pe_offset"] = 1


def _loss_pad_counted(logits, bt, smoothing=T.SMOOTHING, lam=T.LAM):
    tgt = torch.as_tensor(bt["tgt"]).reshape(-1)
    rows = torch.as_tensor(HE.emotion_rows(bt["tgt"], bt["emo_class"])).to(logits.dtype)
    chord = torch.nn.CrossEntropyLoss(label_smoothing=smoothing)(logits.reshape(-1, C.CHORD_SIZE), tgt)
    emotion = torch.nn.BCEWithLogitsLoss()(logits, rows)
    return lam * chord + (1 - lam) * emotion, chord, emotion


def _v_pad_counted(v):
    v["loss"] = _loss_pad_counted


def _v_no_smoothing(v):
    v["smoothing"] = 0.0


def _v_causal(v):
    v["causal"] = True


SMALL = ("d96_h3", "hd128_d1024", "one_by_one", "L64", "L65", "all_pad_clip", "plain_noncausal")     # under 0.1 s each in fp64
# variant: (edit, changes the forward, the cases named for it)
VARIANTS = {
    "layernorm_eps_1e-6": (_v_eps, True, tuple(n for n, c in CASES.items() if c["small_norms"])),
    "er_first_rows": (_v_er_first_rows, True, tuple(n for n, c in CASES.items()
                                                      if c["cfg"]["rpr"] and c["cfg"]["max_sequence_chord"] > c["L"] and n in SMALL + ("dropout/d96_h3", "small_norms/d96_h3", "small_norms/hd128_d1024"))),
    "er_shifted_one_row": (_v_er_shifted, True, ("d96_h3", "hd128_d1024", "L64", "L65", "all_pad_clip", "k_gt_1536")),
    "keep_mask_unscaled": (_v_keep_unscaled, True, tuple(n for n, c in CASES.items() if c["p"] > 0)),
    "mask_one_site_late": (_v_mask_one_site_late, True, tuple(n for n, c in CASES.items() if c["p"] > 0)),
    "key_column_dropped": (_v_no_key, True, SMALL),
    "tail_features_dropped": (_v_tail_features_dropped, True, tuple(n for n, c in CASES.items() if c["cfg"]["total_vf_dim"] in (37, 776)
                                                                    and (n in SMALL or n == "deployed_width"))),
    "pe_row_off_by_one": (_v_pe_off_by_one, True, SMALL),
    "pad_rows_counted": (_v_pad_counted, False, tuple(n for n in SMALL if n != "one_by_one")),
    "no_label_smoothing": (_v_no_smoothing, False, SMALL),
    "causal_decoder": (_v_causal, True, ("plain_noncausal",)),
}
RECIPE_EPS_CASES = ("deployed_width", "hd128_d1024", "d96_h3")     # where eps 1e-6 stays under 2 bounds: why the small-norms cases exist


def variant_miss(name, variant):
    """(worst gradient error / (8 e32), logits error / (4 e32_y)) of a wrong variant in fp64 against the case's fp64 reference."""
    ref = reference(name)
    _, y, g = run(name, torch.float64, variant)
    errs = grad_errors(g, ref["g64"])
    return max(errs.values()) / (GRAD_FACTOR * ref["e32"]), logit_err(y, ref["y64"]) / (LOGIT_FACTOR * ref["e32_y"]), errs


# ---- what one training step launches ----

def products(cfg, B, S, L):
    """Every dense product of one training step as (pass, name, M, N, K, act): the forward's LinearFn calls of `_forward_train` and what
    `autograd._linear_backward` / `EmbeddingFn.backward` build from them (`mm_nt` for dx, `mm_tn(..., ones=True)` for dw | db)."""
    d, ff, F, n = cfg["d_model"], cfg["dim_feedforward"], cfg["total_vf_dim"], cfg["n_layers"]
    c32 = lambda v: (v + 31) // 32 * 32
    out = []

    def linear(name, M, N, K0, act=0, need_x=True):
        out.append(("fwd", name, M, N, c32(K0), act))
        if need_x:
            out.append(("bwd", name + ".dx", M, K0, c32(N), 0))
        out.append(("bwd", name + ".dw", N, c32(K0) + 1, c32(M), 0))

    def attn(pre, Mq, Mkv, cross):
        if cross:
            linear(pre + ".q", Mq, d, d)
            linear(pre + ".kv", Mkv, 2 * d, d)
        else:
            linear(pre + ".qkv", Mq, 3 * d, d)
        linear(pre + ".out_proj", Mq, d, d)

    linear("Linear_vis", B * S, d, F, need_x=False)
    linear("Linear_chord", B * L, d, d + 1)
    out.append(("bwd", "embedding_root", 15, d, c32(B * L), 0))
    out.append(("bwd", "embedding_attr", 16, d, c32(B * L), 0))
    for i in range(n):
        attn(f"enc{i}.self_attn", B * S, B * S, False)
        linear(f"enc{i}.linear1", B * S, ff, d, act=1)
        linear(f"enc{i}.linear2", B * S, d, ff)
    for i in range(n):
        attn(f"dec{i}.self_attn", B * L, B * L, False)
        attn(f"dec{i}.multihead_attn", B * L, B * S, True)
        linear(f"dec{i}.linear1", B * L, ff, d, act=1)
        linear(f"dec{i}.linear2", B * L, d, ff)
    linear("Wout", B * L, C.CHORD_SIZE, d)
    return out


def attentions(cfg, B, S, L):
    """(name, B, H, Lq, Lk, head_dim, Er) of the attentions of one layer's worth (all layers are alike)."""
    H, hd = cfg["num_heads"], cfg["d_model"] // cfg["num_heads"]
    return [("enc.self_attn", B, H, S, S, hd, False), ("dec.self_attn", B, H, L, L, hd, bool(cfg["rpr"])),
            ("dec.multihead_attn", B, H, L, S, hd, False)]


def gemm_kernel_and_epilogue(M, N, K, act=0):
    """(the library's route, activation and on the tiled kernels 'vector' / 'elementwise' stores) of `ops.linear_ex` (ldc = N, no residual)."""
    kernel = R.gemm_route(M, N, K, act)
    epi = {0: "none", 1: "relu", 2: "sigmoid"}[act]
    return kernel, epi if kernel == "skinny" else epi + (":vector" if R.vec_ok(N, N) else ":elementwise")


def routes(cfg, B, S, L):
    """{(pass, name): (kernel, epilogue)} of the GEMMs and {name: (kernel, head_dim, Er)} of the forward attentions of one training step."""
    g = {(ps, name): gemm_kernel_and_epilogue(M, N, K, act) for ps, name, M, N, K, act in products(cfg, B, S, L)}
    a = {name: (R.attn_route(b, H, Lq, Lk, hd, er), hd, er) for name, b, H, Lq, Lk, hd, er in attentions(cfg, B, S, L)}
    return g, a
