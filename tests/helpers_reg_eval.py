"""Regression-evaluation test infrastructure: the miniature dataset's regression targets, the seeded inputs of the kernel tests,
an fp64 numpy restatement of what `amt_reg_metrics_fwd` computes, and the error bounds the tests hold it to."""
import os

import numpy as np

from tests.helpers_features import mini_dataset_content, write_mini_dataset

N_INST = 40
U = 2.0 ** -24                    # unit roundoff of fp32
FIELDS = ("sse_note_density", "sse_loudness", "bce_sum", "n_rows")
FIGURES = ("total_loss", "rmse_note_density", "rmse_loudness", "bce_instrument")      # the order eval_model returns them in

# the golden's two models: the reference's evaluation defaults, and the callers' default head at its usual size
MODELS = {"bilstm": dict(regModel="bilstm", d_model=64, n_layers=2, dim_feedforward=256),
          "bimamba+": dict(regModel="bimamba+", d_model=128, n_layers=2, dim_feedforward=256)}
LENGTHS = ((300, 300), (200, 300))          # (max_seq_chord, max_seq_video) pairs the reader is checked at


def reg_dataset_content(seed=29):
    """`mini_dataset_content` (clip "003": 40 s, so 260 padded rows are counted; clip "017": 320 s, cut at 300) plus seeded targets:
    note density in [0, 8) and loudness in [0, 4) to four decimals, instrument rows of 0s and 1s (about a quarter 1s)."""
    c = mini_dataset_content(seed=7)
    rng = np.random.default_rng(seed)
    for fid in c["ids"]:
        n = len(c[f"{fid}_chords"])
        c[f"{fid}_note_density"] = np.round(8 * rng.random(n), 4)
        c[f"{fid}_loudness"] = np.round(4 * rng.random(n), 4)
        c[f"{fid}_instrument"] = (rng.random((n, N_INST)) < 0.25).astype(np.int64)
    return c


def write_reg_dataset(root, c):
    """`write_mini_dataset(..., with_targets=True)`, then the three target files overwritten with the content's own."""
    write_mini_dataset(root, c, with_targets=True)
    for fid in c["ids"]:
        for sub, key in (("vevo_loudness", "loudness"), ("vevo_note_density", "note_density")):
            with open(os.path.join(root, sub, "origin", fid + ".lab"), "w") as f:
                f.write("".join(f"{t} {v:.4f}\n" for t, v in enumerate(c[f"{fid}_{key}"])))
        with open(os.path.join(root, "vevo_instrument", "thresholding", fid + ".csv"), "w") as f:
            f.write(",".join(f"inst{j}" for j in range(N_INST)) + "\n")
            f.write("".join(",".join(str(int(v)) for v in row) + "\n" for row in c[f"{fid}_instrument"]))


def content_of(g):
    """The dataset content recorded in g_reg_eval.npz."""
    c = {k[3:]: g[k] for k in g if k.startswith("in_")}
    c["ids"] = [str(i) for i in g["ids"]]
    return c


# ---- seeded inputs of the kernel tests (and of the CPU condition check on the same inputs) ----

KERNEL_CASES = [(B, S, W) for B in (1, 3) for S in (1, 5, 63, 64, 65, 300) for W in (8, 40, 128, 256)] + [(2, 5, 1024)]
Z_MAX = 6.0


def case_seed(B, S, W):
    return 100000 * B + 100 * S + W


def make_case(B, S, W, seed=None):
    """feat (B, S, W) ~ N(0, 1); regressor rows ~ N(0, 1 / W) with biases of a few units; classifier rows scaled so that the largest
    instrument logit (in fp64) is 5.9 at the most; note density in [0, 8), loudness in [0, 4), instrument 0 / 1.  All fp32."""
    rng = np.random.default_rng(case_seed(B, S, W) if seed is None else seed)
    feat = rng.standard_normal((B, S, W)).astype(np.float32)
    reg_w = (rng.standard_normal((2, W)) / np.sqrt(W)).astype(np.float32)
    reg_b = np.array([4.0, 2.0], dtype=np.float32) + rng.standard_normal(2).astype(np.float32)
    cls_w = (1.5 * rng.standard_normal((N_INST, W)) / np.sqrt(W)).astype(np.float32)
    cls_b = (0.5 * rng.standard_normal(N_INST)).astype(np.float32)
    z = np.abs(feat.astype(np.float64) @ cls_w.astype(np.float64).T + cls_b).max()
    if z > 5.9:
        cls_w, cls_b = (cls_w * np.float32(5.9 / z)).astype(np.float32), (cls_b * np.float32(5.9 / z)).astype(np.float32)
    return {"feat": feat, "reg_w": reg_w, "reg_b": reg_b, "cls_w": cls_w, "cls_b": cls_b,
            "note_density": np.round(8 * rng.random((B, S)), 3).astype(np.float32),
            "loudness": np.round(4 * rng.random((B, S)), 3).astype(np.float32),
            "instrument": (rng.random((B, S, N_INST)) < 0.3).astype(np.float32)}


def pack_heads(reg_w, reg_b, cls_w, cls_b):
    """The (W + 1, 64) layout `amt_reg_metrics_fwd` reads (include/amt_hip.h), built independently of `ops.pack_reg_heads`."""
    W = reg_w.shape[1]
    t = np.zeros((W + 1, 64), dtype=np.float32)
    for k in range(W):
        t[k, :N_INST], t[k, N_INST], t[k, N_INST + 1] = cls_w[:, k], reg_w[0, k], reg_w[1, k]
    t[W, :N_INST], t[W, N_INST:N_INST + 2] = cls_b, reg_b
    return t


# ---- fp64 restatement ----

def heads64(feat, reg_w, reg_b, cls_w, cls_b):
    """Both heads in fp64 from the fp32 inputs: ln_nd (..., 2), z (..., 40), and the head-value bound of every output,
    delta = (W + 2) 2^-24 (sum_k |x_k w_k| + |b|): W fused multiply-adds and the bias add in any order."""
    x = np.asarray(feat, dtype=np.float32).astype(np.float64)
    W = x.shape[-1]
    out = []
    for w, b in ((reg_w, reg_b), (cls_w, cls_b)):
        w, b = np.asarray(w, dtype=np.float32).astype(np.float64), np.asarray(b, dtype=np.float32).astype(np.float64)
        out += [x @ w.T + b, (W + 2) * U * (np.abs(x) @ np.abs(w).T + np.abs(b))]
    return {"ln_nd": out[0], "d_ln_nd": out[1], "z": out[2], "d_z": out[3]}


def prob32(z):
    """sigmoid of fp64 logits, rounded to fp32: the probability the reference's BCE sees."""
    with np.errstate(over="ignore"):
        return (1.0 / (1.0 + np.exp(-np.asarray(z, dtype=np.float64)))).astype(np.float32)


def bce_terms(p32, t):
    """torch's binary_cross_entropy on fp32 probabilities, the logs taken in fp64 and clamped at -100."""
    p, t = np.asarray(p32, dtype=np.float32).astype(np.float64), np.asarray(t, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return -(t * np.maximum(np.log(p), -100.0) + (1.0 - t) * np.maximum(np.log(1.0 - p), -100.0))


def sums(ln_nd, p32, note_density, loudness, instrument):
    """Per-row squared errors and BCE sums and the (B, 4) per-clip rows in the order of FIELDS, from head outputs (..., S, 2) /
    (..., S, 40) and the targets."""
    y = np.asarray(ln_nd).astype(np.float64)
    e = np.stack([y[..., 0] - np.asarray(note_density, dtype=np.float64), y[..., 1] - np.asarray(loudness, dtype=np.float64)], axis=-1)
    terms = bce_terms(p32, instrument)
    S = y.shape[-2]
    clip = np.stack([(e[..., 0] ** 2).sum(-1), (e[..., 1] ** 2).sum(-1), terms.sum((-1, -2)), np.full(y.shape[:-2], float(S))], axis=-1)
    return {"err": e, "terms": terms, "clip": clip}


def restate(feat, reg_w, reg_b, cls_w, cls_b, note_density, loudness, instrument):
    """The kernel restated: fp64 heads, p rounded to fp32, fp64 logs with the clamp, per-row and per-clip sums, and the bounds:

      squared-error sums   sum_rows (2 |e| delta + delta^2) + S 2^-24 sse
      BCE sum              sum_terms (delta + 4 2^-24 / min(p, 1 - p) + 4 2^-24 |term|) + S 2^-24 bce_sum

    delta the head-value bound of `heads64` (a logit's error reaches its term at a slope of 1 at the most); 4 2^-24 / min(p, 1 - p)
    covers the fp32 sigmoid (a few ulps of p) seen through the two logs; 4 2^-24 |term| the logs' own rounding, the products and the
    row's 40-term tree; the last part of each is the ordered fp32 sum over the clip's S rows.  A saturated p (0 or 1 in fp32) makes
    the BCE bound infinite: such rows are checked for exactness instead."""
    h = heads64(feat, reg_w, reg_b, cls_w, cls_b)
    p32 = prob32(h["z"])
    r = sums(h["ln_nd"], p32, note_density, loudness, instrument)
    S = h["z"].shape[-2]
    e, d = np.abs(r["err"]), h["d_ln_nd"]
    sse_bound = (2 * e * d + d * d).sum(-2) + S * U * r["clip"][..., :2]
    p = p32.astype(np.float64)
    with np.errstate(divide="ignore"):
        term_bound = h["d_z"] + 4 * U / np.minimum(p, 1 - p) + 4 * U * np.abs(r["terms"])
    bce_bound = term_bound.sum((-1, -2)) + S * U * r["clip"][..., 2]
    bound = np.concatenate([sse_bound, bce_bound[..., None], np.zeros_like(bce_bound)[..., None]], axis=-1)
    return dict(r, ln_nd=h["ln_nd"], d_ln_nd=h["d_ln_nd"], z=h["z"], d_z=h["d_z"], p32=p32, bound=bound)


def figures(clip):
    """(total_loss, rmse_note_density, rmse_loudness, bce_instrument) per clip from (B, 4) rows, as eval_model forms them at its
    batch size of 1 (utilities/run_model_regression.py:106-118)."""
    c = np.asarray(clip, dtype=np.float64)
    S = c[:, 3]
    bce = c[:, 2] / (N_INST * S)
    return np.stack([np.sqrt((c[:, 0] + c[:, 1]) / (2 * S)) + bce, np.sqrt(c[:, 0] / S), np.sqrt(c[:, 1] / S), bce], axis=1)
