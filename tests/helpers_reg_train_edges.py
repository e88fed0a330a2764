"""Case table, inputs, fp64 / fp32 oracles and bounds of the regression heads' training edge tests: one training step of
`VideoRegression` for the eight heads that train, at the shapes where the launch plan of a step changes
(tests/test_reg_train_edges_host.py checks the table on the CPU, tests/test_reg_train_edges_gpu.py runs it on the GPU).

A case is regModel, d_model / d_hidden / total_vf_dim / B clips / S frames / n_layers / seed, named for its edge.  Weights are the
procedural ones of `video2music_amd.synthetic` over `helpers_reg_parity.named_shapes`, inputs are drawn here, every dropout rate is 0.
The yardsticks are the existing restatements in double: `helpers_reg_train.model_grads64` (recurrent heads),
`helpers_reg_mamba_train.model_grads` ('bimamba+' / 'bimamba'), `helpers_moe_train.model_grads` (the mixture heads).

Bound of every gradient tensor: rel_err(got, g64) <= max(8 e32, rows U), rows = B S, e32 the error of the same restatement in fp32
on one CPU thread against the same fp64, U = 2^-24 -- the bound of tests/test_reg_*_train_gpu.py with e32 computed per case and
tensor.  An fp64 gradient that is exactly zero is exactly zero on the device.  ln_nd and p: max(8 e32, W U) of their largest value, W
the feature width.  The loss: what those two bounds move it by (SmoothL1's slope is at most 1; a BCE term moves by dp / min(p, 1 - p))
plus the roundings of the fused loss's own sums, `loss_adds` of them on the longest path, and 8 for the logarithms.

Conditioning, so that bounds made of rounding can hold (tests/helpers_train_edges.py's lesson): the biases of a feed-forward column
with a ReLU pre-activation within KINK x the layer's rms of 0 are moved (`clear_kinks`), a regression target whose residual lies
within SL1_MARGIN of +-1 is moved by 4 SL1_MARGIN (`batch`); the host test asserts the margins that result.

Measured by tests/test_reg_train_edges_host.py (fp64, CPU): every 8 e32 stays under `helpers_reg_parity.CAP` = 1e-4; the largest
bound of the table is the rows U floor of the two 4097-row cases, 2.44e-4.  The smallest err / bound of a wrong variant in a case
named for the edge it breaks is 352 (the in-projection's weight gradient over the first 1536 of 1540 rows, `bigru_rows1540`; 544 at
`bimambap_rows1540`); every other variant misses by more than 2900 bounds, or puts a nonzero where fp64 has an exact zero."""
import contextlib
import functools
import math
import re
from collections import namedtuple

import numpy as np
import torch

from tests import helpers_moe_train as M
from tests import helpers_reg_mamba_train as MB
from tests import helpers_reg_parity as P
from tests import helpers_reg_train as R
from tests import launch_routes as LR
from video2music_amd import ops, synthetic

U = R.U
GRAD_FACTOR = 8
KINK = 2.0 ** -14              # no ReLU pre-activation within KINK x its layer's rms of 0
SL1_MARGIN = 2.0 ** -12        # no SmoothL1 residual within this of +-1
P_MARGIN = 1e-6                # no probability within this of 0 or 1
CAP = P.CAP                    # no 8 e32 of the table above this; a bound above it is the rows U floor of a 4097-row case

RECURRENT, MAMBA, MIXTURE = ("lstm", "bilstm", "gru", "bigru"), ("bimamba+", "bimamba"), ("moe_bimamba+", "sharedmoe_bimamba+")
Case = namedtuple("Case", "name rm d dh vf B S n_layers seed edge")

# seed: of the weights (seed) and of the inputs (seed + 1000).  A seed whose mixture layers leave a gate gap under M.GAP, or which
# fails a conditioning margin, is replaced here, never skipped at run time.
_TABLE = [
    # ---- recurrent ----
    Case("lstm_one_row", "lstm", 96, 64, 37, 1, 1, 3, 3101, "one row: every weight-gradient K is 1 padded to 32; the weight_hh gradients are exact zeros"),
    Case("bilstm_half48", "bilstm", 96, 64, 37, 2, 77, 3, 3102, "half rows of 48 recurrent weights; layers 1 and 2 read 192 columns"),
    Case("gru_d128", "gru", 128, 64, 37, 3, 11, 1, 3103, "the hidden-size limit; B = 3; 33 rows pad to K = 64"),
    Case("bigru_rows1540", "bigru", 64, 64, 37, 7, 220, 2, 3104, "1540 rows: weight-gradient K above skinny_k, the data products still skinny"),
    Case("bilstm_rows4097", "bilstm", 32, 64, 37, 17, 241, 1, 3105, "4097 rows: above small_m, the data products leave the skinny GEMM too"),
    # ---- Mamba ----
    Case("bimambap_dt10", "bimamba+", 160, 96, 37, 1, 33, 1, 3201, "dt_rank 10, ldbc 42 -> 44, ED 320 = five conv channel blocks, one step past a scan chunk"),
    Case("bimamba_dt6", "bimamba", 96, 64, 32, 3, 31, 2, 3202, "dt_rank 6, ldbc 38 -> 40, B = 3, one step short of a chunk; total_vf_dim 32; two layers"),
    Case("bimambap_below_conv", "bimamba+", 256, 64, 37, 1, 3, 1, 3203, "dt_rank 16; S = 3 below d_conv"),
    Case("bimamba_one_step", "bimamba", 64, 64, 37, 2, 1, 1, 3204, "S = 1: one step per clip"),
    Case("bimambap_rows1540", "bimamba+", 32, 64, 774, 7, 220, 1, 3205, "1540 rows; Fpad 800"),
    Case("bimamba_rows4097", "bimamba", 32, 64, 37, 17, 241, 1, 3206, "4097 rows"),
    # ---- mixture ----
    Case("shared_split2", "sharedmoe_bimamba+", 32, 64, 37, 3, 235, 1, 3323, "705 tokens: the experts' weight gradients in S = 2 runs, the shared expert's in 6"),
    Case("moe_split3", "moe_bimamba+", 64, 64, 7, 3, 363, 1, 3314, "1089 tokens: S = 3, an expert with a single tile (two empty runs) beside one with five"),
    Case("moe_one_token", "moe_bimamba+", 128, 64, 37, 1, 1, 1, 3305, "expert width 257 -> 288; one token: four experts without a row"),
    Case("shared_two_layers", "sharedmoe_bimamba+", 64, 64, 37, 2, 65, 2, 3306, "two mixture layers, 130 tokens each"),
]
CASES = {c.name: c for c in _TABLE}
NAMES = list(CASES)


def family(c):
    return "recurrent" if c.rm in RECURRENT else "mamba" if c.rm in MAMBA else "mixture"


def model_kwargs(c):
    """Constructor arguments of `VideoRegression` for case `c` (every dropout rate 0; the experts' own is set by the GPU test)."""
    return dict(n_layers=c.n_layers, d_model=c.d, d_hidden=c.dh, total_vf_dim=c.vf, regModel=c.rm, dropout=0.0)


def derived(c):
    """helpers_reg_parity.derived (dt_rank, ldbc, chunk, expert width, Fpad, ...) of the case."""
    return P.derived(P.RegCase(c.name, c.rm, c.d, c.dh, c.vf, c.B, c.S, c.n_layers, c.seed, None, c.edge))


# ---- weights and inputs --------------------------------------------------------------------------------------------------------------
def _draw(c):
    rs = np.random.RandomState(c.seed + 1000)
    sem = rs.standard_normal((c.B, c.S, c.vf - P.EMO_DIM)).astype(np.float32)
    z = rs.standard_normal((c.B, c.S, P.EMO_DIM))
    e = np.exp(z - z.max(-1, keepdims=True))
    emo = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    nd, loud = (1.5 * rs.standard_normal((c.B, c.S))).astype(np.float32), (1.5 * rs.standard_normal((c.B, c.S))).astype(np.float32)
    inst = (rs.random_sample((c.B, c.S, P.INSTRUMENTS)) < 0.3).astype(np.float32)
    return sem, emo, nd, loud, inst


def ffn_bias_keys(c):
    """The first-Linear biases of the ReLU feed-forwards, in the order the forward reaches them ('bimamba+': ffn; 'bimamba': ffn1, ffn2)."""
    names = {"bimamba+": ("ffn",), "bimamba": ("ffn1", "ffn2")}.get(c.rm, ())
    return [f"model.layers.{i}.{f}.0.bias" for i in range(c.n_layers) for f in names]


def pre_relu(sd, c, dtype):
    """The feed-forward pre-activations of the restatement's forward, one (rows, d_hidden) float64 array per ReLU in forward order."""
    sem, emo = _draw(c)[:2]
    tap = []
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    with torch.no_grad():
        MB.model_forward({k: t(v) for k, v in sd.items()}, c.rm, c.n_layers, t(sem), t(emo), pre_relu=tap)
    return [z.reshape(-1, z.shape[-1]).double().numpy() for z in tap]


def clear_kinks(sd, c):
    """tests/helpers_train_edges.py's `clear_kinks` for the Mamba heads' feed-forwards: in forward order, the bias of every hidden
    column with a pre-activation within KINK x the layer's rms of 0 (fp64) moves by the smallest multiple of twice that margin which
    leaves the whole column clear."""
    for j, k in enumerate(ffn_bias_keys(c)):
        z = pre_relu(sd, c, torch.float64)[j]
        delta = KINK * float(np.sqrt((z * z).mean()))
        b = sd[k].copy()
        for col in np.nonzero(np.abs(z).min(axis=0) < delta)[0]:
            for step in (s * n * 2 * delta for n in range(1, 9) for s in (1, -1)):
                moved = float(np.float32(b[col] + step)) - float(b[col])
                if np.abs(z[:, col] + moved).min() >= delta:
                    b[col] = np.float32(b[col] + step)
                    break
            else:
                raise AssertionError(f"{c.name}: no clear position for column {col} of {k}")
        sd[k] = b
    return sd


def plain_state_dict(c):
    return synthetic.synthetic_state_dict(P.named_shapes(**model_kwargs(c)), seed=c.seed)


@functools.lru_cache(maxsize=None)
def state_dict(name):
    """The case's weights (numpy fp32; shared, read-only): the synthetic recipe, the feed-forward biases nudged by `clear_kinks`."""
    c = CASES[name]
    return clear_kinks(dict(plain_state_dict(c)), c)


def _grads(c, sd, data, dtype64=True, **kw):
    """The family's restatement on `data` = (sem, emo, note_density, loudness, instrument)."""
    if c.rm in RECURRENT:
        return R.model_grads64(sd, c.rm, c.n_layers, *data, dtype=np.float64 if dtype64 else np.float32, **kw)
    fn = MB.model_grads if c.rm in MAMBA else M.model_grads
    return fn(sd, c.rm, c.n_layers, *data, dtype=torch.float64 if dtype64 else torch.float32, **kw)


@functools.lru_cache(maxsize=None)
def batch(name):
    """(sem, emo, note_density, loudness, instrument) of the case, numpy fp32.  A target whose fp64 residual lies within SL1_MARGIN of
    +-1 is moved by 4 SL1_MARGIN (a handful of the 8194 values of the largest cases)."""
    c = CASES[name]
    sem, emo, nd, loud, inst = _draw(c)
    ln = _grads(c, state_dict(name), (sem, emo, nd, loud, inst))["ln_nd"].reshape(c.B, c.S, 2)
    for j, tgt in enumerate((nd, loud)):
        close = np.abs(np.abs(ln[..., j] - tgt.astype(np.float64)) - 1.0) < SL1_MARGIN
        tgt[close] += np.float32(4 * SL1_MARGIN)
    return sem, emo, nd, loud, inst


@functools.lru_cache(maxsize=None)
def reference(name):
    """fp64 and fp32 (one CPU thread) runs of the case's restatement, computed once and never written to:
    {o64, e32: {key: rel err of the fp32 gradient}, e32_ln, e32_p, l32}."""
    c, sd, data = CASES[name], state_dict(name), batch(name)
    o64 = _grads(c, sd, data)
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        o32 = _grads(c, sd, data, dtype64=False)
    finally:
        torch.set_num_threads(n)
    e32 = {k: (R.rel_err(o32["grads"][k], g) if np.abs(g).max() > 0 else float(np.abs(o32["grads"][k]).max())) for k, g in o64["grads"].items()}
    return {"o64": o64, "e32": e32, "e32_ln": R.rel_err(o32["ln_nd"], o64["ln_nd"]), "e32_p": R.rel_err(o32["p"], o64["p"]), "l32": float(o32["loss"])}


def rows(c):
    return c.B * c.S


def grad_bound(name, key):
    return max(GRAD_FACTOR * reference(name)["e32"][key], rows(CASES[name]) * U)


def output_bounds(name):
    """(relative bound of ln_nd, of p): max(8 e32, W U), W the width of the rows the two heads read."""
    r, W = reference(name), derived(CASES[name])["feature_width"]
    return max(GRAD_FACTOR * r["e32_ln"], W * U), max(GRAD_FACTOR * r["e32_p"], W * U)


def loss_adds(n_rows):
    """Additions on the longest path of the fused loss's sums (csrc/reg_loss.hip): a thread's 4 values, the 6 levels of a wave's
    tree, 16 wave sums, one sum per workgroup of 4096 instrument values."""
    return 4 + 6 + 16 + -(-40 * n_rows // 4096)


def loss_bound(name):
    c, o = CASES[name], reference(name)["o64"]
    b_ln, b_p = output_bounds(name)
    p = o["p"]
    return (b_ln * np.abs(o["ln_nd"]).max() + b_p * p.max() * float((1.0 / np.minimum(p, 1 - p)).mean())
            + (loss_adds(rows(c)) + 8) * U * abs(o["loss"]))


def grad_errors(got, name):
    """{key: err / bound}; an fp64 gradient that is exactly zero must be exactly zero (inf otherwise)."""
    out = {}
    for k, want in reference(name)["o64"]["grads"].items():
        g = np.asarray(got[k], dtype=np.float64)
        assert g.shape == want.shape, (k, g.shape, want.shape)
        if (g[want == 0.0] != 0.0).any():
            out[k] = float("inf")
        elif np.abs(want).max() == 0.0:
            out[k] = 0.0
        else:
            out[k] = R.rel_err(g, want) / grad_bound(name, k)
    return out


# ---- the mixture heads' plan ---------------------------------------------------------------------------------------------------------
def expert_splits(c, dense=False):
    """S of the mixture layers' weight-gradient products in this case, as the launcher answers."""
    w = (derived(c)["expert_width"] + 31) // 32 * 32
    return ops.moe_wgrad_splits(rows(c), c.d, w, M.N_EXPERTS, M.TOP_K, dense)


def layer_plans(name):
    """Per mixture layer: helpers_moe_train.split_plan of its fp64 routing at the case's S."""
    c = CASES[name]
    return [M.split_plan(r["idx"].numpy(), M.N_EXPERTS, expert_splits(c)) for r in reference(name)["o64"]["routing"]]


# ---- the dense products of a training step (video2music_amd/autograd.py) ----------------------------------------------------------------
Product = namedtuple("Product", "name kind M N K act")     # kind: fwd | dx (a data gradient) | dw (a weight gradient: K is the row count)


def _c32(n):
    return (n + 31) // 32 * 32


def products(rm, d, dh, vf, B, S, n_layers):
    """Every `ops.linear_ex` call of one forward + backward of `regression_train_loss` at dropout 0, written once per head family from
    autograd.py: LinearFn / SigmoidHeadFn (dx = mm_nt(dz, w^T), dw | db = mm_tn(dz, x, ones)), RnnLayerFn, MambaBlockFn.  The mixture
    layers' own products run inside amt_moe_train_fwd / amt_moe_bwd and are not listed."""
    M_, Mp, out = B * S, _c32(B * S), []
    add = lambda name, kind, m, n, k, act=0: out.append(Product(name, kind, m, n, k, act))

    def linear(tag, n_out, k_in, act=0, need_x=True, k_fwd=None):
        add(tag, "fwd", M_, n_out, k_fwd or k_in, act)
        if need_x:
            add(tag + ".dx", "dx", M_, k_in, _c32(n_out))
        add(tag + ".dw", "dw", n_out, (k_fwd or k_in) + 1, Mp)

    def mamba(tag):
        ED, Rk = 2 * d, math.ceil(d / 16)
        ld = (Rk + 32 + 3) // 4 * 4
        add(tag + ".in_proj", "fwd", M_, 2 * ED, d), add(tag + ".x_proj", "fwd", M_, ld, ED), add(tag + ".dt_proj", "fwd", M_, ED, 32)
        add(tag + ".out_proj", "fwd", M_, d, ED)
        add(tag + ".out_proj.dx", "dx", M_, ED, d), add(tag + ".out_proj.dw", "dw", d, ED + 1, Mp)
        add(tag + ".dt_proj.dx", "dx", M_, Rk, ED), add(tag + ".dt_proj.dw", "dw", ED, Rk + 1, Mp)
        add(tag + ".x_proj.dx", "dx", M_, ED, _c32(ld)), add(tag + ".x_proj.dw", "dw", ld, ED, Mp)
        add(tag + ".in_proj.dx", "dx", M_, d, 2 * ED), add(tag + ".in_proj.dw", "dw", 2 * ED, d + 1, Mp)

    linear("in_proj", d, vf, need_x=False, k_fwd=_c32(vf))
    width = d
    if rm in RECURRENT:
        gates, dirs = (4 if "lstm" in rm else 3), (2 if "bi" in rm else 1)
        width = dirs * d
        for l in range(n_layers):
            k_in, Rg = (d if l == 0 else dirs * d), gates * d
            add(f"rnn{l}.ih", "fwd", M_, dirs * Rg, k_in), add(f"rnn{l}.ih.dx", "dx", M_, k_in, dirs * Rg)
            add(f"rnn{l}.ih.dw", "dw", dirs * Rg, k_in + 1, Mp)
            for r in range(dirs):
                add(f"rnn{l}.hh{r}.dw", "dw", Rg, d + 1, Mp)
    else:
        for l in range(n_layers):
            mamba(f"layer{l}.fwd"), mamba(f"layer{l}.bwd")
            for f in {"bimamba+": ("ffn",), "bimamba": ("ffn1", "ffn2")}.get(rm, ()):
                linear(f"layer{l}.{f}.0", dh, d, act=1), linear(f"layer{l}.{f}.3", d, dh)
    linear("regressor", 2, width), linear("classifier", P.INSTRUMENTS, width, act=2)
    return out


def case_products(c):
    return products(c.rm, c.d, c.dh, c.vf, c.B, c.S, c.n_layers)


def routes(prods):
    """{(kind, route)} -> names, as the library's launcher answers for each product."""
    out = {}
    for q in prods:
        out.setdefault((q.kind, LR.gemm_route(q.M, q.N, q.K, q.act)), []).append(q.name)
    return out


# ---- wrong variants for the sensitivity check --------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _wrong_expert_runs(mode, S):
    """helpers_moe_train.expert with one run of every expert's weight gradient wrong: the rows of an expert arrive in segment order
    (ascending token), tiles per run = ceil(tiles / S); the last non-empty run's rows go through weights that are detached
    ("dropped": that run's partial is missing) or counted twice ("twice": 2 w - w.detach() has w's value and twice its gradient)."""
    orig = M.expert

    def expert(Pd, pre, x, mask_h=None):
        if re.search(r"\.experts\.\d+\.$", pre) is None:
            return orig(Pd, pre, x, mask_h)
        tiles = -(-x.shape[0] // M.TILE)
        per = -(-tiles // S)
        cut = (-(-tiles // per) - 1) * per * M.TILE                  # first row of the last non-empty run
        Pw = {k: ((v.detach() if mode == "dropped" else 2 * v - v.detach()) if k.startswith(pre) else v) for k, v in Pd.items()}
        part = lambda Q, sl: orig(Q, pre, x[sl], None if mask_h is None else mask_h[sl])
        return torch.cat([part(Pd, slice(0, cut)), part(Pw, slice(cut, None))])
    M.expert = expert
    try:
        yield
    finally:
        M.expert = orig


def _first_rows_only(c, sd, data, n=1536):
    """The in-projection's weight gradient summed over the first n rows only, the rest as they are: dL/d(in_proj output) per row is the
    gradient of a bias given per row (a (B, S, d) tensor in the bias's place broadcasts as the bias does)."""
    g = dict(reference(c.name)["o64"]["grads"])
    if c.rm in RECURRENT:
        col = {}
        _grads(c, sd, data, collect=col)
        d_x0, vf = col["d_x0"], col["vf"]
    else:
        per_row = dict(sd)
        per_row["in_proj.0.bias"] = np.broadcast_to(sd["in_proj.0.bias"], (c.B, c.S, c.d)).copy()
        d_x0 = _grads(c, per_row, data)["grads"]["in_proj.0.bias"].reshape(rows(c), c.d)
        vf = np.concatenate([data[0], data[1]], axis=-1).reshape(rows(c), -1).astype(np.float64)
    assert R.rel_err(d_x0.T @ vf, g["in_proj.0.weight"]) < 1e-12
    g["in_proj.0.weight"] = d_x0[:n].T @ vf[:n]
    return g


# variant: (what it breaks, the cases named for that edge)
VARIANTS = {
    "expert_last_run_dropped": ("an expert's weight gradient without its last run", ("shared_split2", "moe_split3")),
    "expert_run_twice": ("a run of an expert's weight gradient added twice", ("shared_split2", "moe_split3")),
    "wgrad_first_1536_rows": ("a weight gradient over the first 1536 rows only",
                              ("bigru_rows1540", "bilstm_rows4097", "bimambap_rows1540", "bimamba_rows4097")),
    "ddbc_dt_columns_zero": ("ddbc's first dt_rank columns left zero", ("bimambap_dt10", "bimamba_dt6", "bimambap_below_conv")),
    "reverse_conv_taps_unflipped": ("the reverse branch's conv taps unflipped", ("bimambap_dt10", "bimambap_below_conv", "bimamba_one_step")),
    "gru_hidden_n_without_r": ("the GRU n gate's hidden side without r", ("gru_d128", "bigru_rows1540")),
}


def variant_grads(name, variant):
    """The fp64 gradients of the case with the named error."""
    c, sd, data = CASES[name], state_dict(name), batch(name)
    if variant in ("expert_last_run_dropped", "expert_run_twice"):
        with _wrong_expert_runs(variant.split("_")[-1] if variant.endswith("dropped") else "twice", expert_splits(c)):
            return _grads(c, sd, data)["grads"]
    if variant == "wgrad_first_1536_rows":
        return _first_rows_only(c, sd, data)
    return _grads(c, sd, data, wrong=(variant,))["grads"]


def variant_miss(name, variant):
    """(largest err / bound over the tensors, the tensor) of a wrong variant against the case's fp64 gradients."""
    errs = grad_errors(variant_grads(name, variant), name)
    worst = max(errs, key=errs.get)
    return errs[worst], worst
