"""Case table, input builders and bounds of the regression-head forward parity tests: `get_feature` and `forward` of
`VideoRegression` for all thirteen regModels against `oracle.reg_oracle.forward` in float64 (test_reg_parity_host.py checks the table
on the CPU, test_reg_forward_parity_gpu.py runs it on the GPU).  Nothing here imports the model class or the HIP library: the state
dicts are built from the key lists below (both tests check them against the class), the weights are the procedural ones of
`video2music_amd.synthetic`, the inputs are drawn here.

Every case names the edge it exists for.  A case is regModel, d_model / d_hidden / total_vf_dim / B clips / S frames / n_layers.  What the
shape arithmetic of the head turns these into (restated in `derived`):
  dt_rank = ceil(d_model / 16)           the head reads the first 32 columns of `dbc` against a dt_proj weight zero-padded to 32 columns
  ldbc    = dt_rank + 2 d_state, up to a multiple of 4: the row stride the scan walks
  d_state = 16 (d_conv 4), or d_hidden (d_conv 8) for 'moemamba': the N = 16 scan works in 32-step chunks, the wide scan in 16-step ones
  expert width 2 d_model + 1, zero-padded to a multiple of 32
  Fpad    = total_vf_dim up to a multiple of 32

Error measure: max |got - ref64| / max(1, max |ref64|), taken separately over `get_feature`, the (note density, loudness) pair and the
instrument probabilities.  Bound per case and output: 8 x e32, e32 being the same measure of the oracle's float32 run on the CPU (ROUTE_GAP,
BOUND_FACTOR, CAP and SENSITIVITY are those of helpers_family_parity.py).
"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from oracle import reg_oracle as R
from video2music_amd import synthetic
from tests.helpers_family_parity import BOUND_FACTOR, CAP, ROUTE_GAP, SENSITIVITY, chosen, rel_err, route_gap       # noqa: F401 (re-exported)
from tests import launch_routes as LR

REG_MODELS = ("bimamba+", "bimamba", "mamba", "mamba+", "moe_bimamba+", "sharedmoe_bimamba+", "moemamba", "lstm", "bilstm", "gru", "bigru",
              "cnngru", "cnnbigru")
MAMBA = REG_MODELS[:7]
N_EXPERTS = 6
EMO_DIM = 6
INSTRUMENTS = 40
OUTPUTS = ("feature", "lnnd", "inst")
# With rows of mean square ~1 a norm eps of 1e-6 in place of 1e-5 moves the outputs by about 4e-6, the size of the bounds: no case could tell
# a wrong eps.  In the Mamba heads the input projection is scaled by NORM_GAIN, and in the LayerNorm heads ('bimamba' in the name) every
# norm gain and bias too, so that the rows the norms see have a mean square of ~3e-3: in the first layer of the RMSNorm stacks, whose
# residual stream no norm bounds, and in every layer of the LayerNorm heads.
NORM_GAIN = 0.05

RegCase = namedtuple("RegCase", "name rm d dh vf B S n_layers seed gemm edge")


def _c(rm, d, dh, vf, B, S, n_layers, seed, edge):
    name = f"{rm.replace('+', 'p')}_{d}_{dh}_{vf}_{B}x{S}_L{n_layers}"
    return RegCase(name, rm, d, dh, vf, B, S, n_layers, seed, frozenset({"skinny", "tile64"}), edge)


# seed: of the weights (seed) and of the inputs (seed + 1000).  The seeds listed are those whose mixture layers keep every row's 2nd-vs-3rd
# gate-logit gap above ROUTE_GAP and whose bounds stay under CAP (test_reg_parity_host.py); a seed that fails either is replaced here, never
# skipped at run time; so is a seed whose float32 run comes out luckier than four roundings of an output (`bound_floor`), which happens to
# the two numbers of the (note density, loudness) pair at B S = 1.  The claimed GEMM routes are the same in every case: the sigmoid of the instrument head keeps its product (N = 40)
# on the 64-tile kernel, as do the mixture layers' fused epilogues; every other product -- M down to 1, N from 2, K from 32 -- is skinny.
CASES = [
    # ---- N = 16 scans: dt rank against the 32 zero-padded dt_proj columns, ldbc, 32-step chunks, S below d_conv = 4 ----
    _c("bimamba+", 32, 64, 7, 2, 33, 1, 1101, "dt_rank 2, ldbc 34 -> 36; one semantic column + six emotions (Fpad 32 mostly padding); one step past a 32-step chunk; one layer"),
    _c("bimamba+", 64, 64, 37, 2, 1, 3, 1102, "dt_rank 4, ldbc 36; S = 1: the conv sees its own frame only, the backward branch equals the forward one's form; three layers"),
    _c("bimamba+", 256, 64, 37, 1, 3, 1, 1103, "dt_rank 16, ldbc 48; S = 3 below d_conv"),
    _c("bimamba+", 128, 256, 774, 2, 65, 3, 1104, "deployed widths (dt_rank 8, ldbc 40, 774 features: Fpad 800); two full chunks and one step"),
    _c("bimamba", 96, 64, 32, 3, 31, 2, 1105, "dt_rank 6, ldbc 38 -> 40; total_vf_dim 32: the padded in-projection is a plain copy; one step short of a chunk; B = 3"),
    _c("bimamba", 128, 32, 64, 2, 1, 1, 1106, "version 0 layer at S = 1; total_vf_dim 64; d_hidden 32"),
    _c("bimamba", 160, 96, 37, 1, 65, 2, 1107, "dt_rank 10, ldbc 42 -> 44; d_model 160 and d_hidden 96 are no powers of two"),
    _c("mamba", 256, 64, 774, 2, 32, 2, 1108, "dt_rank 16; exactly one 32-step chunk; 774 features"),
    _c("mamba", 64, 64, 37, 2, 1, 1, 1109, "one-directional stack at S = 1, one layer"),
    _c("mamba", 32, 64, 32, 3, 31, 3, 1110, "dt_rank 2 on the RMSNorm stack, B = 3, three layers"),
    _c("mamba+", 512, 64, 64, 1, 8, 1, 1111, "dt_rank 32: dt_proj fills all 32 columns of the padded weight, ldbc 64"),
    _c("mamba+", 96, 64, 7, 3, 3, 3, 1112, "dt_rank 6 with the Mamba+ gate; S = 3 below d_conv; total_vf_dim 7; B = 3"),
    _c("mamba+", 128, 64, 37, 1, 1, 2, 1113, "Mamba+ stack with one token"),
    # ---- 'moemamba': d_state = d_hidden, d_conv = 8, 16-step chunks of the wide scan ----
    _c("moemamba", 32, 16, 37, 2, 17, 2, 1201, "d_state 16: the N = 16 scan kernel with d_conv 8 inside the MoEMamba stack; ldbc 34 -> 36; B = 2"),
    _c("moemamba", 64, 32, 7, 1, 1, 1, 1202, "d_state 32 at S = 1: one token per mixture layer; ldbc 68"),
    _c("moemamba", 32, 128, 64, 2, 15, 1, 1203, "d_state 128, one step short of a 16-step chunk; ldbc 258 -> 260"),
    _c("moemamba", 32, 256, 37, 1, 33, 2, 1204, "d_state 256: ldbc 514 -> 516; two chunks and one step"),
    _c("moemamba", 96, 32, 37, 3, 5, 1, 1205, "S = 5 below d_conv 8; dt_rank 6, ldbc 70 -> 72; B = 3; expert width 193 -> 224"),
    _c("moemamba", 64, 128, 32, 2, 16, 2, 1206, "d_state 128, exactly one 16-step chunk; dt_rank 4, ldbc 260"),
    # ---- conv7 as seven GEMMs over clips laid end to end ----
    _c("cnngru", 64, 64, 37, 3, 1, 1, 1301, "conv7 at S = 1: six of seven taps read padding only; B = 3"),
    _c("cnngru", 32, 64, 7, 3, 6, 2, 1302, "conv7 at S = 6 < 7: no output row sees seven frames; B = 3"),
    _c("cnnbigru", 96, 64, 37, 3, 3, 1, 1303, "conv7 at S = 3: the three zero frames between clips are as long as the clips; half rows of 48"),
    _c("cnnbigru", 64, 64, 32, 3, 7, 3, 1304, "conv7 at S = 7: only the middle row sees seven frames; three layers"),
    _c("cnnbigru", 128, 64, 774, 3, 40, 2, 1305, "conv7 at S = 40, B = 3: 132 GEMM rows, two clip boundaries inside them"),
    # ---- recurrent heads: half rows of 32 and of 48 weights per thread ----
    _c("lstm", 64, 64, 37, 2, 77, 1, 1401, "half rows of 32 weights; one layer"),
    _c("lstm", 96, 64, 7, 1, 1, 3, 1402, "half rows of 48 (twelve float4s); S = 1; three layers"),
    _c("bilstm", 96, 64, 37, 2, 77, 3, 1403, "half rows of 48, both directions, layers 1 and 2 read 192 columns"),
    _c("bilstm", 64, 64, 64, 3, 1, 1, 1404, "S = 1: both directions see one frame; B = 3"),
    _c("gru", 96, 64, 37, 2, 77, 1, 1405, "GRU at half rows of 48"),
    _c("gru", 64, 64, 32, 1, 1, 3, 1806, "GRU with one token, three layers"),                 # 1406: lnnd bound at the floor
    _c("bigru", 64, 64, 37, 2, 77, 3, 1407, "bidirectional GRU at half rows of 32, three layers"),
    _c("bigru", 96, 64, 774, 2, 1, 1, 1408, "bidirectional GRU at S = 1, 774 features"),
    # ---- mixture layer in the FFN's place: expert widths 129 -> 160 and 257 -> 288 ----
    _c("moe_bimamba+", 64, 64, 37, 1, 1, 2, 2001, "expert width 129; one token per mixture layer"),       # 1501, 1601: lnnd bound within 2.5x of the floor
    _c("moe_bimamba+", 128, 64, 774, 2, 260, 1, 1502, "expert width 257; 520 tokens, 1040 routed rows over 6 experts: segments past one 128-row tile"),
    _c("sharedmoe_bimamba+", 128, 64, 37, 1, 1, 1, 1603, "expert width 257 with the shared expert; one token"),
    _c("sharedmoe_bimamba+", 64, 64, 32, 2, 260, 2, 1504, "expert width 129 with the shared expert; 520 tokens; two layers"),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


def model_kwargs(c):
    """Constructor arguments of `VideoRegression` for case `c`."""
    return dict(n_layers=c.n_layers, d_model=c.d, d_hidden=c.dh, total_vf_dim=c.vf, regModel=c.rm)


def derived(c):
    """The shape arithmetic of the head for case `c` (the module docstring's table)."""
    mamba = c.rm in MAMBA
    N = c.dh if c.rm == "moemamba" else 16
    R_ = math.ceil(c.d / 16)
    dirs = 2 if c.rm in ("bilstm", "bigru", "cnnbigru") else 1
    return dict(dt_rank=R_ if mamba else None, d_state=N if mamba else None, d_conv=(8 if c.rm == "moemamba" else 4) if mamba else None,
                ldbc=(R_ + 2 * N + 3) // 4 * 4 if mamba else None, chunk=(32 if N == 16 else 16) if mamba else None,
                expert_width=2 * c.d + 1 if "moe" in c.rm else None, Fpad=(c.vf + 31) // 32 * 32, dirs=dirs,
                feature_width=c.d * dirs, tokens=c.B * c.S)


# ---- state dicts by key list ---------------------------------------------------------------------------------------------------------
def named_shapes(regModel, n_layers, d_model, d_hidden, total_vf_dim, **_):
    """(name, shape) list of the state dict of `VideoRegression` built with these arguments."""
    d, dh, rm = d_model, d_hidden, regModel
    out = []

    def mamba(p, N, K):
        ed, R_ = 2 * d, math.ceil(d / 16)
        return [(p + "A_log", (ed, N)), (p + "D", (ed,)), (p + "in_proj.weight", (2 * ed, d)), (p + "in_proj.bias", (2 * ed,)),
                (p + "conv1d.weight", (ed, 1, K)), (p + "conv1d.bias", (ed,)), (p + "x_proj.weight", (R_ + 2 * N, ed)),
                (p + "dt_proj.weight", (ed, R_)), (p + "dt_proj.bias", (ed,)), (p + "out_proj.weight", (d, ed)), (p + "out_proj.bias", (d,))]

    def glu(p):
        w = 2 * d + 1
        return [(p + "linear1.weight", (w, d)), (p + "linear1.bias", (w,)), (p + "linear2.weight", (d, w)), (p + "linear2.bias", (d,)),
                (p + "gate.weight", (w, d)), (p + "gate.bias", (w,))]

    def moe(p, shared):
        o = []
        for e in range(N_EXPERTS):
            o += glu(p + f"experts.{e}.")
        o += [(p + "gate.weight", (N_EXPERTS, d)), (p + "gate.bias", (N_EXPERTS,))]
        return o + (glu(p + "shared_expert.") if shared else [])

    def ffn(p):
        return [(p + "0.weight", (dh, d)), (p + "0.bias", (dh,)), (p + "3.weight", (d, dh)), (p + "3.bias", (d,))]

    def norms(p, n):
        return [(p + f"norm{i}.{f}", (d,)) for i in range(1, n + 1) for f in ("weight", "bias")]

    if rm in ("lstm", "bilstm", "gru", "bigru", "cnngru", "cnnbigru"):
        gates, dirs = (4 if "lstm" in rm else 3), (2 if "bi" in rm else 1)
        pre = "model."
        if rm.startswith("cnn"):
            out += [("model.cnn.0.weight", (d, d, 7)), ("model.cnn.0.bias", (d,))]
            pre = "model.gru."
        for l in range(n_layers):
            for sfx in ("", "_reverse")[:dirs]:
                out += [(f"{pre}weight_ih_l{l}{sfx}", (gates * d, d if l == 0 else dirs * d)), (f"{pre}weight_hh_l{l}{sfx}", (gates * d, d)),
                        (f"{pre}bias_ih_l{l}{sfx}", (gates * d,)), (f"{pre}bias_hh_l{l}{sfx}", (gates * d,))]
    else:
        for l in range(n_layers):
            p = f"model.layers.{l}."
            if rm == "moemamba":
                out += mamba(p + "0.mixer.", dh, 8) + [(p + "0.norm.weight", (d,))] + moe(p + "1.moe_layer.", True) + [(p + "1.norm.weight", (d,))]
            elif rm in ("mamba", "mamba+"):
                out += mamba(p + "mixer.", 16, 4) + [(p + "norm.weight", (d,))]
            else:
                out += mamba(p + "mamba_forward.", 16, 4) + mamba(p + "mamba_backward.", 16, 4)
                if rm == "bimamba":
                    out += norms(p, 4) + ffn(p + "ffn1.") + ffn(p + "ffn2.")
                elif rm == "bimamba+":
                    out += norms(p, 3) + ffn(p + "ffn.")
                else:
                    out += norms(p, 3) + moe(p + "ffn.", rm == "sharedmoe_bimamba+")
    width = d * (2 if rm in ("bilstm", "bigru", "cnnbigru") else 1)
    return out + [("in_proj.0.weight", (d, total_vf_dim)), ("in_proj.0.bias", (d,)), ("regressor.weight", (2, width)), ("regressor.bias", (2,)),
                  ("classifier.0.weight", (INSTRUMENTS, width)), ("classifier.0.bias", (INSTRUMENTS,))]


@functools.lru_cache(maxsize=4)
def state_dict(name):
    """Seeded fp32 state dict of case `name` ({key: torch tensor})."""
    c = BY_NAME[name]
    sd = {k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(named_shapes(**model_kwargs(c)), seed=c.seed).items()}
    if c.rm in MAMBA:
        rms = "bimamba" not in c.rm
        for k in sd:
            if k.startswith("in_proj.0.") or ("norm" in k and not rms):
                sd[k] = sd[k] * NORM_GAIN
    return sd


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def inputs(name):
    """fp32 inputs of case `name`: semantic (B, S, total_vf_dim - 6) ~ N(0, 1), emotion (B, S, 6) softmax rows; every clip its own draw."""
    c = BY_NAME[name]
    rs = np.random.RandomState(c.seed + 1000)
    sem = rs.standard_normal((c.B, c.S, c.vf - EMO_DIM)).astype(np.float32)
    z = rs.standard_normal((c.B, c.S, EMO_DIM))
    e = np.exp(z - z.max(-1, keepdims=True))
    return dict(semantic=torch.from_numpy(sem), emotion=torch.from_numpy((e / e.sum(-1, keepdims=True)).astype(np.float32)))


def oracle_outputs(name, dtype, wrong=()):
    """`reg_oracle.forward` on the whole batch of case `name` in `dtype`: ({"feature", "lnnd", "inst"}, gate logits of every mixture layer)."""
    c = BY_NAME[name]
    f = inputs(name)
    col = {}
    with torch.no_grad():
        ln_nd, inst = R.forward(state_dict(name), f["semantic"], f["emotion"], collect=col, reg_model=c.rm, dtype=dtype, wrong=wrong)
    return dict(feature=col["feature"], lnnd=ln_nd, inst=inst), tuple(col["gates"])


@functools.lru_cache(maxsize=None)
def ref64(name):
    """Float64 outputs and gate logits of case `name`; computed once per process and never written to."""
    return oracle_outputs(name, torch.float64)


@functools.lru_cache(maxsize=None)
def ref32(name):
    """The float32 run, on one thread: the summation order of a threaded BLAS moves e32 by up to 2x from machine to machine, more where an
    output holds two numbers (B S = 1); the seeds of the table were checked against the one-thread figures."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return oracle_outputs(name, torch.float32)
    finally:
        torch.set_num_threads(n)


def errors(got, ref):
    """{output: max |got - ref| / max(1, max |ref|)}."""
    return {k: rel_err(got[k], ref[k]) for k in OUTPUTS}


def e32(name):
    return errors(ref32(name)[0], ref64(name)[0])


def bounds(name):
    return {k: BOUND_FACTOR * v for k, v in e32(name).items()}


FLOOR_ROUNDINGS = 4.0


def bound_floor(name):
    """{output: 4 x 2^-24 x max |ref64|}: four roundings of the largest value to float32.  A bound under it says more about the luck of
    the float32 oracle's few roundings (an output of two numbers can come out nearly exact) than about a kernel: such a seed is replaced."""
    return {k: FLOOR_ROUNDINGS * 2.0 ** -24 * float(ref64(name)[0][k].abs().max()) for k in OUTPUTS}


def n_mixture_layers(c):
    return c.n_layers if "moe" in c.rm else 0


# ---- what the forward issues ---------------------------------------------------------------------------------------------------------
def gemm_calls(c):
    """The GEMM launches of `forward` for case `c` as launch_routes.GemmCall rows.  act 0 / 1 / 2 / 3: plain, ReLU, sigmoid, SiLU epilogue;
    other: the products inside the fused mixture layer (silu-multiply, grouped expert rows), forms only the library's own callers set."""
    q = derived(c)
    d, M = c.d, c.B * c.S
    out = []
    g = lambda tag, M_, N, K, act=0, other=False: out.append(LR.GemmCall(tag, M_, N, K, act, other))

    def mamba(tag):
        g(tag + ".in_proj", M, 4 * d, d), g(tag + ".x_proj", M, q["ldbc"], 2 * d), g(tag + ".dt_proj", M, 2 * d, 32), g(tag + ".out_proj", M, d, 2 * d)

    def moe(tag, shared):
        w = (q["expert_width"] + 31) // 32 * 32
        g(tag + ".experts.up", 2 * M, w, d, other=True), g(tag + ".experts.gate", 2 * M, w, d, other=True), g(tag + ".experts.down", 2 * M, d, w, other=True)
        if shared:
            g(tag + ".shared.up", M, w, d, other=True), g(tag + ".shared.gate", M, w, d, other=True), g(tag + ".shared.down", M, d, w, other=True)

    g("in_proj", M, d, q["Fpad"])
    if c.rm.startswith("cnn"):
        for j in range(7):
            g(f"conv7.tap{j}", c.B * (c.S + 6) - 6, d, d, 3 if j == 6 else 0)
    for l in range(c.n_layers):
        t = f"layer{l}"
        if c.rm not in MAMBA:
            g(t + ".ih", M, q["dirs"] * (4 if "lstm" in c.rm else 3) * d, d if l == 0 else q["dirs"] * d)
        elif c.rm == "moemamba":
            mamba(t + ".mixer"), moe(t + ".moe", True)
        elif c.rm in ("mamba", "mamba+"):
            mamba(t + ".mixer")
        else:
            mamba(t + ".fwd"), mamba(t + ".bwd")
            if "moe" in c.rm:
                moe(t + ".ffn", c.rm == "sharedmoe_bimamba+")
            else:
                for f in (("ffn1", "ffn2") if c.rm == "bimamba" else ("ffn",)):
                    g(f"{t}.{f}.0", M, c.dh, d, 1), g(f"{t}.{f}.3", M, d, c.dh)
    g("regressor", M, 2, q["feature_width"]), g("classifier", M, INSTRUMENTS, q["feature_width"], 2)
    return out


def routes(c):
    """{GEMM tag: route} as the library's launcher answers (tests/launch_routes.py)."""
    return {q.name: LR.route_of(q) for q in gemm_calls(c)}


# ---- wrong variants for the sensitivity check ----------------------------------------------------------------------------------------
def wrong_variants(c):
    """[(variant of R.WRONG_VARIANTS that touches code case `c` runs, None or the reason it cannot change this case)]."""
    out = []
    if c.rm in MAMBA:
        out += [("conv_shifted_one_tap", None), ("no_Dx", None)]
        if c.rm.endswith("+"):
            out.append(("gate_sigmoid_z", None))
        if "bimamba" in c.rm:
            out += [("ln_eps_1e-6", None), ("backward_not_flipped_back", "a one-frame clip is its own flip" if c.S == 1 else None)]
        else:
            out.append(("rms_eps_1e-6", None))
        if c.rm == "bimamba":
            out.append(("ffn2_reads_xb", None))
    else:
        out.append(("lstm_forget_input_swapped" if "lstm" in c.rm else "gru_candidate_without_r", None))
        if c.rm.startswith("cnn"):
            out.append(("conv7_padding_2", None))
    return out
