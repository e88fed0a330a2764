"""Case table, input builders and bounds of the family forward parity tests: the teacher-forced eval forward of
VideoMusicTransformer_V1 / _V2 / _V3 against `oracle.amt_oracle.forward_family` in float64 (test_family_parity_host.py checks the
table on the CPU, test_family_forward_parity_gpu.py runs it on the GPU).  Nothing here imports the model classes, and the HIP
library is asked for launch routes only (tests/launch_routes.py; no GPU): the state dicts are built from the key lists below (the
GPU test checks them against the classes), the weights and video features are the procedural ones of `video2music_amd.synthetic`.

Every case names the edge it exists for.  Shapes (d_model, heads, L chord positions, S frames, B clips):
  s1  128, 4 (head_dim 32),  L 300, S 300, B 2   every attention on the split-key kernel (Lk 300, 24 workgroups), for V3 through the
                                                 even / odd-head strides; three 128-row query blocks; 600 tokens per mixture layer
  s2  256, 4 (head_dim 64),  L 257, S 256, B 1   the cross-attention's Lk at the split-key threshold 256; a one-row last query block
                                                 and a ragged last key tile in the causal self-attention
  s3  256, 2 (head_dim 128), L 129, S 17,  B 3   128-row kernel at head_dim 128, a one-row second block; B = 3 through the raw views;
                                                 S below one key tile
  s4  128, 8 (head_dim 16),  L 33,  S 120, B 2   head_dim 16 in the attention and in diff_subln
  s5  128, 4 (head_dim 32),  L 1,   S 1,   B 1   one query, one key, one frame
  s6  512, 8 (head_dim 64),  L 40,  S 300, B 2   dim_feedforward 1024: plain products of up to 600 x 1024 = 614400 outputs on the
                                                 skinny GEMM next to the fused-epilogue ones (SiLU, silu-multiply, grouped experts) on
                                                 the 64-tile kernel; encoder and cross-attention on the split-key kernel, the decoder's
                                                 self-attention (Lk 40) on the 128-row kernel
Three layers (V2 / V3 then hold three GLU layers and no mixture; every V1 layer is a mixture), four for '1.3.3' / '1.3.4' so that
one mixture layer follows their three GLU layers.  dim_feedforward 192 (narrower than the 2 d_model of the V1 SiLU experts) except s6.

Error measure: max |got - ref64| / max(1, max |ref64|) over the whole logits tensor.  Bound per case: 8 x e32, e32 being the same
measure of the oracle run in float32 on the CPU; 8 is the project's factor for another summation order and a device exp a few ulps
wide (test_rnn_train_gpu.py, test_train_gpu.py).  A bound over CAP = 1e-4 (the fuzz's tolerance) would mean an ill-conditioned case.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle import amt_oracle as O
from video2music_amd import synthetic
from tests import launch_routes as R
from tests.helpers_ops_edges import AttnCase

ROUTE_GAP = 1e-5            # smallest relative 2nd-vs-3rd gate-logit gap a row may have (test_lockstep_parity_gpu.py)
BOUND_FACTOR = 8.0
CAP = 1e-4
SENSITIVITY = 10.0          # a wrong variant of the restatement must miss the case's bound by this factor
N_EXPERTS = 6
SCENE_OFFSET_MAX = 300
DROP_RATE = 0.3
RMS_GAIN = 0.1              # scale of every norm gain in the rms_norm=True cases (see state_dict)

Shape = namedtuple("Shape", "d H L S B dff attn gemm what")
SHAPES = {
    "s1": Shape(128, 4, 300, 300, 2, 192, dict(enc="splitk", self="splitk", cross="splitk"), {"skinny", "tile64"},
                "split-key kernel in every attention (Lk 300), three query blocks, 600 tokens per mixture layer"),
    "s2": Shape(256, 4, 257, 256, 1, 192, dict(enc="splitk", self="splitk", cross="splitk"), {"skinny", "tile64"},
                "Lk at the 256 threshold in the cross-attention; a one-row last query block and a ragged last key tile"),
    "s3": Shape(256, 2, 129, 17, 3, 192, dict(enc="rows128", self="rows128", cross="rows128"), {"skinny", "tile64"},
                "128-row kernel at head_dim 128; B = 3 through the raw views; S below one key tile"),
    "s4": Shape(128, 8, 33, 120, 2, 192, dict(enc="rows128", self="rows128", cross="rows128"), {"skinny", "tile64"},
                "head_dim 16 in the attention and in diff_subln"),
    "s5": Shape(128, 4, 1, 1, 1, 192, dict(enc="rows128", self="rows128", cross="rows128"), {"skinny", "tile64"},
                "one query, one key, one frame"),
    "s6": Shape(512, 8, 40, 300, 2, 1024, dict(enc="splitk", self="rows128", cross="splitk"), {"skinny", "tile64"},
                "dim_feedforward 1024: plain products up to 614400 outputs on the skinny GEMM, fused epilogues on the 64-tile kernel"),
}

FamilyCase = namedtuple("FamilyCase", "name version shape n_layers seed rms_norm chord_embed scene_embed mask drop edge")


def _c(version, shape, seed, what, rms_norm=False, chord_embed=False, scene_embed=False, mask=True, drop=False):
    tag = "v" + version.replace(".", "") + ("rms" if rms_norm else "") + ("ce" if chord_embed else "") + ("se" if scene_embed else "") \
        + ("nomask" if not mask else "") + ("drop" if drop else "")
    n_layers = 4 if version in ("1.3.3", "1.3.4") else 3
    return FamilyCase(f"{shape}_{tag}", version, shape, n_layers, seed, rms_norm, chord_embed, scene_embed, mask, drop,
                      f"{what}; {SHAPES[shape].what}")


# seed: of the weights (seed), the video features (seed + 1000) and the chord ids (seed + 2000).  The seeds listed are those whose
# mixture layers keep every row's 2nd-vs-3rd gate-logit gap above ROUTE_GAP and whose bound stays under CAP
# (test_family_parity_host.py); a seed that fails either is replaced here, never skipped at run time.
CASES = [
    # ---- s1: the split-key kernel, three query blocks, mixture segments over 128 rows ----
    _c("3.0", "s1", 101, "V3 decoder maps through the even / odd-head strides on the split-key kernel, rotary encoder with the 2 d_model cache"),
    _c("3.1", "s1", 102, "V3 differential attention in both stacks on the split-key kernel"),
    _c("3.2", "s1", 103, "V3 pre-norm on the split-key kernel"),
    _c("1.2", "s1", 104, "V1 RoPE by the substring rule, learned tables to their last row (300), shared SiLU mixtures of 600 tokens"),
    _c("1.1", "s1", 135, "V1 rms_norm=True, GLU mixtures of 600 tokens without a shared expert", rms_norm=True),     # 105, 115, 125: gaps of 1e-6 .. 9e-6
    _c("2.2", "s1", 106, "V2 dropTokenRate mask on 600 frames", drop=True),
    # ---- s2: the 256 threshold ----
    _c("3.1", "s2", 201, "V3 at head_dim 64: a one-row last block in (B, H, L, hd) viewed as (L, B, E)"),
    _c("1.2", "s2", 202, "V1 RoPE at head_dim 64, 257 of the 300 table rows"),
    _c("1.3.3", "s2", 203, "three GLU layers, then one shared SiLU mixture (2 d_model = 512 wide) after them"),
    _c("2.1", "s2", 204, "V2 '2.1': rotary, the top-k scheduler idle in eval"),
    # ---- s3: head_dim 128, B = 3 ----
    _c("3.0", "s3", 301, "V3 raw views with B = 3 at head_dim 128"),
    _c("3.1", "s3", 302, "V3 raw views with B = 3 in both stacks, 17 frames"),
    _c("3.2", "s3", 303, "V3 pre-norm with B = 3"),
    _c("2.0", "s3", 304, "V2 '2.0': learned tables, no rotary, scene offsets through the embedding", scene_embed=True),
    _c("1.0", "s3", 305, "V1 '1.0' rms_norm=True: SiLU mixtures without a shared expert", rms_norm=True),
    _c("1.3.4", "s3", 306, "three GLU layers, then one SiLU mixture without a shared expert"),
    # ---- s4: head_dim 16 ----
    _c("3.0", "s4", 401, "V3 diff_subln at head_dim 16"),
    _c("3.1", "s4", 402, "V3 diff_subln at head_dim 16 in both stacks"),
    _c("3.2", "s4", 403, "V3 pre-norm at head_dim 16"),
    _c("1.3.3", "s4", 404, "V1 '1.3.3' at head_dim 16"),
    _c("2.2", "s4", 405, "V2 chord ids through the frozen table", chord_embed=True),
    _c("1.3", "s4", 406, "V1 '1.3': shared GLU mixtures"),
    # ---- s5: 1 x 1 ----
    _c("3.2", "s5", 501, "V3 with one position: both softmax maps are [1], the views are trivial, lambda_init by depth still acts"),
    _c("1.3", "s5", 502, "V1 with one token per mixture layer"),
    _c("2.0", "s5", 503, "V2 '2.0' with one position"),
    # ---- s6: the wide model ----
    _c("2.1", "s6", 601, "V2 forward(mask=False) at d_model 512", mask=False),
    _c("1.1", "s6", 602, "V1 '1.1': GLU mixtures 1024 wide"),
    _c("1.0", "s6", 603, "V1 '1.0': SiLU mixtures 1024 wide"),
    _c("1.3.4", "s6", 604, "V1 '1.3.4': GLU layers 1024 wide, then a SiLU mixture"),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


def family_of(version):
    return "V" + version[0]


def model_kwargs(c):
    """Constructor arguments of the model class for case `c`."""
    s = SHAPES[c.shape]
    kw = dict(version_name=c.version, n_layers=c.n_layers, num_heads=s.H, d_model=s.d, dim_feedforward=s.dff, max_sequence_chord=300,
              max_sequence_video=300, total_vf_dim=synthetic.total_vf_dim(1) - int(c.scene_embed), scene_embed=c.scene_embed,
              chord_embed=c.chord_embed)
    if c.rms_norm:
        kw["rms_norm"] = True
    return kw


# ---- state dicts by key list ---------------------------------------------------------------------------------------------------------
def _layer_plan(version, i):
    """(attention kind of the encoder layer, of the decoder layer, feed-forward kind) of layer i: attention "mha" | "diff"; feed-forward
    "glu" or (expert kind, shared expert, balancing buffer)."""
    fam = version[0]
    if fam == "1":
        expert = "glu" if version in ("1.1", "1.3") else "silu"
        mix = (expert, version not in ("1.0", "1.1", "1.3.4"), False)
        return "mha", "mha", ("glu" if version in ("1.3.3", "1.3.4") and i < 3 else mix)
    if fam == "2":
        return "mha", "mha", ("glu" if i < 3 else ("glu", True, False))
    return ("mha" if version == "3.0" else "diff"), "diff", ("glu" if i < 3 else ("glu", True, True))


def named_shapes(version, n_layers, num_heads, d_model, dim_feedforward, total_vf_dim, max_sequence_chord=300, max_sequence_video=300,
                 rms_norm=False, chord_embed=False, scene_embed=False, **_):
    """(name, shape) list of the state dict of the reference's V1 / V2 / V3 class built with these arguments."""
    d, ff, hd = d_model, dim_feedforward, d_model // num_heads
    fam = version[0]
    layer_norm = fam == "2" or (fam == "1" and not rms_norm)
    learned_pos = O.family_plan(version)[0]
    out = [("embedding.weight", (159, d)), ("embedding_root.weight", (15, d)), ("embedding_attr.weight", (16, d)),
           ("Linear_vis.weight", (d, total_vf_dim)), ("Linear_vis.bias", (d,)), ("Linear_chord.weight", (d, d + 1)), ("Linear_chord.bias", (d,)),
           ("condition_linear.weight", (d, 1)), ("condition_linear.bias", (d,)), ("Wout.weight", (159, d)), ("Wout.bias", (159,))]
    if scene_embed:
        out.append(("scene_embedding.weight", (SCENE_OFFSET_MAX, d)))
    if chord_embed:
        out.append(("chord_embedding_model.weight", (159, d)))
    if learned_pos:
        out += [("positional_embedding.weight", (max_sequence_chord, d)), ("positional_embedding_video.weight", (max_sequence_video, d))]

    def attn(p, kind):
        if kind == "mha":
            return [(p + "in_proj_weight", (3 * d, d)), (p + "in_proj_bias", (3 * d,)), (p + "out_proj.weight", (d, d)), (p + "out_proj.bias", (d,))]
        return [(p + n, (hd,)) for n in ("lambda_q1", "lambda_k1", "lambda_q2", "lambda_k2", "subln.weight")] + \
               [(p + "q_proj.weight", (2 * d, d)), (p + "k_proj.weight", (2 * d, d)), (p + "v_proj.weight", (d, d)), (p + "out_proj.weight", (d, d))]

    def expert(p, kind):
        if kind == "glu":
            return [(p + "linear1.weight", (ff, d)), (p + "linear1.bias", (ff,)), (p + "linear2.weight", (d, ff)), (p + "linear2.bias", (d,)),
                    (p + "gate.weight", (ff, d)), (p + "gate.bias", (ff,))]
        return [(p + "0.weight", (2 * d, d)), (p + "0.bias", (2 * d,)), (p + "3.weight", (d, 2 * d)), (p + "3.bias", (d,))]

    def ffn(p, plan):
        if plan == "glu":
            return expert(p, "glu")
        kind, shared, balancing = plan
        o = [(p + "gate.weight", (N_EXPERTS, d)), (p + "gate.bias", (N_EXPERTS,))]
        for e in range(N_EXPERTS):
            o += expert(p + f"experts.{e}.", kind)
        if shared:
            o += expert(p + "shared_expert.", kind)
        if balancing:
            o.append((p + "bias", (N_EXPERTS, 1)))
        return o

    def norm(p):
        return [(p + "weight", (d,))] + ([(p + "bias", (d,))] if layer_norm else [])

    for stack in ("encoder", "decoder"):
        for i in range(n_layers):
            p = f"transformer.{stack}.layers.{i}."
            enc_attn, dec_attn, plan = _layer_plan(version, i)
            out += attn(p + "self_attn.", enc_attn if stack == "encoder" else dec_attn)
            if stack == "decoder":
                out += attn(p + "cross_attn.", dec_attn)
            out += ffn(p + "ff.", plan)
            for n in range(1, 3 if stack == "encoder" else 4):
                out += norm(p + f"norm{n}.")
        out += norm(f"transformer.{stack}.norm.")
    return out


@functools.lru_cache(maxsize=4)
def state_dict(name):
    """Seeded fp32 state dict of case `name` ({key: torch tensor})."""
    c = BY_NAME[name]
    sd = {k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(named_shapes(**dict(model_kwargs(c), version=c.version)), seed=c.seed).items()}
    if c.rms_norm:
        # With rows of mean square ~1 an RMSNorm eps of 1e-5 in place of 1e-6 moves the logits by ~5e-6, the size of the bound: the
        # case could not tell a wrong eps.  Norm gains of RMS_GAIN keep the rows the norms see at a mean square of ~1e-2, where it can.
        for k in sd:
            if "norm" in k and k.endswith(".weight"):
                sd[k] = sd[k] * RMS_GAIN
    return sd


def n_mixture_layers(c):
    return 2 * sum(1 for i in range(c.n_layers) if _layer_plan(c.version, i)[2] != "glu")


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def drop_seed(c):
    """torch.manual_seed value under which the model draws the case's dropTokenRate mask."""
    return c.seed + 3000


@functools.lru_cache(maxsize=4)
def inputs(name):
    """fp32 / int64 inputs of case `name`: ids (chord ids, used with chord_embed), root, attr (B, L) -- pads included --, the video
    features of `synthetic_features(B, n_frames=S)`, and `drop_keep` (B, S) = torch.rand(B, S) > DROP_RATE under drop_seed, or None."""
    c = BY_NAME[name]
    s = SHAPES[c.shape]
    f = {k: torch.from_numpy(v) for k, v in synthetic.synthetic_features(s.B, seed=c.seed + 1000, n_frames=s.S).items()}
    rs = np.random.RandomState(c.seed + 2000)
    f["ids"] = torch.from_numpy(rs.randint(0, 159, size=(s.B, s.L)))
    f["root"] = torch.from_numpy(rs.randint(0, 15, size=(s.B, s.L)))
    f["attr"] = torch.from_numpy(rs.randint(0, 16, size=(s.B, s.L)))
    f["drop_keep"] = (torch.rand(s.B, s.S, generator=torch.Generator().manual_seed(drop_seed(c))) > DROP_RATE) if c.drop else None
    return f


def oracle_logits(name, dtype, wrong=(), collect=None):
    """`forward_family` on the whole batch of case `name` in `dtype` (state dict and features cast): logits (B, L, 159)."""
    c = BY_NAME[name]
    sd = {k: v.to(dtype) for k, v in state_dict(name).items()}
    f = inputs(name)
    fl = lambda k: f[k].to(dtype)
    with torch.no_grad():
        return O.forward_family(sd, c.version, SHAPES[c.shape].H, f["ids"] if c.chord_embed else f["root"], f["attr"], fl("semantic"), fl("key"),
                                fl("scene_offset"), fl("motion"), fl("emotion"), max_seq_video=300, mask=c.mask, drop_keep=f["drop_keep"],
                                collect=collect, wrong=wrong)


@functools.lru_cache(maxsize=None)
def ref64(name):
    """(float64 logits, gate logits of every mixture layer) of case `name`; computed once per process and never written to."""
    gates = []
    y = oracle_logits(name, torch.float64, collect=gates)
    return y, tuple(gates)


@functools.lru_cache(maxsize=None)
def ref32(name):
    gates = []
    y = oracle_logits(name, torch.float32, collect=gates)
    return y, tuple(gates)


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / max(1.0, float(ref.abs().max())))


def worst(got, ref):
    """(b, l, chord) of the largest |got - ref|."""
    i = int((got.double() - ref.double()).abs().argmax())
    return tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape)))


def e32(name):
    return rel_err(ref32(name)[0], ref64(name)[0])


def bound(name):
    return BOUND_FACTOR * e32(name)


def route_gap(gates):
    """Smallest relative gap between the 2nd and 3rd gate logit over the rows of every mixture layer (inf without one)."""
    g = float("inf")
    for t in gates:
        s = t.sort(dim=-1, descending=True).values
        g = min(g, float(((s[..., 1] - s[..., 2]) / s.abs().max(dim=-1).values.clamp(min=1.0)).min()))
    return g


def chosen(gates):
    return [t.topk(2, dim=-1).indices for t in gates]


# ---- what the forward issues ---------------------------------------------------------------------------------------------------------
def attention_calls(c):
    """{"enc" | "self" | "cross": AttnCase} of the attention launches of case `c` (V3's two maps share B, H, Lq, Lk, hd)."""
    s = SHAPES[c.shape]
    hd = s.d // s.H
    mk = lambda Lq, Lk, causal: AttnCase(c.name, s.B, s.H, Lq, Lk, hd, causal, 1, "seq", 1, None, False, "")
    return dict(enc=mk(s.S, s.S, 0), self=mk(s.L, s.L, int(c.mask)), cross=mk(s.L, s.S, 0))


def gemm_calls(c):
    """The GEMM launches of the forward of case `c` as launch_routes.GemmCall rows.  act 0: plain epilogue (bias, residual), act 3: SiLU;
    other: a form only the library's own callers set (the silu-multiply of the GLU up branch, grouped / gathered expert rows)."""
    s = SHAPES[c.shape]
    d, hd = s.d, s.d // s.H
    pad32 = lambda n: (n + 31) // 32 * 32
    out = []
    g = lambda tag, M, N, K, act=0, other=False: out.append(R.GemmCall(tag, M, N, K, act, other))

    def attn(tag, kind, nq, nk):
        w = 2 * d if kind == "diff" else d
        g(tag + ".q", nq, w, d), g(tag + ".k", nk, w, d), g(tag + ".v", nk, d, d), g(tag + ".out", nq, d, d)

    def ffn(tag, plan, n):
        kind, shared, grouped = ("glu", True, False) if plan == "glu" else (plan[0], plan[1], True)
        dff = pad32(s.dff) if kind == "glu" else 2 * d
        silu = 0 if kind == "glu" else 3                         # the SiLU experts' one activation sits in their gate product
        if grouped:
            rows = 2 * n                                         # top-2 rows sorted by expert (plus the plan's per-expert tile padding)
            g(tag + ".experts.gate", rows, dff, d, silu, other=True), g(tag + ".experts.down", rows, d, dff, other=True)
            if kind == "glu":
                g(tag + ".experts.up", rows, dff, d, other=True)
        if shared:
            g(tag + ".gate", n, dff, d, silu), g(tag + ".down", n, d, dff)
            if kind == "glu":
                g(tag + ".up", n, dff, d, other=True)

    g("Linear_vis", s.S * s.B, d, pad32(synthetic.total_vf_dim(1)))
    for i in range(c.n_layers):
        enc_attn, dec_attn, plan = _layer_plan(c.version, i)
        attn(f"enc{i}.self", enc_attn, s.S * s.B, s.S * s.B), ffn(f"enc{i}.ff", plan, s.S * s.B)
        attn(f"dec{i}.self", dec_attn, s.L * s.B, s.L * s.B), attn(f"dec{i}.cross", dec_attn, s.L * s.B, s.S * s.B)
        ffn(f"dec{i}.ff", plan, s.L * s.B)
    g("Wout", s.B * s.L, 159, d)
    return out


def routes(c):
    """(attention kernels by call, set of GEMM routes) as the library's launchers answer (tests/launch_routes.py)."""
    return {k: R.attn_route(a.B, a.H, a.Lq, a.Lk, a.hd) for k, a in attention_calls(c).items()}, {R.route_of(q) for q in gemm_calls(c)}


# ---- wrong variants for the sensitivity check ----------------------------------------------------------------------------------------
def wrong_variants(c):
    """[(variant of O.WRONG_VARIANTS, None or the reason it cannot change this case)]."""
    s = SHAPES[c.shape]
    one = s.L == 1 and s.S == 1
    out = []
    if c.version[0] == "3":
        out = [("odd_heads_from_0", "with one key both softmax maps are [1]" if one else None),
               ("rope_dim_d_model", "position 0 is rotated by the identity whatever the cache" if one else None),
               ("transposed_output", "the (1, H, 1, hd) and (1, 1, E) layouts coincide" if one else None),
               ("lambda_init_depth0", None)]
    if c.version == "1.2":
        out.append(("no_rope", None))
    if c.rms_norm:
        out.append(("rms_eps_1e-5", None))
    return out
