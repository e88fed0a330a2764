"""Case tables, input builders and fp64 restatements of the operator edge tests (test_ops_edges_host.py on the CPU;
test_gemm_routes_gpu.py, test_attn_strided_gpu.py, test_moe_plan_gpu.py, test_ops_rowwise_gpu.py on the GPU).

The restatements are plain numpy / torch in float64, written from the contracts of include/amt_hip.h and from
oracle/amt_oracle.py; nothing here calls the library.  Every case names the route, kernel or plan edge it exists for
(`edge`): the routes are those of csrc/gemm_f32.hip, csrc/attn_prefill.hip and csrc/moe.hip at the boundaries of
tests/launch_routes.py, where test_ops_edges_host.py asks the library for the route of every GEMM and attention case.

Tolerances come from the project (2e-5: test_linear, test_cross_attention_prefill; 1e-6: test_moe_other_top_k_vs_oracle;
1e-4: fuzz_parity.py) or from a restatement of the arithmetic run here on the CPU -- never from the code under test.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from tests.launch_routes import vec_ok

SENTINEL = np.float32(-7.0e37)          # written everywhere an output buffer must stay untouched; compared as bits
GUARD = 64                              # floats in front of and behind every output buffer (keeps 16-byte alignment)
TOL = 2e-5                              # dense GEMM (act 0/1/2, K <= 2048) and attention: the bound of tests/test_ops_gpu.py


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def untouched(buf, written_mask):
    """True when every float of `buf` outside `written_mask` still holds the sentinel's bits."""
    return bool(np.all(bits(buf)[~written_mask] == bits(np.array([SENTINEL]))[0]))


# =====================================================================================================================
# A. dense GEMM routes and epilogues
# =====================================================================================================================
# entry "ex": amt_linear_ex_fwd, "plain": amt_linear_fwd.  dx/dw/dy/dr: leading dimension minus its natural width
# (K, K, N, N); xcol: column of a wider matrix at which x starts.  act: 0 none, 1 ReLU, 2 sigmoid, 3 SiLU.
GemmCase = namedtuple("GemmCase", "name entry M N K act bias resid dx dw dy dr xcol route vec edge")


def _g(name, M, N, K, act=0, bias=True, resid=False, dx=0, dw=0, dy=0, dr=0, xcol=0, entry="ex", route="tile64", edge=""):
    vec = route != "skinny" and vec_ok(N, N + dy, N + dr if resid else None)      # the skinny kernel has one element-wise epilogue
    return GemmCase(name, entry, M, N, K, act, bias, resid, dx, dw, dy, dr, xcol, route, vec, edge)


GEMM_CASES = [
    # ---- skinny route: act 0 / 1, K, M and M*N within the skinny boundaries ----
    _g("skinny_1x16x32", 1, 16, 32, route="skinny", edge="skinny GEMM, one row, one k-tile pair, one column tile"),
    _g("skinny_strided", 33, 159, 96, act=1, resid=True, dx=4, dw=8, dy=1, dr=3, xcol=8, route="skinny",
       edge="skinny GEMM through ldw (un-packed weights) with ldx, ldy, ldr all different from K / N, ragged row block and column tile"),
    _g("skinny_under_switch", 4096, 158, 64, entry="plain", route="skinny",
       edge="M*N = 647168, just under the route switch: the last shape on the skinny GEMM"),
    # ---- route-switch partners: the 64x64 tile ----
    _g("t64_over_switch", 4096, 159, 64, entry="plain", route="tile64",
       edge="M*N = 651264, just over the switch: 64-tile kernel, N % 4 != 0 so the element-wise epilogue, nk = 2"),
    _g("t64_over_small_m", 4097, 16, 64, entry="plain", route="tile64",
       edge="M = 4097, one row over the skinny limit: 64-tile kernel with a one-row last row tile, vector epilogue, 65 tiles (65 mod 8 = 1)"),
    # ---- 64-tile kernel because the activation or K excludes the skinny route ----
    _g("t64_sigmoid_nk1", 5, 40, 32, act=2, route="tile64", edge="sigmoid keeps a small product off the skinny route; nk = 1: the second prefetch stage re-reads k-tile 0"),
    _g("t64_silu_nk3", 70, 132, 96, act=3, route="tile64", edge="SiLU on the 64-tile kernel; odd nk = 3; 6 tiles, fewer than the 8 XCDs of the tile remap"),
    _g("t64_sigmoid_resid_elt", 130, 66, 64, act=2, resid=True, route="tile64", edge="sigmoid + residual, N % 4 != 0: element-wise epilogue of the 64-tile kernel"),
    _g("t64_silu_resid_elt", 130, 66, 64, act=3, resid=True, route="tile64", edge="SiLU + residual, N % 4 != 0: element-wise epilogue of the 64-tile kernel"),
    _g("t64_long_k", 15, 64, 1568, route="tile64", edge="K = 1568 > 1536 keeps 15 rows off the skinny route; nk = 49, odd"),
    _g("t64_wgrad_k9600", 96, 40, 9600, route="tile64", edge="the weight-gradient shape class of the autograd (K = 9600, nk = 300)"),
    # ---- each clause of vec_ok ----
    _g("vec_all_mult4", 130, 64, 64, act=3, resid=True, route="tile64", edge="vec_ok: every leading dimension a multiple of 4: vector epilogue through the LDS transpose"),
    _g("vec_ldy_odd", 130, 64, 64, act=3, resid=True, dy=2, route="tile64", edge="vec_ok clause ldc % 4: ldy = N + 2 falls back to the element-wise epilogue"),
    _g("vec_ldr_odd", 130, 64, 64, act=3, resid=True, dr=2, route="tile64", edge="vec_ok clause ldr % 4: ldr = N + 2 falls back to the element-wise epilogue"),
    _g("vec_padded", 130, 64, 64, act=3, resid=True, dy=4, dr=8, route="tile64", edge="vector epilogue with ldy = N + 4, ldr = N + 8: 16-byte stores must leave the padding columns alone"),
    # ---- 128x128 tile: K >= 2048 and at least 768 tiles ----
    _g("t128_vec", 3100, 4100, 2048, resid=True, route="tile128",
       edge="128-tile kernel, 25 x 33 = 825 tiles (825 mod 8 = 1 in the XCD remap), ragged last row and column tile, vector epilogue"),
    _g("t128_silu_elt", 3100, 4101, 2048, act=3, route="tile128", edge="128-tile kernel with N % 4 != 0: element-wise epilogue on the big tile, SiLU"),
]
GEMM_BY_NAME = {c.name: c for c in GEMM_CASES}


@functools.lru_cache(maxsize=None)
def gemm_inputs(name):
    """x ~ N(0,1) with row stride ldx behind a base offset of xcol floats, w ~ N(0, 1/K), bias and resid ~ N(0,1); padding columns hold other random numbers."""
    c = GEMM_BY_NAME[name]
    rs = np.random.RandomState((c.M * 7919 + c.N * 104729 + c.K * 31 + c.act * 5 + c.dx + 3 * c.dy + 7 * c.dr) % (2 ** 31))
    ldx, ldw, ldr = c.K + c.dx, c.K + c.dw, c.N + c.dr
    xbuf = rs.standard_normal(c.xcol + c.M * ldx).astype(np.float32)       # x[r][k] = xbuf[xcol + r * ldx + k]
    w = (rs.standard_normal((c.N, ldw)) * c.K ** -0.5).astype(np.float32)
    bias = rs.standard_normal(c.N).astype(np.float32) if c.bias else None
    resid = rs.standard_normal((c.M, ldr)).astype(np.float32) if c.resid else None
    return dict(xbuf=xbuf, w=w, bias=bias, resid=resid, ldx=ldx, ldw=ldw, ldr=ldr, ldy=c.N + c.dy)


def _act64(v, act):
    if act == 1:
        return np.maximum(v, 0.0)
    if act == 2:
        return 1.0 / (1.0 + np.exp(-v))
    if act == 3:
        return v / (1.0 + np.exp(-v))
    return v


def _gemm_operands(c, inp, rows=None):
    x = inp["xbuf"][c.xcol:].reshape(c.M, inp["ldx"])[:, :c.K]
    r = inp["resid"][:, :c.N] if c.resid else None
    if rows is not None:
        x, r = x[rows], (r[rows] if r is not None else None)
    return x, inp["w"][:, :c.K], inp["bias"], r


@functools.lru_cache(maxsize=None)
def gemm_ref64(name):
    """act(x w^T + bias (+ resid)) in float64 (include/amt_hip.h: amt_linear_ex_fwd)."""
    c = GEMM_BY_NAME[name]
    x, w, b, r = _gemm_operands(c, gemm_inputs(name))
    v = (torch.from_numpy(x).double() @ torch.from_numpy(w).double().t()).numpy()
    if b is not None:
        v = v + b.astype(np.float64)
    if r is not None:
        v = v + r.astype(np.float64)
    return _act64(v, c.act)


def gemm_ref32_torch(name):
    """The same in fp32 on the CPU with torch (the condition test: the inputs must not make fp32 itself miss the bound)."""
    c = GEMM_BY_NAME[name]
    x, w, b, r = _gemm_operands(c, gemm_inputs(name))
    v = torch.from_numpy(np.ascontiguousarray(x)) @ torch.from_numpy(np.ascontiguousarray(w)).t()
    if b is not None:
        v = v + torch.from_numpy(b)
    if r is not None:
        v = v + torch.from_numpy(np.ascontiguousarray(r))
    v = {0: lambda t: t, 1: torch.relu, 2: torch.sigmoid, 3: torch.nn.functional.silu}[c.act](v)
    return v.numpy()


def gemm_restatement_rows(c):
    """Rows on which the kernel-order restatement runs: all of them, or for the 128-tile cases the first and last 32 (a maximum
    over fewer rows can only be smaller, so the tolerance derived from it is never wider than one over all rows)."""
    return np.arange(c.M) if c.M <= 256 else np.concatenate([np.arange(32), np.arange(c.M - 32, c.M)])


def gemm_kernel_order_f32(name):
    """The kernel's summation restated in numpy: one fp32 accumulator per output, k ascending, bias and residual added in fp32,
    fp32 exp in the activation.  Returns (rows, values)."""
    c = GEMM_BY_NAME[name]
    rows = gemm_restatement_rows(c)
    x, w, b, r = _gemm_operands(c, gemm_inputs(name), rows)
    xt, wt = np.ascontiguousarray(x.T), np.ascontiguousarray(w.T)          # [K][rows], [K][N]
    acc = np.zeros((len(rows), c.N), dtype=np.float32)
    for k in range(c.K):
        acc += xt[k][:, None] * wt[k][None, :]                              # fp32 product, fp32 add (the fma keeps more, never less)
    if b is not None:
        acc = acc + b[None, :]
    if r is not None:
        acc = acc + r
    one = np.float32(1.0)
    if c.act == 1:
        acc = np.maximum(acc, np.float32(0))
    elif c.act == 2:
        acc = one / (one + np.exp(-acc, dtype=np.float32))
    elif c.act == 3:
        acc = acc / (one + np.exp(-acc, dtype=np.float32))
    return rows, acc.astype(np.float32)


@functools.lru_cache(maxsize=None)
def gemm_tol(name):
    """2e-5 where the project already holds these kernels to it (act 0/1/2, K <= 2048).  SiLU and K = 9600:
    max(2e-5, 4 x the error of the kernel-order fp32 restatement against fp64); the 4 covers __expf and the MFMA's pairing of two k
    per step.  Values printed by test_ops_edges_host.py::test_gemm_tolerances:
      t64_silu_nk3, t64_silu_resid_elt, vec_* : restatement error 1.1e-6 .. 1.3e-6 -> 2.0e-5 (the floor)
      t64_wgrad_k9600: restatement error 1.04e-5 -> 4.17e-5;   t128_silu_elt: 8.57e-6 (64 rows) -> 3.43e-5"""
    c = GEMM_BY_NAME[name]
    if c.act != 3 and c.K <= 2048:
        return TOL
    rows, v = gemm_kernel_order_f32(name)
    err = float(np.abs(v.astype(np.float64) - gemm_ref64(name)[rows]).max())
    return max(TOL, 4.0 * err)


# =====================================================================================================================
# B. amt_attn_fwd: strided, grouped, scaled
# =====================================================================================================================
# layout: seq (L,B,E) | clip (B,L,E) | v3e / v3o (q, k as (B,L,2H,hd) even / odd heads, v (B,Lk,H,hd), o (B,H,Lq,hd)) |
#         grp (q (B,Lq,H,hd), k, v (B,Lk,H/g,hd)) | pad (clip-major with row strides E + 8)
# qs: 0 -> q_scale = 0 (means 1), 1 -> hd^-0.5, 2 -> 0.37.  kernel: "splitk" | "rows128" (attn_prefill.hip: launch_hd)
AttnCase = namedtuple("AttnCase", "name B H Lq Lk hd causal qs layout g kernel spikes edge")
LAYOUTS = ("seq", "clip", "v3e", "v3o", "grp", "pad")
SPLITK_PAIRS = [(1, 300, 0, "one query row, 10 key tiles over the four waves"),
                (40, 300, 1, "causal: the first row block has one key tile, so three waves own none and merge with m = -inf"),
                (129, 256, 0, "Lk at the threshold 256; a last row block of one row"),
                (257, 257, 1, "causal, ragged last key tile and a one-row last block"),
                (77, 300, 1, "causal, last row block partly filled"),
                (300, 257, 1, "causal with Lq > Lk: rows past Lk see every key")]


def _attn_cases():
    out = []
    n = 0

    def add(B, H, Lq, Lk, hd, causal, kernel, what, layout=None, g=None, qs=None, spikes=False, name=None):
        nonlocal n
        layout = layout or LAYOUTS[n % len(LAYOUTS)]
        if qs is None:
            # q_scale = 0 (no scaling) only below head_dim 64: with q ~ 0.5 N(0,1) the unscaled scores at head_dim 64 / 128 reach +-16,
            # where fp32 itself is 7e-6 off on the CPU and the condition of test_ops_edges_host.py (a quarter of 2e-5) no longer holds
            qs = n % 3 if hd < 64 or n % 3 else 1 + (n // 3) % 2
        if layout == "grp":
            g = g or (2, 4, H)[(n // len(LAYOUTS)) % 3]
            if H % g:
                g = H
        else:
            g = 1
        name = name or f"{kernel}_hd{hd}_{Lq}x{Lk}{'c' if causal else ''}_{layout}{g if layout == 'grp' else ''}_qs{qs}"
        out.append(AttnCase(name, B, H, Lq, Lk, hd, causal, qs, layout, g, kernel, spikes, f"{kernel} kernel, {layout} layout: {what}"))
        n += 1

    for hd in (32, 64):                           # split-K kernel: hd 32 / 64, Lk >= 256, fewer than 512 workgroups of 128 rows
        for (Lq, Lk, causal, what) in SPLITK_PAIRS:
            add(2, 4, Lq, Lk, hd, causal, "splitk", what)
        n += 1                                    # shift the layout / scale cycle for the next head_dim
    for hd in (16, 128):                          # the same pairs where the head_dim keeps them on the 128-row kernel
        for (Lq, Lk, causal, what) in SPLITK_PAIRS:
            add(2 if hd == 16 else 1, 4, Lq, Lk, hd, causal, "rows128",
                f"the split-K pair ({Lq}, {Lk}){' causal' if causal else ''} at a head_dim that stays on the 128-row kernel")
        n += 1
    for (Lq, Lk, causal, what) in [(33, 31, 0, "short keys, Lk < one tile"), (130, 77, 0, "two row blocks, Lk < 256"),
                                   (77, 130, 1, "causal with Lk > Lq"), (1, 1, 0, "one query, one key")]:
        add(2, 4, Lq, Lk, 64, causal, "rows128", what)
    # layouts the cycle above has not paired with every head_dim / mask / scale (checked by test_ops_edges_host.py)
    add(1, 4, 40, 300, 32, 1, "splitk", "grouped heads with the causal mask and idle waves", layout="grp", g=2, qs=1)
    add(1, 4, 40, 300, 64, 1, "splitk", "one kv head for all query heads", layout="grp", g=4, qs=2)
    add(2, 2, 129, 256, 64, 0, "splitk", "V3 odd heads: base offset hd, head stride 2 hd", layout="v3o", qs=1)
    add(2, 2, 77, 300, 32, 1, "splitk", "V3 even heads, o as (B,H,Lq,hd)", layout="v3e", qs=1)
    add(1, 2, 130, 77, 16, 0, "rows128", "V3 odd heads at head_dim 16", layout="v3o", qs=0)
    add(1, 2, 33, 31, 128, 1, "rows128", "V3 even heads at head_dim 128", layout="v3e", qs=2)
    add(1, 4, 77, 130, 16, 1, "rows128", "grouped heads at head_dim 16", layout="grp", g=2, qs=0)
    add(1, 4, 33, 300, 128, 0, "rows128", "grouped heads at head_dim 128", layout="grp", g=4, qs=2)
    add(1, 2, 33, 31, 128, 0, "rows128", "seq-first at head_dim 128", layout="seq", qs=2)
    add(1, 2, 77, 130, 16, 1, "rows128", "padded rows at head_dim 16", layout="pad", qs=0)
    add(1, 2, 130, 77, 128, 1, "rows128", "padded rows at head_dim 128", layout="pad", qs=1)
    add(1, 2, 77, 130, 16, 0, "rows128", "clip-major at head_dim 16", layout="clip", qs=2)
    add(1, 2, 40, 300, 128, 1, "rows128", "clip-major at head_dim 128", layout="clip", qs=1)
    add(1, 2, 33, 31, 16, 0, "rows128", "seq-first at head_dim 16", layout="seq", qs=0)
    add(1, 2, 40, 300, 16, 1, "rows128", "V3 even heads at head_dim 16", layout="v3e", qs=1)
    add(1, 2, 129, 256, 128, 0, "rows128", "V3 odd heads at head_dim 128", layout="v3o", qs=2)
    # Lk >= 256 that stays on the 128-row kernel: the grid is 1 * 16 * 32 = 512, not below 512
    add(32, 16, 5, 257, 32, 1, "rows128", "Lk >= 256 with a grid of exactly 512 workgroups: stays on the 128-row kernel; kv_group 4",
        layout="grp", g=4, qs=1, name="rows128_hd32_biggrid")
    # rescale and merge in the split-K kernel
    add(1, 1, 32, 300, 64, 0, "splitk", "score spikes in key tiles 3, 9 and 0 (waves 3, 1, 0): per-wave rescale and the four-wave merge",
        layout="clip", qs=0, spikes=True, name="splitk_spikes")
    return out


ATTN_CASES = _attn_cases()
ATTN_BY_NAME = {c.name: c for c in ATTN_CASES}
QS_VALUES = lambda hd: (0.0, float(hd) ** -0.5, 0.37)


def attn_layout(c):
    """Element strides {q,k,v,o}: (base, bs, hs, ls) and buffer sizes in floats.  o always carries padding."""
    B, H, Lq, Lk, hd, g = c.B, c.H, c.Lq, c.Lk, c.hd, c.g
    E, Hk = H * hd, H // c.g
    lay = c.layout
    if lay == "seq":           # (L, B, E): strides (E, hd, B*E)
        q = (0, E, hd, B * E, Lq * B * E)
        k = v = (0, E, hd, B * E, Lk * B * E)
        Eo = E + 4
        o = (0, Eo, hd, B * Eo, Lq * B * Eo)
    elif lay in ("clip", "pad"):
        p = 8 if lay == "pad" else 0
        q = (0, Lq * (E + p), hd, E + p, B * Lq * (E + p))
        k = v = (0, Lk * (E + p), hd, E + p, B * Lk * (E + p))
        Eo = E + 4
        o = (0, Lq * Eo, hd, Eo, B * Lq * Eo)
    elif lay in ("v3e", "v3o"):
        base = hd if lay == "v3o" else 0
        q = (base, Lq * 2 * E, 2 * hd, 2 * E, B * Lq * 2 * E)
        k = (base, Lk * 2 * E, 2 * hd, 2 * E, B * Lk * 2 * E)
        v = (0, Lk * E, hd, E, B * Lk * E)
        o = (0, H * (Lq + 1) * hd, (Lq + 1) * hd, hd, B * H * (Lq + 1) * hd)      # (B,H,Lq,hd) with one padding row per head
    elif lay == "grp":
        Ek = Hk * hd
        q = (0, Lq * E, hd, E, B * Lq * E)
        k = v = (0, Lk * Ek, hd, Ek, B * Lk * Ek)
        Eo = E + 4
        o = (0, Lq * Eo, hd, Eo, B * Lq * Eo)
    else:
        raise ValueError(lay)
    return dict(q=q, k=k, v=v, o=o)


def _index(base, bs, hs, ls, B, H, L, hd):
    b, h, l, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(L), np.arange(hd), indexing="ij")
    return base + b * bs + h * hs + l * ls + c


@functools.lru_cache(maxsize=None)
def attn_inputs(name):
    """Flat fp32 buffers (every float random: what the strides skip is noise, not zeros), q scaled by 0.5 as in
    test_cross_attention_prefill, and the 12 strides amt_attn_fwd takes."""
    c = ATTN_BY_NAME[name]
    rs = np.random.RandomState((c.Lq * 7 + c.Lk + 1000 * c.hd + 31 * LAYOUTS.index(c.layout) + c.qs) % (2 ** 31))
    lay = attn_layout(c)
    bufs = {}
    for t, amp in (("q", 0.5), ("k", 1.0), ("v", 1.0)):
        bufs[t] = (rs.standard_normal(lay[t][4]) * amp).astype(np.float32)
    if c.spikes:                # as test_softmax_rescale_branch_forced, at Lk = 300: smaller inputs, three spikes
        for t in ("q", "k"):
            bufs[t] *= np.float32(0.3 / (0.5 if t == "q" else 1.0))
        qi = _index(*lay["q"][:4], c.B, c.H, c.Lq, c.hd)
        ki = _index(*lay["k"][:4], c.B, c.H // c.g, c.Lk, c.hd)
        for (key, row, amp) in ((100, 7, 40.0), (290, 20, 25.0), (3, 12, 25.0)):
            bufs["k"][ki[0, 0, key]] = bufs["q"][qi[0, 0, row]] * np.float32(amp)
    strides = [lay[t][i] for t in ("q", "k", "v", "o") for i in (1, 2, 3)]
    return dict(bufs=bufs, strides=strides, lay=lay, q_scale=QS_VALUES(c.hd)[c.qs])


def attn_o_index(c):
    lay = attn_layout(c)
    return _index(*lay["o"][:4], c.B, c.H, c.Lq, c.hd), lay["o"][4]


def _attn_restate(c, inp, dtype):
    lay, bufs = inp["lay"], inp["bufs"]
    Hk = c.H // c.g
    q = torch.from_numpy(bufs["q"][_index(*lay["q"][:4], c.B, c.H, c.Lq, c.hd)]).to(dtype)
    k = torch.from_numpy(bufs["k"][_index(*lay["k"][:4], c.B, Hk, c.Lk, c.hd)]).to(dtype)
    v = torch.from_numpy(bufs["v"][_index(*lay["v"][:4], c.B, Hk, c.Lk, c.hd)]).to(dtype)
    k, v = k.repeat_interleave(c.g, dim=1), v.repeat_interleave(c.g, dim=1)      # query head h reads kv head h // g
    qs = inp["q_scale"] or 1.0
    s = (q * torch.tensor(np.float32(qs)).to(dtype)) @ k.transpose(-1, -2)
    if c.causal:                # key j visible to query i iff j <= i (top-left aligned)
        s = s + torch.triu(torch.full((c.Lq, c.Lk), float("-inf"), dtype=dtype), diagonal=1)
    return (torch.softmax(s, -1) @ v).numpy()                # (B, H, Lq, hd)


@functools.lru_cache(maxsize=None)
def attn_ref64(name):
    return _attn_restate(ATTN_BY_NAME[name], attn_inputs(name), torch.float64)


def attn_ref32_torch(name):
    return _attn_restate(ATTN_BY_NAME[name], attn_inputs(name), torch.float32)


# =====================================================================================================================
# C. MoE with steered routing
# =====================================================================================================================
# routing: (n_tok, k) expert ids, largest logit first.  tie: a pair of experts with identical gate rows and biases.
MoeCase = namedtuple("MoeCase", "name n_tok d dff n_exp k chosen shared glu gate_b tie edge")


def _route_all(n_tok, pair):
    return np.tile(np.asarray(pair, dtype=np.int64), (n_tok, 1))


def _route_counts(pairs_counts):
    rows = []
    for pair, n in pairs_counts:
        rows += [pair] * n
    return np.asarray(rows, dtype=np.int64)


def _route_mixed(n_tok, n_exp, k):
    """Token t starts at expert t % n_exp and steps on by 1 + t % 3 (ids made distinct): every expert is used, in both slot orders."""
    out = np.zeros((n_tok, k), dtype=np.int64)
    for t in range(n_tok):
        seen = []
        for j in range(k):
            e = (t + j * (1 + t % 3)) % n_exp
            while e in seen:
                e = (e + 1) % n_exp
            seen.append(e)
        out[t] = seen
    return out


def _route_perm(n_tok, n_exp, seed):
    rs = np.random.RandomState(seed)
    return np.stack([rs.permutation(n_exp) for _ in range(n_tok)]).astype(np.int64)


def _m(name, chosen, edge, d=128, dff=192, n_exp=8, shared=False, glu=True, gate_b=True, tie=None):
    chosen = np.asarray(chosen, dtype=np.int64)
    return MoeCase(name, chosen.shape[0], d, dff, n_exp, chosen.shape[1], chosen, shared, glu, gate_b, tie, edge)


MOE_CASES = [
    _m("full_two_segments", _route_all(128, (0, 1)), "two exactly full 128-row segments, six empty experts", shared=True),
    _m("full_plus_one", _route_all(129, (1, 0)), "129 rows per expert: a second tile of one row; slot order (1, 0) against expert order"),
    _m("full_plus_one_shared", _route_all(129, (0, 1)), "the same with the shared expert", shared=True),
    _m("full_plus_one_lsl", _route_all(129, (0, 1)), "the same with Linear-SiLU-Linear experts (w1 = null)", glu=False),
    _m("full_plus_one_lsl_shared", _route_all(129, (1, 0)), "Linear-SiLU-Linear experts with the shared expert", glu=False, shared=True),
    _m("one_token", _route_all(1, (6, 2)), "n_tok = 1: two one-row segments"),
    # the issue's counts {127, 1, 0, 132, 0, 0, 0, 0} need 132 tokens on expert 3, and a token holds an expert once: n_tok = 132,
    # the four assignments that are left go to expert 7
    _m("ragged_counts", _route_counts([((3, 0), 127), ((1, 3), 1), ((3, 7), 4)]),
       "per-expert counts {127, 1, 0, 132, 0, 0, 0, 4}: one row short of full, a single row, an empty expert between, full plus four", shared=True),
    _m("ragged_counts_other", _route_counts([((5, 2), 100), ((2, 6), 32)]),
       "the same shape with counts {0, 0, 132, 0, 0, 100, 32, 0}: the second call on ragged_counts' scratch must see re-zeroed counts", shared=True),
    _m("experts_63_and_0", _route_all(70, (63, 0)), "the last of 64 experts (and the first), 62 empty experts", n_exp=64),
    _m("five_experts", _route_mixed(37, 5, 2), "n_exp = 5: the router's 8-wide pass clamps three surplus slots; expert 4 of 5", n_exp=5, shared=True),
    _m("two_experts", _route_mixed(37, 2, 2), "n_exp = 2: every token on both experts", n_exp=2),
    _m("narrow_d32", _route_mixed(37, 8, 2), "d = 32, dff = 96: 8 router lanes busy, one k-tile in the gate product", d=32, dff=96, glu=True),
    _m("d288", _route_mixed(37, 8, 2), "d = 288: a router chunk of 256 columns plus a partly filled one", d=288, shared=True, glu=False),
    _m("no_gate_bias", _route_mixed(37, 8, 2), "gate_b = null", gate_b=False),
    _m("tie_top2", _route_all(9, (2, 5)), "experts 2 and 5 share their gate row and bias: bit-equal logits, lower id first", tie=(2, 5)),
    # amt_moe_topk_fwd, n_exp = 8
    _m("topk1_one_expert", _route_all(300, (5,)), "k = 1, 300 tokens on expert 5: three tiles (128, 128, 44) and seven empty experts"),
    _m("topk8_all", _route_perm(20, 8, 3), "k = 8: every token on every expert, each in its own order", shared=True),
    _m("topk3", _route_mixed(50, 8, 3), "k = 3", shared=True, glu=False),
    _m("tie_topk3", np.tile(np.asarray([[1, 6, 4]], dtype=np.int64), (9, 1)), "k = 3 router with experts 1 and 6 tied at the top: lower id first", tie=(1, 6)),
]
MOE_BY_NAME = {c.name: c for c in MOE_CASES}


@functools.lru_cache(maxsize=None)
def moe_inputs(name):
    """Steered tokens and weights.  Token t holds k, k-1, .., 1 at its chosen experts' coordinates (0 at the other experts'), N(0,1)
    behind them; gate_w[e, e] = 8, the rest of a gate row N(0, 1e-4); expert weights N(0, 1/fan_in).  With a tie (a, b) expert b
    copies expert a's gate row and bias, and the token's step for b is left out: a and b then see the same logit, bit for bit."""
    c = MOE_BY_NAME[name]
    rs = np.random.RandomState((c.n_tok * 13 + c.d * 7 + c.n_exp * 3 + c.k) % (2 ** 31))
    x = rs.standard_normal((c.n_tok, c.d)).astype(np.float32)
    x[:, :c.n_exp] = 0.0
    for j in range(c.k):
        x[np.arange(c.n_tok), c.chosen[:, j]] = c.k - j
    gate_w = (rs.standard_normal((c.n_exp, c.d)) * 1e-2).astype(np.float32)
    gate_w[np.arange(c.n_exp), np.arange(c.n_exp)] = 8.0
    gate_b = (rs.standard_normal(c.n_exp) * 1e-2).astype(np.float32) if c.gate_b else None
    if c.tie:
        a, b = c.tie
        x[:, b] = 0.0                                        # b's logit comes from a's coordinate through the shared row
        gate_w[b] = gate_w[a]
        if gate_b is not None:
            gate_b[b] = gate_b[a]

    def lin(*shape):
        return (rs.standard_normal(shape) * shape[-1] ** -0.5).astype(np.float32)

    def expert_set(n):
        small = lambda *s: (rs.standard_normal(s) * 0.1).astype(np.float32)
        return dict(w1=lin(n, c.dff, c.d) if c.glu else None, b1=small(n, c.dff) if c.glu else None,
                    wg=lin(n, c.dff, c.d), bg=small(n, c.dff), w2=lin(n, c.d, c.dff), b2=small(n, c.d))

    return dict(x=x, gate_w=gate_w, gate_b=gate_b, experts=expert_set(c.n_exp), shared=expert_set(1) if c.shared else None)


def expert_apply(x, w, e, dtype):
    """GLUExpert (oracle.glu_expert): W2((W1 x + b1) * silu(Wg x + bg)) + b2; w1 = null: W2 silu(Wg x + bg) + b2."""
    T = lambda a: torch.from_numpy(a[e]).to(dtype)
    x = torch.as_tensor(x).to(dtype)
    g = torch.nn.functional.silu(x @ T(w["wg"]).t() + T(w["bg"]))
    h = (x @ T(w["w1"]).t() + T(w["b1"])) * g if w["w1"] is not None else g
    return h @ T(w["w2"]).t() + T(w["b2"])


def moe_logits64(inp):
    lg = inp["x"].astype(np.float64) @ inp["gate_w"].astype(np.float64).T
    return lg + inp["gate_b"].astype(np.float64) if inp["gate_b"] is not None else lg


def moe_weights64(name):
    """softmax over the k chosen logits in fp64 (moe.py:190,288)."""
    c = MOE_BY_NAME[name]
    lg = np.take_along_axis(moe_logits64(moe_inputs(name)), c.chosen, axis=1)
    e = np.exp(lg - lg.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def _moe_restate(name, dtype):
    """moe.py's sum with the steered routing: experts in index order, out[tok] += w_e * expert_e(x[tok]); shared expert / k."""
    c, inp = MOE_BY_NAME[name], moe_inputs(name)
    wts = torch.from_numpy(moe_weights64(name)).to(dtype)
    idx = torch.from_numpy(c.chosen)
    x = torch.from_numpy(inp["x"]).to(dtype)
    out = torch.zeros(c.n_tok, c.d, dtype=dtype)
    for e in range(c.n_exp):
        sel = idx == e
        tok = sel.any(-1)
        if not tok.any():
            continue
        we = (wts * sel).sum(-1)[tok]
        out[tok] += we.unsqueeze(-1) * expert_apply(x[tok], inp["experts"], e, dtype)
    if c.shared:
        out = out + (1.0 / c.k) * expert_apply(x, inp["shared"], 0, dtype)
    return out.numpy()


@functools.lru_cache(maxsize=None)
def moe_ref64(name):
    return _moe_restate(name, torch.float64)


MOE_TOL_CAP = 1e-4


@functools.lru_cache(maxsize=None)
def moe_tol(name):
    """max(2e-5, 8 x the CPU fp32 restatement's error against fp64) on the same inputs and routing; never above 1e-4."""
    err = float(np.abs(_moe_restate(name, torch.float32).astype(np.float64) - moe_ref64(name)).max())
    return max(TOL, 8.0 * err), err


def plan_counts(chosen, n_exp):
    return np.bincount(np.asarray(chosen).reshape(-1), minlength=n_exp)


# pieces ------------------------------------------------------------------------------------------------------------------
GLU_PIECES = [(n, d, dff, glu) for n in (1, 129) for (d, dff) in ((32, 96), (128, 192)) for glu in (True, False)]


@functools.lru_cache(maxsize=None)
def glu_piece_inputs(n, d, dff, glu):
    rs = np.random.RandomState(n * 1000 + d + dff + int(glu))
    lin = lambda *s: (rs.standard_normal(s) * s[-1] ** -0.5).astype(np.float32)
    w = dict(w1=lin(1, dff, d) if glu else None, b1=(rs.standard_normal((1, dff)) * 0.1).astype(np.float32) if glu else None,
             wg=lin(1, dff, d), bg=(rs.standard_normal((1, dff)) * 0.1).astype(np.float32),
             w2=lin(1, d, dff), b2=(rs.standard_normal((1, d)) * 0.1).astype(np.float32))
    return rs.standard_normal((n, d)).astype(np.float32), w


def glu_piece_tol(n, d, dff, glu):
    x, w = glu_piece_inputs(n, d, dff, glu)
    r64 = expert_apply(x, w, 0, torch.float64).numpy()
    err = float(np.abs(expert_apply(x, w, 0, torch.float32).numpy().astype(np.float64) - r64).max())
    return max(TOL, 8.0 * err), err, r64


EP_RECV_COUNTS = np.asarray([[129, 0], [3, 64]], dtype=np.int32)      # [world = 2][e_local = 2]


def ep_expert_of_row(recv_counts):
    """Local expert of every arrival row: rows arrive grouped by (source rank, local expert)."""
    out = []
    for s in range(recv_counts.shape[0]):
        for j in range(recv_counts.shape[1]):
            out += [j] * int(recv_counts[s, j])
    return np.asarray(out, dtype=np.int64)


# =====================================================================================================================
# D. row-wise entry points
# =====================================================================================================================
NORM_SHAPES = [(rows, dim) for rows in (1, 5) for dim in (4, 36, 260, 2048)]      # 36, 260: a 256-column chunk partly filled; 2048: the limit
NORM_REFUSED = (2052, 6)


@functools.lru_cache(maxsize=None)
def norm_inputs(rows, dim):
    rs = np.random.RandomState(rows * 10007 + dim)
    f = lambda *s, scale=1.0: (rs.standard_normal(s) * scale).astype(np.float32)
    return dict(x=f(rows, dim, scale=3.0), resid=f(rows, dim), post=f(rows, dim), w=f(dim), b=f(dim))


@functools.lru_cache(maxsize=None)
def norm_inputs_small_variance(rows, dim, std):
    """`norm_inputs` with every second row of x and resid scaled to standard deviation `std`: with std^2 near a norm's epsilon the
    output depends on the epsilon, which rows of unit scale cannot show."""
    inp = {k: v.copy() for k, v in norm_inputs(rows, dim).items()}
    inp["x"][1::2] *= np.float32(std / 3.0)
    inp["resid"][1::2] *= np.float32(std)
    return inp


def layernorm64(x, w, b, eps=1e-5):
    x = x.astype(np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)            # biased, eps inside the root: torch.nn.LayerNorm
    return (x - mu) / np.sqrt(var + eps) * w.astype(np.float64) + b.astype(np.float64)


def rmsnorm64(x, w, eps=1e-6):
    x = x.astype(np.float64)                                 # custom_transformer.py:38-45
    y = x / np.sqrt((x * x).mean(-1, keepdims=True) + eps)
    return y * w.astype(np.float64) if w is not None else y


def chord_embed64(root, attr, key, PR, PA, wkey, bias, pe):
    """xf[b, l] = PR[root] + PA[attr] + key[b] * wkey + bias + pe[l] (include/amt_hip.h)."""
    f = lambda a: a.astype(np.float64)
    return f(PR)[root] + f(PA)[attr] + f(key)[:, None, None] * f(wkey) + f(bias) + f(pe)[None, :root.shape[1]]


# =====================================================================================================================
# device-side plumbing of the GPU tests (torch only)
# =====================================================================================================================
def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda().contiguous()


class Guarded:
    """An output buffer of n floats between two guards of GUARD floats, everything pre-filled with the sentinel."""

    def __init__(self, n):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")

    def addr(self, offset=0):
        return self.buf.data_ptr() + 4 * (GUARD + offset)

    def check(self, written_index):
        """Returns the n floats (numpy) after asserting that everything outside `written_index` (flat indices into them, or a boolean
        mask) still holds the sentinel's bits -- the guards included."""
        host = self.buf.cpu().numpy()
        mask = np.zeros(host.size, dtype=bool)
        if written_index.dtype == bool:
            mask[GUARD:GUARD + self.n] = written_index.reshape(-1)
        else:
            mask[GUARD + np.asarray(written_index).reshape(-1)] = True
        assert untouched(host, mask), "the kernel wrote outside its rows x columns"
        return host[GUARD:GUARD + self.n]


def rect_mask(rows, ld, cols):
    m = np.zeros((rows, ld), dtype=bool)
    m[:, :cols] = True
    return m
