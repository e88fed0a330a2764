"""Input conditions of the operator edge tests, checked on the CPU (the library is asked for launch routes only, which needs no
GPU): every case takes the route its comment names, the case tables cover the edges they are meant to, the steered MoE routing is not a rounding question, and on each
case's inputs the plain fp32 restatement is within a quarter of the bound of the fp64 one -- so a GPU test that misses its bound
cannot blame its inputs.  The computed tolerances are printed (pytest -s)."""
import numpy as np
import pytest
import torch

from tests import helpers_ops_edges as H
from tests import launch_routes as R


# ---- A. GEMM -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in H.GEMM_CASES])
def test_gemm_case_route_and_condition(name):
    c = H.GEMM_BY_NAME[name]
    assert c.edge, "every case names the route or edge it exists for"
    assert R.route_of(c) == c.route
    assert c.K % 32 == 0 and (c.K + c.dx) % 4 == 0 and (c.K + c.dw) % 4 == 0 and c.xcol % 4 == 0      # what the launcher accepts
    inp = H.gemm_inputs(name)
    assert inp["ldy"] >= c.N and inp["ldr"] >= c.N
    ref = H.gemm_ref64(name)
    assert ref.shape == (c.M, c.N) and np.isfinite(ref).all()
    err32 = float(np.abs(H.gemm_ref32_torch(name).astype(np.float64) - ref).max())
    tol = H.gemm_tol(name)
    print(f"{name}: route {c.route}, {'vector' if c.vec else 'element-wise'} epilogue, fp32 torch error {err32:.2e}, tolerance {tol:.2e}")
    assert err32 <= tol / 4


def test_gemm_table_covers_the_named_edges():
    C = H.GEMM_CASES
    B = R.BOUNDARIES
    for route in ("tile64", "tile128"):
        assert {c.vec for c in C if c.route == route} == {True, False}, f"both epilogues on {route}"
    nk = {c.K // 32 for c in C if c.route == "tile64"}
    assert 1 in nk and any(n % 2 == 1 and n > 1 for n in nk)
    assert any(c.route == "skinny" and B["small_mn"] - B["small_m"] < c.M * c.N <= B["small_mn"] for c in C)
    assert any(c.route == "tile64" and c.M <= B["small_m"] and B["small_mn"] < c.M * c.N < B["small_mn"] + B["small_m"] and c.K <= B["skinny_k"] and c.act == 0 for c in C)
    assert any(c.route == "tile64" and c.M == B["small_m"] + 1 for c in C)
    assert any(c.route == "skinny" and c.dx and c.dw and c.dy and c.dr and c.xcol for c in C)
    assert {c.act for c in C if c.route == "tile64"} == {0, 2, 3}
    t128 = [c for c in C if c.route == "tile128"]
    assert all((-(-c.M // 128) * -(-c.N // 128)) % 8 != 0 and c.M % 128 and c.N % 128 for c in t128)
    vec = {c.name: c.vec for c in C if c.name.startswith("vec_")}
    assert vec == {"vec_all_mult4": True, "vec_ldy_odd": False, "vec_ldr_odd": False, "vec_padded": True}


def test_gemm_tolerances():
    """SiLU and K = 9600: max(2e-5, 4 x the kernel-order fp32 restatement's error against fp64); everything else 2e-5."""
    for c in H.GEMM_CASES:
        tol = H.gemm_tol(c.name)
        if c.act == 3 or c.K > 2048:
            rows, v = H.gemm_kernel_order_f32(c.name)
            err = float(np.abs(v.astype(np.float64) - H.gemm_ref64(c.name)[rows]).max())
            print(f"{c.name}: kernel-order fp32 restatement error {err:.2e} over {len(rows)} rows -> tolerance {tol:.2e}")
            assert tol == max(H.TOL, 4 * err)
        else:
            assert tol == H.TOL
        assert tol < 1e-4                # a restatement error that large would mean the inputs are badly conditioned


# ---- B. attention ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in H.ATTN_CASES])
def test_attn_case_kernel_and_condition(name):
    c = H.ATTN_BY_NAME[name]
    assert c.edge and R.attn_route(c.B, c.H, c.Lq, c.Lk, c.hd) == c.kernel
    assert c.H % c.g == 0 and c.hd in (16, 32, 64, 128)
    inp = H.attn_inputs(name)
    st = inp["strides"]
    assert st[2] % 4 == 0 and st[5] % 4 == 0 and st[8] % 4 == 0          # q_ls, k_ls, v_ls: what the launcher accepts
    assert all(inp["lay"][t][0] % 4 == 0 for t in "qkvo")                # 16-byte aligned bases
    oi, osize = H.attn_o_index(c)
    assert oi.max() < osize and len(np.unique(oi)) == oi.size < osize     # o has padding the kernel must not touch
    for t, Hn, L in (("q", c.H, c.Lq), ("k", c.H // c.g, c.Lk), ("v", c.H // c.g, c.Lk)):
        assert H._index(*inp["lay"][t][:4], c.B, Hn, L, c.hd).max() < inp["lay"][t][4]
    ref = H.attn_ref64(name)
    assert np.isfinite(ref).all()
    err32 = float(np.abs(H.attn_ref32_torch(name).astype(np.float64) - ref).max())
    print(f"{name}: fp32 torch error {err32:.2e}")
    assert err32 <= H.TOL / 4


def test_attn_table_covers_the_named_edges():
    C = H.ATTN_CASES
    merged = lambda c: "v3" if c.layout.startswith("v3") else c.layout
    for lay in ("seq", "clip", "v3", "grp", "pad"):
        mine = [c for c in C if merged(c) == lay]
        assert {c.hd for c in mine} == {16, 32, 64, 128}, lay
        assert {c.causal for c in mine} == {0, 1}, lay
        assert {c.qs for c in mine} == {0, 1, 2}, lay
    assert {c.layout for c in C} >= {"v3e", "v3o"}
    assert {c.g for c in C if c.layout == "grp"} >= {2, 4}
    sk = [c for c in C if c.kernel == "splitk"]
    for hd in (32, 64):
        assert {(c.Lq, c.Lk, c.causal) for c in sk if c.hd == hd} >= {p[:3] for p in H.SPLITK_PAIRS}
    assert all(c.B <= 2 and c.H <= 4 for c in sk)
    assert any(c.causal and c.Lq >= 32 and c.Lk >= 256 for c in sk)                    # causal mask; first row block: one key tile, idle waves
    assert any(c.g > 1 for c in sk) and any(c.spikes for c in sk)
    assert any(c.kernel == "rows128" and c.Lk >= 256 and c.hd == 32 and -(-c.Lq // 128) * c.H * c.B == 512 and c.g == 4 and c.causal for c in C)
    for hd in (16, 128):
        assert {(c.Lq, c.Lk, c.causal) for c in C if c.hd == hd} >= {p[:3] for p in H.SPLITK_PAIRS}
    assert {(c.Lq, c.Lk) for c in C if c.hd == 64 and c.kernel == "rows128"} >= {(33, 31), (130, 77), (77, 130), (1, 1)}


def test_attn_spikes_sit_where_the_case_says():
    c = H.ATTN_BY_NAME["splitk_spikes"]
    inp = H.attn_inputs(c.name)
    lay, bufs = inp["lay"], inp["bufs"]
    q = bufs["q"][H._index(*lay["q"][:4], 1, 1, c.Lq, c.hd)][0, 0].astype(np.float64)
    k = bufs["k"][H._index(*lay["k"][:4], 1, 1, c.Lk, c.hd)][0, 0].astype(np.float64)
    s = q @ k.T
    for row, key in ((7, 100), (20, 290), (12, 3)):                      # key tiles 3, 9, 0 -> waves 3, 1, 0 (tile % 4)
        assert s[row].argmax() == key and s[row, key] - np.partition(s[row], -2)[-2] > 20.0
    assert [key // 32 % 4 for key in (100, 290, 3)] == [3, 1, 0]


# ---- C. MoE ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in H.MOE_CASES])
def test_moe_case_steering_and_tolerance(name):
    c = H.MOE_BY_NAME[name]
    assert c.edge and 1 <= c.k <= min(8, c.n_exp) and c.d % 32 == 0 and c.dff % 32 == 0
    assert all(len(set(row)) == c.k for row in c.chosen.tolist())
    inp = H.moe_inputs(name)
    lg = H.moe_logits64(inp)
    order = np.argsort(-lg, axis=1, kind="stable")                        # stable: the lower id first among equals
    assert np.array_equal(order[:, :c.k], c.chosen)
    chosen = np.take_along_axis(lg, c.chosen, axis=1)
    gaps = chosen[:, :-1] - chosen[:, 1:]
    unchosen = np.where((np.arange(c.n_exp)[None, None, :] == c.chosen[:, :, None]).any(1), -np.inf, lg)
    last_gap = chosen[:, -1] - unchosen.max(1) if c.k < c.n_exp else np.full(c.n_tok, np.inf)
    if c.tie:
        a, b = c.tie
        lg32 = inp["x"] @ inp["gate_w"].T                                 # whatever the summation order, identical rows give identical sums
        assert np.array_equal(H.bits(lg32[:, a]), H.bits(lg32[:, b])) and np.array_equal(inp["gate_w"][a], inp["gate_w"][b])
        ja = int(np.where(c.chosen[0] == a)[0][0])
        assert c.chosen[0, ja + 1] == b and a < b and np.all(gaps[:, ja] == 0.0)
        gaps = np.delete(gaps, ja, axis=1)
    assert gaps.size == 0 or gaps.min() >= 1.0, "consecutive chosen logits differ by at least 1"
    assert last_gap.min() >= 1.0, "the last chosen logit beats the best unchosen one by at least 1"
    tol, err32 = H.moe_tol(name)
    print(f"{name}: counts {H.plan_counts(c.chosen, c.n_exp).tolist()}, fp32 torch error {err32:.2e}, tolerance {tol:.2e}")
    assert tol <= H.MOE_TOL_CAP and np.isfinite(H.moe_ref64(name)).all()


def test_moe_table_covers_the_named_edges():
    counts = {c.name: H.plan_counts(c.chosen, c.n_exp) for c in H.MOE_CASES}
    assert counts["full_two_segments"].tolist() == [128, 128, 0, 0, 0, 0, 0, 0]
    assert counts["full_plus_one"].tolist() == [129, 129, 0, 0, 0, 0, 0, 0]
    assert counts["ragged_counts"].tolist() == [127, 1, 0, 132, 0, 0, 0, 4]
    assert counts["experts_63_and_0"][63] == 70 and counts["experts_63_and_0"][0] == 70 and counts["experts_63_and_0"].sum() == 140
    assert counts["five_experts"].min() > 0 and len(counts["five_experts"]) == 5
    assert counts["topk1_one_expert"].tolist() == [0, 0, 0, 0, 0, 300, 0, 0]
    assert counts["topk8_all"].tolist() == [20] * 8
    C = H.MOE_CASES
    assert {(c.shared, c.glu) for c in C} == {(a, b) for a in (True, False) for b in (True, False)}
    assert any(not c.gate_b for c in C) and any(c.tie and c.k == 2 for c in C) and any(c.tie and c.k == 3 for c in C)
    assert {c.n_exp for c in C} >= {2, 5, 8, 64} and {c.d for c in C} >= {32, 128, 288} and {c.k for c in C} >= {1, 2, 3, 8}
    assert any(c.n_tok == 1 for c in C)


def test_glu_piece_tolerances():
    for (n, d, dff, glu) in H.GLU_PIECES:
        tol, err, _ = H.glu_piece_tol(n, d, dff, glu)
        print(f"glu piece n={n} d={d} dff={dff} glu={glu}: fp32 torch error {err:.2e}, tolerance {tol:.2e}")
        assert tol <= H.MOE_TOL_CAP


def test_ep_recv_plan():
    e = H.ep_expert_of_row(H.EP_RECV_COUNTS)
    assert len(e) == 196 and np.bincount(e).tolist() == [132, 64]          # expert 0: full plus four rows over two sources; expert 1: half a tile
    assert e[:129].tolist() == [0] * 129 and e[129:132].tolist() == [0] * 3 and e[132:].tolist() == [1] * 64


# ---- D. row-wise -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,dim", H.NORM_SHAPES)
def test_norm_restatements_against_torch(rows, dim):
    """The fp64 restatements are the operations torch names (a check of the reference, not of the library), and fp32 on these inputs
    is well inside the 2e-5 the norm kernels are held to."""
    inp = H.norm_inputs(rows, dim)
    x, w, b = inp["x"] + inp["resid"], inp["w"], inp["b"]
    ln = torch.nn.functional.layer_norm(torch.from_numpy(x).double(), (dim,), torch.from_numpy(w).double(), torch.from_numpy(b).double(), 1e-5)
    assert np.abs(H.layernorm64(x, w, b) - ln.numpy()).max() < 1e-12
    ln32 = torch.nn.functional.layer_norm(torch.from_numpy(x), (dim,), torch.from_numpy(w), torch.from_numpy(b), 1e-5)
    assert np.abs(ln32.numpy() - H.layernorm64(x, w, b)).max() <= H.TOL / 4
    xt = torch.from_numpy(x).double()
    rms = xt * torch.rsqrt(xt.pow(2).mean(-1, keepdim=True) + 1e-6) * torch.from_numpy(w).double()
    assert np.abs(H.rmsnorm64(x, w) - rms.numpy()).max() < 1e-12
    assert dim % 4 == 0 and dim <= 2048 and all(d % 4 != 0 or d > 2048 for d in H.NORM_REFUSED)
