// Training of the mixture-of-experts layer (model/moe.py:36-49 GLUExpert, :150-200 MoELayer, :202-302 SharedMoELayer; the
// Linear -> SiLU -> Dropout -> Linear experts of video_music_transformer.py:80-85): the forward that keeps what the backward reads, and
// the backward.
//
// Forward (amt_moe_train_fwd): moe.hip's router, plan, grouped GEMMs and combine.  The eval path gates the up projection in its GEMM
// epilogue; here the up branch U is a launch of its own and a small kernel forms H = U silu(G) (x the dropout multiplier) with the
// epilogue's expression, so that without multipliers the bits are the eval path's.  The placement inside a segment is the stable one
// (moe_place_stable_kernel: rows ascend with the assignment index), which the forward's values do not depend on and the backward's
// sums over a segment's rows do.
//
// Backward (amt_moe_bwd), for assignment a = (t, j) in slot s of expert e:
//   1 moe_bwd_dy        dY[s] = (wts[a] dout[t]) mask_y[a]  (zeros in the padding slots),  dw[a] = <dout[t], Y[s]>
//   2 moe_bwd_dlogit    dlogit[t, idx[a]] = wts[a] (dw[a] - sum_i wts[t,i] dw[t,i]) / temperature, zero elsewhere
//   3 grouped GEMM      dH = dY W2[e]                       (the forward's grouped kernel over the transposed stacked weights)
//   4 moe_bwd_act       dH *= mask_h[a];  dU = dH silu(G),  dG = dH U silu'(G)   (dG = dH silu'(G) for SiLU experts)
//   5 grouped GEMMs     dX[s] = dU W1[e] + dG Wg[e]
//   6 moe_wgrad x 3     dW2[e] = dY_e^T H_e, db2;  dW1[e] = dU_e^T x_e, db1;  dWg[e] = dG_e^T x_e, dbg      (x gathered through perm)
//   7 the shared expert: the same, dense, from dout / k
//   8 moe_wgrad         dgate_w = dlogit^T x, dgate_b
//   9 moe_bwd_dx        dx[t] = sum_j dX[slot_pos[t,j]] (j ascending) + shared dX[t] + sum_j dlogit[t, idx[t,j]] gate_w[idx[t,j]]
//
// moe_wgrad (moe_train_kernels.h, shared with the plain GLU layer's training in family_train.hip, as are the two activation kernels)
// is the grouped weight-gradient product: out[e] (N x K) = sum over the rows r of expert e's segment of P[r][:]^T Q[r][:] on
// the fp32 MFMA (32x32x2: the two reduction slots of an instruction are two consecutive rows).  A wave owns one 32 x 32 output tile
// and walks its expert's rows in ascending order; both operands are read straight from global memory (for a fixed row the 32 lanes of
// a half-wave read 32 consecutive floats), the bias gradient is the running sum of the P operand.  With S > 1 the rows of an expert are
// cut into S runs of whole 128-row tiles, each run's partial goes to the workspace and moe_wgrad_reduce adds them in ascending order.
// It visits only [seg[e], seg[e+1]): rows of unused tiles are never written by the forward and never read here.
// Nothing here uses a floating-point atomic; every sum has one order fixed by the shapes and the plan.
#include "../../include/amt_hip.h"
#include "amt_common.h"
#include "kernels.h"
#include "moe_train_kernels.h"

namespace {

constexpr int KMAX = 8;

// `saved`: moe_fwd_impl's scratch layout first (moe.hip), then what only training keeps
struct Saved {
    float *G, *H, *Y, *Gs, *Hs, *Ys, *wts, *U, *Us;
    int *perm, *slot_pos, *tile_group, *idx, *plan_ints, *slot_assign, *dense_group;
    int Mp;
    size_t floats;
};
Saved saved_layout(float* base, int n_tok, int d, int dff, int n_exp, int k, int glu) {
    Saved s{};
    const size_t A = (size_t)k * n_tok;
    s.Mp = (k * n_tok + TILE - 1) / TILE * TILE + TILE * n_exp;
    const size_t Mp = s.Mp;
    s.G = base;
    s.H = s.G + Mp * dff;
    s.Y = s.H + Mp * dff;
    s.Gs = s.Y + Mp * d;
    s.Hs = s.Gs + (size_t)n_tok * dff;
    s.Ys = s.Hs + (size_t)n_tok * dff;
    s.perm = (int*)(s.Ys + (size_t)n_tok * d);
    s.slot_pos = s.perm + align4(Mp);
    s.tile_group = s.slot_pos + align4(A);
    s.idx = s.tile_group + align4(Mp / TILE + 1);
    s.wts = (float*)(s.idx + align4(A));
    s.plan_ints = (int*)(s.wts + align4(A));                  // [0..63] counts, [64..128] segment offsets, [192..255] cursors
    s.slot_assign = s.plan_ints + 256 + 64;
    s.dense_group = s.slot_assign + align4(Mp);               // zeros: one weight group for every row tile of a dense product
    s.U = (float*)(s.dense_group + align4((size_t)n_tok / TILE + 2));
    s.Us = s.U + (glu ? Mp * dff : 0);
    s.floats = (size_t)((s.Us + (glu ? (size_t)n_tok * dff : 0)) - base);
    return s;
}

// slot_assign[slot_pos[a]] = a (the padding slots keep -1)
__global__ __launch_bounds__(256) void moe_slot_assign_kernel(const int* __restrict__ slot_pos, int n_assign, int* __restrict__ slot_assign) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a < n_assign) slot_assign[slot_pos[a]] = a;
}

// Y[slot_pos[a]] *= mask_y[a]; one wave per assignment
__global__ __launch_bounds__(256) void moe_mask_rows_kernel(float* __restrict__ Y, const int* __restrict__ slot_pos, const float* __restrict__ mask,
                                                            int n_assign, int d) {
    const int a = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (a >= n_assign) return;
    float* y = Y + (size_t)slot_pos[a] * d;
    for (int c = lane * 4; c < d; c += 256) {
        const float4 v = ld4(y + c), m = ld4(mask + (size_t)a * d + c);
        st4(y + c, make_float4(v.x * m.x, v.y * m.y, v.z * m.z, v.w * m.w));
    }
}

// ---- backward ----
// one wave per slot row of a used tile
__global__ __launch_bounds__(256) void moe_bwd_dy_kernel(const float* __restrict__ dout, const float* __restrict__ Y, const float* __restrict__ wts,
                                                         const float* __restrict__ mask_y, const int* __restrict__ slot_assign,
                                                         const int* __restrict__ tile_group, float* __restrict__ dY, float* __restrict__ dw,
                                                         int Mp, int d, int k) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= Mp || tile_group[row / TILE] < 0) return;
    const int a = slot_assign[row];
    if (a < 0) {                                    // a padding slot: its saved rows are finite, its gradient row is zero
        for (int c = lane * 4; c < d; c += 256) st4(dY + (size_t)row * d + c, make_float4(0.f, 0.f, 0.f, 0.f));
        return;
    }
    const int t = a / k;
    const float w = wts[a];
    float acc = 0.f;
    for (int c = lane * 4; c < d; c += 256) {
        const float4 g = ld4(dout + (size_t)t * d + c), y = ld4(Y + (size_t)row * d + c);
        acc += g.x * y.x + g.y * y.y + g.z * y.z + g.w * y.w;
        float4 v = make_float4(w * g.x, w * g.y, w * g.z, w * g.w);
        if (mask_y) {
            const float4 m = ld4(mask_y + (size_t)a * d + c);
            v.x *= m.x; v.y *= m.y; v.z *= m.z; v.w *= m.w;
        }
        st4(dY + (size_t)row * d + c, v);
    }
    acc = wave_sum(acc);
    if (lane == 0) dw[a] = acc;
}

// one thread per token: the softmax over the k chosen logits, backward; dlogit (n_tok, n_exp) dense, dl (n_tok, k) its k entries
__global__ __launch_bounds__(256) void moe_bwd_dlogit_kernel(const float* __restrict__ dw, const float* __restrict__ wts, const int* __restrict__ idx,
                                                             float* __restrict__ dlogit, float* __restrict__ dl, int n_tok, int n_exp, int k,
                                                             float inv_temperature) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tok) return;
    float s = 0.f;
    for (int i = 0; i < k; ++i) s += wts[t * k + i] * dw[t * k + i];
    for (int e = 0; e < n_exp; ++e) dlogit[(size_t)t * n_exp + e] = 0.f;
    for (int j = 0; j < k; ++j) {
        const float v = wts[t * k + j] * (dw[t * k + j] - s) * inv_temperature;
        dlogit[(size_t)t * n_exp + idx[t * k + j]] = v;
        dl[t * k + j] = v;
    }
}

__global__ __launch_bounds__(256) void moe_scale_kernel(const float* __restrict__ in, float* __restrict__ out, long n4, float s) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 v = ld4(in + i * 4);
    st4(out + i * 4, make_float4(v.x * s, v.y * s, v.z * s, v.w * s));
}

// one wave per token
__global__ __launch_bounds__(256) void moe_bwd_dx_kernel(const float* __restrict__ dXs, const int* __restrict__ slot_pos, const float* __restrict__ dXsh,
                                                         const float* __restrict__ dl, const int* __restrict__ idx, const float* __restrict__ gate_w,
                                                         float* __restrict__ dx, int n_tok, int d, int k) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= n_tok) return;
    for (int c = lane * 4; c < d; c += 256) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < k; ++j) {
            const float4 v = ld4(dXs + (size_t)slot_pos[t * k + j] * d + c);
            o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
        }
        if (dXsh) {
            const float4 v = ld4(dXsh + (size_t)t * d + c);
            o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
        }
        for (int j = 0; j < k; ++j) {
            const float g = dl[t * k + j];
            const float4 w = ld4(gate_w + (size_t)idx[t * k + j] * d + c);
            o.x += g * w.x; o.y += g * w.y; o.z += g * w.z; o.w += g * w.w;
        }
        st4(dx + (size_t)t * d + c, o);
    }
}

// amt_moe_bwd's S: of the experts' products over the plan's k n_tok assignments, or (dense) of the one-group products over the tokens
int wgrad_plan_splits(int n_tok, int d, int dff, int n_exp, int k, int dense) {
    const int cap = wgrad_split_cap(n_exp, d, dff);
    return dense ? wgrad_splits(((long)n_tok + TILE - 1) / TILE, 1, cap) : wgrad_splits(((long)k * n_tok + TILE - 1) / TILE, n_exp, cap);
}

struct BwdWs {
    float *dY, *dU, *dG, *dXs, *dw, *dl, *dlogit, *dYs, *dUs, *dGs, *dXsh, *dXtmp, *split;
    size_t floats;
};
BwdWs bwd_layout(float* base, int n_tok, int d, int dff, int n_exp, int k) {
    BwdWs w{};
    const size_t Mp = (size_t)((k * n_tok + TILE - 1) / TILE * TILE + TILE * n_exp), A = (size_t)k * n_tok;
    w.dY = base;
    w.dU = w.dY + Mp * d;
    w.dG = w.dU + Mp * dff;
    w.dXs = w.dG + Mp * dff;
    w.dw = w.dXs + Mp * d;
    w.dl = w.dw + align4(A);
    w.dlogit = w.dl + align4(A);
    w.dYs = w.dlogit + align4((size_t)n_tok * n_exp);
    w.dUs = w.dYs + (size_t)n_tok * d;
    w.dGs = w.dUs + (size_t)n_tok * dff;
    w.dXsh = w.dGs + (size_t)n_tok * dff;
    w.dXtmp = w.dXsh + (size_t)n_tok * d;
    w.split = w.dXtmp + (size_t)n_tok * d;
    // the largest product's partials: n_exp groups of (dff x d + dff), or the gate's / the shared expert's single group
    w.floats = (size_t)(w.split - base) + (size_t)wgrad_split_cap(n_exp, d, dff) * n_exp * ((size_t)dff * d + (dff > d ? dff : d));
    return w;
}

}  // namespace

extern "C" int64_t amt_moe_train_scratch_floats(int32_t n_tok, int32_t d, int32_t dff, int32_t n_exp, int32_t k, int32_t glu) {
    return (int64_t)saved_layout(nullptr, n_tok, d, dff, n_exp, k, glu).floats;
}

extern "C" int64_t amt_moe_bwd_ws_floats(int32_t n_tok, int32_t d, int32_t dff, int32_t n_exp, int32_t k) {
    return (int64_t)bwd_layout(nullptr, n_tok, d, dff, n_exp, k).floats;
}

extern "C" int32_t amt_moe_wgrad_splits(int32_t n_tok, int32_t d, int32_t dff, int32_t n_exp, int32_t k, int32_t dense) {
    if (n_tok <= 0 || d <= 0 || dff <= 0 || n_exp < 2 || n_exp > 64 || k < 1 || k > KMAX || k > n_exp) return -1;
    return wgrad_plan_splits(n_tok, d, dff, n_exp, k, dense);
}

// amt_moe_train_fwd, and with sel_bias given amt_moe_train_fwd_balanced: only the router and the bias_delta launch differ
static int32_t moe_train_fwd_impl(const char* entry, const float* x, const float* gate_w, const float* gate_b,
                                  const float* w1, const float* b1, const float* wg, const float* bg, const float* w2, const float* b2,
                                  const float* sw1, const float* sb1, const float* swg, const float* sbg, const float* sw2, const float* sb2,
                                  const float* mask_h, const float* mask_y, const float* mask_hs,
                                  float* out, int32_t* idx_out, float* w_out, float* saved,
                                  int32_t n_tok, int32_t d, int32_t dff, int32_t dff_raw, int32_t n_exp, int32_t k, void* stream,
                                  const float* sel_bias, float update_rate, float* bias_delta) {
    AMT_CHECK_ARG(x && gate_w && wg && w2 && out && saved, "%s: null pointer", entry);
    AMT_CHECK_ARG(n_tok > 0 && n_exp >= 2 && n_exp <= 64, "%s: need 2 <= n_experts <= 64", entry);
    AMT_CHECK_ARG(k >= 1 && k <= KMAX && k <= n_exp, "%s: n_experts_per_token=%d outside 1..min(%d, n_experts)", entry, k, KMAX);
    AMT_CHECK_ARG(d % 32 == 0 && dff % 32 == 0, "%s: d and d_ff must be multiples of 32", entry);
    AMT_CHECK_ARG(dff_raw > 0 && dff_raw <= dff, "%s: the experts' own width %d is outside 1..d_ff=%d", entry, dff_raw, dff);
    AMT_CHECK_ARG((long)k * n_tok + (long)TILE * (n_exp + 1) < (1L << 31) / (dff > d ? dff : d), "%s: the plan's rows do not fit 32-bit indices", entry);
    AMT_CHECK_ARG(!mask_hs || swg, "%s: mask_hs without a shared expert", entry);
    hipStream_t s = (hipStream_t)stream;
    const int glu = w1 != nullptr;
    const Saved sv = saved_layout(saved, n_tok, d, dff, n_exp, k, glu);
    const int Mp = sv.Mp, A = k * n_tok;
    int32_t rc;
    if ((rc = amt_launch_moe_route_plan(x, gate_w, gate_b, sv.idx, sv.wts, sv.plan_ints, sv.perm, sv.slot_pos, sv.tile_group, n_tok, d, n_exp, k, Mp, s,
                                        sel_bias, update_rate, bias_delta)))
        return rc;
    AMT_HIP(hipMemsetAsync(sv.slot_assign, 0xFF, (size_t)Mp * sizeof(int), s));
    AMT_HIP(hipMemsetAsync(sv.dense_group, 0, ((size_t)n_tok / TILE + 2) * sizeof(int), s));
    hipLaunchKernelGGL(moe_slot_assign_kernel, dim3(cdiv(A, 256)), dim3(256), 0, s, sv.slot_pos, A, sv.slot_assign);
    AMT_LAUNCH_CHECK();
    if (idx_out) AMT_HIP(hipMemcpyAsync(idx_out, sv.idx, (size_t)A * sizeof(int), hipMemcpyDeviceToDevice, s));
    if (w_out) AMT_HIP(hipMemcpyAsync(w_out, sv.wts, (size_t)A * sizeof(float), hipMemcpyDeviceToDevice, s));
    // gate branch G = x_e Wg[e]^T + bg[e]; up branch U = x_e W1[e]^T + b1[e] (GLU experts); H from both
    GemmParams g = gemm_params(x, d, wg, d, sv.G, dff, Mp, dff, d, bg);
    g.a_gather = sv.perm; g.tile_group = sv.tile_group; g.w_group_stride = (size_t)dff * d; g.bias_group_stride = dff;
    if ((rc = amt_launch_gemm(g, s))) return rc;
    if (glu) {
        GemmParams u = g;
        u.W = w1; u.bias = b1; u.C = sv.U;
        if ((rc = amt_launch_gemm(u, s))) return rc;
    }
    hipLaunchKernelGGL(moe_act_fwd_kernel, dim3(cdiv(Mp, 4)), dim3(256), 0, s, sv.G, glu ? sv.U : nullptr, sv.H, mask_h, sv.slot_assign, sv.tile_group,
                       Mp, dff, dff_raw);
    AMT_LAUNCH_CHECK();
    GemmParams dn = gemm_params(sv.H, dff, w2, dff, sv.Y, d, Mp, d, dff, b2);
    dn.tile_group = sv.tile_group; dn.w_group_stride = (size_t)d * dff; dn.bias_group_stride = d;
    if ((rc = amt_launch_gemm(dn, s))) return rc;
    if (mask_y) {
        hipLaunchKernelGGL(moe_mask_rows_kernel, dim3(cdiv(A, 4)), dim3(256), 0, s, sv.Y, sv.slot_pos, mask_y, A, d);
        AMT_LAUNCH_CHECK();
    }
    const float* shared = nullptr;
    if (swg) {
        AMT_CHECK_ARG(sw2 && (sw1 != nullptr) == (w1 != nullptr), "%s: incomplete shared expert", entry);
        // the eval path's gate launch as it is for GLU experts; where that path has an epilogue the tiled kernel needs (the SiLU of
        // a SiLU expert, the gate of the up projection) the plain product takes the same kernel through a one-group tile plan
        GemmParams a = gemm_params(x, d, swg, d, sv.Gs, dff, n_tok, dff, d, sbg);
        if (!glu) a.tile_group = sv.dense_group;
        if ((rc = amt_launch_gemm(a, s))) return rc;
        if (glu) {
            GemmParams b = gemm_params(x, d, sw1, d, sv.Us, dff, n_tok, dff, d, sb1);
            b.tile_group = sv.dense_group;
            if ((rc = amt_launch_gemm(b, s))) return rc;
        }
        hipLaunchKernelGGL(moe_act_fwd_kernel, dim3(cdiv(n_tok, 4)), dim3(256), 0, s, sv.Gs, glu ? sv.Us : nullptr, sv.Hs, mask_hs, nullptr, nullptr,
                           n_tok, dff, dff_raw);
        AMT_LAUNCH_CHECK();
        GemmParams c = gemm_params(sv.Hs, dff, sw2, dff, sv.Ys, d, n_tok, d, dff, sb2);
        if ((rc = amt_launch_gemm(c, s))) return rc;
        shared = sv.Ys;
    }
    return amt_launch_moe_combine_k(sv.Y, sv.slot_pos, sv.idx, sv.wts, shared, out, n_tok, d, k, s);
}

extern "C" int32_t amt_moe_train_fwd(const float* x, const float* gate_w, const float* gate_b,
                                     const float* w1, const float* b1, const float* wg, const float* bg, const float* w2, const float* b2,
                                     const float* sw1, const float* sb1, const float* swg, const float* sbg, const float* sw2, const float* sb2,
                                     const float* mask_h, const float* mask_y, const float* mask_hs,
                                     float* out, int32_t* idx_out, float* w_out, float* saved,
                                     int32_t n_tok, int32_t d, int32_t dff, int32_t dff_raw, int32_t n_exp, int32_t k, void* stream) {
    return moe_train_fwd_impl("amt_moe_train_fwd", x, gate_w, gate_b, w1, b1, wg, bg, w2, b2, sw1, sb1, swg, sbg, sw2, sb2, mask_h, mask_y, mask_hs,
                              out, idx_out, w_out, saved, n_tok, d, dff, dff_raw, n_exp, k, stream, nullptr, 0.f, nullptr);
}

extern "C" int32_t amt_moe_train_fwd_balanced(const float* x, const float* gate_w, const float* gate_b,
                                              const float* w1, const float* b1, const float* wg, const float* bg, const float* w2, const float* b2,
                                              const float* sw1, const float* sb1, const float* swg, const float* sbg, const float* sw2, const float* sb2,
                                              const float* mask_h, const float* mask_y, const float* mask_hs,
                                              float* out, int32_t* idx_out, float* w_out, float* saved,
                                              int32_t n_tok, int32_t d, int32_t dff, int32_t dff_raw, int32_t n_exp, int32_t k, void* stream,
                                              const float* sel_bias, float update_rate, float* bias_delta) {
    AMT_CHECK_ARG(sel_bias && bias_delta, "amt_moe_train_fwd_balanced: null pointer");
    return moe_train_fwd_impl("amt_moe_train_fwd_balanced", x, gate_w, gate_b, w1, b1, wg, bg, w2, b2, sw1, sb1, swg, sbg, sw2, sb2, mask_h, mask_y,
                              mask_hs, out, idx_out, w_out, saved, n_tok, d, dff, dff_raw, n_exp, k, stream, sel_bias, update_rate, bias_delta);
}

extern "C" int32_t amt_moe_bwd(const float* dout, const float* x, const float* gate_w, const float* saved,
                               const float* w1t, const float* wgt, const float* w2t, const float* sw1t, const float* swgt, const float* sw2t,
                               const float* mask_h, const float* mask_y, const float* mask_hs,
                               float* dx, float* dgate_w, float* dgate_b,
                               float* dw1, float* db1, float* dwg, float* dbg, float* dw2, float* db2,
                               float* dsw1, float* dsb1, float* dswg, float* dsbg, float* dsw2, float* dsb2,
                               float* ws, int32_t n_tok, int32_t d, int32_t dff, int32_t dff_raw, int32_t n_exp, int32_t k, int32_t glu,
                               int32_t has_shared, float temperature, void* stream) {
    AMT_CHECK_ARG(dout && x && gate_w && saved && wgt && w2t && dx && dgate_w && dgate_b && dwg && dbg && dw2 && db2 && ws, "amt_moe_bwd: null pointer");
    AMT_CHECK_ARG(n_tok > 0 && n_exp >= 2 && n_exp <= 64, "amt_moe_bwd: need 2 <= n_experts <= 64");
    AMT_CHECK_ARG(k >= 1 && k <= KMAX && k <= n_exp, "amt_moe_bwd: n_experts_per_token=%d outside 1..min(%d, n_experts)", k, KMAX);
    AMT_CHECK_ARG(d % 32 == 0 && dff % 32 == 0, "amt_moe_bwd: d and d_ff must be multiples of 32");
    AMT_CHECK_ARG(dff_raw > 0 && dff_raw <= dff, "amt_moe_bwd: the experts' own width %d is outside 1..d_ff=%d", dff_raw, dff);
    AMT_CHECK_ARG((long)k * n_tok + (long)TILE * (n_exp + 1) < (1L << 31) / (dff > d ? dff : d), "amt_moe_bwd: the plan's rows do not fit 32-bit indices");
    AMT_CHECK_ARG(!glu || (w1t && dw1 && db1), "amt_moe_bwd: GLU experts need w1t, dw1 and db1");
    AMT_CHECK_ARG(!has_shared || (swgt && sw2t && dswg && dsbg && dsw2 && dsb2 && (!glu || (sw1t && dsw1 && dsb1))), "amt_moe_bwd: incomplete shared expert");
    AMT_CHECK_ARG(!mask_hs || has_shared, "amt_moe_bwd: mask_hs without a shared expert");
    AMT_CHECK_ARG(temperature > 0.f, "amt_moe_bwd: temperature must be positive");
    hipStream_t s = (hipStream_t)stream;
    const Saved sv = saved_layout(const_cast<float*>(saved), n_tok, d, dff, n_exp, k, glu);
    const BwdWs w = bwd_layout(ws, n_tok, d, dff, n_exp, k);
    const int Mp = sv.Mp, A = k * n_tok;
    const int* seg = sv.plan_ints + 64;
    int32_t rc;
    // 1, 2: through the combine and the softmax of the chosen logits
    hipLaunchKernelGGL(moe_bwd_dy_kernel, dim3(cdiv(Mp, 4)), dim3(256), 0, s, dout, sv.Y, sv.wts, mask_y, sv.slot_assign, sv.tile_group, w.dY, w.dw, Mp, d, k);
    hipLaunchKernelGGL(moe_bwd_dlogit_kernel, dim3(cdiv(n_tok, 256)), dim3(256), 0, s, w.dw, sv.wts, sv.idx, w.dlogit, w.dl, n_tok, n_exp, k,
                       1.0f / temperature);
    AMT_LAUNCH_CHECK();
    // 3: dH = dY W2[e]
    GemmParams gh = gemm_params(w.dY, d, w2t, d, w.dU, dff, Mp, dff, d, nullptr);
    gh.tile_group = sv.tile_group; gh.w_group_stride = (size_t)dff * d;
    if ((rc = amt_launch_gemm(gh, s))) return rc;
    // 4: dU (in place), dG
    hipLaunchKernelGGL(moe_bwd_act_kernel, dim3(cdiv(Mp, 4)), dim3(256), 0, s, w.dU, w.dG, sv.G, glu ? sv.U : nullptr, mask_h, sv.slot_assign,
                       sv.tile_group, Mp, dff, dff_raw);
    AMT_LAUNCH_CHECK();
    // 5: dX = dG Wg[e] (+ dU W1[e])
    GemmParams gx = gemm_params(w.dG, dff, wgt, dff, w.dXs, d, Mp, d, dff, nullptr);
    gx.tile_group = sv.tile_group; gx.w_group_stride = (size_t)d * dff;
    if ((rc = amt_launch_gemm(gx, s))) return rc;
    if (glu) {
        gx.A = w.dU; gx.W = w1t; gx.resid = w.dXs; gx.ldr = d;       // the tiled kernel: each element is read and rewritten by the thread that owns it
        if ((rc = amt_launch_gemm(gx, s))) return rc;
    }
    // 6: the experts' weight gradients, over their own segments only
    WgradParams p{};
    p.seg = seg; p.n_groups = n_exp; p.S = wgrad_plan_splits(n_tok, d, dff, n_exp, k, 0);
    p.P = w.dY; p.ldp = d; p.N = d; p.Q = sv.H; p.ldq = dff; p.K = dff; p.q_gather = nullptr; p.out = dw2; p.bias = db2;
    if ((rc = launch_wgrad(p, w.split, s))) return rc;
    p.P = w.dG; p.ldp = dff; p.N = dff; p.Q = x; p.ldq = d; p.K = d; p.q_gather = sv.perm; p.out = dwg; p.bias = dbg;
    if ((rc = launch_wgrad(p, w.split, s))) return rc;
    if (glu) {
        p.P = w.dU; p.out = dw1; p.bias = db1;
        if ((rc = launch_wgrad(p, w.split, s))) return rc;
    }
    // 7: the shared expert on every token, from dout / k
    WgradParams q{};
    q.rows = n_tok; q.n_groups = 1; q.S = wgrad_plan_splits(n_tok, d, dff, n_exp, k, 1);
    if (has_shared) {
        hipLaunchKernelGGL(moe_scale_kernel, dim3((unsigned)(((long)n_tok * d / 4 + 255) / 256)), dim3(256), 0, s, dout, w.dYs, (long)n_tok * d / 4,
                           1.0f / (float)k);
        AMT_LAUNCH_CHECK();
        if ((rc = amt_launch_gemm(gemm_params(w.dYs, d, sw2t, d, w.dUs, dff, n_tok, dff, d, nullptr), s))) return rc;
        hipLaunchKernelGGL(moe_bwd_act_kernel, dim3(cdiv(n_tok, 4)), dim3(256), 0, s, w.dUs, w.dGs, sv.Gs, glu ? sv.Us : nullptr, mask_hs, nullptr,
                           nullptr, n_tok, dff, dff_raw);
        AMT_LAUNCH_CHECK();
        GemmParams sx = gemm_params(w.dGs, dff, swgt, dff, glu ? w.dXtmp : w.dXsh, d, n_tok, d, dff, nullptr);
        if ((rc = amt_launch_gemm(sx, s))) return rc;
        if (glu) {                                                   // a dense product may take the skinny kernel: its own output buffer
            sx.A = w.dUs; sx.W = sw1t; sx.C = w.dXsh; sx.resid = w.dXtmp; sx.ldr = d;
            if ((rc = amt_launch_gemm(sx, s))) return rc;
        }
        q.P = w.dYs; q.ldp = d; q.N = d; q.Q = sv.Hs; q.ldq = dff; q.K = dff; q.out = dsw2; q.bias = dsb2;
        if ((rc = launch_wgrad(q, w.split, s))) return rc;
        q.P = w.dGs; q.ldp = dff; q.N = dff; q.Q = x; q.ldq = d; q.K = d; q.out = dswg; q.bias = dsbg;
        if ((rc = launch_wgrad(q, w.split, s))) return rc;
        if (glu) {
            q.P = w.dUs; q.out = dsw1; q.bias = dsb1;
            if ((rc = launch_wgrad(q, w.split, s))) return rc;
        }
    }
    // 8: the router
    q.P = w.dlogit; q.ldp = n_exp; q.N = n_exp; q.Q = x; q.ldq = d; q.K = d; q.out = dgate_w; q.bias = dgate_b;
    if ((rc = launch_wgrad(q, w.split, s))) return rc;
    // 9: the token's gradient
    hipLaunchKernelGGL(moe_bwd_dx_kernel, dim3(cdiv(n_tok, 4)), dim3(256), 0, s, w.dXs, sv.slot_pos, has_shared ? w.dXsh : nullptr, w.dl, sv.idx, gate_w,
                       dx, n_tok, d, k);
    AMT_LAUNCH_CHECK();
    return 0;
}
