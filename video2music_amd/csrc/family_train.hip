// What the training of the V1 / V2 chord models needs beside the base model's operators: the backward of the rotary embedding and the
// plain GLU / SiLU feed-forward in training (the backward of RMSNorm is norm_bwd.hip's).
//
// amt_rope_bwd: y = R(theta) x per interleaved pair under rope_kernel's index rule (norm.hip), so dx = R(theta)^T dy:
//   dx0 = dy0 cos + dy1 sin,  dx1 = dy1 cos - dy0 sin.  One thread per pair reads its pair before it writes it: dx may alias dy.
//
// amt_glu_train_fwd / amt_glu_bwd: one GLUExpert (model/moe.py:36-49; w1 null: Linear -> SiLU -> Dropout -> Linear) on n dense rows,
// the shared expert's path of moe_bwd.hip without a mixture around it.  The forward issues amt_glu_expert_fwd's products, but for the
// fused gate of the up projection: the up branch U is a launch of its own through the same tiled kernel (a one-group tile plan) and
// moe_act_fwd_kernel forms H = U silu(G) (x mask_h) with the epilogue's expression, so that without a mask the bits are the eval
// path's.  Kept: G, U (GLU only) and H as fed to the down projection; x and the weights are the caller's.  Backward:
//   dH = dout W2;  dH *= mask_h;  dU = dH silu(G),  dG = dH U silu'(G);  dx = dG Wg + dU W1
//   dW2 = dout^T H, db2;  dWg = dG^T x, dbg;  dW1 = dU^T x, db1          (moe_wgrad, one group over the n rows)
//
// Nothing here uses a floating-point atomic: the order of every addition is a function of the shapes alone.
#include "../../include/amt_hip.h"
#include "amt_common.h"
#include "kernels.h"
#include "moe_train_kernels.h"

namespace {

// ---------------- rotary embedding ----------------
// dy / dx viewed as [n0][seq][n2][hd]; the cache as rope_kernel reads it.  No __restrict__: dx may be dy.
__global__ __launch_bounds__(256) void rope_bwd_kernel(const float* dy, const float* __restrict__ cache, float* dx,
                                                       int seq, int n2, int hd, long total_pairs, int bcast) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total_pairs) return;
    const int half = hd / 2;
    const int p = (int)(i % half);
    long r = i / half;
    r /= n2;
    const int s = (int)(r % seq);
    const int a = bcast ? 0 : (int)(r / seq);
    const size_t ci = (((size_t)a * seq + s) * half + p) * 2;
    const float c = cache[ci], sn = cache[ci + 1];
    const float2 g = *reinterpret_cast<const float2*>(dy + 2 * i);
    *reinterpret_cast<float2*>(dx + 2 * i) = make_float2(g.x * c + g.y * sn, g.y * c - g.x * sn);
}

// ---------------- the plain GLU / SiLU expert ----------------
struct GluSaved {
    float *G, *U, *H;
    int* dense_group;               // zeros: one weight group for every row tile of a dense product
    size_t floats;
};
GluSaved glu_saved_layout(float* base, int n, int dff, int glu) {
    GluSaved s{};
    const size_t R = (size_t)n * dff;
    s.G = base;
    s.H = s.G + R;
    s.U = s.H + R;
    s.dense_group = (int*)(s.U + (glu ? R : 0));
    s.floats = (size_t)((float*)(s.dense_group + align4((size_t)n / TILE + 2)) - base);
    return s;
}
struct GluWs {
    float *dU, *dG, *dXtmp, *split;
    size_t floats;
};
int glu_wgrad_splits(int n, int d, int dff) { return wgrad_splits(((long)n + TILE - 1) / TILE, 1, wgrad_split_cap(1, d, dff)); }
GluWs glu_ws_layout(float* base, int n, int d, int dff) {
    GluWs w{};
    w.dU = base;
    w.dG = w.dU + (size_t)n * dff;
    w.dXtmp = w.dG + (size_t)n * dff;
    w.split = w.dXtmp + (size_t)n * d;
    w.floats = (size_t)(w.split - base) + (size_t)wgrad_split_cap(1, d, dff) * ((size_t)dff * d + (dff > d ? dff : d));
    return w;
}
bool glu_shape_ok(int n, int d, int dff, int dff_raw) {
    return n > 0 && d > 0 && dff > 0 && d % 32 == 0 && dff % 32 == 0 && dff_raw > 0 && dff_raw <= dff &&
           (long)n + TILE < (1L << 31) / (dff > d ? dff : d);
}

}  // namespace

extern "C" int32_t amt_rope_bwd(const float* dy, const float* cache, float* dx, int32_t n0, int32_t seq, int32_t n2, int32_t hd,
                                int32_t cache_half, void* stream) {
    AMT_CHECK_ARG(dy && cache && dx, "amt_rope_bwd: null pointer");
    AMT_CHECK_ARG(n0 > 0 && seq > 0 && n2 > 0 && hd > 0 && hd % 2 == 0, "amt_rope_bwd: bad shape");
    const int bcast = (cache_half * 2 == hd) ? 1 : 0;
    AMT_CHECK_ARG(bcast || (long)cache_half * 2 >= (long)n0 * hd, "amt_rope_bwd: cache has %d pairs per position, need %d (or exactly %d)",
                  cache_half, n0 * hd / 2, hd / 2);
    AMT_CHECK_ARG(((uintptr_t)dy & 7) == 0 && ((uintptr_t)dx & 7) == 0, "amt_rope_bwd: dy and dx must be 8-byte aligned");
    const long total = (long)n0 * seq * n2 * (hd / 2);
    hipLaunchKernelGGL(rope_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, cache, dx, seq, n2, hd,
                       total, bcast);
    AMT_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t amt_glu_train_scratch_floats(int32_t n, int32_t dff, int32_t glu) {
    return (int64_t)glu_saved_layout(nullptr, n, dff, glu).floats;
}

extern "C" int64_t amt_glu_bwd_ws_floats(int32_t n, int32_t d, int32_t dff) { return (int64_t)glu_ws_layout(nullptr, n, d, dff).floats; }

extern "C" int32_t amt_glu_train_fwd(const float* x, const float* w1, const float* b1, const float* wg, const float* bg, const float* w2,
                                     const float* b2, const float* mask_h, float* out, float* saved, int32_t n, int32_t d, int32_t dff,
                                     int32_t dff_raw, void* stream) {
    AMT_CHECK_ARG(x && wg && w2 && out && saved, "amt_glu_train_fwd: null pointer");
    AMT_CHECK_ARG(glu_shape_ok(n, d, dff, dff_raw), "amt_glu_train_fwd: bad shape n=%d d=%d d_ff=%d (own width %d)", n, d, dff, dff_raw);
    hipStream_t s = (hipStream_t)stream;
    const int glu = w1 != nullptr;
    const GluSaved sv = glu_saved_layout(saved, n, dff, glu);
    int32_t rc;
    AMT_HIP(hipMemsetAsync(sv.dense_group, 0, ((size_t)n / TILE + 2) * sizeof(int), s));
    // the eval path's gate launch as it is for a GLU expert; where that path has an epilogue the tiled kernel needs (the SiLU of a SiLU
    // expert, the gate of the up projection) the plain product takes the same kernel through a one-group tile plan
    GemmParams a = gemm_params(x, d, wg, d, sv.G, dff, n, dff, d, bg);
    if (!glu) a.tile_group = sv.dense_group;
    if ((rc = amt_launch_gemm(a, s))) return rc;
    if (glu) {
        GemmParams b = gemm_params(x, d, w1, d, sv.U, dff, n, dff, d, b1);
        b.tile_group = sv.dense_group;
        if ((rc = amt_launch_gemm(b, s))) return rc;
    }
    hipLaunchKernelGGL(moe_act_fwd_kernel, dim3(cdiv(n, 4)), dim3(256), 0, s, sv.G, glu ? sv.U : nullptr, sv.H, mask_h, nullptr, nullptr, n, dff,
                       dff_raw);
    AMT_LAUNCH_CHECK();
    return amt_launch_gemm(gemm_params(sv.H, dff, w2, dff, out, d, n, d, dff, b2), s);
}

extern "C" int32_t amt_glu_bwd(const float* dout, const float* x, const float* saved, const float* w1t, const float* wgt, const float* w2t,
                               const float* mask_h, float* dx, float* dw1, float* db1, float* dwg, float* dbg, float* dw2, float* db2,
                               float* ws, int32_t n, int32_t d, int32_t dff, int32_t dff_raw, int32_t glu, void* stream) {
    AMT_CHECK_ARG(dout && x && saved && wgt && w2t && dx && dwg && dbg && dw2 && db2 && ws, "amt_glu_bwd: null pointer");
    AMT_CHECK_ARG(glu_shape_ok(n, d, dff, dff_raw), "amt_glu_bwd: bad shape n=%d d=%d d_ff=%d (own width %d)", n, d, dff, dff_raw);
    AMT_CHECK_ARG(!glu || (w1t && dw1 && db1), "amt_glu_bwd: a GLU expert needs w1t, dw1 and db1");
    hipStream_t s = (hipStream_t)stream;
    const GluSaved sv = glu_saved_layout(const_cast<float*>(saved), n, dff, glu);
    const GluWs w = glu_ws_layout(ws, n, d, dff);
    int32_t rc;
    // dH = dout W2, then dU (in place) and dG
    if ((rc = amt_launch_gemm(gemm_params(dout, d, w2t, d, w.dU, dff, n, dff, d, nullptr), s))) return rc;
    hipLaunchKernelGGL(moe_bwd_act_kernel, dim3(cdiv(n, 4)), dim3(256), 0, s, w.dU, w.dG, sv.G, glu ? sv.U : nullptr, mask_h, nullptr, nullptr, n, dff,
                       dff_raw);
    AMT_LAUNCH_CHECK();
    // dx = dG Wg (+ dU W1); a dense product may take the skinny kernel: the second writes its own output buffer
    GemmParams gx = gemm_params(w.dG, dff, wgt, dff, glu ? w.dXtmp : dx, d, n, d, dff, nullptr);
    if ((rc = amt_launch_gemm(gx, s))) return rc;
    if (glu) {
        gx.A = w.dU; gx.W = w1t; gx.C = dx; gx.resid = w.dXtmp; gx.ldr = d;
        if ((rc = amt_launch_gemm(gx, s))) return rc;
    }
    WgradParams q{};
    q.rows = n; q.n_groups = 1; q.S = glu_wgrad_splits(n, d, dff);
    q.P = dout; q.ldp = d; q.N = d; q.Q = sv.H; q.ldq = dff; q.K = dff; q.out = dw2; q.bias = db2;
    if ((rc = launch_wgrad(q, w.split, s))) return rc;
    q.P = w.dG; q.ldp = dff; q.N = dff; q.Q = x; q.ldq = d; q.K = d; q.out = dwg; q.bias = dbg;
    if ((rc = launch_wgrad(q, w.split, s))) return rc;
    if (glu) {
        q.P = w.dU; q.out = dw1; q.bias = db1;
        if ((rc = launch_wgrad(q, w.split, s))) return rc;
    }
    return 0;
}
