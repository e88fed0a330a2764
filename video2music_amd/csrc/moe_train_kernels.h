// Kernels the training paths of the feed-forward blocks share: the mixture layer (moe_bwd.hip) and the plain GLU / SiLU expert
// (family_train.hip).  The activation pair H = U silu(G) and its backward, and the grouped weight-gradient product with its split plan.
// Everything sits in an unnamed namespace: each translation unit that includes this compiles its own copy of the same code.
#pragma once
#include "amt_common.h"

namespace {

constexpr int TILE = 128;
constexpr int WGRAD_SPLIT_MAX = 32;                  // runs per group of the weight-gradient product, at most
constexpr long WGRAD_WS_FLOATS = 16L << 20;          // ... and as many as keep the partials within this many floats

inline size_t align4(size_t n) { return (n + 3) / 4 * 4; }

// H = U * silu(G) (U null: silu(G)), times the multiplier of the row's assignment; the GEMM epilogue's expressions (gemm_f32.hip).
// One wave per row; tile_group null: dense rows, the assignment is the row.
__global__ __launch_bounds__(256) void moe_act_fwd_kernel(const float* __restrict__ G, const float* __restrict__ U, float* __restrict__ H,
                                                          const float* __restrict__ mask, const int* __restrict__ slot_assign,
                                                          const int* __restrict__ tile_group, int rows, int dff, int dff_raw) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    if (tile_group && tile_group[row / TILE] < 0) return;
    const int a = slot_assign ? slot_assign[row] : row;
    for (int c = lane * 4; c < dff; c += 256) {
        const float4 g = ld4(G + (size_t)row * dff + c);
        float v[4];
        if (U) {
            const float4 u = ld4(U + (size_t)row * dff + c);
            v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
            v[0] *= g.x / (1.0f + __expf(-g.x)); v[1] *= g.y / (1.0f + __expf(-g.y));
            v[2] *= g.z / (1.0f + __expf(-g.z)); v[3] *= g.w / (1.0f + __expf(-g.w));
        } else {
            v[0] = g.x / (1.0f + __expf(-g.x)); v[1] = g.y / (1.0f + __expf(-g.y));
            v[2] = g.z / (1.0f + __expf(-g.z)); v[3] = g.w / (1.0f + __expf(-g.w));
        }
        if (mask && a >= 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (c + i < dff_raw) v[i] *= mask[(size_t)a * dff_raw + c + i];
        }
        st4(H + (size_t)row * dff + c, make_float4(v[0], v[1], v[2], v[3]));
    }
}

// dH (in dU_or_dH) -> dU (in place; GLU experts) and dG; one wave per row, rows of unused tiles are skipped
__global__ __launch_bounds__(256) void moe_bwd_act_kernel(float* __restrict__ dH, float* __restrict__ dG, const float* __restrict__ G,
                                                          const float* __restrict__ U, const float* __restrict__ mask,
                                                          const int* __restrict__ slot_assign, const int* __restrict__ tile_group, int rows,
                                                          int dff, int dff_raw) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    if (tile_group && tile_group[row / TILE] < 0) return;
    const int a = slot_assign ? slot_assign[row] : row;
    for (int c = lane * 4; c < dff; c += 256) {
        const size_t o = (size_t)row * dff + c;
        const float4 g4 = ld4(G + o), h4 = ld4(dH + o);
        const float g[4] = {g4.x, g4.y, g4.z, g4.w};
        float dh[4] = {h4.x, h4.y, h4.z, h4.w}, du[4], dg[4];
        float u[4] = {1.f, 1.f, 1.f, 1.f};
        if (U) { const float4 u4 = ld4(U + o); u[0] = u4.x; u[1] = u4.y; u[2] = u4.z; u[3] = u4.w; }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (mask && a >= 0 && c + i < dff_raw) dh[i] *= mask[(size_t)a * dff_raw + c + i];
            const float sg = 1.0f / (1.0f + __expf(-g[i]));
            du[i] = dh[i] * (g[i] * sg);                                  // dH silu(G)
            dg[i] = dh[i] * u[i] * (sg * (1.0f + g[i] * (1.0f - sg)));    // dH U silu'(G)
        }
        if (U) st4(dH + o, make_float4(du[0], du[1], du[2], du[3]));
        st4(dG + o, make_float4(dg[0], dg[1], dg[2], dg[3]));
    }
}

// ---- the grouped weight-gradient product ----
struct WgradParams {
    const float* P; int ldp;        // [rows][N]: the rows' gradients (dY, dU, dG, dlogit)
    const float* Q; int ldq;        // [rows][K], or [tokens][K] read through q_gather
    const int* q_gather;            // Q's row of row r (< 0: a padding slot, a zero row), or null
    const int* seg;                 // device: group e owns rows [seg[e], seg[e + 1]) (multiples of 128); null: one group, rows [0, rows)
    int rows;
    float* out; float* bias;        // [group][N][K], [group][N]; with S > 1 the kernel writes [z][the same two] into ws instead
    int N, K, n_groups, S;
};

__global__ __launch_bounds__(256) void moe_wgrad_kernel(WgradParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 31, fh = lane >> 5;
    const int tiles_k = (p.K + 31) / 32, tiles_n = (p.N + 31) / 32;
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= tiles_n * tiles_k) return;                   // wave-uniform; the kernel has no barrier
    const int tn = tile / tiles_k, tk = tile - tn * tiles_k;
    const int e = blockIdx.y, z = blockIdx.z;
    int r0 = p.seg ? p.seg[e] : 0, r1 = p.seg ? p.seg[e + 1] : p.rows;
    if (p.S > 1) {                                           // run z of the group's 128-row tiles, ascending
        const int per = ((r1 - r0 + TILE - 1) / TILE + p.S - 1) / p.S * TILE;
        r0 = min(r0 + z * per, r1);
        r1 = min(r0 + per, r1);
    }
    const int n = tn * 32 + fr, kk = tk * 32 + fr;
    const bool nv = n < p.N, kv = kk < p.K;
    const float* Pc = p.P + min(n, p.N - 1);
    const float* Qc = p.Q + min(kk, p.K - 1);
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    float bs = 0.f;
    constexpr int NI = 8;                                    // MFMAs per trip: 16 rows, all their loads requested before the first is used
    for (int r = r0; r < r1; r += 2 * NI) {
        float a[NI], b[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {                       // rows r + 2 i + fh: the two reduction slots of MFMA i
            const int rr = r + 2 * i + fh;
            const bool ok = rr < r1;
            const int rc = ok ? rr : r0;                     // a valid row of the run; its value is not used
            const int q = p.q_gather ? p.q_gather[rc] : rc;
            const float av = Pc[(size_t)rc * p.ldp], bv = Qc[(size_t)max(q, 0) * p.ldq];
            a[i] = ok && nv ? av : 0.f;
            b[i] = ok && kv && q >= 0 ? bv : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[i], acc, 0, 0, 0);
            bs += a[i];
        }
    }
    bs += __shfl_xor(bs, 32, 64);                            // even rows + odd rows
    float* out = p.out;
    float* bias = p.bias;
    if (p.S > 1) {
        out += (size_t)z * p.n_groups * ((size_t)p.N * p.K + p.N);
        bias = out + (size_t)p.n_groups * p.N * p.K;
    }
    out += (size_t)e * p.N * p.K;
    bias += (size_t)e * p.N;
    // C/D layout of the 32x32 tile: col = lane & 31 (Q's column), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (P's column)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int nn = tn * 32 + (i & 3) + 8 * (i >> 2) + 4 * fh;
        if (nn < p.N && kv) out[(size_t)nn * p.K + kk] = acc[i];
    }
    if (tk == 0 && fh == 0 && nv) bias[n] = bs;
}

// dst = sum over z (ascending) of the S partials; the first n_out elements go to out, the rest to bias
__global__ __launch_bounds__(256) void moe_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out, float* __restrict__ bias,
                                                               long n_out, long n_all, int S) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_all) return;
    float s = 0.f;
    for (int z = 0; z < S; ++z) s += ws[(size_t)z * n_all + i];
    if (i < n_out) out[i] = s;
    else bias[i - n_out] = s;
}

// runs per group: one per 128-row tile a group holds on average, within the cap the workspace was sized with
int wgrad_split_cap(int n_exp, int d, int dff) {
    const long cap = WGRAD_WS_FLOATS / ((long)n_exp * ((long)dff * d + (dff > d ? dff : d)));
    return (int)(cap < 1 ? 1 : cap > WGRAD_SPLIT_MAX ? WGRAD_SPLIT_MAX : cap);
}
int wgrad_splits(long row_tiles, int n_groups, int cap) {
    const long per = row_tiles / n_groups;
    return (int)(per < 1 ? 1 : per > cap ? cap : per);
}

int32_t launch_wgrad(WgradParams p, float* ws, hipStream_t s) {
    float* out = p.out;
    float* bias = p.bias;
    if (p.S > 1) p.out = ws;
    const int tiles = cdiv(p.N, 32) * cdiv(p.K, 32);
    hipLaunchKernelGGL(moe_wgrad_kernel, dim3(cdiv(tiles, 4), p.n_groups, p.S), dim3(256), 0, s, p);
    AMT_LAUNCH_CHECK();
    if (p.S > 1) {
        const long n_out = (long)p.n_groups * p.N * p.K, n_all = n_out + (long)p.n_groups * p.N;
        hipLaunchKernelGGL(moe_wgrad_reduce_kernel, dim3((unsigned)((n_all + 255) / 256)), dim3(256), 0, s, ws, out, bias, n_out, n_all, p.S);
        AMT_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace
