// Backward of the two row norms from the forward's own inputs, one kernel (norm_bwd_kernel<RMS>, as the forward is norm_kernel<RMS>):
//   amt_layernorm_bwd: y = LayerNorm(x (+ resid)) * w + b (torch.nn.LayerNorm: biased variance, eps inside the square root), the
//     post-norm step of every layer of the base model (model/rpr.py:59-69, torch's TransformerEncoderLayer) and its two final norms;
//   amt_rmsnorm_bwd:   y = RMSNorm(x (+ resid)) * w, the norm of the V1 / V2 chord models.
//
// With u = x (+ resid) and g = dy w over a row of `dim` values:
//   LayerNorm: xh = (u - mean) rstd,  du = rstd (g - mean(g) - xh mean(g xh)),  dw = sum over rows of dy xh,  db = sum over rows of dy
//   RMSNorm:   xh = u r, r = rsqrt(mean(u^2) + eps),  du = r (g - xh mean(g xh)),  dw = sum over rows of dy xh
// du is the gradient of both addends.  The row statistics are formed again from u the way norm.hip forms them (LayerNorm: two passes
// over the row held in registers; RMSNorm: norm_kernel<true>'s expression), so nothing but the forward's input is kept.  One wave per
// row, float4 lanes; a workgroup of 4 waves takes a contiguous range of the rows, wave w of it the range's rows w, w + 4, ... in that
// order, each lane adding its columns' dw (/ db) terms in registers.  The 4 waves' sums meet in LDS in wave order and go to the
// workgroup's slab in ws, [dw (dim) | db (dim)] or [dw (dim)]; the last workgroup (last_workgroup.h) adds the slabs in workgroup
// order.  No floating-point atomic: the order of every addition is a function of (rows, dim) alone.
#include "../../include/amt_hip.h"
#include "amt_common.h"
#include "last_workgroup.h"

namespace {

constexpr int CHUNKS = 4;                   // dim <= 64 lanes * 4 floats * 4 = 1024
constexpr int MAX_DIM = 64 * 4 * CHUNKS;
constexpr int MAX_BLOCKS = 128;
constexpr int ROWS_PER_BLOCK = 16;          // below MAX_BLOCKS workgroups; above, the rows are spread evenly over MAX_BLOCKS

inline int norm_bwd_blocks(int rows) { return cdiv(rows, ROWS_PER_BLOCK) < MAX_BLOCKS ? cdiv(rows, ROWS_PER_BLOCK) : MAX_BLOCKS; }

template <bool RMS>
__global__ __launch_bounds__(256) void norm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                       const float* __restrict__ resid, const float* __restrict__ w,
                                                       float* __restrict__ dx, float* __restrict__ dw, float* __restrict__ db,
                                                       float* ws, int rows, int dim, float eps) {
    constexpr int NS = RMS ? 1 : 2;          // sums per column: dw, and LayerNorm's db (db is null for RMSNorm)
    __shared__ __attribute__((aligned(16))) float s_part[4][NS][MAX_DIM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nb = gridDim.x, blk = blockIdx.x;
    const int per = (rows + nb - 1) / nb, r_end = min(rows, (blk + 1) * per);
    float4 gw[CHUNKS], aw[CHUNKS], ab[CHUNKS];
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
        const int i = (c * 64 + lane) * 4;
        gw[c] = i < dim ? ld4(w + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        aw[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        ab[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int row = blk * per + wave; row < r_end; row += 4) {
        const size_t base = (size_t)row * dim;
        float4 v[CHUNKS], g[CHUNKS];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
            const int i = (c * 64 + lane) * 4;
            if (i < dim) {
                v[c] = ld4(x + base + i);
                if (resid) {
                    const float4 r = ld4(resid + base + i);
                    v[c].x += r.x; v[c].y += r.y; v[c].z += r.z; v[c].w += r.w;
                }
                g[c] = ld4(dy + base + i);
                if (RMS) s += v[c].x * v[c].x + v[c].y * v[c].y + v[c].z * v[c].z + v[c].w * v[c].w;      // norm_kernel<true>'s expression
                else s += v[c].x + v[c].y + v[c].z + v[c].w;
            }
        }
        float mean = 0.f, rstd;
        if (RMS) {
            rstd = rsqrtf(wave_sum(s) / dim + eps);
        } else {
            mean = wave_sum(s) / dim;
            float q = 0.f;
#pragma unroll
            for (int c = 0; c < CHUNKS; ++c) {
                const int i = (c * 64 + lane) * 4;
                if (i < dim) {
                    const float a0 = v[c].x - mean, a1 = v[c].y - mean, a2 = v[c].z - mean, a3 = v[c].w - mean;
                    q += a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3;
                }
            }
            rstd = 1.0f / sqrtf(wave_sum(q) / dim + eps);
        }
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
            const int i = (c * 64 + lane) * 4;
            if (i < dim) {
                const float4 d = g[c];
                if (RMS) {
                    v[c].x *= rstd; v[c].y *= rstd; v[c].z *= rstd; v[c].w *= rstd;
                } else {
                    v[c].x = (v[c].x - mean) * rstd; v[c].y = (v[c].y - mean) * rstd;
                    v[c].z = (v[c].z - mean) * rstd; v[c].w = (v[c].w - mean) * rstd;
                }
                aw[c].x += d.x * v[c].x; aw[c].y += d.y * v[c].y; aw[c].z += d.z * v[c].z; aw[c].w += d.w * v[c].w;
                if (!RMS) { ab[c].x += d.x; ab[c].y += d.y; ab[c].z += d.z; ab[c].w += d.w; }
                g[c].x = d.x * gw[c].x; g[c].y = d.y * gw[c].y; g[c].z = d.z * gw[c].z; g[c].w = d.w * gw[c].w;
                if (!RMS) s1 += (g[c].x + g[c].y) + (g[c].z + g[c].w);
                s2 += (g[c].x * v[c].x + g[c].y * v[c].y) + (g[c].z * v[c].z + g[c].w * v[c].w);
            }
        }
        const float m1 = RMS ? 0.f : wave_sum(s1) / dim, m2 = wave_sum(s2) / dim;
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
            const int i = (c * 64 + lane) * 4;
            if (i < dim) {
                float4 o;
                if (RMS) {
                    o.x = rstd * (g[c].x - v[c].x * m2); o.y = rstd * (g[c].y - v[c].y * m2);
                    o.z = rstd * (g[c].z - v[c].z * m2); o.w = rstd * (g[c].w - v[c].w * m2);
                } else {
                    o.x = rstd * ((g[c].x - m1) - v[c].x * m2); o.y = rstd * ((g[c].y - m1) - v[c].y * m2);
                    o.z = rstd * ((g[c].z - m1) - v[c].z * m2); o.w = rstd * ((g[c].w - m1) - v[c].w * m2);
                }
                st4(dx + base + i, o);
            }
        }
    }
    // the 4 waves' column sums, added in wave order, are this workgroup's slab
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
        const int i = (c * 64 + lane) * 4;
        if (i < dim) {
            st4(&s_part[wave][0][i], aw[c]);
            if (!RMS) st4(&s_part[wave][NS - 1][i], ab[c]);
        }
    }
    __syncthreads();
    float* slab = ws + WS_HEAD + (size_t)blk * NS * dim;
    for (int f = tid * 4; f < NS * dim; f += 1024) {
        const int k = !RMS && f >= dim, i = f - k * dim;
        float4 a = ld4(&s_part[0][k][i]);
#pragma unroll
        for (int wv = 1; wv < 4; ++wv) {
            const float4 t = ld4(&s_part[wv][k][i]);
            a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
        }
        st4(slab + f, a);
    }
    // the flag goes through the one LDS array: its sums were read before the hand-off's first barrier
    if (!last_workgroup(ws, nb, reinterpret_cast<unsigned*>(&s_part[0][0][0]))) return;
    for (int f = tid * 4; f < NS * dim; f += 1024) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int k = 0; k < nb; ++k) {
            const float4 t = ld4(ws + WS_HEAD + (size_t)k * NS * dim + f);
            a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
        }
        st4(RMS || f < dim ? dw + f : db + (f - dim), a);
    }
}

template <bool RMS>
int32_t launch_norm_bwd(const char* entry, const float* dy, const float* x, const float* resid, const float* w, float* dx, float* dw, float* db,
                        float* ws, int rows, int dim, float eps, hipStream_t stream) {
    AMT_CHECK_ARG(dy && x && w && dx && dw && (RMS || db), "%s: null pointer", entry);
    AMT_CHECK_ARG(rows > 0, "%s: rows=%d must be positive", entry, rows);
    AMT_CHECK_ARG(dim > 0 && dim % 4 == 0 && dim <= MAX_DIM, "%s: dim=%d must be a multiple of 4 in [4, %d]", entry, dim, MAX_DIM);
    if (const int32_t rc = last_workgroup_reset(ws, entry, stream)) return rc;
    hipLaunchKernelGGL(norm_bwd_kernel<RMS>, dim3(norm_bwd_blocks(rows)), dim3(256), 0, stream, dy, x, resid, w, dx, dw, db, ws, rows, dim, eps);
    AMT_LAUNCH_CHECK();
    return 0;
}

static_assert(WS_HEAD + 2 * MAX_BLOCKS * MAX_DIM == AMT_LAYERNORM_BWD_WS_FLOATS(MAX_DIM), "amt_hip.h states the workspace size");
static_assert(WS_HEAD + MAX_BLOCKS * MAX_DIM == AMT_RMSNORM_BWD_WS_FLOATS(MAX_DIM), "amt_hip.h states the workspace size");

}  // namespace

extern "C" int32_t amt_rmsnorm_bwd_blocks(int32_t rows) { return rows > 0 ? norm_bwd_blocks(rows) : -1; }

extern "C" int32_t amt_layernorm_bwd(const float* dy, const float* x, const float* resid, const float* w, float* dx, float* dw, float* db,
                                     float* ws, int32_t rows, int32_t dim, float eps, void* stream) {
    return launch_norm_bwd<false>("amt_layernorm_bwd", dy, x, resid, w, dx, dw, db, ws, rows, dim, eps, (hipStream_t)stream);
}

extern "C" int32_t amt_rmsnorm_bwd(const float* dy, const float* x, const float* resid, const float* w, float* dx, float* dw, float* ws,
                                   int32_t rows, int32_t dim, float eps, void* stream) {
    return launch_norm_bwd<true>("amt_rmsnorm_bwd", dy, x, resid, w, dx, dw, nullptr, ws, rows, dim, eps, (hipStream_t)stream);
}
