// Backward of y = LayerNorm(x (+ resid)) * w + b (torch.nn.LayerNorm: biased variance, eps inside the square root), the post-norm
// step of every layer of the base model (model/rpr.py:59-69, torch's TransformerEncoderLayer) and its two final norms.
//
// With u = x (+ resid), xh = (u - mean) rstd and g = dy w over a row of `dim` values:
//   du = rstd (g - mean(g) - xh mean(g xh))         (the gradient of both addends)
//   dw = sum over rows of dy xh,   db = sum over rows of dy
// The row statistics are formed again from u the way norm.hip forms them (two passes over the row held in registers), so nothing but
// the forward's input is kept.  One wave per row, float4 lanes; a workgroup of 4 waves takes a contiguous range of the rows, wave w
// of it the range's rows w, w + 4, ... in that order, each lane adding its columns' dw / db terms in registers.  The 4 waves' sums
// meet in LDS in wave order and go to the workgroup's slab in ws; the workgroup that draws the last ticket of ws's counter adds the
// slabs in workgroup order.  No floating-point atomic: the order of every addition is a function of (rows, dim) alone.
#include "../../include/amt_hip.h"
#include "amt_common.h"

namespace {

constexpr int CHUNKS = 4;                   // dim <= 64 lanes * 4 floats * 4 = 1024
constexpr int MAX_DIM = 64 * 4 * CHUNKS;
constexpr int MAX_BLOCKS = 128;
constexpr int ROWS_PER_BLOCK = 16;          // below MAX_BLOCKS workgroups; above, the rows are spread evenly over MAX_BLOCKS
constexpr int WS_HEAD = 4;                  // ws[0]: the ticket counter (a block of 16 bytes, zeroed before every launch)

__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                            const float* __restrict__ resid, const float* __restrict__ w,
                                                            float* __restrict__ dx, float* __restrict__ dw, float* __restrict__ db,
                                                            float* ws, int rows, int dim, float eps) {
    __shared__ __attribute__((aligned(16))) float s_part[4][2][MAX_DIM];
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
                s += v[c].x + v[c].y + v[c].z + v[c].w;
            }
        }
        const float mean = wave_sum(s) / dim;
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
            const int i = (c * 64 + lane) * 4;
            if (i < dim) {
                const float a0 = v[c].x - mean, a1 = v[c].y - mean, a2 = v[c].z - mean, a3 = v[c].w - mean;
                q += a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3;
            }
        }
        const float rstd = 1.0f / sqrtf(wave_sum(q) / dim + eps);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
            const int i = (c * 64 + lane) * 4;
            if (i < dim) {
                const float4 d = g[c];
                v[c].x = (v[c].x - mean) * rstd; v[c].y = (v[c].y - mean) * rstd;
                v[c].z = (v[c].z - mean) * rstd; v[c].w = (v[c].w - mean) * rstd;
                aw[c].x += d.x * v[c].x; aw[c].y += d.y * v[c].y; aw[c].z += d.z * v[c].z; aw[c].w += d.w * v[c].w;
                ab[c].x += d.x; ab[c].y += d.y; ab[c].z += d.z; ab[c].w += d.w;
                g[c].x = d.x * gw[c].x; g[c].y = d.y * gw[c].y; g[c].z = d.z * gw[c].z; g[c].w = d.w * gw[c].w;
                s1 += (g[c].x + g[c].y) + (g[c].z + g[c].w);
                s2 += (g[c].x * v[c].x + g[c].y * v[c].y) + (g[c].z * v[c].z + g[c].w * v[c].w);
            }
        }
        const float m1 = wave_sum(s1) / dim, m2 = wave_sum(s2) / dim;
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
            const int i = (c * 64 + lane) * 4;
            if (i < dim) {
                float4 o;
                o.x = rstd * ((g[c].x - m1) - v[c].x * m2); o.y = rstd * ((g[c].y - m1) - v[c].y * m2);
                o.z = rstd * ((g[c].z - m1) - v[c].z * m2); o.w = rstd * ((g[c].w - m1) - v[c].w * m2);
                st4(dx + base + i, o);
            }
        }
    }
    // the 4 waves' column sums, added in wave order, are this workgroup's slab: [dw (dim) | db (dim)]
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
        const int i = (c * 64 + lane) * 4;
        if (i < dim) {
            st4(&s_part[wave][0][i], aw[c]);
            st4(&s_part[wave][1][i], ab[c]);
        }
    }
    __syncthreads();
    float* slab = ws + WS_HEAD + (size_t)blk * 2 * dim;
    for (int f = tid * 4; f < 2 * dim; f += 1024) {
        const int k = f >= dim, i = f - k * dim;
        float4 a = ld4(&s_part[0][k][i]);
#pragma unroll
        for (int wv = 1; wv < 4; ++wv) {
            const float4 t = ld4(&s_part[wv][k][i]);
            a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
        }
        st4(slab + f, a);
    }
    // publish the slab, then draw a ticket: every wave's stores have landed before lane 0's agent-scope release
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned ticket = __hip_atomic_fetch_add(reinterpret_cast<unsigned*>(ws), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = ticket == (unsigned)nb - 1;
        s_part[0][0][0] = last ? 1.0f : 0.0f;              // "I am last" goes through the one LDS array: its sums were read before the barrier above
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (s_part[0][0][0] == 0.0f) return;
    for (int f = tid * 4; f < 2 * dim; f += 1024) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int k = 0; k < nb; ++k) {
            const float4 t = ld4(ws + WS_HEAD + (size_t)k * 2 * dim + f);
            a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
        }
        st4(f < dim ? dw + f : db + (f - dim), a);
    }
}

}  // namespace

extern "C" int32_t amt_layernorm_bwd(const float* dy, const float* x, const float* resid, const float* w, float* dx, float* dw, float* db,
                                     float* ws, int32_t rows, int32_t dim, float eps, void* stream) {
    AMT_CHECK_ARG(dy && x && w && dx && dw && db && ws, "amt_layernorm_bwd: null pointer");
    AMT_CHECK_ARG(rows > 0, "amt_layernorm_bwd: rows=%d must be positive", rows);
    AMT_CHECK_ARG(dim > 0 && dim % 4 == 0 && dim <= MAX_DIM, "amt_layernorm_bwd: dim=%d must be a multiple of 4 in [4, %d]", dim, MAX_DIM);
    AMT_CHECK_ARG(((uintptr_t)ws & 15) == 0, "amt_layernorm_bwd: ws must be 16-byte aligned");
    static_assert(WS_HEAD + 2 * MAX_BLOCKS * MAX_DIM == AMT_LAYERNORM_BWD_WS_FLOATS(MAX_DIM), "amt_hip.h states the workspace size");
    const int blocks = cdiv(rows, ROWS_PER_BLOCK) < MAX_BLOCKS ? cdiv(rows, ROWS_PER_BLOCK) : MAX_BLOCKS;
    AMT_HIP(hipMemsetAsync(ws, 0, WS_HEAD * sizeof(float), (hipStream_t)stream));
    hipLaunchKernelGGL(layernorm_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dy, x, resid, w, dx, dw, db, ws, rows, dim, eps);
    AMT_LAUNCH_CHECK();
    return 0;
}
