// Training of the differential-attention tail (custom_transformer.py:818-826): y = RMSNorm_hd(o1 - lambda o2) w out_scale per (clip,
// head, position) row of hd values, with lambda one float in DEVICE memory (it is a function of four parameters, which change with
// every step: the eval path's host scalar would cost a synchronisation per attention per step).
//
//   amt_diff_subln_train_fwd: norm.hip's diff_subln_kernel expression for expression, lambda loaded instead of passed: for the same
//     lambda value y is amt_diff_subln_fwd's bits.
//   amt_diff_subln_bwd, hd 32 / 64 / 128: with u = o1 - lambda o2, r = rsqrt(mean(u^2) + eps), xh = u r, g = dy w out_scale
//       du = r (g - xh mean(g xh)),  d_o1 = du,  d_o2 = -lambda du,  dw = out_scale sum over rows of dy xh,  dlambda = -sum du o2
//     The row statistics are formed again from o1 / o2 (as norm_bwd.hip does from x), so nothing but the forward's inputs is kept.
//     One pass: three 16-byte loads and two 16-byte stores per lane and row.  A row takes hd / 4 lanes (8 / 4 / 2 rows per wave: no
//     lane idles at hd 32) and its two means are DPP / shuffle sums inside that lane group.  A workgroup of 4 waves takes a contiguous
//     range of the rows, wave w of it the row groups w, w + 4, ... in that order, each lane adding its columns' dw terms and its
//     share of dlambda in registers.  The waves' sums meet in LDS (row groups of a wave, then waves, in order) and go to the workgroup's
//     slab in ws, [dw (hd) | dlambda | 3 unused]; the last workgroup (last_workgroup.h) adds the slabs in workgroup order.  No
//     floating-point atomic: the order of every addition is a function of (rows, hd) alone.
#include "../../include/amt_hip.h"
#include "amt_common.h"
#include "last_workgroup.h"

namespace {

constexpr int MAX_BLOCKS = 128;
constexpr int GROUPS_PER_WAVE_AND_BLOCK = 4;    // below MAX_BLOCKS workgroups a workgroup takes 4 waves x 4 row groups; above, the rows are spread evenly

inline int rows_per_wave(int hd) { return 256 / hd; }
inline int subln_bwd_blocks(int rows, int hd) {
    const int per = 4 * GROUPS_PER_WAVE_AND_BLOCK * rows_per_wave(hd);
    return cdiv(rows, per) < MAX_BLOCKS ? cdiv(rows, per) : MAX_BLOCKS;
}

__global__ void diff_subln_dev_lambda_kernel(const float* __restrict__ o1, const float* __restrict__ o2, const float* __restrict__ w,
                                             const float* __restrict__ lambda_dev, float* __restrict__ y, int rows, int hd, float out_scale,
                                             float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float lambda = lambda_dev[0];
    const size_t base = (size_t)row * hd;
    float v[2], ss = 0.f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int c = lane + 64 * k;
        v[k] = c < hd ? o1[base + c] - lambda * o2[base + c] : 0.f;
        ss += v[k] * v[k];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float r = rsqrtf(ss / (float)hd + eps);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int c = lane + 64 * k;
        if (c < hd) y[base + c] = v[k] * r * w[c] * out_scale;
    }
}

// G = hd / 4 lanes per row
template <int G>
__global__ __launch_bounds__(256) void diff_subln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ o1,
                                                             const float* __restrict__ o2, const float* __restrict__ w,
                                                             const float* __restrict__ lambda_dev, float* __restrict__ d_o1,
                                                             float* __restrict__ d_o2, float* __restrict__ dw, float* __restrict__ dlambda,
                                                             float* ws, int rows, float out_scale, float eps) {
    constexpr int HD = 4 * G, RPW = 64 / G, SLAB = HD + 4;
    __shared__ __attribute__((aligned(16))) float s_part[4 * 256 + 4];      // per wave its lanes' float4 sums; then the 4 waves' dlambda
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nb = gridDim.x, blk = blockIdx.x;
    const int per = (rows + nb - 1) / nb, r_end = min(rows, (blk + 1) * per);
    const int sub = lane / G, c0 = (lane % G) * 4;
    const float lambda = lambda_dev[0];
    const float4 gw = ld4(w + c0);
    float4 aw = make_float4(0.f, 0.f, 0.f, 0.f);
    float al = 0.f;
    // every lane walks the loop (the trip count is the wave's); a lane group past the range's end works on zeros and stores nothing
    for (int first = blk * per + wave * RPW; first < r_end; first += 4 * RPW) {
        const int row = first + sub;
        const bool valid = row < r_end;
        const size_t base = (size_t)row * HD + c0;
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 d = valid ? ld4(dy + base) : zero, a = valid ? ld4(o1 + base) : zero, b = valid ? ld4(o2 + base) : zero;
        float4 u = make_float4(a.x - lambda * b.x, a.y - lambda * b.y, a.z - lambda * b.z, a.w - lambda * b.w);
        const float r = rsqrtf(group_sum<G>(u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w) / (float)HD + eps);
        u.x *= r; u.y *= r; u.z *= r; u.w *= r;                                                   // xh
        aw.x += d.x * u.x; aw.y += d.y * u.y; aw.z += d.z * u.z; aw.w += d.w * u.w;
        const float4 g = make_float4(d.x * gw.x * out_scale, d.y * gw.y * out_scale, d.z * gw.z * out_scale, d.w * gw.w * out_scale);
        const float m = group_sum<G>((g.x * u.x + g.y * u.y) + (g.z * u.z + g.w * u.w)) / (float)HD;
        const float4 du = make_float4(r * (g.x - u.x * m), r * (g.y - u.y * m), r * (g.z - u.z * m), r * (g.w - u.w * m));
        al += (du.x * b.x + du.y * b.y) + (du.z * b.z + du.w * b.w);
        if (valid) {
            st4(d_o1 + base, du);
            st4(d_o2 + base, make_float4(-lambda * du.x, -lambda * du.y, -lambda * du.z, -lambda * du.w));
        }
    }
    // the wave's row groups, then the 4 waves, added in order, are this workgroup's slab
    st4(&s_part[wave * 256 + lane * 4], aw);                     // lane * 4 = sub * HD + c0
    al = wave_sum(al);
    if (lane == 0) s_part[1024 + wave] = al;
    __syncthreads();
    float* slab = ws + WS_HEAD + (size_t)blk * SLAB;
    if (tid < G) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int wv = 0; wv < 4; ++wv)
#pragma unroll
            for (int s = 0; s < RPW; ++s) {
                const float4 t = ld4(&s_part[wv * 256 + s * HD + tid * 4]);
                acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
            }
        st4(slab + tid * 4, acc);
    } else if (tid == 64) {
        slab[HD] = ((s_part[1024] + s_part[1025]) + s_part[1026]) + s_part[1027];
    }
    // the flag goes through the one LDS array: its sums were read before the hand-off's first barrier
    if (!last_workgroup(ws, nb, reinterpret_cast<unsigned*>(&s_part[0]))) return;
    if (tid < G) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
        for (int k = 0; k < nb; ++k) {
            const float4 t = ld4(ws + WS_HEAD + (size_t)k * SLAB + tid * 4);
            acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
        }
        st4(dw + tid * 4, make_float4(out_scale * acc.x, out_scale * acc.y, out_scale * acc.z, out_scale * acc.w));
    } else if (tid == 64) {
        float acc = 0.f;
#pragma unroll 8
        for (int k = 0; k < nb; ++k) acc += ws[WS_HEAD + (size_t)k * SLAB + HD];
        dlambda[0] = -acc;
    }
}

static_assert(WS_HEAD + MAX_BLOCKS * (128 + 4) == AMT_DIFF_SUBLN_BWD_WS_FLOATS(128), "amt_hip.h states the workspace size");

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int32_t amt_diff_subln_train_fwd(const float* o1, const float* o2, const float* w, const float* lambda_dev, float* y,
                                            int32_t rows, int32_t hd, float out_scale, float eps, void* stream) {
    AMT_CHECK_ARG(o1 && o2 && w && lambda_dev && y, "amt_diff_subln_train_fwd: null pointer");
    AMT_CHECK_ARG(rows > 0 && hd > 0 && hd <= 128, "amt_diff_subln_train_fwd: bad shape rows=%d hd=%d", rows, hd);
    hipLaunchKernelGGL(diff_subln_dev_lambda_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, o1, o2, w, lambda_dev, y, rows, hd,
                       out_scale, eps);
    AMT_LAUNCH_CHECK();
    return 0;
}

extern "C" int32_t amt_diff_subln_bwd_blocks(int32_t rows, int32_t hd) {
    return rows > 0 && (hd == 32 || hd == 64 || hd == 128) ? subln_bwd_blocks(rows, hd) : -1;
}

extern "C" int32_t amt_diff_subln_bwd(const float* dy, const float* o1, const float* o2, const float* w, const float* lambda_dev,
                                      float* d_o1, float* d_o2, float* dw, float* dlambda, float* ws, int32_t rows, int32_t hd,
                                      float out_scale, float eps, void* stream) {
    AMT_CHECK_ARG(dy && o1 && o2 && w && lambda_dev && d_o1 && d_o2 && dw && dlambda, "amt_diff_subln_bwd: null pointer");
    AMT_CHECK_ARG(rows > 0, "amt_diff_subln_bwd: rows=%d must be positive", rows);
    AMT_CHECK_ARG(hd == 32 || hd == 64 || hd == 128, "amt_diff_subln_bwd: hd=%d must be 32, 64 or 128", hd);
    AMT_CHECK_ARG(aligned16(dy) && aligned16(o1) && aligned16(o2) && aligned16(w) && aligned16(d_o1) && aligned16(d_o2) && aligned16(dw),
                  "amt_diff_subln_bwd: dy, o1, o2, w, d_o1, d_o2 and dw must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (const int32_t rc = last_workgroup_reset(ws, "amt_diff_subln_bwd", s)) return rc;
    const dim3 grid(subln_bwd_blocks(rows, hd)), block(256);
    if (hd == 32) hipLaunchKernelGGL(diff_subln_bwd_kernel<8>, grid, block, 0, s, dy, o1, o2, w, lambda_dev, d_o1, d_o2, dw, dlambda, ws, rows, out_scale, eps);
    else if (hd == 64) hipLaunchKernelGGL(diff_subln_bwd_kernel<16>, grid, block, 0, s, dy, o1, o2, w, lambda_dev, d_o1, d_o2, dw, dlambda, ws, rows, out_scale, eps);
    else hipLaunchKernelGGL(diff_subln_bwd_kernel<32>, grid, block, 0, s, dy, o1, o2, w, lambda_dev, d_o1, d_o2, dw, dlambda, ws, rows, out_scale, eps);
    AMT_LAUNCH_CHECK();
    return 0;
}
