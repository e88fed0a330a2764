// Training loss of the regression head (reference utilities/run_model_regression.py:33-39, train_epoch) and its gradient in one launch:
//   loss = SmoothL1Loss()(ln_nd, [note_density | loudness]) + binary_cross_entropy(inst, instrument)
// SmoothL1 (beta 1, mean over 2 rows values): 0.5 e^2 where |e| < 1, else |e| - 0.5; gradient e or sign(e), over 2 rows.
// BCE (mean over 40 rows values) on the fp32 probability with both logs clamped at -100, as reg_metrics.hip forms it.  Its gradient
// is handed out with respect to the LOGIT: torch's binary_cross_entropy backward composed with the sigmoid's,
//   (p - t) / max((1 - p) p, 1e-12) / N * (1 - p) * p,
// in torch's order of operations: (p - t) / N to rounding where 0 < p < 1, exactly 0 where p has rounded to 0 or 1.
//
// The values (42 per row, 400 k at the reference's batch of 32 x 300 rows) are spread over up to 256 workgroups of 1024 threads,
// one per 4096 instrument values: two logs and two divisions per value keep one CU busy for 200 us at that batch, all CUs for a few.
// Workgroup b takes a contiguous range of the values, thread i of it the range's values i, i + 1024, ... in that order; the 64 lanes
// of a wave meet in the fixed DPP tree of wave_sum, thread 0 adds the 16 wave sums in wave order and leaves the workgroup's two sums in
// ws.  Thread 0 of the last workgroup (last_workgroup.h; nobody waits for anybody) adds the workgroups' sums in workgroup order.  No
// floating-point atomic: the order of every addition is a function of the row count alone, so the same inputs give the same bits.
#include "../../include/amt_hip.h"
#include "amt_common.h"
#include "last_workgroup.h"

namespace {

constexpr int N_INST = 40;
constexpr int THREADS = 1024;
constexpr int MAX_BLOCKS = 256;
constexpr int VALUES_PER_BLOCK = 4 * THREADS;

__global__ __launch_bounds__(THREADS) void reg_loss_kernel(const float* __restrict__ ln_nd, const float* __restrict__ inst,
                                                           const float* __restrict__ note_density, const float* __restrict__ loudness,
                                                           const float* __restrict__ instrument, int rows, float* __restrict__ loss,
                                                           float* __restrict__ d_ln_nd, float* __restrict__ d_logit, float* ws) {
    __shared__ float s_part[2][THREADS / 64];
    const int tid = threadIdx.x, nb = gridDim.x, b = blockIdx.x;
    const float n_reg = 2.0f * (float)rows, n_bce = (float)N_INST * (float)rows;
    float sl1 = 0.0f, bce = 0.0f;
    {                                                                // value i: row i / 2, column i & 1 (0 note density, 1 loudness)
        const int total = 2 * rows, chunk = (total + nb - 1) / nb, end = min(total, (b + 1) * chunk);
        for (int i = b * chunk + tid; i < end; i += THREADS) {
            const float e = ln_nd[i] - ((i & 1) ? loudness[i >> 1] : note_density[i >> 1]);
            const float a = fabsf(e);
            sl1 += a < 1.0f ? 0.5f * e * e : a - 0.5f;
            d_ln_nd[i] = (a < 1.0f ? e : (e > 0.0f ? 1.0f : -1.0f)) / n_reg;
        }
    }
    {
        const int total = N_INST * rows, chunk = (total + nb - 1) / nb, end = min(total, (b + 1) * chunk);
#pragma unroll 4
        for (int i = b * chunk + tid; i < end; i += THREADS) {
            const float p = inst[i], t = instrument[i];
            bce += -(t * fmaxf(logf(p), -100.0f) + (1.0f - t) * fmaxf(logf(1.0f - p), -100.0f));
            const float g = (p - t) / fmaxf((1.0f - p) * p, 1e-12f) / n_bce;
            d_logit[i] = g * (1.0f - p) * p;
        }
    }
    sl1 = wave_sum(sl1);
    bce = wave_sum(bce);
    if ((tid & 63) == 0) { s_part[0][tid >> 6] = sl1; s_part[1][tid >> 6] = bce; }
    __syncthreads();
    float* part = ws + WS_HEAD;
    if (tid == 0) {
        float a = 0.0f, c = 0.0f;
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) { a += s_part[0][w]; c += s_part[1][w]; }
        part[2 * b] = a;
        part[2 * b + 1] = c;
    }
    if (!last_workgroup(ws, nb, reinterpret_cast<unsigned*>(&s_part[0][0])) || tid != 0) return;
    float a = 0.0f, c = 0.0f;
    for (int k = 0; k < nb; ++k) { a += part[2 * k]; c += part[2 * k + 1]; }
    loss[0] = a / n_reg + c / n_bce;
    loss[1] = a / n_reg;
    loss[2] = c / n_bce;
}

}  // namespace

extern "C" int32_t amt_reg_loss_fwd_bwd(const float* ln_nd, const float* inst, const float* note_density, const float* loudness,
                                        const float* instrument, int32_t rows, float* loss, float* d_ln_nd, float* d_logit,
                                        float* ws, void* stream) {
    AMT_CHECK_ARG(ln_nd && inst && note_density && loudness && instrument && loss && d_ln_nd && d_logit, "amt_reg_loss_fwd_bwd: null pointer");
    AMT_CHECK_ARG(rows > 0 && rows <= (1 << 24), "amt_reg_loss_fwd_bwd: rows=%d must be in [1, 2^24] (the divisors 2 rows and 40 rows are exact in fp32)", rows);
    if (const int32_t rc = last_workgroup_reset(ws, "amt_reg_loss_fwd_bwd", (hipStream_t)stream)) return rc;
    static_assert(WS_HEAD + 2 * MAX_BLOCKS == AMT_REG_LOSS_WS_FLOATS, "amt_hip.h states the workspace size");
    const int64_t values = (int64_t)N_INST * rows;
    const int blocks = (int)((values + VALUES_PER_BLOCK - 1) / VALUES_PER_BLOCK < MAX_BLOCKS ? (values + VALUES_PER_BLOCK - 1) / VALUES_PER_BLOCK : MAX_BLOCKS);
    hipLaunchKernelGGL(reg_loss_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, ln_nd, inst, note_density, loudness, instrument,
                       rows, loss, d_ln_nd, d_logit, ws);
    AMT_LAUNCH_CHECK();
    return 0;
}
