// Test-split figures of the regression head (reference utilities/run_model_regression.py:70-125, eval_model): the two heads of
// model/video_regression.py:240-245 applied to the encoder output and reduced against the targets in one pass on the device,
// instead of two head GEMMs, a sigmoid, a concat, three mse_loss, one binary_cross_entropy and four float() reads per clip.
//
// One workgroup per clip, 16 rows per wave.  The heads are a (16 rows) x (W) x (48 >= 42 outputs) product on the fp32 matrix pipe:
// three v_mfma_f32_16x16x4_f32 accumulators (output columns 0..15, 16..31, 32..47; 0..39 the instrument logits, 40 note density,
// 41 loudness), each a k-ordered fp32 fma chain.  Eight columns of the rows per step: lane (row l & 15, group l >> 4) reads
// x[row][k0 + 2 group + {0, 1}] (asked for one step ahead; the other waves of the SIMD cover what latency remains) and the matching rows of w_t,
// the host's transposed, 64-wide packed copy of both heads, streamed through L1 / L2.  One code path for every width.  The
// accumulators leave output column l & 15 (+ 16 t) of rows 4 (l >> 4) + i in register i, so a row's 40 BCE terms are three
// in-lane adds and one 16-lane DPP tree.  The per-row sums go to LDS and lanes 0..2 of wave 0 add them in row order, so a
// clip's sums depend neither on the wave count nor on timing (no floating-point atomics).
#include "../../include/amt_hip.h"
#include "amt_common.h"

namespace {

constexpr int N_INST = 40;                  // utilities/constants.py:84 INSTRUMENT_SIZE
constexpr int N_OUT = N_INST + 2;           // + note density, loudness
constexpr int WT_LD = 64;                   // row stride of the packed heads: one dword per lane
constexpr int MAX_W = 1024;
constexpr int CHUNK = 1024;                 // rows whose sums wait in LDS for the ordered pass
constexpr int MAX_WAVES = 16;
constexpr int TILE = 16;                    // rows per wave and pass: one MFMA tile

__global__ __launch_bounds__(64 * MAX_WAVES) void reg_metrics_kernel(
        const float* __restrict__ feat, int ld, int W, const float* __restrict__ w_t, const float* __restrict__ note_density,
        const float* __restrict__ loudness, const float* __restrict__ instrument, int S, float* __restrict__ clip_out,
        float* __restrict__ ln_nd_out, float* __restrict__ inst_out) {
    __shared__ float s_val[3][CHUNK];       // per row: squared error of note density, of loudness, BCE sum
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int rl = lane & 15, g = lane >> 4;
    const size_t row0 = (size_t)blockIdx.x * S;
    float bias[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) bias[t] = w_t[(size_t)W * WT_LD + 16 * t + rl];
    float sum = 0.0f;                       // wave 0: lanes 0 / 1 / 2 hold the clip's three sums

    for (int base = 0; base < S; base += CHUNK) {
        const int n = min(CHUNK, S - base);
        for (int r = wave * TILE; r < n; r += nw * TILE) {
            // A operand: x[row rl][k0 + 2 g + j]; B operand: w_t[k0 + 2 g + j][16 t + rl]; j = 0, 1 are two MFMAs.  Rows past the
            // clip's last repeat it; their results are dropped
            const float* xp = feat + (row0 + base + min(r + rl, n - 1)) * ld + 2 * g;
            const float* wp = w_t + (size_t)(2 * g) * WT_LD + rl;
            f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            float a0 = xp[0], a1 = xp[1];
            for (int k0 = 0; k0 < W; k0 += 8) {
                const int kn = k0 + 8 < W ? k0 + 8 : k0;        // the last step reloads its own columns
                const float n0 = xp[kn], n1 = xp[kn + 1];
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, wp[(size_t)k0 * WT_LD + 16 * t], acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, wp[(size_t)(k0 + 1) * WT_LD + 16 * t], acc[t], 0, 0, 0);
                }
                a0 = n0; a1 = n1;
            }
            // register i of acc[t]: output 16 t + rl of row r + 4 g + i
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rr = r + 4 * g + i;
                const bool valid = rr < n;
                const size_t row = row0 + base + min(rr, n - 1);
                float s = 0.0f;
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const int col = 16 * t + rl;
                    const float y = acc[t][i] + bias[t];
                    if (col < N_INST) {
                        // torch's binary_cross_entropy on the fp32 probability, logs clamped at -100: a saturated p gives exactly 100
                        const float p = 1.0f / (1.0f + expf(-y));
                        const float tg = instrument[row * N_INST + col];
                        s += -(tg * fmaxf(logf(p), -100.0f) + (1.0f - tg) * fmaxf(logf(1.0f - p), -100.0f));
                        if (inst_out && valid) inst_out[row * N_INST + col] = p;
                    } else if (col < N_OUT && valid) {
                        const float e = y - (col == N_INST ? note_density[row] : loudness[row]);
                        s_val[col - N_INST][rr] = e * e;
                        if (ln_nd_out) ln_nd_out[row * 2 + (col - N_INST)] = y;
                    }
                }
                s = row_sum16(s);           // the 16 lanes of a group hold one row's outputs
                if (valid && rl == 0) s_val[2][rr] = s;
            }
        }
        __syncthreads();
        if (wave == 0 && lane < 3) {
#pragma unroll 8
            for (int r = 0; r < n; ++r) sum += s_val[lane][r];       // row order: the same sum whatever the wave count; reads run ahead
        }
        __syncthreads();
    }
    if (wave == 0 && lane < 4) clip_out[(size_t)blockIdx.x * 4 + lane] = lane < 3 ? sum : (float)S;
}

}  // namespace

extern "C" int32_t amt_reg_metrics_fwd(const float* feat, int32_t ld, int32_t W, const float* w_heads, const float* note_density,
                                       const float* loudness, const float* instrument, int32_t B, int32_t S, float* clip_out,
                                       float* ln_nd_out, float* inst_out, void* stream) {
    AMT_CHECK_ARG(feat && w_heads && note_density && loudness && instrument && clip_out, "amt_reg_metrics_fwd: null pointer");
    AMT_CHECK_ARG(W > 0 && W % 8 == 0 && W <= MAX_W, "amt_reg_metrics_fwd: width %d is not a positive multiple of 8 up to %d", W, MAX_W);
    AMT_CHECK_ARG(ld >= W, "amt_reg_metrics_fwd: row stride %d is below the width %d", ld, W);
    AMT_CHECK_ARG(B > 0 && S > 0, "amt_reg_metrics_fwd: B=%d, S=%d must be positive", B, S);
    AMT_CHECK_ARG(S <= (1 << 24) && (int64_t)B * S <= INT32_MAX, "amt_reg_metrics_fwd: B=%d x S=%d rows: the row count is exact in fp32 up to S = 2^24", B, S);
    const int waves = cdiv(S, TILE) < MAX_WAVES ? cdiv(S, TILE) : MAX_WAVES;
    hipLaunchKernelGGL(reg_metrics_kernel, dim3(B), dim3(64 * waves), 0, (hipStream_t)stream, feat, ld, W, w_heads, note_density,
                       loudness, instrument, S, clip_out, ln_nd_out, inst_out);
    AMT_LAUNCH_CHECK();
    return 0;
}
