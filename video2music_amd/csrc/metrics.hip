// Test-split chord metrics of the reference's evaluation (dataset/vevo_dataset.py:653-701,747-810: compute_vevo_accuracy,
// compute_hits_k, compute_vevo_correspondence; utilities/run_model_vevo.py:306-332: CrossEntropyLoss(ignore_index=CHORD_PAD) and
// BCEWithLogitsLoss against the emotion rows of dataset/vevo_dataset.py:461-515), computed from the (B, L, 159) logits in one
// pass on the device instead of Python loops with one .item() per token.
//
// One workgroup per clip, one wave per row: the wave reads the row's 159 logits once (lane-strided dwords, the next row's loads in
// flight under this row's arithmetic) and reduces them with the wave trees of amt_common.h.  The per-row cross-entropy and BCE
// sums go to LDS; lanes 0 / 1 of wave 0 then add them in row order, so a clip's sums depend neither on the wave count nor on
// timing (no floating-point atomics; the integer counts are exact in any order).  HBM-bound: 636 bytes per row.
#include "../../include/amt_hip.h"
#include "amt_common.h"
#include "chord_rows.h"

namespace {

constexpr int CHUNK = 1024;                             // rows whose sums wait in LDS for the ordered pass
constexpr int MAX_WAVES = 16;
constexpr int N_NEUTRAL = 5;

enum { C_VALID, C_TOP1, C_HIT1, C_HIT3, C_HIT5, C_COUNTED, C_RIGHT, N_COUNTS };

__global__ __launch_bounds__(64 * MAX_WAVES) void chord_metrics_kernel(
        const float* __restrict__ logits, int ld, const int64_t* __restrict__ tgt, const int32_t* __restrict__ emo_class,
        const float* __restrict__ emo_prob, float emo_threshold, int L, float* __restrict__ clip_out,
        int32_t* __restrict__ pred_out, int32_t* __restrict__ rank_out, float* __restrict__ ce_out) {
    __shared__ float s_val[2][CHUNK];       // [0]: cross-entropy of the row (0 for an ignored one), [1]: its BCE sum
    __shared__ int s_cnt[N_COUNTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const size_t row0 = (size_t)blockIdx.x * L;
    if (threadIdx.x < N_COUNTS) s_cnt[threadIdx.x] = 0;
    int cnt[N_COUNTS] = {0, 0, 0, 0, 0, 0, 0};      // this wave's counts (wave-uniform)
    float acc = 0.0f;                               // wave 0: lane 0 the clip's cross-entropy sum, lane 1 its BCE sum
    const bool has2 = lane < NC - 128;
    const int q0 = (lane + 12) % 13, q1 = (lane + 63) % 13, q2 = (lane + 127) % 13;   // (j - 1) % 13 of this lane's three classes

    for (int base = 0; base < L; base += CHUNK) {
        const int n = min(CHUNK, L - base);
        float y0 = 0.f, y1 = 0.f, y2 = 0.f;
        if (wave < n) load_row(logits + (row0 + base + wave) * ld, lane, y0, y1, y2);
        for (int r = wave; r < n; r += nw) {
            float n0 = 0.f, n1 = 0.f, n2 = 0.f;
            if (r + nw < n) load_row(logits + (row0 + base + r + nw) * ld, lane, n0, n1, n2);
            const size_t row = row0 + base + r;
            const int64_t t64 = tgt[row];
            const int t = __builtin_amdgcn_readfirstlane(t64 >= 0 && t64 < NC ? (int)t64 : ID_PAD);   // an id outside the vocabulary is ignored like PAD
            const int emo = emo_class[row];
            const float prob = emo_prob[row];
            const bool chord = t < ID_END;
            const uint32_t qm = quality_mask(emo);

            // arg-max, lowest index among equal maxima
            const float m = wave_max(fmaxf(fmaxf(y0, y1), y2));
            const int cand = y0 == m ? lane : y1 == m ? lane + 64 : (has2 && y2 == m) ? lane + 128 : 4 * NC;
            int pred = (int)-wave_max(-(float)cand);
            if (pred >= NC) pred = 0;               // a row of NaNs

            // rank of the target: classes above it, equal ones before it
            const float ysel = t < 64 ? y0 : t < 128 ? y1 : y2;
            const float yt = readlane_f(ysel, t & 63);
            const int above = (int)(y0 > yt || (y0 == yt && lane < t)) + (int)(y1 > yt || (y1 == yt && lane + 64 < t)) +
                              (int)(has2 && (y2 > yt || (y2 == yt && lane + 128 < t)));
            const int rank = (int)wave_sum((float)above);

            // cross-entropy, max-subtracted
            const float se = wave_sum((expf(y0 - m) + expf(y1 - m)) + (has2 ? expf(y2 - m) : 0.0f));
            const float ce = logf(se) - (yt - m);           // not (m + log se) - yt: see chord_loss.hip

            // BCE against the emotion row of the target's second
            const bool t0 = chord && lane != 0 && ((qm >> q0) & 1u);
            const bool t1 = chord && ((qm >> q1) & 1u);
            const bool t2 = lane + 128 == ID_END ? t == ID_END : lane + 128 == ID_PAD ? t == ID_PAD : (chord && ((qm >> q2) & 1u));
            const float bce = wave_sum((bce_term(y0, t0) + bce_term(y1, t1)) + (has2 ? bce_term(y2, t2) : 0.0f));

            const bool valid = t != ID_PAD;
            const bool counted = chord && emo >= 0 && emo < N_NEUTRAL && !(prob < emo_threshold);
            const int q = pred == 0 ? 1 : (pred - 1) % 13 + 1;       // "N" has one part, which the reference reads as maj (:790-792)
            const bool right = counted && pred < ID_END && ((qm >> (q - 1)) & 1u);
            cnt[C_VALID] += valid;
            cnt[C_TOP1] += valid && pred == t;
            cnt[C_HIT1] += valid && rank < 1;
            cnt[C_HIT3] += valid && rank < 3;
            cnt[C_HIT5] += valid && rank < 5;
            cnt[C_COUNTED] += counted;
            cnt[C_RIGHT] += right;
            if (lane == 0) {
                s_val[0][r] = valid ? ce : 0.0f;
                s_val[1][r] = bce;
                if (pred_out) pred_out[row] = pred;
                if (rank_out) rank_out[row] = rank;
                if (ce_out) ce_out[row] = valid ? ce : 0.0f;
            }
            y0 = n0; y1 = n1; y2 = n2;
        }
        __syncthreads();
        if (wave == 0 && lane < 2)
            for (int r = 0; r < n; ++r) acc += s_val[lane][r];       // row order: the same sum whatever the wave count
        __syncthreads();
    }
    if (lane == 0)
        for (int k = 0; k < N_COUNTS; ++k) atomicAdd(&s_cnt[k], cnt[k]);     // integer LDS adds: exact in any order
    __syncthreads();
    if (wave == 0) {
        const float ce_sum = readlane_f(acc, 0), bce_sum = readlane_f(acc, 1);
        if (lane == 0) {
            float* o = clip_out + (size_t)blockIdx.x * 10;
            o[0] = (float)s_cnt[C_VALID];
            o[1] = (float)s_cnt[C_TOP1];
            o[2] = (float)s_cnt[C_HIT1];
            o[3] = (float)s_cnt[C_HIT3];
            o[4] = (float)s_cnt[C_HIT5];
            o[5] = ce_sum;
            o[6] = bce_sum;
            o[7] = (float)s_cnt[C_COUNTED];
            o[8] = (float)s_cnt[C_RIGHT];
            o[9] = (float)L;
        }
    }
}

}  // namespace

extern "C" int32_t amt_chord_metrics_fwd(const float* logits, int32_t ld, const int64_t* tgt, const int32_t* emo_class,
                                         const float* emo_prob, float emo_threshold, int32_t B, int32_t L, float* clip_out,
                                         int32_t* pred_out, int32_t* rank_out, float* ce_out, void* stream) {
    AMT_CHECK_ARG(logits && tgt && emo_class && emo_prob && clip_out, "amt_chord_metrics_fwd: null pointer");
    AMT_CHECK_ARG(ld >= NC, "amt_chord_metrics_fwd: row stride %d is below the %d classes of a row", ld, NC);
    AMT_CHECK_ARG(B > 0 && L > 0, "amt_chord_metrics_fwd: B=%d, L=%d must be positive", B, L);
    AMT_CHECK_ARG(L <= (1 << 24) && (int64_t)B * L <= INT32_MAX, "amt_chord_metrics_fwd: B=%d x L=%d rows: counts are exact in fp32 up to L = 2^24", B, L);
    const int waves = L < MAX_WAVES ? L : MAX_WAVES;
    hipLaunchKernelGGL(chord_metrics_kernel, dim3(B), dim3(64 * waves), 0, (hipStream_t)stream, logits, ld, tgt, emo_class,
                       emo_prob, emo_threshold, L, clip_out, pred_out, rank_out, ce_out);
    AMT_LAUNCH_CHECK();
    return 0;
}
