// Training loss of the chord model (reference utilities/run_model_vevo.py:101-119, train_epoch) and its gradient in one launch:
//   total = lambda CrossEntropyLoss(ignore_index=CHORD_PAD, label_smoothing=eps)(y, tgt) + (1 - lambda) BCEWithLogitsLoss()(y, tgt_emotion)
// on the (B L, 159) logits, with the emotion rows built from (tgt, emo_class) exactly as amt_chord_metrics_fwd builds them.
//
// One wave per row, as in metrics.hip: the row's 159 logits sit in three registers per lane and are reduced by the wave trees of
// amt_common.h.  A workgroup of 16 waves takes 64 consecutive rows of ONE clip (a clip is ceil(L / 64) workgroups), so that the
// per-clip sums the epoch figures need come out of the same launch: the rows' two sums go to LDS, lanes 0 / 1 of wave 0 add them in
// row order and leave the workgroup's {ce, bce, n_valid} in ws.  The last workgroup (last_workgroup.h) adds
// the workgroups of each clip in order (clip_out), then the clips in order (loss).  The gradient's chord part is divided by the
// batch's count of valid targets, which every workgroup counts for itself from tgt (integers: exact in any order; B L <= 10^5 ids out
// of L2) before its rows, so that dlogits needs no second launch.  No floating-point atomic: the order of every addition is a function
// of (B, L) alone, and forward-only mode (dlogits null) runs the same additions, so loss and clip_out are the same bits either way.
#include "../../include/amt_hip.h"
#include "amt_common.h"
#include "chord_rows.h"
#include "last_workgroup.h"

namespace {

constexpr int WAVES = 16, THREADS = 64 * WAVES;
constexpr int ROWS = 64;                    // rows per workgroup

__global__ __launch_bounds__(THREADS) void chord_loss_kernel(const float* __restrict__ logits, int ld, const int64_t* __restrict__ tgt,
                                                             const int32_t* __restrict__ emo_class, int B, int L, float lambda, float smoothing,
                                                             float* __restrict__ loss, float* __restrict__ clip_out, float* __restrict__ dlogits,
                                                             float* ws) {
    __shared__ float s_val[2][ROWS];        // [0]: the row's smoothed cross-entropy (0 for an ignored one), [1]: its BCE sum
    __shared__ int s_cnt[3];                // [0]: valid targets among this workgroup's rows, [1]: in the whole batch, [2]: last to finish
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int spc = (L + ROWS - 1) / ROWS;                 // workgroups per clip
    const int clip = blockIdx.x / spc, l0 = (blockIdx.x % spc) * ROWS, n = min(ROWS, L - l0);
    const size_t row0 = (size_t)clip * L + l0;
    const int n_rows = B * L;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    float inv_valid = 0.0f;
    if (dlogits) {
        int c = 0;
        for (int i = tid; i < n_rows; i += THREADS) {
            const int64_t t = tgt[i];
            c += (t >= 0 && t < NC && t != ID_PAD);
        }
        c = (int)wave_sum((float)c);                        // at most 64 ceil(n_rows / 1024): exact
        if (lane == 0) atomicAdd(&s_cnt[1], c);             // integer LDS adds: exact in any order
        __syncthreads();
        inv_valid = 1.0f / (float)s_cnt[1];
    }
    const float inv_bce = 1.0f / ((float)n_rows * (float)NC);
    const bool has2 = lane < NC - 128;
    const int q0 = (lane + 12) % 13, q1 = (lane + 63) % 13, q2 = (lane + 127) % 13;   // (j - 1) % 13 of this lane's three classes
    int valid_cnt = 0;
    for (int r = wave; r < n; r += WAVES) {
        const size_t row = row0 + r;
        float y0, y1, y2;
        load_row(logits + row * ld, lane, y0, y1, y2);
        const int64_t t64 = tgt[row];
        const int t = __builtin_amdgcn_readfirstlane(t64 >= 0 && t64 < NC ? (int)t64 : ID_PAD);   // an id outside the vocabulary is ignored like PAD
        const bool valid = t != ID_PAD, chord = t < ID_END;
        const uint32_t qm = quality_mask(emo_class[row]);

        // log-softmax, max-subtracted: -log p_c = log se - (y_c - m).  m + log se is never formed: at logits of 1000 its spacing, 6e-5,
        // would be the error of every row's loss, whatever the loss's size.  -sum_c log p_c = 159 log se - sum_c (y_c - m)
        const float m = wave_max(fmaxf(fmaxf(y0, y1), y2));
        const float e0 = expf(y0 - m), e1 = expf(y1 - m), e2 = has2 ? expf(y2 - m) : 0.0f;
        const float se = wave_sum((e0 + e1) + e2);
        const float lse = logf(se);
        const float ysel = t < 64 ? y0 : t < 128 ? y1 : y2;
        const float nll = lse - (readlane_f(ysel, t & 63) - m);
        float ce = nll;
        if (smoothing != 0.0f) {
            const float sy = wave_sum(((y0 - m) + (y1 - m)) + (has2 ? y2 - m : 0.0f));
            ce = (1.0f - smoothing) * nll + smoothing * (((float)NC * lse - sy) / (float)NC);
        }

        // BCE against the emotion row of the target's second
        const bool t0 = chord && lane != 0 && ((qm >> q0) & 1u);
        const bool t1 = chord && ((qm >> q1) & 1u);
        const bool t2 = lane + 128 == ID_END ? t == ID_END : lane + 128 == ID_PAD ? t == ID_PAD : (chord && ((qm >> q2) & 1u));
        const float bce = wave_sum((bce_term(y0, t0) + bce_term(y1, t1)) + (has2 ? bce_term(y2, t2) : 0.0f));

        valid_cnt += valid;
        if (lane == 0) {
            s_val[0][r] = valid ? ce : 0.0f;
            s_val[1][r] = bce;
        }
        if (dlogits) {
            float* g = dlogits + row * NC;
            const float inv_se = 1.0f / se, cs = valid ? lambda * inv_valid : 0.0f, bs = (1.0f - lambda) * inv_bce;
            const float off = smoothing / (float)NC, hit = 1.0f - smoothing;
            auto grad = [&](float y, float e, int j, bool tj) {
                const float soft = (e * inv_se - (j == t ? hit : 0.0f)) - off;
                const float sig = 1.0f / (1.0f + expf(-y));
                return (valid ? cs * soft : 0.0f) + bs * (sig - (tj ? 1.0f : 0.0f));
            };
            g[lane] = grad(y0, e0, lane, t0);
            g[lane + 64] = grad(y1, e1, lane + 64, t1);
            if (has2) g[lane + 128] = grad(y2, e2, lane + 128, t2);
        }
    }
    if (lane == 0) atomicAdd(&s_cnt[0], valid_cnt);
    __syncthreads();
    float acc = 0.0f;
    if (wave == 0 && lane < 2)
        for (int r = 0; r < n; ++r) acc += s_val[lane][r];           // row order: the same sum whatever the wave count
    float* part = ws + WS_HEAD;
    if (wave == 0) {
        if (lane < 2) part[3 * blockIdx.x + lane] = acc;
        if (lane == 2) part[3 * blockIdx.x + 2] = (float)s_cnt[0];
    }
    if (!last_workgroup(ws, gridDim.x, reinterpret_cast<unsigned*>(&s_cnt[2])) || tid != 0) return;
    float ce_all = 0.0f, bce_all = 0.0f, valid_all = 0.0f;
    for (int b = 0; b < B; ++b) {
        float ce = 0.0f, bce = 0.0f, nv = 0.0f;
        for (int s = 0; s < spc; ++s) {
            const float* q = part + 3 * (b * spc + s);
            ce += q[0]; bce += q[1]; nv += q[2];
        }
        float* o = clip_out + 4 * b;
        o[0] = nv; o[1] = ce; o[2] = bce; o[3] = (float)L;
        ce_all += ce; bce_all += bce; valid_all += nv;
    }
    const float chord = ce_all / valid_all, emotion = bce_all * inv_bce;     // no valid target in the batch: NaN, as torch gives
    loss[0] = lambda * chord + (1.0f - lambda) * emotion;
    loss[1] = chord;
    loss[2] = emotion;
}

}  // namespace

extern "C" int64_t amt_chord_loss_ws_floats(int32_t B, int32_t L) {
    if (B <= 0 || L <= 0) return 0;
    return WS_HEAD + 3 * (int64_t)B * ((L + ROWS - 1) / ROWS);
}

extern "C" int32_t amt_chord_loss_fwd_bwd(const float* logits, int32_t ld, const int64_t* tgt, const int32_t* emo_class, int32_t B,
                                          int32_t L, float lambda, float smoothing, float* loss, float* clip_out, float* dlogits,
                                          float* ws, void* stream) {
    AMT_CHECK_ARG(logits && tgt && emo_class && loss && clip_out, "amt_chord_loss_fwd_bwd: null pointer");
    AMT_CHECK_ARG(ld >= NC, "amt_chord_loss_fwd_bwd: row stride %d is below the %d classes of a row", ld, NC);
    AMT_CHECK_ARG(B > 0 && L > 0, "amt_chord_loss_fwd_bwd: B=%d, L=%d must be positive", B, L);
    AMT_CHECK_ARG((int64_t)B * L * NC <= (1 << 24), "amt_chord_loss_fwd_bwd: B=%d x L=%d rows: the divisor 159 B L is exact in fp32 up to 2^24", B, L);
    AMT_CHECK_ARG(smoothing >= 0.0f && smoothing < 1.0f, "amt_chord_loss_fwd_bwd: smoothing=%g must be in [0, 1)", (double)smoothing);
    if (const int32_t rc = last_workgroup_reset(ws, "amt_chord_loss_fwd_bwd", (hipStream_t)stream)) return rc;
    const int blocks = B * ((L + ROWS - 1) / ROWS);
    hipLaunchKernelGGL(chord_loss_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, logits, ld, tgt, emo_class, B, L, lambda,
                       smoothing, loss, clip_out, dlogits, ws);
    AMT_LAUNCH_CHECK();
    return 0;
}
