// The chord training loss with the reference's -auxiliary_loss (train.py:221-229, model/loss.py:85-141):
//   chord = (CE + A_3 + A_5) / count,   A_k = w_k sum_{valid rows} relu(mean(top-k of p) - p_t) / n_valid,   (k, w_k) = (3, 3), (5, 5)
//   total = w_chord chord + w_emotion BCEWithLogitsLoss()(y, tgt_emotion)
// with CE and BCE exactly what chord_loss.hip forms on the natural rows, p the softmax of an auxiliary row and count the number of the
// three fp32 terms above 1e-10 -- a constant under differentiation that is known only after the batch-wide sum.
//
// The auxiliary rows come in two layouts.  AMT_CHORD_AUX_ROWS: row (b, l) is logits[b, l, :159], what eval_model hands the loss.
// AMT_CHORD_AUX_VIEW: what train_epoch hands it, the (B, C, L) permute RESHAPED to (B, L, C): row (b, r) is the 159 consecutive
// elements f = 159 r + j of the clip's class-major flattening, element j = logits[b, f % L, f / L], paired with tgt[b, r].
//
// Launch 1, chord_aux_kernel: chord_loss.hip's grid and row schedule (B ceil(L / 64) workgroups of 16 waves; a workgroup takes 64
// consecutive row indices of one clip, a wave one index at a time).  For an index the wave reads the natural row (CE, BCE) and the
// auxiliary row of the same index -- the same registers in the rows layout, three lane-strided gathers in the view layout: lane j
// reads logits[b, f % L, f / L], neighbouring lanes neighbouring l, so one load touches 64 lines of the clip's slab, which sits in L2
// (6 MB at (32, 299)); an LDS transpose would have to hold 159 x 64 x 4 = 40 KB per workgroup and still read the slab column-wise.
// Top-k: five rounds of wave_max over the lanes' not-yet-taken values, the taker fixed by ballot (lowest slot, lowest lane), so ties
// resolve the same way every call; the top-k mean does not depend on how.  Selecting on the logits is selecting on p.
// Per workgroup {ce, bce, n_valid, a3, a5} go to ws, the last workgroup (last_workgroup.h) adds them per clip, then over clips, forms
// count and the seven losses.  Gradient pieces, all fully written: dlogits <- w_emotion dBCE; N (natural coordinates) <- dCE; V
// (natural coordinates, scattered in the view layout -- every logit belongs to exactly one auxiliary row, so no two waves write one
// word) <- dA_3 + dA_5.
// Launch 2, chord_aux_combine_kernel: dlogits += (w_chord / count) (N + V), count read from loss[6] on the device: no host sync.
// No floating-point atomic; forward-only mode (dlogits null) runs launch 1's additions alone: the same loss / clip_out bits.
#include "../../include/amt_hip.h"
#include "amt_common.h"
#include "chord_rows.h"
#include "last_workgroup.h"

namespace {

constexpr int WAVES = 16, THREADS = 64 * WAVES;
constexpr int ROWS = 64;                    // row indices per workgroup
constexpr int PARTS = 5;                    // per workgroup: ce, bce, n_valid, a3, a5
constexpr float COUNT_FLOOR = 1e-10f;       // CombinedLoss: `if l > 1e-10: count += 1` on the fp32 term

__device__ __forceinline__ int64_t parts_floats(int64_t blocks) { return (PARTS * blocks + 3) & ~(int64_t)3; }

// The hinge terms of one auxiliary row z (three lane-strided dwords, z2 = -inf past class 158) with target t, and, with V given, the
// row's dz = p_j sum_k c_k ([j in top-k] / k - [j = t] - h_k) (c_k = w_k / n_valid where the row is valid and h_k > 0, else 0), stored
// at V + o0 / o1 / o2.
__device__ __forceinline__ void aux_row(float z0, float z1, float z2, int t, bool valid, int lane, bool has2, float inv_valid, float* V,
                                        size_t o0, size_t o1, size_t o2, float& a3, float& a5) {
    const float m = wave_max(fmaxf(fmaxf(z0, z1), z2));
    const float e0 = expf(z0 - m), e1 = expf(z1 - m), e2 = has2 ? expf(z2 - m) : 0.0f;
    const float inv_se = 1.0f / wave_sum((e0 + e1) + e2);
    float c0 = z0, c1 = z1, c2 = z2;        // candidates: a taken one becomes -inf
    int r0 = 8, r1 = 8, r2 = 8;             // the round in which this lane's value was taken
    float s3 = 0.0f, s5 = 0.0f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const float mk = wave_max(fmaxf(fmaxf(c0, c1), c2));
        const uint64_t b0 = __ballot(c0 == mk), b1 = __ballot(c1 == mk), b2 = __ballot(c2 == mk);
        const int slot = b0 ? 0 : b1 ? 1 : 2;
        const uint64_t bm = b0 ? b0 : b1 ? b1 : b2;
        const bool mine = bm != 0 && lane == __builtin_ctzll(bm);
        if (mine && slot == 0) { c0 = -INFINITY; r0 = k; }
        if (mine && slot == 1) { c1 = -INFINITY; r1 = k; }
        if (mine && slot == 2) { c2 = -INFINITY; r2 = k; }
        s5 += expf(mk - m) * inv_se;        // the taken lane's own e * inv_se: the same operands
        if (k == 2) s3 = s5;
    }
    const float esel = t < 64 ? e0 : t < 128 ? e1 : e2;
    const float pt = readlane_f(esel, t & 63) * inv_se;
    const float h3 = s3 / 3.0f - pt, h5 = s5 / 5.0f - pt;
    a3 = valid ? fmaxf(h3, 0.0f) : 0.0f;
    a5 = valid ? fmaxf(h5, 0.0f) : 0.0f;
    if (V) {
        const float k3 = valid && h3 > 0.0f ? 3.0f * inv_valid : 0.0f, k5 = valid && h5 > 0.0f ? 5.0f * inv_valid : 0.0f;
        auto dz = [&](float e, int rank, int j) {
            const float hit = j == t ? 1.0f : 0.0f;
            const float g3 = ((rank < 3 ? 1.0f / 3.0f : 0.0f) - hit) - h3, g5 = ((rank < 5 ? 1.0f / 5.0f : 0.0f) - hit) - h5;
            return (e * inv_se) * (k3 * g3 + k5 * g5);
        };
        V[o0] = dz(e0, r0, lane);
        V[o1] = dz(e1, r1, lane + 64);
        if (has2) V[o2] = dz(e2, r2, lane + 128);
    }
}

__global__ __launch_bounds__(THREADS) void chord_aux_kernel(const float* __restrict__ logits, int ld, const int64_t* __restrict__ tgt,
                                                            const int32_t* __restrict__ emo_class, int B, int L, float w_chord,
                                                            float w_emotion, float smoothing, int layout, float* __restrict__ loss,
                                                            float* __restrict__ clip_out, float* __restrict__ dlogits, float* ws) {
    __shared__ float s_val[4][ROWS];        // per row index: ce (0 for an ignored one), bce, a3, a5
    __shared__ int s_cnt[3];                // [0]: valid targets among this workgroup's rows, [1]: in the whole batch, [2]: last to finish
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int spc = (L + ROWS - 1) / ROWS;                 // workgroups per clip
    const int clip = blockIdx.x / spc, l0 = (blockIdx.x % spc) * ROWS, n = min(ROWS, L - l0);
    const size_t row0 = (size_t)clip * L + l0;
    const int n_rows = B * L;
    const size_t n_el = (size_t)n_rows * NC;
    float* part = ws + WS_HEAD;
    float* gN = dlogits ? part + parts_floats(gridDim.x) : nullptr;
    float* gV = dlogits ? gN + n_el : nullptr;
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

        // the natural row: chord_loss.hip's cross-entropy and BCE, operation for operation
        const float m = wave_max(fmaxf(fmaxf(y0, y1), y2));
        const float e0 = expf(y0 - m), e1 = expf(y1 - m), e2 = has2 ? expf(y2 - m) : 0.0f;
        const float se = wave_sum((e0 + e1) + e2);
        const float lse = logf(se);                         // not m + log se: see chord_loss.hip
        const float ysel = t < 64 ? y0 : t < 128 ? y1 : y2;
        const float nll = lse - (readlane_f(ysel, t & 63) - m);
        float ce = nll;
        if (smoothing != 0.0f) {
            const float sy = wave_sum(((y0 - m) + (y1 - m)) + (has2 ? y2 - m : 0.0f));
            ce = (1.0f - smoothing) * nll + smoothing * (((float)NC * lse - sy) / (float)NC);
        }
        const bool t0 = chord && lane != 0 && ((qm >> q0) & 1u);
        const bool t1 = chord && ((qm >> q1) & 1u);
        const bool t2 = lane + 128 == ID_END ? t == ID_END : lane + 128 == ID_PAD ? t == ID_PAD : (chord && ((qm >> q2) & 1u));
        const float bce = wave_sum((bce_term(y0, t0) + bce_term(y1, t1)) + (has2 ? bce_term(y2, t2) : 0.0f));

        // the auxiliary row of the same index
        float a3, a5;
        if (layout == AMT_CHORD_AUX_ROWS) {
            const size_t o = row * NC + lane;
            aux_row(y0, y1, y2, t, valid, lane, has2, inv_valid, gV, o, o + 64, o + 128, a3, a5);
        } else {
            const int f = NC * (l0 + r) + lane;             // < 159 L: l < L and c < 159 below
            const int la = f % L, ca = f / L, lb = (f + 64) % L, cb = (f + 64) / L, lc = (f + 128) % L, cc = (f + 128) / L;
            const size_t base = (size_t)clip * L;
            const float z0 = logits[(base + la) * ld + ca], z1 = logits[(base + lb) * ld + cb];
            const float z2 = has2 ? logits[(base + lc) * ld + cc] : -INFINITY;
            aux_row(z0, z1, z2, t, valid, lane, has2, inv_valid, gV, (base + la) * NC + ca, (base + lb) * NC + cb, (base + lc) * NC + cc, a3, a5);
        }

        valid_cnt += valid;
        if (lane == 0) {
            s_val[0][r] = valid ? ce : 0.0f;
            s_val[1][r] = bce;
            s_val[2][r] = a3;
            s_val[3][r] = a5;
        }
        if (dlogits) {
            const size_t o = row * NC + lane;
            const float inv_se = 1.0f / se, cs = valid ? inv_valid : 0.0f, bs = w_emotion * inv_bce;
            const float off = smoothing / (float)NC, hit = 1.0f - smoothing;
            auto soft = [&](float e, int j) { return valid ? cs * ((e * inv_se - (j == t ? hit : 0.0f)) - off) : 0.0f; };
            auto emo = [&](float y, bool tj) { return bs * (1.0f / (1.0f + expf(-y)) - (tj ? 1.0f : 0.0f)); };
            gN[o] = soft(e0, lane);
            gN[o + 64] = soft(e1, lane + 64);
            dlogits[o] = emo(y0, t0);
            dlogits[o + 64] = emo(y1, t1);
            if (has2) {
                gN[o + 128] = soft(e2, lane + 128);
                dlogits[o + 128] = emo(y2, t2);
            }
        }
    }
    if (lane == 0) atomicAdd(&s_cnt[0], valid_cnt);
    __syncthreads();
    float acc = 0.0f;
    if (wave == 0 && lane < 4)
        for (int r = 0; r < n; ++r) acc += s_val[lane][r];           // row order: the same sum whatever the wave count
    if (wave == 0) {
        float* q = part + PARTS * blockIdx.x;
        if (lane < 2) q[lane] = acc;
        if (lane == 2 || lane == 3) q[lane + 1] = acc;
        if (lane == 4) q[2] = (float)s_cnt[0];
    }
    if (!last_workgroup(ws, gridDim.x, reinterpret_cast<unsigned*>(&s_cnt[2])) || tid != 0) return;
    float ce_all = 0.0f, bce_all = 0.0f, valid_all = 0.0f, a3_all = 0.0f, a5_all = 0.0f;
    for (int b = 0; b < B; ++b) {
        float ce = 0.0f, bce = 0.0f, nv = 0.0f, a3 = 0.0f, a5 = 0.0f;
        for (int s = 0; s < spc; ++s) {
            const float* q = part + PARTS * (b * spc + s);
            ce += q[0]; bce += q[1]; nv += q[2]; a3 += q[3]; a5 += q[4];
        }
        float* o = clip_out + 6 * b;
        o[0] = nv; o[1] = ce; o[2] = bce; o[3] = (float)L; o[4] = a3; o[5] = a5;
        ce_all += ce; bce_all += bce; valid_all += nv; a3_all += a3; a5_all += a5;
    }
    // no valid target in the batch: NaN terms, count 0, chord NaN, as the reference gives
    const float cet = ce_all / valid_all, aux3 = a3_all / valid_all * 3.0f, aux5 = a5_all / valid_all * 5.0f;
    const float emotion = bce_all * inv_bce;
    const int count = (cet > COUNT_FLOOR) + (aux3 > COUNT_FLOOR) + (aux5 > COUNT_FLOOR);
    const float chordl = ((cet + aux3) + aux5) / (float)count;
    // a weight of exactly 0 drops its term, as -drop_loss drops it from the reference's graph (0 x NaN would keep it)
    loss[0] = (w_chord != 0.0f ? w_chord * chordl : 0.0f) + (w_emotion != 0.0f ? w_emotion * emotion : 0.0f);
    loss[1] = chordl;
    loss[2] = emotion;
    loss[3] = cet;
    loss[4] = aux3;
    loss[5] = aux5;
    loss[6] = (float)count;
}

__global__ __launch_bounds__(256) void chord_aux_combine_kernel(float* __restrict__ dlogits, const float* __restrict__ gN,
                                                                const float* __restrict__ gV, const float* __restrict__ loss,
                                                                float w_chord, size_t n_el) {
    const float s = w_chord != 0.0f ? w_chord / loss[6] : 0.0f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_el; i += (size_t)gridDim.x * 256)
        dlogits[i] = dlogits[i] + s * (gN[i] + gV[i]);
}

}  // namespace

extern "C" int64_t amt_chord_loss_aux_ws_floats(int32_t B, int32_t L) {
    if (B <= 0 || L <= 0) return 0;
    const int64_t blocks = (int64_t)B * ((L + ROWS - 1) / ROWS);
    return WS_HEAD + ((PARTS * blocks + 3) & ~(int64_t)3) + 2 * (int64_t)B * L * NC;
}

extern "C" int32_t amt_chord_loss_aux_fwd_bwd(const float* logits, int32_t ld, const int64_t* tgt, const int32_t* emo_class, int32_t B,
                                              int32_t L, float w_chord, float w_emotion, float smoothing, int32_t layout, float* loss,
                                              float* clip_out, float* dlogits, float* ws, void* stream) {
    AMT_CHECK_ARG(logits && tgt && emo_class && loss && clip_out, "amt_chord_loss_aux_fwd_bwd: null pointer");
    AMT_CHECK_ARG(ld >= NC, "amt_chord_loss_aux_fwd_bwd: row stride %d is below the %d classes of a row", ld, NC);
    AMT_CHECK_ARG(B > 0 && L > 0, "amt_chord_loss_aux_fwd_bwd: B=%d, L=%d must be positive", B, L);
    AMT_CHECK_ARG((int64_t)B * L * NC <= (1 << 24), "amt_chord_loss_aux_fwd_bwd: B=%d x L=%d rows: the divisor 159 B L is exact in fp32 up to 2^24", B, L);
    AMT_CHECK_ARG(smoothing >= 0.0f && smoothing < 1.0f, "amt_chord_loss_aux_fwd_bwd: smoothing=%g must be in [0, 1)", (double)smoothing);
    AMT_CHECK_ARG(layout == AMT_CHORD_AUX_ROWS || layout == AMT_CHORD_AUX_VIEW,
                  "amt_chord_loss_aux_fwd_bwd: layout=%d is neither AMT_CHORD_AUX_ROWS (0) nor AMT_CHORD_AUX_VIEW (1)", layout);
    if (const int32_t rc = last_workgroup_reset(ws, "amt_chord_loss_aux_fwd_bwd", (hipStream_t)stream)) return rc;
    const int blocks = B * ((L + ROWS - 1) / ROWS);
    hipLaunchKernelGGL(chord_aux_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, logits, ld, tgt, emo_class, B, L, w_chord,
                       w_emotion, smoothing, layout, loss, clip_out, dlogits, ws);
    AMT_LAUNCH_CHECK();
    if (dlogits) {
        const size_t n_el = (size_t)B * L * NC;
        const float* gN = ws + WS_HEAD + ((PARTS * (int64_t)blocks + 3) & ~(int64_t)3);
        const int cb = (int)((n_el + 1023) / 1024 < 2048 ? (n_el + 1023) / 1024 : 2048);
        hipLaunchKernelGGL(chord_aux_combine_kernel, dim3(cb), dim3(256), 0, (hipStream_t)stream, dlogits, gN, gN + n_el, loss, w_chord, n_el);
        AMT_LAUNCH_CHECK();
    }
    return 0;
}
