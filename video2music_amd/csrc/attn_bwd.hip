// Backward of the prefill attention (attn_prefill.hip, TRAIN instantiations) in fp32 on the matrix cores.  With qs = q q_scale,
//   S_ij = qs_i . k_j (+ qs_i . Er[er_len-1-(i-j)]),  P = softmax_j(S),  Pd = P o keep keep_scale,  O = Pd V
// and D_i = sum_d dO_id O_id:
//   dP = (dO V^T) o keep keep_scale,  dS = P o (dP - D_i)
//   dv = Pd^T dO,  dk = dS^T qs,  dqs = dS k (+ sum_j dS_ij Er[er_len-1-(i-j)]),  dEr[r] = sum over (b, h, i - j = er_len-1-r) of dS_ij qs_i
//
// Pass A (attn_bwd_dq_kernel), flash-style and laid out exactly like the forward: a workgroup is 128 query rows of one (clip, head),
// one query per lane, keys in LDS tiles of 32.  P^T is recomputed tile by tile from the saved log-sum-exp (S^T = K . Q^T with the
// forward's relative-position ring), dP^T = V . dO^T is the same product on the V tile, and dqs^T += K^T . dS^T is the forward's
// O^T += V^T . P^T on the K tile.  It also leaves dS and Pd in two (B H, Lq, ld) scratches, ld = Lk rounded up to 32, for the sums
// over the queries that a query-per-lane pass cannot form.  With relative positions key j of query i sits in column L-1-(i-j) of
// its row -- the un-skewed form, column = row of the table's last L rows -- otherwise in column j.
// Pass B (attn_bwd_dkv_kernel): one wave per 32 keys; dk = dS^T qs and dv = Pd^T dO as MFMA chains over the query rows in order,
// operands straight from global memory (the scratch rows and the q / dO rows are read along their contiguous dimension), the query
// heads of a key head's group one after the other.
// Relative positions: dq's second term is one dense product of the un-skewed scratch with the table's last L rows (the library's
// GEMM), dEr a per-(clip, head) MFMA chain (attn_bwd_der_kernel: scratch^T qs) into one slab each, the slabs added in (clip, head)
// order; rows of Er no pair reaches are written as exact zeros.
// No atomics anywhere: the order of every addition is a function of the shapes alone.
#include "../../include/amt_hip.h"
#include "amt_common.h"
#include "kernels.h"

namespace {

constexpr int QB = 128;      // query rows per workgroup (pass A)
constexpr int KT = 32;       // keys per tile

struct Scratch { float* dS; float* Pd; int ld; };

template <int HD, bool RPR>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(AttnParams p, const float* __restrict__ dO, float* __restrict__ dq, Scratch w) {
    static_assert(HD >= 32, "the 32-row d tile of dq^T needs whole 32-column K tiles");
    constexpr int LD = HD + 4;
    constexpr int NS = HD / 8;           // ds_read_b128 k-groups per operand row
    constexpr int ND = HD / 32;          // 32-wide d tiles of dq^T
    constexpr int SCR = 2 * 32 * 33 > 32 * (HD + 1) ? 2 * 32 * 33 : 32 * (HD + 1);   // two 32x33 distance chunks / the dq transpose
    __shared__ __attribute__((aligned(16))) float Ks[KT * LD];
    __shared__ __attribute__((aligned(16))) float Vs[KT * LD];
    __shared__ __attribute__((aligned(16))) float scr_all[4 * SCR];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int n_bh = p.H * p.B, n_qb = (p.Lq + QB - 1) / QB;
    const int qblk = n_qb - 1 - (int)(blockIdx.x / n_bh);
    const int bh = blockIdx.x % n_bh;
    const int h = bh % p.H, b = bh / p.H;
    const int hk = h / p.kv_group;
    const int I0 = qblk * QB, i0 = I0 + wave * 32, iq = i0 + li;
    const bool q_ok = iq < p.Lq;
    float* scr = scr_all + wave * SCR;

    const float* qp = p.q + (size_t)b * p.q_bs + (size_t)h * p.q_hs;
    const float* kp = p.k + (size_t)b * p.k_bs + (size_t)hk * p.k_hs;
    const float* vp = p.v + (size_t)b * p.v_bs + (size_t)hk * p.v_hs;
    const float* op = p.o + (size_t)b * p.o_bs + (size_t)h * p.o_hs;
    const float* gp = dO + (size_t)b * p.o_bs + (size_t)h * p.o_hs;

    // Q^T and dO^T fragments: reg[4s+e] = X[iq][8s + 4*lh + e]; D = dO . O of the row (each half-lane holds half of the columns)
    const float qs = p.q_scale == 0.f ? 1.f : p.q_scale;
    float qreg[HD / 2], doreg[HD / 2];
    float Dq = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 t = q_ok ? ld4(qp + (size_t)iq * p.q_ls + 8 * s + 4 * lh) : z;
        const float4 g = q_ok ? ld4(gp + (size_t)iq * p.o_ls + 8 * s + 4 * lh) : z;
        const float4 o = q_ok ? ld4(op + (size_t)iq * p.o_ls + 8 * s + 4 * lh) : z;
        qreg[4 * s + 0] = t.x * qs; qreg[4 * s + 1] = t.y * qs; qreg[4 * s + 2] = t.z * qs; qreg[4 * s + 3] = t.w * qs;
        doreg[4 * s + 0] = g.x; doreg[4 * s + 1] = g.y; doreg[4 * s + 2] = g.z; doreg[4 * s + 3] = g.w;
        Dq += (g.x * o.x + g.y * o.y) + (g.z * o.z + g.w * o.w);
    }
    Dq += __shfl_xor(Dq, 32, 64);
    const float lse = q_ok ? p.lse[(size_t)bh * p.Lq + iq] : 0.f;
    const size_t srow = ((size_t)bh * p.Lq + (q_ok ? iq : 0)) * w.ld;
    const uint8_t* kr = p.keep ? p.keep + ((size_t)bh * p.Lq + (q_ok ? iq : 0)) * p.Lk : nullptr;

    f32x16 qacc[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) qacc[dt][e] = 0.f;

    int k_end = p.Lk;
    if (p.causal) k_end = min(p.Lk, I0 + QB);
    const int n_tiles = (k_end + KT - 1) / KT;

    // K/V tile staging: 32 rows x HD/4 float4 per tensor over 256 threads (attn_prefill_kernel's)
    constexpr int F4_ROW = HD / 4, F4_TILE = KT * F4_ROW, PER_T = (F4_TILE + 255) / 256;
    static_assert(F4_TILE % 256 == 0, "a K/V tile is a whole number of 256-thread passes");
    float4 kst[PER_T], vst[PER_T];
    auto gload = [&](int j0) {
#pragma unroll
        for (int i = 0; i < PER_T; ++i) {
            const int f = tid + i * 256;
            const int r = f / F4_ROW, c = (f - r * F4_ROW) * 4;
            const int j = min(j0 + r, p.Lk - 1);          // keys past the end re-read the last row: their P is 0
            kst[i] = ld4(kp + (size_t)j * p.k_ls + c);
            vst[i] = ld4(vp + (size_t)j * p.v_ls + c);
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < PER_T; ++i) {
            const int f = tid + i * 256;
            const int r = f / F4_ROW, c = (f - r * F4_ROW) * 4;
            st4(&Ks[r * LD + c], kst[i]);
            st4(&Vs[r * LD + c], vst[i]);
        }
    };

    float4 er_next[NS];                    // Er rows of the chunk the next tile will need (relative positions only)
    bool er_primed = false;
    gload(0);
    for (int kt = 0; kt < n_tiles; ++kt) {
        const int j0 = kt * KT;
        __syncthreads();                 // previous tile fully consumed
        lstore();
        __syncthreads();
        if (kt + 1 < n_tiles) gload(j0 + KT);
        if (p.causal && j0 > i0 + 31) continue;          // whole tile above this wave's diagonal

        // ---- S^T = K . Q^T and dP^T = V . dO^T ----
        f32x16 sacc, pacc;
#pragma unroll
        for (int e = 0; e < 16; ++e) { sacc[e] = 0.f; pacc[e] = 0.f; }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const float4 a = ld4(&Ks[li * LD + 8 * s + 4 * lh]);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, qreg[4 * s + 0], sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, qreg[4 * s + 1], sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, qreg[4 * s + 2], sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, qreg[4 * s + 3], sacc, 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const float4 a = ld4(&Vs[li * LD + 8 * s + 4 * lh]);
            pacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, doreg[4 * s + 0], pacc, 0, 0, 0);
            pacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, doreg[4 * s + 1], pacc, 0, 0, 0);
            pacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, doreg[4 * s + 2], pacc, 0, 0, 0);
            pacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, doreg[4 * s + 3], pacc, 0, 0, 0);
        }

        // ---- relative-position term of S, as the forward forms it (attn_prefill_kernel: chunk ring per wave) ----
        if constexpr (RPR) {
            const int k = (i0 - j0) / 32;
            auto er_load = [&](int c, float4 (&ef)[NS]) {
                int row = p.er_len - 1 - (32 * c + li);
                row = max(0, min(p.er_len - 1, row));      // out-of-range rows belong to masked pairs
                const float* ep = p.Er + (size_t)row * HD + 4 * lh;
#pragma unroll
                for (int s = 0; s < NS; ++s) ef[s] = ld4(ep + 8 * s);
            };
            auto chunk = [&](int c, const float4 (&ef)[NS]) {
                f32x16 racc;
#pragma unroll
                for (int e = 0; e < 16; ++e) racc[e] = 0.f;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    racc = __builtin_amdgcn_mfma_f32_32x32x2f32(ef[s].x, qreg[4 * s + 0], racc, 0, 0, 0);
                    racc = __builtin_amdgcn_mfma_f32_32x32x2f32(ef[s].y, qreg[4 * s + 1], racc, 0, 0, 0);
                    racc = __builtin_amdgcn_mfma_f32_32x32x2f32(ef[s].z, qreg[4 * s + 2], racc, 0, 0, 0);
                    racc = __builtin_amdgcn_mfma_f32_32x32x2f32(ef[s].w, qreg[4 * s + 3], racc, 0, 0, 0);
                }
                float* slot = scr + (c & 1) * (32 * 33);
#pragma unroll
                for (int e = 0; e < 16; ++e) slot[li * 33 + (e & 3) + 8 * (e >> 2) + 4 * lh] = racc[e];
            };
            if (!er_primed) {                                // first tile this wave computes: both chunks are new
                float4 e0[NS];
                er_load(k, e0);
                chunk(k, e0);
                er_load(k - 1, er_next);
                er_primed = true;
            }
            if (k >= 1) chunk(k - 1, er_next);
            if (k >= 2) er_load(k - 2, er_next);             // for the next tile (it reads chunk k-2 as its k-1)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int krow = (e & 3) + 8 * (e >> 2) + 4 * lh;
                const int dlt = li - krow;                  // distance - D
                const int c = dlt >= 0 ? k : k - 1;
                sacc[e] += scr[(c & 1) * (32 * 33) + li * 33 + (dlt & 31)];
            }
        }

        // ---- P from the saved log-sum-exp, then dS^T and Pd^T; both go to the scratches for the sums over the queries ----
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int j = j0 + (e & 3) + 8 * (e >> 2) + 4 * lh;
            const bool vis = j < p.Lk && !(p.causal && j > iq);
            const float pr = vis ? __expf(sacc[e] - lse) : 0.f;
            const float kp_ = kr ? ((vis && kr[min(j, p.Lk - 1)]) ? p.keep_scale : 0.f) : 1.f;
            const float pd = pr * kp_;
            const float ds = pr * (pacc[e] * kp_ - Dq);
            if (vis && q_ok) {
                const size_t at = srow + (RPR ? p.Lk - 1 - iq + j : j);
                w.dS[at] = ds;
                w.Pd[at] = pd;
            }
            sacc[e] = ds;
        }

        // ---- dqs^T += K^T . dS^T : k-step e pairs key krow(e,0) (lanes 0-31) with krow(e,1) ----
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int krow = (e & 3) + 8 * (e >> 2) + 4 * lh;
#pragma unroll
            for (int dt = 0; dt < ND; ++dt) {
                const float a = Ks[krow * LD + dt * 32 + li];
                qacc[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, sacc[e], qacc[dt], 0, 0, 0);
            }
        }
    }

    // ---- transpose through the wave's scratch, store rows coalesced; without the relative term this is dq itself ----
    const float out_scale = RPR ? 1.f : qs;
    __syncthreads();                     // all waves are done with their scratch as R band
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int dd = dt * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
            scr[li * (HD + 1) + dd] = qacc[dt][e] * out_scale;
        }
    float* dqp = dq + (size_t)b * p.q_bs + (size_t)h * p.q_hs;
    for (int r = 0; r < 32; ++r) {
        const int i = i0 + r;
        if (i >= p.Lq) break;
        for (int c = lane; c < HD; c += 64) dqp[(size_t)i * p.q_ls + c] = scr[r * (HD + 1) + c];
    }
}

// dk[j][d] = sum_i dS_ij qs_id, dv[j][d] = sum_i Pd_ij dO_id for 32 keys per wave: C[key][d] += A[key][i] B[i][d], two query rows per
// MFMA, i ascending; the query heads of the key head's group in order
template <int HD, bool RPR>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(AttnParams p, const float* __restrict__ dO, float* __restrict__ dk,
                                                           float* __restrict__ dv, Scratch w) {
    constexpr int ND = HD / 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int Hk = p.H / p.kv_group, n_kb = (p.Lk + QB - 1) / QB;
    const int kblk = blockIdx.x % n_kb, bhk = blockIdx.x / n_kb;
    const int hk = bhk % Hk, b = bhk / Hk;
    const int j0 = kblk * QB + wave * 32, j = j0 + li;
    if (j0 >= p.Lk) return;                                  // no barrier below: the waves are independent
    const float qs = p.q_scale == 0.f ? 1.f : p.q_scale;
    f32x16 kacc[ND], vacc[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) { kacc[dt][e] = 0.f; vacc[dt][e] = 0.f; }
    for (int g = 0; g < p.kv_group; ++g) {
        const int h = hk * p.kv_group + g, bh = b * p.H + h;
        const float* qp = p.q + (size_t)b * p.q_bs + (size_t)h * p.q_hs;
        const float* gp = dO + (size_t)b * p.o_bs + (size_t)h * p.o_hs;
        for (int i0 = p.causal ? j0 : 0; i0 < p.Lq; i0 += 8) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int i = i0 + 2 * t + lh;
                const bool row_ok = i < p.Lq;
                const int ic = row_ok ? i : 0;              // every address stays inside its tensor, whatever the predicate
                const bool ok = row_ok && j < p.Lk && !(p.causal && j > i);
                const size_t at = ((size_t)bh * p.Lq + ic) * w.ld + (ok ? (RPR ? p.Lk - 1 - i + j : j) : 0);
                const float a_ds = ok ? w.dS[at] : 0.f, a_pd = ok ? w.Pd[at] : 0.f;
#pragma unroll
                for (int dt = 0; dt < ND; ++dt) {
                    const float bq = row_ok ? qp[(size_t)ic * p.q_ls + dt * 32 + li] * qs : 0.f;
                    const float bg = row_ok ? gp[(size_t)ic * p.o_ls + dt * 32 + li] : 0.f;
                    kacc[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_ds, bq, kacc[dt], 0, 0, 0);
                    vacc[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_pd, bg, vacc[dt], 0, 0, 0);
                }
            }
        }
    }
    float* dkp = dk + (size_t)b * p.k_bs + (size_t)hk * p.k_hs;
    float* dvp = dv + (size_t)b * p.v_bs + (size_t)hk * p.v_hs;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int key = j0 + (e & 3) + 8 * (e >> 2) + 4 * lh;
            if (key < p.Lk) {
                dkp[(size_t)key * p.k_ls + dt * 32 + li] = kacc[dt][e];
                dvp[(size_t)key * p.v_ls + dt * 32 + li] = vacc[dt][e];
            }
        }
}

// slab[bh][r][d] = sum_i dS[bh][i][r] qs[b][h][i][d] over the un-skewed scratch (column r = row er_len - L + r of the table), 32 columns
// per wave, i ascending.  Column r of row i is reached only for i >= L-1-r; the columns before a row's first pair are zeros.
template <int HD>
__global__ __launch_bounds__(256) void attn_bwd_der_kernel(AttnParams p, Scratch w, float* __restrict__ slab) {
    constexpr int ND = HD / 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int L = p.Lq, n_rb = (L + QB - 1) / QB;
    const int rblk = blockIdx.x % n_rb, bh = blockIdx.x / n_rb;
    const int h = bh % p.H, b = bh / p.H;
    const int r0 = rblk * QB + wave * 32, r = r0 + li;
    if (r0 >= L) return;
    const float qs = p.q_scale == 0.f ? 1.f : p.q_scale;
    const float* qp = p.q + (size_t)b * p.q_bs + (size_t)h * p.q_hs;
    f32x16 acc[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[dt][e] = 0.f;
    const int i_first = max(0, L - 32 - r0) & ~7;
    for (int i0 = i_first; i0 < L; i0 += 8) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = i0 + 2 * t + lh;
            const bool ok = i < L;
            const int ic = ok ? i : 0;
            const float a = (ok && r < L) ? w.dS[((size_t)bh * L + ic) * w.ld + min(r, L - 1)] : 0.f;
#pragma unroll
            for (int dt = 0; dt < ND; ++dt) {
                const float bq = ok ? qp[(size_t)ic * p.q_ls + dt * 32 + li] * qs : 0.f;
                acc[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bq, acc[dt], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int rr = r0 + (e & 3) + 8 * (e >> 2) + 4 * lh;
            if (rr < L) slab[((size_t)bh * L + rr) * HD + dt * 32 + li] = acc[dt][e];
        }
}

// dEr[row][d]: the slabs added in (clip, head) order for the table's last L rows, exact zeros for the rows no pair reaches
__global__ void der_reduce_kernel(const float* __restrict__ slab, float* __restrict__ dEr, int n_bh, int L, int hd, int er_len) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= er_len * hd) return;
    const int row = f / hd, d = f - row * hd, r = row - (er_len - L);
    float a = 0.f;
    if (r >= 0)
        for (int k = 0; k < n_bh; ++k) a += slab[((size_t)k * L + r) * hd + d];
    dEr[f] = a;
}

// ErT[d][c] = Er[er_len - L + c][d] for c < L, zeros up to ld: the right operand of dq's relative-position product
__global__ void er_transpose_kernel(const float* __restrict__ Er, float* __restrict__ ErT, int L, int hd, int er_len, int ld) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= hd * ld) return;
    const int d = f / ld, c = f - d * ld;
    ErT[f] = c < L ? Er[(size_t)(er_len - L + c) * hd + d] : 0.f;
}

// dq = (dq + dq_er) q_scale, dq_er (B H, L, hd) contiguous
__global__ void dq_finish_kernel(AttnParams p, float* __restrict__ dq, const float* __restrict__ dq_er) {
    const size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = (size_t)p.B * p.H * p.Lq * p.hd;
    if (f >= n) return;
    const int d = (int)(f % p.hd);
    const size_t row = f / p.hd;
    const int i = (int)(row % p.Lq);
    const int bh = (int)(row / p.Lq);
    const int h = bh % p.H, b = bh / p.H;
    const float qs = p.q_scale == 0.f ? 1.f : p.q_scale;
    float* at = dq + (size_t)b * p.q_bs + (size_t)h * p.q_hs + (size_t)i * p.q_ls + d;
    *at = (*at + dq_er[f]) * qs;
}

inline int ceil32(int n) { return (n + 31) / 32 * 32; }

template <int HD>
int32_t launch_hd(const AttnBwdParams& P, hipStream_t stream) {
    const AttnParams& p = P.f;
    const int n_bh = p.B * p.H, ld = ceil32(p.Lk);
    const size_t n1 = (size_t)n_bh * p.Lq * ld;
    Scratch w{P.ws, P.ws + n1, ld};
    const dim3 grid_a(cdiv(p.Lq, QB) * n_bh), grid_b(cdiv(p.Lk, QB) * (p.H / p.kv_group) * p.B);
    if (!p.Er) {
        hipLaunchKernelGGL((attn_bwd_dq_kernel<HD, false>), grid_a, dim3(256), 0, stream, p, P.dO, P.dq, w);
        hipLaunchKernelGGL((attn_bwd_dkv_kernel<HD, false>), grid_b, dim3(256), 0, stream, p, P.dO, P.dk, P.dv, w);
        return 0;
    }
    const int L = p.Lq;
    float* ErT = P.ws + 2 * n1;
    float* dq_er = ErT + (size_t)HD * ld;
    float* slab = dq_er + (size_t)n_bh * L * HD;
    AMT_HIP(hipMemsetAsync(w.dS, 0, n1 * sizeof(float), stream));        // the columns before each row's first pair
    hipLaunchKernelGGL((attn_bwd_dq_kernel<HD, true>), grid_a, dim3(256), 0, stream, p, P.dO, P.dq, w);
    hipLaunchKernelGGL((attn_bwd_dkv_kernel<HD, true>), grid_b, dim3(256), 0, stream, p, P.dO, P.dk, P.dv, w);
    hipLaunchKernelGGL(er_transpose_kernel, dim3(cdiv(HD * ld, 256)), dim3(256), 0, stream, p.Er, ErT, L, HD, p.er_len, ld);
    GemmParams g = gemm_params(w.dS, ld, ErT, ld, dq_er, HD, n_bh * L, HD, ld, nullptr);
    const int32_t rc = amt_launch_gemm(g, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(dq_finish_kernel, dim3((unsigned)(((size_t)n_bh * L * HD + 255) / 256)), dim3(256), 0, stream, p, P.dq, dq_er);
    if (P.dEr) {
        hipLaunchKernelGGL((attn_bwd_der_kernel<HD>), dim3(cdiv(L, QB) * n_bh), dim3(256), 0, stream, p, w, slab);
        hipLaunchKernelGGL(der_reduce_kernel, dim3(cdiv(p.er_len * HD, 256)), dim3(256), 0, stream, slab, P.dEr, n_bh, L, HD, p.er_len);
    }
    return 0;
}

}  // namespace

int64_t amt_attn_bwd_ws_floats_of(int B, int H, int Lq, int Lk, int hd, int rpr) {
    const int64_t n_bh = (int64_t)B * H, ld = ceil32(Lk);
    return 2 * n_bh * Lq * ld + (rpr ? hd * ld + 2 * n_bh * Lq * hd : 0);
}

int32_t amt_launch_attn_bwd(const AttnBwdParams& P, hipStream_t stream) {
    const AttnParams& p = P.f;
    AMT_CHECK_ARG(p.B > 0 && p.H > 0 && p.Lq > 0 && p.Lk > 0, "attn_bwd: bad shape");
    AMT_CHECK_ARG(p.kv_group >= 1 && p.H % p.kv_group == 0, "attn_bwd: bad kv_group %d", p.kv_group);
    AMT_CHECK_ARG(p.Er == nullptr || (p.causal && p.Lq == p.Lk && p.Lq <= p.er_len && p.kv_group == 1),
                  "attn_bwd: relative positions need causal self-attention with L=%d <= er_len=%d and kv_group 1", p.Lq, p.er_len);
    AMT_CHECK_ARG(p.q_ls % 4 == 0 && p.k_ls % 4 == 0 && p.v_ls % 4 == 0 && p.o_ls % 4 == 0, "attn_bwd: row strides must be multiples of 4 floats");
    AMT_CHECK_ARG((int64_t)p.B * p.H * p.Lq <= (1 << 24), "attn_bwd: B H Lq = %lld rows, at most 2^24", (long long)p.B * p.H * p.Lq);
    int32_t rc = 0;
    switch (p.hd) {
        case 32: rc = launch_hd<32>(P, stream); break;
        case 64: rc = launch_hd<64>(P, stream); break;
        case 128: rc = launch_hd<128>(P, stream); break;
        default: AMT_CHECK_ARG(false, "attn_bwd: head_dim %d not in {32,64,128} (16 is not built for training: the backward's 32-row "
                                      "d tiles need whole 32-column K tiles)", p.hd);
    }
    if (rc) return rc;
    AMT_LAUNCH_CHECK();
    return 0;
}
