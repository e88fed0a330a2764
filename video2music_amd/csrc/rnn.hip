// LSTM / GRU recurrences of the regression head `VideoRegression(regModel='lstm' | 'bilstm' | 'gru' | 'bigru')`
// (model/video_regression.py:124-135: torch.nn.LSTM / nn.GRU, batch_first, hidden = d_model; the arithmetic lives in torch,
// whose documented cell equations are restated here):
//   LSTM  i,f,g,o = split(W_ih x + b_ih + W_hh h + b_hh);  c' = sigmoid(f) c + sigmoid(i) tanh(g);  h' = sigmoid(o) tanh(c')
//   GRU   r = sigmoid(x_r + h_r);  z = sigmoid(x_z + h_z);  n = tanh(x_n + r * h_n);  h' = (1 - z) n + z h
//         with x_* = W_i* x + b_i* and h_* = W_h* h + b_h*
// The input projections of all time steps are one dense GEMM (amt_linear_ex_fwd) per layer and direction; this kernel is
// the part that cannot be batched over time.  One workgroup per (clip, direction) walks the sequence; the hidden-to-hidden
// matrix (G*d rows x d columns, G = 4 or 3 gates) stays in registers for the whole walk -- two threads per row, d/2 columns
// each (64 registers at d = 128) --, h lives in LDS and is read as broadcast float4s, so a step costs one half-row dot
// product per thread, one lane exchange, two barriers and d cell updates: ~1 us, no global traffic besides the step's
// G*d projected inputs and d outputs.
// Training: the same walk with the activations kept (amt_rnn_seq_train_fwd) and backpropagation through time over them
// (amt_rnn_seq_bwd, further down); the weight gradients are dense products the host runs on the GEMM.
#include "../../include/amt_hip.h"
#include "amt_common.h"
#include "kernels.h"

namespace {

__device__ __forceinline__ float sigm(float v) { return 1.0f / (1.0f + __expf(-v)); }

constexpr int MAXD = 128;               // hidden size limit: d/2 weights per thread in registers
__host__ __device__ constexpr int rsv_cols(int G) { return G == 4 ? 5 : 4; }      // reserve columns per direction, in units of d

// xp: [B][L][ldxp] projected inputs of this direction (columns [0, G*d): W_ih x + b_ih); whh [G*d][d]; bhh [G*d];
// y: [B][L][ldy], this direction writes columns [0, d) of its y pointer.  reverse: walk t = L-1 .. 0.
// gridDim.y == 2 (both directions of a bidirectional layer at once): direction dir = blockIdx.y reads columns
// [dir*G*d, (dir+1)*G*d) of xp, the dir-th of the stacked whh / bhh, writes columns [dir*d, (dir+1)*d) of y; dir 1 walks backwards.
// TRAIN: the same walk also leaves, per (row, direction), what the backward needs in rsv [B][L][ldr] (layout: amt_hip.h,
// amt_rnn_seq_train_fwd); y's arithmetic is untouched, and the eval instantiation is the kernel it was before the flag existed.
template <int G, bool TRAIN>
__device__ __forceinline__ void rnn_seq_body(const float* __restrict__ xp, int ldxp, const float* __restrict__ whh,
                                             const float* __restrict__ bhh, float* __restrict__ y, int ldy, int L, int d, int reverse,
                                             float* __restrict__ rsv, int ldr) {
    __shared__ __attribute__((aligned(16))) float sh[MAXD];          // h_{t-1}
    __shared__ float sa[4 * MAXD];                                  // W_hh h + b_hh per gate row
    const int tid = threadIdx.x, b = blockIdx.x;
    const int row = tid >> 1, half = tid & 1, R = G * d, hc = d >> 1;
    if (gridDim.y == 2) {
        const int dir = blockIdx.y;
        xp += dir * R; whh += (size_t)dir * R * d; bhh += dir * R; y += dir * d; reverse = dir;
        if constexpr (TRAIN) rsv += dir * rsv_cols(G) * d;
    }
    // this thread's half row of W_hh
    float w[MAXD / 2];
#pragma unroll
    for (int j = 0; j < MAXD / 2; ++j) w[j] = (row < R && j < hc) ? whh[(size_t)row * d + half * hc + j] : 0.f;
    const float bh = row < R ? bhh[row] : 0.f;
    float c = 0.f;                                                  // LSTM cell state of unit `tid` (tid < d)
    if (tid < d) sh[tid] = 0.f;
    __syncthreads();
    xp += (size_t)b * L * ldxp;
    y += (size_t)b * L * ldy;
    if constexpr (TRAIN) rsv += (size_t)b * L * ldr;
    for (int s = 0; s < L; ++s) {
        const int t = reverse ? L - 1 - s : s;
        const float* xr = xp + (size_t)t * ldxp;
        // issue this step's projected inputs early: they do not depend on the recurrence
        float xg[G];
        if (tid < d) {
#pragma unroll
            for (int g = 0; g < G; ++g) xg[g] = xr[g * d + tid];
        }
        float acc = 0.f;
        const float4* h4 = reinterpret_cast<const float4*>(sh + half * hc);
#pragma unroll
        for (int j = 0; j < MAXD / 8; ++j) {
            if (4 * j < hc) {
                const float4 hv = h4[j];
                acc += w[4 * j] * hv.x + w[4 * j + 1] * hv.y + w[4 * j + 2] * hv.z + w[4 * j + 3] * hv.w;
            }
        }
        acc += __shfl_xor(acc, 1, 64);
        if (row < R && half == 0) sa[row] = acc + bh;
        __syncthreads();
        if (tid < d) {
            float hn;
            if constexpr (G == 4) {
                const float ig = sigm(xg[0] + sa[tid]), fg = sigm(xg[1] + sa[d + tid]);
                const float gg = tanhf(xg[2] + sa[2 * d + tid]), og = sigm(xg[3] + sa[3 * d + tid]);
                c = fg * c + ig * gg;
                hn = og * tanhf(c);
                if constexpr (TRAIN) {
                    float* rr = rsv + (size_t)t * ldr + tid;
                    rr[0] = ig; rr[d] = fg; rr[2 * d] = gg; rr[3 * d] = og; rr[4 * d] = c;
                }
            } else {
                const float r = sigm(xg[0] + sa[tid]), z = sigm(xg[1] + sa[d + tid]);
                const float n = tanhf(xg[2] + r * sa[2 * d + tid]);
                hn = (1.0f - z) * n + z * sh[tid];
                if constexpr (TRAIN) {
                    float* rr = rsv + (size_t)t * ldr + tid;
                    rr[0] = r; rr[d] = z; rr[2 * d] = n; rr[3 * d] = sa[2 * d + tid];
                }
            }
            y[(size_t)t * ldy + tid] = hn;
            sh[tid] = hn;           // every reader of the old h has passed the barrier above
        }
        __syncthreads();
    }
}


template <int G>
__global__ __launch_bounds__(2 * 4 * MAXD) void rnn_seq_kernel(const float* __restrict__ xp, int ldxp, const float* __restrict__ whh,
                                                               const float* __restrict__ bhh, float* __restrict__ y, int ldy,
                                                               int L, int d, int reverse) {
    rnn_seq_body<G, false>(xp, ldxp, whh, bhh, y, ldy, L, d, reverse, nullptr, 0);
}

template <int G>
__global__ __launch_bounds__(2 * 4 * MAXD) void rnn_seq_train_kernel(const float* __restrict__ xp, int ldxp, const float* __restrict__ whh,
                                                                     const float* __restrict__ bhh, float* __restrict__ y, int ldy,
                                                                     int L, int d, int reverse, float* __restrict__ rsv, int ldr) {
    rnn_seq_body<G, true>(xp, ldxp, whh, bhh, y, ldy, L, d, reverse, rsv, ldr);
}

// ---- backpropagation through time ----
// One workgroup per (clip, direction) walks the forward's steps backwards.  With a = the pre-activations, per step:
//   LSTM  dh = dy_t + dh_rec;  dc = dc_next f_next + dh o (1 - tanh^2 c);  da_i = dc g i(1-i);  da_f = dc c_prev f(1-f);
//         da_g = dc i (1-g^2);  da_o = dh tanh(c) o(1-o);                  dh_rec = W_hh^T da
//   GRU   dh = dy_t + dh_rec + dh_next z_next;  da_n = dh (1-z)(1-n^2);  da_z = dh (h_prev - n) z(1-z);  da_r = da_n hl r(1-r);
//         the hidden side of the n gate sees da_n r (written to dhn; the input side sees da_n):  dh_rec = W_hh^T [da_r, da_z, da_n r]
// Eight threads per hidden unit j; thread (j, q) keeps W_hh[r][j] for the rows r of every eighth float4 of da (r = 32 k + 4 q + e)
// in registers for the whole walk: 64 at d = 128, the forward's budget.  The unit's eight lanes all do its (cheap) cell arithmetic so
// that dh stays in registers; lane q = 0 puts the G d values of da into LDS, every thread reads them back as float4s (the eight
// lanes of a unit read 128 consecutive bytes, the units of a wave the same ones) and a three-step DPP sum closes the dot product.
// da is double-buffered, so a step has one barrier.  The step's reserve / dy / h_prev values are asked for one step ahead.
constexpr int BW_PARTS = 8;
constexpr int MAXRP = 4 * MAXD;         // G d rounded up to a multiple of 32 (GRU at d = 8: 24 rows, 32 slots)

template <int G>
__global__ __launch_bounds__(BW_PARTS * MAXD) void rnn_seq_bwd_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ rsv,
                                                                      int ldr, const float* __restrict__ y, int ldy,
                                                                      const float* __restrict__ whh, float* __restrict__ dxp, int ldxp,
                                                                      float* __restrict__ dhn, int lddhn, int L, int d, int reverse) {
    __shared__ __attribute__((aligned(16))) float sda[2][MAXRP];    // da as the hidden side sees it
    __shared__ float sdn[2][MAXD];                                  // GRU: da_n as the input side sees it
    constexpr int NV = G == 4 ? 7 : 6;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int j = tid >> 3, q = tid & (BW_PARTS - 1), R = G * d, Rp = (R + 31) & ~31;
    if (gridDim.y == 2) {
        const int dir = blockIdx.y;
        dy += dir * d; rsv += dir * rsv_cols(G) * d; y += dir * d; whh += (size_t)dir * R * d; dxp += dir * R; reverse = dir;
        if constexpr (G == 3) dhn += dir * d;
    }
    float w[MAXRP / BW_PARTS];
#pragma unroll
    for (int k = 0; k < MAXRP / 32; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = 32 * k + 4 * q + e;
            w[4 * k + e] = r < R ? whh[(size_t)r * d + j] : 0.f;
        }
    }
    for (int i = tid; i < 2 * MAXRP; i += blockDim.x) (&sda[0][0])[i] = 0.f;      // the slots past G d stay zero
    __syncthreads();
    dy += (size_t)b * L * lddy; rsv += (size_t)b * L * ldr; y += (size_t)b * L * ldy; dxp += (size_t)b * L * ldxp;
    if constexpr (G == 3) dhn += (size_t)b * L * lddhn;

    // step s of the forward's order happened at time t(s); its predecessor's state is zero at s = 0
    auto load = [&](int s, float (&v)[NV]) {
        const int t = reverse ? L - 1 - s : s, tp = reverse ? t + 1 : t - 1;
        const float* rr = rsv + (size_t)t * ldr + j;
#pragma unroll
        for (int g = 0; g < rsv_cols(G); ++g) v[g] = rr[g * d];
        v[rsv_cols(G)] = dy[(size_t)t * lddy + j];
        if constexpr (G == 4) v[6] = s > 0 ? rsv[(size_t)tp * ldr + 4 * d + j] : 0.f;     // c_{prev}
        else v[5] = s > 0 ? y[(size_t)tp * ldy + j] : 0.f;                                // h_{prev}
    };
    float v[NV], nv[NV];
    load(L - 1, v);
    float dh_rec = 0.f, carry = 0.f;            // carry: LSTM dc_next f_next; GRU dh_next z_next
    for (int s = L - 1; s >= 0; --s) {
        const int cur = (L - 1 - s) & 1;
        const int t = reverse ? L - 1 - s : s;
#pragma unroll
        for (int i = 0; i < NV; ++i) nv[i] = 0.f;
        if (s > 0) load(s - 1, nv);
        if constexpr (G == 4) {
            const float ig = v[0], fg = v[1], gg = v[2], og = v[3], tc = tanhf(v[4]), cp = v[6];
            const float dh = v[5] + dh_rec;
            const float dc = carry + dh * og * (1.0f - tc * tc);
            carry = dc * fg;
            if (q == 0) {
                sda[cur][j] = dc * gg * ig * (1.0f - ig);
                sda[cur][d + j] = dc * cp * fg * (1.0f - fg);
                sda[cur][2 * d + j] = dc * ig * (1.0f - gg * gg);
                sda[cur][3 * d + j] = dh * tc * og * (1.0f - og);
            }
        } else {
            const float r = v[0], z = v[1], n = v[2], hl = v[3], hp = v[5];
            const float dh = v[4] + dh_rec + carry;
            const float dan = dh * (1.0f - z) * (1.0f - n * n);
            carry = dh * z;
            if (q == 0) {
                sda[cur][j] = dan * hl * r * (1.0f - r);
                sda[cur][d + j] = dh * (hp - n) * z * (1.0f - z);
                sda[cur][2 * d + j] = dan * r;
                sdn[cur][j] = dan;
            }
        }
        __syncthreads();
        if (tid < R) {                          // the step's one write of dxproj, coalesced
            float val = sda[cur][tid];
            if constexpr (G == 3) {
                if (tid >= 2 * d) {
                    dhn[(size_t)t * lddhn + tid - 2 * d] = val;
                    val = sdn[cur][tid - 2 * d];
                }
            }
            dxp[(size_t)t * ldxp + tid] = val;
        }
        float acc = 0.f;
        const float4* a4 = reinterpret_cast<const float4*>(sda[cur]) + q;
#pragma unroll
        for (int k = 0; k < MAXRP / 32; ++k) {
            if (32 * k < Rp) {
                const float4 a = a4[BW_PARTS * k];
                acc += w[4 * k] * a.x + w[4 * k + 1] * a.y + w[4 * k + 2] * a.z + w[4 * k + 3] * a.w;
            }
        }
        dh_rec = group_sum<BW_PARTS>(acc);
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = nv[i];
    }
}

}  // namespace

extern "C" int32_t amt_rnn_seq_fwd(const float* xproj, int32_t ldxp, const float* w_hh, const float* b_hh, float* y, int32_t ldy,
                                   int32_t B, int32_t L, int32_t d, int32_t gates, int32_t reverse, int32_t n_dirs, void* stream) {
    AMT_CHECK_ARG(xproj && w_hh && b_hh && y, "amt_rnn_seq_fwd: null pointer");
    AMT_CHECK_ARG(gates == 3 || gates == 4, "amt_rnn_seq_fwd: gates=%d (4 = LSTM, 3 = GRU)", gates);
    AMT_CHECK_ARG(B > 0 && L > 0 && d >= 8 && d <= MAXD && d % 8 == 0, "amt_rnn_seq_fwd: hidden size %d must be a multiple of 8, at most %d", d, MAXD);
    AMT_CHECK_ARG(n_dirs == 1 || n_dirs == 2, "amt_rnn_seq_fwd: n_dirs=%d", n_dirs);
    AMT_CHECK_ARG(ldxp >= n_dirs * gates * d && ldy >= n_dirs * d, "amt_rnn_seq_fwd: bad leading dimensions");
    hipStream_t s = (hipStream_t)stream;
    const int threads = 2 * gates * d;                       // two threads per gate row
    if (gates == 4) hipLaunchKernelGGL(rnn_seq_kernel<4>, dim3(B, n_dirs), dim3(threads), 0, s, xproj, ldxp, w_hh, b_hh, y, ldy, L, d, reverse);
    else hipLaunchKernelGGL(rnn_seq_kernel<3>, dim3(B, n_dirs), dim3(threads), 0, s, xproj, ldxp, w_hh, b_hh, y, ldy, L, d, reverse);
    AMT_LAUNCH_CHECK();
    return 0;
}

/* ---- training ---- */
static int32_t rnn_check(const char* fn, int32_t B, int32_t L, int32_t d, int32_t gates, int32_t n_dirs) {
    AMT_CHECK_ARG(gates == 3 || gates == 4, "%s: gates=%d (4 = LSTM, 3 = GRU)", fn, gates);
    AMT_CHECK_ARG(B > 0 && L > 0 && d >= 8 && d <= MAXD && d % 8 == 0, "%s: hidden size %d must be a multiple of 8, at most %d", fn, d, MAXD);
    AMT_CHECK_ARG(n_dirs == 1 || n_dirs == 2, "%s: n_dirs=%d", fn, n_dirs);
    return 0;
}

extern "C" int32_t amt_rnn_seq_train_fwd(const float* xproj, int32_t ldxp, const float* w_hh, const float* b_hh, float* y, int32_t ldy,
                                         float* reserve, int32_t ldr, int32_t B, int32_t L, int32_t d, int32_t gates, int32_t reverse,
                                         int32_t n_dirs, void* stream) {
    AMT_CHECK_ARG(xproj && w_hh && b_hh && y && reserve, "amt_rnn_seq_train_fwd: null pointer");
    if (rnn_check("amt_rnn_seq_train_fwd", B, L, d, gates, n_dirs)) return -1;
    AMT_CHECK_ARG(ldxp >= n_dirs * gates * d && ldy >= n_dirs * d && ldr >= n_dirs * rsv_cols(gates) * d,
                  "amt_rnn_seq_train_fwd: bad leading dimensions");
    hipStream_t s = (hipStream_t)stream;
    const int threads = 2 * gates * d;
    if (gates == 4) hipLaunchKernelGGL(rnn_seq_train_kernel<4>, dim3(B, n_dirs), dim3(threads), 0, s, xproj, ldxp, w_hh, b_hh, y, ldy, L, d, reverse, reserve, ldr);
    else hipLaunchKernelGGL(rnn_seq_train_kernel<3>, dim3(B, n_dirs), dim3(threads), 0, s, xproj, ldxp, w_hh, b_hh, y, ldy, L, d, reverse, reserve, ldr);
    AMT_LAUNCH_CHECK();
    return 0;
}

extern "C" int32_t amt_rnn_seq_bwd(const float* dy, int32_t lddy, const float* reserve, int32_t ldr, const float* y, int32_t ldy,
                                   const float* w_hh, float* dxproj, int32_t ldxp, float* dhn, int32_t lddhn, int32_t B, int32_t L,
                                   int32_t d, int32_t gates, int32_t reverse, int32_t n_dirs, void* stream) {
    AMT_CHECK_ARG(dy && reserve && y && w_hh && dxproj, "amt_rnn_seq_bwd: null pointer");
    if (rnn_check("amt_rnn_seq_bwd", B, L, d, gates, n_dirs)) return -1;
    AMT_CHECK_ARG(gates == 4 || dhn, "amt_rnn_seq_bwd: a GRU needs dhn (the hidden side of the n gate)");
    AMT_CHECK_ARG(lddy >= n_dirs * d && ldy >= n_dirs * d && ldr >= n_dirs * rsv_cols(gates) * d && ldxp >= n_dirs * gates * d &&
                  (gates == 4 || lddhn >= n_dirs * d), "amt_rnn_seq_bwd: bad leading dimensions");
    hipStream_t s = (hipStream_t)stream;
    const int threads = BW_PARTS * d;                        // eight threads per hidden unit
    if (gates == 4) hipLaunchKernelGGL(rnn_seq_bwd_kernel<4>, dim3(B, n_dirs), dim3(threads), 0, s, dy, lddy, reserve, ldr, y, ldy, w_hh, dxproj, ldxp, dhn, lddhn, L, d, reverse);
    else hipLaunchKernelGGL(rnn_seq_bwd_kernel<3>, dim3(B, n_dirs), dim3(threads), 0, s, dy, lddy, reserve, ldr, y, ldy, w_hh, dxproj, ldxp, dhn, lddhn, L, d, reverse);
    AMT_LAUNCH_CHECK();
    return 0;
}
