// LSTM / GRU recurrences of the regression heads beyond the register kernel's width (csrc/rnn.hip keeps W_hh in registers and stops
// at d = 128): hidden sizes 32 .. 512, a multiple of 32.  Same cell equations, same gate order, same sigm / tanhf, same layouts of
// xproj, y, reserve, dxproj and dhn as rnn.hip; the two files differ in who holds W_hh.
//
// Here nobody holds it: one step kernel is launched per time step on the caller's stream, and the stream's launch order is the only
// synchronisation between steps -- no flag, ticket, grid barrier or spin loop, no workgroup waits for another.  Both directions of a
// layer share a grid (direction on blockIdx.z, direction 1 walks t = L-1-s); further clips are further tiles on blockIdx.y.
//
// Both products run on the fp32 matrix pipe as 16 x 16 tiles (v_mfma_f32_16x16x4_f32): a step is bound by the L2 bytes and the MFMA
// passes of its busiest CU, so the tile that spreads a step over the most workgroups wins -- 16 columns rather than 32 doubles their
// number (profiles/rnn_wide_tiles32.json: 11.2 us per LSTM step at d = 512 with 32 x 32 tiles and one chunk in flight per wave, 7.2 now).  The K range is
// dealt to the waves in chunks of 16 (wave w takes chunks w, w + WAVES, ...: one float4 per lane and operand feeds four MFMAs, lane
// quarter q holding k = 16 c + 4 q + e); a wave asks for a whole batch of chunks before it multiplies the first, so a step pays one
// or two L2 round trips, not one per chunk.  The waves' partial tiles meet in LDS and are added in wave order: the sum's order is fixed.
//
// Forward step: a workgroup owns FW_U = 4 hidden units, i.e. the G * 4 <= 16 rows of W_hh that produce their gates (row slot n =
// gate n / 4, unit n % 4; a GRU leaves 4 slots zero), for 32 clips as two M tiles that share the W fragments (16 or fewer clips: one
// tile).  a[clip][slot] = h_{t-1}[clip][:] . W_hh[row][:]; h_{t-1} is read from y itself, the row the previous launch wrote; at the
// first step it is a predicate (the product is skipped), not a read.  Then 32 x 4 threads run the cell.  The LSTM's c lives in the
// caller's workspace in eval (each workgroup touches its own units only; the first step does not read it) and comes from the
// reserve row of the previous step in training, so both forwards compute y with the same operations.
//
// Backward step, the mirror image: a workgroup owns BW_U = 16 units (16 columns of W_hh, read as they lie: 16 lanes, 64 consecutive
// bytes per k) for 16 clips, K = G d rows of da_{t+1} -- the dxproj row the previous launch wrote, for a GRU its n block from dhn.
// It adds dy_t and the carried term (LSTM dc f, GRU dh z: B * n_dirs * d floats of workspace, again private to the workgroup's units
// and clips and not read at the first step), runs the cell backward from the reserve and writes dxproj (and dhn) once.  No atomics
// anywhere: the same inputs give the same bits.
#include "../../include/amt_hip.h"
#include "amt_common.h"
#include "kernels.h"

namespace {

__device__ __forceinline__ float sigm(float v) { return 1.0f / (1.0f + __expf(-v)); }

constexpr int WMIN = 32, WMAX = 512;                    // hidden sizes: multiples of 32 in [WMIN, WMAX]
constexpr int TILE = 16;                                // M and N of the MFMA, and the k's of a chunk
constexpr int FW_U = 4, FW_CLIPS = 2 * TILE;            // forward: units (4 * 4 = 16 row slots) and clips per workgroup
constexpr int FW_WAVES = 8, FW_BATCH = 4;               //          waves sharing K, chunks a wave asks for at once (d = 512: all of its 4)
constexpr int BW_U = TILE, BW_CLIPS = TILE;             // backward: units and clips per workgroup
constexpr int BW_WAVES = 16, BW_BATCH = 8;              //          (LSTM at d = 512: 128 chunks, 8 per wave, one batch)
constexpr int PLD = TILE + 1;                           // row stride of a partial tile in LDS
__host__ __device__ constexpr int rsv_cols(int G) { return G == 4 ? 5 : 4; }

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// acc += A[16 x 16] . B[16 x 16] for one chunk: lane quarter q holds k = 4 q + e of both operands, MFMA e sums over q
__device__ __forceinline__ f32x4 mfma_chunk(const float4 a, const float4 b, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}

// C/D layout of the 16x16 tile: col = lane & 15, row = 4 (lane >> 4) + reg
__device__ __forceinline__ void put_tile(float* part, const f32x4 acc, int lane) {
#pragma unroll
    for (int e = 0; e < 4; ++e) part[(4 * (lane >> 4) + e) * PLD + (lane & 15)] = acc[e];
}

// One time step s of the walk (time t = s, or L-1-s in a reversed direction) for FW_U units of up to FW_CLIPS clips.
// cws: eval LSTM only, c of (direction, clip, unit) at [(dir * B + b) * d + j].
template <int G, bool TRAIN>
__global__ __launch_bounds__(64 * FW_WAVES) void rnn_wide_fwd_step(const float* __restrict__ xp, int ldxp, const float* __restrict__ whh,
                                                                    const float* __restrict__ bhh, float* y, int ldy, float* rsv, int ldr,
                                                                    float* __restrict__ cws, int B, int L, int d, int s, int reverse) {
    __shared__ float part[FW_WAVES][FW_CLIPS * PLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int u0 = blockIdx.x * FW_U, b0 = blockIdx.y * FW_CLIPS, R = G * d;
    int dir = 0;
    if (gridDim.z == 2) {
        dir = blockIdx.z;
        xp += dir * R; whh += (size_t)dir * R * d; bhh += dir * R; y += dir * d; reverse = dir;
        if constexpr (TRAIN) rsv += dir * rsv_cols(G) * d;
    }
    const int t = reverse ? L - 1 - s : s, tp = reverse ? t + 1 : t - 1;
    // the cell's thread: clip m of the workgroup's, unit u of the slice
    const int m = tid / FW_U, u = tid % FW_U, b = b0 + m, j = u0 + u;
    const bool live = tid < FW_CLIPS * FW_U && b < B;
    // this step's projected inputs and the carried state do not depend on the product: ask early
    float xg[G], prev = 0.f;
    if (live) {
        const float* xr = xp + ((size_t)b * L + t) * ldxp + j;
#pragma unroll
        for (int g = 0; g < G; ++g) xg[g] = xr[g * d];
        if (s > 0) {
            if constexpr (G == 3) prev = y[((size_t)b * L + tp) * ldy + j];                                   // h_{t-1}
            else if constexpr (TRAIN) prev = rsv[((size_t)b * L + tp) * ldr + 4 * d + j];                     // c_{t-1}
            else prev = cws[((size_t)dir * B + b) * d + j];
        }
    }
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
        const bool two = b0 + TILE < B;                                                                        // clips in the second M tile
        const float* a0 = b0 + r < B ? y + ((size_t)(b0 + r) * L + tp) * ldy : nullptr;                        // h_{t-1} of clip r
        const float* a1 = b0 + TILE + r < B ? y + ((size_t)(b0 + TILE + r) * L + tp) * ldy : nullptr;          // ... of clip 16 + r
        const int g = r / FW_U;
        const float* wrow = g < G ? whh + ((size_t)g * d + u0 + r % FW_U) * d : nullptr;                      // row slot r
        const int nch = d / TILE;
        for (int c0 = wave; c0 < nch; c0 += FW_WAVES * FW_BATCH) {
            float4 va0[FW_BATCH], va1[FW_BATCH], vw[FW_BATCH];
#pragma unroll
            for (int i = 0; i < FW_BATCH; ++i) {
                const int c = c0 + i * FW_WAVES, k = TILE * c + 4 * q;
                const bool ok = c < nch;
                vw[i] = ok && wrow ? ld4(wrow + k) : zero4();
                va0[i] = ok && a0 ? ld4(a0 + k) : zero4();
                va1[i] = ok && a1 ? ld4(a1 + k) : zero4();
            }
#pragma unroll
            for (int i = 0; i < FW_BATCH; ++i) {
                if (c0 + i * FW_WAVES < nch) {
                    acc0 = mfma_chunk(va0[i], vw[i], acc0);
                    if (two) acc1 = mfma_chunk(va1[i], vw[i], acc1);
                }
            }
        }
    }
    put_tile(part[wave], acc0, lane);
    put_tile(part[wave] + TILE * PLD, acc1, lane);
    __syncthreads();
    if (!live) return;
    float sa[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int o = m * PLD + g * FW_U + u;
        sa[g] = (((part[0][o] + part[1][o]) + (part[2][o] + part[3][o])) + ((part[4][o] + part[5][o]) + (part[6][o] + part[7][o]))) + bhh[g * d + j];
    }
    float hn;
    if constexpr (G == 4) {
        const float ig = sigm(xg[0] + sa[0]), fg = sigm(xg[1] + sa[1]);
        const float gg = tanhf(xg[2] + sa[2]), og = sigm(xg[3] + sa[3]);
        const float c = fg * prev + ig * gg;
        hn = og * tanhf(c);
        if constexpr (TRAIN) {
            float* rr = rsv + ((size_t)b * L + t) * ldr + j;
            rr[0] = ig; rr[d] = fg; rr[2 * d] = gg; rr[3 * d] = og; rr[4 * d] = c;
        } else {
            cws[((size_t)dir * B + b) * d + j] = c;
        }
    } else {
        const float rg = sigm(xg[0] + sa[0]), z = sigm(xg[1] + sa[1]);
        const float n = tanhf(xg[2] + rg * sa[2]);
        hn = (1.0f - z) * n + z * prev;
        if constexpr (TRAIN) {
            float* rr = rsv + ((size_t)b * L + t) * ldr + j;
            rr[0] = rg; rr[d] = z; rr[2 * d] = n; rr[3 * d] = sa[2];
        }
    }
    y[((size_t)b * L + t) * ldy + j] = hn;
}

// Step s of the forward's order, walked from s = L-1 down: equations as rnn.hip's backward.
// cws: the carried term of (direction, clip, unit) at [(dir * B + b) * d + j]: LSTM dc f, GRU dh z.
template <int G>
__global__ __launch_bounds__(64 * BW_WAVES) void rnn_wide_bwd_step(const float* __restrict__ dy, int lddy, const float* __restrict__ rsv, int ldr,
                                                                    const float* __restrict__ y, int ldy, const float* __restrict__ whh,
                                                                    float* dxp, int ldxp, float* dhn, int lddhn, float* __restrict__ cws,
                                                                    int B, int L, int d, int s, int reverse) {
    __shared__ float part[BW_WAVES][BW_CLIPS * PLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int u0 = blockIdx.x * BW_U, b0 = blockIdx.y * BW_CLIPS, R = G * d;
    int dir = 0;
    if (gridDim.z == 2) {
        dir = blockIdx.z;
        dy += dir * d; rsv += dir * rsv_cols(G) * d; y += dir * d; whh += (size_t)dir * R * d; dxp += dir * R; reverse = dir;
        if constexpr (G == 3) dhn += dir * d;
    }
    const int t = reverse ? L - 1 - s : s, tp = reverse ? t + 1 : t - 1, tn = reverse ? t - 1 : t + 1;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (s < L - 1) {                                        // dh_rec = da_{s+1} W_hh[:, units]
        const bool ok = b0 + r < B;
        const float* ax = ok ? dxp + ((size_t)(b0 + r) * L + tn) * ldxp : nullptr;
        const float* an = nullptr;
        if constexpr (G == 3) an = ok ? dhn + ((size_t)(b0 + r) * L + tn) * lddhn : nullptr;
        const float* wcol = whh + u0 + r;
        const int nch = R / TILE;
        for (int c0 = wave; c0 < nch; c0 += BW_WAVES * BW_BATCH) {
            float4 va[BW_BATCH], vw[BW_BATCH];
#pragma unroll
            for (int i = 0; i < BW_BATCH; ++i) {
                const int c = c0 + i * BW_WAVES, k = TILE * c + 4 * q;
                va[i] = vw[i] = zero4();
                if (c < nch) {
                    if (ok) va[i] = (G == 3 && k >= 2 * d) ? ld4(an + (k - 2 * d)) : ld4(ax + k);
                    const float* w = wcol + (size_t)k * d;
                    vw[i] = make_float4(w[0], w[d], w[2 * (size_t)d], w[3 * (size_t)d]);
                }
            }
#pragma unroll
            for (int i = 0; i < BW_BATCH; ++i)
                if (c0 + i * BW_WAVES < nch) acc = mfma_chunk(va[i], vw[i], acc);
        }
    }
    put_tile(part[wave], acc, lane);
    __syncthreads();
    const int m = tid / BW_U, u = tid % BW_U, b = b0 + m, j = u0 + u;
    if (tid >= BW_CLIPS * BW_U || b >= B) return;
    const int o = m * PLD + u;
    float dh_rec = 0.f;
    {
        float p4[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) p4[w] = (part[4 * w][o] + part[4 * w + 1][o]) + (part[4 * w + 2][o] + part[4 * w + 3][o]);
        dh_rec = (p4[0] + p4[1]) + (p4[2] + p4[3]);
    }
    float* cw = cws + ((size_t)dir * B + b) * d + j;
    const float carry = s < L - 1 ? *cw : 0.f;
    const float* rr = rsv + ((size_t)b * L + t) * ldr + j;
    const float dyv = dy[((size_t)b * L + t) * lddy + j];
    float* dx = dxp + ((size_t)b * L + t) * ldxp + j;
    if constexpr (G == 4) {
        const float ig = rr[0], fg = rr[d], gg = rr[2 * d], og = rr[3 * d], tc = tanhf(rr[4 * d]);
        const float cp = s > 0 ? rsv[((size_t)b * L + tp) * ldr + 4 * d + j] : 0.f;
        const float dh = dyv + dh_rec;
        const float dc = carry + dh * og * (1.0f - tc * tc);
        *cw = dc * fg;
        dx[0] = dc * gg * ig * (1.0f - ig);
        dx[d] = dc * cp * fg * (1.0f - fg);
        dx[2 * d] = dc * ig * (1.0f - gg * gg);
        dx[3 * d] = dh * tc * og * (1.0f - og);
    } else {
        const float rg = rr[0], z = rr[d], n = rr[2 * d], hl = rr[3 * d];
        const float hp = s > 0 ? y[((size_t)b * L + tp) * ldy + j] : 0.f;
        const float dh = dyv + dh_rec + carry;
        const float dan = dh * (1.0f - z) * (1.0f - n * n);
        *cw = dh * z;
        dx[0] = dan * hl * rg * (1.0f - rg);
        dx[d] = dh * (hp - n) * z * (1.0f - z);
        dx[2 * d] = dan;
        dhn[((size_t)b * L + t) * lddhn + j] = dan * rg;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int32_t wide_check(const char* fn, int32_t B, int32_t L, int32_t d, int32_t gates, int32_t n_dirs) {
    AMT_CHECK_ARG(gates == 3 || gates == 4, "%s: gates=%d (4 = LSTM, 3 = GRU)", fn, gates);
    AMT_CHECK_ARG(d >= WMIN && d <= WMAX && d % 32 == 0, "%s: hidden size %d must be a multiple of 32 in %d..%d", fn, d, WMIN, WMAX);
    AMT_CHECK_ARG(B > 0 && L > 0, "%s: B=%d L=%d", fn, B, L);
    AMT_CHECK_ARG(n_dirs == 1 || n_dirs == 2, "%s: n_dirs=%d", fn, n_dirs);
    return 0;
}

template <bool TRAIN>
int32_t wide_fwd(const char* fn, const float* xproj, int32_t ldxp, const float* w_hh, const float* b_hh, float* y, int32_t ldy, float* reserve,
                 int32_t ldr, int32_t B, int32_t L, int32_t d, int32_t gates, int32_t reverse, int32_t n_dirs, float* ws, void* stream) {
    if (wide_check(fn, B, L, d, gates, n_dirs)) return -1;
    AMT_CHECK_ARG(ldxp >= n_dirs * gates * d && ldy >= n_dirs * d && (!TRAIN || ldr >= n_dirs * rsv_cols(gates) * d),
                  "%s: bad leading dimensions (ldxp=%d ldy=%d ldr=%d)", fn, ldxp, ldy, ldr);
    AMT_CHECK_ARG(ldy % 4 == 0 && aligned16(y) && aligned16(w_hh), "%s: y (ldy=%d) and w_hh are read as float4: 16-byte rows", fn, ldy);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(d / FW_U, cdiv(B, FW_CLIPS), n_dirs), block(64 * FW_WAVES);
    for (int s = 0; s < L; ++s) {
        if (gates == 4) hipLaunchKernelGGL((rnn_wide_fwd_step<4, TRAIN>), grid, block, 0, st, xproj, ldxp, w_hh, b_hh, y, ldy, reserve, ldr, ws, B, L, d, s, reverse);
        else hipLaunchKernelGGL((rnn_wide_fwd_step<3, TRAIN>), grid, block, 0, st, xproj, ldxp, w_hh, b_hh, y, ldy, reserve, ldr, ws, B, L, d, s, reverse);
    }
    AMT_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int64_t amt_rnn_wide_ws_floats(int32_t B, int32_t d, int32_t gates, int32_t n_dirs) {
    if (B <= 0 || d < WMIN || d > WMAX || d % 32 || (gates != 3 && gates != 4) || (n_dirs != 1 && n_dirs != 2)) return -1;
    return (int64_t)B * n_dirs * d;
}

extern "C" int32_t amt_rnn_wide_seq_fwd(const float* xproj, int32_t ldxp, const float* w_hh, const float* b_hh, float* y, int32_t ldy,
                                        int32_t B, int32_t L, int32_t d, int32_t gates, int32_t reverse, int32_t n_dirs, float* ws,
                                        void* stream) {
    AMT_CHECK_ARG(xproj && w_hh && b_hh && y && ws, "amt_rnn_wide_seq_fwd: null pointer");
    return wide_fwd<false>("amt_rnn_wide_seq_fwd", xproj, ldxp, w_hh, b_hh, y, ldy, nullptr, 0, B, L, d, gates, reverse, n_dirs, ws, stream);
}

extern "C" int32_t amt_rnn_wide_seq_train_fwd(const float* xproj, int32_t ldxp, const float* w_hh, const float* b_hh, float* y, int32_t ldy,
                                              float* reserve, int32_t ldr, int32_t B, int32_t L, int32_t d, int32_t gates, int32_t reverse,
                                              int32_t n_dirs, float* ws, void* stream) {
    AMT_CHECK_ARG(xproj && w_hh && b_hh && y && reserve && ws, "amt_rnn_wide_seq_train_fwd: null pointer");
    return wide_fwd<true>("amt_rnn_wide_seq_train_fwd", xproj, ldxp, w_hh, b_hh, y, ldy, reserve, ldr, B, L, d, gates, reverse, n_dirs, ws, stream);
}

extern "C" int32_t amt_rnn_wide_seq_bwd(const float* dy, int32_t lddy, const float* reserve, int32_t ldr, const float* y, int32_t ldy,
                                        const float* w_hh, float* dxproj, int32_t ldxp, float* dhn, int32_t lddhn, int32_t B, int32_t L,
                                        int32_t d, int32_t gates, int32_t reverse, int32_t n_dirs, float* ws, void* stream) {
    const char* fn = "amt_rnn_wide_seq_bwd";
    AMT_CHECK_ARG(dy && reserve && y && w_hh && dxproj && ws, "%s: null pointer", fn);
    if (wide_check(fn, B, L, d, gates, n_dirs)) return -1;
    AMT_CHECK_ARG(gates == 4 || dhn, "%s: a GRU needs dhn (the hidden side of the n gate)", fn);
    AMT_CHECK_ARG(lddy >= n_dirs * d && ldy >= n_dirs * d && ldr >= n_dirs * rsv_cols(gates) * d && ldxp >= n_dirs * gates * d &&
                  (gates == 4 || lddhn >= n_dirs * d), "%s: bad leading dimensions (lddy=%d ldr=%d ldy=%d ldxp=%d lddhn=%d)", fn, lddy, ldr, ldy,
                  ldxp, lddhn);
    AMT_CHECK_ARG(ldxp % 4 == 0 && aligned16(dxproj) && (gates == 4 || (lddhn % 4 == 0 && aligned16(dhn))),
                  "%s: dxproj (ldxp=%d) and dhn (lddhn=%d) are read back as float4: 16-byte rows", fn, ldxp, lddhn);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(d / BW_U, cdiv(B, BW_CLIPS), n_dirs), block(64 * BW_WAVES);
    for (int s = L - 1; s >= 0; --s) {
        if (gates == 4) hipLaunchKernelGGL(rnn_wide_bwd_step<4>, grid, block, 0, st, dy, lddy, reserve, ldr, y, ldy, w_hh, dxproj, ldxp, dhn, lddhn, ws, B, L, d, s, reverse);
        else hipLaunchKernelGGL(rnn_wide_bwd_step<3>, grid, block, 0, st, dy, lddy, reserve, ldr, y, ldy, w_hh, dxproj, ldxp, dhn, lddhn, ws, B, L, d, s, reverse);
    }
    AMT_LAUNCH_CHECK();
    return 0;
}
