// Backward of the two Mamba kernels of mamba.hip, for training VideoRegression(regModel = 'bimamba+' / 'bimamba'):
//   amt_selective_scan_bwd    from amt_selective_scan_train_fwd's un-gated y and its per-chunk state checkpoints
//   amt_dwconv1d_silu_bwd     from the forward's own inputs (the pre-activation is formed again)
//
// The scan's backward keeps the forward's block shape: 16 channels x 16 states per 256-thread block, a channel's states on 16
// adjacent lanes, grid (ceil(ED / 16), B).  It walks the chunks of SCAN_TCH steps from the last to the first.  Per chunk: the
// element-wise part (softplus, SiLU, the gate's derivative, dz) runs in parallel over (step, channel) and stages the recurrence's
// operands in LDS; every thread recomputes its state h_s for the chunk's steps from the checkpoint into registers; the sweep then
// runs the steps backwards with the carried dh.  With delta = softplus(draw + bias), a = exp(delta A):
//   dh += C_s dy;   dC_s[n] += h_s dy;   dB_s[n] += dh delta x;   d delta = sum_n dh (A a h_{s-1} + B_s x);
//   dx = sum_n dh delta B_s + ...;   dA[c][n] += dh delta a h_{s-1};   dh <- a dh
// Steps past the end of the sequence are staged as delta = 0, x = 0, dy = 0, B = C = 0: they change nothing.
//
// No floating-point atomic anywhere: dB / dC are summed over a wave's 4 channels by lane exchange, over the block's 4 waves through
// LDS, and over the ceil(ED / 16) blocks by a second launch that reads the workspace in a fixed order; dA and dD are per-(clip, block)
// partials that the same second launch sums over the clips.  The same inputs give the same bits.
// exp / sigmoid here are the accurate expf: the gradients are held to an fp64 yardstick at fp32 training noise.
//
//   amt_selective_scan_wide_bwd   the same for N = 32 / 64 / 128 / 256 states per channel ('moemamba': d_state = d_hidden), from
//                                 amt_selective_scan_wide_train_fwd's y_pre and checkpoints (every 32 steps, the same interval)
//   amt_silu_bwd                  da = dy silu'(a), the launch the backward of CNN_GRU's dense convolution front lacks
// The wide backward is the N = 16 kernel run per slice of 16 states, grid (ceil(ED / 16), B, N / 16), and not a lane that owns
// N / 16 states: hs[32] and as[32] per lane would become 32 N / 16 values each (1024 at N = 256), far past the register file, and a
// checkpoint interval short enough to fit them would multiply the checkpoint memory (already B ceil(L / 32) ED N floats).  Sliced, the
// register and LDS footprint is the N = 16 kernel's, and a B = 1 call has N / 16 times the workgroups.  The price is that every
// slice forms softplus and the gate's dy again (element-wise, cheap beside the recurrence) and that the sums over all states cross
// blocks: they go through the workspace as per-slice partials and are added in slice order by the second launch.
#include "../../include/amt_hip.h"
#include "amt_common.h"
#include "kernels.h"

namespace {

constexpr int N = 16, TCH = SCAN_TCH, CPB = SCAN_CPB, NT = CPB * N, WAVES = NT / 64;
constexpr int CONV_MAXK = 8, CONV_CH = 64, CONV_ROWS = 64;     // conv backward: channels x rows of a block's tile

__device__ __forceinline__ float sigmoid_acc(float v) { return 1.0f / (1.0f + expf(-v)); }

struct ScanBwdParams {
    const float* dout; int lddo;        // [B*L][ED] gradient of the gated output
    const float* x; int ldx;
    const float* draw; int ldd;
    const float* dt_bias; const float* A_log;
    const float* Bm; const float* Cm; int ldbc;
    const float* D;
    const float* z; int ldz;
    const float* ypre; int ldyp;
    const float* hck;
    float* dx; int lddx;                // [B*L][ED]
    float* ddraw; int lddd;             // [B*L][ED]
    float* dz; int lddz;                // [B*L][ED] (the z half of dxz)
    float* ws;                          // [B][nblk][L][2N] dB | dC partials, then [B][ED][N] dA partials, then [B][ED] dD partials
    int B, L, ED, version, reverse;
};

__global__ __launch_bounds__(NT) void selective_scan_bwd_kernel(ScanBwdParams p) {
    __shared__ float sx[TCH][CPB], sd[TCH][CPB], sdy[TCH][CPB], sdd[TCH][CPB], sdxs[TCH][CPB], sB[TCH][N], sC[TCH][N];
    __shared__ float pB[TCH][WAVES][N], pC[TCH][WAVES][N], sDp[NT / CPB][CPB];
    const int tid = threadIdx.x, n = tid % N, cl = tid / N, wave = tid / 64, lane = tid % 64;
    const int c0 = blockIdx.x * CPB, b = blockIdx.y, nblk = gridDim.x, nch = (p.L + TCH - 1) / TCH;
    const int ch = c0 + cl;
    const float A = ch < p.ED ? -expf(p.A_log[(size_t)ch * N + n]) : 0.f;
    // the element-wise mapping: this thread's channel ecc, steps es and es + NT / CPB of a chunk
    constexpr int EPT = TCH * CPB / NT, BPT = TCH * N / NT, ESTEP = NT / CPB;
    const int ecc = tid % CPB, es = tid / CPB;
    const bool ech = c0 + ecc < p.ED;
    const float e_bias = ech ? p.dt_bias[c0 + ecc] : 0.f, e_D = ech ? p.D[c0 + ecc] : 0.f;
    float* wsBC = p.ws + ((size_t)b * nblk + blockIdx.x) * p.L * (2 * N);
    float dh = 0.f, dA = 0.f, dDp = 0.f;

    for (int k = nch - 1; k >= 0; --k) {
        const int s0 = k * TCH, steps = min(TCH, p.L - s0);
        float r_sig[EPT], r_dxe[EPT];
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int s = es + e * ESTEP;
            const int t = p.reverse ? p.L - 1 - (s0 + s) : s0 + s;
            const size_t row = (size_t)b * p.L + t;
            const bool ok = s < steps && ech;
            float xv = 0.f, delta = 0.f, dy = 0.f;
            r_sig[e] = 0.f; r_dxe[e] = 0.f;
            if (ok) {
                xv = p.x[row * p.ldx + c0 + ecc];
                const float dr = p.draw[row * p.ldd + c0 + ecc] + e_bias, zv = p.z[row * p.ldz + c0 + ecc];
                const float dov = p.dout[row * p.lddo + c0 + ecc], yp = p.ypre[row * p.ldyp + c0 + ecc];
                delta = dr > 20.f ? dr : log1pf(expf(dr));               // torch's softplus, threshold 20
                r_sig[e] = dr > 20.f ? 1.0f : sigmoid_acc(dr);            // and its derivative
                const float sgz = sigmoid_acc(zv), zs = zv * sgz;
                dy = dov * zs;
                float dzs = dov * yp, dxe = e_D * dy;
                if (p.version == 1) {                                      // out = y zs + x (1 - sigmoid(zs))
                    const float sg = sigmoid_acc(zs);
                    dzs -= dov * xv * (sg * (1.0f - sg));
                    dxe += dov * (1.0f - sg);
                }
                p.dz[row * p.lddz + c0 + ecc] = dzs * (sgz * (1.0f + zv * (1.0f - sgz)));
                r_dxe[e] = dxe;
                dDp += dy * xv;
            }
            sx[s][ecc] = xv; sd[s][ecc] = delta; sdy[s][ecc] = dy;
        }
#pragma unroll
        for (int e = 0; e < BPT; ++e) {
            const int i = tid + e * NT, s = i / N, nn = i % N;
            const int t = p.reverse ? p.L - 1 - (s0 + s) : s0 + s;
            const size_t row = (size_t)b * p.L + t;
            sB[s][nn] = s < steps ? p.Bm[row * p.ldbc + nn] : 0.f;
            sC[s][nn] = s < steps ? p.Cm[row * p.ldbc + nn] : 0.f;
        }
        const float h0 = ch < p.ED ? p.hck[(((size_t)b * nch + k) * p.ED + ch) * N + n] : 0.f;
        __syncthreads();
        // the chunk's states again, from its checkpoint
        float hs[TCH], as[TCH];
        {
            float h = h0;
#pragma unroll
            for (int s = 0; s < TCH; ++s) {
                const float delta = sd[s][cl];
                as[s] = expf(delta * A);
                h = as[s] * h + (delta * sB[s][n]) * sx[s][cl];
                hs[s] = h;
            }
        }
        // the sweep against the walking order
#pragma unroll
        for (int s = TCH - 1; s >= 0; --s) {
            const float delta = sd[s][cl], xv = sx[s][cl], dy = sdy[s][cl], Bn = sB[s][n], Cn = sC[s][n];
            const float hp = s > 0 ? hs[s - 1] : h0;
            dh += Cn * dy;
            float cC = hs[s] * dy, cB = dh * delta * xv;
            cC += __shfl_xor(cC, 16, 64); cC += __shfl_xor(cC, 32, 64);          // the wave's 4 channels
            cB += __shfl_xor(cB, 16, 64); cB += __shfl_xor(cB, 32, 64);
            if (lane < N) { pC[s][wave][n] = cC; pB[s][wave][n] = cB; }
            const float t1 = dh * as[s] * hp;                                     // dh a h_{s-1}
            const float dd = group_sum<N>(A * t1 + dh * Bn * xv);
            const float dxs = group_sum<N>(dh * delta * Bn);
            if (n == 0) { sdd[s][cl] = dd; sdxs[s][cl] = dxs; }
            dA += delta * t1;
            dh = as[s] * dh;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int s = es + e * ESTEP;
            const int t = p.reverse ? p.L - 1 - (s0 + s) : s0 + s;
            const size_t row = (size_t)b * p.L + t;
            if (s < steps && ech) {
                p.ddraw[row * p.lddd + c0 + ecc] = sdd[s][ecc] * r_sig[e];
                p.dx[row * p.lddx + c0 + ecc] = sdxs[s][ecc] + r_dxe[e];
            }
        }
#pragma unroll
        for (int e = 0; e < BPT; ++e) {
            const int i = tid + e * NT, s = i / N, nn = i % N;
            const int t = p.reverse ? p.L - 1 - (s0 + s) : s0 + s;
            if (s < steps) {
                float vB = pB[s][0][nn], vC = pC[s][0][nn];
#pragma unroll
                for (int w = 1; w < WAVES; ++w) { vB += pB[s][w][nn]; vC += pC[s][w][nn]; }
                wsBC[(size_t)t * (2 * N) + nn] = vB;
                wsBC[(size_t)t * (2 * N) + N + nn] = vC;
            }
        }
        __syncthreads();
    }
    float* wsA = p.ws + (size_t)p.B * nblk * p.L * (2 * N);
    float* wsD = wsA + (size_t)p.B * p.ED * N;
    if (ch < p.ED) wsA[((size_t)b * p.ED + ch) * N + n] = dA;
    sDp[es][ecc] = dDp;
    __syncthreads();
    if (tid < CPB && c0 + tid < p.ED) {
        float v = sDp[0][tid];
        for (int i = 1; i < NT / CPB; ++i) v += sDp[i][tid];
        wsD[(size_t)b * p.ED + c0 + tid] = v;
    }
}

// The second launch: dB | dC over the channel blocks, dA (times A: the gradient of A_log) and dD over the clips, each in index order.
__global__ void scan_bwd_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ A_log, float* __restrict__ dBm,
                                       float* __restrict__ dCm, int ldbc, float* __restrict__ dA_log, float* __restrict__ dD,
                                       int B, int L, int ED, int nblk) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nBC = (size_t)B * L * (2 * N), nA = (size_t)ED * N;
    if (idx < nBC) {
        const size_t row = idx / (2 * N);
        const int j = (int)(idx % (2 * N)), b = (int)(row / L), t = (int)(row % L);
        float v = 0.f;
        for (int blk = 0; blk < nblk; ++blk) v += ws[(((size_t)b * nblk + blk) * L + t) * (2 * N) + j];
        if (j < N) dBm[row * ldbc + j] = v;
        else dCm[row * ldbc + (j - N)] = v;
    } else if (idx < nBC + nA) {
        const size_t i = idx - nBC;
        const float* wsA = ws + (size_t)B * nblk * L * (2 * N);
        float v = 0.f;
        for (int b = 0; b < B; ++b) v += wsA[(size_t)b * nA + i];
        dA_log[i] = v * -expf(A_log[i]);
    } else if (idx < nBC + nA + (size_t)ED) {
        const size_t c = idx - nBC - nA;
        const float* wsD = ws + (size_t)B * nblk * L * (2 * N) + (size_t)B * nA;
        float v = 0.f;
        for (int b = 0; b < B; ++b) v += wsD[(size_t)b * ED + c];
        dD[c] = v;
    }
}

// ---- the wide-state scan (N = 32 .. 256 states per channel) ----
// State slices: grid (ceil(ED / 16), B, N / 16); slice z does the kernel above's work on states [16 z, 16 z + 16) of its 16 channels.
// What a slice cannot finish alone goes to the workspace and is finished by the second launch in index order: its 16 columns of the
// per-channel-block dB | dC copies, its dA, and the two sums over all N states (d delta and the scan's part of dx) as per-slice
// partials.  The element-wise part that does not depend on the state (softplus', dz, the D x and Mamba+ terms of dx) is done once,
// in the second launch; slice 0 keeps the per-clip partial of dD, as the kernel above does.
// The staging, the recomputation, the sweep and the dB | dC write-out below are selective_scan_bwd_kernel's, line for line, with the
// state offset z16 and the row width NF in the indices: a change to either kernel belongs in both.  They are two kernels and not one
// templated body because the merged body compiled to 225 (N = 16) and 210 (sliced) VGPRs against 171 and 157 apart, which takes the
// sliced kernel from 3 waves per SIMD to 2.
struct ScanWideBwdParams {
    ScanBwdParams q;                    // q.ws: [B][nblk][L][2N] dB | dC, [B][ED][N] dA, [B][ED] dD, [N/16][B*L][ED] d delta, the same of dx
    int N;
};

__global__ __launch_bounds__(NT) void selective_scan_wide_bwd_kernel(ScanWideBwdParams pw) {
    const ScanBwdParams& p = pw.q;
    __shared__ float sx[TCH][CPB], sd[TCH][CPB], sdy[TCH][CPB], sdd[TCH][CPB], sdxs[TCH][CPB], sB[TCH][N], sC[TCH][N];
    __shared__ float pB[TCH][WAVES][N], pC[TCH][WAVES][N], sDp[NT / CPB][CPB];
    const int NF = pw.N, z16 = blockIdx.z * N;
    const int tid = threadIdx.x, n = tid % N, cl = tid / N, wave = tid / 64, lane = tid % 64;
    const int c0 = blockIdx.x * CPB, b = blockIdx.y, nblk = gridDim.x, nch = (p.L + TCH - 1) / TCH;
    const int ch = c0 + cl;
    const float A = ch < p.ED ? -expf(p.A_log[(size_t)ch * NF + z16 + n]) : 0.f;
    constexpr int EPT = TCH * CPB / NT, BPT = TCH * N / NT, ESTEP = NT / CPB;
    const int ecc = tid % CPB, es = tid / CPB;
    const bool ech = c0 + ecc < p.ED;
    const float e_bias = ech ? p.dt_bias[c0 + ecc] : 0.f;
    const size_t rows = (size_t)p.B * p.L;
    float* wsBC = p.ws + ((size_t)b * nblk + blockIdx.x) * p.L * (2 * NF);
    float* wsA = p.ws + (size_t)p.B * nblk * p.L * (2 * NF);
    float* wsD = wsA + (size_t)p.B * p.ED * NF;
    float* wsDd = wsD + (size_t)p.B * p.ED + (size_t)blockIdx.z * rows * p.ED;
    float* wsDx = wsDd + (size_t)gridDim.z * rows * p.ED;
    float dh = 0.f, dA = 0.f, dDp = 0.f;

    for (int k = nch - 1; k >= 0; --k) {
        const int s0 = k * TCH, steps = min(TCH, p.L - s0);
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int s = es + e * ESTEP;
            const int t = p.reverse ? p.L - 1 - (s0 + s) : s0 + s;
            const size_t row = (size_t)b * p.L + t;
            float xv = 0.f, delta = 0.f, dy = 0.f;
            if (s < steps && ech) {
                xv = p.x[row * p.ldx + c0 + ecc];
                const float dr = p.draw[row * p.ldd + c0 + ecc] + e_bias, zv = p.z[row * p.ldz + c0 + ecc];
                delta = dr > 20.f ? dr : log1pf(expf(dr));
                dy = p.dout[row * p.lddo + c0 + ecc] * (zv * sigmoid_acc(zv));
                dDp += dy * xv;
            }
            sx[s][ecc] = xv; sd[s][ecc] = delta; sdy[s][ecc] = dy;
        }
#pragma unroll
        for (int e = 0; e < BPT; ++e) {
            const int i = tid + e * NT, s = i / N, nn = i % N;
            const int t = p.reverse ? p.L - 1 - (s0 + s) : s0 + s;
            const size_t row = (size_t)b * p.L + t;
            sB[s][nn] = s < steps ? p.Bm[row * p.ldbc + z16 + nn] : 0.f;
            sC[s][nn] = s < steps ? p.Cm[row * p.ldbc + z16 + nn] : 0.f;
        }
        const float h0 = ch < p.ED ? p.hck[(((size_t)b * nch + k) * p.ED + ch) * NF + z16 + n] : 0.f;
        __syncthreads();
        float hs[TCH], as[TCH];
        {
            float h = h0;
#pragma unroll
            for (int s = 0; s < TCH; ++s) {
                const float delta = sd[s][cl];
                as[s] = expf(delta * A);
                h = as[s] * h + (delta * sB[s][n]) * sx[s][cl];
                hs[s] = h;
            }
        }
#pragma unroll
        for (int s = TCH - 1; s >= 0; --s) {
            const float delta = sd[s][cl], xv = sx[s][cl], dy = sdy[s][cl], Bn = sB[s][n], Cn = sC[s][n];
            const float hp = s > 0 ? hs[s - 1] : h0;
            dh += Cn * dy;
            float cC = hs[s] * dy, cB = dh * delta * xv;
            cC += __shfl_xor(cC, 16, 64); cC += __shfl_xor(cC, 32, 64);
            cB += __shfl_xor(cB, 16, 64); cB += __shfl_xor(cB, 32, 64);
            if (lane < N) { pC[s][wave][n] = cC; pB[s][wave][n] = cB; }
            const float t1 = dh * as[s] * hp;
            const float dd = group_sum<N>(A * t1 + dh * Bn * xv);
            const float dxs = group_sum<N>(dh * delta * Bn);
            if (n == 0) { sdd[s][cl] = dd; sdxs[s][cl] = dxs; }
            dA += delta * t1;
            dh = as[s] * dh;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int s = es + e * ESTEP;
            const int t = p.reverse ? p.L - 1 - (s0 + s) : s0 + s;
            const size_t row = (size_t)b * p.L + t;
            if (s < steps && ech) {
                wsDd[row * p.ED + c0 + ecc] = sdd[s][ecc];
                wsDx[row * p.ED + c0 + ecc] = sdxs[s][ecc];
            }
        }
#pragma unroll
        for (int e = 0; e < BPT; ++e) {
            const int i = tid + e * NT, s = i / N, nn = i % N;
            const int t = p.reverse ? p.L - 1 - (s0 + s) : s0 + s;
            if (s < steps) {
                float vB = pB[s][0][nn], vC = pC[s][0][nn];
#pragma unroll
                for (int w = 1; w < WAVES; ++w) { vB += pB[s][w][nn]; vC += pC[s][w][nn]; }
                wsBC[(size_t)t * (2 * NF) + z16 + nn] = vB;
                wsBC[(size_t)t * (2 * NF) + NF + z16 + nn] = vC;
            }
        }
        __syncthreads();
    }
    if (ch < p.ED) wsA[((size_t)b * p.ED + ch) * NF + z16 + n] = dA;
    if (blockIdx.z == 0) {
        sDp[es][ecc] = dDp;
        __syncthreads();
        if (tid < CPB && c0 + tid < p.ED) {
            float v = sDp[0][tid];
            for (int i = 1; i < NT / CPB; ++i) v += sDp[i][tid];
            wsD[(size_t)b * p.ED + c0 + tid] = v;
        }
    }
}

// The second launch: dB | dC over the channel blocks, dA (times A) and dD over the clips, and per (row, channel) the slices' partials in
// slice order with the element-wise part: ddraw = d delta softplus', dx = the scan's part + D dy (+ the Mamba+ term), dz.
__global__ void scan_wide_bwd_reduce_kernel(ScanWideBwdParams pw, float* __restrict__ dBm, float* __restrict__ dCm, int ldbc,
                                            float* __restrict__ dA_log, float* __restrict__ dD, int nblk) {
    const ScanBwdParams& p = pw.q;
    const int NF = pw.N, B = p.B, L = p.L, ED = p.ED, nsl = NF / N;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t rows = (size_t)B * L, nBC = rows * (2 * NF), nA = (size_t)ED * NF, nE = rows * ED;
    const float* wsA = p.ws + (size_t)B * nblk * L * (2 * NF);
    const float* wsD = wsA + (size_t)B * nA;
    const float* wsDd = wsD + (size_t)B * ED;
    const float* wsDx = wsDd + (size_t)nsl * nE;
    if (idx < nBC) {
        const size_t row = idx / (2 * NF);
        const int j = (int)(idx % (2 * NF)), b = (int)(row / L), t = (int)(row % L);
        float v = 0.f;
        for (int blk = 0; blk < nblk; ++blk) v += p.ws[(((size_t)b * nblk + blk) * L + t) * (2 * NF) + j];
        if (j < NF) dBm[row * ldbc + j] = v;
        else dCm[row * ldbc + (j - NF)] = v;
    } else if (idx < nBC + nA) {
        const size_t i = idx - nBC;
        float v = 0.f;
        for (int b = 0; b < B; ++b) v += wsA[(size_t)b * nA + i];
        dA_log[i] = v * -expf(p.A_log[i]);
    } else if (idx < nBC + nA + (size_t)ED) {
        const size_t c = idx - nBC - nA;
        float v = 0.f;
        for (int b = 0; b < B; ++b) v += wsD[(size_t)b * ED + c];
        dD[c] = v;
    } else if (idx < nBC + nA + (size_t)ED + nE) {
        const size_t i = idx - nBC - nA - ED, row = i / ED;
        const int c = (int)(i % ED);
        float dd = 0.f, dxs = 0.f;
        for (int s = 0; s < nsl; ++s) { dd += wsDd[(size_t)s * nE + i]; dxs += wsDx[(size_t)s * nE + i]; }
        const float xv = p.x[row * p.ldx + c], dr = p.draw[row * p.ldd + c] + p.dt_bias[c], zv = p.z[row * p.ldz + c];
        const float dov = p.dout[row * p.lddo + c], yp = p.ypre[row * p.ldyp + c];
        const float sgz = sigmoid_acc(zv), zs = zv * sgz, dy = dov * zs;
        float dzs = dov * yp, dxe = p.D[c] * dy;
        if (p.version == 1) {
            const float sg = sigmoid_acc(zs);
            dzs -= dov * xv * (sg * (1.0f - sg));
            dxe += dov * (1.0f - sg);
        }
        p.dz[row * p.lddz + c] = dzs * (sgz * (1.0f + zv * (1.0f - sgz)));
        p.ddraw[row * p.lddd + c] = dd * (dr > 20.f ? 1.0f : sigmoid_acc(dr));
        p.dx[row * p.lddx + c] = dxs + dxe;
    }
}

// da = dy silu'(a)
__global__ void silu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ a, float* __restrict__ da, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = a[i], sg = sigmoid_acc(v);
    da[i] = dy[i] * (sg * (1.0f + v * (1.0f - sg)));
}

// ---- depthwise conv + SiLU ----
// dacc = dy silu'(acc), acc the forward's pre-activation formed again
__global__ void dwconv_silu_dacc_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ x, int ldx,
                                        const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ dacc,
                                        int B, int L, int C, int K, int reverse) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)B * L * C;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const int l = (int)((idx / C) % L);
    const int b = (int)(idx / ((size_t)C * L));
    float acc = bias ? bias[c] : 0.f;
    for (int j = 0; j < K; ++j) {
        const int t = reverse ? l + (K - 1 - j) : l - (K - 1) + j;
        if (t >= 0 && t < L) acc += w[c * K + j] * x[((size_t)b * L + t) * ldx + c];
    }
    const float sg = sigmoid_acc(acc);
    dacc[idx] = dy[((size_t)b * L + l) * lddy + c] * (sg * (1.0f + acc * (1.0f - sg)));
}

// One block: CONV_CH channels x CONV_ROWS rows.  dx of its rows; its rows' share of dw | dbias -> part[slice][c][K + 1].
__global__ __launch_bounds__(256) void dwconv_silu_bwd_kernel(const float* __restrict__ dacc, const float* __restrict__ x, int ldx,
                                                              const float* __restrict__ w, float* __restrict__ dx, int lddx,
                                                              float* __restrict__ part, int B, int L, int C, int K, int reverse) {
    constexpr int RL = 256 / CONV_CH;                      // row lanes
    __shared__ float sred[RL][CONV_CH][CONV_MAXK + 1];
    const int cx = threadIdx.x % CONV_CH, rl = threadIdx.x / CONV_CH;
    const int c = blockIdx.x * CONV_CH + cx;
    const size_t rows = (size_t)B * L;
    float wr[CONV_MAXK], dwp[CONV_MAXK], dbp = 0.f;
#pragma unroll
    for (int j = 0; j < CONV_MAXK; ++j) {
        wr[j] = (c < C && j < K) ? w[c * K + j] : 0.f;
        dwp[j] = 0.f;
    }
    if (c < C) {
        for (int i = 0; i < CONV_ROWS / RL; ++i) {
            const size_t row = (size_t)blockIdx.y * CONV_ROWS + rl + (size_t)i * RL;
            if (row >= rows) break;
            const int b = (int)(row / L), l = (int)(row % L);
            const float da = dacc[row * C + c];
            float g = 0.f;
#pragma unroll
            for (int j = 0; j < CONV_MAXK; ++j) {
                if (j < K) {
                    // output position lo read x[l] through tap j; this row's own output read x[ti] through tap j
                    const int lo = reverse ? l - (K - 1) + j : l + (K - 1) - j;
                    if (lo >= 0 && lo < L) g += wr[j] * dacc[((size_t)b * L + lo) * C + c];
                    const int ti = reverse ? l + (K - 1 - j) : l - (K - 1) + j;
                    if (ti >= 0 && ti < L) dwp[j] += da * x[((size_t)b * L + ti) * ldx + c];
                }
            }
            dbp += da;
            dx[row * lddx + c] = g;
        }
    }
#pragma unroll
    for (int j = 0; j < CONV_MAXK; ++j) sred[rl][cx][j] = dwp[j];
    sred[rl][cx][CONV_MAXK] = dbp;
    __syncthreads();
    if (rl == 0 && c < C) {
        for (int j = 0; j <= K; ++j) {
            const int jj = j < K ? j : CONV_MAXK;
            float v = sred[0][cx][jj];
            for (int r = 1; r < RL; ++r) v += sred[r][cx][jj];
            part[((size_t)blockIdx.y * C + c) * (K + 1) + j] = v;
        }
    }
}

__global__ void dwconv_silu_bwd_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ dbias,
                                              int slices, int C, int K) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= C * (K + 1)) return;
    const int c = idx / (K + 1), j = idx % (K + 1);
    float v = 0.f;
    for (int s = 0; s < slices; ++s) v += part[((size_t)s * C + c) * (K + 1) + j];
    if (j < K) dw[c * K + j] = v;
    else if (dbias) dbias[c] = v;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" int64_t amt_selective_scan_bwd_ws_floats(int32_t B, int32_t L, int32_t ED, int32_t Ns) {
    if (B <= 0 || L <= 0 || ED <= 0 || Ns != N) return 0;
    return (int64_t)B * cdiv(ED, CPB) * L * (2 * N) + (int64_t)B * ED * (N + 1);
}

extern "C" int32_t amt_selective_scan_bwd(const float* dout, int32_t ld_dout, const float* x, int32_t ldx, const float* delta_raw,
                                          int32_t ld_delta, const float* dt_bias, const float* A_log, const float* Bm, const float* Cm,
                                          int32_t ld_bc, const float* D, const float* z, int32_t ldz, const float* y_pre, int32_t ld_ypre,
                                          const float* h_chunks, float* dx, int32_t lddx, float* ddraw, int32_t ld_ddraw, float* dz,
                                          int32_t lddz, float* dBm, float* dCm, int32_t ld_dbc, float* dA_log, float* dD, float* ws,
                                          int32_t B, int32_t L, int32_t ED, int32_t Ns, int32_t version, int32_t reverse, void* stream) {
    AMT_CHECK_ARG(dout && x && delta_raw && dt_bias && A_log && Bm && Cm && D && z && y_pre && h_chunks, "amt_selective_scan_bwd: null input pointer");
    AMT_CHECK_ARG(dx && ddraw && dz && dBm && dCm && dA_log && dD && ws, "amt_selective_scan_bwd: null output pointer");
    AMT_CHECK_ARG(B > 0 && L > 0 && ED > 0, "amt_selective_scan_bwd: bad shape B=%d L=%d ED=%d", B, L, ED);
    AMT_CHECK_ARG(Ns == N, "amt_selective_scan_bwd: d_state=%d: the backward is built for 16 states per channel (the reference's default) "
                  "only; wider states run inference", Ns);
    AMT_CHECK_ARG(version == 0 || version == 1, "amt_selective_scan_bwd: version %d not in {0,1}", version);
    AMT_CHECK_ARG(ld_dout >= ED && ldx >= ED && ld_delta >= ED && ldz >= ED && ld_ypre >= ED && lddx >= ED && ld_ddraw >= ED && lddz >= ED &&
                  ld_bc >= N && ld_dbc >= N, "amt_selective_scan_bwd: bad leading dimension");
    const int64_t total = (int64_t)B * L * (2 * N) + (int64_t)ED * (N + 1);         // elements of the second launch
    AMT_CHECK_ARG(B <= 65535 && (total + 255) / 256 <= 0x7fffffff, "amt_selective_scan_bwd: B=%d L=%d exceed the launch grid", B, L);
    ScanBwdParams p{};
    p.dout = dout; p.lddo = ld_dout; p.x = x; p.ldx = ldx; p.draw = delta_raw; p.ldd = ld_delta; p.dt_bias = dt_bias; p.A_log = A_log;
    p.Bm = Bm; p.Cm = Cm; p.ldbc = ld_bc; p.D = D; p.z = z; p.ldz = ldz; p.ypre = y_pre; p.ldyp = ld_ypre; p.hck = h_chunks;
    p.dx = dx; p.lddx = lddx; p.ddraw = ddraw; p.lddd = ld_ddraw; p.dz = dz; p.lddz = lddz; p.ws = ws;
    p.B = B; p.L = L; p.ED = ED; p.version = version; p.reverse = reverse;
    const int nblk = cdiv(ED, CPB);
    hipLaunchKernelGGL(selective_scan_bwd_kernel, dim3(nblk, B), dim3(NT), 0, (hipStream_t)stream, p);
    AMT_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_bwd_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws, A_log, dBm, dCm,
                       ld_dbc, dA_log, dD, B, L, ED, nblk);
    AMT_LAUNCH_CHECK();
    return 0;
}

static_assert(SCAN_WIDE_CKPT == TCH, "the wide backward recomputes one checkpoint interval per chunk");

extern "C" int64_t amt_selective_scan_wide_bwd_ws_floats(int32_t B, int32_t L, int32_t ED, int32_t Ns) {
    if (B <= 0 || L <= 0 || ED <= 0 || !(Ns == 32 || Ns == 64 || Ns == 128 || Ns == 256)) return 0;
    return (int64_t)B * cdiv(ED, CPB) * L * (2 * Ns) + (int64_t)B * ED * (Ns + 1) + 2 * (int64_t)(Ns / N) * B * L * ED;
}

extern "C" int32_t amt_selective_scan_wide_bwd(const float* dout, int32_t ld_dout, const float* x, int32_t ldx, const float* delta_raw,
                                               int32_t ld_delta, const float* dt_bias, const float* A_log, const float* Bm, const float* Cm,
                                               int32_t ld_bc, const float* D, const float* z, int32_t ldz, const float* y_pre, int32_t ld_ypre,
                                               const float* h_chunks, float* dx, int32_t lddx, float* ddraw, int32_t ld_ddraw, float* dz,
                                               int32_t lddz, float* dBm, float* dCm, int32_t ld_dbc, float* dA_log, float* dD, float* ws,
                                               int32_t B, int32_t L, int32_t ED, int32_t Ns, int32_t version, int32_t reverse, void* stream) {
    AMT_CHECK_ARG(dout && x && delta_raw && dt_bias && A_log && Bm && Cm && D && z && y_pre && h_chunks, "amt_selective_scan_wide_bwd: null input pointer");
    AMT_CHECK_ARG(dx && ddraw && dz && dBm && dCm && dA_log && dD && ws, "amt_selective_scan_wide_bwd: null output pointer");
    AMT_CHECK_ARG(B > 0 && L > 0 && ED > 0, "amt_selective_scan_wide_bwd: bad shape B=%d L=%d ED=%d", B, L, ED);
    AMT_CHECK_ARG(Ns != N, "amt_selective_scan_wide_bwd: d_state=16 trains through amt_selective_scan_train_fwd / amt_selective_scan_bwd");
    AMT_CHECK_ARG(Ns == 32 || Ns == 64 || Ns == 128 || Ns == 256, "amt_selective_scan_wide_bwd: d_state=%d not in {32, 64, 128, 256}", Ns);
    AMT_CHECK_ARG(version == 0 || version == 1, "amt_selective_scan_wide_bwd: version %d not in {0,1}", version);
    AMT_CHECK_ARG(ld_dout >= ED && ldx >= ED && ld_delta >= ED && ldz >= ED && ld_ypre >= ED && lddx >= ED && ld_ddraw >= ED && lddz >= ED &&
                  ld_bc >= Ns && ld_dbc >= Ns, "amt_selective_scan_wide_bwd: bad leading dimension");
    const int64_t total = (int64_t)B * L * (2 * Ns) + (int64_t)ED * (Ns + 1) + (int64_t)B * L * ED;     // elements of the second launch
    AMT_CHECK_ARG(B <= 65535 && (total + 255) / 256 <= 0x7fffffff, "amt_selective_scan_wide_bwd: B=%d L=%d exceed the launch grid", B, L);
    ScanWideBwdParams pw{};
    ScanBwdParams& p = pw.q;
    pw.N = Ns;
    p.dout = dout; p.lddo = ld_dout; p.x = x; p.ldx = ldx; p.draw = delta_raw; p.ldd = ld_delta; p.dt_bias = dt_bias; p.A_log = A_log;
    p.Bm = Bm; p.Cm = Cm; p.ldbc = ld_bc; p.D = D; p.z = z; p.ldz = ldz; p.ypre = y_pre; p.ldyp = ld_ypre; p.hck = h_chunks;
    p.dx = dx; p.lddx = lddx; p.ddraw = ddraw; p.lddd = ld_ddraw; p.dz = dz; p.lddz = lddz; p.ws = ws;
    p.B = B; p.L = L; p.ED = ED; p.version = version; p.reverse = reverse;
    const int nblk = cdiv(ED, CPB);
    hipLaunchKernelGGL(selective_scan_wide_bwd_kernel, dim3(nblk, B, Ns / N), dim3(NT), 0, (hipStream_t)stream, pw);
    AMT_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_wide_bwd_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pw, dBm, dCm,
                       ld_dbc, dA_log, dD, nblk);
    AMT_LAUNCH_CHECK();
    return 0;
}

extern "C" int32_t amt_silu_bwd(const float* dy, const float* a, float* da, int64_t n, void* stream) {
    AMT_CHECK_ARG(dy && a && da, "amt_silu_bwd: null pointer");
    AMT_CHECK_ARG(n > 0 && (n + 255) / 256 <= 0x7fffffff, "amt_silu_bwd: n=%lld", (long long)n);
    hipLaunchKernelGGL(silu_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, a, da, n);
    AMT_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t amt_dwconv1d_silu_bwd_ws_floats(int32_t B, int32_t L, int32_t C, int32_t K) {
    if (B <= 0 || L <= 0 || C <= 0 || K <= 0) return 0;
    const int64_t rows = (int64_t)B * L;
    return rows * C + (rows + CONV_ROWS - 1) / CONV_ROWS * C * (K + 1);
}

extern "C" int32_t amt_dwconv1d_silu_bwd(const float* dy, int32_t lddy, const float* x, int32_t ldx, const float* w, const float* bias,
                                         float* dx, int32_t lddx, float* dw, float* dbias, float* ws, int32_t B, int32_t L, int32_t C,
                                         int32_t K, int32_t reverse, void* stream) {
    AMT_CHECK_ARG(dy && x && w && dx && dw && ws, "amt_dwconv1d_silu_bwd: null pointer");
    AMT_CHECK_ARG((bias == nullptr) == (dbias == nullptr), "amt_dwconv1d_silu_bwd: bias and dbias go together");
    AMT_CHECK_ARG(B > 0 && L > 0 && C > 0 && K > 0 && ldx >= C && lddy >= C && lddx >= C, "amt_dwconv1d_silu_bwd: bad shape B=%d L=%d C=%d K=%d "
                  "ldx=%d lddy=%d lddx=%d", B, L, C, K, ldx, lddy, lddx);
    AMT_CHECK_ARG(K <= CONV_MAXK, "amt_dwconv1d_silu_bwd: kernel size %d: the backward keeps a channel's taps in registers, at most %d", K, CONV_MAXK);
    const int64_t rows = (int64_t)B * L;
    const int64_t slices = (rows + CONV_ROWS - 1) / CONV_ROWS;
    AMT_CHECK_ARG(slices <= 65535, "amt_dwconv1d_silu_bwd: B*L=%lld rows exceed %d", (long long)rows, 65535 * CONV_ROWS);
    float* dacc = ws;
    float* part = ws + rows * C;
    const size_t total = (size_t)rows * C;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(dwconv_silu_dacc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, dy, lddy, x, ldx, w, bias, dacc, B, L, C, K, reverse);
    AMT_LAUNCH_CHECK();
    hipLaunchKernelGGL(dwconv_silu_bwd_kernel, dim3(cdiv(C, CONV_CH), (unsigned)slices), dim3(256), 0, s, dacc, x, ldx, w, dx, lddx, part, B, L, C, K, reverse);
    AMT_LAUNCH_CHECK();
    hipLaunchKernelGGL(dwconv_silu_bwd_reduce_kernel, dim3(cdiv(C * (K + 1), 256)), dim3(256), 0, s, part, dw, dbias, (int)slices, C, K);
    AMT_LAUNCH_CHECK();
    return 0;
}
