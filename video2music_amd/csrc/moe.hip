// Mixture-of-experts gated FFN (model/moe.py:36-49 GLUExpert, :150-200 MoELayer, :202-302
// SharedMoELayer; eval mode) and MultiheadGQA (model/grouped_query_attention.py:286-358) as
// compositions of the library's kernels.
//
// MoE: instead of the reference's python loop over experts with torch.where gather / scatter
//   router (one wave per token: 8 dot products, top-2, softmax)  ->  plan (sort the 2*n_tok
//   assignments by expert into 128-row aligned segments)  ->  three GROUPED fp32-MFMA GEMMs whose
//   row tiles pick their expert's weights (gate, up * silu(gate), down)  ->  combine (each token
//   sums its two expert rows, lower expert id first, + shared expert / k).
// Every step is deterministic: no float atomics, fixed summation order per token.
#include "../../include/amt_hip.h"
#include "amt_common.h"
#include "kernels.h"

namespace {

constexpr int TILE = 128;

// top-2 routing of one token by one wave: gate logits, the two largest (largest first like torch.topk), softmax over the pair
// (moe.py:190,288).  Every lane returns the same values.
__device__ __forceinline__ void route_token(const float* __restrict__ xrow, const float* __restrict__ gw, const float* __restrict__ gb,
                                            int d, int n_exp, int lane, int& i0, int& i1, float& w0, float& w1) {
    float best0 = -INFINITY, best1 = -INFINITY;
    i0 = 0; i1 = 0;
    // eight experts per pass, their gate rows requested together (unguarded: surplus slots re-read the last expert's row): one expert per
    // loop iteration was one L2 round trip per expert, which is what a one-token launch of the lockstep decode step pays for.  Every
    // expert's sum runs over the chunks in the same order as before (bit-identical logits).
    for (int e0 = 0; e0 < n_exp; e0 += 8) {
        float s[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = 0.f;
        for (int c = lane * 4; c < d; c += 256) {
            const float4 a = ld4(xrow + c);
            float4 w[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = ld4(gw + (size_t)min(e0 + j, n_exp - 1) * d + c);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += a.x * w[j].x + a.y * w[j].y + a.z * w[j].z + a.w * w[j].w;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = e0 + j;
            if (e < n_exp) {
                const float sj = wave_sum(s[j]) + (gb ? gb[e] : 0.f);
                if (sj > best0) { best1 = best0; i1 = i0; best0 = sj; i0 = e; }
                else if (sj > best1) { best1 = sj; i1 = e; }
            }
        }
    }
    const float e1 = __expf(best1 - best0);
    w0 = 1.0f / (1.0f + e1);
    w1 = e1 * w0;
}

__global__ __launch_bounds__(256) void moe_route_kernel(const float* __restrict__ x, const float* __restrict__ gw,
                                                        const float* __restrict__ gb, int n_tok, int d, int n_exp,
                                                        int* __restrict__ idx, float* __restrict__ wts) {
    const int lane = threadIdx.x & 63;
    const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tok >= n_tok) return;
    int i0, i1;
    float w0, w1;
    route_token(x + (size_t)tok * d, gw, gb, d, n_exp, lane, i0, i1, w0, w1);
    if (lane == 0) {
        idx[tok * 2] = i0; idx[tok * 2 + 1] = i1;
        wts[tok * 2] = w0; wts[tok * 2 + 1] = w1;
    }
}

// top-k routing for k other than the class default of 2 (MoELayer(n_experts_per_token=k), moe.py:150-200): the k largest gate logits,
// largest first and the lower expert id first among equals like torch.topk, softmax over those k (fp32, max subtracted)
constexpr int KMAX = 8;
__global__ __launch_bounds__(256) void moe_route_k_kernel(const float* __restrict__ x, const float* __restrict__ gw,
                                                          const float* __restrict__ gb, int n_tok, int d, int n_exp, int k,
                                                          int* __restrict__ idx, float* __restrict__ wts) {
    const int lane = threadIdx.x & 63;
    const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tok >= n_tok) return;
    const float* xrow = x + (size_t)tok * d;
    float bv[KMAX];
    int bi[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) { bv[j] = -INFINITY; bi[j] = 0; }
    for (int e = 0; e < n_exp; ++e) {
        float s = 0.f;
        for (int c = lane * 4; c < d; c += 256) {
            const float4 a = ld4(xrow + c), w = ld4(gw + (size_t)e * d + c);
            s += a.x * w.x + a.y * w.y + a.z * w.z + a.w * w.w;
        }
        s = wave_sum(s) + (gb ? gb[e] : 0.f);
        // insert into the sorted list (strictly greater moves ahead: equal logits keep the lower expert id first)
        float cv = s;
        int ci = e;
        bool ins = false;                           // once inserted, everything below moves down one place
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            if (j < k && (ins || cv > bv[j])) {
                const float tv = bv[j]; const int ti = bi[j];
                bv[j] = cv; bi[j] = ci; cv = tv; ci = ti;
                ins = true;
            }
        }
    }
    float sum = 0.f, ev[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) { ev[j] = j < k ? __expf(bv[j] - bv[0]) : 0.f; sum += ev[j]; }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j < k) { idx[tok * k + j] = bi[j]; wts[tok * k + j] = ev[j] / sum; }
    }
}

// The router of SharedMoELayer(balancing=True) in training mode (moe.py:257-268): the k experts are those with the largest
// logit + sel_bias[e] (largest first, the lower expert id first among equals), and the weights are the softmax over the RAW logits of
// those k, their own maximum subtracted.  The logits are moe_route_k_kernel's sums (route_token's too: the same chunk order); with
// sel_bias all zero the k raw logits arrive sorted and the weights are route_token's expression at k = 2, moe_route_k_kernel's
// otherwise: the bits of the plain routers.
__global__ __launch_bounds__(256) void moe_route_biased_kernel(const float* __restrict__ x, const float* __restrict__ gw,
                                                               const float* __restrict__ gb, const float* __restrict__ sel_bias, int n_tok,
                                                               int d, int n_exp, int k, int* __restrict__ idx, float* __restrict__ wts) {
    const int lane = threadIdx.x & 63;
    const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tok >= n_tok) return;
    const float* xrow = x + (size_t)tok * d;
    float bv[KMAX], rv[KMAX];                       // the selection value and the raw logit of the j-th choice
    int bi[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) { bv[j] = -INFINITY; rv[j] = -INFINITY; bi[j] = 0; }
    for (int e = 0; e < n_exp; ++e) {
        float s = 0.f;
        for (int c = lane * 4; c < d; c += 256) {
            const float4 a = ld4(xrow + c), w = ld4(gw + (size_t)e * d + c);
            s += a.x * w.x + a.y * w.y + a.z * w.z + a.w * w.w;
        }
        s = wave_sum(s) + (gb ? gb[e] : 0.f);
        float cv = s + sel_bias[e], cr = s;
        int ci = e;
        bool ins = false;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            if (j < k && (ins || cv > bv[j])) {
                const float tv = bv[j], tr = rv[j]; const int ti = bi[j];
                bv[j] = cv; rv[j] = cr; bi[j] = ci; cv = tv; cr = tr; ci = ti;
                ins = true;
            }
        }
    }
    float ev[KMAX];
    if (k == 2) {
        const bool first = rv[0] >= rv[1];          // the larger raw logit takes route_token's w0
        const float e1 = __expf(first ? rv[1] - rv[0] : rv[0] - rv[1]);
        const float hi = 1.0f / (1.0f + e1), lo = e1 * hi;
        ev[0] = first ? hi : lo;
        ev[1] = first ? lo : hi;
    } else {
        float mx = rv[0], sum = 0.f;
#pragma unroll
        for (int j = 1; j < KMAX; ++j) if (j < k) mx = fmaxf(mx, rv[j]);
#pragma unroll
        for (int j = 0; j < KMAX; ++j) { ev[j] = j < k ? __expf(rv[j] - mx) : 0.f; sum += ev[j]; }
#pragma unroll
        for (int j = 0; j < KMAX; ++j) ev[j] = ev[j] / sum;
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j < k) { idx[tok * k + j] = bi[j]; wts[tok * k + j] = ev[j]; }
    }
}

// bias_delta[e] = update_rate (mean(c) - c[e]) from the plan's integer counts (moe.py:270-279: c = bincount as fp32, mean = sum / n);
// between moe_count_kernel and moe_offsets_kernel, which zeroes the counts.  One wave.
__global__ __launch_bounds__(64) void moe_bias_delta_kernel(const int* __restrict__ counts, int n_exp, float update_rate,
                                                            float* __restrict__ bias_delta) {
    float sum = 0.f;
    for (int e = 0; e < n_exp; ++e) sum += (float)counts[e];
    const float mean = sum / (float)n_exp;
    const int e = threadIdx.x;
    if (e < n_exp) bias_delta[e] = update_rate * (mean - (float)counts[e]);
}

// combine for k != 2: the token's k expert rows in expert-index order (moe.py:191-199), then shared / k
__global__ void moe_combine_k_kernel(const float* __restrict__ Y, const int* __restrict__ slot_pos, const int* __restrict__ idx,
                                     const float* __restrict__ wts, const float* __restrict__ shared, float shared_scale,
                                     float* __restrict__ out, int d, int k) {
    const int tok = blockIdx.x;
    int ord[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) ord[j] = j;
    for (int a = 1; a < k; ++a)                     // insertion sort of the k slots by expert id (k <= 8, uniform per block)
        for (int b = a; b > 0 && idx[tok * k + ord[b]] < idx[tok * k + ord[b - 1]]; --b) { const int t = ord[b]; ord[b] = ord[b - 1]; ord[b - 1] = t; }
    for (int c = threadIdx.x * 4; c < d; c += blockDim.x * 4) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < k; ++j) {
            const int sl = tok * k + ord[j];
            const float w = wts[sl];
            const float4 y = ld4(Y + (size_t)slot_pos[sl] * d + c);
            o.x += w * y.x; o.y += w * y.y; o.z += w * y.z; o.w += w * y.w;
        }
        if (shared) {
            const float4 sh = ld4(shared + (size_t)tok * d + c);
            o.x += shared_scale * sh.x; o.y += shared_scale * sh.y; o.z += shared_scale * sh.z; o.w += shared_scale * sh.w;
        }
        st4(out + (size_t)tok * d + c, o);
    }
}

// plan, three small launches (counts -> 128-aligned segment offsets -> placement).  Rows of one expert may land in
// any order inside its segment: every output row is computed independently, so the values do not depend on it.
__global__ __launch_bounds__(256) void moe_count_kernel(const int* __restrict__ idx, int n_assign, int* __restrict__ counts) {
    __shared__ int c[64];
    if (threadIdx.x < 64) c[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_assign) atomicAdd(&c[idx[i]], 1);
    __syncthreads();
    if (threadIdx.x < 64 && c[threadIdx.x]) atomicAdd(&counts[threadIdx.x], c[threadIdx.x]);
}

// counts[0..63] in, offsets[0..64] out (segment starts, multiples of TILE), cursors zeroed, perm = -1, tile_group filled
__global__ __launch_bounds__(1024) void moe_offsets_kernel(int* __restrict__ counts, int* __restrict__ offsets, int* __restrict__ cursors,
                                                           int n_exp, int* __restrict__ perm, int* __restrict__ tile_group, int Mp) {
    __shared__ int off[65], cnt[64];
    const int tid = threadIdx.x;
    if (tid < 64) { cnt[tid] = tid < n_exp ? counts[tid] : 0; }
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int e = 0; e < n_exp; ++e) { off[e] = o; o += (cnt[e] + TILE - 1) / TILE * TILE; }
        off[n_exp] = o;
    }
    __syncthreads();
    if (tid <= n_exp) offsets[tid] = off[tid];
    if (tid < 64) { cursors[tid] = 0; counts[tid] = 0; }     // counts are re-zeroed for the next call
    for (int i = tid; i < Mp; i += 1024) perm[i] = -1;
    for (int t = tid; t < Mp / TILE; t += 1024) {
        int g = -1;
        for (int e = 0; e < n_exp; ++e)
            if (t * TILE >= off[e] && t * TILE < off[e] + cnt[e]) g = e;
        tile_group[t] = g;
    }
}

__global__ __launch_bounds__(256) void moe_place_kernel(const int* __restrict__ idx, int n_assign, const int* __restrict__ offsets,
                                                        int* __restrict__ cursors, int* __restrict__ perm, int* __restrict__ slot_pos, int k) {
    __shared__ int c[64], base[64];
    if (threadIdx.x < 64) c[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    int e = -1, local = 0;
    if (i < n_assign) { e = idx[i]; local = atomicAdd(&c[e], 1); }
    __syncthreads();
    if (threadIdx.x < 64 && c[threadIdx.x]) base[threadIdx.x] = atomicAdd(&cursors[threadIdx.x], c[threadIdx.x]);
    __syncthreads();
    if (e >= 0) {
        const int pos = offsets[e] + base[e] + local;
        perm[pos] = i / k;
        slot_pos[i] = pos;
    }
}

// The placement in assignment order, for training: expert e's rows ascend with the assignment index token * k + j, so that a sum over
// a segment's rows (the backward's weight gradients) has one order whatever the scheduling -- moe_place_kernel's order inside a segment
// follows its atomics.  One block per expert walks the assignments 256 at a time (ballot + prefix of the four waves' counts).
__global__ __launch_bounds__(256) void moe_place_stable_kernel(const int* __restrict__ idx, int n_assign, const int* __restrict__ offsets,
                                                               int* __restrict__ perm, int* __restrict__ slot_pos, int k) {
    __shared__ int wsum[4];
    const int e = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = offsets[e];
    for (int i0 = 0; i0 < n_assign; i0 += 256) {             // the trip count is the block's: the barriers are uniform
        const int i = i0 + threadIdx.x;
        const bool mine = i < n_assign && idx[i] == e;
        const unsigned long long b = __ballot(mine);
        const int before = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(b);
        __syncthreads();
        int off = 0, total = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) off += wsum[w];
            total += wsum[w];
        }
        if (mine) {
            const int pos = base + off + before;
            perm[pos] = i / k;
            slot_pos[i] = pos;
        }
        base += total;
        __syncthreads();
    }
}

__global__ void moe_combine_kernel(const float* __restrict__ Y, const int* __restrict__ slot_pos,
                                   const int* __restrict__ idx, const float* __restrict__ wts,
                                   const float* __restrict__ shared, float shared_scale, float* __restrict__ out, int d,
                                   const float* __restrict__ resid = nullptr, int dense_B = 0) {
    const int tok = blockIdx.x;
    int a = 0, b = 1;
    if (idx[tok * 2] > idx[tok * 2 + 1]) { a = 1; b = 0; }        // accumulate in expert-index order (moe.py:191-199)
    const float wa = wts[tok * 2 + a], wb = wts[tok * 2 + b];
    // dense_B > 0: Y is [expert][dense_B tokens][d] (every expert evaluated on every token): the row follows from the expert id
    const float* ya = Y + (size_t)(dense_B > 0 ? idx[tok * 2 + a] * dense_B + tok : slot_pos[tok * 2 + a]) * d;
    const float* yb = Y + (size_t)(dense_B > 0 ? idx[tok * 2 + b] * dense_B + tok : slot_pos[tok * 2 + b]) * d;
    for (int c = threadIdx.x * 4; c < d; c += blockDim.x * 4) {
        const float4 p = ld4(ya + c), q = ld4(yb + c);
        float4 o;
        o.x = wa * p.x + wb * q.x; o.y = wa * p.y + wb * q.y; o.z = wa * p.z + wb * q.z; o.w = wa * p.w + wb * q.w;
        if (shared) {
            const float4 s = ld4(shared + (size_t)tok * d + c);
            o.x += shared_scale * s.x; o.y += shared_scale * s.y; o.z += shared_scale * s.z; o.w += shared_scale * s.w;
        }
        if (resid) {                           // the layer's residual: out = mixture(x) + x (the sum the following norm takes)
            const float4 r = ld4(resid + (size_t)tok * d + c);
            o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
        }
        st4(out + (size_t)tok * d + c, o);
    }
}

// Routing and combine of the lockstep decode step in one launch (every expert was evaluated on every row: Y is
// [expert][n_tok][d]): each block routes its own token (wave 0, same arithmetic as moe_route_kernel), then mixes the two rows in
// expert-index order, adds the shared expert and the layer's residual.
__global__ __launch_bounds__(128) void moe_route_combine_kernel(const float* __restrict__ x, const float* __restrict__ gw, const float* __restrict__ gb,
                                                                int n_exp, const float* __restrict__ Y, const float* __restrict__ shared,
                                                                float shared_scale, const float* __restrict__ resid, float* __restrict__ out,
                                                                int n_tok, int d) {
    __shared__ int s_i[2];
    __shared__ float s_w[2];
    const int tok = blockIdx.x;
    if (threadIdx.x < 64) {
        int i0, i1;
        float w0, w1;
        route_token(x + (size_t)tok * d, gw, gb, d, n_exp, threadIdx.x, i0, i1, w0, w1);
        if (threadIdx.x == 0) {
            const bool sw = i0 > i1;                         // accumulate in expert-index order (moe.py:191-199)
            s_i[0] = sw ? i1 : i0; s_i[1] = sw ? i0 : i1;
            s_w[0] = sw ? w1 : w0; s_w[1] = sw ? w0 : w1;
        }
    }
    __syncthreads();
    const float wa = s_w[0], wb = s_w[1];
    const float* ya = Y + ((size_t)s_i[0] * n_tok + tok) * d;
    const float* yb = Y + ((size_t)s_i[1] * n_tok + tok) * d;
    for (int c = threadIdx.x * 4; c < d; c += blockDim.x * 4) {
        const float4 p = ld4(ya + c), q = ld4(yb + c);
        float4 o;
        o.x = wa * p.x + wb * q.x; o.y = wa * p.y + wb * q.y; o.z = wa * p.z + wb * q.z; o.w = wa * p.w + wb * q.w;
        if (shared) {
            const float4 sh = ld4(shared + (size_t)tok * d + c);
            o.x += shared_scale * sh.x; o.y += shared_scale * sh.y; o.z += shared_scale * sh.z; o.w += shared_scale * sh.w;
        }
        if (resid) {
            const float4 r = ld4(resid + (size_t)tok * d + c);
            o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
        }
        st4(out + (size_t)tok * d + c, o);
    }
}

inline size_t align4(size_t n) { return (n + 3) / 4 * 4; }


// ---- expert-parallel execution: plans built on the device ----
// Dispatch side: exact (un-padded) segment starts per expert, so that the rows of one destination rank are contiguous in the
// send buffer and the buffer is what all_to_all_single takes.  counts[0..63] in; offsets[0..64], counts_out[0..n_exp) out;
// cursors zeroed, counts re-zeroed for the next call.
__global__ __launch_bounds__(64) void moe_ep_offsets_kernel(int* __restrict__ counts, int* __restrict__ offsets, int* __restrict__ cursors,
                                                            int* __restrict__ counts_out, int n_exp) {
    __shared__ int cnt[64];
    const int tid = threadIdx.x;
    cnt[tid] = tid < n_exp ? counts[tid] : 0;
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int e = 0; e < n_exp; ++e) { offsets[e] = o; o += cnt[e]; }
        offsets[n_exp] = o;
    }
    if (tid < n_exp) counts_out[tid] = cnt[tid];
    cursors[tid] = 0;
    counts[tid] = 0;
}

// dst[i] = src[index[i]]  (index < 0: a row of zeros); one wave per row, float4 lanes
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ src, const int* __restrict__ index, float* __restrict__ dst,
                                                          int n_rows, int d) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows) return;
    const int from = index[row];
    for (int c = lane * 4; c < d; c += 256) {
        const float4 v = from >= 0 ? ld4(src + (size_t)from * d + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        st4(dst + (size_t)row * d + c, v);
    }
}

// Expert side: the received rows arrive grouped by (source rank, local expert): segment (s, j) has recv_counts[s * e_local + j]
// rows.  The grouped GEMMs want the rows of one local expert in one TILE-aligned run: perm[slot] = arrival row (or -1 in the
// padding), slot_of[arrival row] = slot, tile_group[tile] = local expert (or -1).  One workgroup (world * e_local <= 64 segments).
__global__ __launch_bounds__(1024) void moe_ep_expert_plan_kernel(const int* __restrict__ recv_counts, int world, int e_local, int n_recv, int Mp,
                                                                  int* __restrict__ perm, int* __restrict__ slot_of, int* __restrict__ tile_group) {
    __shared__ int seg_src[64], seg_dst[64], seg_n[64], off[65], cnt[64];
    const int tid = threadIdx.x, nseg = world * e_local;
    if (tid == 0) {
        for (int j = 0; j < e_local; ++j) { cnt[j] = 0; for (int s2 = 0; s2 < world; ++s2) cnt[j] += recv_counts[s2 * e_local + j]; }
        int o = 0;
        for (int j = 0; j < e_local; ++j) { off[j] = o; o += (cnt[j] + TILE - 1) / TILE * TILE; }
        off[e_local] = o;
        int src = 0;
        for (int s2 = 0; s2 < world; ++s2)
            for (int j = 0; j < e_local; ++j) {
                const int n = recv_counts[s2 * e_local + j];
                int before = 0;
                for (int s3 = 0; s3 < s2; ++s3) before += recv_counts[s3 * e_local + j];
                seg_src[s2 * e_local + j] = src; seg_dst[s2 * e_local + j] = off[j] + before; seg_n[s2 * e_local + j] = n;
                src += n;
            }
    }
    __syncthreads();
    for (int i = tid; i < Mp; i += 1024) perm[i] = -1;
    for (int t = tid; t < Mp / TILE; t += 1024) {
        int g = -1;
        for (int j = 0; j < e_local; ++j)
            if (t * TILE >= off[j] && t * TILE < off[j] + cnt[j]) g = j;
        tile_group[t] = g;
    }
    __syncthreads();
    for (int sg = 0; sg < nseg; ++sg)
        for (int i = tid; i < seg_n[sg]; i += 1024) {
            const int r = seg_src[sg] + i, slot = seg_dst[sg] + i;
            if (r < n_recv) { perm[slot] = r; slot_of[r] = slot; }
        }
}

}  // namespace

extern "C" int64_t amt_moe_topk_scratch_floats(int32_t n_tok, int32_t d, int32_t dff, int32_t n_exp, int32_t k) {
    const size_t Mp = ((size_t)k * n_tok + TILE - 1) / TILE * TILE + (size_t)TILE * n_exp;
    // G, H : Mp x dff ; Y : Mp x d ; shared G,H : n_tok x dff ; shared Y : n_tok x d ; ints: perm, slot_pos, tile_group
    return (int64_t)(2 * Mp * dff + Mp * d + 2 * (size_t)n_tok * dff + (size_t)n_tok * d +
                     align4(Mp) + 3 * align4(k * (size_t)n_tok) + align4(Mp / TILE + 1) + 256 + 64);
}
extern "C" int64_t amt_moe_scratch_floats(int32_t n_tok, int32_t d, int32_t dff, int32_t n_exp) {
    return amt_moe_topk_scratch_floats(n_tok, d, dff, n_exp, 2);
}

static int32_t moe_fwd_impl(const float* x, const float* gate_w, const float* gate_b,
                            const float* w1, const float* b1, const float* wg, const float* bg, const float* w2, const float* b2,
                            const float* sw1, const float* sb1, const float* swg, const float* sbg, const float* sw2, const float* sb2,
                            float* out, int32_t* idx_out, float* w_out, float* scratch,
                            int32_t n_tok, int32_t d, int32_t dff, int32_t n_exp, int32_t k, void* stream) {
    AMT_CHECK_ARG(x && gate_w && wg && w2 && out && scratch, "amt_moe_fwd: null pointer");
    AMT_CHECK_ARG(n_tok > 0 && n_exp >= 2 && n_exp <= 64, "amt_moe_fwd: need 2 <= n_experts <= 64");
    AMT_CHECK_ARG(k >= 1 && k <= KMAX && k <= n_exp, "amt_moe_fwd: n_experts_per_token=%d outside 1..min(%d, n_experts)", k, KMAX);
    AMT_CHECK_ARG(d % 32 == 0 && dff % 32 == 0, "amt_moe_fwd: d and d_ff must be multiples of 32");
    hipStream_t s = (hipStream_t)stream;
    const int Mp = (k * n_tok + TILE - 1) / TILE * TILE + TILE * n_exp;     // multiple of the row tile
    float* G = scratch;
    float* Hh = G + (size_t)Mp * dff;
    float* Y = Hh + (size_t)Mp * dff;
    float* Gs = Y + (size_t)Mp * d;
    float* Hs = Gs + (size_t)n_tok * dff;
    float* Ys = Hs + (size_t)n_tok * dff;
    int* perm = (int*)(Ys + (size_t)n_tok * d);
    int* slot_pos = perm + align4(Mp);
    int* tile_group = slot_pos + align4(k * (size_t)n_tok);
    int* idx = tile_group + align4(Mp / TILE + 1);
    float* wts = (float*)(idx + align4(k * (size_t)n_tok));
    int* plan_ints = (int*)(wts + align4(k * (size_t)n_tok));     // [0..63] counts, [64..128] offsets, [192..255] cursors
    if (idx_out) idx = idx_out;
    if (w_out) wts = w_out;
    AMT_HIP(hipMemsetAsync(plan_ints, 0, 64 * sizeof(int), s));

    if (k == 2) hipLaunchKernelGGL(moe_route_kernel, dim3(cdiv(n_tok, 4)), dim3(256), 0, s, x, gate_w, gate_b, n_tok, d, n_exp, idx, wts);
    else hipLaunchKernelGGL(moe_route_k_kernel, dim3(cdiv(n_tok, 4)), dim3(256), 0, s, x, gate_w, gate_b, n_tok, d, n_exp, k, idx, wts);
    AMT_LAUNCH_CHECK();
    hipLaunchKernelGGL(moe_count_kernel, dim3(cdiv(k * n_tok, 256)), dim3(256), 0, s, idx, k * n_tok, plan_ints);
    hipLaunchKernelGGL(moe_offsets_kernel, dim3(1), dim3(1024), 0, s, plan_ints, plan_ints + 64, plan_ints + 192, n_exp, perm, tile_group, Mp);
    hipLaunchKernelGGL(moe_place_kernel, dim3(cdiv(k * n_tok, 256)), dim3(256), 0, s, idx, k * n_tok, plan_ints + 64, plan_ints + 192, perm, slot_pos, k);
    AMT_LAUNCH_CHECK();
    int32_t rc;
    // gate branch: G = x_e . Wg[e]^T + bg[e]
    // (w1 == null: the experts are Linear -> SiLU -> Linear, video_music_transformer.py:80-85: H = silu(G), one launch)
    GemmParams g = gemm_params(x, d, wg, d, w1 ? G : Hh, dff, Mp, dff, d, bg);
    g.a_gather = perm; g.tile_group = tile_group; g.w_group_stride = (size_t)dff * d; g.bias_group_stride = dff;
    g.relu = w1 ? 0 : 2;
    if ((rc = amt_launch_gemm(g, s))) return rc;
    if (w1) {
        // up branch fused with the gate: H = (x_e . W1[e]^T + b1[e]) * silu(G)
        GemmParams u = gemm_params(x, d, w1, d, Hh, dff, Mp, dff, d, b1);
        u.a_gather = perm; u.tile_group = tile_group; u.w_group_stride = (size_t)dff * d; u.bias_group_stride = dff;
        u.silu_mul = G; u.ld_silu = dff;
        if ((rc = amt_launch_gemm(u, s))) return rc;
    }
    // down: Y = H . W2[e]^T + b2[e]
    GemmParams dn = gemm_params(Hh, dff, w2, dff, Y, d, Mp, d, dff, b2);
    dn.tile_group = tile_group; dn.w_group_stride = (size_t)d * dff; dn.bias_group_stride = d;
    if ((rc = amt_launch_gemm(dn, s))) return rc;
    const float* shared = nullptr;
    if (swg) {
        AMT_CHECK_ARG(sw2 && (sw1 != nullptr) == (w1 != nullptr), "amt_moe_fwd: incomplete shared expert");
        GemmParams a = gemm_params(x, d, swg, d, sw1 ? Gs : Hs, dff, n_tok, dff, d, sbg);
        a.relu = sw1 ? 0 : 2;
        if ((rc = amt_launch_gemm(a, s))) return rc;
        if (sw1) {
            GemmParams b = gemm_params(x, d, sw1, d, Hs, dff, n_tok, dff, d, sb1);
            b.silu_mul = Gs; b.ld_silu = dff;
            if ((rc = amt_launch_gemm(b, s))) return rc;
        }
        GemmParams c = gemm_params(Hs, dff, sw2, dff, Ys, d, n_tok, d, dff, sb2);
        if ((rc = amt_launch_gemm(c, s))) return rc;
        shared = Ys;
    }
    if (k == 2) hipLaunchKernelGGL(moe_combine_kernel, dim3(n_tok), dim3(128), 0, s, Y, slot_pos, idx, wts, shared, 0.5f, out, d);
    else hipLaunchKernelGGL(moe_combine_k_kernel, dim3(n_tok), dim3(128), 0, s, Y, slot_pos, idx, wts, shared, 1.0f / (float)k, out, d, k);
    AMT_LAUNCH_CHECK();
    return 0;
}

extern "C" int32_t amt_moe_fwd(const float* x, const float* gate_w, const float* gate_b,
                               const float* w1, const float* b1, const float* wg, const float* bg, const float* w2, const float* b2,
                               const float* sw1, const float* sb1, const float* swg, const float* sbg, const float* sw2, const float* sb2,
                               float* out, int32_t* idx_out, float* w_out, float* scratch,
                               int32_t n_tok, int32_t d, int32_t dff, int32_t n_exp, void* stream) {
    return moe_fwd_impl(x, gate_w, gate_b, w1, b1, wg, bg, w2, b2, sw1, sb1, swg, sbg, sw2, sb2, out, idx_out, w_out, scratch, n_tok, d, dff, n_exp, 2, stream);
}
// the same layer with n_experts_per_token = k (1 <= k <= 8): idx_out / w_out are (n_tok, k); scratch from amt_moe_topk_scratch_floats
extern "C" int32_t amt_moe_topk_fwd(const float* x, const float* gate_w, const float* gate_b,
                                    const float* w1, const float* b1, const float* wg, const float* bg, const float* w2, const float* b2,
                                    const float* sw1, const float* sb1, const float* swg, const float* sbg, const float* sw2, const float* sb2,
                                    float* out, int32_t* idx_out, float* w_out, float* scratch,
                                    int32_t n_tok, int32_t d, int32_t dff, int32_t n_exp, int32_t k, void* stream) {
    return moe_fwd_impl(x, gate_w, gate_b, w1, b1, wg, bg, w2, b2, sw1, sb1, swg, sbg, sw2, sb2, out, idx_out, w_out, scratch, n_tok, d, dff, n_exp, k, stream);
}

// ---- pieces of the MoE layer for expert-parallel execution (video2music_amd/model/moe.py: route on every rank,
//      exchange rows with all_to_all, run the local experts, exchange back, combine) ----
extern "C" int32_t amt_moe_route_fwd(const float* x, const float* gate_w, const float* gate_b, int32_t* idx_out, float* w_out,
                                     int32_t n_tok, int32_t d, int32_t n_exp, void* stream) {
    AMT_CHECK_ARG(x && gate_w && idx_out && w_out, "amt_moe_route_fwd: null pointer");
    AMT_CHECK_ARG(n_tok > 0 && n_exp >= 2 && n_exp <= 64 && d % 4 == 0, "amt_moe_route_fwd: bad shape");
    hipLaunchKernelGGL(moe_route_kernel, dim3(cdiv(n_tok, 4)), dim3(256), 0, (hipStream_t)stream, x, gate_w, gate_b, n_tok, d, n_exp, idx_out, w_out);
    AMT_LAUNCH_CHECK();
    return 0;
}

extern "C" int32_t amt_glu_expert_fwd(const float* x, const float* w1, const float* b1, const float* wg, const float* bg,
                                      const float* w2, const float* b2, float* out, float* scratch,
                                      int32_t n, int32_t d, int32_t dff, void* stream) {
    AMT_CHECK_ARG(x && wg && w2 && out && scratch, "amt_glu_expert_fwd: null pointer");
    AMT_CHECK_ARG(n > 0 && d % 32 == 0 && dff % 32 == 0, "amt_glu_expert_fwd: bad shape");
    hipStream_t s = (hipStream_t)stream;
    float* G = scratch;                     // [n][dff] gate branch
    float* Hh = G + (size_t)n * dff;        // [n][dff] (x W1^T + b1) * silu(G)
    int32_t rc;
    GemmParams g = gemm_params(x, d, wg, d, w1 ? G : Hh, dff, n, dff, d, bg);
    g.relu = w1 ? 0 : 2;                    // w1 == null: Linear -> SiLU -> Linear expert, H = silu(x Wg^T + bg)
    if ((rc = amt_launch_gemm(g, s))) return rc;
    if (w1) {
        GemmParams u = gemm_params(x, d, w1, d, Hh, dff, n, dff, d, b1);
        u.silu_mul = G; u.ld_silu = dff;
        if ((rc = amt_launch_gemm(u, s))) return rc;
    }
    return amt_launch_gemm(gemm_params(Hh, dff, w2, dff, out, d, n, d, dff, b2), s);
}

int32_t amt_launch_moe_combine(const float* y_rows, const int32_t* slot_pos, const int32_t* idx, const float* wts, const float* shared,
                               float shared_scale, const float* resid, float* out, int n_tok, int d, hipStream_t stream, int dense_B) {
    hipLaunchKernelGGL(moe_combine_kernel, dim3(n_tok), dim3(128), 0, stream, y_rows, slot_pos, idx, wts, shared, shared_scale, out, d, resid, dense_B);
    AMT_LAUNCH_CHECK();
    return 0;
}

int32_t amt_launch_moe_route_combine(const float* x, const float* gate_w, const float* gate_b, int n_exp, const float* y_all, const float* shared,
                                     float shared_scale, const float* resid, float* out, int n_tok, int d, hipStream_t stream) {
    AMT_CHECK_ARG(n_tok > 0 && n_exp >= 2 && n_exp <= 64 && d % 4 == 0, "moe_route_combine: bad shape");
    hipLaunchKernelGGL(moe_route_combine_kernel, dim3(n_tok), dim3(128), 0, stream, x, gate_w, gate_b, n_exp, y_all, shared, shared_scale, resid, out,
                       n_tok, d);
    AMT_LAUNCH_CHECK();
    return 0;
}

// ---- the layer's first and last launches for the training forward (moe_bwd.hip): moe_fwd_impl's kernels in its order, but for the
//      placement, which is the stable one (every output row is computed independently: the forward's values do not depend on it) ----
// router + plan: idx / wts (n_tok, k), perm (Mp), slot_pos (n_tok k), tile_group (Mp / 128), plan_ints (256: [64..128] keeps the segment offsets)
// sel_bias (n_exp) given: the balancing router (moe_route_biased_kernel), and bias_delta (n_exp) from the plan's counts
int32_t amt_launch_moe_route_plan(const float* x, const float* gate_w, const float* gate_b, int32_t* idx, float* wts, int32_t* plan_ints,
                                  int32_t* perm, int32_t* slot_pos, int32_t* tile_group, int n_tok, int d, int n_exp, int k, int Mp,
                                  hipStream_t s, const float* sel_bias, float update_rate, float* bias_delta) {
    AMT_HIP(hipMemsetAsync(plan_ints, 0, 64 * sizeof(int), s));
    if (sel_bias) hipLaunchKernelGGL(moe_route_biased_kernel, dim3(cdiv(n_tok, 4)), dim3(256), 0, s, x, gate_w, gate_b, sel_bias, n_tok, d, n_exp, k, idx, wts);
    else if (k == 2) hipLaunchKernelGGL(moe_route_kernel, dim3(cdiv(n_tok, 4)), dim3(256), 0, s, x, gate_w, gate_b, n_tok, d, n_exp, idx, wts);
    else hipLaunchKernelGGL(moe_route_k_kernel, dim3(cdiv(n_tok, 4)), dim3(256), 0, s, x, gate_w, gate_b, n_tok, d, n_exp, k, idx, wts);
    AMT_LAUNCH_CHECK();
    hipLaunchKernelGGL(moe_count_kernel, dim3(cdiv(k * n_tok, 256)), dim3(256), 0, s, idx, k * n_tok, plan_ints);
    if (bias_delta) hipLaunchKernelGGL(moe_bias_delta_kernel, dim3(1), dim3(64), 0, s, plan_ints, n_exp, update_rate, bias_delta);
    hipLaunchKernelGGL(moe_offsets_kernel, dim3(1), dim3(1024), 0, s, plan_ints, plan_ints + 64, plan_ints + 192, n_exp, perm, tile_group, Mp);
    hipLaunchKernelGGL(moe_place_stable_kernel, dim3(n_exp), dim3(256), 0, s, idx, k * n_tok, plan_ints + 64, perm, slot_pos, k);
    AMT_LAUNCH_CHECK();
    return 0;
}

int32_t amt_launch_moe_combine_k(const float* y_rows, const int32_t* slot_pos, const int32_t* idx, const float* wts, const float* shared,
                                 float* out, int n_tok, int d, int k, hipStream_t s) {
    if (k == 2) hipLaunchKernelGGL(moe_combine_kernel, dim3(n_tok), dim3(128), 0, s, y_rows, slot_pos, idx, wts, shared, 0.5f, out, d);
    else hipLaunchKernelGGL(moe_combine_k_kernel, dim3(n_tok), dim3(128), 0, s, y_rows, slot_pos, idx, wts, shared, 1.0f / (float)k, out, d, k);
    AMT_LAUNCH_CHECK();
    return 0;
}

extern "C" int32_t amt_moe_combine_fwd(const float* y_rows, const int32_t* slot_pos, const int32_t* idx, const float* wts,
                                       const float* shared, float shared_scale, float* out, int32_t n_tok, int32_t d, void* stream) {
    AMT_CHECK_ARG(y_rows && slot_pos && idx && wts && out && n_tok > 0 && d % 4 == 0, "amt_moe_combine_fwd: bad argument");
    hipLaunchKernelGGL(moe_combine_kernel, dim3(n_tok), dim3(128), 0, (hipStream_t)stream, y_rows, slot_pos, idx, wts, shared, shared_scale, out, d);
    AMT_LAUNCH_CHECK();
    return 0;
}

// ---- expert-parallel pieces, device side (the host only learns the split sizes) ----
// Dispatch plan of one rank's routed (token, slot) assignments idx[2 * n_tok]: counts_out[n_exp] rows per expert, perm[2 * n_tok]
// (send-buffer row -> token) and slot_pos[2 * n_tok] (assignment -> send-buffer row); the send buffer is ordered by expert, exact
// packing.  ints: >= 256 words of scratch, zero before the first call (the plan leaves them zero again).
extern "C" int32_t amt_moe_ep_dispatch_plan_fwd(const int32_t* idx, int32_t n_tok, int32_t n_exp, int32_t* counts_out, int32_t* perm,
                                                int32_t* slot_pos, int32_t* ints, void* stream) {
    AMT_CHECK_ARG(idx && counts_out && perm && slot_pos && ints && n_tok > 0 && n_exp >= 2 && n_exp <= 64, "amt_moe_ep_dispatch_plan_fwd: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int n_assign = 2 * n_tok;
    hipLaunchKernelGGL(moe_count_kernel, dim3(cdiv(n_assign, 256)), dim3(256), 0, s, idx, n_assign, ints);
    hipLaunchKernelGGL(moe_ep_offsets_kernel, dim3(1), dim3(64), 0, s, ints, ints + 64, ints + 192, counts_out, n_exp);
    hipLaunchKernelGGL(moe_place_kernel, dim3(cdiv(n_assign, 256)), dim3(256), 0, s, idx, n_assign, ints + 64, ints + 192, perm, slot_pos, 2);
    AMT_LAUNCH_CHECK();
    return 0;
}

extern "C" int32_t amt_gather_rows_fwd(const float* src, const int32_t* index, float* dst, int32_t n_rows, int32_t d, void* stream) {
    AMT_CHECK_ARG(src && index && dst && n_rows >= 0 && d % 4 == 0, "amt_gather_rows_fwd: bad argument");
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(cdiv(n_rows, 4)), dim3(256), 0, (hipStream_t)stream, src, index, dst, n_rows, d);
    AMT_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t amt_moe_ep_expert_scratch_floats(int32_t n_recv, int32_t d, int32_t dff, int32_t e_local) {
    const size_t Mp = ((size_t)n_recv + TILE - 1) / TILE * TILE + (size_t)TILE * e_local;
    return (int64_t)(2 * Mp * dff + Mp * d + align4(Mp) + align4((size_t)n_recv + 1) + align4(Mp / TILE + 1) + 64);
}

// The local experts of one rank on the rows it received: rows [n_recv][d] grouped by (source rank, local expert) as the
// all_to_all delivers them, recv_counts (DEVICE, [world][e_local]) the segment sizes; w1 .. b2 the stacked tensors of the rank's
// e_local experts (as amt_moe_fwd takes them; w1 null: Linear -> SiLU -> Linear experts).  y_out [n_recv][d] in ARRIVAL order
// (what the return all_to_all sends back).  One grouped launch per projection (moe.py:36-49 per expert).
extern "C" int32_t amt_moe_ep_expert_fwd(const float* rows, const int32_t* recv_counts, int32_t world, int32_t e_local, int32_t n_recv,
                                         const float* w1, const float* b1, const float* wg, const float* bg, const float* w2, const float* b2,
                                         float* y_out, float* scratch, int32_t d, int32_t dff, void* stream) {
    AMT_CHECK_ARG(rows && recv_counts && wg && w2 && y_out && scratch, "amt_moe_ep_expert_fwd: null pointer");
    AMT_CHECK_ARG(world >= 1 && e_local >= 1 && world * e_local <= 64 && n_recv >= 0 && d % 32 == 0 && dff % 32 == 0, "amt_moe_ep_expert_fwd: bad shape");
    if (n_recv == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int Mp = (n_recv + TILE - 1) / TILE * TILE + TILE * e_local;
    float* G = scratch;
    float* Hh = G + (size_t)Mp * dff;
    float* Y = Hh + (size_t)Mp * dff;
    int* perm = (int*)(Y + (size_t)Mp * d);
    int* slot_of = perm + align4(Mp);
    int* tile_group = slot_of + align4((size_t)n_recv + 1);
    hipLaunchKernelGGL(moe_ep_expert_plan_kernel, dim3(1), dim3(1024), 0, s, recv_counts, world, e_local, n_recv, Mp, perm, slot_of, tile_group);
    AMT_LAUNCH_CHECK();
    int32_t rc;
    GemmParams g = gemm_params(rows, d, wg, d, w1 ? G : Hh, dff, Mp, dff, d, bg);
    g.a_gather = perm; g.tile_group = tile_group; g.w_group_stride = (size_t)dff * d; g.bias_group_stride = dff;
    g.relu = w1 ? 0 : 2;
    if ((rc = amt_launch_gemm(g, s))) return rc;
    if (w1) {
        GemmParams u = gemm_params(rows, d, w1, d, Hh, dff, Mp, dff, d, b1);
        u.a_gather = perm; u.tile_group = tile_group; u.w_group_stride = (size_t)dff * d; u.bias_group_stride = dff;
        u.silu_mul = G; u.ld_silu = dff;
        if ((rc = amt_launch_gemm(u, s))) return rc;
    }
    GemmParams dn = gemm_params(Hh, dff, w2, dff, Y, d, Mp, d, dff, b2);
    dn.tile_group = tile_group; dn.w_group_stride = (size_t)d * dff; dn.bias_group_stride = d;
    if ((rc = amt_launch_gemm(dn, s))) return rc;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(cdiv(n_recv, 4)), dim3(256), 0, s, Y, slot_of, y_out, n_recv, d);
    AMT_LAUNCH_CHECK();
    return 0;
}

static int32_t gqa_impl(const float* query, const float* key, const float* value,
                        const float* wq, const float* bq, const float* wk, const float* bk, const float* wv, const float* bv,
                        const float* ln_w, const float* ln_b, const float* wo, const float* bo,
                        float* out, float* scratch, int32_t L, int32_t S, int32_t B, int32_t E, int32_t query_heads,
                        int32_t kv_heads, int32_t is_causal, float ln_eps, const float* rope_cache, int32_t cache_half, void* stream) {
    AMT_CHECK_ARG(query && key && value && wq && wk && wv && wo && out && scratch, "amt_gqa_fwd: null pointer");
    AMT_CHECK_ARG(query_heads > 0 && kv_heads > 0 && query_heads % kv_heads == 0 && E % query_heads == 0, "amt_gqa_fwd: bad head counts");
    hipStream_t s = (hipStream_t)stream;
    const int hd = E / query_heads, Ekv = hd * kv_heads;
    float* q = scratch;                         // [L*B][E]
    float* k = q + (size_t)L * B * E;           // [S*B][Ekv]
    float* v = k + (size_t)S * B * Ekv;
    float* a = v + (size_t)S * B * Ekv;         // [L*B][E] attention output, then LayerNorm in place
    int32_t rc;
    GemmParams gq = gemm_params(query, E, wq, E, q, E, L * B, E, E, bq);
    gq.scale = 1.0f / sqrtf((float)hd); gq.scale_cols = E;       // query / sqrt(hd), grouped_query_attention.py:121-123
    if ((rc = amt_launch_gemm(gq, s))) return rc;
    if ((rc = amt_launch_gemm(gemm_params(key, E, wk, E, k, Ekv, S * B, Ekv, E, bk), s))) return rc;
    if ((rc = amt_launch_gemm(gemm_params(value, E, wv, E, v, Ekv, S * B, Ekv, E, bv), s))) return rc;
    if (rope_cache) {
        // RoPE on the raw (heads, len, B, hd) view of the projection buffers (:316-322), in place.  The reference rotates before
        // it divides the query by sqrt(hd) (:121-123); the rotation is linear, so the scaled query rotates to the same values up
        // to fp32 rounding
        if ((rc = amt_launch_rope(q, rope_cache, q, query_heads, L, B, hd, cache_half, s))) return rc;
        if ((rc = amt_launch_rope(k, rope_cache, k, kv_heads, S, B, hd, cache_half, s))) return rc;
    }
    // the reference reinterprets the (L,B,.) projection buffers in memory order as (B,L,.) (:316-326):
    // batch-first strides on the same memory; the output is written transposed back as (L',B',E) (:159)
    AttnParams p{};
    p.q = q; p.k = k; p.v = v; p.o = a;
    p.q_bs = (size_t)L * E; p.q_ls = E; p.q_hs = hd;
    p.k_bs = p.v_bs = (size_t)S * Ekv; p.k_ls = p.v_ls = Ekv; p.k_hs = p.v_hs = hd;
    p.o_bs = E; p.o_ls = (size_t)B * E; p.o_hs = hd;
    p.B = B; p.H = query_heads; p.Lq = L; p.Lk = S; p.hd = hd; p.causal = is_causal; p.kv_group = query_heads / kv_heads;
    if ((rc = amt_launch_attn_prefill(p, s))) return rc;
    const float* proj_in = a;
    if (ln_w) {
        if ((rc = amt_launch_layernorm(a, nullptr, ln_w, ln_b, nullptr, nullptr, a, L * B, E, ln_eps, s))) return rc;
    }
    return amt_launch_gemm(gemm_params(proj_in, E, wo, E, out, E, L * B, E, E, bo), s);
}

extern "C" int32_t amt_gqa_fwd(const float* query, const float* key, const float* value,
                               const float* wq, const float* bq, const float* wk, const float* bk, const float* wv, const float* bv,
                               const float* ln_w, const float* ln_b, const float* wo, const float* bo,
                               float* out, float* scratch, int32_t L, int32_t S, int32_t B, int32_t E, int32_t query_heads,
                               int32_t kv_heads, int32_t is_causal, float ln_eps, void* stream) {
    return gqa_impl(query, key, value, wq, bq, wk, bk, wv, bv, ln_w, ln_b, wo, bo, out, scratch, L, S, B, E, query_heads, kv_heads, is_causal,
                    ln_eps, nullptr, 0, stream);
}

extern "C" int32_t amt_gqa_rope_fwd(const float* query, const float* key, const float* value,
                                    const float* wq, const float* bq, const float* wk, const float* bk, const float* wv, const float* bv,
                                    const float* ln_w, const float* ln_b, const float* wo, const float* bo,
                                    float* out, float* scratch, int32_t L, int32_t S, int32_t B, int32_t E, int32_t query_heads,
                                    int32_t kv_heads, int32_t is_causal, float ln_eps, const float* rope_cache, int32_t cache_rows,
                                    int32_t cache_half, void* stream) {
    AMT_CHECK_ARG(rope_cache && cache_half > 0 && cache_rows >= L && cache_rows >= S, "amt_gqa_rope_fwd: the rope cache has %d rows, the sequences %d / %d",
                  cache_rows, L, S);
    return gqa_impl(query, key, value, wq, bq, wk, bk, wv, bv, ln_w, ln_b, wo, bo, out, scratch, L, S, B, E, query_heads, kv_heads, is_causal,
                    ln_eps, rope_cache, cache_half, stream);
}
