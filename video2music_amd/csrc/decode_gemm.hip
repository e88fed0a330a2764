// Skinny GEMM for one autoregressive decode step:  y[B<=32, N] = epi( LN(x)[B, K] . W[N, K]^T )
//
// At B = 32 clips the projections of a decode step are weight-streaming GEMVs: every weight byte
// is used for 32 rows only, so the kernel is shaped around reading W exactly once, coalesced, and
// around the launch count of the step (the LayerNorm that precedes each projection in the
// post-norm decoder, model/rpr.py:59-69, is folded into the prologue; bias / residual / ReLU /
// q-scaling / KV-cache scatter into the epilogue).
//
//  * weights are pre-packed once at load time into 16(n) x 16(k) tiles laid out in MFMA operand
//    order, so one wave-instruction (64 lanes x 16 B) fetches a whole 1 KiB tile contiguously and
//    feeds 4 v_mfma_f32_16x16x4_f32 per 16-row block without any shuffle;
//  * one 1024-thread workgroup per 16 output columns x 16 rows; its 16 waves split K, all their tile loads are
//    issued up front (nothing depends on the LayerNorm prologue), partial tiles are summed in a
//    fixed order through LDS (deterministic, no atomics);
//  * the (normalised) input rows are staged once in LDS ([16][K+8] floats: conflict-free
//    ds_read_b128 A-fragments).
#include <limits.h>
#include <stdlib.h>

#include <atomic>
#include <mutex>

#include "amt_common.h"
#include "kernels.h"

namespace {

constexpr int MAXB = 4096;       // rows per launch (16 per workgroup, blockIdx.y); the decode step uses 32
constexpr int XPAD = 8;

// (ldw: row stride of W in floats -- a column range [k0, k0 + K) of a wider matrix is packed as W + k0 with ldw = its full width)
__global__ void pack_weight_kernel(const float* __restrict__ W, float* __restrict__ P, int N, int K, int ldw) {
    const int kt_n = K / 16;
    const size_t tile = blockIdx.x;                 // nt*kt_n + kt
    const int nt = (int)(tile / kt_n), kt = (int)(tile % kt_n);
    const int lane = threadIdx.x;
    const int n = nt * 16 + (lane & 15), k = kt * 16 + 4 * (lane >> 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n < N) v = ld4(W + (size_t)n * ldw + k);
    st4(P + (tile * 64 + lane) * 4, v);
}

constexpr int NW = 16;           // waves per workgroup: K is split 16 ways, one staged row per wave
constexpr int MT = 16;           // rows per workgroup (one MFMA row block); blockIdx.y selects the block

__device__ __forceinline__ float sum4(const float4 a) { return (a.x + a.y) + (a.z + a.w); }
// (the mean is splat into a full register pair: the packed subtract then has no half it does not define, which
// otherwise picks up a false dependency on whatever load targets the neighbouring register)
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float sq4(const float4 a, float m) {
    const f32x2 mm = {m, m};
    f32x2 lo = {a.x, a.y}, hi = {a.z, a.w};
    lo -= mm; hi -= mm;
    lo *= lo; hi *= hi;
    return (lo.x + lo.y) + (hi.x + hi.y);
}

// What the kernel does to its input rows before the product (launch_variant maps DecodeGemmParams onto it)
enum class Pro {
    Plain,       // rows as they are
    LayerNorm,   // LayerNorm prologue
    FoldedFfn,   // folded-FFN prologue: [ relu((raw - mu*g)*rstd + c) | LayerNorm(u) ]
    Glu,         // gated-linear-unit prologue: x * silu(gate)
    LayerNorm2,  // two LayerNorms in a row (norm3 of the last layer, then decoder.norm)
    FoldedGlu,   // folded gated FFN prologue (FoldedFfn with a gate: up * silu(gate) in place of the ReLU)
};
constexpr bool pro_layernorm(Pro p) { return p == Pro::LayerNorm || p == Pro::LayerNorm2; }
constexpr bool pro_folded(Pro p) { return p == Pro::FoldedFfn || p == Pro::FoldedGlu; }      // per-column vectors handed over through LDS
constexpr bool pro_gated(Pro p) { return p == Pro::Glu || p == Pro::FoldedGlu; }

// KCH = float4 chunks per lane and row (K <= KCH*256) = weight tiles per wave; FULL: K == KCH*256, no lane predicates.
// First column of chunk c in this lane, and the same clamped into the row (out-of-range lanes re-read the last float4 and discard it)
__device__ __forceinline__ int chunk_col(int c, int lane) { return (c * 64 + lane) * 4; }
template <bool FULL>
__device__ __forceinline__ int chunk_col(int c, int lane, int K) { const int i = chunk_col(c, lane); return FULL ? i : min(i, K - 4); }

__device__ __forceinline__ float silu(float x) { return x / (1.0f + __expf(-x)); }
// the LayerNorm of one float4: (v - mean) * rstd * gamma + beta
__device__ __forceinline__ float4 ln4(const float4 v, float mean, float rstd, const float4 g, const float4 h) {
    return make_float4((v.x - mean) * rstd * g.x + h.x, (v.y - mean) * rstd * g.y + h.y, (v.z - mean) * rstd * g.z + h.z, (v.w - mean) * rstd * g.w + h.w);
}
// the gated-linear-unit prologue of one float4: u * silu(g) (um = 1, uo = 0), or silu(g) alone (um = 0, uo = 1)
__device__ __forceinline__ float4 glu4(const float4 v, const float4 g, float um, float uo) {
    return make_float4((v.x * um + uo) * silu(g.x), (v.y * um + uo) * silu(g.y), (v.z * um + uo) * silu(g.z), (v.w * um + uo) * silu(g.w));
}

// Two-pass statistics over n columns of the row a wave holds in v.  MUL: w(c) is a 0/1 float weight per chunk and multiplies the
// chunk's sums (the folded prologues: branch-free); otherwise w(c) is a predicate and guards them (LayerNorm: compile-time true when
// the row is full).  It takes n, not 1/n, and divides behind the first sum: a reciprocal formed by the caller is scheduled in front of
// the sums and moves a wait of the folded-FFN prologue (profiles/r06_decode_gemm_refactor_codegen.txt).
struct RowStats { float mean, rstd; };
// C0: the first chunk the wave holds (rows staged by LDS-DMA keep only the u half in registers: the chunks in front of it have w(c) = 0)
template <bool MUL, int C0 = 0, int KCH, typename F>
__device__ __forceinline__ RowStats row_stats(const float4 (&v)[KCH], F w, float n, float eps) {
    float s = 0.f;
#pragma unroll
    for (int c = C0; c < KCH; ++c) {
        if constexpr (MUL) s += w(c) * sum4(v[c]);
        else if (w(c)) s += sum4(v[c]);
    }
    const float inv_n = 1.0f / n;
    const float mean = wave_sum(s) * inv_n;
    float q = 0.f;
#pragma unroll
    for (int c = C0; c < KCH; ++c) {
        if constexpr (MUL) q += w(c) * sq4(v[c], mean);
        else if (w(c)) q += sq4(v[c], mean);
    }
    return {mean, rsqrtf(wave_sum(q) * inv_n + eps)};
}

// the LayerNorm vectors' chunks of this lane
template <int KCH, bool FULL>
__device__ __forceinline__ void load_ln(float4 (&g)[KCH], float4 (&h)[KCH], const float* w, const float* b, int lane, int K) {
#pragma unroll
    for (int c = 0; c < KCH; ++c) {
        const int ic = chunk_col<FULL>(c, lane, K);
        g[c] = ld4(w + ic);
        h[c] = ld4(b + ic);
    }
}

// the four MFMAs of one 16 x 16 weight tile: one accumulator chain, .x .y .z .w
__device__ __forceinline__ f32x4 mfma_tile(const float4 a, const float4 w, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w.w, acc, 0, 0, 0);
    return acc;
}
// a wave's partial tile into its [4 r][64 lanes] slot, and the fixed-order sum of the 16 waves' partials for output e
__device__ __forceinline__ void store_partials(float* rw, const f32x4 acc, int lane) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) rw[rr * 64 + lane] = acc[rr];
}
__device__ __forceinline__ float sum_partials(const float* red, int e) {
    float val = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) val += red[w * 256 + e];
    return val;
}

// epilogue of a paired gate | up tile (DecodeGemmParams::glu_pair): lanes 0-7 of a 16-lane row hold the gate columns, lanes 8-15 the up
// columns of the same 8 hidden columns; every lane gets up * silu(gate), the up lanes store it
__device__ __forceinline__ float glu_pair_value(float val, int c) {
    const float other = __shfl_xor(val, 8, 64);
    const float g = c < 8 ? val : other, u = c < 8 ? other : val;
    return u * silu(g);
}
__device__ __forceinline__ float act(float v, int relu) { return relu == 1 ? fmaxf(v, 0.f) : relu == 2 ? silu(v) : v; }
// column of the stacked bias that belongs to interleaved column n (N = stacked width)
__device__ __forceinline__ int glu_pair_bias_col(int n, int N) { const int c = n & 15; return (c < 8 ? 0 : N / 2 - 8) + (n >> 4) * 8 + c; }

// Everything the kernel reads from global memory is issued up front in ONE branch-free sequence: rows, prologue
// vectors, weight tiles, epilogue operands (out-of-range lanes read a clamped address and discard the value).
// Vector loads return in issue order and the compiler can only count them across straight-line code: with the
// rows first and no branch in between, the prologue waits for the (L2-resident) rows alone while the weight tiles
// (Infinity Cache / HBM) are still in flight.  A conditional load anywhere in that sequence degrades every later
// wait to vmcnt(0), i.e. serialises the prologue behind the weights.
#ifdef AMT_STAMPS
#define STAMP(i) do { __builtin_amdgcn_sched_barrier(0); st_[i] = __builtin_amdgcn_s_memrealtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define STAMP(i) do { } while (0)
#endif

// The folded-FFN fix of one A fragment (Pro::FoldedFfn).  It is VALU-bound (16 x 1536 elements per workgroup, every workgroup of the
// launch redoes them: with (a - mu*g)*rstd + c spelled as mul / sub / mul / add / max the fix cost 0.75 us of a 7.5 us launch), so each
// half is two fused multiply-adds per element with nm = -mu*rstd per row,
//   raw half        relu(a*rstd + (c - mu*rstd*g))        LayerNorm half   (a*rstd - mu*rstd)*gamma + beta
// The two spellings are bit-identical.  PACKED issues packed pairs (v_pk_fma_f32): the serial loop's form, and the pipelined loop's
// under AMT_FIXUP_PACKED; the pipelined loop's default is scalar fmaf: beside MFMAs a packed f32 op costs more than the two plain ones
// it replaces.
// SIDE 0: raw half, 1: LayerNorm half, 2: `raw` (wave-uniform) chooses per tile -- both forms are computed and one is selected, so the
// one wave whose tile range straddles K1 stays branch-free too.
#ifdef AMT_FIXUP_PACKED
constexpr bool FIXUP_PACKED = true;
#else
constexpr bool FIXUP_PACKED = false;
#endif
template <int SIDE, bool PACKED = FIXUP_PACKED>
__device__ __forceinline__ float4 ffn_fix(const float4 a, const float4 g, const float4 h, float rs, float nm, bool raw) {
    float4 r = a, l = a;
    if constexpr (PACKED) {
        const f32x2 a_lo = {a.x, a.y}, a_hi = {a.z, a.w}, g_lo = {g.x, g.y}, g_hi = {g.z, g.w}, h_lo = {h.x, h.y}, h_hi = {h.z, h.w};
        const f32x2 rs2 = {rs, rs}, nm2 = {nm, nm};
        if (SIDE != 1) {
            const f32x2 t_lo = __builtin_elementwise_fma(a_lo, rs2, __builtin_elementwise_fma(nm2, g_lo, h_lo));
            const f32x2 t_hi = __builtin_elementwise_fma(a_hi, rs2, __builtin_elementwise_fma(nm2, g_hi, h_hi));
            r = make_float4(fmaxf(t_lo.x, 0.f), fmaxf(t_lo.y, 0.f), fmaxf(t_hi.x, 0.f), fmaxf(t_hi.y, 0.f));
        }
        if (SIDE != 0) {
            const f32x2 t_lo = __builtin_elementwise_fma(__builtin_elementwise_fma(a_lo, rs2, nm2), g_lo, h_lo);
            const f32x2 t_hi = __builtin_elementwise_fma(__builtin_elementwise_fma(a_hi, rs2, nm2), g_hi, h_hi);
            l = make_float4(t_lo.x, t_lo.y, t_hi.x, t_hi.y);
        }
    } else {
        if (SIDE != 1) {
            r.x = fmaxf(fmaf(a.x, rs, fmaf(nm, g.x, h.x)), 0.f); r.y = fmaxf(fmaf(a.y, rs, fmaf(nm, g.y, h.y)), 0.f);
            r.z = fmaxf(fmaf(a.z, rs, fmaf(nm, g.z, h.z)), 0.f); r.w = fmaxf(fmaf(a.w, rs, fmaf(nm, g.w, h.w)), 0.f);
        }
        if (SIDE != 0) {
            l.x = fmaf(fmaf(a.x, rs, nm), g.x, h.x); l.y = fmaf(fmaf(a.y, rs, nm), g.y, h.y);
            l.z = fmaf(fmaf(a.z, rs, nm), g.z, h.z); l.w = fmaf(fmaf(a.w, rs, nm), g.w, h.w);
        }
    }
    if (SIDE == 0) return r;
    if (SIDE == 1) return l;
    return raw ? r : l;
}

// ---- the tile loop of decode_gemm_kernel<.., PIPE = true> ----
// A wave that owns all KCH tiles walks them in ONE basic block, one tile ahead: tile i+1's ds_read_b128 (A fragment; FoldedFfn: g and h
// too) are requested before tile i's four MFMAs and its fix is finished in their shadow, in a second register set.  The group barriers pin
// that interleave (the scheduler otherwise sinks each read to its use).  One accumulator chain, tiles and .x .y .z .w in the serial order.
template <int KCH, Pro PRO, int SIDE>
__device__ __forceinline__ f32x4 tiles_pipelined(const float* xa, const float* fg, int K, const float4 (&wt)[KCH], float rs, float nm, int k0, int K1) {
    constexpr bool FIX = PRO == Pro::FoldedFfn;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float4 a[2], g[2], h[2];
    a[0] = ld4(xa);
    if (FIX) {
        g[0] = ld4(fg); h[0] = ld4(fg + K);
        a[0] = ffn_fix<SIDE>(a[0], g[0], h[0], rs, nm, k0 < K1);
    }
    __builtin_amdgcn_sched_barrier(0);               // (the groups below must not pick tile 0's reads and fix)
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
        const int c = i & 1, n = c ^ 1;
        if (i + 1 < KCH) {
            a[n] = ld4(xa + (i + 1) * 16);
            if (FIX) { g[n] = ld4(fg + (i + 1) * 16); h[n] = ld4(fg + K + (i + 1) * 16); }
        }
        acc = mfma_tile(a[c], wt[i], acc);
        if (FIX && i + 1 < KCH) a[n] = ffn_fix<SIDE>(a[n], g[n], h[n], rs, nm, k0 + (i + 1) * 16 < K1);
        if (i + 1 < KCH) {
            __builtin_amdgcn_sched_group_barrier(0x100, FIX ? 3 : 1, 0);           // next tile's LDS reads
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                      // MFMA .x .y
            if (FIX) __builtin_amdgcn_sched_group_barrier(0x002, SIDE == 2 ? 12 : 6, 0);      // first half of the next fix
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                      // MFMA .z
            if (FIX) __builtin_amdgcn_sched_group_barrier(0x002, SIDE == 2 ? 12 : 6, 0);      // second half
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                      // MFMA .w
        }
    }
    return acc;
}

// A wave that owns 0 < nown < KCH tiles: one scalar branch per tile, the next tile's reads still one ahead.  (The read-ahead behind the
// last owned tile touches at most 16 floats past its row / vector: inside the LDS allocation -- the partial-tile region follows --
// and never used.)
template <int KCH, Pro PRO, int SIDE>
__device__ __forceinline__ f32x4 tiles_partial(const float* xa, const float* fg, int K, const float4 (&wt)[KCH], float rs, float nm, int k0, int K1, int nown) {
    constexpr bool FIX = PRO == Pro::FoldedFfn;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float4 a_n = ld4(xa), g_n = a_n, h_n = a_n;
    if (FIX) { g_n = ld4(fg); h_n = ld4(fg + K); }
#pragma unroll
    for (int i = 0; i < KCH - 1; ++i) {
        if (i < nown) {
            float4 a0 = a_n;
            const float4 g = g_n, h = h_n;
            a_n = ld4(xa + (i + 1) * 16);
            if (FIX) { g_n = ld4(fg + (i + 1) * 16); h_n = ld4(fg + K + (i + 1) * 16); }
            if (FIX) a0 = ffn_fix<SIDE>(a0, g, h, rs, nm, k0 + i * 16 < K1);
            acc = mfma_tile(a0, wt[i], acc);
        }
    }
    return acc;
}

// a float4 at a wave-uniform base plus the lane's byte offset: `global_load_dwordx4 v, v_off, s[base:base+1]`, no per-lane 64-bit address
// (the global address space spelled out: a base that went through an opaque asm is otherwise loaded from as a flat address)
__device__ __forceinline__ float4 ld4_s(const char* sbase, unsigned lane_off) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) char* gptr;
    const f4 t = *(const __attribute__((address_space(1))) f4*)((gptr)sbase + lane_off);
    return make_float4(t.x, t.y, t.z, t.w);
}

// ... and through a buffer descriptor: a wave-uniform byte offset in an SGPR, the lane's in a VGPR (as attn_decode.hip's key stream)
using wbuf_t = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ float4 ld4_buf(wbuf_t r, unsigned voff, unsigned soff) {
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 t = __builtin_bit_cast(f4, (u4)__builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
    return make_float4(t.x, t.y, t.z, t.w);
}

// s_waitcnt's gfx9 immediate for vmcnt(n) alone: vmcnt in bits 3:0 (and 15:14), expcnt 6:4 and lgkmcnt 11:8 left at their maxima
constexpr int vmcnt_imm(int n) { return (n & 15) | ((n >> 4) << 14) | 0x0f70; }
// A counted wait that the compiler's own wait bookkeeping follows (an asm statement's it does not see).  The s_nop takes the wait:
// into a wait that stands directly in front of an instruction the compiler folds whatever that instruction needs by its own count,
// and while a global_load_lds is in flight (a pending flat access to it) that is vmcnt(0) for any loaded register.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    __builtin_amdgcn_s_waitcnt(vmcnt_imm(N));
    asm volatile("s_nop 0");
}
// ... and straight into LDS (gfx950 LDS-DMA, `global_load_lds_dwordx4 v_off, s[base:base+1] offset:OFF`): lane l's 16 bytes land at
// lds + OFF + 16 l, one contiguous KiB per wave-instruction, no VGPR in between.  `lds` is wave-uniform (it travels in M0); OFF is
// the instruction's immediate and moves source and destination alike.  The load counts on vmcnt like a register load, in issue
// order with them; nothing but the issuing wave's own wait (and then a barrier, for the other waves) orders a ds_read behind it.
template <int OFF>
__device__ __forceinline__ void dma16_s(const char* sbase, unsigned lane_off, float* lds) {
    typedef const __attribute__((address_space(1))) char* gptr;
    __builtin_amdgcn_global_load_lds((gptr)sbase + lane_off, (__attribute__((address_space(3))) void*)lds, 16, OFF, 0);
}
// chunks C .. N-1 of a row by LDS-DMA: chunk c from (256 c < K1 ? xr : x2r) + 1024 c to row + 256 c (floats).  As in the register
// front, chunks 0-3 ride in the immediate; from the fourth on 4 KiB go into the scalar base and into the LDS base
template <int C, int N>
__device__ __forceinline__ void dma_row_chunks(const char* xr, const char* x2r, int K1, unsigned lane_off, float* row) {
    if constexpr (C < N) {
        const char* side = (256 * C < K1 ? xr : x2r) + (C >= 4 ? 4096 : 0);
        if (C >= 4) asm volatile("" : "+s"(side));
        dma16_s<1024 * (C & 3)>(side, lane_off, row + (C >= 4 ? 1024 : 0));
        dma_row_chunks<C + 1, N>(xr, x2r, K1, lane_off, row);
    }
}

// PIPE: the tile loop with wave-uniform control and one tile of read-ahead; false keeps the serial loop
// (DecodeGemmParams::serial_loop: A/B and the bit-identity tests)
// LEAN: the scalar address front (amt_decode_gemm_lean_ok: two-source rows of whole 256-column chunks, packed weights, none of the
// options below).  Between kernel entry and the last load request everything wave-uniform is SALU work on kernel arguments that
// arrive in one round of scalar loads (DecodeGemmFront): the row, the side of K1 a chunk lies on, the column tile's weight base and
// the clamped tile indices are scalars, a load is a scalar base plus ONE lane offset (lane * 16 bytes).  What is loaded, and
// everything behind the loads, is the generic kernel's.
// DMA (lean front only; amt_decode_gemm_rows_dma_ok): the row chunks that nothing is done to on their way go from memory into the
// staged row by LDS-DMA instead of through registers and a ds_write_b128 each.  Plain: all KCH chunks, the wave holds no row register
// at all.  FoldedFfn: the raw columns below K1 (the launcher admits K1 = 2 (K - K1): the first 2/3 of the chunks); the u half stays
// in registers for the statistics, is requested first and written by the wave itself.  The wave waits for its own DMA loads with a
// counted vmcnt -- the weight tiles behind them stay in flight -- and the one staging barrier follows that wait.  What is staged, and
// every arithmetic instruction, is the register path's.
template <int KCH, bool FULL, Pro PRO, bool PIPE, bool LEAN = false, bool DMA = false>
__global__ __launch_bounds__(NW * 64) void decode_gemm_kernel(DecodeGemmParams p) {
    static_assert(!LEAN || (PIPE && FULL && (PRO == Pro::Plain || PRO == Pro::FoldedFfn)), "the lean front serves the folded chain's launches");
    static_assert(!DMA || (LEAN && (PRO == Pro::Plain || KCH % 3 == 0)), "LDS-DMA rows: the lean front, a u half of KCH / 3 chunks");
    constexpr int DCH = !DMA ? 0 : PRO == Pro::Plain ? KCH : KCH - KCH / 3;      // row chunks 0 .. DCH-1 go by LDS-DMA, the others through v[]
    extern __shared__ __attribute__((aligned(16))) float smem[];
#ifdef AMT_STAMPS
    unsigned long long st_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long st_land = 0, st_lds = 0;     // this wave's row: landed (registers, or LDS by DMA) and complete in LDS
#endif
    STAMP(0);
    constexpr bool FFN = pro_folded(PRO), LN1 = pro_layernorm(PRO);
    const int tid = threadIdx.x, lane = tid & 63;
    const int nt = blockIdx.x, m0 = blockIdx.y * MT;
    float* xs = smem;                               // [16][LD]
    // what the two fronts hand to the rest of the kernel
    int K, LD, wave, nts, K1, kt_n, tpw, kt0, zg, grp;
    bool high;
    float* red;
    float4 v[KCH], wt[KCH];
    // FoldedGlu: at least one 256-column chunk belongs to the u half (two at K = 1536, where the launcher asks for K - K1 >= 512: one
    // float4 more per lane would spill at the 128-VGPR budget of a 16-wave workgroup)
    constexpr int GCH = PRO == Pro::FoldedGlu ? (KCH == 6 ? 4 : KCH > 1 ? KCH - 1 : 1) : KCH;
    float4 gv[pro_gated(PRO) ? GCH : 1];
    float4 g0[LN1 ? KCH : 1], h0[LN1 ? KCH : 1], g1[PRO == Pro::LayerNorm2 ? KCH : 1], h1[PRO == Pro::LayerNorm2 ? KCH : 1];
    float4 gs_val = make_float4(0.f, 0.f, 0.f, 0.f), gs2_val = make_float4(0.f, 0.f, 0.f, 0.f);
    int gs_vec = 0, gs_i = 0, gs2_vec = 0, gs2_i = 0;
    if constexpr (LEAN) {
        const DecodeGemmFront& f = p.front;
        const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
        const unsigned loff = (unsigned)lane * 16u;
        wave = wv; zg = 0; grp = 0;
        K = f.K; LD = f.LD; K1 = f.K1; nts = f.nts;
        red = smem + f.red_off;
        high = nt >= nts;
        kt_n = high ? f.ktn_hi : f.ktn_lo; tpw = high ? f.tpw_hi : f.tpw_lo;
        kt0 = wv * tpw;
        // ---- 1. the row this wave stages (32-bit byte offsets: checked by the launcher) ----
        const unsigned rc = (unsigned)min(m0 + wv, f.B - 1);
        const char* xr = reinterpret_cast<const char*>(f.x) + rc * f.x_row_bytes;
        const char* x2r = reinterpret_cast<const char*>(f.x2b) + rc * f.x2_row_bytes;
#pragma unroll
        for (int c = DCH; c < KCH; ++c) {
            // chunks 0-3 ride in the instruction's immediate offset; from the fourth on 4 KiB go into the base on the scalar unit (opaque:
            // the compiler otherwise adds them to the lane's 64-bit address)
            const char* side = (256 * c < K1 ? xr : x2r) + (c >= 4 ? 4096 : 0);
            if (c >= 4) asm volatile("" : "+s"(side));
            v[c] = ld4_s(side + 1024 * (c & 3), loff);
        }
        if constexpr (DMA) {
            // (the u half's register loads in front: its statistics start while the DMA chunks land)
            if (DCH < KCH) asm volatile("" ::: "memory");
            dma_row_chunks<0, DCH>(xr, x2r, K1, loff, xs + wv * LD);
        }
        // rows first: the prologue's wait counts the loads behind them.  (A compiler barrier for memory operations, not a scheduling
        // boundary: behind sched_barrier(0) the epilogue's kernel arguments are requested and waited for between the rows and the weights.)
        asm volatile("" ::: "memory");
        // ---- 2. folded FFN: wave w of the first K / 128 takes 256 columns of one of the two vectors (the others repeat the last of them) ----
        if (FFN) {
            const int gw = min(wv, (K >> 7) - 1), vec = gw >= (K >> 8) ? 1 : 0, col0 = (gw - vec * (K >> 8)) * 256;
            const float* a = col0 < K1 ? (vec ? f.fold_c : f.fold_g) : (vec ? f.ln_bb : f.ln_wb);
            gs_vec = vec; gs_i = col0 + lane * 4;
            gs_val = ld4_s(reinterpret_cast<const char*>(a + col0), loff);
            asm volatile("" ::: "memory");
        }
        // ---- 3. this wave's weight tiles (tile index clamped on the scalar unit) ----
        // through a buffer descriptor on the column tile's k-tiles (`buffer_load_dwordx4 v, v_off, s[rsrc], s_off offen`): the tile part of
        // the address is the scalar offset.  (As a pointer sum the compiler adds the lane offset first and each tile's 64-bit address on the VALU.)
        const float* wb = (high ? f.Wp2 : f.Wp) + (size_t)((unsigned)((high ? nt - nts : nt) * kt_n) * 1024u) / 4;
        const wbuf_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wb), 0, kt_n * 1024, 0x00020000);
#pragma unroll
        for (int i = 0; i < KCH; ++i) wt[i] = ld4_buf(wr, loff, (unsigned)min(kt0 + i, kt_n - 1) * 1024u);
    } else {
    wave = tid >> 6;
    K = p.K; LD = K + XPAD;
    // [16 waves][4 r][64 lanes] partial tiles in a region of their own (behind the staged rows and the folded-FFN vectors): a wave stores its
    // partials as soon as its MFMAs are done, with no barrier in between (sharing the rows' region cost one: +0.6 % tokens/s without it)
    red = smem + MT * LD + (PRO == Pro::FoldedFfn ? 2 * K + 2 * MT : PRO == Pro::FoldedGlu ? 2 * K + 2 * p.K1 : 0);
    // column split: tiles below n_split multiply the first K1 input columns by Wp, the others all K by Wp2
    nts = p.n_split >> 4;
    high = p.n_split > 0 && nt >= nts;
    K1 = p.x2 ? p.K1 : K;                           // first column taken from x2
    const int Kw = (p.n_split > 0 && !high) ? p.K1 : K;
    kt_n = Kw / 16; tpw = (kt_n + NW - 1) / NW;
    kt0 = wave * tpw;

    // ---- 1. the row this wave stages: row m0+wave (clamped to the last valid row) ----
    zg = p.n_groups > 1 ? (int)blockIdx.z : 0;      // grouped launch: one expert per blockIdx.z
    const int r = m0 + wave, rc = min(r, p.B - 1);
    const float* xr = p.x + (size_t)zg * p.x_group_off + (size_t)rc * p.ldx;
    const float* x2r = p.x2 ? p.x2 + (size_t)rc * p.ldx2 - K1 : xr;
#pragma unroll
    for (int c = 0; c < KCH; ++c) {
        const int ic = chunk_col<FULL>(c, lane, K);
        v[c] = ld4((ic < K1 ? xr : x2r) + ic);
    }
    if (PRO == Pro::Glu) {
        const float* gr = p.glu_gate + (size_t)zg * p.x_group_off + (size_t)rc * p.ldx;
#pragma unroll
        for (int c = 0; c < KCH; ++c) gv[c] = ld4(gr + min(chunk_col<FULL>(c, lane, K), K1 - 4));      // (two-source rows: the chunks past K1 are not gated and re-read the last gate chunk)
    }
    if (PRO == Pro::FoldedGlu) {                      // raw gate columns of the first K1 staged columns (chunks past K1 re-read the last one)
        const float* gr = p.glu_gate + (size_t)rc * p.ldx;
#pragma unroll
        for (int c = 0; c < GCH; ++c) gv[c] = ld4(gr + min(chunk_col(c, lane), K1 - 4));
    }
    // ---- 2. prologue vectors ----
    if constexpr (LN1) load_ln<KCH, FULL>(g0, h0, p.ln_w, p.ln_b, lane, K);
    if constexpr (PRO == Pro::LayerNorm2) load_ln<KCH, FULL>(g1, h1, p.ln2_w, p.ln2_b, lane, K);
    // folded FFN: the per-column vectors (same for all 16 rows) go through LDS, one float4 per thread (K/2 <= 1024)
    const int gs_t = min(tid, K / 2 - 1);
    gs_vec = gs_t >= K / 4; gs_i = (gs_t - gs_vec * (K / 4)) * 4;
    if (FFN) {
        const float* a = gs_i < K1 ? p.fold_g + gs_i : p.ln_w + (gs_i - K1);
        const float* b = gs_i < K1 ? p.fold_c + gs_i : p.ln_b + (gs_i - K1);
        gs_val = ld4(gs_vec ? b : a);
    }
    // folded gated FFN: the gate's two vectors [g2 (K1) | c2 (K1)], one more float4 for the first K1/2 threads (clamped)
    const int gs2_t = min(tid, K1 / 2 - 1);
    gs2_vec = gs2_t >= K1 / 4; gs2_i = (gs2_t - gs2_vec * (K1 / 4)) * 4;
    if (PRO == Pro::FoldedGlu) gs2_val = ld4((gs2_vec ? p.fold_c2 : p.fold_g2) + gs2_i);
    // ---- 3. this wave's weight tiles (tile index clamped: surplus loads repeat the last tile) ----
    grp = p.sel ? *p.sel : zg;                      // device-chosen weight group (mixture-of-experts, one token) or the launch's group
    const float* wbase = high ? p.Wp2 + (size_t)(nt - nts) * kt_n * 256 : p.Wp + (size_t)grp * p.sel_w_stride + (size_t)nt * kt_n * 256;
    // un-packed weights (ldw > 0): lane (n = lane & 15, k-quad = lane >> 4) reads its float4 of row n directly: 16 rows x 64 B
    // per tile instead of one 1 KiB run, still one fully used 64-B segment per row
    const float* wrow = p.Wp + (size_t)min(nt * 16 + (lane & 15), p.N - 1) * p.ldw + 4 * (lane >> 4);
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
        const int kt = min(kt0 + i, kt_n - 1);
        wt[i] = ld4(p.ldw ? wrow + (size_t)kt * 16 : wbase + ((size_t)kt * 64 + lane) * 4);
    }
    }
    int n_u = K - K1;                               // width of the u half (the folded prologues' statistics)
    __builtin_amdgcn_sched_barrier(0);              // the scheduler must not sink any of these loads below this point
    if constexpr (LEAN) {
        // ... and nothing that reads a row may rise above it (with every operand of the statistics in SGPRs early, instruction selection
        // otherwise places them, and their wait, between the row loads and the weight loads)
        // (DMA: a global_load_lds in flight counts as a pending flat access, in front of which the compiler waits vmcnt(0) for any
        // loaded register -- the weight tiles included.  So the waits up to the one that retires the DMA loads are spelled out, through
        // the builtin, which its bookkeeping follows: here for the u half, the loads behind it still in flight.)
        if constexpr (DMA && DCH < KCH) {
            wait_vmcnt<DCH + 1 + KCH>();
            __builtin_amdgcn_sched_barrier(0);      // (not a register copy in front of the wait either)
        }
#pragma unroll
        for (int c = DCH; c < KCH; ++c) asm volatile("" : "+v"(v[c].x), "+v"(v[c].y), "+v"(v[c].z), "+v"(v[c].w));
        asm volatile("" : "+s"(n_u));               // (the division by the u half's width as well)
    }
    STAMP(1);
    const int el = tid & 63, er = (tid >> 6) & 3;
    const int row = m0 + 4 * (el >> 4) + er, n = nt * 16 + (el & 15);
    const bool live = tid < 256 && row < p.B && n < p.N;
    // ---- prologue math ----
    const auto in_row = [&](int c) { return FULL || chunk_col(c, lane) < K; };
    // the folded prologues take their statistics from the u half (columns K1..K-1): 1 there, 0 elsewhere (a multiply keeps the sums branch-free)
    const auto u_half = [&](int c) { return (chunk_col(c, lane) >= K1 && in_row(c)) ? 1.f : 0.f; };
    if (PRO == Pro::FoldedFfn) {
        // folded FFN, [ relu((raw - mu*g)*rstd + c) | LayerNorm(u) ] with the statistics of the u half: the rows are
        // staged RAW, the wave leaves its row's (mu, rstd) and the per-column vectors in LDS, and the fix is applied to the A fragments
        // when they are read for the MFMAs -- under the shadow of the weight tiles still in flight, every element exactly once (a wave
        // owns its k range), and with ONE barrier instead of two (1.56 us of a 6.5 us launch were this prologue)
        float* gs = smem + MT * LD;                 // [2][K]: g|gamma , c|beta ; then [16][2]: mu, rstd per staged row
        const RowStats st = row_stats<true, DCH>(v, u_half, (float)n_u, p.eps);
        if constexpr (DMA) {
            // the vector's float4 and, in front of it, this wave's DMA chunks; the KCH weight tiles stay in flight
            asm volatile("" ::: "memory");
            wait_vmcnt<KCH>();
            asm volatile("" ::: "memory");
#ifdef AMT_STAMPS
            __builtin_amdgcn_sched_barrier(0); st_[6] = __builtin_amdgcn_s_memrealtime(); __builtin_amdgcn_sched_barrier(0);      // (kept for st_land below; STAMP 6 overwrites it)
#endif
        }
        gs[2 * K + 2 * wave + (lane & 1)] = (lane & 1) ? st.rstd : st.mean;      // (every lane stores one of the two words: no branch)
        st4(gs + gs_vec * K + gs_i, gs_val);        // unconditional (surplus threads repeat the last float4): a guarded
                                                    // store lets the compiler sink the load behind the weight loads
    } else if (PRO == Pro::FoldedGlu) {
        // [ up * silu(gate) | LayerNorm(u) ], both halves of the gated unit finished with the statistics of the u half
        float* gs = smem + MT * LD;                 // [2][K]: g|gamma , c|beta , then [2][K1]: the gate's g2 , c2
        st4(gs + gs_vec * K + gs_i, gs_val);
        st4(gs + 2 * K + gs2_vec * K1 + gs2_i, gs2_val);
        const RowStats st = row_stats<true>(v, u_half, (float)n_u, p.eps);
        const float mean = st.mean, rstd = st.rstd;
        __syncthreads();
        // one half of the gated unit, folded: (raw - mu*g)*rstd + c
        const auto fold = [&](float a, float g, float h) { return (a - mean * g) * rstd + h; };
#pragma unroll
        for (int c = 0; c < KCH; ++c) {
            const int ic = chunk_col<FULL>(c, lane, K);
            const float4 g = ld4(gs + ic), h = ld4(gs + K + ic);
            // K1 is a multiple of 256 (checked by the launcher): a 256-column chunk lies on one side of it and the side is wave-uniform
            if (256 * c + 256 <= K1) {               // gated half: up * silu(gate)
                if (c < GCH) {
                    const float4 g2 = ld4(gs + 2 * K + ic), h2 = ld4(gs + 2 * K + K1 + ic);
                    const float ux = fold(v[c].x, g.x, h.x), uy = fold(v[c].y, g.y, h.y), uz = fold(v[c].z, g.z, h.z), uw = fold(v[c].w, g.w, h.w);
                    const float tx = fold(gv[c].x, g2.x, h2.x), ty = fold(gv[c].y, g2.y, h2.y), tz = fold(gv[c].z, g2.z, h2.z), tw = fold(gv[c].w, g2.w, h2.w);
                    v[c] = make_float4(ux * silu(tx), uy * silu(ty), uz * silu(tz), uw * silu(tw));
                }
            } else {                                 // LayerNorm half: (u - mu)*rstd*gamma + beta
                v[c] = ln4(v[c], mean, rstd, g, h);
            }
        }
    } else if (LN1) {
#pragma unroll
        for (int pass = 0; pass < (PRO == Pro::LayerNorm2 ? 2 : 1); ++pass) {
            const RowStats st = row_stats<false>(v, in_row, (float)K, p.eps);
            const bool second = PRO == Pro::LayerNorm2 && pass == 1;
#pragma unroll
            for (int c = 0; c < KCH; ++c) v[c] = ln4(v[c], st.mean, st.rstd, second ? g1[c] : g0[c], second ? h1[c] : h0[c]);
        }
    }
    if (PRO == Pro::Glu) {
        const float um = p.glu_only ? 0.f : 1.f, uo = p.glu_only ? 1.f : 0.f;      // h = u * silu(g), or silu(g) alone
#pragma unroll
        for (int c = 0; c < KCH; ++c) {
            // two-source rows [x * silu(gate) (K1 columns) | x2]: whole 256-column chunks on either side (checked by the launcher)
            if (p.x2 && 256 * c + 256 > K1) continue;
            v[c] = glu4(v[c], gv[c], um, uo);
        }
    }
#pragma unroll
    for (int c = DCH; c < KCH; ++c) {
        const int i = chunk_col(c, lane);             // (the column kept in a local: through in_row() the Plain kernels take two VGPRs more)
        if (FULL || i < K) st4(xs + wave * LD + i, v[c]);    // (rows >= B hold a copy of row B-1; their outputs are never stored)
    }
    STAMP(2);
#ifdef AMT_STAMPS
    // the matrix phase's end stamp, and the latest "row landed" and "row complete in LDS" stamps of the 16 waves (all below)
    if (tid < 3) reinterpret_cast<unsigned long long*>(red + NW * 256)[tid] = 0;
    st_land = st_[1];                               // (lean front: the pins in front of STAMP 1 wait for the row registers)
#endif
    if constexpr (DMA) {
        // This wave's DMA chunks are in LDS once at most the loads requested behind them are outstanding: the KCH weight tiles.
        // __syncthreads() would wait vmcnt(0) for the fence in front of it, so the wait is spelled out, then the LDS writes of this
        // wave, then the bare barrier.  Through the builtin the compiler's wait bookkeeping sees the DMA loads retired: left to an asm
        // statement it waits vmcnt(0) -- weight tiles and epilogue operands -- in front of the first ds_read behind the barrier.
        asm volatile("" ::: "memory");
        if constexpr (!FFN) wait_vmcnt<KCH>();                      // (FoldedFfn: waited for in front of the vectors' LDS writes)
#ifdef AMT_STAMPS
        if (FFN) st_land = st_[6];
        else { __builtin_amdgcn_sched_barrier(0); st_land = __builtin_amdgcn_s_memrealtime(); __builtin_amdgcn_sched_barrier(0); }
#endif
        __builtin_amdgcn_s_waitcnt(0xc07f);                         // lgkmcnt(0)
#ifdef AMT_STAMPS
        __builtin_amdgcn_sched_barrier(0); st_lds = __builtin_amdgcn_s_memrealtime(); __builtin_amdgcn_sched_barrier(0);
#endif
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    } else {
#ifdef AMT_STAMPS
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0); st_lds = __builtin_amdgcn_s_memrealtime(); __builtin_amdgcn_sched_barrier(0);
#endif
        __syncthreads();
    }
    STAMP(3);
#ifdef AMT_STAMPS
    if (lane == 0) {
        atomicMax(reinterpret_cast<unsigned long long*>(red + NW * 256) + 1, st_land);
        atomicMax(reinterpret_cast<unsigned long long*>(red + NW * 256) + 2, st_lds);
    }
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long clk3 = __builtin_amdgcn_s_memtime();                  // shader-clock counter, against the 100 MHz stamps
    __builtin_amdgcn_sched_barrier(0);
#endif

    // ---- 4. epilogue operands: issued behind the prologue so that no register of the prologue's arithmetic sits
    // next to a pending load (packed VALU ops read register pairs).  Absent operands read a zero word instead of
    // being masked after the load: a select on a loaded value would be scheduled early and wait for the weights ----
    const float* bp = high ? p.bias2 : (p.bias ? p.bias + (size_t)grp * p.sel_b_stride : nullptr);      // (grp = blockIdx.z in a grouped launch)
    const bool has_b = live && bp != nullptr, has_r = !FFN && live && !high && p.mode == 0 && p.resid != nullptr;
    const float e_bias = *(has_b ? bp + (high ? n - p.n_split : p.glu_pair ? glu_pair_bias_col(n, p.N) : n) : p.zero);
    float e_res = 0.f;
    if (!FFN) e_res = *(has_r ? p.resid + (size_t)row * p.ldr + n : p.zero);
    const int t = *(p.pos ? p.pos : reinterpret_cast<const int*>(p.zero));

    // the normalised rows are the residual of the following block: workgroup (nt, m-block) publishes its
    // 16 rows x columns 16nt..16nt+15 -- and, when the product has fewer column tiles than the rows have 16-column blocks
    // (N < K: a feed-forward narrower than half the model width), the blocks one grid width further on as well
    if (LN1 && p.xn && tid < 256) {
        const int rr = tid >> 4, c = tid & 15;
        for (int cb = nt * 16; cb < K; cb += (int)gridDim.x * 16)
            if (m0 + rr < p.B) p.xn[(size_t)(m0 + rr) * K + cb + c] = xs[rr * LD + cb + c];
    }
    // folded FFN: the LayerNorm half of the staged row is the residual of the low columns
    if (PRO == Pro::FoldedGlu && live && !high) e_res = xs[(row - m0) * LD + K1 + n];
    const float* fgs = smem + MT * LD;              // FoldedFfn: the per-column vectors and the rows' statistics
    float f_mu = 0.f, f_rs = 0.f;
    if (PRO == Pro::FoldedFfn) {
        f_mu = fgs[2 * K + 2 * (lane & 15)]; f_rs = fgs[2 * K + 2 * (lane & 15) + 1];       // A-fragment row of this lane
        if (live && !high) {
            const float* sr = fgs + 2 * K + 2 * (row - m0);
            e_res = fmaf(fmaf(xs[(row - m0) * LD + K1 + n], sr[1], -sr[0] * sr[1]), fgs[K1 + n], fgs[K + K1 + n]);      // (same spelling as the fragments')
        }
    }

    // ---- main: 4 MFMAs per k-tile ----
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    constexpr bool FIX = PRO == Pro::FoldedFfn;
    if constexpr (PIPE) {
        // The wave index through readfirstlane: the compiler then knows that the first tile, the tile count and the side of K1 are
        // wave-uniform -- scalar branches (none at all for a wave that owns KCH tiles) and the uniform address parts in SGPRs.
        const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int kt0s = wv * tpw, nown = min(tpw, kt_n - kt0s);      // tiles kt0s .. kt0s + nown - 1 (none when nown <= 0)
        const float* xa = xs + (lane & 15) * LD + 4 * (lane >> 4) + kt0s * 16;
        const float* fg = fgs + 4 * (lane >> 4) + kt0s * 16;
        const float f_nm = -f_mu * f_rs;
        if (nown == KCH) {
            // every wave of the high / unsplit column tiles at K = KCH * 256
            if (!FIX || (kt0s + KCH) * 16 <= K1) acc = tiles_pipelined<KCH, PRO, 0>(xa, fg, K, wt, f_rs, f_nm, kt0s * 16, K1);
            else if (kt0s * 16 >= K1) acc = tiles_pipelined<KCH, PRO, 1>(xa, fg, K, wt, f_rs, f_nm, kt0s * 16, K1);
            else acc = tiles_pipelined<KCH, PRO, 2>(xa, fg, K, wt, f_rs, f_nm, kt0s * 16, K1);
        } else if (nown > 0) {
            // fewer tiles (low-column tiles of a split launch, ragged K)
            if (!FIX || (kt0s + nown) * 16 <= K1) acc = tiles_partial<KCH, PRO, 0>(xa, fg, K, wt, f_rs, f_nm, kt0s * 16, K1, nown);
            else if (kt0s * 16 >= K1) acc = tiles_partial<KCH, PRO, 1>(xa, fg, K, wt, f_rs, f_nm, kt0s * 16, K1, nown);
            else acc = tiles_partial<KCH, PRO, 2>(xa, fg, K, wt, f_rs, f_nm, kt0s * 16, K1, nown);
        }
    } else {                                         // the serial loop: every tile behind its own (lane-level) guard, reads at their use
        const float* xa = xs + (lane & 15) * LD + kt0 * 16 + 4 * (lane >> 4);
#pragma unroll
        for (int i = 0; i < KCH; ++i) {
            if (i < tpw && kt0 + i < kt_n) {
                float4 a0 = ld4(xa + i * 16);
                if (FIX) {
                    // the folded-FFN fix of this fragment, in packed pairs.  The side of K1 is wave-uniform (K1 % 16 == 0).
                    const int kc = (kt0 + i) * 16 + 4 * (lane >> 4);
                    const float4 g = ld4(fgs + kc), h = ld4(fgs + K + kc);
                    const float f_nm = -f_mu * f_rs;
                    if ((kt0 + i) * 16 < K1) a0 = ffn_fix<0, true>(a0, g, h, f_rs, f_nm, true);
                    else a0 = ffn_fix<1, true>(a0, g, h, f_rs, f_nm, false);
                }
                acc = mfma_tile(a0, wt[i], acc);
            }
        }
    }
    // ---- cross-wave reduction in fixed order ----
#ifdef AMT_STAMPS
    if (acc[0] == 1.2345e-30f) st_[6] = 1;          // the stamp must follow the MFMA results, not just their issue
#endif
    STAMP(4);
#ifdef AMT_STAMPS
    // end of the workgroup's matrix phase: the latest end-of-MFMA stamp of its 16 waves (one LDS max per wave, in the word behind the partial tiles)
    unsigned long long* wg_end = reinterpret_cast<unsigned long long*>(red + NW * 256);
    if (lane == 0) atomicMax(wg_end, st_[4]);
#endif
    store_partials(red + wave * 256, acc, lane);
    __syncthreads();
    STAMP(5);
#ifdef AMT_STAMPS
    // slot 7: high word = the workgroup's matrix phase (staging barrier -> last wave's MFMA results) in 10 ns ticks, low word = shader
    // clocks that wave 0 counted between STAMP 3 and STAMP 5 (their ratio to st[5] - st[3] is the in-kernel clock under MFMA load)
    {
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long clk5 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
        st_[7] = ((*wg_end - st_[3]) << 32) | ((clk5 - clk3) & 0xffffffffull);
        st_land = wg_end[1]; st_lds = wg_end[2];
    }
#endif
    float val = 0.f;
    if (tid < 256) val = sum_partials(red, tid) + e_bias;
    if (p.rope) {
        // interleaved pairs sit in adjacent lanes of the same row (16-column tiles): even column y = x*c - x'*s, odd y = x*c + x'*s
        const float other = __shfl_xor(val, 1, 64);
        if (n < p.rope_cols) {
            const int e2 = (n % p.rope_dim) & ~1;
            const float* rp = p.rope + (size_t)t * p.rope_dim + e2;
            const float c = rp[0], sn = rp[1];
            val = (n & 1) ? val * c + other * sn : val * c - other * sn;
        }
    }
    if (p.glu_pair) {                                // (outside `live`: the exchange takes every lane of the wave)
        val = glu_pair_value(val, n & 15);
        if (live && (n & 8)) p.y[(size_t)row * p.ldy + (n >> 4) * 8 + (n & 7)] = val;
    } else if (live) {
        float* ybase = p.y + (size_t)zg * p.y_group_off;
        if (high) {
            p.y2[(size_t)row * p.ldy2 + (n - p.n_split)] = val;
        } else {
            if (n < p.scale_cols) val *= p.scale;
            if (p.mode == 0) {
                val += e_res;
                val = act(val, p.relu);
                ybase[(size_t)row * p.ldy + n] = val;
            } else if (n < p.d) {
                ybase[(size_t)row * p.ldy + n] = val;
            } else {
                const int nn = (n < 2 * p.d) ? n - p.d : n - 2 * p.d;
                const int hh = nn / p.hd, cc = nn - hh * p.hd;
                float* dst = (n < 2 * p.d) ? p.kcache : p.vcache;
                dst[(((size_t)row * p.H + hh) * p.cap + t) * p.hd + cc] = val;
            }
        }
    }
#ifdef AMT_STAMPS
    STAMP(6);
    if (p.stamps && tid == 0) {
        unsigned long long* o = p.stamps + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8;
        for (int i = 0; i < 8; ++i) o[i] = st_[i];
        if (p.stamps_rows) {
            unsigned long long* r = p.stamps_rows + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
            r[0] = st_land; r[1] = st_lds;
        }
    }
#endif
}

int32_t device_ordinal(int* dev) {
    AMT_HIP(hipGetDevice(dev));
    AMT_CHECK_ARG(*dev >= 0 && *dev < 64, "decode_gemm: device ordinal %d out of range", *dev);
    return 0;
}

// > 64 KiB of dynamic LDS needs the opt-in (gfx950: 160 KiB per CU).  The attribute belongs to the (function, device)
// pair, so the flag is kept per device ordinal and per kernel, under a lock (host threads may launch concurrently)
template <auto Kernel>
int32_t allow_big_lds() {
    static bool attr_set[64] = {false};
    static std::mutex mu;
    int dev = 0;
    if (int32_t rc = device_ordinal(&dev)) return rc;
    std::lock_guard<std::mutex> lock(mu);
    if (!attr_set[dev]) {
        AMT_HIP(hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set[dev] = true;
    }
    return 0;
}

template <int KCH, bool FULL, Pro PRO, bool PIPE, bool LEAN = false, bool DMA = false>
int32_t launch_one_loop(const DecodeGemmParams& p, size_t lds, hipStream_t stream) {
    if (int32_t rc = allow_big_lds<decode_gemm_kernel<KCH, FULL, PRO, PIPE, LEAN, DMA>>()) return rc;
    hipLaunchKernelGGL((decode_gemm_kernel<KCH, FULL, PRO, PIPE, LEAN, DMA>), dim3(cdiv(p.N, 16), cdiv(p.B, MT), p.n_groups > 1 ? p.n_groups : 1), dim3(NW * 64), lds, stream, p);
    AMT_LAUNCH_CHECK();
    return 0;
}

// what the lean front reads, from the parameters of a launch that amt_decode_gemm_lean_ok() accepts
DecodeGemmFront lean_front(const DecodeGemmParams& p) {
    DecodeGemmFront f{};
    f.x = p.x; f.x2b = p.x2 - p.K1; f.Wp = p.Wp; f.Wp2 = p.Wp2;
    f.fold_g = p.fold_g; f.fold_c = p.fold_c; f.ln_wb = p.ln_w ? p.ln_w - p.K1 : nullptr; f.ln_bb = p.ln_b ? p.ln_b - p.K1 : nullptr;
    f.x_row_bytes = (unsigned)p.ldx * 4u; f.x2_row_bytes = (unsigned)p.ldx2 * 4u;
    f.B = p.B; f.K = p.K; f.K1 = p.K1; f.LD = p.K + XPAD;
    f.nts = p.n_split > 0 ? p.n_split >> 4 : INT_MAX;
    f.ktn_lo = (p.n_split > 0 ? p.K1 : p.K) / 16; f.tpw_lo = cdiv(f.ktn_lo, NW);
    f.ktn_hi = p.K / 16; f.tpw_hi = cdiv(f.ktn_hi, NW);
    f.red_off = MT * f.LD + (p.pro == 1 ? 2 * p.K + 2 * MT : 0);
    return f;
}

// The pipelined tile loop serves the plain and the folded-FFN prologue (every skinny GEMM of the folded decode chain); the other
// prologues keep the serial loop (LayerNorm2 / FoldedGlu sit at 114 - 126 VGPRs of the 128 a 16-wave workgroup may use).
// With it goes the lean front wherever the launcher's rule admits it.
template <int KCH, bool FULL, Pro PRO>
int32_t launch_one(const DecodeGemmParams& p, size_t lds, hipStream_t stream) {
    if constexpr (PRO == Pro::Plain || PRO == Pro::FoldedFfn) {
        if constexpr (FULL && KCH >= 2) {
            if (amt_decode_gemm_lean_ok(p)) {
                DecodeGemmParams q = p;
                q.front = lean_front(p);
                if constexpr (PRO == Pro::Plain || KCH % 3 == 0) {
                    if (amt_decode_gemm_rows_dma_ok(p)) return launch_one_loop<KCH, FULL, PRO, true, true, true>(q, lds, stream);
                }
                return launch_one_loop<KCH, FULL, PRO, true, true>(q, lds, stream);
            }
        }
        if (!p.serial_loop) return launch_one_loop<KCH, FULL, PRO, true>(p, lds, stream);
    }
    return launch_one_loop<KCH, FULL, PRO, false>(p, lds, stream);
}

// ---- parts shared by the two wide kernels below (K = KCH * 256, packed weights, Plain / LayerNorm / Glu) ----
// all NTW x KCH weight tiles of a wave (surplus column tiles repeat the last one)
template <int KCH, int NTW>
__device__ __forceinline__ void wide_load_tiles(float4 (&wt)[NTW][KCH], const float* Wp, int nt0, int n_tiles, int kt0, int lane) {
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        const float* wbase = Wp + (size_t)min(nt0 + j, n_tiles - 1) * (KCH * 16) * 256;
#pragma unroll
        for (int i = 0; i < KCH; ++i) wt[j][i] = ld4(wbase + ((size_t)(kt0 + i) * 64 + lane) * 4);
    }
}
// the prologue of the row a wave holds
template <int KCH, Pro PRO>
__device__ __forceinline__ void wide_prologue(float4 (&v)[KCH], const float4* gv, const float4* g0, const float4* h0, float eps, int glu_only) {
    if (PRO == Pro::LayerNorm) {
        const RowStats st = row_stats<false>(v, [](int) { return true; }, (float)(KCH * 256), eps);
#pragma unroll
        for (int c = 0; c < KCH; ++c) v[c] = ln4(v[c], st.mean, st.rstd, g0[c], h0[c]);
    }
    if (PRO == Pro::Glu) {
        const float um = glu_only ? 0.f : 1.f, uo = glu_only ? 1.f : 0.f;      // h = u * silu(g), or silu(g) alone
#pragma unroll
        for (int c = 0; c < KCH; ++c) v[c] = glu4(v[c], gv[c], um, uo);
    }
}
// a full row into its LDS slot
template <int KCH>
__device__ __forceinline__ void wide_stage_row(float* xrow, const float4 (&v)[KCH], int lane) {
#pragma unroll
    for (int c = 0; c < KCH; ++c) st4(xrow + chunk_col(c, lane), v[c]);
}
// (The reduce-and-store epilogue of one output -- sum of the 16 partials, bias, paired gate | up or scale / residual / activation,
// store -- stays written out in each wide kernel: as a shared helper it has to be handed the kernel's parameters, every field of them
// is then read at the kernel's start instead of inside the branch that uses it, and MFMA, LDS and global loads of six instantiations
// change places against each other.  glu_pair_value(), act() and, in the one-row-block kernel, sum_partials() are the shared parts.)

// Wide products (N >= 4096: the stacked gate|up projection of a mixture-of-experts layer, 7 x 2 x dff columns): with one 16-column
// tile per workgroup such a launch is 1792 workgroups of two weight tiles per wave each, i.e. several rounds of the fixed
// stage-rows / barrier / reduce latency over the chip (16.3 us for 29 MB at config 2).  Here a workgroup keeps its 16 staged rows
// and walks NTW column tiles: all NTW x KCH weight tiles of a wave are in flight before the prologue, the rows are staged and
// normalised once, and every thread takes part in the final reduction (thread group j reduces tile j).  Same arithmetic per output
// as decode_gemm_kernel (same k order inside a wave, same fixed wave order in the reduction): results are bit-identical.
// Plain single-source products only: Plain / LayerNorm / Glu, packed weights, mode 0, no column split, no rotary epilogue.
template <int KCH, Pro PRO, int NTW>
__global__ __launch_bounds__(NW * 64) void decode_gemm_wide_kernel(DecodeGemmParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int K = KCH * 256, LD = K + XPAD;
    float* xs = smem;                               // [16][LD]
    float* red = smem + MT * LD;                    // [NTW][16 waves][256] partial tiles behind the staged rows (no barrier before they are stored)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // 1-D grid: the row blocks of one tile group are 8 linear ids apart, i.e. dispatched back to back onto the SAME XCD (round-robin
    // placement), so the group's weight tiles cross HBM / the Infinity Cache once and the second row block finds them in that L2
    const int mb = (p.B + MT - 1) / MT, n_tiles = (p.N + 15) >> 4;
    const int grp = ((int)blockIdx.x / (8 * mb)) * 8 + ((int)blockIdx.x & 7);
    if (grp * NTW >= n_tiles) return;               // the grid is padded to whole sets of 8 groups (uniform per workgroup)
    const int nt0 = grp * NTW, m0 = (((int)blockIdx.x >> 3) % mb) * MT;
    const int kt0 = wave * KCH;
    const int zg = p.n_groups > 1 ? (int)blockIdx.y : 0;       // grouped launch: one expert per blockIdx.y
    const int r = m0 + wave, rc = min(r, p.B - 1);
    const float* xr = p.x + (size_t)zg * p.x_group_off + (size_t)rc * p.ldx;
    float4 v[KCH];
#pragma unroll
    for (int c = 0; c < KCH; ++c) v[c] = ld4(xr + chunk_col(c, lane));
    float4 gv[PRO == Pro::Glu ? KCH : 1];
    if (PRO == Pro::Glu) {
        const float* gr = p.glu_gate + (size_t)zg * p.x_group_off + (size_t)rc * p.ldx;
#pragma unroll
        for (int c = 0; c < KCH; ++c) gv[c] = ld4(gr + chunk_col(c, lane));
    }
    float4 g0[PRO == Pro::LayerNorm ? KCH : 1], h0[PRO == Pro::LayerNorm ? KCH : 1];
    if constexpr (PRO == Pro::LayerNorm) load_ln<KCH, true>(g0, h0, p.ln_w, p.ln_b, lane, K);
    float4 wt[NTW][KCH];
    wide_load_tiles(wt, p.Wp + (size_t)zg * p.sel_w_stride, nt0, n_tiles, kt0, lane);
    __builtin_amdgcn_sched_barrier(0);
    wide_prologue<KCH, PRO>(v, gv, g0, h0, p.eps, p.glu_only);
    wide_stage_row(xs + wave * LD, v, lane);
    __syncthreads();

    // thread (jg, e) owns output e of tiles nt0 + jg, nt0 + jg + 4, ...
    constexpr int JN = (NTW + 3) / 4;
    const int jg = tid >> 8, e = tid & 255;
    const int el = e & 63, er = (e >> 6) & 3;
    const int row = m0 + 4 * (el >> 4) + er;
    float e_bias[JN], e_res[JN];
#pragma unroll
    for (int q = 0; q < JN; ++q) {
        const int j = jg + 4 * q, n = (nt0 + j) * 16 + (el & 15);
        const bool live = j < NTW && row < p.B && n < p.N;
        e_bias[q] = *((live && p.bias) ? p.bias + (size_t)zg * p.sel_b_stride + (p.glu_pair ? glu_pair_bias_col(n, p.N) : n) : p.zero);
        e_res[q] = *((live && p.resid) ? p.resid + (size_t)row * p.ldr + n : p.zero);
        if (PRO == Pro::LayerNorm && p.xn && j < NTW && (nt0 + j) * 16 < K) {
            const int rr = e >> 4, c = e & 15;
            if (m0 + rr < p.B) p.xn[(size_t)(m0 + rr) * K + (nt0 + j) * 16 + c] = xs[rr * LD + (nt0 + j) * 16 + c];
        }
    }

    f32x4 acc[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* xa = xs + (lane & 15) * LD + kt0 * 16 + 4 * (lane >> 4);
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
        const float4 a0 = ld4(xa + i * 16);
#pragma unroll
        for (int j = 0; j < NTW; ++j) acc[j] = mfma_tile(a0, wt[j][i], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < NTW; ++j) store_partials(red + (j * NW + wave) * 256, acc[j], lane);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < JN; ++q) {
        const int j = jg + 4 * q, n = (nt0 + j) * 16 + (el & 15);
        if (j < NTW) {
            float val = sum_partials(red + j * NW * 256, e) + e_bias[q];
            if (p.glu_pair) {                        // (j < NTW is uniform per 256-thread group: whole waves take the exchange)
                val = glu_pair_value(val, n & 15);
                if (row < p.B && n < p.N && (n & 8)) p.y[(size_t)row * p.ldy + (n >> 4) * 8 + (n & 7)] = val;      // (never a grouped launch)
            } else if (row < p.B && n < p.N) {
                if (n < p.scale_cols) val *= p.scale;
                val += e_res[q];
                val = act(val, p.relu);
                p.y[(size_t)zg * p.y_group_off + (size_t)row * p.ldy + n] = val;
            }
        }
    }
}

// The wide product for up to 32 rows in ONE workgroup (RB2): both 16-row blocks share the workgroup's weight tiles, so a tile
// group's weights cross L2 -> L1 once instead of once per row block, and the launch is half as many workgroups -- the stacked
// gate | up product of a mixture layer at 32 clips (1792 column tiles, K = 512) becomes 224 workgroups = ONE round over the chip
// instead of 448 = two (13.6 -> 11.3 us in the lockstep step's trace; lockstep V2 generate 97.6 -> 96.2 ms alternating in one
// process, profiles/r03_v2_ab.json).  Wave w stages rows w and 16 + w;
// per k-tile a weight fragment feeds two MFMA chains; the partial tiles of the two row blocks go through the same LDS region one
// after the other.  Same arithmetic per output as decode_gemm_wide_kernel (bit-identical results).  K = KCH * 256 <= 512.
template <int KCH, Pro PRO, int NTW>
__global__ __launch_bounds__(NW * 64) void decode_gemm_wide2_kernel(DecodeGemmParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int K = KCH * 256, LD = K + XPAD;
    float* xs = smem;                               // [2][16][LD]
    float* red = smem + 2 * MT * LD;                // [NTW][16 waves][256] partial tiles of ONE row block at a time
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_tiles = (p.N + 15) >> 4;
    const int grp = (int)blockIdx.x;
    if (grp * NTW >= n_tiles) return;
    const int nt0 = grp * NTW;
    const int kt0 = wave * KCH;
    float4 v[2][KCH];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const float* xr = p.x + (size_t)min(rb * MT + wave, p.B - 1) * p.ldx;
#pragma unroll
        for (int c = 0; c < KCH; ++c) v[rb][c] = ld4(xr + chunk_col(c, lane));
    }
    float4 g0[PRO == Pro::LayerNorm ? KCH : 1], h0[PRO == Pro::LayerNorm ? KCH : 1];
    if constexpr (PRO == Pro::LayerNorm) load_ln<KCH, true>(g0, h0, p.ln_w, p.ln_b, lane, K);
    float4 wt[NTW][KCH];
    wide_load_tiles(wt, p.Wp, nt0, n_tiles, kt0, lane);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) wide_prologue<KCH, PRO>(v[rb], nullptr, g0, h0, p.eps, p.glu_only);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) wide_stage_row(xs + (rb * MT + wave) * LD, v[rb], lane);
    __syncthreads();

    // thread (jg, e) owns output e of tiles nt0 + jg, nt0 + jg + 4, ... of each row block
    constexpr int JN = (NTW + 3) / 4;
    const int jg = tid >> 8, e = tid & 255;
    const int el = e & 63, er = (e >> 6) & 3;
    const int rloc = 4 * (el >> 4) + er;
    float e_bias[JN];
#pragma unroll
    for (int q = 0; q < JN; ++q) {
        const int j = jg + 4 * q, n = (nt0 + j) * 16 + (el & 15);
        e_bias[q] = *((j < NTW && n < p.N && p.bias) ? p.bias + (p.glu_pair ? glu_pair_bias_col(n, p.N) : n) : p.zero);
        if (PRO == Pro::LayerNorm && p.xn && j < NTW && (nt0 + j) * 16 < K) {
            const int rr = e >> 4, c = e & 15;
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
                if (rb * MT + rr < p.B) p.xn[(size_t)(rb * MT + rr) * K + (nt0 + j) * 16 + c] = xs[(rb * MT + rr) * LD + (nt0 + j) * 16 + c];
        }
    }

    f32x4 acc[2][NTW];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int j = 0; j < NTW; ++j) acc[rb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* xa = xs + (lane & 15) * LD + kt0 * 16 + 4 * (lane >> 4);
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
        const float4 a0 = ld4(xa + i * 16), a1 = ld4(xa + MT * LD + i * 16);
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            acc[0][j] = mfma_tile(a0, wt[j][i], acc[0][j]);
            acc[1][j] = mfma_tile(a1, wt[j][i], acc[1][j]);
        }
    }
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        if (rb) __syncthreads();                    // the first row block's partial tiles are consumed
#pragma unroll
        for (int j = 0; j < NTW; ++j) store_partials(red + (j * NW + wave) * 256, acc[rb][j], lane);
        __syncthreads();
        const int row = rb * MT + rloc;
#pragma unroll
        for (int q = 0; q < JN; ++q) {
            const int j = jg + 4 * q, n = (nt0 + j) * 16 + (el & 15);
            if (j < NTW) {
                // (written out, not sum_partials(): with the helper, in either indexing, three MFMAs and the LDS traffic next to them change places)
                float val = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w) val += red[(j * NW + w) * 256 + e];
                val += e_bias[q];
                if (p.glu_pair) {
                    val = glu_pair_value(val, n & 15);
                    if (row < p.B && n < p.N && (n & 8)) p.y[(size_t)row * p.ldy + (n >> 4) * 8 + (n & 7)] = val;
                } else if (row < p.B && n < p.N) {
                    if (n < p.scale_cols) val *= p.scale;
                    if (p.resid) val += p.resid[(size_t)row * p.ldr + n];      // (read late: not one more operand held across the MFMAs of two row blocks)
                    val = act(val, p.relu);
                    p.y[(size_t)row * p.ldy + n] = val;
                }
            }
        }
    }
}

template <int KCH, Pro PRO, int NTW>
int32_t launch_wide2(const DecodeGemmParams& p, hipStream_t stream) {
    if (int32_t rc = allow_big_lds<decode_gemm_wide2_kernel<KCH, PRO, NTW>>()) return rc;
    constexpr size_t lds = (size_t)2 * MT * (KCH * 256 + XPAD) * sizeof(float) + (size_t)NTW * NW * 256 * sizeof(float);      // rows of both blocks | partial tiles
    static_assert(lds <= 160 * 1024, "rows + partial tiles must fit the 160 KiB of LDS");
    hipLaunchKernelGGL((decode_gemm_wide2_kernel<KCH, PRO, NTW>), dim3(cdiv(cdiv(p.N, 16), NTW)), dim3(NW * 64), lds, stream, p);
    AMT_LAUNCH_CHECK();
    return 0;
}

template <int KCH, Pro PRO, int NTW>
int32_t launch_wide(const DecodeGemmParams& p, hipStream_t stream) {
    if (int32_t rc = allow_big_lds<decode_gemm_wide_kernel<KCH, PRO, NTW>>()) return rc;
    constexpr size_t lds = (size_t)MT * (KCH * 256 + XPAD) * sizeof(float) + (size_t)NTW * NW * 256 * sizeof(float);      // rows | partial tiles
    static_assert(lds <= 160 * 1024, "rows + partial tiles must fit the 160 KiB of LDS");
    const int groups8 = cdiv(cdiv(cdiv(p.N, 16), NTW), 8) * 8;
    hipLaunchKernelGGL((decode_gemm_wide_kernel<KCH, PRO, NTW>), dim3(groups8 * cdiv(p.B, MT), p.n_groups > 1 ? p.n_groups : 1), dim3(NW * 64), lds, stream, p);
    AMT_LAUNCH_CHECK();
    return 0;
}

// The one place that maps DecodeGemmParams::pro (0 none, 1 folded FFN, 2 folded gated FFN), glu_gate and ln_w / ln2_w onto the prologue.
// (The `if constexpr` guards only keep instantiations from being compiled that the launcher's checks rule out.)
template <int KCH, bool FULL>
int32_t launch_variant(const DecodeGemmParams& p, size_t lds, hipStream_t stream) {
#ifdef AMT_EXPERIMENT
    // timing only (wrong values): what does the folded-FFN prologue cost?  exp_a = 1 launches the same product with the plain staging
    if (p.pro == 1 && amt_tuning().exp_a == 1) return launch_one<KCH, FULL, Pro::Plain>(p, lds, stream);
#endif
    if (p.pro == 1) return launch_one<KCH, FULL, Pro::FoldedFfn>(p, lds, stream);
    if (p.pro == 2) { if constexpr (FULL && KCH >= 2) return launch_one<KCH, FULL, Pro::FoldedGlu>(p, lds, stream); }
    if (p.glu_gate) return launch_one<KCH, FULL, Pro::Glu>(p, lds, stream);
    if (p.ln_w && p.ln2_w) { if constexpr (KCH <= 4) return launch_one<KCH, FULL, Pro::LayerNorm2>(p, lds, stream); }
    if (p.ln_w) { if constexpr (KCH <= 4) return launch_one<KCH, FULL, Pro::LayerNorm>(p, lds, stream); }
    return launch_one<KCH, FULL, Pro::Plain>(p, lds, stream);
}

}  // namespace

// The lean front's rule, in one place: the folded chain's form of launch.  (launch_variant maps pro and the prologue pointers onto
// Plain / FoldedFfn exactly when glu_gate, ln2_w and -- with pro 0 -- ln_w are absent; two sources of whole 256-column chunks make
// K one of 512 / 768 / 1024 / 1536, i.e. a FULL instantiation.)
bool amt_decode_gemm_lean_ok(const DecodeGemmParams& p) {
    if (p.generic_front || p.serial_loop) return false;
    if (!p.x || !p.x2 || !p.Wp || p.B <= 0 || p.ldw != 0 || p.K1 <= 0 || p.K1 >= p.K || p.K1 % 256 != 0 || p.K % 256 != 0 || p.K > 1536 || p.K == 1280) return false;
    if (p.sel || p.n_groups > 1 || p.pos || p.mode != 0 || p.rope || p.glu_pair || p.glu_gate || p.ln2_w || p.xn) return false;
    if (p.pro == 1 ? !(p.fold_g && p.fold_c && p.ln_w && p.ln_b) : (p.pro != 0 || p.ln_w)) return false;
    if (p.n_split > 0 && p.n_split < p.N && !p.Wp2) return false;
    // 32-bit byte offsets: the last row's end in x and x2, the last output, and the last tile of either packed weight
    const unsigned long long lim = 1ull << 32, rows = (unsigned long long)(p.B - 1);
    const unsigned long long n_lo = p.n_split > 0 ? p.n_split : p.N, n_hi = p.N - n_lo;
    if ((rows * p.ldx + p.K1) * 4 >= lim || (rows * p.ldx2 + (p.K - p.K1)) * 4 >= lim) return false;
    if ((rows * p.ldy + n_lo) * 4 >= lim || (rows * p.ldy2 + n_hi) * 4 >= lim) return false;
    if ((n_lo + 15) / 16 * (p.n_split > 0 ? p.K1 : p.K) * 64 >= lim || (n_hi + 15) / 16 * p.K * 64 >= lim) return false;
    return true;
}

// Rows by LDS-DMA: what the lean front already asks for (whole 256-column chunks, 32-bit offsets, 16-byte aligned rows: ldx and
// ldx2 are multiples of four floats) and, behind the folded-FFN prologue, a u half of exactly a third of the chunks (dff = 2 d_model:
// K1 = 2 (K - K1)), which is what the kernel's instantiations keep in registers.  reg_rows 1 keeps the registers, 0 follows the
// process-wide default, -1 takes the DMA form whatever that says.
static std::atomic<int> g_rows_dma{AMT_GEMM_ROWS_DMA_DEFAULT};
void amt_decode_gemm_rows_dma(int on) { g_rows_dma.store(on ? 1 : 0, std::memory_order_relaxed); }
bool amt_decode_gemm_rows_dma_ok(const DecodeGemmParams& p) {
    if (p.reg_rows > 0 || (p.reg_rows == 0 && g_rows_dma.load(std::memory_order_relaxed) == 0) || !amt_decode_gemm_lean_ok(p)) return false;
    if (((uintptr_t)p.x | (uintptr_t)p.x2) % 16 != 0) return false;
    return p.pro == 0 || p.K1 == 2 * (p.K - p.K1);
}

int32_t amt_launch_pack_weight(const float* W, float* P, int N, int K, hipStream_t stream, int ldw) {
    AMT_CHECK_ARG(K % 16 == 0 && (ldw == 0 || (ldw >= K && ldw % 4 == 0)), "pack_weight: K=%d must be a multiple of 16 (ldw=%d)", K, ldw);
    const int tiles = cdiv(N, 16) * (K / 16);
    hipLaunchKernelGGL(pack_weight_kernel, dim3(tiles), dim3(64), 0, stream, W, P, N, K, ldw ? ldw : K);
    AMT_LAUNCH_CHECK();
    return 0;
}

// a few zero words in global memory per device (absent bias / residual / position read these)
static int32_t zero_words(const float** out) {
    static float* buf[64] = {nullptr};
    static std::mutex mu;                            // several host threads may launch concurrently (one stream each)
    int dev = 0;
    if (int32_t rc = device_ordinal(&dev)) return rc;
    std::lock_guard<std::mutex> lock(mu);
    if (!buf[dev]) {
        AMT_HIP(hipMalloc((void**)&buf[dev], 256));
        AMT_HIP(hipMemset(buf[dev], 0, 256));
    }
    *out = buf[dev];
    return 0;
}

int32_t amt_decode_gemm_init() { const float* z; return zero_words(&z); }

int32_t amt_launch_decode_gemm(const DecodeGemmParams& p_in, hipStream_t stream) {
    DecodeGemmParams p = p_in;
    if (int32_t zrc = zero_words(&p.zero)) return zrc;
    AMT_CHECK_ARG(p.B > 0 && p.B <= MAXB, "decode_gemm: B=%d outside (0,%d]", p.B, MAXB);
    AMT_CHECK_ARG(p.K % 32 == 0 && p.K <= 1536, "decode_gemm: K=%d must be a multiple of 32 and <= 1536", p.K);
    AMT_CHECK_ARG(p.N > 0 && p.ldx % 4 == 0, "decode_gemm: bad N/ldx");
    AMT_CHECK_ARG(p.mode == 0 || (p.kcache && p.vcache && p.d > 0 && p.N == 3 * p.d && p.d == p.H * p.hd), "decode_gemm: bad QKV epilogue");
    if (p.x2) AMT_CHECK_ARG(p.K1 > 0 && p.K1 < p.K && p.K1 % 16 == 0 && p.ldx >= p.K1 && p.ldx2 >= p.K - p.K1 && p.ldx2 % 4 == 0,
                            "decode_gemm: bad two-source split K1=%d of K=%d", p.K1, p.K);
    else AMT_CHECK_ARG(p.ldx >= p.K, "decode_gemm: ldx=%d < K=%d", p.ldx, p.K);
    if (p.n_split) AMT_CHECK_ARG(p.x2 && p.n_split % 16 == 0 && p.n_split <= p.N && p.mode == 0 && (p.n_split == p.N || (p.Wp2 && p.y2)),
                                 "decode_gemm: bad column split %d of N=%d", p.n_split, p.N);
    AMT_CHECK_ARG(!p.sel || p.n_split == 0, "decode_gemm: a device-selected weight group cannot be combined with a column split");
    AMT_CHECK_ARG(p.ldw == 0 || (p.ldw >= p.K && p.ldw % 4 == 0 && p.n_split == 0 && !p.sel), "decode_gemm: bad un-packed weight (ldw=%d)", p.ldw);
    AMT_CHECK_ARG(p.n_groups <= 1 || (!p.sel && p.n_split == 0 && !p.x2 && p.ldw == 0 && !p.resid && p.mode == 0 && p.n_groups <= 65535), "decode_gemm: a grouped launch takes plain single-source products");
    AMT_CHECK_ARG(!p.glu_gate || p.pro == 2 || (!p.ln_w && p.pro == 0 && (!p.x2 || (p.K1 % 256 == 0 && p.K % 256 == 0 && p.n_groups <= 1 && !p.glu_only))),
                  "decode_gemm: the gated prologue takes no LayerNorm, and a second source only behind whole 256-column chunks");
    AMT_CHECK_ARG(!p.glu_pair || (p.N % 16 == 0 && p.mode == 0 && !p.resid && !p.rope && p.n_split == 0 && !p.sel && p.n_groups <= 1 && p.scale_cols == 0 &&
                                  !p.relu && p.ldy >= p.N / 2), "decode_gemm: the paired gate | up epilogue takes a plain product of N %% 16 == 0 columns");
    AMT_CHECK_ARG(!p.rope || (p.pos && p.rope_dim > 0 && p.rope_dim % 2 == 0 && p.rope_cols % 2 == 0 && p.n_split == 0), "decode_gemm: bad rotary epilogue");
    if (p.pro == 2) {
        AMT_CHECK_ARG(p.x2 && p.glu_gate && p.fold_g && p.fold_c && p.fold_g2 && p.fold_c2 && p.ln_w && p.ln_b && !p.resid && p.K1 % 256 == 0 &&
                      (p.K == 512 || p.K == 768 || p.K == 1024 || (p.K == 1536 && p.K - p.K1 >= 512)) && p.n_groups <= 1 && !p.sel && p.ldw == 0,
                      "decode_gemm: incomplete folded gated-FFN prologue (K1=%d K=%d)", p.K1, p.K);
    } else if (p.pro == 1) {
        AMT_CHECK_ARG(p.x2 && p.fold_g && p.fold_c && p.ln_w && p.ln_b && !p.resid, "decode_gemm: incomplete folded-FFN prologue");
    } else {
        AMT_CHECK_ARG(!p.ln_w || (!p.x2 && p.K <= 1024), "decode_gemm: the LayerNorm prologue takes a single source of K <= 1024");
    }
    AMT_CHECK_ARG(!p.ln2_w || (p.ln_w && p.ln_b && p.ln2_b && p.pro == 0 && !p.glu_gate), "decode_gemm: the second LayerNorm follows a first one");
    // wide plain products: several column tiles per workgroup (see decode_gemm_wide_kernel)
    // the grouped down projections of a mixture layer (gated prologue): more workgroups than the chip holds at once with one
    // tile each, one round with two
    const int wide_grp = amt_tuning().wide_grouped;
    if (wide_grp > 0 && p.n_groups > 1 && !p.ln_w && p.pro == 0 && !p.rope && !p.x2 && p.mode == 0 && p.ldw == 0 && !p.sel &&
        (p.K == 512 || p.K == 1024) && cdiv(p.N, 16) * cdiv(p.B, MT) * p.n_groups > 256) {
        if (p.glu_gate) return p.K == 512 ? launch_wide<2, Pro::Glu, 2>(p, stream) : launch_wide<4, Pro::Glu, 2>(p, stream);
        return p.K == 512 ? launch_wide<2, Pro::Plain, 2>(p, stream) : launch_wide<4, Pro::Plain, 2>(p, stream);      // (gated already: the producer's paired epilogue)
    }
    const int wide_ntw = amt_tuning().wide_ntw;
    if (wide_ntw > 0 && p.N >= 4096 && !p.x2 && p.n_split == 0 && !p.sel && p.n_groups <= 1 && p.mode == 0 && !p.rope && !p.glu_gate && p.pro == 0 &&
        p.ldw == 0 && (p.K == 512 || p.K == 1024) && (!p.ln_w || p.ln_b) && !p.ln2_w) {
        const bool ln = p.ln_w != nullptr;
        // 17 .. 32 rows: both row blocks in one workgroup (half the workgroups, the weights through L1 once)
        if (p.K == 512 && p.B > MT && p.B <= 2 * MT && amt_tuning().wide_rb2) return ln ? launch_wide2<2, Pro::LayerNorm, 4>(p, stream) : launch_wide2<2, Pro::Plain, 4>(p, stream);
        if (p.K == 512) {
            if (wide_ntw == 7) return ln ? launch_wide<2, Pro::LayerNorm, 7>(p, stream) : launch_wide<2, Pro::Plain, 7>(p, stream);
            return ln ? launch_wide<2, Pro::LayerNorm, 4>(p, stream) : launch_wide<2, Pro::Plain, 4>(p, stream);
        }
        return ln ? launch_wide<4, Pro::LayerNorm, 4>(p, stream) : launch_wide<4, Pro::Plain, 4>(p, stream);
    }
    // staged rows | folded-FFN vectors | the waves' partial tiles
    const size_t lds = (size_t)MT * (p.K + XPAD) * sizeof(float) + (p.pro == 1 ? (size_t)(2 * p.K + 2 * MT) * sizeof(float) : 0) +
                       (p.pro == 2 ? (size_t)(2 * p.K + 2 * p.K1) * sizeof(float) : 0) + (size_t)NW * 256 * sizeof(float)
#ifdef AMT_STAMPS
                       + 32                          // the matrix phase's end stamp, the rows' two
#endif
        ;
    int32_t rc;
    switch (p.K) {
        case 256: rc = launch_variant<1, true>(p, lds, stream); break;
        case 512: rc = launch_variant<2, true>(p, lds, stream); break;
        case 768: rc = launch_variant<3, true>(p, lds, stream); break;
        case 1024: rc = launch_variant<4, true>(p, lds, stream); break;
        case 1536: rc = launch_variant<6, true>(p, lds, stream); break;
        default:
            if (p.K < 256) rc = launch_variant<1, false>(p, lds, stream);
            else if (p.K < 1024) rc = launch_variant<4, false>(p, lds, stream);
            else rc = launch_variant<6, false>(p, lds, stream);
    }
    if (rc) return rc;
    AMT_LAUNCH_CHECK();
    return 0;
}
