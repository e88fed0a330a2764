// Go/no-go for sourcing layer 0's self-attention keys from shared tables: the stream shape of
// attn_decode_body at config 2 (256 workgroups x 512 threads, hd = 64: 16 lanes per key row, 4 keys per wave-instruction, 8 waves,
// 4 key groups per batch, two batches in flight, + Er, online softmax, both merges), with the key / value rows taken from
//   (a) a per-(clip, head) cache [B][H][cap][64] x 2 with non-temporal loads, as the library does today (three caches cycled, 403 MB,
//       so that neither L2 nor the Infinity Cache serves them), or
//   (b) ONE table [H][T][K64 | V64] shared by the 32 clips of a head (plain loads, meant to stay in L2) plus, per key and side, two
//       16-byte LDS reads (the head's TR / TA slices, staged once per workgroup; ids staged as bytes) and the sum
//       ((TR[root] + TA[attr]) + key * tk) + TP[j] of write_next_input, or
//   (c) = (b) with the workgroup order transposed (linear id = b + B*h): if workgroups are dealt to the 8 XCDs round-robin by linear
//       id, (b) puts the 32 clips of a head on one XCD and (c) spreads them over all 8, i.e. every L2 fetches every head's table.
// Between two timed launches a 64 MB buffer is streamed through L2; the cost of that flush launch alone is measured and subtracted.
// usage: ubench_layer0_tables.bin      (prints one line per variant and key count)
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/ubench_layer0_tables.cpp -o tools/ubench_layer0_tables.bin
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <functional>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

constexpr int B = 32, H = 8, HD = 64, T = 1024, CAP = 1025, ROWS = 32;
constexpr int NW = 8, UNROLL = 4, LPK = HD / 4, KPW = 64 / LPK, STRIDE = NW * KPW * UNROLL;

struct P {
    const float* k; const float* v;          // (a): [B][H][CAP][HD]
    const float* tab;                        // (b): [H][T][2*HD]
    const float* tr; const float* ta;        // [H][ROWS][2*HD]
    const float* tk;                         // [H][2*HD]
    const float* key;                        // [B]
    const int64_t* roots; const int64_t* attrs;   // [B][T]
    const float* Er;                         // [T][HD]
    const float* q;                          // [B][H][HD]
    float* o;                                // [B][H][HD]
    int n_keys, transposed;
};

struct Batch { float4 k[UNROLL], v[UNROLL], e[UNROLL]; };

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 ld4_nt(const float* p) {
    typedef float v4 __attribute__((ext_vector_type(4)));
    v4 t = __builtin_nontemporal_load(reinterpret_cast<const v4*>(p));
    return make_float4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ float group_sum16(float s) {
#pragma unroll
    for (int off = 1; off < LPK; off <<= 1) s += __shfl_xor(s, off, 64);
    return s;
}

template <bool TAB>
__device__ __forceinline__ void load_batch(Batch& bt, const float* kb, const float* vb, const float* eb, int j0, int sub, int c4, int n_keys) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const int j = j0 + u * NW * KPW + sub, jc = j < n_keys ? j : 0;
        if (TAB) {
            bt.k[u] = ld4(kb + (unsigned)(jc * 2 * HD + c4));
            bt.v[u] = ld4(kb + (unsigned)(jc * 2 * HD + HD + c4));
        } else {
            bt.k[u] = ld4_nt(kb + (unsigned)(jc * HD + c4));
            bt.v[u] = ld4_nt(vb + (unsigned)(jc * HD + c4));
        }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const int j = j0 + u * NW * KPW + sub;
        bt.e[u] = ld4(eb + (unsigned)((j < n_keys ? j : 0) * HD + c4));
    }
}

template <bool TAB>
__device__ __forceinline__ void consume_batch(const Batch& bt, const float4 q4, int j0, int sub, int c4, int n_keys, const float* s_tr, const float* s_ta,
                                              const unsigned char* s_root, const unsigned char* s_attr, float kv, const float4 tkk, const float4 tkv,
                                              float& m, float& l, float4& o) {
    float4 tk4[UNROLL], tv4[UNROLL];
    if (TAB) {
        // the batch's ids, then its sixteen rows, then the sums, in front of the softmax chain (read key by key inside it, as the first
        // version of this tool did, every key pays three serial LDS round trips: profiles/r06_layer0_tables_ubench.txt has both)
        int ir[UNROLL], ia[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int j = j0 + u * NW * KPW + sub, jc = j < n_keys ? j : 0;
            ir[u] = s_root[jc]; ia[u] = s_attr[jc];
        }
        float4 rk[UNROLL], ak[UNROLL], rv[UNROLL], av[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const float* r = s_tr + ir[u] * 2 * HD + c4;
            const float* a = s_ta + ia[u] * 2 * HD + c4;
            rk[u] = ld4(r); ak[u] = ld4(a); rv[u] = ld4(r + HD); av[u] = ld4(a + HD);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            tk4[u].x = ((rk[u].x + ak[u].x) + kv * tkk.x) + bt.k[u].x; tk4[u].y = ((rk[u].y + ak[u].y) + kv * tkk.y) + bt.k[u].y;
            tk4[u].z = ((rk[u].z + ak[u].z) + kv * tkk.z) + bt.k[u].z; tk4[u].w = ((rk[u].w + ak[u].w) + kv * tkk.w) + bt.k[u].w;
            tv4[u].x = ((rv[u].x + av[u].x) + kv * tkv.x) + bt.v[u].x; tv4[u].y = ((rv[u].y + av[u].y) + kv * tkv.y) + bt.v[u].y;
            tv4[u].z = ((rv[u].z + av[u].z) + kv * tkv.z) + bt.v[u].z; tv4[u].w = ((rv[u].w + av[u].w) + kv * tkv.w) + bt.v[u].w;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const int j = j0 + u * NW * KPW + sub;
        float4 k4 = bt.k[u], v4 = bt.v[u];
        if (TAB) { k4 = tk4[u]; v4 = tv4[u]; }
        k4.x += bt.e[u].x; k4.y += bt.e[u].y; k4.z += bt.e[u].z; k4.w += bt.e[u].w;
        float s = q4.x * k4.x + q4.y * k4.y + q4.z * k4.z + q4.w * k4.w;
        s = group_sum16(s);
        if (j < n_keys) {
            const float mn = fmaxf(m, s);
            const float alpha = __expf(m - mn), pj = __expf(s - mn);
            l = l * alpha + pj;
            o.x = o.x * alpha + pj * v4.x; o.y = o.y * alpha + pj * v4.y;
            o.z = o.z * alpha + pj * v4.z; o.w = o.w * alpha + pj * v4.w;
            m = mn;
        }
    }
}

template <bool TAB>
__global__ __launch_bounds__(NW * 64) void k_stream(P p) {
    __shared__ float sm_m[NW], sm_l[NW];
    __shared__ __attribute__((aligned(16))) float sm_o[NW][HD];
    __shared__ __attribute__((aligned(16))) float s_tr[TAB ? ROWS * 2 * HD : 4], s_ta[TAB ? ROWS * 2 * HD : 4];
    __shared__ unsigned char s_root[TAB ? T : 4], s_attr[TAB ? T : 4];
    const int lin = blockIdx.x;
    const int h = p.transposed ? lin / B : lin % H, b = p.transposed ? lin % B : lin / H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c4 = (lane % LPK) * 4, sub = lane / LPK;
    const int n_keys = p.n_keys;
    const float* kb = TAB ? p.tab + (size_t)h * T * 2 * HD : p.k + ((size_t)b * H + h) * CAP * HD;
    const float* vb = TAB ? nullptr : p.v + ((size_t)b * H + h) * CAP * HD;
    const float* eb = p.Er + (size_t)(T - 1 - n_keys) * HD;
    Batch b0, b1;
    int j0 = wave * KPW;
    float kv = 0.f;
    float4 tkk = make_float4(0.f, 0.f, 0.f, 0.f), tkv = tkk;
    if (TAB) {
        // the small L2 loads in front of the stream (vector loads return in issue order), complete at the one barrier
        float4 r4[2], a4[2];             // ROWS * 2 * HD floats = 2 float4 per thread
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            r4[i] = ld4(p.tr + (size_t)h * ROWS * 2 * HD + (i * NW * 64 + threadIdx.x) * 4);
            a4[i] = ld4(p.ta + (size_t)h * ROWS * 2 * HD + (i * NW * 64 + threadIdx.x) * 4);
        }
        int64_t ri[2], ai[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int j = i * NW * 64 + threadIdx.x;
            ri[i] = p.roots[(size_t)b * T + (j < n_keys ? j : 0)];
            ai[i] = p.attrs[(size_t)b * T + (j < n_keys ? j : 0)];
        }
        kv = p.key[b];
        tkk = ld4(p.tk + h * 2 * HD + c4); tkv = ld4(p.tk + h * 2 * HD + HD + c4);
        load_batch<TAB>(b0, kb, vb, eb, j0, sub, c4, n_keys);
        load_batch<TAB>(b1, kb, vb, eb, j0 + STRIDE, sub, c4, n_keys);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *reinterpret_cast<float4*>(&s_tr[(i * NW * 64 + threadIdx.x) * 4]) = r4[i];
            *reinterpret_cast<float4*>(&s_ta[(i * NW * 64 + threadIdx.x) * 4]) = a4[i];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            s_root[i * NW * 64 + threadIdx.x] = (unsigned char)ri[i];
            s_attr[i * NW * 64 + threadIdx.x] = (unsigned char)ai[i];
        }
    } else {
        load_batch<TAB>(b0, kb, vb, eb, j0, sub, c4, n_keys);
        load_batch<TAB>(b1, kb, vb, eb, j0 + STRIDE, sub, c4, n_keys);
    }
    const float4 q4 = ld4(p.q + ((size_t)b * H + h) * HD + c4);
    __syncthreads();                                   // (the library's FOLD 5 prologue has this barrier too, for the decision's ids)
    float m = -INFINITY, l = 0.f;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#define CONSUME(bt) consume_batch<TAB>(bt, q4, j0, sub, c4, n_keys, s_tr, s_ta, s_root, s_attr, kv, tkk, tkv, m, l, o)
    CONSUME(b0);
    j0 += STRIDE;
    while (j0 < n_keys) {
        load_batch<TAB>(b0, kb, vb, eb, j0 + STRIDE, sub, c4, n_keys);
        __builtin_amdgcn_sched_barrier(0);
        CONSUME(b1);
        j0 += STRIDE;
        if (j0 >= n_keys) break;
        load_batch<TAB>(b1, kb, vb, eb, j0 + STRIDE, sub, c4, n_keys);
        __builtin_amdgcn_sched_barrier(0);
        CONSUME(b0);
        j0 += STRIDE;
    }
#undef CONSUME
#pragma unroll
    for (int off = LPK; off < 64; off <<= 1) {
        const float m2 = __shfl_xor(m, off, 64), l2 = __shfl_xor(l, off, 64);
        float4 o2;
        o2.x = __shfl_xor(o.x, off, 64); o2.y = __shfl_xor(o.y, off, 64);
        o2.z = __shfl_xor(o.z, off, 64); o2.w = __shfl_xor(o.w, off, 64);
        const float mn = fmaxf(m, m2);
        const float a1 = (m == -INFINITY) ? 0.f : __expf(m - mn);
        const float a2 = (m2 == -INFINITY) ? 0.f : __expf(m2 - mn);
        l = l * a1 + l2 * a2;
        o.x = o.x * a1 + o2.x * a2; o.y = o.y * a1 + o2.y * a2;
        o.z = o.z * a1 + o2.z * a2; o.w = o.w * a1 + o2.w * a2;
        m = mn;
    }
    if (sub == 0) {
        if (c4 == 0) { sm_m[wave] = m; sm_l[wave] = l; }
        *reinterpret_cast<float4*>(&sm_o[wave][c4]) = o;
    }
    __syncthreads();
    if (wave == 0 && sub == 0) {
        float mn = sm_m[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) mn = fmaxf(mn, sm_m[w]);
        float lt = 0.f;
        float4 ot = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float a = (sm_m[w] == -INFINITY) ? 0.f : __expf(sm_m[w] - mn);
            const float4 ow = ld4(&sm_o[w][c4]);
            lt += sm_l[w] * a;
            ot.x += ow.x * a; ot.y += ow.y * a; ot.z += ow.z * a; ot.w += ow.w * a;
        }
        const float inv = 1.0f / lt;
        ot.x *= inv; ot.y *= inv; ot.z *= inv; ot.w *= inv;
        *reinterpret_cast<float4*>(p.o + ((size_t)b * H + h) * HD + c4) = ot;
    }
}

// streams n4 float4 per thread through L2 (values discarded)
__global__ __launch_bounds__(256) void k_flush(const float4* __restrict__ x, int n4, float* sink) {
    const float4* xp = x + (size_t)blockIdx.x * n4 * 256 + threadIdx.x;
    float acc = 0.f;
    for (int i = 0; i < n4; ++i) acc += xp[(size_t)i * 256].x;
    if (acc == 123456.f) sink[0] = acc;
}

static double bench(std::function<void(hipStream_t, int)> body, int reps) {
    hipStream_t s; CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    body(s, 0); CK(hipStreamSynchronize(s));
    hipGraph_t g; hipGraphExec_t ge;
    CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < reps; ++i) body(s, i);
    CK(hipStreamEndCapture(s, &g));
    CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    CK(hipGraphLaunch(ge, s)); CK(hipStreamSynchronize(s));
    double best = 1e30;
    for (int r = 0; r < 3; ++r) {
        CK(hipEventRecord(a, s)); CK(hipGraphLaunch(ge, s)); CK(hipEventRecord(b, s)); CK(hipStreamSynchronize(s));
        float ms; CK(hipEventElapsedTime(&ms, a, b));
        if (ms * 1e3 / reps < best) best = ms * 1e3 / reps;
    }
    CK(hipGraphExecDestroy(ge)); CK(hipGraphDestroy(g)); CK(hipStreamDestroy(s));
    return best;
}

int main() {
    auto falloc = [](size_t n, float scale) {
        std::vector<float> hbuf(n);
        unsigned st = 12345u + (unsigned)n;
        for (auto& x : hbuf) { st = st * 1664525u + 1013904223u; x = ((float)(st >> 8) / 16777216.f - 0.5f) * scale; }
        float* p; CK(hipMalloc(&p, n * 4)); CK(hipMemcpy(p, hbuf.data(), n * 4, hipMemcpyHostToDevice)); return p;
    };
    constexpr int NC = 3;
    float *kc[NC], *vc[NC];
    for (int i = 0; i < NC; ++i) { kc[i] = falloc((size_t)B * H * CAP * HD, 1.f); vc[i] = falloc((size_t)B * H * CAP * HD, 1.f); }
    P p{};
    p.tab = falloc((size_t)H * T * 2 * HD, 1.f);
    p.tr = falloc((size_t)H * ROWS * 2 * HD, 1.f); p.ta = falloc((size_t)H * ROWS * 2 * HD, 1.f);
    p.tk = falloc((size_t)H * 2 * HD, 1.f); p.key = falloc(B, 1.f);
    p.Er = falloc((size_t)T * HD, 1.f); p.q = falloc((size_t)B * H * HD, 0.25f); p.o = falloc((size_t)B * H * HD, 0.f);
    std::vector<int64_t> ids((size_t)B * T);
    int64_t *roots, *attrs;
    CK(hipMalloc(&roots, ids.size() * 8)); CK(hipMalloc(&attrs, ids.size() * 8));
    for (size_t i = 0; i < ids.size(); ++i) ids[i] = (int64_t)((i * 2654435761u >> 7) % 15);
    CK(hipMemcpy(roots, ids.data(), ids.size() * 8, hipMemcpyHostToDevice));
    for (size_t i = 0; i < ids.size(); ++i) ids[i] = (int64_t)((i * 40503u >> 3) % 16);
    CK(hipMemcpy(attrs, ids.data(), ids.size() * 8, hipMemcpyHostToDevice));
    p.roots = roots; p.attrs = attrs;
    const size_t flush_bytes = (size_t)64 << 20;
    const int flush_wgs = 1024, flush_n4 = (int)(flush_bytes / 16 / 256 / flush_wgs);
    float* fl = falloc(flush_bytes / 4, 1.f);
    float* sink = falloc(64, 0.f);
    auto flush = [&](hipStream_t s) { hipLaunchKernelGGL(k_flush, dim3(flush_wgs), dim3(256), 0, s, reinterpret_cast<const float4*>(fl), flush_n4, sink); };
    const int reps = 60;
    const double t_flush = bench([&](hipStream_t s, int) { flush(s); }, reps);
    printf("flush launch alone (64 MB through L2): %.2f us; figures below are (flush + attention) - flush, best of 3 replays of %d pairs\n", t_flush, reps);
    printf("%-8s %-44s %-44s %-44s\n", "keys", "(a) per-clip cache, non-temporal", "(b) shared table + LDS rows, head per XCD", "(c) = (b), clips of a head over 8 XCDs");
    for (int n : {256, 512, 1023}) {
        p.n_keys = n;
        double r[3];
        for (int var = 0; var < 3; ++var) {
            r[var] = bench([&](hipStream_t s, int i) {
                P q = p;
                q.k = kc[i % NC]; q.v = vc[i % NC]; q.transposed = var == 2;
                flush(s);
                if (var == 0) hipLaunchKernelGGL(k_stream<false>, dim3(B * H), dim3(NW * 64), 0, s, q);
                else hipLaunchKernelGGL(k_stream<true>, dim3(B * H), dim3(NW * 64), 0, s, q);
            }, reps) - t_flush;
        }
        printf("%-8d %-44.2f %-44.2f %-44.2f\n", n, r[0], r[1], r[2]);
        fflush(stdout);
    }
    return 0;
}
