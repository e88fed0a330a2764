// Fused multi-tensor optimiser step: RAdam, RAdamW and the reference's RAdanW (model/RAdanW.py) in its two variants.
//
// One launch updates up to AMT_OPTIM_MAX_TENSORS tensors of a parameter group that share a step count: the parameter, exp_avg,
// exp_avg_sq, and under RAdanW exp_diff, exp_diff_sq, neg_prev_grad and the gradient itself (both variants write into it).  The
// pointer table travels in the kernel arguments (the gradients of a training loop are new allocations every step, so a table in
// device memory would need a copy and an event per step); nothing is staged, nothing waits on the host.
//
// The work is cut into chunks of OPT_CHUNK elements, numbered tensor after tensor; a block walks the chunks blockIdx.x,
// blockIdx.x + gridDim.x, ... and finds a chunk's tensor in the prefix sums of the table (uniform per block: scalar loads and
// compares).  Inside a chunk every lane moves 16 bytes per stream per pass; the numel % 4 elements behind the last whole float4 go
// through the same per-element function on the first lanes of the block that owns the tensor's last chunk.  An element's
// arithmetic depends on its values and the step's scalars alone, so the bits depend neither on the grid nor on how tensors are
// batched into launches.  No LDS, no atomics, no communication between blocks.
//
// Every step-dependent scalar (bias corrections, rho_t, the rectification factor, 1 - lr wd, the step sizes) is formed on the host
// in double as torch's / the reference's Python forms it and arrives as a float, the value torch's foreach kernels read a Python
// scalar as; the kernel has no pow and one uniform flag for the rectified branch.  The file is built with -ffp-contract=off: each
// product and sum below is rounded once, in the order the foreach (or single-tensor) code applies its operators.
#include "../../include/amt_hip.h"
#include "amt_common.h"

namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_VEC_PER_LANE = 4;                                     // float4 per lane per stream per chunk
constexpr int OPT_CHUNK = OPT_THREADS * OPT_VEC_PER_LANE * 4;           // 4096 elements
constexpr int OPT_MAX_BLOCKS = 2048;                                    // 256 CUs x 8 blocks: the rest is grid-strided

struct OptTable {
    float* p[AMT_OPTIM_MAX_TENSORS];
    float* g[AMT_OPTIM_MAX_TENSORS];
    float* m[AMT_OPTIM_MAX_TENSORS];
    float* v[AMT_OPTIM_MAX_TENSORS];
    float* ed[AMT_OPTIM_MAX_TENSORS];
    float* eds[AMT_OPTIM_MAX_TENSORS];
    float* npg[AMT_OPTIM_MAX_TENSORS];
    int64_t numel[AMT_OPTIM_MAX_TENSORS];
    int32_t chunk0[AMT_OPTIM_MAX_TENSORS + 1];      // first chunk of tensor t; [n] = the launch's chunk count
    int32_t n;
};

struct OptScalars {
    float decay, wd, w1, beta2, omb2, eps;
    float rect_step, unrect_step;                   // foreach form: -(sqrt(bc2) lr rect / bc1), -(lr / bc1)
    float bc1, lr, bc2_sqrt, rect;                  // single-tensor form
    float beta3, omb3, neg_omb3, beta4, omb4;
    int32_t rectified, npg_from_grad;
};

struct Elem {
    float p, g, m, v, ed, eds, npg;
};

// torch's lerp for a weight below 0.5
__device__ __forceinline__ float lerp_lo(float a, float b, float w) { return a + w * (b - a); }

template <int MODE>
__device__ __forceinline__ void update(Elem& e, const OptScalars& s) {
    constexpr bool ADAN = MODE == AMT_OPTIM_RADANW_FOREACH || MODE == AMT_OPTIM_RADANW_SINGLE;
    float g = e.g;
    if (MODE != AMT_OPTIM_RADAM) e.p = e.p * s.decay;
    else if (s.wd != 0.f) g = g + s.wd * e.p;
    e.m = lerp_lo(e.m, g, s.w1);
    e.v = e.v * s.beta2;
    e.v = e.v + (s.omb2 * g) * g;
    if (MODE == AMT_OPTIM_RADANW_SINGLE) {          // RAdanW.py:274-300
        float t = (e.m / s.bc1) * s.lr;
        if (s.rectified) {
            t = t * (s.bc2_sqrt / (sqrtf(e.v) + s.eps));
            t = t * s.rect;
        }
        e.p = e.p - t;
    } else {                                        // the foreach form of torch's RAdam and of RAdanW.py:408-415
        float buf = s.unrect_step;
        if (s.rectified) buf = 1.f / ((sqrtf(e.v) + s.eps) / s.rect_step);
        e.p = e.p + e.m * buf;
    }
    if (ADAN) {
        const float d = (s.npg_from_grad ? -e.g : e.npg) + e.g;         // g_t - g_(t-1)
        if (MODE == AMT_OPTIM_RADANW_FOREACH) {     // RAdanW.py:418-444
            e.ed = e.ed * s.beta3 + d * s.omb3;
            const float buf = d * s.omb3;
            e.g = e.g + buf;
            e.eds = e.eds * s.beta4 + (buf * buf) * s.omb4;
            const float eta = s.lr / (sqrtf(e.eds) + s.eps);
            e.p = e.p + ((e.ed * eta) * s.neg_omb3) * s.decay;
            e.npg = 0.f + e.g * -1.0f;
        } else {                                    // RAdanW.py:303-317
            e.ed = e.ed * s.beta3 + s.omb3 * d;
            const float gn = e.g + s.omb3 * d;
            e.g = gn * gn;
            e.eds = e.eds * s.beta4 + s.omb4 * e.g;
            const float eta = s.lr / (sqrtf(e.eds) + s.eps);
            e.ed = e.ed * eta;
            e.p = e.p + s.neg_omb3 * e.ed;
            e.npg = 0.f + -1.0f * e.g;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(OPT_THREADS) void optim_step_kernel(const OptTable tab, const OptScalars s) {
    constexpr bool ADAN = MODE == AMT_OPTIM_RADANW_FOREACH || MODE == AMT_OPTIM_RADANW_SINGLE;
    const int n_chunks = tab.chunk0[tab.n];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        int t = 0;
        while (tab.chunk0[t + 1] <= c) ++t;                             // t < tab.n: c < chunk0[n]
        const int64_t numel = tab.numel[t];
        const int64_t n4 = numel >> 2;
        const int64_t base4 = (int64_t)(c - tab.chunk0[t]) * (OPT_CHUNK / 4);
        float4* __restrict__ p4 = reinterpret_cast<float4*>(tab.p[t]);
        float4* __restrict__ g4 = reinterpret_cast<float4*>(tab.g[t]);
        float4* __restrict__ m4 = reinterpret_cast<float4*>(tab.m[t]);
        float4* __restrict__ v4 = reinterpret_cast<float4*>(tab.v[t]);
        float4* __restrict__ ed4 = ADAN ? reinterpret_cast<float4*>(tab.ed[t]) : nullptr;
        float4* __restrict__ eds4 = ADAN ? reinterpret_cast<float4*>(tab.eds[t]) : nullptr;
        float4* __restrict__ npg4 = ADAN ? reinterpret_cast<float4*>(tab.npg[t]) : nullptr;
#pragma unroll
        for (int k = 0; k < OPT_VEC_PER_LANE; ++k) {
            const int64_t i = base4 + k * OPT_THREADS + threadIdx.x;
            if (i >= n4) continue;
            float4 P = p4[i], G = g4[i], M = m4[i], V = v4[i], ED, EDS, NPG;
            if (ADAN) {
                ED = ed4[i];
                EDS = eds4[i];
                if (!s.npg_from_grad) NPG = npg4[i];
                else NPG = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            float* Pf = &P.x; float* Gf = &G.x; float* Mf = &M.x; float* Vf = &V.x;
            float* EDf = &ED.x; float* EDSf = &EDS.x; float* NPGf = &NPG.x;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                Elem e{Pf[j], Gf[j], Mf[j], Vf[j], ADAN ? EDf[j] : 0.f, ADAN ? EDSf[j] : 0.f, ADAN ? NPGf[j] : 0.f};
                update<MODE>(e, s);
                Pf[j] = e.p; Mf[j] = e.m; Vf[j] = e.v;
                if (ADAN) { Gf[j] = e.g; EDf[j] = e.ed; EDSf[j] = e.eds; NPGf[j] = e.npg; }
            }
            p4[i] = P; m4[i] = M; v4[i] = V;
            if (ADAN) { g4[i] = G; ed4[i] = ED; eds4[i] = EDS; npg4[i] = NPG; }
        }
        // the numel % 4 elements behind the last float4: the block that owns the tensor's last chunk, one lane each
        const int64_t tail = (n4 << 2) + threadIdx.x;
        if (c + 1 == tab.chunk0[t + 1] && tail < numel) {
            Elem e{tab.p[t][tail], tab.g[t][tail], tab.m[t][tail], tab.v[t][tail], 0.f, 0.f, 0.f};
            if (ADAN) {
                e.ed = tab.ed[t][tail];
                e.eds = tab.eds[t][tail];
                if (!s.npg_from_grad) e.npg = tab.npg[t][tail];
            }
            update<MODE>(e, s);
            tab.p[t][tail] = e.p; tab.m[t][tail] = e.m; tab.v[t][tail] = e.v;
            if (ADAN) { tab.g[t][tail] = e.g; tab.ed[t][tail] = e.ed; tab.eds[t][tail] = e.eds; tab.npg[t][tail] = e.npg; }
        }
    }
}

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

}  // namespace

extern "C" int32_t amt_optim_plan(int32_t what) {
    switch (what) {
        case AMT_OPTIM_PLAN_MAX_TENSORS: return AMT_OPTIM_MAX_TENSORS;
        case AMT_OPTIM_PLAN_CHUNK: return OPT_CHUNK;
        case AMT_OPTIM_PLAN_MAX_BLOCKS: return OPT_MAX_BLOCKS;
        case AMT_OPTIM_PLAN_THREADS: return OPT_THREADS;
        default: return -1;
    }
}

extern "C" int32_t amt_optim_step(const amt_optim_args* a, void* stream) {
    AMT_CHECK_ARG(a, "amt_optim_step: null argument struct");
    const int mode = a->mode;
    AMT_CHECK_ARG(mode >= AMT_OPTIM_RADAM && mode <= AMT_OPTIM_RADANW_SINGLE, "amt_optim_step: mode %d", mode);
    const bool adan = mode == AMT_OPTIM_RADANW_FOREACH || mode == AMT_OPTIM_RADANW_SINGLE;
    AMT_CHECK_ARG(a->n_tensors >= 1 && a->n_tensors <= AMT_OPTIM_MAX_TENSORS, "amt_optim_step: n_tensors=%d (1..%d per launch)", a->n_tensors,
                  AMT_OPTIM_MAX_TENSORS);
    AMT_CHECK_ARG(a->p && a->g && a->m && a->v && a->numel, "amt_optim_step: null pointer table");
    AMT_CHECK_ARG(!adan || (a->ed && a->eds && a->npg), "amt_optim_step: RAdanW needs exp_diff, exp_diff_sq and neg_prev_grad");
    OptTable tab;
    tab.n = a->n_tensors;
    int64_t chunks = 0;
    for (int t = 0; t < AMT_OPTIM_MAX_TENSORS; ++t) {
        const bool live = t < a->n_tensors;
        tab.p[t] = live ? a->p[t] : nullptr;
        tab.g[t] = live ? a->g[t] : nullptr;
        tab.m[t] = live ? a->m[t] : nullptr;
        tab.v[t] = live ? a->v[t] : nullptr;
        tab.ed[t] = live && adan ? a->ed[t] : nullptr;
        tab.eds[t] = live && adan ? a->eds[t] : nullptr;
        tab.npg[t] = live && adan ? a->npg[t] : nullptr;
        tab.numel[t] = live ? a->numel[t] : 0;
        tab.chunk0[t] = (int32_t)chunks;
        if (!live) continue;
        AMT_CHECK_ARG(a->numel[t] > 0, "amt_optim_step: tensor %d has %lld elements", t, (long long)a->numel[t]);
        AMT_CHECK_ARG(tab.p[t] && tab.g[t] && tab.m[t] && tab.v[t] && (!adan || (tab.ed[t] && tab.eds[t] && tab.npg[t])),
                      "amt_optim_step: tensor %d: null pointer", t);
        AMT_CHECK_ARG(aligned16(tab.p[t]) && aligned16(tab.g[t]) && aligned16(tab.m[t]) && aligned16(tab.v[t]) && aligned16(tab.ed[t]) &&
                          aligned16(tab.eds[t]) && aligned16(tab.npg[t]),
                      "amt_optim_step: tensor %d is not 16-byte aligned", t);
        chunks += (a->numel[t] + OPT_CHUNK - 1) / OPT_CHUNK;
        AMT_CHECK_ARG(chunks <= 0x7fffffff, "amt_optim_step: %lld chunks in one launch", (long long)chunks);
    }
    tab.chunk0[AMT_OPTIM_MAX_TENSORS] = (int32_t)chunks;
    for (int t = a->n_tensors; t <= AMT_OPTIM_MAX_TENSORS; ++t) tab.chunk0[t] = (int32_t)chunks;
    OptScalars s;
    s.decay = a->decay; s.wd = a->weight_decay; s.w1 = a->one_minus_beta1; s.beta2 = a->beta2; s.omb2 = a->one_minus_beta2; s.eps = a->eps;
    s.rect_step = a->rect_step_size; s.unrect_step = a->unrect_step_size;
    s.bc1 = a->bias_correction1; s.lr = a->lr; s.bc2_sqrt = a->bias_correction2_sqrt; s.rect = a->rect;
    s.beta3 = a->beta3; s.omb3 = a->one_minus_beta3; s.neg_omb3 = a->neg_one_minus_beta3; s.beta4 = a->beta4; s.omb4 = a->one_minus_beta4;
    s.rectified = a->rectified != 0; s.npg_from_grad = a->npg_from_grad != 0;
    const dim3 grid((unsigned)(chunks < OPT_MAX_BLOCKS ? chunks : OPT_MAX_BLOCKS)), block(OPT_THREADS);
    hipStream_t st = (hipStream_t)stream;
    switch (mode) {
        case AMT_OPTIM_RADAM: hipLaunchKernelGGL(optim_step_kernel<AMT_OPTIM_RADAM>, grid, block, 0, st, tab, s); break;
        case AMT_OPTIM_RADAMW: hipLaunchKernelGGL(optim_step_kernel<AMT_OPTIM_RADAMW>, grid, block, 0, st, tab, s); break;
        case AMT_OPTIM_RADANW_FOREACH: hipLaunchKernelGGL(optim_step_kernel<AMT_OPTIM_RADANW_FOREACH>, grid, block, 0, st, tab, s); break;
        default: hipLaunchKernelGGL(optim_step_kernel<AMT_OPTIM_RADANW_SINGLE>, grid, block, 0, st, tab, s); break;
    }
    AMT_LAUNCH_CHECK();
    return 0;
}
