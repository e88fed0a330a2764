// C-ABI layer of libamt_hip, handle half: model handle, weight loading / repacking, encoder / prefill / decode
// orchestration (hipGraph-captured decode step).  The stateless operator entry points live in ops_api.hip.
// See include/amt_hip.h for the contract and the reference code each entry point replaces.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/amt_hip.h"
#include "amt_common.h"
#include "kernels.h"

// ------------------------------------------------------------------------------------------------
// error channel
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";

void amt_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* amt_last_error(void) { return g_err; }
extern "C" int32_t amt_abi_version(void) { return AMT_ABI_VERSION; }

// ------------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int V = 159;
constexpr float LN_EPS = 1e-5f;
constexpr int VS = 160;                  // V rounded up to the skinny GEMM's 16-column tiles
constexpr int FFN_CHUNK = 1024;          // column range of linear2 per skinny-GEMM launch when dim_feedforward > 1536

struct Tensor {
    float* p = nullptr;
    std::vector<int64_t> shape;
    size_t numel() const { size_t n = 1; for (auto s : shape) n *= (size_t)s; return n; }
};

struct DecLayer {   // raw + packed weights of one decoder layer
    const float *sa_w, *sa_b, *Er, *sa_ow, *sa_ob, *ca_w, *ca_b, *ca_ow, *ca_ob, *l1w, *l1b, *l2w, *l2b;
    const float *n1w, *n1b, *n2w, *n2b, *n3w, *n3b;
    float *p_sa, *p_sao, *p_caq, *p_cao, *p_l1, *p_l2;   // MFMA-ordered copies for the decode step
    // LayerNorm folded through the following projection (fold.hip): packed [Wc | W'] and the vectors g | c | dv
    //   a: norm1 -> cross-attention query        (N = d,   K = d + d)
    //   b: norm2 -> linear1                       (N = dff, K = d + d)
    //   c: norm3 -> next layer's self-attn in-proj (N = 3d, K = dff + d), absent in the last layer
    float *pf_a, *pf_b, *pf_c, *va, *vb, *vc;
};
struct EncLayer {
    const float *sa_w, *sa_b, *sa_ow, *sa_ob, *l1w, *l1b, *l2w, *l2b, *n1w, *n1b, *n2w, *n2b;
};

}  // namespace

struct amt_handle {
    amt_config cfg{};
    int d = 0, H = 0, hd = 0, dff = 0, nl = 0, Scap = 0, Tcap = 0, F = 0, Fpad = 0, maxB = 0;
    std::map<std::string, Tensor> w;
    std::vector<void*> owned;            // every hipMalloc of the handle
    bool finalized = false;
    std::vector<DecLayer> dec;
    std::vector<EncLayer> enc;
    // derived tensors
    float *Wvis_pad = nullptr, *Wc_main = nullptr, *wkey = nullptr, *PR = nullptr, *PA = nullptr;
    const float *pe = nullptr, *pe_v = nullptr;
    // encoder state of the last amt_encode
    int encB = 0, encS = 0;
    float* KVx = nullptr;                // [2][nl][maxB][H][kx_rows][hd]
    size_t kvx_layer = 0, kvx_part = 0;
    float* memory = nullptr;             // [maxB*Scap][d]
    // shared big workspaces (rows = maxB * max(Scap, Tcap))
    size_t ws_rows = 0;
    float *wsX = nullptr, *wsU = nullptr, *wsQKV = nullptr, *wsO = nullptr, *wsH = nullptr, *wsA0 = nullptr, *wsQc = nullptr;
    // decode state
    float* KVc = nullptr;                // [2][nl][maxB][H][kv_rows][hd]
    size_t kvc_layer = 0, kvc_part = 0;
    // rows per (clip, head) of the self-attention cache: Tcap made odd.  With Tcap = 1024 rows of 256 B the heads lie exactly
    // 256 KiB apart and the 256 workgroups of a decode-attention launch, which all stream the same row range at the same time,
    // camp on the same HBM channels: one padding row de-aliases them (in-kernel timeline of the step at t = 1023: 342 -> 309 us)
    int kv_rows = 0, kx_rows = 0;     // (kx_rows: the same for the cross-attention K/V, Scap rows per head)
    float *x_in = nullptr, *u1 = nullptr, *u2 = nullptr, *u3 = nullptr, *xa = nullptr, *xb = nullptr, *xc = nullptr;
    float *qb = nullptr, *ob = nullptr, *hb = nullptr, *keyb = nullptr;
    bool fold = false;                   // decode chain with folded LayerNorms (5 kernels per layer instead of 8)
    float *qraw = nullptr, *hraw = nullptr, *qkvraw = nullptr;          // raw projections of the un-normalised sums
    float *tWs = nullptr, *tT = nullptr, *tWc = nullptr, *tComb = nullptr, *tWs2 = nullptr;   // load-time scratch of build_fold
    // folded output head: packed [W''.W2 | W''] (W'' = Wout o g3 o gf), vectors h1|h2|dv|h3|h4|- (VS floats each), raw logits
    float *pf_s = nullptr, *vs = nullptr, *lraw = nullptr;
    // layer-0 q/k/v as table sums: rows of (root, attr, key column, position) projected through layer 0's in-proj
    float *tab_r = nullptr, *tab_a = nullptr, *tab_k = nullptr, *tab_p = nullptr, *tab_cb = nullptr;
    // their k / v columns again, sliced by head (pure copies, rebuilt with them): tab_p0 [H][Tcap][k hd | v hd], tab_ra0 [H][n_root + 16][k hd | v hd]
    float *tab_p0 = nullptr, *tab_ra0 = nullptr;
    int* pos = nullptr;
    float* unif = nullptr;               // [Tcap][maxB] uniforms of the device-side categorical draw (amt_generate_set_uniforms)
    int use_unif = 0;
    int64_t *tokens = nullptr, *roots = nullptr, *attrs = nullptr;   // [maxB][Tcap]
    // current generation
    int genB = 0, genT = 0, genP = 0, beam = 0, mcN = 0, mcC = 2, steps_done = 0;
    int n_root = 15;                     // rows of the "root" input table: 15 chord roots, or the chord-embedding table's rows (chord_embed)
    bool chord_embed = false;            // amt_set_option("chord_embed"): the chord id is the input index and feeds back
    bool causal_mask = true;             // amt_set_option("causal_mask"): 0 = the forward without the subsequent mask (mask=False)
    const float* vis_resid = nullptr;    // amt_encode_resid: rows added to Linear_vis's output (scene_embed)
    int skip_mask = 0;                   // amt_set_option("profile_skip"): measurement ablation, 1 = no self-attention launches, 2 = no cross-attention launches
    bool fuse_head = true;               // amt_set_option("fuse_sampling_head"): inside a captured graph the head rides in the next step's first attention
    bool short_attn = true;              // amt_set_option("short_context_attn"): graphs whose every step fits one K/V batch use the short-context self-attention
    bool step_short = false;             // set by get_graph while it captures such a graph (eager steps keep the long kernels)
    bool l0_tables = true;               // amt_set_option("layer0_kv_from_tables"): 0 = the attention that carries the sampling head streams layer 0's keys from the cache
    bool gemm_pipe = true;               // amt_set_option("gemm_tile_pipeline"): 0 = the skinny GEMMs of the decode step run the serial tile loop (DecodeGemmParams::serial_loop)
    bool gemm_lean = true;               // amt_set_option("gemm_scalar_front"): 0 = the skinny GEMMs of the decode step keep their generic front (DecodeGemmParams::generic_front)
    bool rows_dma = AMT_GEMM_ROWS_DMA_DEFAULT != 0;      // amt_set_option("gemm_rows_dma"): 0 = the skinny GEMMs of the decode step stage their rows through registers (DecodeGemmParams::reg_rows)
    bool scalar_stream = true;           // amt_set_option("scalar_key_stream"): 0 = the decode attentions keep the per-lane controlled key stream (AttnDecodeParams::lane_key_stream)
    bool plain_chain = false;            // amt_set_option("decode_chain_plain"), before the first amt_finalize: the 49-launch chain without folded LayerNorms
    bool gen_active = false;
    // graphs keyed by the parameters baked into the captured kernel arguments
    struct GraphKey { int B, T, P, beam, mcN, mcC, S, nsteps, skip, pad, short_ctx, parity, gemm_pipe, spare, key_stream, gemm_front, gemm_rows, spare2; float* logits; };      // (compared bytewise: an even number of ints, no padding)
    struct GraphEntry { GraphKey key; hipGraphExec_t exec; hipGraph_t graph; };
    std::vector<GraphEntry> graphs;
    hipStream_t cap_stream = nullptr;    // capture-only stream (the caller's may be the legacy null stream)
};

namespace {

template <typename T>
int32_t dev_alloc(amt_handle* h, T** out, size_t count) {
    void* p = nullptr;
    AMT_HIP(hipMalloc(&p, count * sizeof(T) + 256));
    h->owned.push_back(p);
    *out = (T*)p;
    return 0;
}

const float* W(amt_handle* h, const std::string& name) {
    auto it = h->w.find(name);
    return it == h->w.end() ? nullptr : it->second.p;
}

int32_t need(amt_handle* h, const std::string& name, std::initializer_list<int64_t> shape, const float** out) {
    auto it = h->w.find(name);
    AMT_CHECK_ARG(it != h->w.end(), "weight '%s' was not loaded", name.c_str());
    std::vector<int64_t> want(shape);
    if (it->second.shape != want) {
        std::string got, exp;
        for (auto s : it->second.shape) got += std::to_string(s) + ",";
        for (auto s : want) exp += std::to_string(s) + ",";
        AMT_CHECK_ARG(false, "weight '%s' has shape (%s) but the config needs (%s)", name.c_str(), got.c_str(), exp.c_str());
    }
    *out = it->second.p;
    return 0;
}

int32_t pack(amt_handle* h, const float* w, int N, int K, float** out, hipStream_t s) {
    if (!*out) {                         // re-finalize after a weight reload repacks into the same buffer,
        int32_t rc = dev_alloc(h, out, (size_t)cdiv(N, 16) * 16 * K);   // so captured graphs stay valid
        if (rc) return rc;
    }
    return amt_launch_pack_weight(w, *out, N, K, s);
}

// Folds LayerNorm(gamma, beta) of u = A.Wo^T + bo + r through y = LN(u).W^T + b (see fold.hip):
// packed <- [W'.Wo | W'] (N x (Kin + d)), vec <- g | c | dv (3N floats).  W: [N][d], Wo: [d][Kin].
int32_t build_fold(amt_handle* h, const float* Wm, int N, const float* gamma, const float* beta, const float* b,
                   const float* Wo, int Kin, const float* bo, float** packed, float** vec, hipStream_t s) {
    const int d = h->d;
    int32_t rc;
    if (!*vec && (rc = dev_alloc(h, vec, (size_t)3 * N))) return rc;
    if ((rc = amt_launch_scale_cols(Wm, gamma, h->tWs, N, d, s))) return rc;
    if ((rc = amt_launch_transpose(Wo, h->tT, d, Kin, s))) return rc;                       // [Kin][d]
    if ((rc = amt_launch_gemm(gemm_params(h->tWs, d, h->tT, d, h->tWc, Kin, N, Kin, d, nullptr), s))) return rc;
    const size_t ld = (size_t)(Kin + d) * sizeof(float);
    AMT_HIP(hipMemcpy2DAsync(h->tComb, ld, h->tWc, (size_t)Kin * sizeof(float), (size_t)Kin * sizeof(float), N, hipMemcpyDeviceToDevice, s));
    AMT_HIP(hipMemcpy2DAsync(h->tComb + Kin, ld, h->tWs, (size_t)d * sizeof(float), (size_t)d * sizeof(float), N, hipMemcpyDeviceToDevice, s));
    if ((rc = pack(h, h->tComb, N, Kin + d, packed, s))) return rc;
    return amt_launch_fold_vectors(Wm, h->tWs, beta, b, bo, *vec, *vec + N, *vec + 2 * N, N, d, s);
}

int32_t ensure_workspace(amt_handle* h) {
    if (h->wsX) return 0;
    const size_t R = h->ws_rows;
    int32_t rc;
    if ((rc = dev_alloc(h, &h->wsX, R * h->d))) return rc;
    if ((rc = dev_alloc(h, &h->wsU, R * h->d))) return rc;
    if ((rc = dev_alloc(h, &h->wsO, R * h->d))) return rc;
    if ((rc = dev_alloc(h, &h->wsQc, R * h->d))) return rc;
    if ((rc = dev_alloc(h, &h->wsQKV, R * 3 * h->d))) return rc;
    if ((rc = dev_alloc(h, &h->wsH, R * h->dff))) return rc;
    if ((rc = dev_alloc(h, &h->wsA0, (size_t)h->maxB * h->Scap * h->Fpad))) return rc;
    return 0;
}

// one decoder/encoder sub-block on [rows][d] activations: U = Linear(O) + resid ; X = LN(U)
int32_t proj_resid_ln(amt_handle* h, const float* in, int K, const float* w, const float* b, const float* resid,
                      const float* nw, const float* nb, const float* n2w, const float* n2b, float* U, float* Xout,
                      int rows, hipStream_t s) {
    GemmParams g = gemm_params(in, K, w, K, U, h->d, rows, h->d, K, b);
    g.resid = resid; g.ldr = h->d;
    int32_t rc = amt_launch_gemm(g, s);
    if (rc) return rc;
    return amt_launch_layernorm(U, nullptr, nw, nb, n2w, n2b, Xout, rows, h->d, LN_EPS, s);
}

int32_t ffn_block(amt_handle* h, float* X, const float* l1w, const float* l1b, const float* l2w, const float* l2b,
                  const float* nw, const float* nb, const float* n2w, const float* n2b, float* Xout, int rows, hipStream_t s) {
    GemmParams g = gemm_params(X, h->d, l1w, h->d, h->wsH, h->dff, rows, h->dff, h->d, l1b);
    g.relu = 1;
    int32_t rc = amt_launch_gemm(g, s);
    if (rc) return rc;
    return proj_resid_ln(h, h->wsH, h->dff, l2w, l2b, X, nw, nb, n2w, n2b, h->wsU, Xout, rows, s);
}

// the device-side position pair: the kernels of the step that processes position `step` read slot step & 1 (SampleParams::pos)
int* pos_slot(amt_handle* h, int step) { return h->pos + (step & 1); }

// the head that closes the step processing position `step`
SampleParams sample_params(amt_handle* h, float* logits_out, float* probs_out, int external, int step) {
    SampleParams p{};
    const DecLayer& L = h->dec.back();
    p.u = h->u3; p.ldu = h->d;
    p.ln_w = L.n3w; p.ln_b = L.n3b;
    p.fn_w = W(h, "transformer.decoder.norm.weight"); p.fn_b = W(h, "transformer.decoder.norm.bias");
    p.Wout = W(h, "Wout.weight"); p.bout = W(h, "Wout.bias");
    p.eps = LN_EPS; p.B = h->genB; p.d = h->d;
    p.tokens = h->tokens; p.roots = h->roots; p.attrs = h->attrs; p.T = h->genT;
    p.pos = pos_slot(h, step); p.pos_next = pos_slot(h, step + 1); p.n_primer = h->genP; p.beam = h->beam;
    p.max_conseq_N = h->mcN; p.max_conseq_chord = h->mcC;
    p.logits_out = logits_out; p.probs_out = probs_out;
    p.key = h->keyb; p.PR = h->PR; p.PA = h->PA; p.wkey = h->wkey; p.cbias = W(h, "Linear_chord.bias"); p.pe = h->pe;
    p.x_next = h->x_in; p.sample_external = external; p.chord_embed = h->chord_embed ? 1 : 0;
    p.uniforms = h->use_unif ? h->unif : nullptr;
    if (h->fold) {
        p.lraw = h->lraw; p.ld_lraw = VS; p.h1 = h->vs; p.h2 = h->vs + VS; p.h3 = h->vs + 3 * VS; p.h4 = h->vs + 4 * VS;
        p.tab_r = h->tab_r; p.tab_a = h->tab_a; p.tab_k = h->tab_k; p.tab_p = h->tab_p;
        p.q0 = h->qb; p.kc0 = h->KVc; p.vc0 = h->KVc + h->kvc_part; p.H = h->H; p.hd = h->hd; p.cap = h->kv_rows;
        p.q_scale = 1.0f / sqrtf((float)h->hd);
        p.tab_p0 = h->tab_p0; p.tab_ra0 = h->tab_ra0; p.tab_T = h->Tcap; p.n_root = h->n_root;
    }
    return p;
}

// Optional per-launch timing of an eagerly issued step (bench.py's roofline leg): HIP events are
// recorded on the launch stream right before / after each kernel, classes: 0 = relative-position
// self-attention, 1 = cross-attention, 2 = skinny GEMMs, 3 = sampling head.
struct StepProf {
    std::vector<hipEvent_t> ev;
    std::vector<int> cls;
    size_t used = 0;
    hipStream_t s = nullptr;
    void begin() {
        if (used + 2 > ev.size()) { ev.resize(used + 2, nullptr); (void)hipEventCreate(&ev[used]); (void)hipEventCreate(&ev[used + 1]); }
        (void)hipEventRecord(ev[used], s);
    }
    void end(int c) { (void)hipEventRecord(ev[used + 1], s); cls.push_back(c); used += 2; }
};
#define PROF_BEGIN() do { if (prof) prof->begin(); } while (0)
#define PROF_END(c) do { if (prof) prof->end(c); } while (0)

// every skinny GEMM of a decode step goes through here: the handle's choice of tile loop and of front rides in the parameters
int32_t launch_step_gemm(const amt_handle* h, DecodeGemmParams g, hipStream_t s) {
    g.serial_loop = h->gemm_pipe ? 0 : 1;
    g.generic_front = h->gemm_lean ? 0 : 1;
    g.reg_rows = h->rows_dma ? -1 : 1;
    return amt_launch_decode_gemm(g, s);
}

// One decode step with every LayerNorm folded through the projection behind it (fold.hip): per layer
//   SA  self-attention; layers > 0 finish norm3 of the previous layer in the prologue (q, new k/v, residual row)
//   G1  [u1 | q_raw]   = [o | r] . [Wo | Wc_a,W'_a]      out-proj + residual, and the raw cross-attention query
//   CA  cross-attention, norm1 finished in the prologue
//   G2  [u2 | h_raw]   = [o | x1] . [Wo | Wc_b,W'_b]     out-proj + residual, and the raw FFN-up activations
//   G3  [u3 | qkv_raw] = [relu(norm2-fix(h_raw)) | x2] . [W2 | Wc_c,W'_c]   FFN-down + residual, next layer's raw QKV
// 5 dependent kernels per layer instead of 8.  Layer 0's q/k/v are table sums written by the sampling head (its input is
// a sum of embedding-table rows), the last G3 also emits the raw logits, so a step is 6*5 + 1 = 31 launches.
// fused_sp (captured graphs, round 3): layer 0's self-attention takes the PREVIOUS step's sampling decision in its prologue
// (attn_decode_sample_kernel) -- the step then needs no sampling-head launch in front of it: 30 launches.  That launch reads the
// previous step's slot of the position pair and fills this step's, which the other 29 read.
int32_t enqueue_decoder_step_folded(amt_handle* h, hipStream_t s, int step, StepProf* prof, const SampleParams* fused_sp = nullptr) {
    const int B = h->genB, d = h->d, dff = h->dff, H = h->H, hd = h->hd;
    const float qscale = 1.0f / sqrtf((float)hd);
    int32_t rc;
    for (int l = 0; l < h->nl; ++l) {
        const DecLayer& L = h->dec[l];
        float* Kc = h->KVc + (size_t)l * h->kvc_layer;
        float* Vc = Kc + h->kvc_part;
        const float* Kx = h->KVx + (size_t)l * h->kvx_layer;
        const float* Vx = Kx + h->kvx_part;
        AttnDecodeParams a{};
        a.k = Kc; a.v = Vc; a.o = h->ob; a.B = B; a.H = H; a.hd = hd; a.cap = h->kv_rows;
        a.pos = l == 0 && fused_sp ? fused_sp->pos : pos_slot(h, step); a.Er = L.Er; a.er_len = h->Tcap; a.short_ctx = h->step_short; a.lane_key_stream = h->scalar_stream ? 0 : 1;
        if (l == 0 && fused_sp) {
            a.k_new = Kc; a.v_new = Vc; a.new_kv = 1;      // q / k / v of the new position are summed from the projected tables in the kernel
            // ... and, in the long graphs, the keys of the earlier positions too (shapes the kernel does not stage keep the cache stream)
            a.l0_tables = h->l0_tables && !h->chord_embed && amt_attn_decode_tables_fit(hd, h->kv_rows, h->n_root + 16);
        } else if (l == 0) {
            a.q = h->qb;          // written, with this position's K/V rows, by the previous sampling head / embed_step (table sums)
        } else {
            const DecLayer& P = h->dec[l - 1];
            a.q = h->qkvraw; a.ldq = 3 * d; a.d = d; a.fold_u = h->u3; a.fold_g = P.vc; a.fold_c = P.vc + 3 * d;
            a.fold_lnw = P.n3w; a.fold_lnb = P.n3b; a.xn = h->xa; a.new_kv = 1; a.k_new = Kc; a.v_new = Vc;
            a.eps = LN_EPS; a.q_scale = qscale;
        }
        if (l == 0 && fused_sp) {
            if ((rc = amt_launch_attn_decode_sample(a, *fused_sp, s))) return rc;
        } else if (!(h->skip_mask & 1)) {
            PROF_BEGIN();
            if ((rc = amt_launch_attn_decode(a, s))) return rc;
            PROF_END(0);
        }
        const float* r0 = l == 0 ? h->x_in : h->xa;
        DecodeGemmParams g1{};
        g1.B = B; g1.eps = LN_EPS; g1.scale = 1.f; g1.x = h->ob; g1.ldx = d; g1.x2 = r0; g1.ldx2 = d; g1.K1 = d; g1.K = 2 * d;
        g1.Wp = L.p_sao; g1.bias = L.sa_ob; g1.resid = r0; g1.ldr = d; g1.y = h->u1; g1.ldy = d;
        g1.n_split = d; g1.N = 2 * d; g1.Wp2 = L.pf_a; g1.bias2 = L.va + 2 * d; g1.y2 = h->qraw; g1.ldy2 = d;
        PROF_BEGIN();
        if ((rc = launch_step_gemm(h, g1, s))) return rc;
        PROF_END(2);
        AttnDecodeParams x{};
        x.k = Kx; x.v = Vx; x.o = h->ob; x.B = B; x.H = H; x.hd = hd; x.cap = h->kx_rows; x.n_keys = h->encS; x.lane_key_stream = h->scalar_stream ? 0 : 1;
        x.q = h->qraw; x.ldq = d; x.d = d; x.fold_u = h->u1; x.fold_g = L.va; x.fold_c = L.va + d;
        x.fold_lnw = L.n1w; x.fold_lnb = L.n1b; x.xn = h->xb; x.eps = LN_EPS; x.q_scale = qscale;
        if (!(h->skip_mask & 2)) {
            PROF_BEGIN();
            if ((rc = amt_launch_attn_decode(x, s))) return rc;
            PROF_END(1);
        }
        DecodeGemmParams g2{};
        g2.B = B; g2.eps = LN_EPS; g2.scale = 1.f; g2.x = h->ob; g2.ldx = d; g2.x2 = h->xb; g2.ldx2 = d; g2.K1 = d; g2.K = 2 * d;
        g2.Wp = L.p_cao; g2.bias = L.ca_ob; g2.resid = h->xb; g2.ldr = d; g2.y = h->u2; g2.ldy = d;
        g2.n_split = d; g2.N = d + dff; g2.Wp2 = L.pf_b; g2.bias2 = L.vb + 2 * dff; g2.y2 = h->hraw; g2.ldy2 = dff;
        PROF_BEGIN();
        if ((rc = launch_step_gemm(h, g2, s))) return rc;
        PROF_END(2);
        DecodeGemmParams g3{};
        g3.B = B; g3.eps = LN_EPS; g3.scale = 1.f; g3.pro = 1; g3.x = h->hraw; g3.ldx = dff; g3.x2 = h->u2; g3.ldx2 = d;
        g3.K1 = dff; g3.K = dff + d; g3.fold_g = L.vb; g3.fold_c = L.vb + dff; g3.ln_w = L.n2w; g3.ln_b = L.n2b;
        g3.Wp = L.p_l2; g3.bias = L.l2b; g3.y = h->u3; g3.ldy = d; g3.n_split = d; g3.N = d;
        if (l + 1 < h->nl) { g3.N = 4 * d; g3.Wp2 = L.pf_c; g3.bias2 = L.vc + 6 * d; g3.y2 = h->qkvraw; g3.ldy2 = 3 * d; }
        else { g3.N = d + VS; g3.Wp2 = h->pf_s; g3.bias2 = h->vs + 2 * VS; g3.y2 = h->lraw; g3.ldy2 = VS; }     // raw logits for the sampling head
        PROF_BEGIN();
        if ((rc = launch_step_gemm(h, g3, s))) return rc;
        PROF_END(2);
    }
    return 0;
}

// the kernels of one decode step up to (not including) the sampling head
int32_t enqueue_decoder_step(amt_handle* h, hipStream_t s, int step, StepProf* prof = nullptr) {
    if (h->fold) return enqueue_decoder_step_folded(h, s, step, prof);
    const int B = h->genB, d = h->d, dff = h->dff, H = h->H, hd = h->hd;
    const float qscale = 1.0f / sqrtf((float)hd);
    int32_t rc;
    for (int l = 0; l < h->nl; ++l) {
        const DecLayer& L = h->dec[l];
        float* Kc = h->KVc + (size_t)l * h->kvc_layer;
        float* Vc = Kc + h->kvc_part;
        const float* Kx = h->KVx + (size_t)l * h->kvx_layer;
        const float* Vx = Kx + h->kvx_part;
        // K1: (LN3 of the previous layer) + packed QKV projection, scatter into q / K cache / V cache
        DecodeGemmParams g{};
        g.B = B; g.eps = LN_EPS; g.scale = 1.f;
        g.x = l == 0 ? h->x_in : h->u3; g.ldx = d; g.Wp = L.p_sa; g.bias = L.sa_b; g.N = 3 * d; g.K = d;
        if (l > 0) { g.ln_w = h->dec[l - 1].n3w; g.ln_b = h->dec[l - 1].n3b; g.xn = h->xa; }
        g.mode = 1; g.y = h->qb; g.ldy = d; g.scale = qscale; g.scale_cols = d;
        g.kcache = Kc; g.vcache = Vc; g.H = H; g.hd = hd; g.cap = h->kv_rows; g.pos = pos_slot(h, step); g.d = d;
        PROF_BEGIN();
        if ((rc = launch_step_gemm(h, g, s))) return rc;
        PROF_END(2);
        const float* r0 = l == 0 ? h->x_in : h->xa;
        // K2: relative-position self-attention over the cache
        AttnDecodeParams a{};
        a.q = h->qb; a.k = Kc; a.v = Vc; a.o = h->ob; a.B = B; a.H = H; a.hd = hd; a.cap = h->kv_rows;
        a.pos = pos_slot(h, step); a.Er = L.Er; a.er_len = h->Tcap; a.short_ctx = h->step_short; a.lane_key_stream = h->scalar_stream ? 0 : 1;
        if (!(h->skip_mask & 1)) {
            PROF_BEGIN();
            if ((rc = amt_launch_attn_decode(a, s))) return rc;
            PROF_END(0);
        }
        // K3: out-proj + residual
        DecodeGemmParams o{};
        o.B = B; o.eps = LN_EPS; o.scale = 1.f; o.x = h->ob; o.ldx = d; o.Wp = L.p_sao; o.bias = L.sa_ob; o.N = d; o.K = d;
        o.resid = r0; o.ldr = d; o.y = h->u1; o.ldy = d;
        PROF_BEGIN();
        if ((rc = launch_step_gemm(h, o, s))) return rc;
        PROF_END(2);
        // K4: LN1 + cross-attention query projection
        DecodeGemmParams c{};
        c.B = B; c.eps = LN_EPS; c.x = h->u1; c.ldx = d; c.Wp = L.p_caq; c.bias = L.ca_b; c.N = d; c.K = d;
        c.ln_w = L.n1w; c.ln_b = L.n1b; c.xn = h->xb; c.scale = qscale; c.scale_cols = d; c.y = h->qb; c.ldy = d;
        PROF_BEGIN();
        if ((rc = launch_step_gemm(h, c, s))) return rc;
        PROF_END(2);
        // K5: cross-attention over the clip's video keys
        AttnDecodeParams x{};
        x.q = h->qb; x.k = Kx; x.v = Vx; x.o = h->ob; x.B = B; x.H = H; x.hd = hd; x.cap = h->kx_rows; x.n_keys = h->encS; x.lane_key_stream = h->scalar_stream ? 0 : 1;
        if (!(h->skip_mask & 2)) {
            PROF_BEGIN();
            if ((rc = amt_launch_attn_decode(x, s))) return rc;
            PROF_END(1);
        }
        // K6: out-proj + residual
        DecodeGemmParams o2{};
        o2.B = B; o2.eps = LN_EPS; o2.scale = 1.f; o2.x = h->ob; o2.ldx = d; o2.Wp = L.p_cao; o2.bias = L.ca_ob; o2.N = d; o2.K = d;
        o2.resid = h->xb; o2.ldr = d; o2.y = h->u2; o2.ldy = d;
        PROF_BEGIN();
        if ((rc = launch_step_gemm(h, o2, s))) return rc;
        PROF_END(2);
        // K7: LN2 + FFN up + ReLU
        DecodeGemmParams f1{};
        f1.B = B; f1.eps = LN_EPS; f1.scale = 1.f; f1.x = h->u2; f1.ldx = d; f1.Wp = L.p_l1; f1.bias = L.l1b; f1.N = dff; f1.K = d;
        f1.ln_w = L.n2w; f1.ln_b = L.n2b; f1.xn = h->xc; f1.relu = 1; f1.y = h->hb; f1.ldy = dff;
        PROF_BEGIN();
        if ((rc = launch_step_gemm(h, f1, s))) return rc;
        PROF_END(2);
        // K8: FFN down + residual
        DecodeGemmParams f2{};
        f2.B = B; f2.eps = LN_EPS; f2.scale = 1.f; f2.x = h->hb; f2.ldx = dff; f2.Wp = L.p_l2; f2.bias = L.l2b; f2.N = d; f2.K = dff;
        f2.resid = h->xc; f2.ldr = d; f2.y = h->u3; f2.ldy = d;
        if (dff <= 1536) {
            PROF_BEGIN();
            if ((rc = launch_step_gemm(h, f2, s))) return rc;
            PROF_END(2);
        } else {
            // dim_feedforward beyond the skinny GEMM's 1536 staged columns: column ranges of 1024, every range adding onto the sum of
            // the ones before it (the first takes the bias and the residual)
            for (int k0 = 0; k0 < dff; k0 += FFN_CHUNK) {
                DecodeGemmParams c = f2;
                c.x = h->hb + k0; c.K = std::min(FFN_CHUNK, dff - k0); c.Wp = L.p_l2 + (size_t)cdiv(d, 16) * 16 * k0;
                if (k0) { c.bias = nullptr; c.resid = h->u3; }
                PROF_BEGIN();
                if ((rc = launch_step_gemm(h, c, s))) return rc;
                PROF_END(2);
            }
        }
    }
    return 0;
}

int32_t get_graph(amt_handle* h, int first_pos, int nsteps, float* logits_out, hipGraphExec_t* out) {
    // the graph's steps process positions first_pos .. first_pos + nsteps - 1: when the last of them still has at most one K/V batch
    // of keys, every self-attention of the graph is the short-context instantiation (a graph that straddles the limit keeps the long one)
    const bool short_ctx = h->short_attn && first_pos + nsteps <= amt_attn_decode_stride(h->hd);
    amt_handle::GraphKey key{h->genB, h->genT, h->genP, h->beam, h->mcN, h->mcC, h->encS, nsteps, h->skip_mask | (h->fuse_head ? 4 : 0), h->use_unif,
                             short_ctx ? 1 : 0, first_pos & 1, h->gemm_pipe ? 1 : 0, h->l0_tables ? 1 : 0, h->scalar_stream ? 1 : 0, h->gemm_lean ? 1 : 0, h->rows_dma ? 1 : 0, 0, logits_out};
    for (auto& g : h->graphs)
        if (memcmp(&g.key, &key, sizeof(key)) == 0) { *out = g.exec; return 0; }
    hipGraph_t graph;
    // capture on a private stream: nothing executes during capture, and torch's current stream is
    // often the legacy null stream, which cannot be captured; the graph is launched on the caller's
    if (!h->cap_stream) AMT_HIP(hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
    hipStream_t cs = h->cap_stream;
    AMT_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    int32_t rc = 0;
    // Inside a graph the sampling head between two steps rides in the prologue of the following step's first self-attention
    // (folded chain, decision on the device): [step, head] x n becomes step, (head+step) x (n-1), head.  The measurement hook that
    // leaves the self-attention launches out keeps the separate head (the decision must still happen).
    // Every node carries the slot of the position pair that belongs to its step's parity, so a graph serves the starts of one parity.
    const bool fuse = h->fold && h->fuse_head && !(h->skip_mask & 1);
    h->step_short = short_ctx;
    for (int i = 0; i < nsteps && !rc; ++i) {
        const int step = first_pos + i;
        if (fuse && i > 0) {
            const SampleParams sp = sample_params(h, logits_out, nullptr, 0, step - 1);
            rc = enqueue_decoder_step_folded(h, cs, step, nullptr, &sp);
        } else {
            rc = enqueue_decoder_step(h, cs, step);
        }
        if (!rc && !(fuse && i + 1 < nsteps)) rc = amt_launch_sample(sample_params(h, logits_out, nullptr, 0, step), cs);
    }
    h->step_short = false;
    hipError_t e = hipStreamEndCapture(cs, &graph);
    if (rc) { if (e == hipSuccess) (void)hipGraphDestroy(graph); return rc; }
    AMT_HIP(e);
    hipGraphExec_t exec;
    AMT_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    if (h->graphs.size() >= 32) {        // bound the cache (each distinct logits_out pointer is a new key)
        (void)hipGraphExecDestroy(h->graphs.front().exec);
        (void)hipGraphDestroy(h->graphs.front().graph);
        h->graphs.erase(h->graphs.begin());
    }
    h->graphs.push_back({key, exec, graph});
    *out = exec;
    return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// lifetime
// ------------------------------------------------------------------------------------------------
extern "C" int32_t amt_create(const amt_config* c, amt_handle** out) {
    AMT_CHECK_ARG(c && out, "amt_create: null argument");
    AMT_CHECK_ARG(c->n_layers > 0 && c->num_heads > 0 && c->d_model > 0 && c->dim_feedforward > 0, "amt_create: bad model dims");
    AMT_CHECK_ARG(c->d_model % c->num_heads == 0, "amt_create: d_model %% num_heads != 0");
    const int hd = c->d_model / c->num_heads;
    AMT_CHECK_ARG(hd == 16 || hd == 32 || hd == 64 || hd == 128, "amt_create: head_dim %d not in {16,32,64,128}", hd);
    AMT_CHECK_ARG(c->d_model % 32 == 0 && c->d_model >= 64 && c->d_model <= 1024, "amt_create: d_model must be a multiple of 32, 64 <= d_model <= 1024");
    AMT_CHECK_ARG(c->dim_feedforward % 32 == 0 && c->dim_feedforward <= 8192, "amt_create: dim_feedforward must be a multiple of 32 and <= 8192");
    AMT_CHECK_ARG(c->max_batch > 0 && c->max_batch <= 256, "amt_create: max_batch must be in 1..256 (shard larger batches)");
    AMT_CHECK_ARG(c->max_sequence_video > 0 && c->max_sequence_chord > 0 && c->total_vf_dim > 0, "amt_create: bad sequence dims");
    amt_handle* h = new amt_handle();
    h->cfg = *c;
    h->d = c->d_model; h->H = c->num_heads; h->hd = hd; h->dff = c->dim_feedforward; h->nl = c->n_layers;
    h->Scap = c->max_sequence_video; h->Tcap = c->max_sequence_chord; h->F = c->total_vf_dim;
    h->Fpad = cdiv(h->F, 32) * 32; h->maxB = c->max_batch;
    h->ws_rows = (size_t)h->maxB * (size_t)(h->Scap > h->Tcap ? h->Scap : h->Tcap);
    *out = h;
    return 0;
}

extern "C" int32_t amt_destroy(amt_handle* h) {
    if (!h) return 0;
    (void)hipDeviceSynchronize();
    for (auto& g : h->graphs) { (void)hipGraphExecDestroy(g.exec); (void)hipGraphDestroy(g.graph); }
    if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
    for (void* p : h->owned) (void)hipFree(p);
    delete h;
    return 0;
}

extern "C" int32_t amt_load_weight(amt_handle* h, const char* name, const float* data, int32_t ndim, const int64_t* shape) {
    AMT_CHECK_ARG(h && name && data && ndim > 0 && ndim <= 4 && shape, "amt_load_weight: bad argument");
    Tensor t;
    t.shape.assign(shape, shape + ndim);
    const size_t n = t.numel();
    AMT_CHECK_ARG(n > 0, "amt_load_weight: empty tensor '%s'", name);
    auto it = h->w.find(name);
    if (it != h->w.end() && it->second.numel() == n) {
        t.p = it->second.p;                          // reload in place
    } else {
        int32_t rc = dev_alloc(h, &t.p, n);
        if (rc) return rc;
    }
    AMT_HIP(hipMemcpy(t.p, data, n * sizeof(float), hipMemcpyDefault));
    h->w[name] = t;
    h->finalized = false;
    return 0;
}

extern "C" int32_t amt_finalize(amt_handle* h) {
    AMT_CHECK_ARG(h, "amt_finalize: null handle");
    const int64_t d = h->d, dff = h->dff, F = h->F, hd = h->hd;
    hipStream_t s = nullptr;
    int32_t rc;
    const float *Wvis, *bvis, *Wc, *bc, *Eroot, *Eattr, *Wout, *bout, *enw, *enb, *dnw, *dnb;
    if ((rc = need(h, "Linear_vis.weight", {d, F}, &Wvis))) return rc;
    if ((rc = need(h, "Linear_vis.bias", {d}, &bvis))) return rc;
    if ((rc = need(h, "Linear_chord.weight", {d, d + 1}, &Wc))) return rc;
    if ((rc = need(h, "Linear_chord.bias", {d}, &bc))) return rc;
    {   // 15 chord roots, or (chord_embed) the frozen chord table uploaded under this name: any number of rows
        auto it = h->w.find("embedding_root.weight");
        AMT_CHECK_ARG(it != h->w.end() && it->second.shape.size() == 2, "weight 'embedding_root.weight' was not loaded");
        const int rows = (int)it->second.shape[0];
        AMT_CHECK_ARG(h->chord_embed ? rows >= 1 : rows == 15, "embedding_root.weight has %d rows (15 roots, or a chord table with chord_embed)", rows);
        AMT_CHECK_ARG(!h->KVx || rows == h->n_root, "embedding_root.weight changed its row count (%d -> %d) after the first finalize", h->n_root, rows);
        h->n_root = rows;
    }
    if ((rc = need(h, "embedding_root.weight", {(int64_t)h->n_root, d}, &Eroot))) return rc;
    if ((rc = need(h, "embedding_attr.weight", {16, d}, &Eattr))) return rc;
    if ((rc = need(h, "Wout.weight", {V, d}, &Wout))) return rc;
    if ((rc = need(h, "Wout.bias", {V}, &bout))) return rc;
    if ((rc = need(h, "transformer.encoder.norm.weight", {d}, &enw))) return rc;
    if ((rc = need(h, "transformer.encoder.norm.bias", {d}, &enb))) return rc;
    if ((rc = need(h, "transformer.decoder.norm.weight", {d}, &dnw))) return rc;
    if ((rc = need(h, "transformer.decoder.norm.bias", {d}, &dnb))) return rc;
    if ((rc = need(h, "positional_encoding.pe", {h->Tcap, 1, d}, &h->pe))) return rc;
    if ((rc = need(h, "positional_encoding_video.pe", {h->Scap, 1, d}, &h->pe_v))) return rc;

    if ((rc = amt_decode_gemm_init())) return rc;
    if ((int)h->enc.size() != h->nl) h->enc.assign(h->nl, EncLayer{});
    if ((int)h->dec.size() != h->nl) h->dec.assign(h->nl, DecLayer{});      // keeps the packed buffers across re-finalize
    for (int l = 0; l < h->nl; ++l) {
        const std::string e = "transformer.encoder.layers." + std::to_string(l) + ".";
        EncLayer& E = h->enc[l];
        if ((rc = need(h, e + "self_attn.in_proj_weight", {3 * d, d}, &E.sa_w))) return rc;
        if ((rc = need(h, e + "self_attn.in_proj_bias", {3 * d}, &E.sa_b))) return rc;
        if ((rc = need(h, e + "self_attn.out_proj.weight", {d, d}, &E.sa_ow))) return rc;
        if ((rc = need(h, e + "self_attn.out_proj.bias", {d}, &E.sa_ob))) return rc;
        if ((rc = need(h, e + "linear1.weight", {dff, d}, &E.l1w))) return rc;
        if ((rc = need(h, e + "linear1.bias", {dff}, &E.l1b))) return rc;
        if ((rc = need(h, e + "linear2.weight", {d, dff}, &E.l2w))) return rc;
        if ((rc = need(h, e + "linear2.bias", {d}, &E.l2b))) return rc;
        if ((rc = need(h, e + "norm1.weight", {d}, &E.n1w))) return rc;
        if ((rc = need(h, e + "norm1.bias", {d}, &E.n1b))) return rc;
        if ((rc = need(h, e + "norm2.weight", {d}, &E.n2w))) return rc;
        if ((rc = need(h, e + "norm2.bias", {d}, &E.n2b))) return rc;
        const std::string p = "transformer.decoder.layers." + std::to_string(l) + ".";
        DecLayer& D = h->dec[l];
        if ((rc = need(h, p + "self_attn.in_proj_weight", {3 * d, d}, &D.sa_w))) return rc;
        if ((rc = need(h, p + "self_attn.in_proj_bias", {3 * d}, &D.sa_b))) return rc;
        if ((rc = need(h, p + "self_attn.Er", {h->Tcap, hd}, &D.Er))) return rc;
        if ((rc = need(h, p + "self_attn.out_proj.weight", {d, d}, &D.sa_ow))) return rc;
        if ((rc = need(h, p + "self_attn.out_proj.bias", {d}, &D.sa_ob))) return rc;
        if ((rc = need(h, p + "multihead_attn.in_proj_weight", {3 * d, d}, &D.ca_w))) return rc;
        if ((rc = need(h, p + "multihead_attn.in_proj_bias", {3 * d}, &D.ca_b))) return rc;
        if ((rc = need(h, p + "multihead_attn.out_proj.weight", {d, d}, &D.ca_ow))) return rc;
        if ((rc = need(h, p + "multihead_attn.out_proj.bias", {d}, &D.ca_ob))) return rc;
        if ((rc = need(h, p + "linear1.weight", {dff, d}, &D.l1w))) return rc;
        if ((rc = need(h, p + "linear1.bias", {dff}, &D.l1b))) return rc;
        if ((rc = need(h, p + "linear2.weight", {d, dff}, &D.l2w))) return rc;
        if ((rc = need(h, p + "linear2.bias", {d}, &D.l2b))) return rc;
        if ((rc = need(h, p + "norm1.weight", {d}, &D.n1w))) return rc;
        if ((rc = need(h, p + "norm1.bias", {d}, &D.n1b))) return rc;
        if ((rc = need(h, p + "norm2.weight", {d}, &D.n2w))) return rc;
        if ((rc = need(h, p + "norm2.bias", {d}, &D.n2b))) return rc;
        if ((rc = need(h, p + "norm3.weight", {d}, &D.n3w))) return rc;
        if ((rc = need(h, p + "norm3.bias", {d}, &D.n3b))) return rc;
    }

    if (!h->KVx) {   // first finalize: allocate the persistent state
        h->kx_rows = h->Scap;                    // (300 rows: not a power-of-two stride; an extra row measured no gain)
        h->kvx_part = (size_t)h->nl * h->maxB * h->H * h->kx_rows * h->hd;
        h->kvx_layer = (size_t)h->maxB * h->H * h->kx_rows * h->hd;
        h->kv_rows = amt_tuning().kv_pad >= 0 ? h->Tcap + amt_tuning().kv_pad : (h->Tcap | 1);    // (experiments: 0 = the aliased power-of-two stride)
        h->kvc_part = (size_t)h->nl * h->maxB * h->H * h->kv_rows * h->hd;
        h->kvc_layer = (size_t)h->maxB * h->H * h->kv_rows * h->hd;
        if ((rc = dev_alloc(h, &h->KVx, 2 * h->kvx_part))) return rc;
        if ((rc = dev_alloc(h, &h->KVc, 2 * h->kvc_part))) return rc;
        if ((rc = dev_alloc(h, &h->memory, (size_t)h->maxB * h->Scap * d))) return rc;
        if ((rc = dev_alloc(h, &h->Wvis_pad, (size_t)d * h->Fpad))) return rc;
        if ((rc = dev_alloc(h, &h->Wc_main, (size_t)d * d))) return rc;
        if ((rc = dev_alloc(h, &h->wkey, (size_t)d))) return rc;
        if ((rc = dev_alloc(h, &h->PR, (size_t)h->n_root * d))) return rc;
        if ((rc = dev_alloc(h, &h->PA, (size_t)16 * d))) return rc;
        const size_t mb = (size_t)cdiv(h->maxB, 16) * 16;       // decode rows: whole 16-row blocks of the skinny GEMM
        const size_t bd = mb * d;
        if ((rc = dev_alloc(h, &h->x_in, bd))) return rc;
        if ((rc = dev_alloc(h, &h->u1, bd))) return rc;
        if ((rc = dev_alloc(h, &h->u2, bd))) return rc;
        if ((rc = dev_alloc(h, &h->u3, bd))) return rc;
        if ((rc = dev_alloc(h, &h->xa, bd))) return rc;
        if ((rc = dev_alloc(h, &h->xb, bd))) return rc;
        if ((rc = dev_alloc(h, &h->xc, bd))) return rc;
        if ((rc = dev_alloc(h, &h->qb, bd))) return rc;
        if ((rc = dev_alloc(h, &h->ob, bd))) return rc;
        if ((rc = dev_alloc(h, &h->hb, mb * dff))) return rc;
        // folded chain: K = 2d and dff + d must fit the skinny GEMM, d the attention prologue
        h->fold = !h->plain_chain && d % 32 == 0 && 2 * d <= 1536 && (dff + d) % 64 == 0 && dff + d <= 1536 && dff % 16 == 0;   // G1 / G2 read [o | x]: K = 2d
        if (h->fold) {
            if ((rc = dev_alloc(h, &h->qraw, bd))) return rc;
            if ((rc = dev_alloc(h, &h->hraw, mb * dff))) return rc;
            if ((rc = dev_alloc(h, &h->qkvraw, 3 * bd))) return rc;
            const size_t nmax = (size_t)std::max(3 * d, dff), kmax = (size_t)std::max(d, dff);
            if ((rc = dev_alloc(h, &h->tWs, nmax * d))) return rc;
            if ((rc = dev_alloc(h, &h->tT, kmax * d))) return rc;
            if ((rc = dev_alloc(h, &h->tWc, nmax * kmax))) return rc;
            if ((rc = dev_alloc(h, &h->tComb, nmax * (kmax + d)))) return rc;
            if ((rc = dev_alloc(h, &h->tWs2, (size_t)VS * d))) return rc;
            if ((rc = dev_alloc(h, &h->vs, (size_t)6 * VS))) return rc;
            if ((rc = dev_alloc(h, &h->lraw, mb * VS))) return rc;
            if ((rc = dev_alloc(h, &h->tab_r, (size_t)h->n_root * 3 * d))) return rc;
            if ((rc = dev_alloc(h, &h->tab_a, (size_t)16 * 3 * d))) return rc;
            if ((rc = dev_alloc(h, &h->tab_k, (size_t)3 * d))) return rc;
            if ((rc = dev_alloc(h, &h->tab_cb, (size_t)3 * d))) return rc;
            if ((rc = dev_alloc(h, &h->tab_p, (size_t)h->Tcap * 3 * d))) return rc;
            if ((rc = dev_alloc(h, &h->tab_p0, (size_t)h->Tcap * 2 * d))) return rc;
            if ((rc = dev_alloc(h, &h->tab_ra0, (size_t)(h->n_root + 16) * 2 * d))) return rc;
        }
        if ((rc = dev_alloc(h, &h->keyb, mb))) return rc;
        if ((rc = dev_alloc(h, &h->pos, (size_t)4))) return rc;
        if ((rc = dev_alloc(h, &h->unif, (size_t)h->maxB * h->Tcap))) return rc;
        if ((rc = dev_alloc(h, &h->tokens, (size_t)h->maxB * h->Tcap))) return rc;
        if ((rc = dev_alloc(h, &h->roots, (size_t)h->maxB * h->Tcap))) return rc;
        if ((rc = dev_alloc(h, &h->attrs, (size_t)h->maxB * h->Tcap))) return rc;
        AMT_HIP(hipMemset(h->pos, 0, 16));
    }
    // Linear_vis zero-padded to a multiple of the GEMM K-step; Linear_chord split into its d x d
    // block and the key column (video_music_transformer.py:999-1001: cat([x, key]) -> Linear(d+1, d))
    AMT_HIP(hipMemset(h->Wvis_pad, 0, (size_t)d * h->Fpad * sizeof(float)));
    AMT_HIP(hipMemcpy2D(h->Wvis_pad, h->Fpad * sizeof(float), Wvis, F * sizeof(float), F * sizeof(float), d, hipMemcpyDeviceToDevice));
    AMT_HIP(hipMemcpy2D(h->Wc_main, d * sizeof(float), Wc, (d + 1) * sizeof(float), d * sizeof(float), d, hipMemcpyDeviceToDevice));
    AMT_HIP(hipMemcpy2D(h->wkey, sizeof(float), Wc + d, (d + 1) * sizeof(float), sizeof(float), d, hipMemcpyDeviceToDevice));
    // PR = E_root . Wc_main^T, PA = E_attr . Wc_main^T
    if ((rc = amt_launch_gemm(gemm_params(Eroot, (int)d, h->Wc_main, (int)d, h->PR, (int)d, h->n_root, (int)d, (int)d, nullptr), s))) return rc;
    if ((rc = amt_launch_gemm(gemm_params(Eattr, (int)d, h->Wc_main, (int)d, h->PA, (int)d, 16, (int)d, (int)d, nullptr), s))) return rc;
    for (int l = 0; l < h->nl; ++l) {
        DecLayer& D = h->dec[l];
        if ((rc = pack(h, D.sa_w, 3 * (int)d, (int)d, &D.p_sa, s))) return rc;
        if ((rc = pack(h, D.sa_ow, (int)d, (int)d, &D.p_sao, s))) return rc;
        if ((rc = pack(h, D.ca_w, (int)d, (int)d, &D.p_caq, s))) return rc;      // q rows 0:d of the packed in-proj
        if ((rc = pack(h, D.ca_ow, (int)d, (int)d, &D.p_cao, s))) return rc;
        if ((rc = pack(h, D.l1w, (int)dff, (int)d, &D.p_l1, s))) return rc;
        // linear2 (d x dff): the skinny GEMM stages K <= 1536 input columns; a wider feed-forward is packed -- and multiplied, see
        // FFN_CHUNK -- in column ranges of 1024, one packed block behind the other
        if (dff <= 1536) { if ((rc = pack(h, D.l2w, (int)d, (int)dff, &D.p_l2, s))) return rc; }
        else {
            if (!D.p_l2 && (rc = dev_alloc(h, &D.p_l2, (size_t)cdiv((int)d, 16) * 16 * dff))) return rc;
            for (int k0 = 0; k0 < (int)dff; k0 += FFN_CHUNK) {
                const int kc = std::min(FFN_CHUNK, (int)dff - k0);
                if ((rc = amt_launch_pack_weight(D.l2w + k0, D.p_l2 + (size_t)cdiv((int)d, 16) * 16 * k0, (int)d, kc, s, (int)dff))) return rc;
            }
        }
        if (h->fold) {
            if ((rc = build_fold(h, D.ca_w, (int)d, D.n1w, D.n1b, D.ca_b, D.sa_ow, (int)d, D.sa_ob, &D.pf_a, &D.va, s))) return rc;
            if ((rc = build_fold(h, D.l1w, (int)dff, D.n2w, D.n2b, D.l1b, D.ca_ow, (int)d, D.ca_ob, &D.pf_b, &D.vb, s))) return rc;
            if (l + 1 < h->nl) {
                const DecLayer& Nx = h->dec[l + 1];
                if ((rc = build_fold(h, Nx.sa_w, 3 * (int)d, D.n3w, D.n3b, Nx.sa_b, D.l2w, (int)dff, D.l2b, &D.pf_c, &D.vc, s))) return rc;
            }
        }
    }
    if (h->fold) {
        // layer 0's in-projection of every table the decoder input is a sum of (video_music_transformer.py:984-1001,1029)
        const DecLayer& D0 = h->dec[0];
        const int d3 = 3 * (int)d;
        if ((rc = amt_launch_gemm(gemm_params(h->PR, (int)d, D0.sa_w, (int)d, h->tab_r, d3, h->n_root, d3, (int)d, nullptr), s))) return rc;
        if ((rc = amt_launch_gemm(gemm_params(h->PA, (int)d, D0.sa_w, (int)d, h->tab_a, d3, 16, d3, (int)d, nullptr), s))) return rc;
        if ((rc = amt_launch_gemm(gemm_params(h->wkey, (int)d, D0.sa_w, (int)d, h->tab_k, d3, 1, d3, (int)d, nullptr), s))) return rc;
        if ((rc = amt_launch_gemm(gemm_params(bc, (int)d, D0.sa_w, (int)d, h->tab_cb, d3, 1, d3, (int)d, nullptr), s))) return rc;
        GemmParams gp = gemm_params(h->pe, (int)d, D0.sa_w, (int)d, h->tab_p, d3, h->Tcap, d3, (int)d, D0.sa_b);
        gp.rowadd = h->tab_cb; gp.rowadd_period = 1;
        if ((rc = amt_launch_gemm(gp, s))) return rc;
        // the k / v columns of TP, TR and TA once more with the head outermost (the table-sourced layer-0 key stream of attn_decode_sample):
        // head hh of dst [H][rows][k hd | v hd] takes columns d + hh*hd .. and 2d + hh*hd .. of src [rows][3d]; no arithmetic
        auto head_slices = [&](const float* src, int rows, float* dst, int dst_rows, int row0) -> int32_t {
            for (int hh = 0; hh < h->H; ++hh)
                for (int part = 0; part < 2; ++part)
                    AMT_HIP(hipMemcpy2DAsync(dst + ((size_t)hh * dst_rows + row0) * 2 * hd + (size_t)part * hd, (size_t)2 * hd * sizeof(float),
                                             src + (size_t)(1 + part) * d + (size_t)hh * hd, (size_t)d3 * sizeof(float), (size_t)hd * sizeof(float),
                                             rows, hipMemcpyDeviceToDevice, s));
            return 0;
        };
        if ((rc = head_slices(h->tab_p, h->Tcap, h->tab_p0, h->Tcap, 0))) return rc;
        if ((rc = head_slices(h->tab_r, h->n_root, h->tab_ra0, h->n_root + 16, 0))) return rc;
        if ((rc = head_slices(h->tab_a, 16, h->tab_ra0, h->n_root + 16, h->n_root))) return rc;
        // output head folded through norm3 of the last layer and decoder.norm (see SampleParams::lraw)
        const DecLayer& DL = h->dec[h->nl - 1];
        if ((rc = amt_launch_scale_cols(Wout, dnw, h->tWs2, V, (int)d, s))) return rc;                 // Wout o gf
        if ((rc = amt_launch_scale_cols(h->tWs2, DL.n3w, h->tWs, V, (int)d, s))) return rc;            // W'' = Wout o gf o g3
        if ((rc = amt_launch_transpose(DL.l2w, h->tT, (int)d, (int)dff, s))) return rc;
        if ((rc = amt_launch_gemm(gemm_params(h->tWs, (int)d, h->tT, (int)d, h->tWc, (int)dff, V, (int)dff, (int)d, nullptr), s))) return rc;
        const size_t ld = (size_t)(dff + d) * sizeof(float);
        AMT_HIP(hipMemcpy2DAsync(h->tComb, ld, h->tWc, (size_t)dff * sizeof(float), (size_t)dff * sizeof(float), V, hipMemcpyDeviceToDevice, s));
        AMT_HIP(hipMemcpy2DAsync(h->tComb + dff, ld, h->tWs, (size_t)d * sizeof(float), (size_t)d * sizeof(float), V, hipMemcpyDeviceToDevice, s));
        if ((rc = pack(h, h->tComb, V, (int)(dff + d), &h->pf_s, s))) return rc;
        AMT_HIP(hipMemsetAsync(h->vs, 0, (size_t)6 * VS * sizeof(float), s));
        // h1 = rowsum(W''), h2 = (Wout o gf).b3, dv = W''.b2 ; h3 = rowsum(Wout o gf), h4 = Wout.bf + bout
        if ((rc = amt_launch_fold_vectors(h->tWs2, h->tWs, DL.n3b, nullptr, DL.l2b, h->vs, h->vs + VS, h->vs + 2 * VS, V, (int)d, s))) return rc;
        if ((rc = amt_launch_fold_vectors(Wout, h->tWs2, dnb, bout, DL.l2b, h->vs + 3 * VS, h->vs + 4 * VS, h->vs + 5 * VS, V, (int)d, s))) return rc;
    }
    AMT_HIP(hipDeviceSynchronize());
    // captured graphs hold pointers that stay valid (weights reload in place), nothing to invalidate
    h->finalized = true;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// encoder
// ------------------------------------------------------------------------------------------------
extern "C" int32_t amt_set_option(amt_handle* h, const char* name, int32_t value) {
    if (!h && name && strcmp(name, "scalar_key_stream") == 0) {   // no handle: the process-wide default of the operator entry points and the lockstep step
        amt_attn_decode_scalar_stream(value != 0);
        return 0;
    }
    if (!h && name && strcmp(name, "gemm_rows_dma") == 0) {       // ... and of the skinny-GEMM entry points (amt_decode_gemm_ex_fwd)
        amt_decode_gemm_rows_dma(value != 0);
        return 0;
    }
    AMT_CHECK_ARG(h && name, "amt_set_option: null argument");
    if (strcmp(name, "chord_embed") == 0) {
        AMT_CHECK_ARG(!h->KVx || h->chord_embed == (value != 0), "amt_set_option: chord_embed must be chosen before the first amt_finalize");
        h->chord_embed = value != 0;
        return 0;
    }
    if (strcmp(name, "causal_mask") == 0) {                  // run-time switch of amt_prefill (forward(mask=False), :978-982)
        h->causal_mask = value != 0;
        return 0;
    }
    if (strcmp(name, "decode_chain_plain") == 0) {           // the 49-launch decode chain (also the fall-back of shapes the fold does not cover)
        AMT_CHECK_ARG(!h->KVx || h->plain_chain == (value != 0), "amt_set_option: decode_chain_plain must be chosen before the first amt_finalize");
        h->plain_chain = value != 0;
        return 0;
    }
    if (strcmp(name, "fuse_sampling_head") == 0) {           // 0: every step of a captured graph ends with its own sampling-head launch (31 per step)
        h->fuse_head = value != 0;
        return 0;
    }
    if (strcmp(name, "short_context_attn") == 0) {           // 0: every captured graph uses the long-context self-attention (A/B and parity tests)
        h->short_attn = value != 0;
        return 0;
    }
    if (strcmp(name, "gemm_tile_pipeline") == 0) {           // 0: the decode step's skinny GEMMs keep the serial tile loop (A/B and bit-identity tests); part of the graph key
        h->gemm_pipe = value != 0;
        return 0;
    }
    if (strcmp(name, "gemm_scalar_front") == 0) {            // 0: the decode step's skinny GEMMs keep their generic front (A/B and bit-identity tests); part of the graph key
        h->gemm_lean = value != 0;
        return 0;
    }
    if (strcmp(name, "gemm_rows_dma") == 0) {                // 0: the decode step's skinny GEMMs stage their rows through registers (A/B and bit-identity tests); part of the graph key
        h->rows_dma = value != 0;
        return 0;
    }
    if (strcmp(name, "layer0_kv_from_tables") == 0) {        // 0: layer 0's self-attention always streams its keys from the K/V cache (A/B and bit-identity tests); part of the graph key
        h->l0_tables = value != 0;
        return 0;
    }
    if (strcmp(name, "scalar_key_stream") == 0) {            // 0: the decode attentions of this handle keep the per-lane controlled key stream (A/B and bit-identity tests); part of the graph key
        h->scalar_stream = value != 0;
        return 0;
    }
    if (strcmp(name, "profile_skip") == 0) {                 // measurement hook of bench.py: leave a kernel class out of the captured step
        AMT_CHECK_ARG(value >= 0 && value < 4, "amt_set_option: profile_skip takes 0 (none), 1 (self-attention), 2 (cross-attention) or 3");
        h->skip_mask = value;
        return 0;
    }
    AMT_CHECK_ARG(false, "amt_set_option: unknown option '%s'", name);
    return -1;
}

extern "C" int32_t amt_encode_resid(amt_handle* h, int32_t B, int32_t S, const float* sem, int32_t sem_dim, const float* scene,
                                    const float* motion, int32_t motion_dim, const float* emotion, int32_t emo_dim,
                                    const float* vis_resid, float* memory_out, void* stream) {
    AMT_CHECK_ARG(h, "amt_encode_resid: null handle");
    h->vis_resid = vis_resid;
    const int32_t rc = amt_encode(h, B, S, sem, sem_dim, scene, motion, motion_dim, emotion, emo_dim, memory_out, stream);
    h->vis_resid = nullptr;
    return rc;
}

extern "C" int32_t amt_encode(amt_handle* h, int32_t B, int32_t S, const float* sem, int32_t sem_dim, const float* scene,
                              const float* motion, int32_t motion_dim, const float* emotion, int32_t emo_dim,
                              float* memory_out, void* stream) {
    AMT_CHECK_ARG(h && h->finalized, "amt_encode: handle not finalized");
    AMT_CHECK_ARG(B > 0 && B <= h->maxB, "amt_encode: B=%d outside 1..%d", B, h->maxB);
    AMT_CHECK_ARG(S > 0 && S <= h->Scap, "amt_encode: S=%d outside 1..%d", S, h->Scap);
    AMT_CHECK_ARG(sem_dim + 1 + motion_dim + emo_dim == h->F, "amt_encode: feature widths %d+1+%d+%d != total_vf_dim %d",
                  sem_dim, motion_dim, emo_dim, h->F);
    AMT_CHECK_ARG(sem && scene && motion && emotion, "amt_encode: null feature pointer");
    hipStream_t s = (hipStream_t)stream;
    int32_t rc = ensure_workspace(h);
    if (rc) return rc;
    const int d = h->d, R = B * S;
    const float qscale = 1.0f / sqrtf((float)h->hd);
    if ((rc = amt_launch_concat_features(sem, sem_dim, scene, motion, motion_dim, emotion, emo_dim, h->wsA0, R, h->Fpad, s))) return rc;
    {   // Linear_vis + positional encoding of the frame index
        GemmParams g = gemm_params(h->wsA0, h->Fpad, h->Wvis_pad, h->Fpad, h->wsX, d, R, d, h->Fpad, W(h, "Linear_vis.bias"));
        g.rowadd = h->pe_v; g.rowadd_period = S;
        g.resid = h->vis_resid; g.ldr = d;               // scene_embed: + scene_embedding(feature_scene_offset.int()) (:1026-1027)
        if ((rc = amt_launch_gemm(g, s))) return rc;
    }
    for (int l = 0; l < h->nl; ++l) {
        const EncLayer& E = h->enc[l];
        GemmParams g = gemm_params(h->wsX, d, E.sa_w, d, h->wsQKV, 3 * d, R, 3 * d, d, E.sa_b);
        g.scale = qscale; g.scale_cols = d;
        if ((rc = amt_launch_gemm(g, s))) return rc;
        AttnParams a{};
        a.q = h->wsQKV; a.k = h->wsQKV + d; a.v = h->wsQKV + 2 * d; a.o = h->wsO;
        a.q_bs = a.k_bs = a.v_bs = (size_t)S * 3 * d; a.q_hs = a.k_hs = a.v_hs = h->hd; a.q_ls = a.k_ls = a.v_ls = 3 * d;
        a.o_bs = (size_t)S * d; a.o_hs = h->hd; a.o_ls = d;
        a.B = B; a.H = h->H; a.Lq = S; a.Lk = S; a.hd = h->hd; a.kv_group = 1;
        if ((rc = amt_launch_attn_prefill(a, s))) return rc;
        if ((rc = proj_resid_ln(h, h->wsO, d, E.sa_ow, E.sa_ob, h->wsX, E.n1w, E.n1b, nullptr, nullptr, h->wsU, h->wsX, R, s))) return rc;
        const bool last = l == h->nl - 1;
        if ((rc = ffn_block(h, h->wsX, E.l1w, E.l1b, E.l2w, E.l2b, E.n2w, E.n2b,
                            last ? W(h, "transformer.encoder.norm.weight") : nullptr,
                            last ? W(h, "transformer.encoder.norm.bias") : nullptr,
                            last ? h->memory : h->wsX, R, s))) return rc;
    }
    if (memory_out) AMT_HIP(hipMemcpyAsync(memory_out, h->memory, (size_t)R * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    // per decoder layer: K,V = memory . W[d:3d]^T + b[d:3d], stored head-major for the streaming decode kernel
    for (int l = 0; l < h->nl; ++l) {
        const DecLayer& D = h->dec[l];
        GemmParams g = gemm_params(h->memory, d, D.ca_w + (size_t)d * d, d, h->KVx + (size_t)l * h->kvx_layer, 0, R, 2 * d, d, D.ca_b + d);
        g.head_split = 1; g.hs_seq = S; g.hs_seq_cap = h->kx_rows; g.hs_d = d; g.hs_hd = h->hd; g.hs_heads = h->H;
        g.hs_part_stride = h->kvx_part;
        if ((rc = amt_launch_gemm(g, s))) return rc;
    }
    h->encB = B; h->encS = S;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// teacher-forced decoder pass
// ------------------------------------------------------------------------------------------------
extern "C" int32_t amt_prefill(amt_handle* h, int32_t B, int32_t L, const int64_t* root_ids, const int64_t* attr_ids,
                               const float* key, float* logits_out, float* layer_out, int32_t layer_index, void* stream) {
    AMT_CHECK_ARG(h && h->finalized, "amt_prefill: handle not finalized");
    AMT_CHECK_ARG(B > 0 && B == h->encB, "amt_prefill: B=%d does not match the last amt_encode (B=%d)", B, h->encB);
    AMT_CHECK_ARG(L > 0 && L <= h->Tcap, "amt_prefill: L=%d outside 1..%d (max_sequence_chord)", L, h->Tcap);
    AMT_CHECK_ARG(root_ids && attr_ids && key && logits_out, "amt_prefill: null pointer");
    hipStream_t s = (hipStream_t)stream;
    int32_t rc = ensure_workspace(h);
    if (rc) return rc;
    const int d = h->d, R = B * L, S = h->encS;
    const float qscale = 1.0f / sqrtf((float)h->hd);
    if ((rc = amt_launch_chord_embed(root_ids, attr_ids, key, h->PR, h->PA, h->wkey, W(h, "Linear_chord.bias"), h->pe, h->wsX, B, L, d, s))) return rc;
    for (int l = 0; l < h->nl; ++l) {
        const DecLayer& D = h->dec[l];
        GemmParams g = gemm_params(h->wsX, d, D.sa_w, d, h->wsQKV, 3 * d, R, 3 * d, d, D.sa_b);
        g.scale = qscale; g.scale_cols = d;
        if ((rc = amt_launch_gemm(g, s))) return rc;
        AttnParams a{};
        a.q = h->wsQKV; a.k = h->wsQKV + d; a.v = h->wsQKV + 2 * d; a.o = h->wsO;
        a.q_bs = a.k_bs = a.v_bs = (size_t)L * 3 * d; a.q_hs = a.k_hs = a.v_hs = h->hd; a.q_ls = a.k_ls = a.v_ls = 3 * d;
        a.o_bs = (size_t)L * d; a.o_hs = h->hd; a.o_ls = d;
        a.B = B; a.H = h->H; a.Lq = L; a.Lk = L; a.hd = h->hd; a.causal = h->causal_mask ? 1 : 0; a.Er = D.Er; a.er_len = h->Tcap; a.kv_group = 1;
        if ((rc = amt_launch_attn_prefill(a, s))) return rc;
        if ((rc = proj_resid_ln(h, h->wsO, d, D.sa_ow, D.sa_ob, h->wsX, D.n1w, D.n1b, nullptr, nullptr, h->wsU, h->wsX, R, s))) return rc;
        // cross-attention: q from the chord stream, K/V precomputed per clip by amt_encode
        GemmParams q = gemm_params(h->wsX, d, D.ca_w, d, h->wsQc, d, R, d, d, D.ca_b);
        q.scale = qscale; q.scale_cols = d;
        if ((rc = amt_launch_gemm(q, s))) return rc;
        AttnParams c{};
        c.q = h->wsQc; c.k = h->KVx + (size_t)l * h->kvx_layer; c.v = c.k + h->kvx_part; c.o = h->wsO;
        c.q_bs = (size_t)L * d; c.q_hs = h->hd; c.q_ls = d;
        c.k_bs = c.v_bs = (size_t)h->H * h->kx_rows * h->hd; c.k_hs = c.v_hs = (size_t)h->kx_rows * h->hd; c.k_ls = c.v_ls = h->hd;
        c.o_bs = (size_t)L * d; c.o_hs = h->hd; c.o_ls = d;
        c.B = B; c.H = h->H; c.Lq = L; c.Lk = S; c.hd = h->hd; c.kv_group = 1;
        if ((rc = amt_launch_attn_prefill(c, s))) return rc;
        if ((rc = proj_resid_ln(h, h->wsO, d, D.ca_ow, D.ca_ob, h->wsX, D.n2w, D.n2b, nullptr, nullptr, h->wsU, h->wsX, R, s))) return rc;
        if ((rc = ffn_block(h, h->wsX, D.l1w, D.l1b, D.l2w, D.l2b, D.n3w, D.n3b, nullptr, nullptr, h->wsX, R, s))) return rc;
        if (layer_out && l == layer_index)
            AMT_HIP(hipMemcpyAsync(layer_out, h->wsX, (size_t)R * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    if ((rc = amt_launch_layernorm(h->wsX, nullptr, W(h, "transformer.decoder.norm.weight"), W(h, "transformer.decoder.norm.bias"),
                                   nullptr, nullptr, h->wsU, R, d, LN_EPS, s))) return rc;
    GemmParams g = gemm_params(h->wsU, d, W(h, "Wout.weight"), d, logits_out, V, R, V, d, W(h, "Wout.bias"));
    return amt_launch_gemm(g, s);
}

// ------------------------------------------------------------------------------------------------
// generate
// ------------------------------------------------------------------------------------------------
namespace {
__global__ void init_sequences_kernel(int64_t* tokens, int64_t* roots, int64_t* attrs, const int64_t* primer,
                                      const int64_t* primer_root, const int64_t* primer_attr, int P, int per_clip, int T) {
    const int b = blockIdx.x;
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        int64_t tk = 158, r = 14, a = 15;            // CHORD_PAD, CHORD_ROOT_PAD, CHORD_ATTR_PAD
        if (t < P) {
            const size_t i = per_clip ? (size_t)b * P + t : (size_t)t;
            tk = primer[i]; r = primer_root[i]; a = primer_attr[i];
        }
        tokens[(size_t)b * T + t] = tk; roots[(size_t)b * T + t] = r; attrs[(size_t)b * T + t] = a;
    }
}
}  // namespace

extern "C" int32_t amt_generate_begin(amt_handle* h, int32_t B, const int64_t* primer, const int64_t* primer_root,
                                      const int64_t* primer_attr, int32_t P, int32_t primer_per_clip, const float* key,
                                      int32_t T, int32_t beam, int32_t max_conseq_N, int32_t max_conseq_chord, void* stream) {
    AMT_CHECK_ARG(h && h->finalized, "amt_generate: handle not finalized");
    AMT_CHECK_ARG(B > 0 && B == h->encB, "amt_generate: B=%d does not match the last amt_encode (B=%d)", B, h->encB);
    AMT_CHECK_ARG(T > 0 && T <= h->Tcap, "amt_generate: target_seq_length=%d outside 1..%d (max_sequence_chord)", T, h->Tcap);
    AMT_CHECK_ARG(P > 0 && P <= T, "amt_generate: primer length %d outside 1..%d", P, T);
    AMT_CHECK_ARG(beam == 0 || beam == 1, "amt_generate: beam=%d is not supported (0 = sampling branch, 1 = top-1 branch)", beam);
    AMT_CHECK_ARG(max_conseq_chord >= 1, "amt_generate: max_conseq_chord must be >= 1");
    AMT_CHECK_ARG(primer && primer_root && primer_attr && key, "amt_generate: null pointer");
    hipStream_t s = (hipStream_t)stream;
    h->genB = B; h->genT = T; h->genP = P; h->beam = beam; h->mcN = max_conseq_N; h->mcC = max_conseq_chord;
    h->steps_done = 0; h->gen_active = true; h->use_unif = 0;
    hipLaunchKernelGGL(init_sequences_kernel, dim3(B), dim3(256), 0, s, h->tokens, h->roots, h->attrs, primer, primer_root,
                       primer_attr, P, primer_per_clip, T);
    AMT_LAUNCH_CHECK();
    AMT_HIP(hipMemcpyAsync(h->keyb, key, B * sizeof(float), hipMemcpyDeviceToDevice, s));
    AMT_HIP(hipMemsetAsync(h->pos, 0, 16, s));
    return amt_launch_embed_step(sample_params(h, nullptr, nullptr, 0, 0), 0, s);     // x_in for position 0
}

extern "C" int32_t amt_generate_set_uniforms(amt_handle* h, const float* uniforms, void* stream) {
    AMT_CHECK_ARG(h && h->gen_active, "amt_generate_set_uniforms: no generation in progress");
    AMT_CHECK_ARG(h->beam == 0, "amt_generate_set_uniforms: the categorical draw belongs to the sampling branch (beam=0)");
    h->use_unif = uniforms != nullptr;
    if (uniforms)
        AMT_HIP(hipMemcpyAsync(h->unif, uniforms, (size_t)h->genT * h->genB * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

extern "C" int32_t amt_generate_run(amt_handle* h, int32_t n_steps, float* logits_out, void* stream) {
    AMT_CHECK_ARG(h && h->gen_active, "amt_generate_run: no generation in progress");
    hipStream_t s = (hipStream_t)stream;
    const int remaining = h->genT - 1 - h->steps_done;
    if (n_steps < 0 || n_steps > remaining) n_steps = remaining;
    int32_t rc;
    int left = n_steps;
    const int spg = amt_tuning().steps_per_graph;
    while (left > 0) {
        int ns = spg;                               // whole graphs, then the remainder in halves (each size is captured once)
        while (ns > left) ns >>= 1;
        if (ns < 1) ns = 1;
        hipGraphExec_t exec;
        if ((rc = get_graph(h, h->steps_done + n_steps - left, ns, logits_out, &exec))) return rc;
        AMT_HIP(hipGraphLaunch(exec, s));
        left -= ns;
    }
    h->steps_done += n_steps;
    return 0;
}

extern "C" int32_t amt_generate_profile(amt_handle* h, int32_t n_steps, double* ms_by_class, int64_t* launches_by_class,
                                        int64_t* attn_bytes_by_class, void* stream) {
    AMT_CHECK_ARG(h && h->gen_active && ms_by_class && launches_by_class && attn_bytes_by_class, "amt_generate_profile: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int remaining = h->genT - 1 - h->steps_done;
    if (n_steps < 0 || n_steps > remaining) n_steps = remaining;
    StepProf prof;
    prof.s = s;
    for (int c = 0; c < 5; ++c) { ms_by_class[c] = 0.0; launches_by_class[c] = 0; }
    attn_bytes_by_class[0] = attn_bytes_by_class[1] = 0;
    int32_t rc = 0;
    for (int i = 0; i < n_steps && !rc; ++i) {
        prof.used = 0; prof.cls.clear();
        rc = enqueue_decoder_step(h, s, h->steps_done + i, &prof);
        if (rc) break;
        prof.begin();
        rc = amt_launch_sample(sample_params(h, nullptr, nullptr, 0, h->steps_done + i), s);
        prof.end(3);
        if (rc) break;
        prof.begin();            // class 4: an empty pair = the cost of the event records themselves
        prof.end(4);
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) { amt_set_error("amt_generate_profile: %s", hipGetErrorString(e)); rc = (int32_t)e; break; }
        for (size_t k = 0; k < prof.cls.size(); ++k) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, prof.ev[2 * k], prof.ev[2 * k + 1]);
            ms_by_class[prof.cls[k]] += ms;
            launches_by_class[prof.cls[k]] += 1;
        }
        // algorithmic K/V bytes of this step's attention launches: keys 0..t for self, S for cross
        const int64_t row = (int64_t)h->d * 4 * 2 * h->genB;
        attn_bytes_by_class[0] += (int64_t)h->nl * (h->steps_done + i + 1) * row;
        attn_bytes_by_class[1] += (int64_t)h->nl * h->encS * row;
    }
    for (auto e : prof.ev) if (e) (void)hipEventDestroy(e);
    if (rc) return rc;
    h->steps_done += n_steps;
    return 0;
}

extern "C" int32_t amt_generate_step_probs(amt_handle* h, float* probs_out, void* stream) {
    AMT_CHECK_ARG(h && h->gen_active && probs_out, "amt_generate_step_probs: no generation in progress");
    AMT_CHECK_ARG(h->steps_done < h->genT - 1, "amt_generate_step_probs: sequence is complete");
    hipStream_t s = (hipStream_t)stream;
    int32_t rc = enqueue_decoder_step(h, s, h->steps_done);
    if (rc) return rc;
    return amt_launch_sample(sample_params(h, nullptr, probs_out, 1, h->steps_done), s);
}

namespace {
__global__ void commit_tokens_kernel(int64_t* tokens, const int64_t* chosen, const int* pos, int T, int n_primer) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int cur = *pos + 1;
    if (b < (int)(gridDim.x * blockDim.x) && cur < T && cur >= n_primer) tokens[(size_t)b * T + cur] = chosen[b];
}
}  // namespace

extern "C" int32_t amt_generate_commit(amt_handle* h, const int64_t* chosen, void* stream) {
    AMT_CHECK_ARG(h && h->gen_active && chosen, "amt_generate_commit: no generation in progress");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(commit_tokens_kernel, dim3(1), dim3(h->genB), 0, s, h->tokens, chosen, pos_slot(h, h->steps_done), h->genT, h->genP);
    AMT_LAUNCH_CHECK();
    int32_t rc = amt_launch_embed_step(sample_params(h, nullptr, nullptr, 1, h->steps_done), 1, s);
    if (rc) return rc;
    h->steps_done += 1;
    return 0;
}

// Test access to the self-attention K/V cache, [2 (K, V)][n_layers][max_batch][H][rows][hd] fp32 where rows = max_sequence_chord
// plus the padding row(s) that keep the heads off a power-of-two stride: dims_out (6 values) receives that shape; with buf the whole
// cache is copied out (write = 0) or in (write = 1), n_floats being the caller's count of the product
extern "C" int32_t amt_kv_cache_io(amt_handle* h, float* buf, int64_t n_floats, int32_t write, int64_t* dims_out, void* stream) {
    AMT_CHECK_ARG(h && h->KVc, "amt_kv_cache_io: handle not finalized");
    const int64_t dims[6] = {2, h->nl, h->maxB, h->H, h->kv_rows, h->hd};
    if (dims_out) for (int i = 0; i < 6; ++i) dims_out[i] = dims[i];
    if (!buf) return 0;
    AMT_CHECK_ARG(n_floats == (int64_t)(2 * h->kvc_part), "amt_kv_cache_io: the cache holds %lld floats, not %lld", (long long)(2 * h->kvc_part), (long long)n_floats);
    const size_t bytes = 2 * h->kvc_part * sizeof(float);
    if (write) AMT_HIP(hipMemcpyAsync(h->KVc, buf, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    else AMT_HIP(hipMemcpyAsync(buf, h->KVc, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

extern "C" int32_t amt_generate_set_branch(amt_handle* h, int32_t beam) {
    AMT_CHECK_ARG(h && h->gen_active, "amt_generate_set_branch: no generation in progress");
    AMT_CHECK_ARG(beam == 0 || beam == 1, "amt_generate_set_branch: branch %d (0 = sampling branch, 1 = top-k branch)", beam);
    h->beam = beam;
    return 0;
}

extern "C" int32_t amt_generate_end(amt_handle* h, int64_t* tokens_out, void* stream) {
    AMT_CHECK_ARG(h && h->gen_active && tokens_out, "amt_generate_end: no generation in progress");
    AMT_HIP(hipMemcpyAsync(tokens_out, h->tokens, (size_t)h->genB * h->genT * sizeof(int64_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

extern "C" int32_t amt_generate(amt_handle* h, int32_t B, const int64_t* primer, const int64_t* primer_root,
                                const int64_t* primer_attr, int32_t P, int32_t primer_per_clip, const float* key,
                                int32_t T, int32_t beam, int32_t max_conseq_N, int32_t max_conseq_chord,
                                int64_t* tokens_out, float* logits_out, void* stream) {
    int32_t rc = amt_generate_begin(h, B, primer, primer_root, primer_attr, P, primer_per_clip, key, T, beam,
                                    max_conseq_N, max_conseq_chord, stream);
    if (rc) return rc;
    if ((rc = amt_generate_run(h, -1, logits_out, stream))) return rc;
    return amt_generate_end(h, tokens_out, stream);
}

extern "C" int64_t amt_decode_step_bytes(const amt_handle* h, int32_t B, int32_t n_self_keys, int32_t S) {
    if (!h) return 0;
    // K and V rows streamed by the two attention kernels of every layer (fp32)
    const int64_t row = (int64_t)h->d * 4 * 2;
    return (int64_t)h->nl * B * ((int64_t)n_self_keys + S) * row;
}
