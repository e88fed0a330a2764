/*
 * libamt_hip — C ABI of the MI355X (gfx950) implementation of the Affective Multimodal Transformer
 * forward / generate hot path of khangklj/Video2Music.
 *
 * The reference has no FFI of its own: its seam for this path is the Python nn.Module surface
 *   model/video_music_transformer.py:910-1132   class VideoMusicTransformer (forward, generate)
 *   model/rpr.py:17-455                         TransformerDecoderRPR / MultiheadAttentionRPR / _skew
 *   model/positional_encoding.py:7-23           PositionalEncoding
 *   model/grouped_query_attention.py:172-358    MultiheadGQA
 *   model/moe.py:36-49,150-302                  GLUExpert / MoELayer / SharedMoELayer
 *   model/custom_transformer.py:27-48           RMSNorm
 *   model/rotate_operation.py:50-165            RotaryPositionalEmbeddings
 * Each entry point below names the reference code it replaces.  The Python host module
 * (video2music_amd/model/ python files) binds these with ctypes; INTEGRATION.md shows the stub a maintainer
 * of the reference would add.
 *
 * Conventions
 *   - a function declared amt_status returns a status: 0 = ok, < 0 = bad argument, > 0 = hipError_t;
 *     amt_last_error() returns a thread-local message for the last non-zero return.  Any other return type (int32_t, int64_t,
 *     const char*) is a value, never a status.  amt_status is int32_t: the distinction is for the reader and for
 *     video2music_amd/_lib.py, which reads its ctypes prototypes, struct layouts and constants from this file and raises on a
 *     non-zero return exactly where amt_status is declared.  It reads declarations of the plain forms used below -- `type name(args);`,
 *     `typedef struct name { fields } name;`, `#define AMT_X <integer>` -- over int32_t, int64_t, float, double, const char* and
 *     pointers, and refuses anything else at import.
 *   - all tensor arguments are raw DEVICE pointers, fp32 (ids int64), row-major, 16-byte aligned;
 *     the caller owns inputs and outputs; weights are copied (and repacked) into library-owned
 *     memory by amt_load_weight, so caller storage may be freed afterwards.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     nothing synchronises the device except amt_finalize / amt_destroy.  amt_generate captures
 *     its decode step into a hipGraph on first use for a given (batch, mode).
 *   - threading: one handle per (process, device); a handle and everything it owns (workspaces, K/V caches, captured graphs,
 *     options) belongs to ONE host thread at a time.  The stateless operator entry points may be called from several host
 *     threads concurrently, each on its own stream, as long as they share no output or scratch buffer.
 *   - global state: the library keeps no mutable global besides (a) the thread-local error message, (b) per-device one-time
 *     initialisations (the > 64 KiB dynamic-LDS opt-in of a kernel, a 256-byte block of zero words), each taken under a mutex,
 *     (c) the process-wide key-stream default of amt_set_option(NULL, "scalar_key_stream", v), one atomic int, and (d) the immutable
 *     tuning record of csrc/amt_common.h.  The release build reads NO environment variable; a
 *     -DAMT_EXPERIMENT build (tools/ab_build.sh) reads the A/B switches of DESIGN.md once, under std::call_once.
 *   - amt_abi_version() == AMT_ABI_VERSION of the header the caller was built against, or the caller must refuse the library.
 */
#ifndef AMT_HIP_H
#define AMT_HIP_H
#include <stdint.h>

#define AMT_ABI_VERSION 14   /* 2: argument structs for the step / skinny-GEMM calls, options in place of amt_debug_set_skip;
                                3: the lockstep step's stacked gate | linear1 matrix is packed from rows interleaved in eights;
                                4: amt_chord_metrics_fwd;
                                5: amt_reg_metrics_fwd;
                                6: amt_rnn_seq_train_fwd, amt_rnn_seq_bwd, amt_reg_loss_fwd_bwd;
                                7: amt_attn_train_fwd, amt_attn_bwd, amt_attn_bwd_ws_floats, amt_layernorm_bwd, amt_chord_loss_fwd_bwd,
                                   amt_chord_loss_ws_floats;
                                8: amt_selective_scan_train_fwd, amt_selective_scan_bwd, amt_selective_scan_bwd_ws_floats,
                                   amt_dwconv1d_silu_bwd, amt_dwconv1d_silu_bwd_ws_floats;
                                9: amt_gemm_route, amt_attn_route;
                                10: amt_moe_train_scratch_floats, amt_moe_train_fwd, amt_moe_bwd_ws_floats, amt_moe_bwd;
                                11: amt_moe_wgrad_splits;
                                12: amt_rope_bwd, amt_rmsnorm_bwd, amt_rmsnorm_bwd_blocks, amt_glu_train_scratch_floats, amt_glu_train_fwd,
                                    amt_glu_bwd_ws_floats, amt_glu_bwd;
                                13: amt_diff_subln_train_fwd, amt_diff_subln_bwd, amt_diff_subln_bwd_blocks, amt_moe_train_fwd_balanced;
                                14: amt_selective_scan_wide_train_fwd, amt_selective_scan_wide_ckpt_steps, amt_selective_scan_wide_bwd,
                                    amt_selective_scan_wide_bwd_ws_floats, amt_silu_bwd;
                                    (still 14) amt_rnn_wide_*, amt_chord_loss_aux_*, amt_optim_step, amt_optim_plan: additions only */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct amt_handle amt_handle;
typedef int32_t amt_status;      /* 0 = ok, or an error with amt_last_error(): see the conventions above */

/* Constructor arguments of VideoMusicTransformer (model/video_music_transformer.py:911-914) that
 * shape the computation, plus the batch capacity the reference does not have (it is batch-1). */
typedef struct amt_config {
    int32_t n_layers;            /* encoder and decoder layers (6) */
    int32_t num_heads;           /* 8 */
    int32_t d_model;             /* 512 */
    int32_t dim_feedforward;     /* 1024 */
    int32_t max_sequence_video;  /* 300: rows of positional_encoding_video.pe, key capacity of cross-attention */
    int32_t max_sequence_chord;  /* rows of Er / positional_encoding.pe = longest chord sequence */
    int32_t total_vf_dim;        /* width of the concatenated video feature (generate.py:141-160) */
    int32_t max_batch;           /* clips per call, 1..256: sizes the K/V caches and workspaces (32 = BASELINE.json's per-GPU batch) */
} amt_config;

const char* amt_last_error(void);
int32_t amt_abi_version(void);

/* ---- model lifetime -------------------------------------------------------------------- */
/* Shapes the handle takes (anything else is refused with a message, never computed wrongly): d_model a multiple of 32 with
 * 64 <= d_model <= 1024; head_dim = d_model / num_heads in {16, 32, 64, 128}; dim_feedforward a multiple of 32, <= 8192 (beyond d_model + dim_feedforward = 1536 the decode step runs without folded LayerNorms, beyond
 * dim_feedforward = 1536 its linear2 product runs in column ranges of 1024);
 * max_batch 1..256 clips per decode chain (larger batches are sliced by the caller, video2music_amd/model). */
amt_status amt_create(const amt_config* cfg, amt_handle** out);
amt_status amt_destroy(amt_handle* h);
/* One state_dict entry (reference key names).  `data` may be a host or a
 * device pointer; `shape` has `ndim` entries.  Replaces nn.Module.load_state_dict (generate.py:216). */
amt_status amt_load_weight(amt_handle* h, const char* name, const float* data, int32_t ndim, const int64_t* shape);
/* Validates that every tensor of the hot path is present with the right shape and builds the
 * derived layouts (MFMA-ordered decode weights, Linear_chord tables).  Synchronises the device. */
amt_status amt_finalize(amt_handle* h);

/* ---- VideoMusicTransformer.forward pieces ------------------------------------------------ */
/* Video stream + encoder + per-layer cross-attention K/V (video_music_transformer.py:1005-1033,
 * torch nn.TransformerEncoder).  sem (B,S,sem_dim), scene (B,S), motion (B,S,motion_dim) with
 * motion_dim=1 for the scalar form, emotion (B,S,emo_dim).  Optionally copies the encoder memory
 * (B,S,d) to memory_out.  The handle keeps memory / K / V for amt_prefill and amt_generate. */
amt_status amt_encode(amt_handle* h, int32_t B, int32_t S,
                      const float* sem, int32_t sem_dim, const float* scene,
                      const float* motion, int32_t motion_dim, const float* emotion, int32_t emo_dim,
                      float* memory_out, void* stream);
/* Teacher-forced decoder pass (video_music_transformer.py:984-1001,1027-1044; rpr.py:24-70) over
 * the clips of the last amt_encode: root/attr ids (B,L) int64, key (B) -> logits (B,L,159).
 * layer_out (optional) receives the output of decoder layer `layer_index` (B,L,d). */
amt_status amt_prefill(amt_handle* h, int32_t B, int32_t L, const int64_t* root_ids, const int64_t* attr_ids,
                       const float* key, float* logits_out, float* layer_out, int32_t layer_index, void* stream);

/* ---- VideoMusicTransformer.generate (video_music_transformer.py:1046-1132), batched ------ */
/* Starts a generation over the B clips of the last amt_encode.  primer* are (B,P) int64 when
 * primer_per_clip != 0, else (P) shared by all clips.  beam: 0 = sampling branch, 1 = verbatim
 * top-1 branch.  Resets the KV cache and the device position counter. */
amt_status amt_generate_begin(amt_handle* h, int32_t B, const int64_t* primer, const int64_t* primer_root,
                              const int64_t* primer_attr, int32_t P, int32_t primer_per_clip, const float* key,
                              int32_t T, int32_t beam, int32_t max_conseq_N, int32_t max_conseq_chord, void* stream);
/* Switches the sampling branch (beam=0) of the generation in progress from the arg-max decision to the
 * reference's Categorical draw (video_music_transformer.py:1104-1105), done on device by inverse CDF:
 * uniforms is (T,B) fp32 in [0,1), device memory, copied; the token decided from input position t of clip b
 * is the first id whose cumulative masked probability reaches uniforms[t*B+b] * sum.  null switches back.
 * amt_generate_begin resets to arg-max. */
amt_status amt_generate_set_uniforms(amt_handle* h, const float* uniforms, void* stream);
/* Runs `n_steps` decode steps with the arg-max sampler on device (hipGraph replay; oracle G2 for
 * beam=0, G1 for beam=1).  logits_out (optional) is (T,B,159): row t = logits computed from input
 * position t.  n_steps < 0 runs to the end (T-1 steps in total). */
amt_status amt_generate_run(amt_handle* h, int32_t n_steps, float* logits_out, void* stream);
/* Same steps as amt_generate_run, issued eagerly with a HIP event pair recorded on `stream` around
 * every kernel launch (synchronises once per step).  Accumulates, per kernel class
 * {0: self-attention decode, 1: cross-attention decode, 2: skinny GEMMs, 3: sampling head,
 * 4: an EMPTY event pair per step = the overhead of the two records, to be subtracted}, the
 * summed pair durations (ms) and counts (arrays of 5), and for classes 0/1 the algorithmic K/V bytes
 * (fp32 K and V rows of the keys each launch must read).  Used by bench.py's roofline leg. */
/* Options of the base model that change the input tables (before the first amt_finalize).
 *   "chord_embed" = 1: reference chord_embed=True (model/video_music_transformer.py:931-937, 986-987): the chord id indexes a frozen
 *   table instead of root + attr embeddings.  The caller uploads that table (n_rows, d) under the name "embedding_root.weight" and
 *   an all-zero (16, d) "embedding_attr.weight", passes chord ids as the root ids and zeros as the attr ids; the generated id then
 *   feeds back as the root index in both decision branches. */
/*   "causal_mask" = 0 (any time): amt_prefill runs the decoder self-attention without the subsequent mask (reference
 *   forward(mask=False), :978-982); 1 restores the default.
 *   "decode_chain_plain" = 1 (before the first amt_finalize): the decode step without folded LayerNorms (49 launches instead of
 *   31: model/rpr.py:59-69 operator by operator) -- the chain that shapes outside the fold's range take anyway.
 *   "fuse_sampling_head" = 0 (any time): every step of a captured decode graph ends with its own sampling-head launch (31 launches
 *   per step); 1, the default: inside a graph the head rides in the prologue of the next step's first self-attention (30).
 *   "short_context_attn" = 0 (any time): every captured decode graph uses the long-context self-attention kernels; 1, the default:
 *   a graph whose last step still has at most one K/V batch of keys (128 at head_dim 64) takes the short-context instantiations
 *   (DESIGN.md §5).  Results are bit-identical either way.
 *   "gemm_tile_pipeline" = 0 (any time): the skinny GEMMs of the decode step run their serial tile loop; 1, the default: the pipelined
 *   one (wave-uniform control, next k-tile's LDS reads and folded-FFN fix under this tile's MFMAs).  Part of the key of
 *   a captured graph; results are bit-identical either way.
 *   "gemm_scalar_front" = 0 (any time): the skinny GEMMs of the decode step keep their generic front; 1, the default: the launches
 *   of the folded step take the lean front (row, tile and weight addresses worked out on the scalar unit from one block of kernel
 *   arguments).
 *   Part of the key of a captured graph; results are bit-identical either way.
 *   "gemm_rows_dma" = 0 (any time): every row chunk of the decode step's skinny GEMMs goes through registers and a ds_write; 1, the
 *   default: the lean-front launches request the chunks that nothing is done to on their way (all of a plain launch's; behind the
 *   folded-FFN prologue the raw columns, when K1 = 2 (K - K1)) by LDS-DMA, straight into the staged row.  Part of the
 *   key of a captured graph; results are bit-identical either way.  With a NULL handle the option sets the process-wide default of
 *   the entry points that carry no handle (amt_decode_gemm_ex_fwd; initially 1 as well); a launch takes the DMA form when neither
 *   its handle (or AMT_GEMM_PRO_REG_ROWS) nor, without a handle, the process-wide default says otherwise.
 *   "scalar_key_stream" = 0 (any time): the decode attentions of this handle keep the per-lane controlled key stream (every load
 *   clamped, every key guarded, one batch requested past a wave's last); 1, the default: the scalar-controlled one (per wave a scalar
 *   batch count, buffer loads on a scalar base, nothing requested behind the last batch).  Part of the key of a captured
 *   graph; results are bit-identical either way.  With a NULL handle the option sets the process-wide default instead, which the
 *   operator entry points (amt_attn_decode_fwd, amt_attn_decode_fold_fwd) and the lockstep step (amt_v2_step*) follow: they carry no
 *   handle.  A launch runs the scalar stream when neither its handle (or its new_kv bit 2) nor the process-wide default says otherwise.
 *   "profile_skip" = 1 | 2 | 3 (any time; results become meaningless): measurement hook of bench.py, leaves the self-attention
 *   (bit 0) and / or cross-attention (bit 1) launches out of the captured decode step, so that what a kernel costs the step is
 *   the difference between two timed generates.  0 restores the real step. */
amt_status amt_set_option(amt_handle* h, const char* name, int32_t value);
/* amt_encode with rows [B*S][d] added to Linear_vis's output before the encoder: reference scene_embed=True
 * (:1016-1027: the scene offset is left out of the feature columns and scene_embedding(offset.int()) is added instead).  The
 * caller keeps the scene column in the features and uploads Linear_vis.weight with a zero column at its position. */
amt_status amt_encode_resid(amt_handle* h, int32_t B, int32_t S, const float* sem, int32_t sem_dim, const float* scene,
                            const float* motion, int32_t motion_dim, const float* emotion, int32_t emo_dim,
                            const float* vis_resid, float* memory_out, void* stream);
amt_status amt_generate_profile(amt_handle* h, int32_t n_steps, double* ms_by_class, int64_t* launches_by_class,
                                int64_t* attn_bytes_by_class, void* stream);
/* One decode step that stops before the decision: writes the decision distribution
 * softmax(logits)[:157] with the suppressions applied, (B,157), for a host-side sampler
 * (torch.multinomial = the reference's Categorical.sample), then amt_generate_commit feeds the
 * chosen ids (B) int64 back. */
amt_status amt_generate_step_probs(amt_handle* h, float* probs_out, void* stream);
amt_status amt_generate_commit(amt_handle* h, const int64_t* chosen, void* stream);
/* Between the steps of a host-driven generation (amt_generate_step_probs / amt_generate_commit): the branch of the following
 * steps, 0 = sampling branch (suppressions applied to the distribution, the committed id feeds back as root / attr), 1 = top-k
 * branch (plain softmax[:157], root / attr of the committed position stay PAD).  This is the per-step choice
 * `random.uniform(0,1) <= beam_chance` of model/video_music_transformer.py:1074-1084; the host keeps the `beam` rows. */
amt_status amt_generate_set_branch(amt_handle* h, int32_t beam);
/* Test access to the self-attention K/V cache, fp32 [2 (K, V)][n_layers][max_batch][H][rows][hd] with rows = max_sequence_chord plus
 * the padding rows of DESIGN.md §4: dims_out (optional, 6 values) receives the shape; buf (optional, n_floats = their product, device
 * memory) receives the cache (write = 0) or replaces it (write = 1). */
amt_status amt_kv_cache_io(amt_handle* h, float* buf, int64_t n_floats, int32_t write, int64_t* dims_out, void* stream);
/* Copies the (B,T) int64 token matrix (PAD=158 beyond the generated length) to tokens_out. */
amt_status amt_generate_end(amt_handle* h, int64_t* tokens_out, void* stream);
/* begin + run(-1) + end. */
amt_status amt_generate(amt_handle* h, int32_t B, const int64_t* primer, const int64_t* primer_root,
                        const int64_t* primer_attr, int32_t P, int32_t primer_per_clip, const float* key,
                        int32_t T, int32_t beam, int32_t max_conseq_N, int32_t max_conseq_chord,
                        int64_t* tokens_out, float* logits_out, void* stream);
/* Timing/roofline introspection for bench.py: algorithmic HBM bytes of the decode-attention
 * launches of one step at key count n_keys (self) — see DESIGN.md. */
int64_t amt_decode_step_bytes(const amt_handle* h, int32_t B, int32_t n_self_keys, int32_t S);

/* ---- stateless operator entry points (used by the parity tests and standalone modules) --- */
/* y[M,N] = x[M,K] . w[N,K]^T + bias (+ resid) ; optional ReLU.  torch.nn.functional.linear. K % 32 == 0. */
amt_status amt_linear_fwd(const float* x, const float* w, const float* bias, const float* resid, float* y,
                          int32_t M, int32_t N, int32_t K, int32_t relu, void* stream);
/* y = LayerNorm(x (+ resid)) (torch.nn.LayerNorm; rpr.py:59-69). */
amt_status amt_layernorm_fwd(const float* x, const float* resid, const float* w, const float* b, float* y,
                             int32_t rows, int32_t dim, float eps, void* stream);
/* RMSNorm.forward (custom_transformer.py:38-45); w may be null. */
amt_status amt_rmsnorm_fwd(const float* x, const float* w, float* y, int32_t rows, int32_t dim, float eps, void* stream);
/* Tail of DifferentialMultiheadAttention (custom_transformer.py:818-826; VideoMusicTransformer_V3): with o1 / o2 the
 * attention outputs of the even / odd heads of a pair over the same values, y = RMSNorm_hd(o1 - lambda_full * o2) * w *
 * out_scale (out_scale = 1 - lambda_init), rows of hd <= 128 values. */
amt_status amt_diff_subln_fwd(const float* o1, const float* o2, const float* w, float* y, int32_t rows, int32_t hd,
                              float lambda_full, float out_scale, float eps, void* stream);
/* y = a + b over n floats (n % 4 == 0): the residual add of the pre-norm layers (custom_transformer.py:1241-1249). */
amt_status amt_add_fwd(const float* a, const float* b, float* y, int64_t n, void* stream);
/* y[r][:] = x[r][:] * row_scale[r] (+ add[r][:] when add != null): the video rows dropped by dropTokenRate in the V1 / V2 / V3
 * classes (model/video_music_transformer.py:193-197, 488-492, 798-802: vf * (rand(B,S) > rate), also in eval mode), with the
 * positional rows that follow (:208) as `add`.  dim a multiple of 4. */
amt_status amt_row_scale_add_fwd(const float* x, const float* row_scale, const float* add, float* y, int32_t rows, int32_t dim,
                                 void* stream);
/* RMSNorm(x + resid): the post-norm residual form of the custom layers (custom_transformer.py:1233-1240); resid may be null. */
amt_status amt_rmsnorm_resid_fwd(const float* x, const float* resid, const float* w, float* y, int32_t rows, int32_t dim,
                                 float eps, void* stream);
/* RotaryPositionalEmbeddings.forward (rotate_operation.py:111-165), input_pos=None: x is
 * (n0, seq, n2, hd); cache is the module's (max_seq, cache_half, 2) buffer. */
amt_status amt_rope_fwd(const float* x, const float* cache, float* y, int32_t n0, int32_t seq, int32_t n2, int32_t hd,
                        int32_t cache_half, void* stream);
/* Core of multi_head_attention_forward_rpr (rpr.py:387-414) after the projections: q (already
 * scaled), k, v are (B,L,H*hd) row-major; Er (er_len,hd); causal.  o (B,L,H*hd). */
amt_status amt_rpr_attn_fwd(const float* q, const float* k, const float* v, const float* Er, float* o,
                            int32_t B, int32_t H, int32_t L, int32_t hd, int32_t er_len, void* stream);
/* Core of torch MultiheadAttention as used at rpr.py:62-63 / the video encoder: q (B,Lq,H*hd)
 * scaled, k,v (B,Lk,H*hd); no mask (causal=0) or causal. */
/* The same attention without the causal mask (forward(mask=False), model/video_music_transformer.py:978-982): every key is
 * visible; the relative term stays zero for keys j > i, which is what model/rpr.py:439-455 (_skew) produces. */
amt_status amt_rpr_attn_nomask_fwd(const float* q, const float* k, const float* v, const float* Er, float* o,
                                   int32_t B, int32_t H, int32_t L, int32_t hd, int32_t er_len, void* stream);
amt_status amt_cross_attn_fwd(const float* q, const float* k, const float* v, float* o,
                              int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd, int32_t causal, void* stream);
/* General strided form of the same kernel (used by the V2 stack and MultiheadGQA): tensor[b][h][l][c] lives at
 * base + b*bs + h*hs + l*ls + c with strides = {q_bs,q_hs,q_ls, k_bs,k_hs,k_ls, v_bs,v_hs,v_ls, o_bs,o_hs,o_ls} in
 * elements; q_scale multiplies q (torch MHA: hd^-0.5; 0 = 1); query head h reads kv head h / kv_group. */
amt_status amt_attn_fwd(const float* q, const float* k, const float* v, float* o, const int64_t* strides,
                        int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd, int32_t causal, int32_t kv_group,
                        float q_scale, void* stream);
/* Input stage pieces of forward (video_music_transformer.py:984-1030): out[row][0:ld_out] = [sem | scene | motion |
 * emotion | 0-pad]; xf[b*L+l] = PR[root] + PA[attr] + key[b]*wkey + bias + pe[l] with PR = E_root.Wc[:, :d]^T etc. */
amt_status amt_concat_features_fwd(const float* sem, int32_t sem_dim, const float* scene, const float* motion, int32_t motion_dim,
                                   const float* emotion, int32_t emo_dim, float* out, int32_t rows, int32_t ld_out, void* stream);
amt_status amt_chord_embed_fwd(const int64_t* root, const int64_t* attr, const float* key, const float* PR, const float* PA,
                               const float* wkey, const float* bias, const float* pe, float* out,
                               int32_t B, int32_t L, int32_t d, void* stream);
/* Decode-step forms: q (B,H*hd) for the token at position pos (host value), K/V caches
 * (B,H,cap,hd); keys 0..pos.  Er may be null (cross-attention: pass pos = S-1). */
amt_status amt_attn_decode_fwd(const float* q, const float* kcache, const float* vcache, const float* Er, float* o,
                               int32_t B, int32_t H, int32_t hd, int32_t cap, int32_t pos, int32_t er_len, void* stream);
/* Decode-step projection: y[B,N] = LN?(x)[B,K] . w[N,K]^T + bias (+resid)(relu); packs w on the fly
 * into `w_packed_scratch` (N_pad16*K floats).  ln_w/ln_b may be null.  B <= 32, K % 64 == 0. */
amt_status amt_decode_linear_fwd(const float* x, const float* w, const float* bias, const float* ln_w, const float* ln_b,
                                 const float* resid, float* y, float* xn_out, float* w_packed_scratch,
                                 int32_t B, int32_t N, int32_t K, int32_t relu, float eps, void* stream);
/* The two kernels of the decode step in the form the handle uses them, with a LayerNorm folded through the projection
 * (reference rpr.py:59-69 computes LayerNorm(u) then the projection):
 * amt_attn_decode_fold_fwd: raw (B, ldq) = u . (W o gamma)^T, columns [0,d) query (and [d,2d) key, [2d,3d) value of the new
 *   position when new_kv = 1); u (B, d) the pre-LayerNorm sum; q = ((raw - mu*fold_g) * rstd + fold_c) * q_scale with the row
 *   statistics of u; xn_out (optional) = LayerNorm(u).  new_kv = 1 also writes the key/value of position *pos_dev into the
 *   caches and attends keys 0..pos; new_kv = 0 attends keys 0..n_keys-1 (cross-attention).  new_kv | 2 (Er given): the
 *   short-context instantiation of the relative-position self-attention, bit-identical to the long one at any length; with it u
 *   may be null: raw is then the finished query (B, H*hd) as amt_attn_decode_fwd takes it, keys 0..*pos_dev or 0..n_keys-1.
 *   new_kv | 4: the per-lane controlled key stream instead of the scalar-controlled one (bit-identical; see "scalar_key_stream"); with
 *   it u may be null as well, with or without Er (the plain self- and cross-attention on that stream).
 * amt_decode_gemm_ex_fwd: rows [x (K1 columns) | x2 (K-K1 columns)]; y_low (B, n_low) = act(x . w_low^T + b (+resid)) over the
 *   first K1 columns (all K when x2 is null), y_high (B, n_high) = [x|x2] . w_high^T + b_high.  pro = 1: the staged row is
 *   [relu((x - mu*fold_g)*rstd + fold_c) | LayerNorm(x2)] (statistics of x2's row) and LayerNorm(x2) is y_low's residual.
 *   Weights are given in nn.Linear layout and packed into the scratch buffers (ceil(n/16)*16*K floats each). */
amt_status amt_attn_decode_fold_fwd(const float* raw, int32_t ldq, float* kcache, float* vcache, const float* Er,
                                    const float* u, const float* fold_g, const float* fold_c, const float* ln_w,
                                    const float* ln_b, float* xn_out, float* o, int32_t B, int32_t H, int32_t hd,
                                    int32_t cap, const int32_t* pos_dev, int32_t n_keys, int32_t er_len, int32_t new_kv,
                                    float eps, float q_scale, void* stream);
/* Bit of amt_decode_gemm_args.pro: run the kernel's serial tile loop (LDS read, fix, four MFMAs per k-tile, one after the other) instead
 * of the pipelined one (next tile's reads and fix under this tile's MFMAs).  Same arithmetic in the same order: y_low / y_high are
 * bit-identical either way. */
#define AMT_GEMM_PRO_SERIAL_LOOP 0x100
/* Bit of amt_decode_gemm_args.pro: keep the kernel's generic front (per-lane 64-bit addresses, options decided at run time) where
 * the launch would take the lean one (wave-uniform address work on the scalar unit; see "gemm_scalar_front").  The serial loop
 * implies it.  What is loaded and summed is the same: y_low / y_high are bit-identical either way. */
#define AMT_GEMM_PRO_GENERIC_FRONT 0x200
/* Bit of amt_decode_gemm_args.pro: stage every row chunk through registers where the launch would request it by LDS-DMA (see
 * "gemm_rows_dma").  Only the data path differs: y_low / y_high are bit-identical either way. */
#define AMT_GEMM_PRO_REG_ROWS 0x400
typedef struct amt_decode_gemm_args {
    const float* x;  int32_t ldx;          /* first K1 columns of the rows (all K when x2 is null) */
    const float* x2; int32_t ldx2;         /* remaining K - K1 columns, or null */
    int32_t K1, K;
    const float* w_low;  const float* bias_low;  const float* resid; int32_t relu;   /* y_low = act(x . w_low^T + b (+ resid)) */
    const float* w_high; const float* bias_high;                                     /* y_high = [x | x2] . w_high^T + b_high */
    int32_t n_low, n_high;
    int32_t pro;                           /* 1: folded-FFN prologue (see above); | AMT_GEMM_PRO_SERIAL_LOOP: the serial tile loop; | AMT_GEMM_PRO_GENERIC_FRONT; | AMT_GEMM_PRO_REG_ROWS */
    const float* fold_g; const float* fold_c; const float* ln_w; const float* ln_b;
    float* y_low; float* y_high;
    float* scratch_low; float* scratch_high;   /* packed copies of the weights, ceil(n/16)*16*K floats each */
    int32_t B; float eps;
} amt_decode_gemm_args;
amt_status amt_decode_gemm_ex_fwd(const amt_decode_gemm_args* a, void* stream);
/* Whether amt_decode_gemm_ex_fwd would run this argument block on the kernel's lean front: 1 yes, 0 the generic front (a shape or
 * option outside the lean front's range, or one of the two bits above), negative for a block amt_decode_gemm_ex_fwd refuses.  The
 * launcher's own rule, evaluated on the host: no device, no stream, nothing is read through the pointers; a code, not a status. */
int32_t amt_decode_gemm_ex_lean(const amt_decode_gemm_args* a);
/* MultiheadGQA.forward (grouped_query_attention.py:286-358) without RoPE: query/key/value are the
 * caller's (L,B,E) buffers, weights in nn.Linear layout; scratch >= 4*L*B*E floats. */
amt_status amt_gqa_fwd(const float* query, const float* key, const float* value,
                       const float* wq, const float* bq, const float* wk, const float* bk, const float* wv, const float* bv,
                       const float* ln_w, const float* ln_b, const float* wo, const float* bo,
                       float* out, float* scratch, int32_t L, int32_t S, int32_t B, int32_t E, int32_t query_heads,
                       int32_t kv_heads, int32_t is_causal, float ln_eps, void* stream);
/* The same with MultiheadGQA(RoPE=...) (grouped_query_attention.py:316-322): the projected q and k are rotated through the raw
 * (heads, len, B, head_dim) view with the module's cos/sin cache (cache_rows, cache_half, 2) -- cache_half = dim/2 of the
 * RotaryPositionalEmbeddings the caller built, head_dim/2 or a multiple that the view folds (rotate_operation.py:148-149). */
amt_status amt_gqa_rope_fwd(const float* query, const float* key, const float* value,
                            const float* wq, const float* bq, const float* wk, const float* bk, const float* wv, const float* bv,
                            const float* ln_w, const float* ln_b, const float* wo, const float* bo,
                            float* out, float* scratch, int32_t L, int32_t S, int32_t B, int32_t E, int32_t query_heads,
                            int32_t kv_heads, int32_t is_causal, float ln_eps, const float* rope_cache, int32_t cache_rows,
                            int32_t cache_half, void* stream);
/* MoELayer.forward / SharedMoELayer.forward, eval mode (moe.py:167-200,231-302): x (n_tok,d);
 * gate (n_exp,d)+(n_exp); experts' linear1/gate (n_exp,dff,d)+(n_exp,dff), linear2 (n_exp,d,dff)+(n_exp,d);
 * shared_* may be null.  top-k = 2.  idx_out/w_out (optional) receive the routing (n_tok,2).
 * scratch: see amt_moe_scratch_floats. */
int64_t amt_moe_scratch_floats(int32_t n_tok, int32_t d, int32_t dff, int32_t n_exp);
amt_status amt_moe_fwd(const float* x, const float* gate_w, const float* gate_b,
                       const float* w1, const float* b1, const float* wg, const float* bg, const float* w2, const float* b2,
                       const float* sw1, const float* sb1, const float* swg, const float* sbg, const float* sw2, const float* sb2,
                       float* out, int32_t* idx_out, float* w_out, float* scratch,
                       int32_t n_tok, int32_t d, int32_t dff, int32_t n_exp, void* stream);
/* The same layer with n_experts_per_token = k, 1 <= k <= 8 (MoELayer / SharedMoELayer constructor argument, moe.py:150-160,202-215; every
 * reference model passes 2): idx_out / w_out are (n_tok, k), the shared expert enters with 1/k; scratch from amt_moe_topk_scratch_floats. */
int64_t amt_moe_topk_scratch_floats(int32_t n_tok, int32_t d, int32_t dff, int32_t n_exp, int32_t k);
amt_status amt_moe_topk_fwd(const float* x, const float* gate_w, const float* gate_b,
                    const float* w1, const float* b1, const float* wg, const float* bg, const float* w2, const float* b2,
                    const float* sw1, const float* sb1, const float* swg, const float* sbg, const float* sw2, const float* sb2,
                    float* out, int32_t* idx_out, float* w_out, float* scratch,
                    int32_t n_tok, int32_t d, int32_t dff, int32_t n_exp, int32_t k, void* stream);

/* Training of the same layer (csrc/moe_bwd.hip).  amt_moe_train_fwd issues amt_moe_topk_fwd's launches (the fused gate of the up
 * projection becomes a launch of its own, so that the up branch can be kept) and leaves in the caller-owned `saved`
 * (amt_moe_train_scratch_floats; glu = 1 when w1 is given) what amt_moe_bwd reads: per slot row of the plan G (gate pre-activation), U
 * (the up branch before gating, GLU experts only), H (as fed to the down projection, dropout multiplier included) and Y (as it enters
 * the combine: output dropout multiplier included); the same four of the shared expert; perm, slot_pos, tile_group, the slot ->
 * assignment map, the segment offsets; idx and wts (also copied to idx_out / w_out when given).
 * Dropout multipliers (0 or 1 / (1 - p)), each optional, indexed by ASSIGNMENT a = token * k + j (j the position in idx_out's order):
 * mask_h (n_tok k, dff_raw) on U silu(G) (silu(G) for SiLU experts), mask_y (n_tok k, d) on the expert's output before the routing
 * weight, mask_hs (n_tok, dff_raw) inside the shared expert.  dff_raw <= dff: the experts' own hidden width (dff its zero-padded
 * multiple of 32).  With the three masks null, out / idx_out / w_out are the bits of amt_moe_topk_fwd.
 * amt_moe_bwd: dout (n_tok, d) -> dx (n_tok, d), dgate_w (n_exp, d), dgate_b (n_exp), dw1 (n_exp, dff, d; null for SiLU experts) db1
 * (n_exp, dff) dwg dbg dw2 (n_exp, d, dff) db2 (n_exp, d) and the shared expert's six (null without one), all at the padded width dff
 * (the padding's rows / columns come out zero).  w1t / wgt (n_exp, d, dff) and w2t (n_exp, dff, d) are the TRANSPOSED stacked weights
 * (sw1t, swgt (d, dff), sw2t (dff, d) the shared expert's), prepared by the caller.  An expert without rows gets exact zeros.  No
 * floating-point atomics and a fixed order of every sum: the same inputs give the same bits.  ws: amt_moe_bwd_ws_floats. */
int64_t amt_moe_train_scratch_floats(int32_t n_tok, int32_t d, int32_t dff, int32_t n_exp, int32_t k, int32_t glu);
amt_status amt_moe_train_fwd(const float* x, const float* gate_w, const float* gate_b,
                    const float* w1, const float* b1, const float* wg, const float* bg, const float* w2, const float* b2,
                    const float* sw1, const float* sb1, const float* swg, const float* sbg, const float* sw2, const float* sb2,
                    const float* mask_h, const float* mask_y, const float* mask_hs,
                    float* out, int32_t* idx_out, float* w_out, float* saved,
                    int32_t n_tok, int32_t d, int32_t dff, int32_t dff_raw, int32_t n_exp, int32_t k, void* stream);
int64_t amt_moe_bwd_ws_floats(int32_t n_tok, int32_t d, int32_t dff, int32_t n_exp, int32_t k);
amt_status amt_moe_bwd(const float* dout, const float* x, const float* gate_w, const float* saved,
                       const float* w1t, const float* wgt, const float* w2t, const float* sw1t, const float* swgt, const float* sw2t,
                       const float* mask_h, const float* mask_y, const float* mask_hs,
                       float* dx, float* dgate_w, float* dgate_b,
                       float* dw1, float* db1, float* dwg, float* dbg, float* dw2, float* db2,
                       float* dsw1, float* dsb1, float* dswg, float* dsbg, float* dsw2, float* dsb2,
                       float* ws, int32_t n_tok, int32_t d, int32_t dff, int32_t dff_raw, int32_t n_exp, int32_t k, int32_t glu,
                       int32_t has_shared, float temperature, void* stream);
/* amt_moe_train_fwd for SharedMoELayer(balancing=True) in training mode (moe.py:257-279): amt_moe_train_fwd's arguments, then
 * sel_bias (n_exp), update_rate and bias_delta (n_exp).  The k experts of a token are those with the largest logit + sel_bias[e],
 * largest first and the lower expert id first among equals; idx keeps that order; wts is the softmax over the RAW logits of those k,
 * their own maximum subtracted.  Plan, grouped GEMMs, combine and `saved` are amt_moe_train_fwd's, and amt_moe_bwd reads `saved` as it
 * is: the bias has no gradient.  bias_delta[e] = update_rate (mean(c) - c[e]) with c the plan's integer rows per expert as fp32 and
 * mean(c) = (sum c) / n_exp in fp32: what the caller adds to its bias buffer (the library keeps no state).  With sel_bias all zero
 * out / idx_out / w_out / saved are the bits of amt_moe_train_fwd. */
amt_status amt_moe_train_fwd_balanced(const float* x, const float* gate_w, const float* gate_b,
                    const float* w1, const float* b1, const float* wg, const float* bg, const float* w2, const float* b2,
                    const float* sw1, const float* sb1, const float* swg, const float* sbg, const float* sw2, const float* sb2,
                    const float* mask_h, const float* mask_y, const float* mask_hs,
                    float* out, int32_t* idx_out, float* w_out, float* saved,
                    int32_t n_tok, int32_t d, int32_t dff, int32_t dff_raw, int32_t n_exp, int32_t k, void* stream,
                    const float* sel_bias, float update_rate, float* bias_delta);
/* Into how many runs amt_moe_bwd cuts each group's 128-row tiles in its weight-gradient products for this shape (1: no second pass):
 * dense = 0 the experts' products over the plan's k n_tok assignments, dense != 0 the one-group products over the tokens (shared
 * expert, router).  The launcher's own plan function, evaluated on the host: no device, no stream; a count, not a status; negative
 * for a shape amt_moe_bwd refuses. */
int32_t amt_moe_wgrad_splits(int32_t n_tok, int32_t d, int32_t dff, int32_t n_exp, int32_t k, int32_t dense);

/* Pieces of the same layer for expert-parallel execution (config 5: one expert group per GPU; the token rows
 * travel by all_to_all between amt_moe_route_fwd and amt_moe_combine_fwd, see video2music_amd/model/moe.py):
 * router (moe.py:180-190), one GLUExpert on n rows (moe.py:44-49; scratch >= 2*n*dff floats), and the
 * weighted sum out[t] = w0*y[slot_pos[t,0]] + w1*y[slot_pos[t,1]] in expert-index order (+ shared_scale*shared). */
amt_status amt_moe_route_fwd(const float* x, const float* gate_w, const float* gate_b, int32_t* idx_out, float* w_out,
                             int32_t n_tok, int32_t d, int32_t n_exp, void* stream);
amt_status amt_glu_expert_fwd(const float* x, const float* w1, const float* b1, const float* wg, const float* bg,
                              const float* w2, const float* b2, float* out, float* scratch,
                              int32_t n, int32_t d, int32_t dff, void* stream);
amt_status amt_moe_combine_fwd(const float* y_rows, const int32_t* slot_pos, const int32_t* idx, const float* wts,
                               const float* shared, float shared_scale, float* out, int32_t n_tok, int32_t d, void* stream);
/* Expert-parallel execution with the plans on the DEVICE (video2music_amd/model/moe.py:expert_parallel_moe):
 * amt_moe_ep_dispatch_plan_fwd: from one rank's routing idx[2*n_tok] the rows per expert counts_out[n_exp], the send-buffer order
 *   perm[2*n_tok] (send row -> token; ordered by expert, exact packing, so the rows of one destination rank are contiguous) and
 *   slot_pos[2*n_tok] (assignment token*2+slot -> send row: what amt_moe_combine_fwd takes).  ints: >= 256 int32 of scratch, zero
 *   before the first call.
 * amt_gather_rows_fwd: dst[i] = src[index[i]] (a negative index gives a zero row): the send buffer x[perm].
 * amt_moe_ep_expert_fwd: the rank's e_local experts (stacked tensors as amt_moe_fwd takes them) on the n_recv rows the all_to_all
 *   delivered, grouped by (source rank, local expert) with the segment sizes in DEVICE memory recv_counts[world][e_local]; results
 *   y_out[n_recv][d] in arrival order.  One grouped GEMM launch per projection; scratch: amt_moe_ep_expert_scratch_floats. */
amt_status amt_moe_ep_dispatch_plan_fwd(const int32_t* idx, int32_t n_tok, int32_t n_exp, int32_t* counts_out, int32_t* perm,
                                        int32_t* slot_pos, int32_t* ints, void* stream);
amt_status amt_gather_rows_fwd(const float* src, const int32_t* index, float* dst, int32_t n_rows, int32_t d, void* stream);
int64_t amt_moe_ep_expert_scratch_floats(int32_t n_recv, int32_t d, int32_t dff, int32_t e_local);
amt_status amt_moe_ep_expert_fwd(const float* rows, const int32_t* recv_counts, int32_t world, int32_t e_local, int32_t n_recv,
                                 const float* w1, const float* b1, const float* wg, const float* bg, const float* w2, const float* b2,
                                 float* y_out, float* scratch, int32_t d, int32_t dff, void* stream);

/* ---- VideoMusicTransformer_V2 '2.2': one KV-cached decode step of one clip ------------------------
 * Issues, from one call, the launch sequence of the decoder restricted to position t (reference
 * video_music_transformer.py:437-516, custom_transformer.py:1250-1292): embedding of (root, attr, key), per layer RoPE
 * self-attention over the cache (appends row t), RoPE cross-attention over the clip's video keys, GLU expert or
 * SharedMoE(top-2), post-norm LayerNorms; decoder.norm; Wout -> logits_out[159].
 * Every projection handles one row, so it runs on the skinny decode GEMM over weights packed once by
 * amt_pack_weight_fwd (out: ceil(N/16)*16*K floats; the experts of a MoE layer are packed one after the other).
 * tab: device pointers, 11 global (PR, PA, wkey, Linear_chord.bias, rope cache (max_seq, E/2, 2) or null = no rotation,
 * decoder.norm w, b, packed Wout, Wout b, an int32 pair {0, 1}, learned positional table (max_seq, E) added to the
 * embedding of position t or null: version '2.0' has the table and no rotation, :375-380,497-503) then 48 per layer (packed self in_proj, its bias, packed out_proj, b,
 * norm1 w, b, packed cross in_proj rows 0:E, its bias, packed out_proj, b, norm2 w, b, norm3 w, b, self K cache, V cache
 * (head-major: H, max_seq, hd), cross K (roped), V (head-major: H, S, hd), router w (null = plain GLU layer), router b, packed linear1, b, packed gate, b,
 * packed linear2, b (per expert, stacked, for a MoE layer), shared expert's six tensors (packed weights) or null; then, for the
 * lockstep step, the stacked forms: packed [gate of every expert (+ the shared one) | linear1 of every expert (+ shared)] as one matrix
 * -- with linear1 present its rows are interleaved in eights BEFORE packing (gate rows 8T..8T+7, then linear1 rows 8T..8T+7, T = 0, 1, ...:
 * the product's epilogue writes linear1 * silu(gate) itself) -- and its bias in the stacked order [gate | linear1], packed linear2 of every expert (+ shared) one after the other and their biases (both null for a plain GLU layer,
 * whose linear2 is the per-layer entry above); last, for the lockstep step with norm1 folded through the cross-attention's query
 * projection (all four null: separate launches): packed [(Wq o gamma1) Wo | Wq o gamma1] (E x 2E), its bias (Wq o gamma1) bo,
 * g = rowsum(Wq o gamma1), c = Wq beta1 + bq  (Wo, bo: self-attention out-projection; Wq, bq: cross in_proj rows 0:E)); and, for
 * a plain GLU layer of the lockstep step with norm2 and norm3 folded (all eight null: separate launches; E and dff multiples of
 * 256, dff + E <= 1536): packed [(Wgu o gamma2) Wo | Wgu o gamma2] (2 dff x 2E; Wgu = [gate; linear1], Wo the cross-attention's
 * out-projection), its bias (Wgu o gamma2) bo, g = rowsum(Wgu o gamma2), c = Wgu beta2 + bgu, then -- null in the last layer --
 * packed [(Wn o gamma3) W2 | Wn o gamma3] (3E x (dff + E); Wn the NEXT layer's self in_proj, W2 this layer's linear2), its bias
 * (Wn o gamma3) b2, g = rowsum(Wn o gamma3), c = Wn beta3 + bn.
 * A null norm bias selects RMSNorm (eps 1e-6) for that norm; a null linear1 selects Linear -> SiLU -> Linear experts
 * (h = silu(gate-slot projection)): the V1 family (video_music_transformer.py:22-314).
 * ws: amt_v2_step_ws_floats(E, dff, n_exp) floats.  E, dff multiples of 64, at most 1536.
 * state_dev (optional): int32 {position, root, attr} in device memory; when given, t / root / attr are read there and the
 * position is incremented at the end of the step, so that one captured graph of the step can be replayed for every token. */
amt_status amt_pack_weight_fwd(const float* w, float* out, int32_t N, int32_t K, void* stream);
int64_t amt_v2_step_ws_floats(int32_t E, int32_t dff, int32_t n_exp);
amt_status amt_v2_step(const void* const* tab, int32_t n_layers, int32_t H, int32_t E, int32_t dff, int32_t n_exp,
                       int32_t S, int32_t max_seq, int32_t t, int32_t root, int32_t attr, float key, const int32_t* state_dev,
                       float* logits_out, float* ws, void* stream);
/* ---- regression head, recurrent variants (video_regression.py:124-135: torch.nn.LSTM / nn.GRU, batch_first) -------------
 * The recurrence of one layer and direction over projected inputs xproj (B, L, ldxp) whose columns [0, gates*d) hold
 * W_ih x + b_ih (gate order of torch: LSTM i,f,g,o; GRU r,z,n): gates = 4 LSTM, 3 GRU; w_hh (gates*d, d), b_hh (gates*d);
 * y (B, L, ldy) receives h_t in columns [0, d) of the pointer given (pass y + d for the reverse direction of a
 * bidirectional layer); reverse = 1 walks t = L-1 .. 0 and writes h at t.  d a multiple of 8, at most 128.
 * n_dirs = 2 runs both directions of a bidirectional layer in one launch: xproj then holds [forward | reverse] projections
 * side by side (2*gates*d columns), w_hh / b_hh the two directions stacked, y gets [h_forward | h_reverse] (2*d columns). */
amt_status amt_rnn_seq_fwd(const float* xproj, int32_t ldxp, const float* w_hh, const float* b_hh, float* y, int32_t ldy,
                           int32_t B, int32_t L, int32_t d, int32_t gates, int32_t reverse, int32_t n_dirs, void* stream);

/* amt_rnn_seq_fwd that also keeps what the backward needs: y is computed by the same arithmetic, bit for bit.
 * reserve (B*L, ldr), ldr >= n_dirs * C * d, row b*L + t, direction dir at columns [dir*C*d, (dir+1)*C*d), in blocks of d:
 *   LSTM (C = 5): i, f, g, o (activated), c_t            GRU (C = 4): r, z, n (activated), W_hn h_{t-1} + b_hn */
amt_status amt_rnn_seq_train_fwd(const float* xproj, int32_t ldxp, const float* w_hh, const float* b_hh, float* y, int32_t ldy,
                                 float* reserve, int32_t ldr, int32_t B, int32_t L, int32_t d, int32_t gates, int32_t reverse,
                                 int32_t n_dirs, void* stream);
/* Backpropagation through time of one layer (one workgroup per clip and direction, W_hh^T in registers, no atomics: the same
 * inputs give the same bits).  dy (B*L, lddy): gradient of y, this layer's n_dirs*d columns; reserve / y as amt_rnn_seq_train_fwd
 * left them; w_hh as there.  dxproj (B*L, ldxp), n_dirs*gates*d columns laid out like xproj: the gradient with respect to the
 * pre-activations as the input side sees them (dW_ih = dxproj^T x, db_ih = column sums, dx = dxproj W_ih), written once per step.
 * LSTM: the hidden side sees the same values (dW_hh = dxproj^T h_prev, db_hh = db_ih); dhn is not used (may be null).
 * GRU: the hidden side's n block is r * (the input side's); it goes to dhn (B*L, lddhn), n_dirs*d columns, required.
 * h_prev is y shifted by one step in the direction's order, zero at its start.  Shapes and caps as amt_rnn_seq_fwd. */
amt_status amt_rnn_seq_bwd(const float* dy, int32_t lddy, const float* reserve, int32_t ldr, const float* y, int32_t ldy,
                           const float* w_hh, float* dxproj, int32_t ldxp, float* dhn, int32_t lddhn, int32_t B, int32_t L,
                           int32_t d, int32_t gates, int32_t reverse, int32_t n_dirs, void* stream);

/* ---- the same recurrences for hidden sizes beyond the register kernels (csrc/rnn_wide.hip) ------------------------------------
 * d a multiple of 32, 32 <= d <= 512 (the lower end overlaps amt_rnn_seq_* on purpose); gates, reverse, n_dirs, B, L and every
 * pointer, layout and leading dimension -- xproj, w_hh, b_hh, y, reserve, dy, dxproj, dhn -- mean what they mean in the three
 * functions above, and the results agree with theirs to rounding (another summation order: the products run on the matrix pipe).
 * One step kernel per time step and call, all on `stream` (L launches; the stream's order is the only synchronisation between
 * steps: no workgroup waits for another); clips beyond 32 are further tiles of the grid.  No allocation, no host
 * synchronisation, no atomics: the same inputs give the same bits; amt_rnn_wide_seq_train_fwd's y equals amt_rnn_wide_seq_fwd's
 * bit for bit.  Columns beyond the used widths are neither read nor written.  Rows that are read back as float4 need 16-byte
 * alignment: y and w_hh (ldy a multiple of 4) in the forwards, dxproj and dhn (ldxp, lddhn multiples of 4) in the backward.
 * ws: amt_rnn_wide_ws_floats(B, d, gates, n_dirs) = B * n_dirs * d floats (-1 for arguments the calls refuse), required by all
 * three, never read before it is written (it need not be zero), free again when the call's launches have run: the eval forward
 * keeps the LSTM's c there, the backward the carried term (LSTM dc f, GRU dh z); the training forward takes c_{t-1} from
 * reserve and leaves ws alone.  Calls that may overlap must not share a ws. */
int64_t amt_rnn_wide_ws_floats(int32_t B, int32_t d, int32_t gates, int32_t n_dirs);
amt_status amt_rnn_wide_seq_fwd(const float* xproj, int32_t ldxp, const float* w_hh, const float* b_hh, float* y, int32_t ldy,
                                int32_t B, int32_t L, int32_t d, int32_t gates, int32_t reverse, int32_t n_dirs, float* ws, void* stream);
amt_status amt_rnn_wide_seq_train_fwd(const float* xproj, int32_t ldxp, const float* w_hh, const float* b_hh, float* y, int32_t ldy,
                                      float* reserve, int32_t ldr, int32_t B, int32_t L, int32_t d, int32_t gates, int32_t reverse,
                                      int32_t n_dirs, float* ws, void* stream);
amt_status amt_rnn_wide_seq_bwd(const float* dy, int32_t lddy, const float* reserve, int32_t ldr, const float* y, int32_t ldy,
                                const float* w_hh, float* dxproj, int32_t ldxp, float* dhn, int32_t lddhn, int32_t B, int32_t L,
                                int32_t d, int32_t gates, int32_t reverse, int32_t n_dirs, float* ws, void* stream);

/* The same step for B independent clips in lockstep (all at one position): projections are one launch over B rows (weights
 * read once per step, not once per clip), the caches carry a leading clip dimension (self K/V: B, H, max_seq, hd; cross K/V:
 * B, H, S, hd), a mixture layer evaluates all experts on all rows and combines each row's routed pair in expert-index
 * order.  Same pointer table.  keys_dev: B floats; state_dev: int32 {position, root[B], attr[B]} in device memory, the
 * position is incremented at the end; logits_out (B, 159); ws: amt_v2_step_batch_ws_floats(E, dff, n_exp, B) floats. */
int64_t amt_v2_step_batch_ws_floats(int32_t E, int32_t dff, int32_t n_exp, int32_t B);
amt_status amt_v2_step_batch(const void* const* tab, int32_t n_layers, int32_t H, int32_t E, int32_t dff, int32_t n_exp,
                             int32_t S, int32_t max_seq, int32_t B, const float* keys_dev, int32_t* state_dev,
                             float* logits_out, float* ws, void* stream);

/* Per-clip decision of the lockstep step, on the device (reference model/video_music_transformer.py:547-600: temperature
 * softmax[:157], N / repeat suppression, top-1 / arg-max / Categorical draw by inverse CDF at uniforms[(pos)*B + b], id ->
 * (root, attr) feedback; chord_embed: the id feeds back).  Launch right after amt_v2_step_batch on the same stream (it
 * reads the position from state_dev[0], which that call has advanced): stores tokens[b][pos] (and roots / attrs, all
 * [B][T] int64, primer positions pre-filled) and leaves the position's (root, attr) in state_dev for the next step.
 * No host round trip: the pair (step, decide) is captured once and replayed T-1 times. */
amt_status amt_v2_decide_batch(const float* logits, int32_t ld_logits, int32_t* state_dev, int64_t* tokens, int64_t* roots,
                               int64_t* attrs, int32_t B, int32_t T, int32_t n_primer, int32_t beam, int32_t max_conseq_N,
                               int32_t max_conseq_chord, float temperature, const float* uniforms, int32_t chord_embed, void* stream);
/* amt_v2_step_batch and the decision as ONE launch chain (what the lockstep generate replays T-2 times from a captured graph):
 * the step for the position in state_dev[0] WITHOUT its trailing position increment, then one kernel that decides position
 * state_dev[0] + 1 exactly like amt_v2_decide_batch, writes that position's chord-stream row into ws (the input of the next call,
 * which therefore starts at the first projection: pass first = 1 only for the first call of a generation, whose input row is
 * computed from state_dev) and advances state_dev[0].  state_dev: 2 + 2B int32 {position, root[B], attr[B], ticket = 0}.
 * Inside the chain: a mixture layer's routing happens in its combine kernel, the last layer's norm3 and decoder.norm both in the
 * prologue of the output head. */
typedef struct amt_v2_step_args {          /* the lockstep step: see amt_v2_step_batch */
    const void* const* tab;
    int32_t n_layers, H, E, dff, n_exp, S, max_seq, B;
    const float* keys_dev; int32_t* state_dev; float* logits_out; float* ws;
} amt_v2_step_args;
typedef struct amt_v2_decide_args {        /* the decision: see amt_v2_decide_batch */
    int64_t* tokens; int64_t* roots; int64_t* attrs;     /* [B][T] */
    int32_t T, n_primer, beam, max_conseq_N, max_conseq_chord;
    float temperature;
    const float* uniforms;                 /* (T, B) or null */
    int32_t chord_embed;
} amt_v2_decide_args;
/* The caller issues at most T - 1 - n_done calls per generation (positions 0 .. T-2); the position counter in state_dev never
 * advances past T - 1, so a call too many recomputes the last position instead of leaving the caches (T <= max_seq required). */
amt_status amt_v2_step_decide_batch(const amt_v2_step_args* step, const amt_v2_decide_args* decide, int32_t first, void* stream);
/* Introspection for bench.py: kernel launches issued by the calling thread's last amt_v2_step_batch / amt_v2_step_decide_batch
 * call (a count, not a status). */
int32_t amt_v2_last_step_launches(void);

/* ---- regression head VideoRegression(regModel='bimamba+') (model/video_regression.py:104-245) ---- */
/* Depthwise causal Conv1d(kernel K, padding K-1)[..., :L] + SiLU of MambaBlock.forward (mamba.py:172-175,268-272):
 * x (B,L,C) with row stride ldx, w (C,K) = conv1d.weight (C,1,K), y (B,L,C).  reverse = 1 evaluates the block of the
 * time-flipped sequence and returns it un-flipped (the backward branch of bimamba.py:171-185 without the two flips). */
amt_status amt_dwconv1d_silu_fwd(const float* x, int32_t ldx, const float* w, const float* bias, float* y,
                                 int32_t B, int32_t L, int32_t C, int32_t K, int32_t reverse, void* stream);
/* MambaBlock.ssm + gate (mamba.py:291-354, 281-287): delta = softplus(delta_raw + dt_bias), A = -exp(A_log) (ED,N),
 * h_t = exp(delta A) h_{t-1} + delta B_t x_t, y_t = h_t . C_t + D x_t, out = y*silu(z) [+ x*(1 - sigmoid(silu(z))) for
 * version 1 = "Mamba+"].  x / delta_raw / z / y are (B*L, ED) with their own row strides, Bm / Cm (B*L, N) with stride
 * ld_bc (slices of the x_proj output).  N = 16.  reverse as above. */
amt_status amt_selective_scan_fwd(const float* x, int32_t ldx, const float* delta_raw, int32_t ld_delta, const float* dt_bias,
                                  const float* A_log, const float* Bm, const float* Cm, int32_t ld_bc, const float* D,
                                  const float* z, int32_t ldz, float* y, int32_t ldy, int32_t B, int32_t L, int32_t ED,
                                  int32_t N, int32_t version, int32_t reverse, void* stream);
/* ---- training the Mamba heads ('bimamba+', 'bimamba'): the two kernels above with what their backward needs, and the backward.
 * d_state N = 16 only (other values are refused with the reason).  No floating-point atomics: the same inputs give the same bits. ---- */
/* amt_selective_scan_fwd (y: the same bits) that also writes y_pre (B*L, ld_ypre), the un-gated y_t = h_t . C_t + D x_t, and
 * h_chunks [B][ceil(L / 32)][ED][N], the state at the start of every 32-step chunk in the order the scan walks them (reverse = 1:
 * from the last position). */
amt_status amt_selective_scan_train_fwd(const float* x, int32_t ldx, const float* delta_raw, int32_t ld_delta, const float* dt_bias,
                                        const float* A_log, const float* Bm, const float* Cm, int32_t ld_bc, const float* D,
                                        const float* z, int32_t ldz, float* y, int32_t ldy, float* y_pre, int32_t ld_ypre,
                                        float* h_chunks, int32_t B, int32_t L, int32_t ED, int32_t N, int32_t version, int32_t reverse,
                                        void* stream);
/* Backward of the scan and its gate from dout (B*L, ld_dout), the forward's inputs, y_pre and h_chunks: the states inside a chunk
 * are recomputed from its checkpoint, the chunks walked from the last to the first.  Writes dx, ddraw (the gradient of delta_raw;
 * its column sums are the gradient of dt_bias), dz (each B*L x ED with its own row stride), dBm / dCm (B*L x N, row stride ld_dbc:
 * slices of the x_proj output's gradient), dA_log (ED, N) and dD (ED).  ws: amt_selective_scan_bwd_ws_floats(B, L, ED, N) floats --
 * ceil(ED / 16) per-block copies of dB | dC (B*L x 2N each) and per-clip partials of dA and dD, summed in index order by a second
 * launch. */
int64_t amt_selective_scan_bwd_ws_floats(int32_t B, int32_t L, int32_t ED, int32_t N);
amt_status amt_selective_scan_bwd(const float* dout, int32_t ld_dout, const float* x, int32_t ldx, const float* delta_raw,
                                  int32_t ld_delta, const float* dt_bias, const float* A_log, const float* Bm, const float* Cm,
                                  int32_t ld_bc, const float* D, const float* z, int32_t ldz, const float* y_pre, int32_t ld_ypre,
                                  const float* h_chunks, float* dx, int32_t lddx, float* ddraw, int32_t ld_ddraw, float* dz,
                                  int32_t lddz, float* dBm, float* dCm, int32_t ld_dbc, float* dA_log, float* dD, float* ws,
                                  int32_t B, int32_t L, int32_t ED, int32_t N, int32_t version, int32_t reverse, void* stream);
/* Backward of amt_dwconv1d_silu_fwd from dy (B*L, lddy) and the forward's inputs (the pre-activation is formed again): dx (B*L, C
 * columns, row stride lddx), dw (C, K), dbias (C; null exactly when bias is).  K <= 8.  ws: amt_dwconv1d_silu_bwd_ws_floats floats
 * (the pre-activation's gradient and per-64-row partials of dw | dbias, summed in index order). */
int64_t amt_dwconv1d_silu_bwd_ws_floats(int32_t B, int32_t L, int32_t C, int32_t K);
amt_status amt_dwconv1d_silu_bwd(const float* dy, int32_t lddy, const float* x, int32_t ldx, const float* w, const float* bias,
                                 float* dx, int32_t lddx, float* dw, float* dbias, float* ws, int32_t B, int32_t L, int32_t C,
                                 int32_t K, int32_t reverse, void* stream);
/* ---- training the wide-state heads ('moemamba': d_state = d_hidden): N = 32, 64, 128 or 256; N = 16 is refused with a pointer to
 * the calls above.  Same rules: accurate expf / log1pf, no floating-point atomics, the same inputs give the same bits. ---- */
/* amt_selective_scan_fwd at that N (y: the same bits) that also writes y_pre (B*L, ld_ypre) and h_chunks [B][ceil(L / I)][ED][N], the
 * state at the start of every I-step chunk in walking order, I = amt_selective_scan_wide_ckpt_steps(N) = 32 (two of the kernel's
 * 16-step passes; 0 for an N the call refuses). */
int32_t amt_selective_scan_wide_ckpt_steps(int32_t N);
amt_status amt_selective_scan_wide_train_fwd(const float* x, int32_t ldx, const float* delta_raw, int32_t ld_delta, const float* dt_bias,
                                             const float* A_log, const float* Bm, const float* Cm, int32_t ld_bc, const float* D,
                                             const float* z, int32_t ldz, float* y, int32_t ldy, float* y_pre, int32_t ld_ypre,
                                             float* h_chunks, int32_t B, int32_t L, int32_t ED, int32_t N, int32_t version, int32_t reverse,
                                             void* stream);
/* amt_selective_scan_bwd's outputs at that N.  One workgroup per (16 channels, clip, 16 states).  ws:
 * amt_selective_scan_wide_bwd_ws_floats(B, L, ED, N) floats = ceil(ED / 16) per-block copies of dB | dC (B*L x 2N each), per-clip
 * partials of dA (ED x N) and dD (ED), and N / 16 per-slice partials (B*L x ED each) of d delta and of the scan's part of dx; a second
 * launch adds each in index order and does the element-wise part (softplus', dz, the D x and Mamba+ terms of dx) once. */
int64_t amt_selective_scan_wide_bwd_ws_floats(int32_t B, int32_t L, int32_t ED, int32_t N);
amt_status amt_selective_scan_wide_bwd(const float* dout, int32_t ld_dout, const float* x, int32_t ldx, const float* delta_raw,
                                       int32_t ld_delta, const float* dt_bias, const float* A_log, const float* Bm, const float* Cm,
                                       int32_t ld_bc, const float* D, const float* z, int32_t ldz, const float* y_pre, int32_t ld_ypre,
                                       const float* h_chunks, float* dx, int32_t lddx, float* ddraw, int32_t ld_ddraw, float* dz,
                                       int32_t lddz, float* dBm, float* dCm, int32_t ld_dbc, float* dA_log, float* dD, float* ws,
                                       int32_t B, int32_t L, int32_t ED, int32_t N, int32_t version, int32_t reverse, void* stream);
/* da[i] = dy[i] s (1 + a[i] (1 - s)), s = sigmoid(a[i]) with the accurate expf: the SiLU's derivative at the pre-activation a, the one
 * launch the backward of CNN_GRU's Conv1d + SiLU front (autograd.ConvSiluFn) adds to the GEMMs. */
amt_status amt_silu_bwd(const float* dy, const float* a, float* da, int64_t n, void* stream);
/* out[row] = [a[row][0:da] | b[row][0:db] | 0 ...] (ld_out columns): cat(semantic, emotion) of get_feature
 * (video_regression.py:199-216), zero-padded to the GEMM's K step. */
amt_status amt_concat2_fwd(const float* a, int32_t da, const float* b, int32_t db, float* out, int32_t rows, int32_t ld_out,
                           void* stream);
/* amt_linear_fwd with leading dimensions and an activation: y = act(x[M,K](ldx) . w[N,K](ldw)^T + bias (+ resid(ldr)));
 * act 0 none, 1 ReLU, 2 sigmoid (the classifier head, video_regression.py:188-197), 3 SiLU (CNN_GRU's convolution, :88-91).
 * K % 32 == 0. */
amt_status amt_linear_ex_fwd(const float* x, int32_t ldx, const float* w, int32_t ldw, const float* bias, const float* resid,
                             int32_t ldr, float* y, int32_t ldy, int32_t M, int32_t N, int32_t K, int32_t act, void* stream);
/* Which kernel the dense GEMM launcher takes for y (M, N) = act(x (M, K) w (N, K)^T ...): 0 the skinny GEMM, 1 the 64x64-tile kernel,
 * 2 the 128x128-tile kernel; negative for a shape or act amt_linear_ex_fwd refuses.  act as amt_linear_ex_fwd's; other_forms != 0
 * stands for the operand and epilogue forms only the library's own callers set (head-split store, row addend, silu-multiply,
 * grouped or gathered rows).  The launcher's own rule, evaluated on the host: no device, no stream; a code, not a status. */
int32_t amt_gemm_route(int32_t M, int32_t N, int32_t K, int32_t act, int32_t other_forms);
/* y = LayerNorm(x (+ resid)) + post : the "norm2(x_b + x) then x_f + x_b" step of bimamba.py:183-188 in one pass. */
amt_status amt_layernorm_post_fwd(const float* x, const float* resid, const float* w, const float* b, const float* post,
                                  float* y, int32_t rows, int32_t dim, float eps, void* stream);

/* ---- evaluation: the test-split metrics of evaluate.py (utilities/run_model_vevo.py:198-452) from teacher-forced logits ---- */
/* Replaces compute_vevo_accuracy / compute_hits_k / compute_vevo_correspondence (dataset/vevo_dataset.py:653-701,747-810) and the two
 * losses of eval_model (CrossEntropyLoss(ignore_index=CHORD_PAD), BCEWithLogitsLoss against the emotion rows of :461-515) for the
 * single 159-way head.  logits: (B*L) rows of 159, row stride ld >= 159 floats (any ld: rows are read as dwords); tgt (B*L) int64
 * chord ids, CHORD_PAD = ignored (an id outside 0..158 is treated as CHORD_PAD); emo_class (B*L) the arg-max emotion class of the
 * target's second, 0..5 (5 = neutral; anything else counts as neutral); emo_prob (B*L) that class's probability.  Per row:
 *   pred  = arg-max, the lowest index among equal maxima;
 *   rank  = #{j: y[j] > y[tgt]} + #{j < tgt: y[j] == y[tgt]}  (the target is in the top k iff rank < k; exact);
 *   ce    = logsumexp(y) - y[tgt];
 *   bce   = sum over the 159 classes of max(y,0) - y*t + log1p(exp(-|y|)), t the emotion row: one-hot 157 / 158 for a target END /
 *           PAD, else t[j] = Q[emo_class][(j-1) % 13] for 1 <= j <= 156 with the 6 x 13 quality table of :461-475;
 *   counted = tgt is a chord (< CHORD_END), emo_class != 5, !(emo_prob < emo_threshold);
 *   right   = counted, pred is a chord, Q[emo_class][q-1] == 1 with q = 1 for pred == 0 ("N" reads as maj, :790-792), else
 *           (pred-1) % 13 + 1.
 * clip_out (B, 10) fp32, the two correspondence counts as separate floats: {n_valid (tgt != PAD), n_top1 (pred == tgt, valid rows),
 * n_hit1, n_hit3, n_hit5, ce_sum over valid rows, bce_sum over all L rows, n_counted, n_right, L}.  Counts are exact (L <= 2^24).
 * The sums are deterministic: a wave tree inside a row, then the rows of a clip added in row order; one launch, no atomics on
 * floats.  pred_out / rank_out / ce_out: (B*L) each, optional (null = not written); ce_out is 0 on ignored rows. */
amt_status amt_chord_metrics_fwd(const float* logits, int32_t ld, const int64_t* tgt, const int32_t* emo_class, const float* emo_prob,
                                 float emo_threshold, int32_t B, int32_t L, float* clip_out,
                                 int32_t* pred_out, int32_t* rank_out, float* ce_out, void* stream);

/* Test-split sums of the regression head (reference utilities/run_model_regression.py:70-125): both heads of VideoRegression applied
 * to the encoder output and reduced against the targets, one launch, nothing synchronised.
 * feat (B*S, W) fp32 with row stride ld >= W; W a positive multiple of 8, at most 1024.  w_heads (W + 1, 64) fp32, the packed heads:
 * row k < W = {classifier.weight[0..39][k], regressor.weight[0][k], regressor.weight[1][k], 22 zeros}, row W the biases in the same
 * order.  note_density, loudness (B*S), instrument (B*S, 40): fp32 targets.  Per row, in fp32:
 *   nd = feat . Wr[0] + br[0],  ld = feat . Wr[1] + br[1],  z_j = feat . Wc[j] + bc[j]  (one fp32 fma chain per output on the
 *         matrix pipe, k in a fixed order, the bias added last);
 *   p_j = 1 / (1 + exp(-z_j));
 *   bce = sum over j of -(t_j max(log p_j, -100) + (1 - t_j) max(log(1 - p_j), -100)): torch's binary_cross_entropy on the fp32
 *         probability, NOT the logits form -- where p rounds to 1 or 0 the term is exactly 100 (or 0), as in the reference.
 * clip_out (B, 4) fp32 = {sum (nd - note_density)^2, sum (ld - loudness)^2, sum bce, S} over ALL S rows of the clip (padded seconds
 * count, as the reference averages over max_sequence_video rows).  Deterministic: a fixed 40-term tree inside a row, then the rows of a clip
 * added in row order; no atomics on floats; the optional outputs do not change the sums.
 * ln_nd_out (B*S, 2) = {nd, ld} and inst_out (B*S, 40) = p: optional (null = not written). */
amt_status amt_reg_metrics_fwd(const float* feat, int32_t ld, int32_t W, const float* w_heads, const float* note_density,
                               const float* loudness, const float* instrument, int32_t B, int32_t S, float* clip_out,
                               float* ln_nd_out, float* inst_out, void* stream);

/* Training loss of the regression head (reference utilities/run_model_regression.py:33-39) and its gradient, one launch:
 *   SmoothL1Loss()(ln_nd, [note_density | loudness]) + binary_cross_entropy(inst, instrument)
 * ln_nd (rows, 2) = {nd, ld}; inst (rows, 40) the fp32 probabilities; note_density / loudness (rows); instrument (rows, 40).
 * loss[3] = {total, SmoothL1 part, BCE part}; d_ln_nd (rows, 2); d_logit (rows, 40): the BCE gradient with respect to the
 * classifier's LOGITS (torch's BCE backward times the sigmoid's: (p - t) / (40 rows) for 0 < p < 1, exactly 0 at a saturated p).
 * Logs clamped at -100.  ws: AMT_REG_LOSS_WS_FLOATS floats of scratch, 16-byte aligned, used by this call alone until it has finished
 * (a ticket counter, zeroed by the call, and two partial sums per workgroup).  min(256, ceil(40 rows / 4096)) workgroups of 1024
 * threads; the order of every addition is a function of `rows` alone and no floating-point atomic is used: the same inputs give the
 * same bits. */
#define AMT_REG_LOSS_WS_FLOATS 516
amt_status amt_reg_loss_fwd_bwd(const float* ln_nd, const float* inst, const float* note_density, const float* loudness,
                                const float* instrument, int32_t rows, float* loss, float* d_ln_nd, float* d_logit, float* ws,
                                void* stream);

/* ---- training of the chord model (reference train.py, utilities/run_model_vevo.py:73-119) ---- */
/* amt_attn_fwd that keeps what a backward needs.  Arguments as amt_attn_fwd, plus
 *   Er (er_len, hd), null = no relative term; with Er the call must be causal with Lq == Lk <= er_len and kv_group 1 (as the backward);
 *   keep (B, H, Lq, Lk) contiguous bytes, 1 = kept, null = no dropout; keep_scale = 1 / (1 - p);
 *   lse (B, H, Lq): the row's log-sum-exp of the scores as the kernel forms them.
 * With qs = q q_scale:  S_ij = qs_i . k_j (+ qs_i . Er[er_len-1-(i-j)] for j <= i),  P = softmax_j(S) under the mask,
 * O = (P o keep keep_scale) V; the normaliser is that of the undropped P, as torch drops after the softmax (rpr.py:409-412).
 * The TRAIN instantiations of the prefill kernels, chosen by shape exactly as the inference calls choose theirs: with keep null, O
 * equals amt_rpr_attn_fwd / amt_cross_attn_fwd / amt_attn_fwd bit for bit.  Head dims 32, 64, 128 (16 is refused: the backward
 * has no instantiation for it). */
amt_status amt_attn_train_fwd(const float* q, const float* k, const float* v, float* o, const int64_t* strides,
                              int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd, int32_t causal, int32_t kv_group,
                              float q_scale, const float* Er, int32_t er_len, const uint8_t* keep, float keep_scale, float* lse,
                              void* stream);
/* Backward of amt_attn_train_fwd: from dO (o's strides) and the forward's q, k, v, o, lse, Er, keep the gradients with respect to
 * the tensors as passed: dq (q's strides; includes q_scale), dk, dv (k's / v's strides; with kv_group > 1 the sum over the group's
 * query heads, in head order), dEr (er_len, hd) contiguous, optional.  With D_i = sum_d dO_id O_id:
 *   dP = (dO V^T) o keep keep_scale,  dS = P o (dP - D_i),  dv = (P o keep keep_scale)^T dO,  dk = dS^T qs,
 *   dqs = dS k (+ sum_j dS_ij Er[er_len-1-(i-j)]),  dEr[r] = sum over b, h and the pairs with i - j = er_len-1-r of dS_ij qs_i;
 * rows of Er no pair reaches get exactly 0.  A row whose keep is all zero has O = 0 and finite (zero) gradients.
 * Pass A, one workgroup per 128 queries, recomputes P tile by tile from lse in the forward's layout and forms dq; it leaves dS and
 * P o keep keep_scale in two (B H, Lq, ceil32(Lk)) scratches from which pass B, one wave per 32 keys, forms dk and dv.  With Er the dS
 * scratch is un-skewed (key j of query i in column L-1-(i-j)): dq's second term is one product of it with Er's last L rows on the
 * library's GEMM, dEr one MFMA chain per (clip, head) into a slab each, the slabs added in (clip, head) order.  No atomics: the order
 * of every addition is a function of the shapes alone.  With Er: kv_group 1.  Head dims 32, 64, 128.
 * ws: amt_attn_bwd_ws_floats(B, H, Lq, Lk, hd, Er != null) floats of scratch, 16-byte aligned, this call's alone until it finishes
 * (184 MB at 32 clips x 8 heads x 299 x 299, 226 MB with Er). */
/* Which prefill kernel amt_rpr_attn_fwd / amt_cross_attn_fwd / amt_attn_fwd / amt_attn_train_fwd take for a shape: 0 the 128-row
 * kernel, 1 the split-key kernel (32-row blocks, keys split over the waves); negative for a shape they refuse.  has_er != 0: with a
 * relative position table.  The launcher's own rule, evaluated on the host: no device, no stream; a code, not a status. */
int32_t amt_attn_route(int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd, int32_t has_er);
int64_t amt_attn_bwd_ws_floats(int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd, int32_t rpr);
amt_status amt_attn_bwd(const float* dO, const float* q, const float* k, const float* v, const float* o, const float* lse,
                        const float* Er, int32_t er_len, const uint8_t* keep, float keep_scale, float* dq, float* dk, float* dv,
                        float* dEr, const int64_t* strides, int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd,
                        int32_t causal, int32_t kv_group, float q_scale, float* ws, void* stream);

/* Backward of y = LayerNorm(x (+ resid)) * w + b (amt_layernorm_fwd; torch.nn.LayerNorm).  dy, x, resid (null = none), dx: (rows, dim);
 * w, dw, db: (dim).  x / resid are the forward's inputs: the row statistics are formed again from them as the forward formed them.
 *   dx = rstd (g - mean(g) - xh mean(g xh)),  g = dy w,  xh = (x (+ resid) - mean) rstd      (the gradient of x and of resid alike)
 *   dw = sum over rows of dy xh,   db = sum over rows of dy
 * dim a multiple of 4, at most 1024; any rows > 0.  ws: AMT_LAYERNORM_BWD_WS_FLOATS(dim) floats of scratch, 16-byte aligned, used by
 * this call alone until it has finished (a ticket counter, zeroed by the call, and one [dw | db] slab per workgroup).
 * amt_rmsnorm_bwd_blocks(rows) workgroups of 4 waves (below: one rule, one kernel for both norms; csrc/norm_bwd.hip), one wave per
 * row; a workgroup adds its rows per wave in row order, its waves in wave order, and the last workgroup to finish adds the slabs in
 * workgroup order: the order of every addition is a function of (rows, dim) alone and no floating-point atomic is used, so the same
 * inputs give the same bits. */
#define AMT_LAYERNORM_BWD_WS_FLOATS(dim) (4 + 256 * (dim))
amt_status amt_layernorm_bwd(const float* dy, const float* x, const float* resid, const float* w, float* dx, float* dw, float* db,
                             float* ws, int32_t rows, int32_t dim, float eps, void* stream);

/* What the training of the V1 / V2 chord models adds to the above (csrc/family_train.hip; amt_rmsnorm_bwd: csrc/norm_bwd.hip).  All
 * three are fp32 and stateless, use no floating-point atomic and fix the order of every addition by the shapes alone: the same inputs give the same bits.
 *
 * amt_rope_bwd: the adjoint of amt_rope_fwd under the same index rule and the same shape checks (both cache layouts: the broadcast
 * slab 2 cache_half == hd, and the [seq][cache_half][2] cache read as [n0][seq][hd/2][2]); each pair of dy is rotated by the transpose
 * of the forward's rotation: dx0 = dy0 cos + dy1 sin, dx1 = dy1 cos - dy0 sin.  dx may be dy.  dy / dx 8-byte aligned. */
amt_status amt_rope_bwd(const float* dy, const float* cache, float* dx, int32_t n0, int32_t seq, int32_t n2, int32_t hd,
                        int32_t cache_half, void* stream);
/* Backward of y = RMSNorm(x (+ resid)) * w (amt_rmsnorm_resid_fwd) from the forward's own inputs.  dy, x, resid (null = none), dx:
 * (rows, dim); w, dw: (dim).  With u = x (+ resid), r = rsqrt(mean(u^2) + eps), xh = u r, g = dy w:
 *   dx = r (g - xh mean(g xh))      (the gradient of x and of resid alike),   dw = sum over rows of dy xh
 * dim a multiple of 4, at most 1024; any rows > 0.  ws: AMT_RMSNORM_BWD_WS_FLOATS(dim) floats of scratch, 16-byte aligned, used by this
 * call alone until it has finished (a ticket counter, zeroed by the call, and one dw slab per workgroup).  amt_rmsnorm_bwd_blocks(rows)
 * workgroups of 4 waves (the launcher's own rule, min(128, ceil(rows / 16)), evaluated on the host: a count, not a status; negative for
 * rows <= 0), workgroup b taking rows [b per, (b + 1) per) with per = ceil(rows / blocks), one wave per row: amt_layernorm_bwd's kernel
 * without the mean and db, and its two-stage sum. */
#define AMT_RMSNORM_BWD_WS_FLOATS(dim) (4 + 128 * (dim))
int32_t amt_rmsnorm_bwd_blocks(int32_t rows);
amt_status amt_rmsnorm_bwd(const float* dy, const float* x, const float* resid, const float* w, float* dx, float* dw, float* ws,
                           int32_t rows, int32_t dim, float eps, void* stream);
/* Training of one GLUExpert on n rows (amt_glu_expert_fwd's layer): y = W2((W1 x + b1) * silu(Wg x + bg) * mask_h) + b2, or with
 * w1 == NULL the Linear -> SiLU -> Dropout -> Linear expert y = W2(silu(Wg x + bg) * mask_h) + b2 (amt_moe_train_fwd's convention).
 * x, out (n, d); w1 / wg (dff, d), b1 / bg (dff), w2 (d, dff), b2 (d) at the padded width dff (a multiple of 32, as d); mask_h
 * (n, dff_raw) multipliers or null, dff_raw <= dff the expert's own hidden width.  `saved` (amt_glu_train_scratch_floats(n, dff, glu),
 * glu = 1 when w1 is given; 16-byte aligned) receives what amt_glu_bwd reads: the gate pre-activation G, the up branch U (GLU only) and
 * H as fed to the down projection.  With mask_h null, out is the bits of amt_glu_expert_fwd.
 * amt_glu_bwd: dout (n, d) -> dx (n, d) and dw1 (dff, d; null for a SiLU expert) db1 dwg dbg dw2 (d, dff) db2 at the padded width (the
 * padding's rows / columns come out zero).  w1t / wgt (d, dff) and w2t (dff, d) are the TRANSPOSED weights, prepared by the caller.
 * ws: amt_glu_bwd_ws_floats(n, d, dff) floats, 16-byte aligned. */
int64_t amt_glu_train_scratch_floats(int32_t n, int32_t dff, int32_t glu);
amt_status amt_glu_train_fwd(const float* x, const float* w1, const float* b1, const float* wg, const float* bg, const float* w2,
                             const float* b2, const float* mask_h, float* out, float* saved, int32_t n, int32_t d, int32_t dff,
                             int32_t dff_raw, void* stream);
int64_t amt_glu_bwd_ws_floats(int32_t n, int32_t d, int32_t dff);
amt_status amt_glu_bwd(const float* dout, const float* x, const float* saved, const float* w1t, const float* wgt, const float* w2t,
                       const float* mask_h, float* dx, float* dw1, float* db1, float* dwg, float* dbg, float* dw2, float* db2,
                       float* ws, int32_t n, int32_t d, int32_t dff, int32_t dff_raw, int32_t glu, void* stream);

/* Training of the differential-attention tail of the V3 chord models (csrc/diff_subln_train.hip).  Both are fp32 and stateless, use no
 * floating-point atomic and fix the order of every addition by the shapes alone: the same inputs give the same bits.
 *
 * amt_diff_subln_train_fwd: amt_diff_subln_fwd with lambda_full read from one float in DEVICE memory (it is a function of four
 * parameters, which change with every step; a host scalar would cost a synchronisation per attention per step).  hd <= 128.  For the
 * same lambda value y is amt_diff_subln_fwd's bits.
 * amt_diff_subln_bwd: its backward from the forward's own inputs.  dy, o1, o2, d_o1, d_o2: (rows, hd); w, dw: (hd); lambda_dev, dlambda:
 * one float.  With u = o1 - lambda o2, r = rsqrt(mean_hd(u^2) + eps), xh = u r, g = dy w out_scale:
 *   du = r (g - xh mean_hd(g xh)),  d_o1 = du,  d_o2 = -lambda du,  dw = out_scale sum over rows of dy xh,  dlambda = -sum over rows and
 *   columns of du o2
 * hd 32, 64 or 128 (amt_attn_bwd's head dims); any rows > 0; every pointer but lambda_dev / dlambda 16-byte aligned.  One pass over
 * dy / o1 / o2 and two stores, hd / 4 lanes per row with 16-byte accesses (8 / 4 / 2 rows per wave), the row's means summed inside its
 * lane group.  ws: AMT_DIFF_SUBLN_BWD_WS_FLOATS(hd) floats of scratch, 16-byte aligned, used by this call alone until it has finished
 * (a ticket counter, zeroed by the call, and one [dw | dlambda] slab per workgroup; the last workgroup to finish adds the slabs in
 * workgroup order).  amt_diff_subln_bwd_blocks(rows, hd) workgroups of 4 waves (the launcher's own rule, min(128, ceil(rows / (16 *
 * 256 / hd))), evaluated on the host: a count, not a status; negative for rows <= 0 or another hd), workgroup b taking rows
 * [b per, (b + 1) per) with per = ceil(rows / blocks), wave w of it the groups of 256 / hd rows w, w + 4, ... of that range. */
#define AMT_DIFF_SUBLN_BWD_WS_FLOATS(hd) (4 + 128 * ((hd) + 4))
amt_status amt_diff_subln_train_fwd(const float* o1, const float* o2, const float* w, const float* lambda_dev, float* y, int32_t rows,
                                    int32_t hd, float out_scale, float eps, void* stream);
int32_t amt_diff_subln_bwd_blocks(int32_t rows, int32_t hd);
amt_status amt_diff_subln_bwd(const float* dy, const float* o1, const float* o2, const float* w, const float* lambda_dev, float* d_o1,
                              float* d_o2, float* dw, float* dlambda, float* ws, int32_t rows, int32_t hd, float out_scale, float eps,
                              void* stream);

/* Training loss of the chord model (reference utilities/run_model_vevo.py:101-119) and its gradient, one launch:
 *   total = lambda CrossEntropyLoss(ignore_index=CHORD_PAD, label_smoothing=smoothing)(y, tgt)
 *           + (1 - lambda) BCEWithLogitsLoss()(y, tgt_emotion)
 * logits, ld, tgt, emo_class: as amt_chord_metrics_fwd takes them, and the emotion row t of a target is built exactly as that call
 * documents (an id outside 0..158 is ignored like CHORD_PAD; an emo_class outside 0..4 accepts no quality).  Per row, with p the
 * softmax of the row and eps = smoothing (0 = none):
 *   ce  = (1 - eps) (logsumexp(y) - y[tgt]) + eps (-sum_c log p_c) / 159        (valid rows: tgt != CHORD_PAD)
 *   bce = sum over the 159 classes of max(y,0) - y t + log1p(exp(-|y|))         (all rows)
 * loss[3] = {total, chord, emotion}: chord = sum_b clip ce / sum_b n_valid, emotion = sum bce / (159 B L), total = lambda chord +
 * (1 - lambda) emotion.  A batch without a valid target gives chord = NaN, as torch does.
 * clip_out (B, 4) = {n_valid, sum of ce over the clip's valid rows, sum of bce over its L rows, L}.
 * dlogits (B L, 159) contiguous, optional (null = forward only; loss and clip_out are the same bits either way):
 *   lambda (p - (1 - eps) onehot(tgt) - eps / 159) valid / n_valid_total + (1 - lambda) (sigmoid(y) - t) / (159 B L)
 * ws: amt_chord_loss_ws_floats(B, L) floats of scratch, 16-byte aligned, used by this call alone until it has finished (a ticket
 * counter, zeroed by the call, and three sums per workgroup).  B ceil(L / 64) workgroups of 16 waves, one wave per row: a wave tree
 * inside a row, the rows of a workgroup added in row order, the workgroups of a clip in order, the clips in order; no floating-point
 * atomic, so the same inputs give the same bits.  159 B L <= 2^24. */
int64_t amt_chord_loss_ws_floats(int32_t B, int32_t L);
amt_status amt_chord_loss_fwd_bwd(const float* logits, int32_t ld, const int64_t* tgt, const int32_t* emo_class, int32_t B, int32_t L,
                                  float lambda, float smoothing, float* loss, float* clip_out, float* dlogits, float* ws, void* stream);

/* The same loss with the reference's -auxiliary_loss (train.py:221-229, model/loss.py:85-141) and free weights:
 *   chord = (CE + A_3 + A_5) / count,  total = w_chord chord + w_emotion emotion
 * CE and emotion as above.  For an auxiliary row z of 159 values with target t, p = softmax(z) and a_k = relu(mean(top-k of p) - p_t);
 * A_k = w_k (sum of a_k over the valid rows) / n_valid with (k, w_k) = (3, 3.0), (5, 5.0); count = how many of the three fp32 terms
 * exceed 1e-10 (a constant under differentiation; 0 gives the reference's division by zero).
 * layout: AMT_CHORD_AUX_ROWS -- auxiliary row (b, l) is logits[b, l, :159], as the reference's eval_model passes them;
 *         AMT_CHORD_AUX_VIEW -- as its train_epoch does, the (B, 159, L) permute RESHAPED to (B, L, 159): element j of row (b, r) is
 *         logits[b, f % L, f / L] with f = 159 r + j.  Either way the row pairs with tgt[b, r].
 * loss[7] = {total, chord, emotion, CE, A_3, A_5, count}.  A weight of exactly 0 drops its term from total and from dlogits.
 * clip_out (B, 6) = the four columns above, then the clip's sums of a_3 and a_5 over its valid rows (unweighted).
 * dlogits (B L, 159) contiguous, optional (null = forward only; loss and clip_out are the same bits either way):
 *   (w_chord / count) (dCE + dA_3 + dA_5) + w_emotion dBCE;  an auxiliary row with a_k > 0 gives
 *   dz_j = (w_k / n_valid) p_j (g_j - sum_i g_i p_i),  g_j = [j in top-k] / k - [j = t].
 * ws: amt_chord_loss_aux_ws_floats(B, L) floats, 16-byte aligned, this call's alone until it has finished (the ticket counter, five
 * sums per workgroup and two (B L, 159) gradient pieces).  Two launches on `stream`: the loss kernel (the grid and summation order of
 * amt_chord_loss_fwd_bwd) and, with dlogits, an elementwise one that reads count from loss[6]; nothing waits on the host.  No
 * floating-point atomic: the same inputs give the same bits.  159 B L <= 2^24. */
#define AMT_CHORD_AUX_ROWS 0
#define AMT_CHORD_AUX_VIEW 1
int64_t amt_chord_loss_aux_ws_floats(int32_t B, int32_t L);
amt_status amt_chord_loss_aux_fwd_bwd(const float* logits, int32_t ld, const int64_t* tgt, const int32_t* emo_class, int32_t B, int32_t L,
                                      float w_chord, float w_emotion, float smoothing, int32_t layout, float* loss, float* clip_out,
                                      float* dlogits, float* ws, void* stream);

/* One fused multi-tensor optimiser step (csrc/optim.hip): torch's RAdam (coupled or decoupled weight decay) and the reference's
 * RAdanW (model/RAdanW.py) in its foreach variant (:319-445, what the reference runs on a GPU) and its single-tensor variant
 * (:223-317); the two are different optimisers and both are restated as written, the writes into the gradient included.
 * One launch on `stream` updates n_tensors <= AMT_OPTIM_MAX_TENSORS tensors that share a step count; the pointer tables are read on
 * the host during the call (they travel in the kernel arguments) and may be reused as soon as it returns.  Nothing waits on the host.
 * Tensor t: p (parameter), g (gradient), m (exp_avg), v (exp_avg_sq), and for the RAdanW modes ed (exp_diff), eds (exp_diff_sq),
 * npg (neg_prev_grad): numel[t] contiguous floats each, every pointer 16-byte aligned.  Written: p, m, v; under RAdanW also g, ed,
 * eds, npg.  npg_from_grad != 0: npg is not read, -g stands in for it (the steps at which the reference re-initialises it).
 * The scalars are the step's, formed by the caller in double exactly as the Python of torch / the reference forms them
 * (video2music_amd/optim.py): decay = 1 - lr wd (1 where the mode has none), weight_decay the coupled one of AMT_OPTIM_RADAM (else 0),
 * rectified = rho_t > 5, rect_step_size = -(sqrt(bias_correction2) lr rect / bias_correction1) and unrect_step_size =
 * -(lr / bias_correction1) for the foreach forms; bias_correction1, bias_correction2_sqrt and rect for AMT_OPTIM_RADANW_SINGLE.
 * Refused before any launch (status -1): an unknown mode, n_tensors outside 1..AMT_OPTIM_MAX_TENSORS, a null or misaligned pointer,
 * numel <= 0.  The bits of every output depend on the element's inputs and the scalars alone: not on the grid, not on how the
 * caller batches tensors into launches. */
#define AMT_OPTIM_MAX_TENSORS 48
#define AMT_OPTIM_RADAM 0
#define AMT_OPTIM_RADAMW 1
#define AMT_OPTIM_RADANW_FOREACH 2
#define AMT_OPTIM_RADANW_SINGLE 3
typedef struct amt_optim_args {
    int32_t mode, n_tensors;
    float* const* p;
    float* const* g;
    float* const* m;
    float* const* v;
    float* const* ed;
    float* const* eds;
    float* const* npg;
    const int64_t* numel;
    float lr, decay, weight_decay, one_minus_beta1, beta2, one_minus_beta2, eps;
    float rect_step_size, unrect_step_size, bias_correction1, bias_correction2_sqrt, rect;
    float beta3, one_minus_beta3, neg_one_minus_beta3, beta4, one_minus_beta4;
    int32_t rectified, npg_from_grad;
} amt_optim_args;
amt_status amt_optim_step(const amt_optim_args* a, void* stream);
/* The launcher's own constants, evaluated on the host (no device, no stream; a value, not a status; negative for an unknown query):
 * tensors per launch, elements per chunk (a block's unit of work: tensors are cut into chunks, the chunks dealt to the blocks
 * round-robin), the cap on the grid, and the block size. */
#define AMT_OPTIM_PLAN_MAX_TENSORS 0
#define AMT_OPTIM_PLAN_CHUNK 1
#define AMT_OPTIM_PLAN_MAX_BLOCKS 2
#define AMT_OPTIM_PLAN_THREADS 3
int32_t amt_optim_plan(int32_t what);

#ifdef __cplusplus
}
#endif
#endif /* AMT_HIP_H */
