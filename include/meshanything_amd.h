/*
 * meshanything_amd.h -- C ABI of the MI355X-native MeshAnything inference engine.
 *
 * The reference (buaacyw/MeshAnything @ 2024_08_07) has no native layer and no FFI: its hot path sits behind
 * four Python call boundaries.  Each entry point below names the reference call it
 * replaces; `meshanything_amd/model.py` re-exposes them under the reference's own Python names
 * (MeshAnything.forward / point_encoder.encode_latents / transformer.generate / tokenizer(...)).
 *
 * Conventions
 *   - return 0 (MA_OK) on success, a negative MA_ERR_* code on failure; text via ma_last_error().
 *     No C++ exception crosses this boundary.
 *   - all tensor arguments are caller-owned DEVICE pointers (row-major, dense) unless marked "host";
 *     the engine owns weights, KV cache, workspace and the captured hipGraph.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls are asynchronous on that
 *     stream except where noted (ma_generate / ma_forward read back lengths and therefore synchronise).
 *   - one engine per device; an engine is not thread-safe.
 */
#ifndef MESHANYTHING_AMD_H
#define MESHANYTHING_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MA_API __attribute__((visibility("default")))

enum {
    MA_OK = 0,
    MA_ERR_INVALID = -1,        /* bad argument / config */
    MA_ERR_HIP = -2,            /* a HIP runtime call failed */
    MA_ERR_STATE = -3,          /* call made in the wrong state (e.g. weights not loaded) */
    MA_ERR_UNKNOWN_TENSOR = -4, /* ma_engine_load_weights: key not part of the checkpoint layout */
    MA_ERR_SHAPE = -5,          /* tensor shape/dtype does not match the layout */
    MA_ERR_MISSING = -6,        /* ma_engine_finalize_weights: required tensors were never loaded */
    MA_ERR_NCCL = -7,           /* RCCL call failed / librccl not loadable */
    MA_ERR_CAPACITY = -8        /* an output buffer is smaller than the result (the result's size is still reported) */
};

/* element types: engine policy (ma_config.dtype) and source-tensor dtypes of ma_tensor_desc */
enum { MA_DTYPE_F32 = 0, MA_DTYPE_BF16 = 1, MA_DTYPE_F16 = 2 };

/* Shape + policy.  Field order mirrors meshanything_amd/config.py::MAConfig (all int32).
 * Defaults of the 350M checkpoint in comments; reference sources: MeshAnything/miche/shapevae-256.yaml:7-19,
 * MeshAnything/models/meshanything.py:18,27,88-113, main.py:77-80. */
typedef struct ma_config {
    int32_t struct_size;   /* = sizeof(ma_config) */
    /* point encoder (Michelangelo perceiver) */
    int32_t n_points;      /* 4096 */
    int32_t num_freqs;     /* 8    */
    int32_t enc_width;     /* 768  */
    int32_t enc_heads;     /* 12   */
    int32_t num_latents;   /* 256 (+1 shape token = cond_length 257) */
    int32_t enc_layers;    /* 8    */
    int32_t shape_layers;  /* 16   */
    int32_t embed_dim;     /* 64   */
    /* autoregressive decoder (OPT-350m shape, post-LN, ReLU) */
    int32_t hidden;        /* 1024 */
    int32_t heads;         /* 16   */
    int32_t layers;        /* 24   */
    int32_t ffn;           /* 4096 */
    int32_t codebook_size; /* 8192 (vocab = +3: bos 0, eos 1, pad 2) */
    int32_t codebook_dim;  /* 1024 */
    int32_t n_max_faces;   /* 800  (max_new_tokens = 9*faces + 2) */
    int32_t max_positions; /* 18259 (embed_positions has +2 offset rows) */
    /* detokenizer (BERT-base shape, 6 layers) */
    int32_t tok_width;     /* 768  */
    int32_t tok_heads;     /* 12   */
    int32_t tok_layers;    /* 6    */
    int32_t tok_ffn;       /* 3072 */
    int32_t tok_max_pos;   /* 18000 */
    int32_t discrete_num;  /* 128  */
    /* engine policy */
    int32_t max_batch;     /* largest B accepted by encode/generate/detokenize/forward */
    int32_t dtype;         /* MA_DTYPE_BF16: bf16 weights + KV, GEMM/attention inputs rounded to bf16, fp32 accumulate (BASELINE.json's policy);
                              MA_DTYPE_F16: the same with IEEE half -- the reference's own arithmetic (fp16 autocast, main.py:114-118,149);
                              MA_DTYPE_F32: everything fp32 ("exact" mode for the parity gates) */
    int32_t kv_splits;     /* reserved (the decode attention always splits a head's cache into 16 equal chunks) */
    int32_t use_graph;     /* 1: replay one captured decode step (hipGraph); 0: eager launches */
    int32_t enc_exact;     /* 16-bit policies: 1 = the point encoder (ma_encode: encode_latents + process_point_feature, and the detokenizer's
                              projection of the latents) keeps fp32 weights and computes in fp32 on the fp32 matrix path, so the encoder
                              activations meet the fp32 policy's 1e-5 while prefill / decode / detokenizer stay 16-bit; 0 = everything in
                              the policy dtype.  Ignored under MA_DTYPE_F32. */
} ma_config;

typedef struct ma_engine ma_engine;

/* One checkpoint tensor, by its key in the reference state dict (main.py:99-104; layout SURVEY.md Appendix A).
 * `data` is a HOST pointer to a dense row-major array of `dtype`. */
typedef struct ma_tensor_desc {
    const char *name;
    int32_t dtype;          /* MA_DTYPE_F32 | MA_DTYPE_BF16 | MA_DTYPE_F16 */
    int32_t ndim;           /* 1..3 */
    int64_t shape[4];
    const void *data;
} ma_tensor_desc;

/* Decoding options of transformer.generate(...) as called at meshanything.py:143-162. */
typedef struct ma_sample_cfg {
    int32_t struct_size;    /* = sizeof(ma_sample_cfg) */
    int32_t do_sample;      /* 0: greedy (num_beams=1); 1: top_k -> top_p -> multinomial */
    int32_t top_k;          /* 50 */
    float   top_p;          /* 0.95 */
    int32_t max_new_tokens; /* <= 9*n_max_faces + 2; 0 = that maximum */
    int32_t suppress_eos;   /* 1: never emit eos (full-length throughput runs on random weights) */
    int32_t check_every;    /* poll the all-rows-finished flag every this many steps (0 = 64) */
    int32_t logits_first_step; /* with logits_out: the first step whose logits are kept, in [0, max_new_tokens) (0 = all; outside that range:
                                  MA_ERR_INVALID); ignored, whatever its value, when logits_out is NULL; see logits_out */
    uint64_t seed;          /* in-kernel uniform stream when `uniforms` is NULL */
    const float *uniforms;  /* DEVICE (B, max_new_tokens) uniforms in [0,1), or NULL.  Injected uniforms define
                               sampling parity with the oracle (the reference's Philox stream is not reproducible). */
    /* teacher forcing (parity along the REFERENCE's own token path, tests/test_gpu_reference_anchor.py): when non-NULL, step t still
     * picks its token from its logits and reports it in `tokens`, but the token FED to step t + 1 is forced_tokens[b][t] -- the engine
     * walks the given stream and `tokens` shows what it would have chosen at every step of it.  A forced eos finishes the row. */
    const int64_t *forced_tokens;   /* DEVICE (B, max_new_tokens) int64, or NULL */
    /* when non-NULL, the logits every generated token was picked from: DEVICE (B, max_new_tokens, codebook_size + 3) fp32, row [b][t] =
     * the distribution of token t (as returned by ma_engine_read_logits for the last step; eos is NOT masked in the copy).  With
     * logits_first_step = f > 0 only steps t >= f are kept: DEVICE (B, max_new_tokens - f, vocab), row [b][t - f] (deep-cache parity
     * checks of large batches: 64 rows x 7202 steps of logits would be 15 GB) */
    float *logits_out;
} ma_sample_cfg;

/* ---- lifecycle ---------------------------------------------------------------------------------------- */
MA_API const char *ma_version(void);
MA_API const char *ma_last_error(const ma_engine *e);      /* e may be NULL: last error of a failed create */
/* replaces: MeshAnything(args) construction, meshanything.py:83-123 */
MA_API int  ma_engine_create(ma_engine **out, const ma_config *cfg, int device);
MA_API void ma_engine_destroy(ma_engine *e);
/* integer options (debug / A-B switches); see DESIGN.md.  Unknown names -> MA_ERR_INVALID. */
MA_API int  ma_engine_set_option(ma_engine *e, const char *name, int64_t value);
/* reads an option back as the engine will apply it (e.g. "fuse_qkv_attn" is 1 only if the option is on AND the configuration is
 * eligible).  The list of names, their accepted values and side effects is the table OPTIONS in meshanything_amd/csrc/engine_options.hpp
 * (the read-only names and what the health counters of the fused launches mean).
 * Streams: every entry point enqueues on the caller's stream and is ordered with it.  ma_generate's prefill of >= 8 samples (16-bit
 * policies) additionally runs the last rows of its GEMMs on a second, engine-owned stream of the lowest priority, forked from and
 * joined to the caller's stream inside the call (option "prefill_tail" = 0 keeps everything on the caller's stream). */
MA_API int  ma_engine_get_option(ma_engine *e, const char *name, int64_t *value);

/* ---- weights ------------------------------------------------------------------------------------------ */
/* replaces: safe_open(...) + load_state_dict(strict=True), main.py:99-104.  May be called repeatedly with
 * subsets of the checkpoint; q/k/v projections are fused, matrices converted to the policy dtype.
 * Keys the hot path never reads (embed_tokens, shape_projection, geo_decoder.*) are accepted and dropped. */
MA_API int  ma_engine_load_weights(ma_engine *e, const ma_tensor_desc *tensors, int n);
/* strict=True check: every tensor the hot path needs has been loaded */
MA_API int  ma_engine_finalize_weights(ma_engine *e);
/* the packed device weight arena (for a collective broadcast driven from the host framework) */
MA_API int  ma_engine_arena(ma_engine *e, void **dev_ptr, size_t *bytes);
/* declare the arena valid after it was filled by a broadcast (ranks != root) */
MA_API int  ma_engine_mark_weights_loaded(ma_engine *e);
/* replaces: accelerate.prepare(model) -> DDP initial parameter broadcast, main.py:113-118,146.
 * `nccl_comm` is an ncclComm_t (RCCL); one ncclBroadcast of the arena over xGMI; no per-step collectives. */
MA_API int  ma_engine_broadcast_weights(ma_engine *e, void *nccl_comm, int root, void *stream);

/* host-only arena description (no GPU needed): layout is a pure function of the config */
MA_API int64_t ma_arena_bytes(const ma_config *cfg);
MA_API int     ma_arena_num_entries(const ma_config *cfg);
MA_API int     ma_arena_entry(const ma_config *cfg, int i, char *name, int name_cap, int64_t *offset,
                              int64_t *bytes, int32_t *dtype, int32_t *rows, int32_t *cols);
/* host-only packing of checkpoint tensors into a caller-provided host arena of ma_arena_bytes() bytes
 * (same conversion/fusion as ma_engine_load_weights); ma_engine_upload_arena copies it to the device. */
MA_API int  ma_pack_weights_host(const ma_config *cfg, const ma_tensor_desc *tensors, int n, void *host_arena,
                                 char *err, int err_cap);
MA_API int  ma_engine_upload_arena(ma_engine *e, const void *host_arena, size_t bytes);

/* ---- the hot path ------------------------------------------------------------------------------------- */
/* replaces: point_encoder.encode_latents(pc_normal) (asl_pl_module.py:145-157) and
 * MeshAnything.process_point_feature (meshanything.py:125-132, which calls to_shape_latents).
 *   pc       (B, n_points, 6) xyz+normal, `pc_dtype` F32 or F16 (Dataset yields fp16, main.py:56)
 *   latents  (B, cond_length, enc_width) fp32  -- raw encoder latents (the detokenizer's point_feature)
 *   prefix   (B, cond_length, hidden) fp32     -- decoder prefix (may be NULL to skip)              */
MA_API int  ma_encode(ma_engine *e, const void *pc, int pc_dtype, int B, float *latents, float *prefix, void *stream);

/* the two halves of ma_encode's prefix stage on their own, under the reference's names:
 * replaces: point_encoder.to_shape_latents(latents) (asl_pl_module.py:182-185): (B, num_latents, enc_width) -> same shape */
MA_API int  ma_to_shape_latents(ma_engine *e, const float *latents, int B, float *out, void *stream);
/* replaces: MeshAnything.process_point_feature(point_feature) (meshanything.py:125-132): (B, cond_length, enc_width) -> (B, cond_length, hidden) */
MA_API int  ma_process_point_feature(ma_engine *e, const float *point_feature, int B, float *prefix, void *stream);

/* replaces: transformer.generate(inputs_embeds=prefix, max_new_tokens=..., ...) (meshanything.py:143-162).
 *   tokens      (B, max_new_tokens) int64 device: new tokens only; finished rows padded with pad=2
 *   lengths     host (B): tokens generated per row including its eos
 *   n_generated host: number of valid columns (= max over rows; what generate() would return as shape[1])
 * Synchronises `stream` before returning. */
MA_API int  ma_generate(ma_engine *e, const float *prefix, int B, const ma_sample_cfg *sc, int64_t *tokens,
                        int32_t *lengths, int32_t *n_generated, void *stream);

/* replaces: meshanything.py:163-172 (eos-pad to 9F+2, drop first/last, specials -> -1, others -= 3).
 *   tokens (B rows of n_generated valid columns, ld_tokens elements apart: what generate() returned, in place)
 *   ->  ids (B, 9*n_max_faces) int64 in [-1, codebook_size) */
MA_API int  ma_postprocess_tokens(ma_engine *e, const int64_t *tokens, int ld_tokens, int B, int n_generated, int64_t *ids, void *stream);

/* replaces: MeshAnything.get_codes(indices) (meshanything.py:178-212): ids (B, 9F) in [-1, codebook) -> codes (B, 3F, codebook_dim)
 * fp32, the sum of the three residual-VQ rows of every vertex (pad contributes 0) */
MA_API int  ma_get_codes(ma_engine *e, const int64_t *ids, int B, float *codes, void *stream);

/* replaces: get_codes (meshanything.py:178-212) + tokenizer(ids, codes, point_feature=latents) (50-80).
 *   coords (B, n_max_faces, 3, 3) fp32, NaN rows = invalid faces */
MA_API int  ma_detokenize(ma_engine *e, const int64_t *ids, const float *latents, int B, float *coords, void *stream);
/* the same with the caller's `input_embeds` (B, 3*n_max_faces, codebook_dim) fp32 as the face codes -- the reference's
 * tokenizer(input_ids, input_embeds, point_feature=...) signature (meshanything.py:50-55); codes == NULL: ma_detokenize */
MA_API int  ma_detokenize_embeds(ma_engine *e, const int64_t *ids, const float *codes, const float *latents, int B, float *coords, void *stream);

/* replaces: MeshAnything.forward(pc_normal, sampling) (meshanything.py:134-176): encode -> generate ->
 * postprocess -> detokenize.  `tokens` / `ids` / `latents` may be NULL.  Synchronises. */
MA_API int  ma_forward(ma_engine *e, const void *pc, int pc_dtype, int B, const ma_sample_cfg *sc, float *coords,
                       int64_t *tokens, int32_t *lengths, int32_t *n_generated, int64_t *ids, float *latents, void *stream);

/* ---- kernel-level entry points (parity tests and microbenchmarks call the same kernels the engine runs) */
enum { MA_ACT_NONE = 0, MA_ACT_RELU = 1, MA_ACT_GELU = 2 };
/* y[N] = act(W[N,K] . norm(x)[K] + bias) + res ; optional LayerNorm prologue on x (ln_g != NULL); wdtype F32|BF16.
 * With wdtype BF16, x is rounded to bf16 after the prologue (the engine's bf16 policy). */
MA_API int  ma_op_gemv(int wdtype, const void *W, const float *bias, const float *x, const float *ln_g, const float *ln_b,
                       float ln_eps, const float *res, float *y, float *xn_out, int N, int K, int act, void *stream);
/* C[M,N] = act(A[M,K] . W[N,K]^T + bias[N]) + R[M,N]; K % 32 == 0; impl 0 = MFMA, 1 = plain VALU reference kernel */
MA_API int  ma_op_gemm(int wdtype, int impl, const float *A, int lda, const void *W, const float *bias, const float *R, int ldr,
                       float *C, int ldc, int M, int N, int K, int act, void *stream);
/* the same GEMM on the bf16 policy's native operands (csrc/gemm_tile.hpp: 128x128x64 LDS-DMA-staged MFMA tile): A (M, lda) bf16,
 * W (N, K) bf16; fp32 output C and / or bf16 output Cb (either may be NULL); K % 32 == 0, lda % 8 == 0, ld* % 4 == 0 */
MA_API int  ma_op_gemm_bf16(const void *A, int lda, const void *W, const float *bias, const float *R, int ldr, float *C, int ldc,
                            void *Cb, int ldcb, int M, int N, int K, int act, void *stream);
/* ... in one of its A/B forms (ma_op_gemm_bf16 runs the defaults): `variant` and `tile256` are what the engine options gemm_variant and gemm256 select, with
 * the options' checks -- tile256 outside 0 .. 2 is MA_ERR_INVALID, a variant other than 6 MA_ERR_STATE unless the library was built with MA_EXPERIMENTAL=1.
 * The kernel-level entry points belong to no engine: no engine's options reach them, and nothing set here reaches an engine. */
MA_API int  ma_op_gemm_bf16_tuned(const void *A, int lda, const void *W, const float *bias, const float *R, int ldr, float *C, int ldc,
                                  void *Cb, int ldcb, int M, int N, int K, int act, int variant, int tile256, void *stream);
MA_API int  ma_op_layernorm(const float *x, int ldx, const float *g, const float *b, float eps, float *y, int ldy,
                            int rows, int D, void *stream);
/* O[b,q,h*64+d] = softmax(Q K^T * scale) V, head_dim 64; strides in elements.  round_bf16: 0 fp32 tensors, exact fp32 kernel | 1 fp32 tensors
 * rounded to bf16, first-generation matrix-core kernel | 2 fp32 kernel on bf16-rounded q,k,v | 3 bf16 tensors, first-generation kernel |
 * 4 bf16 tensors, the engine's kernel (csrc/attn2.hpp: packed V^T + swapped-operand 32x32x16 MFMA; all strides multiples of 8) */
MA_API int  ma_op_attention(const float *Q, int q_rs, int q_hs, const float *K, int k_rs, int k_hs, const float *V, int v_rs,
                            int v_hs, float *O, int o_rs, int Sq, int Sk, int H, float scale, int causal_offset /* <0: none */,
                            int round_bf16, void *stream);
/* single-query attention over a KV cache laid out (H, max_seq, 64) of kvdtype; len = number of cached positions.
 * `workspace`: device buffer of ma_decode_attention_workspace_bytes(H) bytes (the split-KV partials). */
MA_API int  ma_op_decode_attention(int kvdtype, const float *q, const void *kcache, const void *vcache, int H, int max_seq,
                                   int len, float *out, void *workspace, void *stream);
MA_API size_t ma_decode_attention_workspace_bytes(int H);
/* the batched decode path's "final" form: one block of `waves` waves (4 | 8 | 16; 0 = the engine's choice for B) per (row, head)
 * over all `len` cached positions, output already normalised and rounded: out = bf16 [B][H*64].  q fp32 [B][H*64]; row b's cache planes start at b * kv_row_stride elements
 * (bf16, each (H, max_seq, 64)).  Replaces [3p] flash_attn_func(q_len = 1) for a batch (meshanything.py:143-162 batch semantics). */
MA_API int  ma_op_decode_attention_rows(const float *q, const void *kcache, const void *vcache, int H, int max_seq, int len, int B,
                                        size_t kv_row_stride, int waves, int halves /* 1 | 2: blocks per (row, head); 2 = in-launch hand-over, 8 waves */,
                                        void *out, void *stream);

/* ---- measurement --------------------------------------------------------------------------------------- */
/* Time the decode step with HIP events on `stream` at KV length `kv_len` (cache contents arbitrary): `steps` back-to-back
 * steps between ONE event pair, (a) eager, (b) as graph replays, (c) once per kernel class with only that class's launches
 * enqueued, so ms[c] / launches[c] is that class's average launch duration including the boundary to the next launch
 * (the view a rocprofv3 kernel trace gives).  Classes: 0 gemv (all weight-streaming launches; out_proj includes the
 * split-KV merge), 1 decode attention, 3 pick/sample. */
typedef struct ma_kernel_timing { int32_t launches[8]; float ms[8]; float step_ms_graph; float step_ms_eager; } ma_kernel_timing;
MA_API int  ma_profile_decode(ma_engine *e, int kv_len, int steps, ma_kernel_timing *out, void *stream);

/* In-kernel timeline of ONE eager decode step at KV length `kv_len`: every weight-streaming / attention launch of the
 * step records, per block, the 100 MHz real-time counter at (0) block start, (1) input vector staged, (2) weights / KV
 * consumed, (3) block end.  host_out[(launch * max_blocks + block) * 4 + point]; kinds[launch]: 0 embed, 1 qkv,
 * 2 attention, 3 out_proj(+merge), 4 fc1, 5 fc2, 6 lm_head; blocks[launch] = grid size.  Diagnostics only. */
MA_API int  ma_trace_decode(ma_engine *e, int kv_len, uint64_t *host_out, int max_launches, int max_blocks, int32_t *kinds,
                            int32_t *blocks, int32_t *n_launches, void *stream);

/* ma_op_gemm_dec_ln (B <= 16, K = 1024): the same GEMM with the LayerNorm prologue of ma_op_rows_prologue inside it -- activation row b =
 * LN(sum of `parts` partial buffers pin[parts][B][1024] + pbias + pres[b]) rounded to bf16; xn_out (B, 1024) fp32 = the LayerNorm
 * output (may be NULL).  The batched decode path's form for small batches ([3p] OPTDecoderLayer post-LN + Linear). */
MA_API int  ma_op_gemm_dec_ln(const void *W, const float *bias, const float *pin, int parts, const float *pbias, const float *pres,
                              const float *ln_g, const float *ln_b, float eps, float *xn_out, float *y, void *yb, int N, int B, int act,
                              void *stream);
/* ---- batched decode step kernels (csrc/gemm_decode.hpp; replace the same nn.Linear calls as ma_op_gemv when B rows step
 * together, meshanything.py:143-162 with batch > 1).  All pointers device.
 * ma_op_gemm_dec: Y[B,N] = act(Xb[B,K] . W[N,K]^T + bias) + res on the bf16 matrix cores; W, Xb bf16; y fp32 and / or yb bf16
 *   output; ksplit > 1: y receives the raw partial sums [ksplit][B][N] (bias / res / act must be null / none).
 * ma_op_gemm_dec_qkv: the fused q/k/v projection epilogue: rows [0,H) -> q (B,H) fp32, [H,2H) / [2H,3H) -> K / V cache
 *   ([B] planes kv_row_stride elements apart, each (H/64, max_seq, 64) bf16) at position `pos`.
 * ma_op_rows_prologue: per-row prologue (pro 0 plain | 1 LayerNorm | 2 merge of the split-KV attention partials): sums
 *   `nparts` partial buffers [nparts][B][K] + bias + res, normalises, writes fp32 (xn_out, may be NULL) and bf16 (xb_out). */
MA_API int  ma_op_gemm_dec(const void *W, const float *bias, const void *xb, const float *res, float *y, void *yb, int N, int K,
                           int B, int act, int ksplit, void *stream);
MA_API int  ma_op_gemm_dec_qkv(const void *W, const float *bias, const void *xb, float *q, void *kcache, void *vcache, int H,
                               int max_seq, int pos, int B, size_t kv_row_stride, void *stream);
MA_API int  ma_op_rows_prologue(int pro, const float *x, int nparts, int B, const float *bias, const float *res, const float *ln_g,
                                const float *ln_b, float ln_eps, const float *attn_ws, int attn_heads, float *xn_out,
                                void *xb_out, int K, void *stream);

/* ---- the token pick and the coordinate argmax on the caller's data (csrc/misc.hpp).  Need no engine; errors via ma_last_error(NULL); every
 * argument is checked before the first launch; all arrays are device memory.
 * ma_op_pick: one decode step's pick_kernel (replaces: [3p] GenerationMixin greedy / sample with TopKLogitsWarper + TopPLogitsWarper and the
 *   generate() bookkeeping, call site meshanything.py:143-162) for B independent rows at step t, one workgroup per row.
 *   logits (B, V) fp32, 3 <= V <= 11264 (the sampler's LDS stage).  nparts > 0: greedy reduces the lm_head's argmax partials part_val / part_idx
 *   (B, nparts) (eos already excluded there when suppressed) instead of sweeping the logits; nparts == 0: both may be NULL.
 *   do_sample: top_k in [1, 64], top_p in (0, 1]; row b's draw is uniforms[b * max_new + t] (uniforms (B, max_new), needs t < max_new), or with
 *   uniforms == NULL the hashed stream of (seed, b, t).  finished (B) int32, in and out: a finished row reports and feeds pad; feeding eos
 *   finishes the row.  forced (B, max_new) int64 or NULL: forced[b * max_new + t], clamped to [0, V), is fed instead of the pick when t < max_new.
 *   tokens (B, max_new) int64: tokens[b * max_new + t] = the reported token when t < max_new, nothing otherwise.  cur_tok (B) int32: the fed
 *   token.  Synchronises `stream`.
 * ma_op_coords_argmax: coords[i] = argmax(logits[i, :]) / nd - 0.5 (lowest index wins ties) for the nf * 9 rows of logits (nf * 9, nd), NaN
 *   where mask[i / 9] == 0 (mask: nf bytes) (replaces: meshanything.py:69-78 + undiscretize, 214-223).  1 <= nf <= 2^24, nd >= 1. */
MA_API int  ma_op_pick(const float *logits, int B, int V, const float *part_val, const int32_t *part_idx, int nparts, int do_sample, int top_k,
                       float top_p, int suppress_eos, const float *uniforms, uint64_t seed, int t, int max_new, const int64_t *forced,
                       int32_t *finished, int64_t *tokens, int32_t *cur_tok, void *stream);
MA_API int  ma_op_coords_argmax(const float *logits, int nf, int nd, const uint8_t *mask, float *coords, void *stream);

/* ---- test aid: holds `n_blocks` workgroups of `lds_bytes` of LDS each (163840 = a whole CU) on the device for `microseconds`
 * (bounded: <= 2 s) on `stream`, doing nothing; ends early once `*release` (device-visible host memory, may be NULL) is non-zero.  Lets a test take CUs away from the engine's stream and check that the fused decode
 * launches -- which need their whole grid resident -- fall back to the five-launch chain instead of failing the request.  Has no
 * reference counterpart (the reference never shares a device between streams). */
MA_API int  ma_op_occupy_cus(int n_blocks, int lds_bytes, int64_t microseconds, const int32_t *release, void *stream);

/* ---- the 16-bit format (MA_DTYPE_BF16, the default, or MA_DTYPE_F16) of the kernel-level entry points above that carry no dtype argument
 * (ma_op_gemm_bf16, ma_op_attention mode 4, ma_op_decode_attention_rows, ma_op_gemm_dec*, ma_op_rows_prologue): their "bf16" operands are then
 * IEEE half.  Per calling thread; parity tests run every 16-bit kernel in both formats.  No reference counterpart. */
MA_API int  ma_op_set_half_dtype(int dtype);

/* ---- test aids: the dense GEMM dispatcher and the LayerNorm row kernel in every form the dense phases use them in (csrc/gemm256.hpp
 * launch_gemm_dense, csrc/gemm.hpp launch_gemm, csrc/dense_ops.hpp launch_ln_rows2 -- the launchers themselves, not a copy of their logic).  Have no
 * reference counterpart (the reference calls nn.Linear / nn.LayerNorm on whole tensors).  Need no engine; errors via ma_last_error(NULL); every
 * argument is checked before the first launch (MA_ERR_INVALID); all arrays are device memory, 16-byte aligned.
 * ma_op_gemm_dense: C = act(A . W^T + bias) + R with everything a dense phase can set.
 *   precision 0: the fp32 kernels (A, W, C fp32; impl 0 = MFMA, 1 = the plain kernel; lda % 4 == 0, K % 32 == 0; no Cb, part, split or KV planes).
 *   precision 1: the 16-bit dispatcher in the format of ma_op_set_half_dtype (A, W, Cb 16-bit; C fp32; either output may be NULL; K % 32 == 0,
 *     lda % 8 == 0, ldc / ldr / ldcb % 4 == 0), `variant` / `tile256` as in ma_op_gemm_bf16_tuned.
 *   Row m of the result leaves for physical row cmap(m) = (m / grp) * gstride + m % grp + off of C / Cb (grp 0: row m); r_mod > 0: the residual row is
 *   m % r_mod.  part 0: all rows | 1: rows [0, M - M % 256) | 2: the rows behind them (needs the identity row map and r_mod 0).
 *   max_parts 2 .. 4: the fp32 output may come as partial sums along K in the buffers C + p * part_stride (bias and residual in part 0), see out_parts.
 *   kv_k / kv_v (both or neither; needs N == 3 * kv_col0, kv_col0 % 64 == 0): the K | V columns [kv_col0, 3 kv_col0) of the leading out_kv_rows rows go
 *   to plane[(m / kv_T) * kv_row_stride + ((col % kv_col0 / 64) * kv_max_seq + m % kv_T) * 64 + col % 64] instead of Cb.
 *   Out (what the dispatcher chose): out_parts (1: not split), out_split_rows (the leading rows that are split; the rows behind them are complete in
 *   part 0), out_kv_rows, out_rows256 (the leading rows computed on 256-row tiles).
 * ma_op_ln_rows: nn.LayerNorm over the D columns of `rows` rows: input row r = x[xin(r) * ldx ..], output row r at physical row yout(r) of y32 (fp32,
 *   optional, may be x itself when the two row maps and leading dimensions agree) and of `act` (optional; act_dtype 0: fp32, 1: the 16-bit format).
 *   parts 2 | 4 (D == 1024 only): the input of rows < split_rows is the sum of `parts` buffers x + p * part_stride.
 *   D % 4 == 0, 0 < D <= 4096, rows > 0, split_rows in [0, rows]; ma_op_layernorm refuses the same shapes. */
typedef struct ma_gemm_dense_args {
    int32_t struct_size;                 /* = sizeof(ma_gemm_dense_args) */
    int32_t precision, impl;
    int32_t M, N, K, act;
    int32_t lda, ldr, ldc, ldcb, r_mod;
    int32_t cmap_grp, cmap_gstride, cmap_off;
    int32_t part;
    int32_t max_parts;                   /* 0 | 1: never split */
    int32_t kv_max_seq, kv_T, kv_col0;
    int32_t variant, tile256;
    int32_t out_parts, out_split_rows, out_kv_rows, out_rows256;
    int64_t part_stride;                 /* floats */
    uint64_t kv_row_stride;              /* elements */
    const void *A, *W;
    const float *bias, *R;
    float *C;
    void *Cb, *kv_k, *kv_v;
} ma_gemm_dense_args;
MA_API int  ma_op_gemm_dense(ma_gemm_dense_args *args, void *stream);
MA_API int  ma_op_ln_rows(const float *x, int ldx, int xin_grp, int xin_gstride, int xin_off, const float *g, const float *b, float eps,
                          float *y32, int ld32, void *act, int lda, int act_dtype, int yout_grp, int yout_gstride, int yout_off,
                          int rows, int D, int parts, int64_t part_stride, int split_rows, void *stream);

/* ---- test aid: dense attention as the dense phases launch it (Dense::attention, csrc/engine_dense.hpp): a batch of samples along grid.z with element
 * strides between the samples, a shortened last sample, the caller's V^T workspace -- csrc/attn.hpp launch_attention and csrc/attn2.hpp
 * launch_attention2 themselves, not a copy of their logic.  Has no reference counterpart (the reference calls attention on whole (B, S, heads, 64)
 * tensors).  Needs no engine; errors via ma_last_error(NULL); every argument is checked before the first launch (MA_ERR_INVALID), what the launchers
 * refuse comes back as MA_ERR_INVALID as well; all arrays are device memory, 16-byte aligned.  Does not synchronise `stream`.
 *   O[b * o_bs + q * o_rs + h * 64 + d] = softmax(Q K^T * scale) V of sample b and head h, head_dim 64;
 *   X[b * x_bs + row * x_rs + h * x_hs + d] for X = Q, K, V: all strides in elements, >= 0 (q_bs == 0: one Q for every sample), row strides >= 64.
 *   kernel 0: the fp32 kernel on fp32 tensors (strides multiples of 4) | 3: the first-generation matrix-core kernel on 16-bit tensors (bf16 only,
 *     strides multiples of 8) | 4: csrc/attn2.hpp on 16-bit tensors in the format of ma_op_set_half_dtype (strides multiples of 8).
 *   causal_offset < 0: every key visible; else query i sees keys <= causal_offset + i.
 *   last_len > 0 (kernel 4 only; < 0: none): the LAST sample has Sq = Sk = last_len <= min(Sq, Sk) rows; what its tensors hold behind them is neither
 *     read nor written.
 *   vt / vt_elems (kernel 4): the V^T workspace of at least ma_attention_vt_workspace_elems(Sk, H, batch) 16-bit elements. */
typedef struct ma_attn_dense_args {
    int32_t struct_size;                 /* = sizeof(ma_attn_dense_args) */
    int32_t kernel;
    int32_t Sq, Sk, H, causal_offset, batch, last_len;
    float scale;
    int32_t q_rs, q_hs, k_rs, k_hs, v_rs, v_hs, o_rs;
    uint64_t q_bs, k_bs, v_bs, o_bs;     /* elements */
    uint64_t vt_elems;
    const void *Q, *K, *V;
    void *O, *vt;
} ma_attn_dense_args;
MA_API int  ma_op_attention_dense(ma_attn_dense_args *args, void *stream);
MA_API size_t ma_attention_vt_workspace_elems(int Sk, int H, int batch);

/* ---- measurement aid: dst[0, bytes) = src[0, bytes) as a 16-byte-per-lane streaming copy; bytes % 16 == 0; mode 0 = 2048 blocks grid-stride with
 * non-temporal accesses, 1 = one element per thread with plain accesses, 2 = one element per thread non-temporal.  bench.py times all three and
 * reports the box's achievable HBM rate next to the 8 TB/s vendor number.  No reference counterpart. */
MA_API int  ma_op_stream_copy(void *dst, const void *src, size_t bytes, int mode, void *stream);

/* ---- persistent decode step (csrc/experimental/persist.hpp; only in libraries built with MA_EXPERIMENTAL=1 -- measured 1.3-1.6x slower than the launch
 * chain; the product build answers MA_ERR_STATE / 0): the whole batch-1 greedy step as ONE resident launch instead of the
 * 123-launch chain.  Select with ma_engine_set_option(e, "decode_impl", 1); it is used when ma_engine_persist_available()
 * and the call is batch 1 / greedy, otherwise the chain runs.  replaces: the same reference calls as ma_generate's steps
 * (shape_opt.py:318-364,403-410,155; meshanything.py:143-151). */
MA_API int  ma_engine_persist_available(ma_engine *e);
/* host_out: 256 * 320 uint64 (comm wave of every workgroup: start, then per edge {sweep start, gather done}, end; 100 MHz
 * ticks), followed by 256 * 512 uint64 (compute wave 0: per weight op {input ready, weights landed, dots done, published},
 * per attention {partial published, partials gathered, merged output published}) */
MA_API int  ma_persist_trace(ma_engine *e, int kv_len, uint64_t *host_out, int32_t *n_events, void *stream);
/* copies the logits of the most recent decode step of batch row `row` (codebook_size + 3 floats) into a device buffer */
MA_API int  ma_engine_read_logits(ma_engine *e, int row, float *out, void *stream);
/* test aid for the decode step's embedding table (engine option "embed_table": row v = input_layer(codebook[v]) + bias, built once per set of
 * weights; the token pick writes the next step's layer-0 input from it, so that the step has no embedding launch).  Writes n rows of `hidden` floats
 * to `out` (device).  what 0: table rows row0 .. row0 + n - 1.  what 1: the embedding launch's own value for the tokens row0 + 3 .. row0 + n + 2 in
 * front of its positional adds (uses batch row 0's state record). */
MA_API int  ma_engine_embed_rows(ma_engine *e, int what, int row0, int n, float *out, void *stream);

/* ---- watertight remeshing of a mesh input (csrc/watertight.hpp).  replaces: export_to_watertight (mesh_to_pc.py:13-40), i.e.
 * mesh2sdf.core.compute + skimage.measure.marching_cubes(np.abs(sdf), level).  Needs no engine; errors via ma_last_error(NULL).
 *
 * ma_op_mesh_udf: unsigned distance to a triangle mesh on a size^3 grid, field (size, size, size) fp32 with axes x, y, z; grid point
 *   (i, j, k) sits at -1 + 2 * (i, j, k) / size.  verts (nv, 3) fp32 and faces (nf, 3) int32 are device arrays; vertices must be finite
 *   (the caller checks).  Narrow band: every grid point within 2 cells of a triangle's index-space bounding box holds the fp32
 *   distance minimum over those triangles, every other point +inf; so every point closer than 2 * (2 / size) to the mesh is exact.
 *   A face whose inradius is below 1/128 of a cell (collinear or near-collinear) counts as its three edges: off by at most its inradius.
 *   Bitwise reproducible.  2 <= size <= 512, 1 <= nf <= MA_MESH_UDF_MAX_FACES.  workspace: ma_mesh_udf_workspace_bytes(nf) bytes of
 *   device memory (0 for an nf outside that range). */
#define MA_MESH_UDF_MAX_FACES (1 << 28)
MA_API int  ma_op_mesh_udf(const float *verts, int nv, const int32_t *faces, int nf, int size, float *field, void *workspace, size_t ws_bytes,
                           void *stream);
MA_API size_t ma_mesh_udf_workspace_bytes(int nf);
/* ma_op_marching_cubes: the level set field == level of a (nx, ny, nz) fp32 grid (C order).  verts (max_verts, 3) fp32 in index space
 *   (as skimage returns them), one per grid edge that crosses the level, placed by linear interpolation; tris (max_tris, 3) int32 vertex
 *   ids in cell-linear order, table order inside a cell, each normal (b - a) x (c - a) pointing toward increasing values.
 *   counts: host int64[2] = {vertices, triangles}, always written.  verts == tris == NULL: count only.  A result larger than
 *   max_verts / max_tris: MA_ERR_CAPACITY, nothing written.  Synchronises `stream`.  workspace: ma_marching_cubes_workspace_bytes. */
MA_API int  ma_op_marching_cubes(const float *field, int nx, int ny, int nz, float level, float *verts, int64_t max_verts, int32_t *tris,
                                 int64_t max_tris, int64_t *counts, void *workspace, size_t ws_bytes, void *stream);
MA_API size_t ma_marching_cubes_workspace_bytes(int nx, int ny, int nz);
/* host only: the marching-cubes table the kernel reads.  tris: 256 * 3 * max_tris_per_cell int8 (edge ids, -1 padded), edges: 12 * 4
 *   int8 (corner offset dx, dy, dz, axis); corner c of a cell is at (c & 1, c >> 1 & 1, c >> 2 & 1), bit c of a case is set when that
 *   corner is >= level.  Any pointer may be NULL (ask for max_tris_per_cell first). */
MA_API int  ma_mc_table(int8_t *tris, int8_t *edges, int32_t *max_tris_per_cell);

/* ---- surface sampling of a mesh (csrc/surface_sample.hpp).  replaces: mesh.sample(n, return_index=True) + face_normals[face_idx]
 * (mesh_to_pc.py:50-54), i.e. mesh_input.mesh_to_pc_normal.  Needs no engine; errors via ma_last_error(NULL); every argument is checked
 * before the first launch.  Device arrays, caller-owned workspace, asynchronous on `stream`.  All arithmetic is float64 in numpy's
 * order without FMA contraction, so for the same draws the output is mesh_input.py's bit for bit, except that the cumulative sum of
 * the areas is a parallel scan: it may round differently from np.cumsum, which can move a draw that lands within that rounding of
 * a face boundary to the neighbouring face.
 *
 * ma_op_mc_vertices_to_frame: verts (nv, 3) float64 = ((double(index_verts) / size) * 2 - 1) / to_orig_scale + center (host double[3]),
 *   the marching-cubes output of ma_op_marching_cubes mapped back to the input's frame (watertight.export_to_watertight).
 * ma_op_surface_cdf: per face of verts (nv, 3) float64 / faces (nf, 3) int32, the unit normal (normals (nf, 3) float64, 0 for a
 *   zero-area face) and the cumulative area (cum (nf) float64, non-decreasing, unchanged across a zero-area face); cum[nf - 1] is the
 *   total area, which the caller reads back and checks (> 0) before it draws.  workspace: ma_surface_sample_workspace_bytes(nf) bytes
 *   (0 for an nf outside [1, MA_SURFACE_SAMPLE_MAX_FACES]).
 * ma_op_sample_surface: `count` points from the draws u (count) and uv (count, 2) in [0, 1): face = the first j with
 *   cum[j] > u * cum[nf - 1] (at most nf - 1), (a, b) = uv folded to (1 - a, 1 - b) when a + b > 1, point = (t0 + a (t1 - t0)) +
 *   b (t2 - t0); out (count, 6) float16 = point, normals[face], each correctly rounded from float64; face_idx (count) int64 or NULL. */
#define MA_SURFACE_SAMPLE_MAX_FACES (1 << 28)
MA_API int  ma_op_mc_vertices_to_frame(const float *index_verts, int nv, int size, double to_orig_scale, const double *center, double *verts,
                                       void *stream);
MA_API int  ma_op_surface_cdf(const double *verts, int nv, const int32_t *faces, int nf, double *normals, double *cum, void *workspace,
                              size_t ws_bytes, void *stream);
MA_API size_t ma_surface_sample_workspace_bytes(int nf);
MA_API int  ma_op_sample_surface(const double *verts, int nv, const int32_t *faces, int nf, const double *normals, const double *cum,
                                 const double *u, const double *uv, int count, uint16_t *out, int64_t *face_idx, void *stream);
/* host only: out[i] = float16 bits of x[i], rounded to nearest even in one step (numpy's astype(float16)): the conversion
 *   ma_op_sample_surface applies, exposed so that it can be checked without a device. */
MA_API int  ma_f64_to_f16(const double *x, int64_t n, uint16_t *out);

/* ---- best-of-N sampling: scores of candidate meshes against the cloud they were generated from (csrc/mesh_score.hpp).  Has no reference
 * counterpart (the reference draws one mesh per cloud; a bad draw is re-run by hand with another seed).  Needs no engine; errors via
 * ma_last_error(NULL); every argument is checked before the first HIP call.  Device arrays, caller-owned workspace, asynchronous on `stream`.
 *
 * ma_op_score_meshes: coords (B, F, 3, 3) fp32 = the detokenizer's output as it is: a face with any non-finite coordinate is invalid and
 *   skipped (the NaN rows of meshanything.py:69-78); every vertex is multiplied by mesh_scale before use.  cloud (B / n_per_cloud, P,
 *   cloud_ld) fp32 with xyz in the first three columns of a row, cloud_ld = 3 or 6 (a pc_normal tensor); candidate b is scored against
 *   cloud b / n_per_cloud.  scores (B, 4) fp32:
 *     [0] cloud to mesh: the mean over the P points of the distance to the nearest valid face; a face whose inradius is below 2^-20 (fp32
 *         cannot resolve its plane) counts as its three edges, as in ma_op_mesh_udf
 *     [1] mesh to cloud: sum_f area_f * (1/7) sum_k nn(q_fk) / sum_f area_f over the valid faces, q_fk = the 3 vertices, the 3 edge
 *         midpoints and the centroid of face f, nn = the distance to the nearest cloud point
 *     [2] sum_f area_f of the scaled mesh      [3] the number of valid faces
 *   [0] = [1] = +inf for a candidate without a valid face, [1] = +inf when every valid face has zero area; no output is NaN.
 *   Bitwise reproducible, and a candidate's four numbers do not depend on B or on NaN rows between its valid faces: per-point and
 *   per-face terms go to the workspace in fp32 (pt_dist (B, P) | face_nn (B, F) | face_area (B, F), -1 = invalid; each part aligned to
 *   256 bytes) and are summed in fp64 in a fixed order; no float atomics.
 *   B >= 1, B % n_per_cloud == 0, 1 <= F <= MA_SCORE_MESHES_MAX_FACES, 1 <= P <= MA_SCORE_MESHES_MAX_POINTS, mesh_scale finite and > 0.
 *   workspace: ma_score_meshes_workspace_bytes(B, F, P) bytes of device memory (0 for arguments outside those limits). */
#define MA_SCORE_MESHES_MAX_FACES (1 << 20)
#define MA_SCORE_MESHES_MAX_POINTS (1 << 20)
MA_API int    ma_op_score_meshes(const float *coords, int B, int F, const float *cloud, int cloud_ld, int P, int n_per_cloud, float mesh_scale,
                                 float *scores, void *workspace, size_t ws_bytes, void *stream);
MA_API size_t ma_score_meshes_workspace_bytes(int B, int F, int P);

/* ---- agreement of a candidate mesh's face normals with the cloud's normals (csrc/mesh_normals.hpp): the normal-consistency term of
 * best-of-N sampling and the winding of the written faces.  Has no reference counterpart (the reference hands the cloud's normals to the
 * encoder and never reads them again; its winding comes from trimesh's fix_normals).  Needs no engine; errors via ma_last_error(NULL);
 * every argument is checked before the first HIP call.  Device arrays, caller-owned workspace, asynchronous on `stream`.
 *
 * ma_op_mesh_normals: coords, cloud, n_per_cloud and mesh_scale as for ma_op_score_meshes, except that cloud_ld must be 6: columns 0..2
 *   are xyz, columns 3..5 the normal, used as given (not re-normalised; finite values are the caller's duty).  Per valid face f with the
 *   scaled vertices A, B, C, all fp32 and without FMA contraction, so that a float32 restatement that rounds every operation gives the same bits:
 *     n = (B - A) x (C - A), l2 = n . n; the face is measurable when l2 is finite and > 0, then nh = n / sqrtf(l2)
 *     q_0..q_6 = A, B, C, the midpoints of AB, BC, CA, the centroid (the quadrature points of ma_op_score_meshes)
 *     j_k = the cloud index p that minimises the pair (d, p), d = fl(fl(dx * dx + dy * dy) + dz * dz), dx = fl(q_k.x - x_p), ...: a total
 *           order, the lowest index wins ties; a NaN or +inf key never wins, so j_k is always in 0 .. P - 1 (0 when every key is)
 *     t_k = fl(fl(nh.x * m.x + nh.y * m.y) + nh.z * m.z), m = the normal of cloud row j_k
 *     a_f = (t_0 + ... + t_6, in that order) * fl(1/7)          signed agreement; < 0: the face is wound against the cloud
 *     u_f = (|t_0| + ... + |t_6|) * fl(1/7)                     unsigned consistency, independent of the winding
 *     area_f = 0.5 * sqrtf(l2), the area ma_op_score_meshes uses; a face that is not measurable has a_f = u_f = area_f = 0 and adds
 *              nothing below
 *   face_agree (B, F) fp32 = a_f, 0 for an invalid or not measurable face.  nscores (B, 4) fp32:
 *     [0] NC = sum_f area_f * u_f / sum_f area_f over the measurable faces       [1] the share of that area whose a_f < 0
 *     [2] sum_f area_f over the measurable faces (at most FLT_MAX)               [3] the number of valid faces
 *   [0] = [1] = 0 (the worst NC) without a measurable face; no output is NaN or infinite.  The cloud -> mesh direction of normal
 *   consistency is not computed: the nearest face of a point is tied between the faces of a shared edge.
 *   Bitwise reproducible, and a candidate's numbers do not depend on B or (nscores) on NaN rows between its valid faces: the per-face terms
 *   are summed in fp64 in the fixed order of ma_op_score_meshes; no float atomics.  workspace: face_abs (B, F) fp32 = u_f | face_area
 *   (B, F) fp32, -1 = invalid face, 0 = not measurable | nn_idx (B, F, 7) int32 = j_k, -1 = invalid face; each part aligned to 256 bytes.
 *   Limits as for ma_op_score_meshes.  workspace: ma_mesh_normals_workspace_bytes(B, F) bytes of device memory (0 outside the limits). */
MA_API int    ma_op_mesh_normals(const float *coords, int B, int F, const float *cloud, int cloud_ld, int P, int n_per_cloud, float mesh_scale,
                                 float *face_agree, float *nscores, void *workspace, size_t ws_bytes, void *stream);
MA_API size_t ma_mesh_normals_workspace_bytes(int B, int F);

/* ---- fit of a generated mesh to the cloud it was generated from (csrc/mesh_fit.hpp; --fit_iters): one pairing of the cloud's points with
 * the mesh's faces and the per-face sums of the point-to-plane normal equations; the caller assembles and solves the vertex system.  Has no
 * reference counterpart (the reference never moves a vertex).  Needs no engine; errors via ma_last_error(NULL); the scalar arguments are
 * checked before the first HIP call.  Device arrays, caller-owned workspace.  UNLIKE the other ma_op_*, the call waits for `stream`: the
 * kernels check the arrays themselves, and a face index outside 0 .. V - 1, a non-finite vertex of a face or a non-finite cloud row is a
 * returned MA_ERR_INVALID (such a face or point takes no part, so the launch itself stays in bounds).
 *
 * ma_op_mesh_fit_pairs: verts (V, 3) fp32 in the CLOUD's units (the caller multiplies by its mesh_scale), faces (M, 3) int32 into them,
 *   cloud (P, cloud_ld = 6) fp32: xyz, then the normal m, used as given.  All arithmetic is fp32 without FMA contraction, every operation
 *   rounded on its own in the order csrc/mesh_fit.hpp states, so that a float32 restatement gives the same bits.
 *   A face is admissible when its indices differ and its inradius |n| / perimeter exceeds `flat` (the rule of ma_op_mesh_udf and
 *   ma_op_score_meshes, which pass 2^-20), and, with min_cos > 0, for a point whose normal has |nh . m| >= min_cos (nh = the face's unit normal).
 *   Every point with a non-zero normal is paired with the admissible face that holds the point c nearest to it, the lowest face index on
 *   equal squared distance, provided |p - c|^2 <= dist * dist:
 *     pt_face (P) int32    the face, -1 = unpaired
 *     pt_w (P, 3) fp32     the weights of c on the face's three vertices (0 when unpaired)
 *     workspace            pt_s (P) fp32 = s = m . (p - c) | pt_r2 (P) fp32 = |p - c|^2 | a status word; each part aligned to 256 bytes
 *   face_sums (M, MA_MESH_FIT_NSUM) int64, per face over its paired points: [0] their number; then in 2^-32 fixed point (every fp32 term
 *   converted to double, times 2^32, rounded half to even, summed as int64):
 *     [1] sum s * s      [2] sum |p - c|^2      [3 + 3 k + a] g[k][a] = sum (w_k * s) * m_a, k = the face's vertex 0..2, a = x, y, z
 *     [12 + 6 kl + ac] H[kl][ac] = sum (w_k * w_l) * (m_a * m_c), kl in (00, 01, 02, 11, 12, 22), ac in (xx, xy, xz, yy, yz, zz)
 *   Integer sums: the same bits on every run, for every launch shape and workspace; no floating-point atomics.  With dist <= 1 and unit
 *   normals every term is at most 1 and the sums stay below 2^55.
 *   1 <= M <= MA_MESH_FIT_MAX_FACES, 1 <= V <= 3 M, 1 <= P <= MA_MESH_FIT_MAX_POINTS, 0 < dist <= 1, 0 <= min_cos < 1 (0 = no normal test),
 *   flat >= 0.  workspace: ma_mesh_fit_workspace_bytes(V, M, P) bytes of device memory (0 for arguments outside those limits). */
#define MA_MESH_FIT_MAX_FACES 4096
#define MA_MESH_FIT_MAX_POINTS (1 << 22)
#define MA_MESH_FIT_NSUM 48
MA_API int    ma_op_mesh_fit_pairs(const float *verts, int V, const int32_t *faces, int M, const float *cloud, int cloud_ld, int P, float dist,
                                   float min_cos, float flat, int32_t *pt_face, float *pt_w, int64_t *face_sums, void *workspace, size_t ws_bytes,
                                   void *stream);
MA_API size_t ma_mesh_fit_workspace_bytes(int V, int M, int P);

/* ---- normals of a raw point cloud, for --input_type pc_xyz (csrc/pc_normals.hpp).  Has no reference counterpart: the reference takes only
 * clouds that already carry unit normals (pc_normal), or meshes.  Needs no engine; errors via ma_last_error(NULL); every argument is
 * checked before the first HIP call.  Device arrays, caller-owned workspace, asynchronous on `stream`.  No atomics: bitwise reproducible.
 *
 * ma_op_pc_knn: for the Q rows query_idx[q] (int32) of ref (N, ref_ld) fp32, xyz in the first three columns, ref_ld = 3 or 6 -- or for
 *   every row when query_idx is NULL (then Q must equal N) -- the k nearest rows of ref: nbr_idx (Q, k) int32 and nbr_d2 (Q, k) fp32,
 *   nearest first.  The key of row r for a query at (qx, qy, qz) is exactly
 *       d = fl32(fl32(dx * dx + dy * dy) + dz * dz),  dx = fl32(qx - rx), dy = fl32(qy - ry), dz = fl32(qz - rz)
 *   (no FMA contraction; a NaN key, which only non-finite coordinates produce, counts as +inf) and neighbours are ordered by the pair
 *   (d, r) ascending.  That is a total order: a point is its own neighbour at distance 0, duplicates are ordinary points, and a numpy
 *   float32 restatement gives the same bits.  The reference range is searched in `splits` chunks by separate workgroups whose partial
 *   lists a second kernel merges; the result does not depend on splits, bit for bit.  splits = 0: the implementation's choice, a
 *   function of N and Q alone.  An index of query_idx outside [0, N) is clamped into it.
 *   MA_PC_KNN_MIN_K <= k <= MA_PC_KNN_MAX_K, k <= N <= MA_PC_KNN_MAX_POINTS, 1 <= Q <= MA_PC_KNN_MAX_QUERIES, 0 <= splits <=
 *   MA_PC_KNN_MAX_SPLITS.  workspace: ma_pc_knn_workspace_bytes(N, Q, k, splits) bytes of device memory (0 for arguments outside those
 *   limits).
 * ma_op_pc_normals: per query q, from the k rows nbr_idx[q] of ref, in float64 without FMA contraction: the centroid c = (sum x) / k, the
 *   covariance (sum (x - c)(x - c)^T) / k, both summed in list order; eigvals (Q, 3) float64 ascending and normals (Q, 3) float64 = the
 *   unit eigenvector of the smallest (cyclic Jacobi), signed so that its component of largest magnitude is positive, the lowest axis
 *   on ties.  Always unit and finite: k coincident neighbours give (0, 0, 1) and zero eigenvalues; a collinear neighbourhood gives
 *   some unit perpendicular, unspecified but deterministic.  An index outside [0, N) is clamped into it.  Same limits on N, Q, k. */
#define MA_PC_KNN_MIN_K 3
#define MA_PC_KNN_MAX_K 32
#define MA_PC_KNN_MAX_POINTS (1 << 22)
#define MA_PC_KNN_MAX_QUERIES (1 << 20)
#define MA_PC_KNN_MAX_SPLITS 64
MA_API int    ma_op_pc_knn(const float *ref, int N, int ref_ld, const int32_t *query_idx, int Q, int k, int splits, int32_t *nbr_idx,
                           float *nbr_d2, void *workspace, size_t ws_bytes, void *stream);
MA_API size_t ma_pc_knn_workspace_bytes(int N, int Q, int k, int splits);
MA_API int    ma_op_pc_normals(const float *ref, int N, int ref_ld, const int32_t *nbr_idx, int Q, int k, double *normals, double *eigvals,
                               void *stream);

/* ---- farthest-point sampling of a point cloud, for --point_sampling fps (csrc/pc_fps.hpp).  Has no reference counterpart: the reference
 * keeps np.random.choice(N, n, replace=False) rows.  Needs no engine; errors via ma_last_error(NULL); every argument is checked before
 * the first HIP call.  Device arrays, caller-owned workspace, asynchronous on `stream`; the host reads nothing back between the picks.
 * No atomics, and no workgroup waits for another inside a launch: bitwise reproducible.
 *
 * ma_op_pc_fps: n of the N rows of ref (N, ref_ld) fp32, xyz in the first three columns, ref_ld = 3 or 6: idx (n) int32 in pick order and
 *   d2 (n) fp32.  With p_i the xyz of row i and
 *       key(a, b) = fl32(fl32(dx * dx + dy * dy) + dz * dz),  dx = fl32(a.x - b.x), dy = fl32(a.y - b.y), dz = fl32(a.z - b.z)
 *   (the key of ma_op_pc_knn, no FMA contraction):  m_i = +inf for every i; for t = 0 .. n - 1:  idx[t] = s_t;  d2[t] = m_{s_t} (+inf
 *   at t = 0);  m_i = min(m_i, key(p_i, p_{s_t})) for every i;  m_{s_t} = -1, so a picked row is never picked again (duplicates of it
 *   are ordinary points);  s_{t+1} = the i of greatest m_i, the lowest index among equals.  s_0 = start, a row in [0, N); with start =
 *   -1 it is the row farthest from the bounding box's centre: per axis lo = min, hi = max, c = fl32(fl32(lo + hi) * 0.5), s_0 = the i of
 *   greatest key(p_i, c), the lowest index among equals -- deterministic, no random numbers.  It follows that the n indices are
 *   distinct for any N >= n, that d2[1:] is non-increasing, exactly, and that after n picks every row lies within sqrt(d2[n - 1]) of a
 *   picked one.  A numpy float32 restatement gives the same indices and the same bits.  Non-finite coordinates: unspecified picks,
 *   every index in [0, N), nothing read or written out of bounds.
 *   form: 1 = one workgroup keeps the cloud in registers for all n picks, one launch, N <= MA_PC_FPS_ONE_MAX_POINTS (a larger N is an
 *   error); 2 = one launch per pick over many workgroups, any N; 0 = the implementation's choice, a function of N alone.  The result
 *   does not depend on form, bit for bit.
 *   1 <= n <= N <= MA_PC_FPS_MAX_POINTS, n <= MA_PC_FPS_MAX_PICKS.  workspace: ma_pc_fps_workspace_bytes(N, n, form) bytes of device
 *   memory (0 for arguments outside those limits); its contents on entry do not matter. */
#define MA_PC_FPS_MAX_POINTS (1 << 22)
#define MA_PC_FPS_MAX_PICKS  (1 << 16)
#define MA_PC_FPS_ONE_MAX_POINTS (1 << 14)
MA_API int    ma_op_pc_fps(const float *ref, int N, int ref_ld, int n, int start, int form, int32_t *idx, float *d2, void *workspace,
                           size_t ws_bytes, void *stream);
MA_API size_t ma_pc_fps_workspace_bytes(int N, int n, int form);

/* ---- neighbours of EVERY point over a uniform cell grid, for statistical outlier removal, --outlier_k (csrc/pc_grid.hpp).  Has no
 * reference counterpart.  Needs no engine; errors via ma_last_error(NULL); every argument is checked before the first HIP call.  Device
 * arrays (origin and dims are HOST arrays of 3), caller-owned workspace, asynchronous on `stream`.
 *
 * ma_op_pc_knn_grid: every row of ref (N, ref_ld) fp32, xyz in the first three columns, ref_ld = 3 or 6, is a query.  The key of row r for a
 *   query at (qx, qy, qz) is ma_op_pc_knn's, exactly
 *       d = fl32(fl32(dx * dx + dy * dy) + dz * dz),  dx = fl32(qx - rx), dy = fl32(qy - ry), dz = fl32(qz - rz)
 *   (no FMA contraction; a NaN key counts as +inf), and neighbours are ordered by the pair (d, r) ascending, a total order.  The k best
 *   under a total order are unique: the result does not depend on the grid, bit for bit, and nbr_idx (N, k) int32 / nbr_d2 (N, k) fp32,
 *   in the original row order, EQUAL what ma_op_pc_knn(ref, N, ref_ld, NULL, N, k, ...) writes.  mean_dist (N) float64 =
 *   (sum_j sqrt((double) d_j)) / k, summed in list order without contraction; the list includes the point itself at distance 0.  Each
 *   of the three outputs may be NULL, at least one must be given; with mean_dist alone the lists are never written to memory.
 *   The grid only decides the time.  origin[3] finite, cell finite and > 0, dims[3] each in 1 .. MA_PC_GRID_MAX_DIM with a product of
 *   at most MA_PC_GRID_MAX_CELLS.  Per axis face[i] = fl32(origin + fl32(i * cell)), i = 0 .. dim, and the cell of a coordinate x is
 *   the largest i in [0, dim - 1] with i = 0 or face[i] <= x, by comparisons alone: the border cells are unbounded outward, a point
 *   outside the box belongs to the nearest border cell (fit the box to the object, not to its strays), a NaN goes to cell 0.  A
 *   query's block of cells grows ring by ring from its own cell until it is the whole grid or the list is full with its k-th key
 *   strictly below fl32(b * b) for the distance b = fl32(q - face) to every side of the block that is not a grid border.  The order of
 *   the points inside a cell comes from atomics and differs between runs; no output depends on it.  Non-finite coordinates: unspecified
 *   neighbours, nothing read or written out of bounds.
 *   MA_PC_KNN_MIN_K <= k <= MA_PC_KNN_MAX_K, k <= N <= MA_PC_GRID_MAX_POINTS.  workspace: ma_pc_knn_grid_workspace_bytes(N, k, nx, ny, nz)
 *   bytes of device memory (0 for arguments outside those limits); its contents on entry do not matter. */
#define MA_PC_GRID_MAX_POINTS (1 << 22)
#define MA_PC_GRID_MAX_DIM 128
#define MA_PC_GRID_MAX_CELLS (1 << 21)
MA_API int    ma_op_pc_knn_grid(const float *ref, int N, int ref_ld, int k, const float *origin, float cell, const int32_t *dims, int32_t *nbr_idx,
                                float *nbr_d2, double *mean_dist, void *workspace, size_t ws_bytes, void *stream);
MA_API size_t ma_pc_knn_grid_workspace_bytes(int N, int k, int nx, int ny, int nz);

/* ---- Euclidean clustering: the connected parts of a cloud, for --cluster_radius (csrc/pc_cluster.hpp).  Has no reference counterpart.
 * Needs no engine; errors via ma_last_error(NULL); every argument is checked before the first HIP call.  Device arrays (origin, dims and
 * pairs_bound are HOST pointers), caller-owned workspace.  NOT asynchronous: the call reads the pair bound back on `stream` before it
 * launches the search, as ma_op_marching_cubes reads its counts.
 *
 * ma_op_pc_cluster: rows i and j of ref (N, ref_ld) fp32, xyz in the first three columns, ref_ld = 3 or 6, are LINKED iff
 *       d(i, j) = fl32(fl32(dx * dx + dy * dy) + dz * dz) <= r2,  dx = fl32(x_i - x_j), dy = fl32(y_i - y_j), dz = fl32(z_i - z_j)
 *   (the key of ma_op_pc_knn, no FMA contraction; a NaN key links nothing) with r2 = fl32(radius * radius), computed once on the host.
 *   The key is symmetric (fl32(a - b) = -fl32(b - a)), equality is included, exact duplicates are always linked.  labels (N) int32:
 *   labels[i] = the smallest row index in the connected component of i under those links.  A function of the cloud and the radius
 *   alone: it does not depend on the grid, on the order the atomics resolve in, or on the run, so a numpy restatement gives EQUAL
 *   labels.  sizes (N) int32, or NULL: sizes[l] = the number of rows with label l where labels[l] == l, 0 elsewhere.
 *   The grid (origin, cell, dims: as for ma_op_pc_knn_grid, the same faces and cell rule) only decides the time.  A query's block of
 *   cells grows ring by ring from its own cell until it is the whole grid or fl32(b * b) > r2 for the distance b = fl32(q - face) to
 *   every side of the block that is not a grid border; every point outside the block then has a key above r2.  The components come
 *   from a lock-free union-find whose every access is an agent-scope atomic; no thread waits for another.
 *   The pair bound, a guard against a radius the size of the cloud (an N^2 job): before the search, sum over the cells c of n_c * (the
 *   points in the block of R = floor(radius / cell) + 2 rings around c, clipped to the grid), 64 bits, an upper bound of the keys the
 *   search evaluates.  It is written to *pairs_bound (if given) and, if it exceeds max_pairs (0 = MA_PC_CLUSTER_MAX_PAIRS), the call
 *   fails with MA_ERR_INVALID, the message giving both numbers, and launches nothing further.  So that the bound holds whatever the
 *   rounding of the faces, a grid whose float32 faces R + 1 cells apart are not more than the radius apart (an origin huge against
 *   the cell) is refused with MA_ERR_INVALID before any device work.
 *   MA_PC_CLUSTER_MAX_PAIRS is a guard value, not a tuning knob: 2^36.  Measured on an MI355X: a uniform cloud of
 *   2^22 points at the radius whose bound is 6.7e10, just under it, takes 42 ms as a whole, far inside the 2 s the value was to be lowered
 *   for, so it was not lowered.
 *   Non-finite coordinates: such a row links nothing and is its own component; nothing is read or written out of bounds.
 *   1 <= N <= MA_PC_GRID_MAX_POINTS, radius finite and > 0, the grid limits of ma_op_pc_knn_grid, radius / cell <= 8.  workspace:
 *   ma_pc_cluster_workspace_bytes(N, nx, ny, nz) bytes of device memory (0 for arguments outside those limits): the grid's layout, the
 *   parent array and the 8-byte total; its contents on entry do not matter. */
#define MA_PC_CLUSTER_MAX_PAIRS  (1ull << 36)
MA_API int    ma_op_pc_cluster(const float *ref, int N, int ref_ld, float radius, const float *origin, float cell, const int32_t *dims,
                               uint64_t max_pairs /* 0 = MA_PC_CLUSTER_MAX_PAIRS */, int32_t *labels, int32_t *sizes /* or NULL */,
                               uint64_t *pairs_bound /* host pointer or NULL: the bound that was computed */,
                               void *workspace, size_t workspace_bytes, void *stream);
MA_API size_t ma_pc_cluster_workspace_bytes(int N, int nx, int ny, int nz);

/* ---- Moving-least-squares smoothing: every row onto the plane fitted to its radius neighbourhood, for --smooth_radius
 * (csrc/pc_smooth.hpp); PCL's MovingLeastSquares without the polynomial.  Has no reference counterpart.  Needs no engine; errors via
 * ma_last_error(NULL); every argument is checked before the first HIP call.  Device arrays (origin, dims and pair_bound are HOST
 * pointers), caller-owned workspace.  NOT asynchronous: the call reads the pair bound back on `stream` before it launches the long
 * kernel, as ma_op_pc_cluster does.
 *
 * ma_op_pc_smooth: ref (N, ref_ld) fp32, xyz in the first three columns, ref_ld = 3 or 6; r2 = fl32(radius * radius), computed once on
 *   the host.  For row i at position q:
 *   Neighbours: every row j, i itself included, with
 *       d = fl32(fl32(dx * dx + dy * dy) + dz * dz) <= r2,  dx = fl32(q_x - x_j), dy = fl32(q_y - y_j), dz = fl32(q_z - z_j)
 *   (the key of ma_op_pc_knn and the link rule of ma_op_pc_cluster, no FMA contraction; a NaN key is not a neighbour; equality is
 *   included).  count (N) int32 = the number of neighbours: a function of the cloud and the radius alone, EQUAL to a brute force.
 *   Weights, float64, no contraction: s = (double)d / (double)r2, u = 1 - s, w = (u * u) * u.  A polynomial, so every term is exact IEEE
 *   arithmetic that a numpy restatement reproduces bit for bit; it is 0 at the rim, so a row whose key equals r2 changes count alone.
 *   Moments over the neighbours with e = ((double)dx, (double)dy, (double)dz), the differences of the key: S0 = sum w, S1 = sum w * e,
 *   S2_ab = sum (w * e_a) * e_b (six entries), summed in the order the walk visits the rows.  That order depends on the grid and, inside
 *   a cell, on the order the build's atomics resolved in: the float outputs are NOT bit-reproducible, they agree with any other
 *   summation order to what float64 resolves (DESIGN.md section 17 has the measured figures).
 *   Plane: mu = S1 / S0, C = S2 / S0 - mu mu^T; the cyclic Jacobi of ma_op_pc_normals; eigvals (N, 3) float64 ascending; normals (N, 3)
 *   float64 = the unit eigenvector of the smallest, its component of largest magnitude positive, the lowest axis on ties.
 *   Projection onto the plane through the weighted centroid q - mu: t = (mu_x * n_x + mu_y * n_y) + mu_z * n_z, moved (N, 3) float64 =
 *   (double)q - t * n per component.  |moved - q| <= |mu| <= radius.
 *   A row STAYS where it is -- moved = (double)q, normal (0, 0, 1), eigenvalues 0 -- if count < min_count, if all its neighbours
 *   coincide, or if anything comes out non-finite; such a row is recognisable from count and the eigenvalues.
 *   No polynomial (order-2) fit is made: a plane projection shrinks a curved surface by roughly radius^2 / (8 * its radius of
 *   curvature) and rounds an edge over a width of the radius.
 *   Each of moved, normals, eigvals and count may be NULL, at least one must be given; outputs are in the ORIGINAL row order and no
 *   neighbour list is ever written to memory.
 *   The grid (origin, cell, dims: as for ma_op_pc_knn_grid, the same faces and cell rule) only decides the time and the summation
 *   order; the walk and its stop rule are ma_op_pc_cluster's.  The pair bound is ma_op_pc_cluster's too: computed before the long
 *   kernel, written to *pair_bound (if given), and if it exceeds max_pairs (0 = MA_PC_CLUSTER_MAX_PAIRS) the call fails with
 *   MA_ERR_INVALID, the message giving both numbers, launches nothing further and writes no output.  A grid whose float32 faces would
 *   break the bound is refused with MA_ERR_INVALID before any device work.
 *   Non-finite coordinates: such a row has no neighbour and stays; nothing is read or written out of bounds.
 *   1 <= N <= MA_PC_GRID_MAX_POINTS, radius finite and > 0, MA_PC_SMOOTH_MIN_COUNT <= min_count, the grid limits of ma_op_pc_knn_grid,
 *   radius / cell <= 8.  workspace: ma_pc_smooth_workspace_bytes(N, nx, ny, nz) bytes of device memory (0 for arguments outside those
 *   limits): the grid's layout and the 8-byte total; its contents on entry do not matter. */
#define MA_PC_SMOOTH_MIN_COUNT 3
MA_API int    ma_op_pc_smooth(const float *ref, int N, int ref_ld, float radius, const float *origin, float cell, const int32_t *dims,
                              int min_count, uint64_t max_pairs /* 0 = MA_PC_CLUSTER_MAX_PAIRS */, double *moved /* or NULL */,
                              double *normals /* or NULL */, double *eigvals /* or NULL */, int32_t *count /* or NULL */,
                              uint64_t *pair_bound /* host pointer or NULL: the bound that was computed */,
                              void *workspace, size_t workspace_bytes, void *stream);
MA_API size_t ma_pc_smooth_workspace_bytes(int N, int nx, int ny, int nz);

/* ---- Upsampling of a sparse cloud: lattice points in every row's plane, kept where the row is the nearest, for --upsample_radius
 * (csrc/pc_upsample.hpp); PCL's MovingLeastSquares::SAMPLE_LOCAL_PLANE upsampling with a Voronoi restriction.  Has no reference
 * counterpart.  Needs no engine; errors via ma_last_error(NULL); every argument is checked before the first HIP call.  Device arrays
 * (origin, dims, total and pair_bound are HOST pointers), caller-owned workspace.  NOT asynchronous: the call reads the pair bound and
 * then the total back on `stream`, as ma_op_marching_cubes reads its counts.
 *
 * ma_op_pc_upsample: ref (N, ref_ld) fp32, xyz in the first three columns, ref_ld >= 3; normals (N, 3) float64, a unit normal per row,
 *   an INPUT (ma_op_pc_smooth fits one); active (N) bytes or NULL; m in 1..MA_PC_UPSAMPLE_MAX_M; step float64, the lattice spacing (pass
 *   radius / m computed in float64).  Seed row i at position q is skipped when active is given and 0, when q is not finite or when its
 *   normal n is not finite.  All of the following is float64 with no FMA contraction, IEEE division and square root.
 *   Frame: a = the axis with the smallest |n_a|, ties to the lowest axis; u0 = e_a - n_a * n, each component as written; u = u0 /
 *   sqrt((u0x*u0x + u0y*u0y) + u0z*u0z); v = n x u, v_x = n_y*u_z - n_z*u_y and cyclically, NOT renormalised.
 *   Candidates: for a in -m..m (outer loop) and b in -m..m (inner loop), (a, b) != (0, 0), integer a*a + b*b <= m*m: da = (double)a * step,
 *   db = (double)b * step, p_x = (double)q_x + (da*u_x + db*v_x), likewise y and z; c = (float)p, round to nearest.  A non-finite c is dropped.
 *   Keep test, a Voronoi restriction: c is kept iff seed i comes first among ALL rows j in the order (d, index),
 *       d = fl32(fl32(dx * dx + dy * dy) + dz * dz),  dx = fl32(c_x - x_j), dy = fl32(c_y - y_j), dz = fl32(c_z - z_j)
 *   (the key of ma_op_pc_knn, no FMA contraction; a NaN key counts as +inf).  A candidate nearer to another row belongs to that row's patch
 *   or to nobody, duplicated rows give all their candidates to the lower index, and the patches of neighbouring seeds do not overlap.
 *   Output: the kept candidates seed-major, within a seed in (a, b) loop order: out_xyz (T, 3) fp32, out_seed (T) int32 the seed of each,
 *   counts (N) int32 the kept candidates per seed (or NULL), *total = T.  The decision and the bits are a function of the inputs alone --
 *   not of the grid, of the order of the records inside a cell, or of the run; nothing is accumulated -- so a numpy restatement that
 *   evaluates the keys against all rows gives EQUAL outputs.
 *   out_xyz = NULL (then out_seed = NULL too): count only; counts and *total are written, whatever the total.  Otherwise a total above
 *   MA_PC_GRID_MAX_POINTS - N, or above `capacity` (the rows out_xyz and out_seed hold), fails with MA_ERR_INVALID with *total set, and
 *   nothing is written to counts, out_xyz or out_seed.
 *   Consequences of the rule, not defects: the patches are flat; an open border grows outward by up to the radius m * step; at a sharp
 *   edge the fitted plane is diagonal and the patch sticks out; choose the radius at about one to two point spacings.
 *   The grid (origin, cell, dims: as for ma_op_pc_knn_grid, the same faces and cell rule) only decides the time.  A candidate's block of
 *   cells grows ring by ring from its own cell; it ends as not kept at the first row that precedes the seed, and as kept when the block
 *   is the whole grid or fl32(b * b) > the seed's key, strictly, for the distance b = fl32(c - face) to every side of the block that is
 *   not a grid border.  The pair bound is ma_op_pc_cluster's with radius fl32(m * step): computed before the long kernels, written to
 *   *pair_bound (if given), and above max_pairs (0 = MA_PC_CLUSTER_MAX_PAIRS) the call fails with MA_ERR_INVALID and launches nothing
 *   further; a grid whose float32 faces would break the bound is refused before any device work.
 *   Non-finite coordinates or normals: such a row seeds nothing; nothing is read or written out of bounds.
 *   1 <= N <= MA_PC_GRID_MAX_POINTS, N * (2m+1)^2 <= 2^31, step finite and > 0, the grid limits of ma_op_pc_knn_grid, m * step / cell <= 8.
 *   workspace: ma_pc_upsample_workspace_bytes(N, nx, ny, nz) bytes of device memory (0 for arguments outside those limits): the grid's
 *   layout, the 8-byte pair total, N + 1 64-bit offsets and their scan's tiles; its contents on entry do not matter. */
#define MA_PC_UPSAMPLE_MAX_M 64
MA_API int    ma_op_pc_upsample(const float *ref, int N, int ref_ld, const double *normals, const uint8_t *active /* or NULL */,
                                int m, double step, const float *origin, float cell, const int32_t *dims, uint64_t max_pairs,
                                int32_t *counts /* or NULL */, float *out_xyz /* or NULL: count only */, int32_t *out_seed /* or NULL */,
                                uint64_t capacity, uint64_t *total /* host */, uint64_t *pair_bound /* host */,
                                void *workspace, size_t workspace_bytes, void *stream);
MA_API size_t ma_pc_upsample_workspace_bytes(int N, int nx, int ny, int nz);

/* ---- Dominant planes: RANSAC hypothesis scoring and one plane applied, for --plane_threshold (csrc/pc_plane.hpp).  Has no reference
 * counterpart.  Needs no engine; errors via ma_last_error(NULL); every argument is checked before the first HIP call.  Device arrays
 * (`plane` is a HOST array of six floats), caller-owned workspace, asynchronous on `stream`.
 *
 * The inlier rule, shared by both calls.  A plane is six float32, a point a and a normal n of any length.  With no FMA contraction:
 *       len2 = fl32(fl32(nx*nx + ny*ny) + nz*nz),  rhs = fl32(t2 * len2),  t2 = fl32(threshold * threshold) computed once on the host
 *       d = fl32(p - a) per axis,  s = fl32(fl32(fl32(nx*dx) + fl32(ny*dy)) + fl32(nz*dz))
 *       row p is an INLIER iff fl32(s*s) <= rhs
 *   Equality is included.  There is no square root and no division, so a numpy float32 restatement gives the same bits.  A plane is
 *   DEGENERATE iff !(len2 > 0) or rhs is not finite; a degenerate plane has no inliers.  A NaN or infinite row is never an inlier.
 *
 * ma_op_pc_plane_score: ref (N, ref_ld) fp32, xyz in the first three columns, ref_ld = 3 or 6; tri (H, 3) int32, the rows (i, j, k) of
 *   hypothesis h.  Its plane: a = p_i, e1 = fl32(p_j - p_i), e2 = fl32(p_k - p_i), n = e1 x e2 with every product and difference rounded
 *   separately, nx = fl32(fl32(e1y*e2z) - fl32(e1z*e2y)) and cyclically.  A triple with an index outside [0, N) is degenerate, nothing
 *   is read out of bounds, and its plane is six zeros.  planes (H, 6) fp32 or NULL: (a, n) per hypothesis.  counts (H) int32: the number
 *   of inlier rows, -1 for a degenerate hypothesis.  best (1) int32: the h with the greatest count, the lowest index among equals, -1 if
 *   every hypothesis is degenerate.  The counts are sums of integer atomics, which add in any order to the same value: the outputs are a
 *   function of the inputs alone, EQUAL to the restatement's and identical on a second run.
 *   3 <= N <= MA_PC_PLANE_MAX_POINTS, 1 <= H <= MA_PC_PLANE_MAX_HYPOTHESES, threshold finite and > 0.
 *
 * ma_op_pc_plane_apply: one plane against every row.  mask (N) uint8, 1 = inlier, exact under the rule; count (1) int32 = the mask's
 *   sum; moments (10) float64 over the inliers with q = (double)p - (double)a: n, Sqx, Sqy, Sqz, Sqxqx, Sqxqy, Sqxqz, Sqyqy, Sqyqz,
 *   Sqzqz.  Each of the three may be NULL, at least one must be given.  The moments come from a reduction of fixed shape, per-workgroup
 *   partials (a fixed tree over 256 threads of 4 rows each) and one pass over the partials in index order; no floating-point atomics, so
 *   two runs give the same bits.  Equality with another summation order is NOT claimed: |got - want| <= n * 2^-52 * S|term| per moment,
 *   the worst case for any order of n float64 terms.  A degenerate plane gives an all-zero mask, count 0 and zero moments.
 *   3 <= N <= MA_PC_PLANE_MAX_POINTS, threshold finite and > 0; the workspace of ma_pc_plane_workspace_bytes(N, 1) suffices.
 *
 * workspace: ma_pc_plane_workspace_bytes(N, H) bytes of device memory (0 for arguments outside the limits): the apply partials and the
 *   eight floats per hypothesis; its contents on entry do not matter. */
#define MA_PC_PLANE_MAX_POINTS      (1 << 22)
#define MA_PC_PLANE_MAX_HYPOTHESES  (1 << 16)
MA_API int    ma_op_pc_plane_score(const float *ref, int N, int ref_ld, const int32_t *tri, int H, float threshold, float *planes /* or NULL */,
                                   int32_t *counts, int32_t *best, void *workspace, size_t workspace_bytes, void *stream);
MA_API int    ma_op_pc_plane_apply(const float *ref, int N, int ref_ld, const float *plane /* host, 6 */, float threshold, uint8_t *mask /* or NULL */,
                                   int32_t *count /* or NULL */, double *moments /* or NULL */, void *workspace, size_t workspace_bytes, void *stream);
MA_API size_t ma_pc_plane_workspace_bytes(int N, int H);

/* ---- Voxel thinning: one surviving row per occupied voxel of a uniform grid, for --voxel_size (csrc/pc_voxel.hpp).
 * Has no reference counterpart.  Needs no engine; errors via ma_last_error(NULL); every argument is checked before the first HIP call.
 * The only cloud op that takes more than 2^22 rows: the cloud passes through in chunks and never has to be on the device at once.
 *
 * The rule (pcl::UniformSampling's: a surviving ROW, not VoxelGrid's centroid).  ref (n, ref_ld) fp32, xyz in the first three columns,
 *   ref_ld = 3 or 6; origin[3] (HOST) and leaf fp32; the caller passes the per-axis minimum of the fp32 cloud as origin.  Per axis, with
 *   no FMA contraction and the IEEE division:
 *       t = fl32(fl32(x - o) / leaf),  i = floor(t)
 *   A row is SKIPPED, tested in this order: a coordinate is not finite; some t is not >= 0; some i >= 2^21, which also raises the
 *   out-of-range flag.  The voxel's key is ix << 42 | iy << 21 | iz.  The row's offset from the voxel's centre in voxel units is
 *   e = fl32(t - ((float)i + 0.5f)), exact for i < 2^21, and d = fl32(fl32(ex*ex + ey*ey) + ez*ez).  The SURVIVOR of a voxel is its row
 *   with the least (d, row index): a total order, so the survivor is unique and a function of the inputs alone, whatever the capacity,
 *   the chunking and the order in which the device evaluates; a numpy float32 restatement gives the same mask byte for byte.
 *
 * The table: `capacity` slots, a power of two in 2 .. 2 * MA_PC_VOXEL_MAX_VOXELS, open addressing with linear probing over the 64-bit
 *   keys, and per slot the least (bits of d) << 32 | row index; then a state block.  ma_pc_voxel_table_bytes(capacity) bytes of device
 *   memory (0 for a capacity outside the limits).  The table may be at most HALF full: a claim that takes `used` above capacity / 2
 *   raises the overflow flag.  Every probe loop is bounded by `capacity` steps and ends early on that flag, so a full table ends in the
 *   flag, never in a spin.
 *
 * ma_op_pc_voxel_reset: every slot empty, the state zero.  Asynchronous on `stream`.
 * ma_op_pc_voxel_insert: the rows row0 .. row0 + n - 1 of the cloud, 1 <= n <= MA_PC_VOXEL_MAX_CHUNK, row0 >= 0, row0 + n <=
 *   MA_PC_VOXEL_MAX_POINTS; call it once per chunk with the same origin, leaf and table.  Asynchronous on `stream`.
 * ma_op_pc_voxel_mark: keep (N) uint8 on the device: 1 for the survivor of every occupied slot, 0 elsewhere (a row index outside [0, N)
 *   is never written); state_out (4) uint32 on the HOST: used (slots claimed), overflow, out_of_range, voxels (occupied slots counted
 *   by this call).  It waits for `stream`, so state_out is valid on return.  With overflow or out_of_range set the mask is not a
 *   result.  1 <= N <= MA_PC_VOXEL_MAX_POINTS. */
#define MA_PC_VOXEL_MAX_POINTS (1 << 28)   /* a guard value: the row index fits 32 bits, the mask is 256 MB */
#define MA_PC_VOXEL_MAX_CHUNK  (1 << 22)
#define MA_PC_VOXEL_MAX_VOXELS (1 << 22)   /* the largest table: 2^23 slots, 128 MB */
MA_API size_t ma_pc_voxel_table_bytes(uint64_t capacity);
MA_API int    ma_op_pc_voxel_reset(void *table, uint64_t capacity, void *stream);
MA_API int    ma_op_pc_voxel_insert(const float *ref, int n, int ref_ld, int64_t row0, const float *origin /* host, 3 */, float leaf, void *table,
                                    uint64_t capacity, void *stream);
MA_API int    ma_op_pc_voxel_mark(void *table, uint64_t capacity, uint8_t *keep, int64_t N, uint32_t *state_out /* host, 4 */, void *stream);

/* ---- The tightest box: the extents of a cloud under candidate rotations, for --align_iters (csrc/pc_align.hpp).
 * Has no reference counterpart.  Needs no engine; errors via ma_last_error(NULL); every argument is checked before the first HIP call.
 * Device arrays (`centre` is a HOST array of three floats), caller-owned workspace, asynchronous on `stream`.
 *
 * ma_op_pc_align_extents: ref (N, ref_ld) fp32, xyz in the first three columns, ref_ld = 3 or 6; rot (H, 9) fp32, hypothesis h as a
 *   row-major 3x3 r, which need not be orthonormal (the caller's concern).  The rule, with no FMA contraction, for row p and axis a:
 *       q   = fl32(p - centre) per axis
 *       u_a = fl32(fl32(fl32(r_a0*qx) + fl32(r_a1*qy)) + fl32(r_a2*qz)) + 0.0f
 *   The + 0.0f turns -0 into +0, so min and max never depend on the order in which a -0 and a +0 meet.  lo_a = the min of u_a over the
 *   rows, hi_a the max.  A hypothesis is BAD iff one of its nine entries, or one u_a of one row, is not finite.
 *   Each output may be NULL, at least one must be given:
 *   extents (H, 6) fp32 = lo0, lo1, lo2, hi0, hi1, hi2; six NaN for a bad hypothesis.
 *   volumes (H) float64 = ((double)hi0 - (double)lo0) * ((double)hi1 - (double)lo1), then * ((double)hi2 - (double)lo2), each operation
 *   rounded once; +inf for a bad hypothesis (every other volume is finite).
 *   best (1) int32 = the hypothesis of the least volume among those not bad, the lowest index among equals, -1 if every one is bad.
 *   Min and max are order-independent and the workgroups combine through integer atomics on a monotone key of the float's bits (no
 *   floating-point atomics): the outputs are a function of the inputs alone, EQUAL to a numpy float32 restatement's and identical on a
 *   second run.  1 <= N <= MA_PC_ALIGN_MAX_POINTS, 1 <= H <= MA_PC_ALIGN_MAX_HYPOTHESES.
 *
 * workspace: ma_pc_align_workspace_bytes(N, H) bytes of device memory (0 for arguments outside the limits): eight words and one float64
 *   per hypothesis; its contents on entry do not matter. */
#define MA_PC_ALIGN_MAX_POINTS      (1 << 22)
#define MA_PC_ALIGN_MAX_HYPOTHESES  (1 << 16)
MA_API int    ma_op_pc_align_extents(const float *ref, int N, int ref_ld, const float *centre /* host, 3 */, const float *rot, int H,
                                     float *extents /* or NULL */, double *volumes /* or NULL */, int32_t *best /* or NULL */,
                                     void *workspace, size_t workspace_bytes, void *stream);
MA_API size_t ma_pc_align_workspace_bytes(int N, int H);

/* ---- Rigid registration of two clouds: one ICP iteration over the cell grid, for --register_dist (csrc/pc_register.hpp; DESIGN.md
 * section 21); PCL's registration module and Open3D's registration_icp do the same job.  Has no reference counterpart.  Needs no engine;
 * errors via ma_last_error(NULL); every argument is checked before the first HIP call.  Device arrays (origin, dims, pose, centre and
 * pair_bound are HOST pointers), caller-owned workspace.
 *
 * ma_op_pc_register_build: target (N, target_ld) and source (M, source_ld) fp32, xyz in the first three columns, each ld = 3 or 6.  Bins
 *   the target over the grid (origin, cell, dims: as for ma_op_pc_knn_grid, the same faces and cell rule), and bins the source ONCE, in
 *   its own frame, so that the step's search threads take source rows in cell order; a rigid motion keeps neighbours neighbours, so one
 *   build serves every pose.  Asynchronous on `stream`.  The grid only decides the time.
 *
 * ma_op_pc_register_step: the same clouds and grid, over the workspace ma_op_pc_register_build filled.  NOT asynchronous: it reads the
 *   pair bound back on `stream` before it launches the search, as ma_op_pc_cluster does.  pose: 12 floats, R row-major, then t; centre: 3
 *   floats; r2 = fl32(max_dist * max_dist), computed once on the host.  With no FMA contraction anywhere, for source row (x, y, z):
 *       p'_a = fl32(fl32(fl32(fl32(R_a0 * x) + fl32(R_a1 * y)) + fl32(R_a2 * z)) + t_a)
 *       d    = fl32(fl32(dx * dx + dy * dy) + dz * dz),  dx = fl32(p'_x - q_x), ...   against target row q: the key of ma_op_pc_knn
 *   The PAIR of the source row is the target row least in (d, index) among the rows with d <= r2: equality is included, a NaN key pairs
 *   nothing, of duplicate target rows the lower index wins.  nn_idx (M) int32 = that row, -1 if there is none; nn_d2 (M) fp32 = its d,
 *   +inf if there is none; both in the source's ORIGINAL row order, a function of the clouds, the pose and max_dist alone -- not of the
 *   grid, the workspace's earlier contents or the run -- so a numpy float32 restatement over all rows gives EQUAL arrays.
 *   The walk is ma_op_pc_knn_grid's ring walk from the cell of p' in the target's grid; it ends at the whole grid, when the pair's key
 *   is STRICTLY below fl32(b * b) for every side of the block that is not a grid border (that call's rule (b) with k = 1), or when
 *   every such side has fl32(b * b) > r2 (ma_op_pc_cluster's rule).
 *   Guard, per call: the transformed source is counted into the target's cells, and sum_c m_c * (target rows in the block of R rings
 *   around c), R = floor(max_dist / cell) + 2, a bound on the keys the search evaluates, is written to *pair_bound (if given); above
 *   max_pairs (0 = MA_PC_CLUSTER_MAX_PAIRS) the call fails with MA_ERR_INVALID, the message giving both numbers, launches nothing
 *   further and writes no output.  A grid whose float32 faces would break the bound is refused before any device work.
 *   sums (MA_PC_REGISTER_SUMS) float64 on the device, over the pairs, c = centre, every term formed in float64 from the float32 p' and q:
 *       [0] pairs used   [1] sum (double)d   [30] pairs skipped   [31] 0
 *     target_normals = NULL, the point metric:  [2..4] sum (p' - c)   [5..7] sum (q - c)   [8..16] sum (p' - c)(q - c)^T, row-major
 *     target_normals (row j at target_normals + j * normals_ld, fp32, normals_ld >= 3; pass target + 3 with ld 6 for a cloud that carries
 *     its normals), the plane metric:  n = normal / sqrt((nx*nx + ny*ny) + nz*nz), e = p' - q, r = (n_x*e_x + n_y*e_y) + n_z*e_z,
 *       u = p' - c, a = u x n (a_x = u_y*n_z - u_z*n_y and cyclically), J = (a, n):
 *       [2] sum r*r   [3..8] sum J_k * r   [9..29] sum J_k * J_l for k <= l, row-major.  A pair whose normal is zero or not finite is
 *       SKIPPED: it counts in [30] and in nothing else.
 *   The sums are formed in a FIXED order and with no floating-point atomics: thread t of workgroup g adds source rows g * 256 * RPT + j *
 *   256 + t for j = 0 .. RPT - 1 (RPT = MA_PC_REGISTER_ROWS_PER_THREAD), then a tree over the MA_PC_REGISTER_THREADS lanes (lane t += lane
 *   t + w, w = 128, 64, .., 1), then one workgroup adds the workgroups' partials in index order.  The same inputs give the same 32
 *   doubles for every grid, every workspace content and every run; against another summation order they agree within depth * 2^-52 *
 *   sum |term| per slot, depth = RPT + 8 + ceil(M / (256 * RPT)).
 *   Each of nn_idx, nn_d2, pair_bound and sums may be NULL; at least one of nn_idx, nn_d2 and sums must be given.
 *   Non-finite coordinates: a source row with a non-finite p' pairs nothing and adds no term; nothing is read or written out of bounds.
 *   1 <= N, M <= MA_PC_GRID_MAX_POINTS, pose and centre finite, max_dist finite and > 0 with a finite square, the grid limits of
 *   ma_op_pc_knn_grid, max_dist / cell <= 8.
 *
 * workspace: ma_pc_register_workspace_bytes(N, M, nx, ny, nz) bytes of device memory (0 for arguments outside the limits): the grid
 *   layouts of both clouds, the 8-byte total, a count per cell, M indices and the partial sums; its contents before the build do not matter. */
#define MA_PC_REGISTER_SUMS            32
#define MA_PC_REGISTER_THREADS         256
#define MA_PC_REGISTER_ROWS_PER_THREAD 16
MA_API int    ma_op_pc_register_build(const float *target, int N, int target_ld, const float *source, int M, int source_ld,
                                      const float *origin, float cell, const int32_t *dims, void *workspace, size_t workspace_bytes,
                                      void *stream);
MA_API int    ma_op_pc_register_step(const float *target, int N, int target_ld, const float *source, int M, int source_ld,
                                     const float *origin, float cell, const int32_t *dims, const float *pose /* host, 12 */,
                                     const float *centre /* host, 3 */, float max_dist, const float *target_normals /* or NULL */,
                                     int normals_ld, uint64_t max_pairs /* 0 = MA_PC_CLUSTER_MAX_PAIRS */, int32_t *nn_idx /* or NULL */,
                                     float *nn_d2 /* or NULL */, uint64_t *pair_bound /* host pointer or NULL */, double *sums /* or NULL */,
                                     void *workspace, size_t workspace_bytes, void *stream);
MA_API size_t ma_pc_register_workspace_bytes(int N, int M, int nx, int ny, int nz);

/* ---- Coarse registration from unknown poses, for --coarse_radius (csrc/pc_coarse.hpp): PCL's FPFHEstimation and
 * SampleConsensusPrerejective, Open3D's compute_fpfh_feature and registration_ransac_based_on_feature_matching do the same job.  Has no
 * reference counterpart.  Needs no engine; errors via ma_last_error(NULL); every argument is checked before the first HIP call.  Device
 * arrays (origin, dims, pair_bound and most_used are HOST pointers).  Each op is a pure function of its inputs, and its integer outputs
 * equal a numpy float32 restatement byte for byte: no FMA contraction, IEEE sqrt and /, no floating-point atomics.
 *
 * ma_op_pc_spfh: ref (N, ref_ld) fp32, xyz in the first three columns, ref_ld = 3 or 6; normals: row i at normals + i * normals_ld, fp32,
 *   normals_ld >= 3 (pass ref + 3 with ld 6 for a cloud that carries its normals); the grid as for ma_op_pc_cluster, radius / cell <= 8.
 *   NOT asynchronous: it reads the pair bound back before the search, as ma_op_pc_cluster does (same guard, same max_pairs, same
 *   refusal), and the largest number of used pairs after it.  r2 = fl32(radius * radius).  For row p with position x_p and normal n_p
 *   the NEIGHBOURS are the rows q with 0 < d <= r2, d = fl32(fl32(dx*dx + dy*dy) + dz*dz), dx = fl32(x_p.x - x_q.x), ...: the key of
 *   ma_op_pc_knn; equality with r2 is included, a NaN key is no neighbour, d = 0 (the row itself, a duplicate) has no direction.  Per pair
 *       dot(u, v) = fl32(fl32(fl32(u_x*v_x) + fl32(u_y*v_y)) + fl32(u_z*v_z)),  len = fl32(sqrt(d)),  D = (dx, dy, dz)
 *       a = fl32(|dot(n_p, D)| / len)   b = fl32(|dot(n_q, D)| / len)   c = |dot(n_p, n_q)|
 *       bin(v) = 10 if fl32(v * 11) >= 10, else (int)fl32(v * 11)
 *   hist (N, MA_PC_SPFH_COLS) uint32, row p: [0..10] the counts of bin(a), [11..21] of bin(b), [22..32] of bin(c), [33] the pairs used.
 *   A pair is skipped and counted nowhere when either normal has a non-finite component or is (0, 0, 0), or when a, b or c is NaN.  The
 *   features carry no sign: a scan's estimated normals are unoriented.  *most_used (if given) = the largest [33] if it is above
 *   MA_PC_SPFH_MAX_USED, else 0; above it the call fails with MA_ERR_INVALID (thin the cloud or use a smaller radius) and hist is not
 *   to be used: under that limit the sums of the gather cannot overflow.
 * ma_op_pc_spfh_gather: the same cloud, radius and grid; hist as above; query (Q) int32, 1 <= Q <= MA_PC_SPFH_MAX_QUERIES, repeats allowed.
 *   desc (Q, MA_PC_SPFH_DESC) uint32, desc[j] = hist[p] + sum over the neighbours q of p = query[j] (0 < d <= r2, nothing else) of hist[q],
 *   columns 0..32, modulo 2^32; a query outside [0, N) gives a zero row.  FPFH's second pass without the 1/d weights: integer sums need
 *   no order.  Builds the grid itself and applies the same guard; NOT asynchronous.
 * workspace of both: ma_pc_spfh_workspace_bytes(N, nx, ny, nz) bytes of device memory (0 outside the limits); its contents do not matter.
 * ma_op_pc_desc_match: A (Ka, 33), B (Kb, 33) uint32, 1 <= Ka, Kb <= MA_PC_COARSE_MAX_KEYPOINTS.  Every block of 11 is normalised by its
 *   integer sum S: x = fl32(fl32(h) / fl32(S)), a zero block stays zero; dist = the SEQUENTIAL fp32 sum over bins 0..32, from 0, of
 *   fl32(fl32(x - y) * fl32(x - y)).  idx (Ka) int32 = the row of B least in (dist, index), dist (Ka, or NULL) fp32 = that distance.  Asynchronous.
 * ma_op_pc_pose_score: poses (H, 12) fp32, R row-major then t, 1 <= H <= MA_PC_COARSE_MAX_HYPOTHESES; P, Q (C, 3) fp32 contiguous, 1 <= C <=
 *   MA_PC_COARSE_MAX_KEYPOINTS; t2 = fl32(max_dist * max_dist).  counts (H) int32 = the number of pairs i whose key between p' (the
 *   transform of ma_op_pc_register_step applied to P_i, rounding for rounding) and Q_i is <= t2; a NaN key agrees with nothing.  best (1,
 *   or NULL) int32 = the h of the highest count, the lowest index among equals (ma_op_pc_plane_score's rule).  Asynchronous. */
#define MA_PC_SPFH_BINS             11
#define MA_PC_SPFH_DESC             33
#define MA_PC_SPFH_COLS             34
#define MA_PC_SPFH_MAX_USED         65535
#define MA_PC_SPFH_MAX_QUERIES      (1 << 20)
#define MA_PC_COARSE_MAX_KEYPOINTS  4096
#define MA_PC_COARSE_MAX_HYPOTHESES (1 << 16)
MA_API int    ma_op_pc_spfh(const float *ref, int N, int ref_ld, const float *normals, int normals_ld, float radius, const float *origin,
                            float cell, const int32_t *dims, uint64_t max_pairs /* 0 = MA_PC_CLUSTER_MAX_PAIRS */, uint32_t *hist,
                            uint64_t *pair_bound /* host pointer or NULL */, uint32_t *most_used /* host pointer or NULL */, void *workspace,
                            size_t workspace_bytes, void *stream);
MA_API int    ma_op_pc_spfh_gather(const float *ref, int N, int ref_ld, float radius, const float *origin, float cell, const int32_t *dims,
                                   uint64_t max_pairs /* 0 = MA_PC_CLUSTER_MAX_PAIRS */, const uint32_t *hist, const int32_t *query, int Q,
                                   uint32_t *desc, uint64_t *pair_bound /* host pointer or NULL */, void *workspace, size_t workspace_bytes,
                                   void *stream);
MA_API size_t ma_pc_spfh_workspace_bytes(int N, int nx, int ny, int nz);
MA_API int    ma_op_pc_desc_match(const uint32_t *A, int Ka, const uint32_t *B, int Kb, int32_t *idx, float *dist /* or NULL */, void *stream);
MA_API int    ma_op_pc_pose_score(const float *poses, int H, const float *P, const float *Q, int C, float max_dist, int32_t *counts,
                                  int32_t *best /* or NULL */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MESHANYTHING_AMD_H */
