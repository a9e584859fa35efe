// Shared state of the host side: error types, the precision-dispatch macros, the resolved weight records (DenseW, DecW), and the engine record (struct ma_engine) with its exchange table and captured steps. (No includes of its own: compiled only inside engine.hip, in its include order.)
#pragma once

namespace {

thread_local std::string g_create_error;

struct MaError : std::exception {
    int code; std::string msg;
    MaError(int c, std::string m) : code(c), msg(std::move(m)) {}
    const char* what() const noexcept override { return msg.c_str(); }
};

// an in-launch exchange of a fused decode launch gave up (its blocks were not all resident): generate() answers by switching this
// engine to the five-launch chain (no co-residency needed, same bits) and running the generation again
struct ChainTimeout : MaError {
    ChainTimeout(std::string m) : MaError(MA_ERR_HIP, std::move(m)) {}
};

#define HIP_CHECK(expr)                                                                                      \
    do {                                                                                                     \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess)                                                                                \
            throw MaError(MA_ERR_HIP, std::string(#expr) + " failed: " + hipGetErrorString(_e) + " (" + __FILE__ + ":" + std::to_string(__LINE__) + ")"); \
    } while (0)

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// The engine's 16-bit format (ma_config.dtype: MA_DTYPE_BF16 | MA_DTYPE_F16) as a compile-time type of the kernels (common.hpp H16):
// H16_CALL evaluates an expression, H16_DO runs statements, with HT = f16_t or bf16_t.
#define H16_CALL(hdt, HT, ...) ((hdt) == MA_DTYPE_F16 ? [&] { using HT = f16_t; return __VA_ARGS__; }() : [&] { using HT = bf16_t; return __VA_ARGS__; }())
#define H16_DO(hdt, HT, ...) do { if ((hdt) == MA_DTYPE_F16) { using HT = f16_t; __VA_ARGS__; } else { using HT = bf16_t; __VA_ARGS__; } } while (0)
// The three-way precision dispatch of a policy: T = float under the exact policy, else the 16-bit type `hdt` names.
// PREC_CALL evaluates an expression, PREC_DO runs statements.
#define PREC_CALL(is16, hdt, T, ...) ((is16) ? H16_CALL(hdt, T, __VA_ARGS__) : [&] { using T = float; return __VA_ARGS__; }())
#define PREC_DO(is16, hdt, T, ...) do { if (is16) H16_DO(hdt, T, __VA_ARGS__); else { using T = float; __VA_ARGS__; } } while (0)
// 16-bit format of the kernel-level entry points that carry no dtype argument (ma_op_set_half_dtype)
thread_local int g_op_hdt = MA_DTYPE_BF16;

// every kernel launch of the host side reports through here
inline void launched(hipError_t r, const char* what) {
    if (r != hipSuccess) throw MaError(MA_ERR_HIP, std::string(what) + " launch failed: " + hipGetErrorString(r));
}

// ... and of a kernel-level entry point (ma_op_*): a shape the kernel refuses is the caller's error
inline void op_launched(hipError_t r, const char* op) {
    if (r != hipSuccess) throw MaError(r == hipErrorInvalidValue ? MA_ERR_INVALID : MA_ERR_HIP, std::string(op) + ": " + hipGetErrorString(r));
}

// roctx ranges around the phases of the hot path (tracing): resolved lazily from libroctx64.so, active only when
// MA_ROCTX=1 is set in the environment (rocprofv3 --marker-trace then shows encode / prefill / decode / detokenize as ranges)
struct RoctxRange {
    typedef int (*push_fn)(const char*);
    typedef int (*pop_fn)();
    static push_fn& push() { static push_fn f = nullptr; return f; }
    static pop_fn& pop() { static pop_fn f = nullptr; return f; }
    static bool enabled() {
        static int state = -1;
        if (state < 0) {
            state = 0;
            const char* v = getenv("MA_ROCTX");
            if (v && v[0] == '1') {
                void* h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
                if (!h) h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
                if (h) {
                    push() = reinterpret_cast<push_fn>(dlsym(h, "roctxRangePushA"));
                    pop() = reinterpret_cast<pop_fn>(dlsym(h, "roctxRangePop"));
                    state = push() && pop() ? 1 : 0;
                }
            }
        }
        return state == 1;
    }
    bool on;
    explicit RoctxRange(const char* name) : on(enabled()) { if (on) push()(name); }
    ~RoctxRange() { if (on) pop()(); }
};

}  // namespace

// ---- the dense phases' weights, resolved from the layout once (build_engine: a name the layout does not have fails engine creation);
// the hot path builds no names and looks nothing up
struct Lin { const void* w; const float* b; int rows, cols, dtype; const char* name; };      // nn.Linear: weight (rows, cols) of `dtype`, fp32 bias or null; name = the weight's arena entry (error messages)
struct LnW { const float *g, *b; float eps; };                                                // nn.LayerNorm
struct ResBlockW { LnW ln1, ln2; Lin qkv, proj, fc, fc_proj; };                               // ResidualAttentionBlock (transformer_blocks.py:109-112)
struct CrossBlockW { LnW ln1, ln2, ln3; Lin q, kv, proj, fc, fc_proj; };                      // ResidualCrossAttentionBlock (transformer_blocks.py:223-226)
struct PostLnLayerW { Lin qkv, o, fc1, fc2; LnW ln1, ln2; };                                  // a post-LN layer, q|k|v fused: OPTDecoderLayer, BertLayer
struct DenseW {
    const float* query; Lin input_proj; CrossBlockW cross; std::vector<ResBlockW> enc; LnW ln_post;          // point encoder
    Lin pre_kl, post_kl; std::vector<ResBlockW> shape; Lin cond_head, cond;                                   // shape latents, prefix
    const float *cond_embed, *embed_pos; std::vector<PostLnLayerW> opt;                                       // prefill
    Lin tok_cond_head, tok_cond, project_down, to_coor; LnW point_ln, face_ln; const float *point_pe, *pos_emb, *codebooks; std::vector<PostLnLayerW> bert;      // detokenizer
};
// ... and what the decode step reads besides its layers (e->dl; LayerNorms: dw.opt[l].ln1 / ln2): resolved by the same function
struct DecW {
    const void *lm_head, *input_w; const float* input_b;                       // lm_head and input_layer matrices in the policy dtype
    const float *codebooks, *extra, *tokpos, *cond, *postab; int pos_rows;      // quantize_codebooks, extra_embeds, token_embed_positions, cond_embed, embed_positions and its rows
};

// A buffer through which blocks of one launch hand data to each other (granules: common.hpp), with the bytes that every generation starts from zero
struct Exchange { void* p; size_t reset_bytes; };
// one captured decode step, by (first row, rows, step implementation): the grids depend on the rows, the pointers on the first row
struct StepGraph { hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; };
typedef std::tuple<int, int, int> StepGraphKey;

struct ma_engine {
    ma_config cfg{};
    int device = 0;
    Layout L;
    PackState ps;
    bool weights_ready = false;
    std::string err;
    char* arena = nullptr;
    void* stage = nullptr; size_t stage_bytes = 0;      // upload staging of ma_engine_load_weights (freed by finalize)
    std::vector<void*> allocs;                          // every dmalloc below (freed by ma_engine_destroy)

    // ---- sizes and policy derived from the configuration (build_engine)
    int T = 0, V = 0, maxnew = 0, maxseq = 0, nf = 0, S = 0;
    bool bf16 = true;                // a 16-bit policy (bf16 OR fp16; the name is historical): 16-bit weights + KV, GEMM / attention inputs rounded
    int hdt = MA_DTYPE_BF16;         // ... and which one: MA_DTYPE_BF16 | MA_DTYPE_F16 (the type tag of the 16-bit kernels, H16_CALL)
    size_t kv_elem = 2;
    size_t kv_plane = 0;             // bytes of one K (or V) plane of one layer
    size_t kv_row_bytes = 0;         // bytes of one batch row's planes (2 * layers * kv_plane)
    int dense_rows = 1, prefill_rows = 1;
    int n_cus = 0;
    int n_parts = 0;                 // blocks of the lm_head GEMV = partial maxima the pick launch reads
    bool persist_shape = false;      // the persistent step's shape / device eligibility (fixed at creation; MA_EXPERIMENTAL)
    bool rf_ok = false;              // the rows-looped second launch (130 KB of LDS) can be resident on every CU of this device (MA_EXPERIMENTAL)
    bool rows_ok = false;            // the two 8-row launches (256 blocks of 512 threads each) can be resident all at once on this device
    bool chain_resident = false;     // the fused launches' 256 blocks fit on the device at once, with margin (their in-launch exchange needs that)
    long resident_blocks = 0;        // 256-thread blocks of the fused launches the device holds at once (CUs x (occupancy - 1))

    // ---- the integer switches of ma_engine_set_option (engine_options.hpp holds names, ranges and side effects); the initialisers are the defaults
    struct Options {
        int gemm_impl = 0;               // 0 MFMA, 1 VALU reference kernel
        int prefill_stepwise = 0;        // 1: run the prefix through the decode-step chain row by row (debug cross-check)
        int profile_batch = 1;           // batch size ma_profile_decode times (<= max_batch)
        int decode_groups = 1;           // row groups of a batched step: 1 = one group (default: measured faster), G = that many (decode_group_count caps it)
        int mfma_min_batch = 4;          // bf16 policy: batches of at least this many rows take the MFMA skinny-GEMM decode path
        int attn_pair = 1;               // final-form attention below 12 rows: two blocks per (row, head)
        int mfma_fc2_ksplit = 0;         // blocks along K of the batched fc2 GEMM: 0 = gemm_dec_ksplit (4) | 1 | 2 | 4
        int mfma_ln_waves = 0;           // waves per block of the LayerNorm-folded skinny GEMM: 0 = by batch (8 for 5..8 rows, else 4) | 4 | 8
        int mfma_fold_ln = 1;            // MFMA decode path, small batches: LayerNorm prologues inside the consuming GEMMs (up to two launches fewer per layer)
        int mfma_fold_fc1_max = 8, mfma_fold_qkv_max = 8;       // largest batch for which LN1 (in front of fc1) / LN2 (in front of q/k/v) is folded
        int attn_final_min_batch = 8;    // MFMA decode path: from this many rows on, one attention block per (row, head) writes the final output (no merge launch)
        int attn_final_waves = 0;        // waves per block of that form: 0 = 4 from 12 rows on, 8 below; or 4 | 8 | 16
        int attn_rowwave = 1;            // MFMA decode path below that: one wave per (row, head, chunk) (1) or one block (0)
        int fuse_qkv_attn = 1;           // launch chain, any policy, hidden 1024: q/k/v projection and decode attention in ONE launch (qkv_attn.hpp)
        int qkv_xcd_local = 1;           // ... the 16 blocks of a head on one XCD (qkv_attn.hpp qkv_block_role)
        int fuse_oproj_fc1 = 1;          // ... and out_proj (+ partial merge) + LayerNorm + fc1 in ONE launch (oproj_fc1.hpp)
        int fuse_fc2 = 1;                // fc2 inside the out_proj + fc1 launch (second in-launch all-gather, 4096 values)
        int oproj_fc1_sweep_waves = 4;   // fused out_proj + fc1 launch: waves per block polling the y1 granules (each its own quarter)
        int fuse_rows_attn = 1;          // matrix-core decode path at 8 rows: LayerNorm + q/k/v + attention + out_proj in ONE launch (rows_attn.hpp)
        int fuse_rows_mlp = 1;           // ... and LayerNorm 1 + fc1 + fc2 in ONE launch (rows_mlp.hpp; its relu(fc1) exchange uses d_ffn_gran)
        int rows_attn_early = 6;         // rows_attn.hpp: when the first cache rounds are requested (A/B, see the kernel): 5 = the q/k/v sweep by scalar loads (waves 0 .. 3), two rounds by the waves 4 .. 7 meanwhile; 6 = 5 + rounds wholly below the newest position run without masks; 3 = one round behind the q/k/v MFMAs, sweep by vector loads
        int rows_mlp_prefetch = 0;       // rows_mlp.hpp step F (measured, not kept: 0 = off): the next layer's first operands pulled into L2 by the blocks that idle during step E -- 1 | 2 rounds, 8 = weights only, 9 = half a round
        int rows_mlp_ln2 = 1;            // rows_mlp.hpp step E: LayerNorm 2 finished in the MLP launch (the next q/k/v starts from 16-bit rows)
        int embed_table = 1;             // GEMV chain: the pick writes the next step's layer-0 input from the load-time table (misc.hpp pick_kernel<true>); 0: an embedding launch per step
        int gemm_xcd_swizzle = 1;        // dense GEMM: hand the tiles out XCD-aware (gemm_tile.hpp)
        int gemm_variant = 6, gemm256 = 2, mfma_chunks = 8;             // GemmTune (gemm_tile.hpp): K-loop variant | 256 x 256 tiles | chunks in flight of the skinny GEMM at 33 .. 64 rows
        int gemv_rpw = 4, gemv_small_rows = 1, gemv_k8_ksplit = 1;      // GemvTune (gemv.hpp): block shapes of the GEMV chain
        GemmTune gemm_tune() const { return GemmTune{gemm_variant, gemm256, mfma_chunks}; }
        GemvTune gemv_tune() const { return GemvTune{gemv_rpw, gemv_small_rows, gemv_k8_ksplit}; }
        int attn_impl = 2;               // bf16 dense attention: 2 = swapped-operand 32x32x16 kernel on packed V^T (attn2.hpp), 1 = attention_mfma_kernel (attn.hpp)
        int qkv_to_cache = 1;            // prefill (16-bit policies): the q|k|v GEMM writes K / V into the cache planes itself where it can (gemm256.hpp KV form); 0: always by kv_fill_rows_kernel (A/B)
        int gemm_splitk = 2;             // prefill fc2 (1) and out_proj (2, default) of small batches as 4 | 2 partial sums along K, added up by the LayerNorm that follows (0: never; A/B)
        int prefill_tail = 2;            // 16-bit prefill of >= 8 samples: the M % 256 rows behind the 256-row tiles run as a chain of their own on a second stream (prefill());
                                         // 2 (default): that stream has the lowest priority -- HIP keeps a pool of hardware queues per priority, so it can never land on the
                                         // hardware queue of the main stream (or of the application's default-priority streams), where it would run IN LINE with them; 1: default priority
        // MA_EXPERIMENTAL libraries only (measured, not kept)
        int fuse_ln = 0;                 // prefill: the two LayerNorms of a layer finished inside the out_proj / fc2 GEMMs where those run on whole 256 x 256 tiles (gemm256.hpp LNF form; needs the grid resident like every in-launch exchange: chain_resident)
        int fuse_layer = 0;              // second half of layer l + first half of layer l + 1 in one launch (layer_fused.hpp)
        int rows_fused = 0;              // 2 .. 8 rows: the two-launch layer with the rows looped inside the 256 blocks (rows_fused.hpp).  Opt-in: bit-identical
                                         // to batch-1 runs, 51 launches per step, but 1.4-1.9x SLOWER than the matrix-core chain (profiles/r03_rows_fused_*)
        int rows_fused_min = 4;          // smallest batch that takes it (below: the batch-1 fused launches with the rows in the grid)
        int decode_impl = 0;             // 0: chain of launches; 1: one persistent launch per step (when eligible; persist.hpp: batch 1, bf16, greedy, 350M-shaped layers on a 256-CU device)
    } opt;

    // ---- decode-step buffers: one slice per batch row
    char* kv = nullptr;              // [max_batch][layers][2][heads][maxseq][64] of KT
    float *d_e = nullptr, *d_q = nullptr, *d_ypre1 = nullptr, *d_ypre2 = nullptr, *d_h0 = nullptr, *d_h1 = nullptr,
          *d_ffn = nullptr, *d_logits = nullptr, *d_part = nullptr, *d_pval = nullptr;
    int* d_pidx = nullptr;
    DecState* d_st = nullptr;        // one record per batch row
    DecState* h_state = nullptr;     // pinned (max_batch)
    long long* h_tokens = nullptr;   // pinned (max_batch * maxnew)
    std::vector<DecLayerPtrs> dl;
    bf16_t *d_xb = nullptr, *d_ffb = nullptr;      // bf16 activations of the batched path: [max_batch][hidden], [max_batch][ffn]
    float *d_ks_o = nullptr, *d_ks_f = nullptr;    // split-K partials of out_proj / fc2: [4][max_batch][hidden]
    unsigned* d_pf_sink = nullptr;                 // (rows_mlp_prefetch)
    // embedding table (option embed_table; engine_decode.hpp ensure_embtab): read by the pick, and by the experimental persistent step
    float* d_embtab = nullptr;       // [codebook_size][hidden] fp32: input_layer(codebook row) + bias, built by the chain's own GEMV
    bool embtab_ready = false;       // ... for the weights in the arena and this engine's gemv_small_rows
    // the persistent step's (MA_EXPERIMENTAL)
    DecLayerPtrs* d_layers = nullptr;
    u64* d_gran = nullptr; unsigned* d_serial = nullptr; unsigned* d_err = nullptr; unsigned* h_err = nullptr;
    u64* d_ptrace = nullptr;

    // ---- exchange buffers of the launches that hand data over inside a launch (granules: common.hpp): each allocated by xalloc, which
    // zeroes it and lists what init_state (engine_generate.hpp) zeroes again for every generation
    std::vector<Exchange> exchanges;
    u64* d_qkv_gran = nullptr;     // fused q/k/v + attention: [max_batch][3 hidden]
    u64* d_y1_gran = nullptr;        // fused out_proj + fc1: [max_batch][hidden]
    u64* d_y2_gran = nullptr;        // [max_batch][hidden] (y2 handed to the next layer inside a launch)
    u64* d_ffn_gran = nullptr;       // [max_batch][ffn] (fc2 in the out_proj + fc1 launch; relu(fc1) of rows_mlp.hpp)
    unsigned long long* d_attn_pair_gran = nullptr;      // [max_batch][heads][ATTN_PAIR_GRANULES]: hand-over of the two-block final-form attention
    u64 *d_ra_qkv_gran = nullptr, *d_ra_out_gran = nullptr;      // rows_attn.hpp: [max_batch][RA_QKV_GRANULES], [max_batch][RA_OUT_GRANULES]
    u64* d_rm_y2_gran = nullptr;     // rows_mlp.hpp step E: [max_batch][RM_Y2_GRANULES]
    u64* d_part_gran = nullptr;      // rows_fused.hpp (MA_EXPERIMENTAL): [max_batch][heads][16][66], its in-launch split-KV partial exchange
    u64* d_ln_gran = nullptr; size_t ln_gran_tiles = 0; unsigned ln_epoch = 0;      // gemm256.hpp LNF form (fuse_ln); its epochs run on across generations: never reset
    unsigned* d_chain_err = nullptr; unsigned* h_chain_err = nullptr;               // error word (reset per generation) + counters (never) of all of them (build_engine)

    // ---- dense-phase workspace: dense_rows samples stacked along the rows.  w_* / p_*: fp32 streams; a_*: activation tensors
    // (dense_ops.hpp: 2-byte elements in a 16-bit phase, 4 in an exact one; every phase entry says which in its Dense context, engine_dense.hpp).
    // The point encoder (ma_encode: encode_latents + process_point_feature, and the detokenizer's projection of the latents) runs in fp32
    // under a 16-bit policy when cfg.enc_exact is set -- the north star's 1e-5 on encoder activations in the benchmarked mode; prefill and
    // the detokenizer's BERT stack follow the policy dtype.
    bool enc_exact = false;          // encoder weights are fp32 arena entries and the encoder's activations fp32 (always true under the fp32 policy)
    DenseW dw;                       // the dense phases' weights
    DecW decw;                       // the decode step's
    float *w_data = nullptr, *w_lat = nullptr, *w_lat2 = nullptr, *w_pf = nullptr, *w_x = nullptr, *w_y = nullptr, *w_fe = nullptr, *w_logit = nullptr;
    float *p_h = nullptr, *p_y = nullptr;
    long p_y_part_stride = 0;        // p_y holds up to 4 partial sums of a GEMM split along K (gemm256.hpp GemmSplitK), this many floats apart, for the small prefills that use it
    void *a_feat = nullptr, *a_dataln = nullptr, *a_kv = nullptr, *a_q = nullptr, *a_ln = nullptr, *a_qkv = nullptr, *a_att = nullptr, *a_mlp = nullptr,
         *a_cat = nullptr, *a_mean = nullptr, *a_fein = nullptr, *a_x = nullptr, *a_ph = nullptr, *a_pqkv = nullptr, *a_patt = nullptr, *a_pffn = nullptr;
    bf16_t* a_vt = nullptr; size_t vt_elems = 0;      // V^T workspace of attn2.hpp
    void* a_patt_tail = nullptr; bf16_t* a_vt_tail = nullptr; size_t vt_tail_elems = 0;      // the prefill tail chain's attention output (64 rows) and V^T workspace (one sample)
    unsigned char* w_mask = nullptr;
    float *w_latents = nullptr, *w_prefix = nullptr;   // ma_forward intermediates (max_batch rows)
    long long *w_tokens = nullptr, *w_ids = nullptr;

    // ---- streams, events, graphs
    std::map<StepGraphKey, StepGraph> graphs;
    hipStream_t cap_stream = nullptr;   // capture happens on a private stream (the caller's may be the legacy null stream)
    // row groups of a batched step (decode_groups): group g steps its rows on grp_stream[g], forked from / joined to the caller's stream
    std::vector<hipStream_t> grp_stream; std::vector<hipEvent_t> grp_done; hipEvent_t grp_fork = nullptr;
    hipStream_t tail_stream_low = nullptr;      // (prefill_tail = 2)
    hipStream_t tail_stream = nullptr; hipEvent_t tail_fork = nullptr, tail_join = nullptr; std::vector<hipEvent_t> tail_kv;      // the prefill tail chain's stream; per layer: "the main rows' K / V are in the planes"

    // ---- health counters (ma_engine_get_option)
    int xchg_last_code = 0;          // the error word of the last generation that fell back (bits of the sweeps that gave up)
    int chain_fallbacks = 0;         // generations that were re-run on the five-launch chain after an exchange timed out
    int gens_since_fallback = 0;     // clean generations on the five-launch chain since then: after CHAIN_REARM_AFTER of them the fused launches get another try

    template <typename Tp> Tp* dmalloc(size_t n) {
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(Tp)));
        allocs.push_back(p);
        return reinterpret_cast<Tp*>(p);
    }
    // an exchange buffer of n elements, zeroed; its first n_reset elements (default: all, 0: none) are zeroed again for every generation
    template <typename Tp> Tp* xalloc(size_t n, size_t n_reset = ~size_t(0)) {
        Tp* p = dmalloc<Tp>(n);
        HIP_CHECK(hipMemset(p, 0, n * sizeof(Tp)));
        if (n_reset) exchanges.push_back(Exchange{p, std::min(n, n_reset) * sizeof(Tp)});
        return p;
    }
    const Entry& entry(const std::string& name) const {
        auto it = L.entry_by_name.find(name);
        if (it == L.entry_by_name.end()) throw MaError(MA_ERR_INVALID, "internal: no arena entry " + name);
        return L.entries[it->second];
    }
    const void* P(const std::string& name) const { return arena + entry(name).offset; }
    const float* PF(const std::string& name) const { return reinterpret_cast<const float*>(P(name)); }
    char* kplane(int row, int layer) const { return kv + (size_t)row * kv_row_bytes + (size_t)(2 * layer) * kv_plane; }
    char* vplane(int row, int layer) const { return kv + (size_t)row * kv_row_bytes + (size_t)(2 * layer + 1) * kv_plane; }
};

namespace {

const std::string SM = "point_encoder.model.shape_model.", DEC = "transformer.model.decoder.", TOK = "tokenizer.";
void require_ready(ma_engine* e) {
    if (!e->weights_ready) throw MaError(MA_ERR_STATE, "weights are not loaded (ma_engine_load_weights + ma_engine_finalize_weights, or ma_engine_mark_weights_loaded)");
}
void check_batch(ma_engine* e, int B) {
    if (B < 1 || B > e->cfg.max_batch) throw MaError(MA_ERR_INVALID, "batch size " + std::to_string(B) + " outside [1, max_batch=" + std::to_string(e->cfg.max_batch) + "]");
}

template <typename F>
int guarded(ma_engine* e, F f) {
    try {
        if (e) { hipError_t r = hipSetDevice(e->device); if (r != hipSuccess) throw MaError(MA_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(r)); }
        f();
        return MA_OK;
    } catch (const MaError& x) {
        if (e) e->err = x.msg; else g_create_error = x.msg;
        return x.code;
    } catch (const std::exception& x) {
        if (e) e->err = x.what(); else g_create_error = x.what();
        return MA_ERR_INVALID;
    } catch (...) {
        if (e) e->err = "unknown exception"; else g_create_error = "unknown exception";
        return MA_ERR_INVALID;
    }
}

}  // namespace
