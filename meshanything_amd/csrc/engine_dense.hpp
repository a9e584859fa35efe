// The dense phases: point encoder, prefill and detokenizer, nb <= dense_rows samples at a time stacked along the GEMM rows. (No includes of its own: compiled only inside engine.hip, in its include order.)
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------ dense-phase helpers
// Buffer kinds (dense_ops.hpp): fp32 "stream" tensors (float*) and "activation" tensors (void*, element = e->act_elem bytes:
// bf16 under the bf16 policy, fp32 under the exact policy).  All dense phases run a CHUNK of nb <= e->dense_rows samples at
// once, stacked along the GEMM rows.
inline void* aoff(ma_engine* e, void* p, size_t elems) { return reinterpret_cast<char*>(p) + elems * e->act_elem; }
inline const void* aoff(ma_engine* e, const void* p, size_t elems) { return reinterpret_cast<const char*>(p) + elems * e->act_elem; }

// the precision of the launches enqueued while it lives (see ma_engine::dense16)
struct DenseScope {
    ma_engine* e; bool saved16; size_t saved_elem;
    DenseScope(ma_engine* e_, bool use16) : e(e_), saved16(e_->dense16), saved_elem(e_->act_elem) { e->dense16 = use16; e->act_elem = use16 ? 2 : 4; }
    ~DenseScope() { e->dense16 = saved16; e->act_elem = saved_elem; }
    DenseScope(const DenseScope&) = delete; DenseScope& operator=(const DenseScope&) = delete;
};

struct GemmOut {                       // exactly one of: fp32 stream output | activation output
    float* c32 = nullptr; void* act = nullptr; int ld = 0; RowMap map{0, 0, 0};
};
// C = act(A . W^T + bias) + R, A an activation tensor (M, lda).  r_mod > 0: the residual row is m % r_mod.
// kv (optional, 16-bit phases): the K / V columns of a fused q|k|v projection may go straight to these KV-cache planes (GemmTArgs::kv_*);
// kv->rows_done = the leading rows for which they did
struct KvDst { void* k = nullptr; void* v = nullptr; size_t row_stride = 0; int max_seq = 0, T = 0, col0 = 0; int rows_done = 0; };
void gemm(ma_engine* e, hipStream_t s, const void* A, int lda, const std::string& w, const char* bias_name, const float* R, int ldr, GemmOut out,
          int M, int act, int r_mod = 0, KvDst* kv = nullptr, GemmSplitK* sk = nullptr, GemmLnFuse* lnf = nullptr, int part = 0) {
    const Entry& en = e->L.get(w);
    const float* bias = bias_name ? e->PF(bias_name) : nullptr;
    hipError_t r;
    if ((en.dtype != MA_DTYPE_F32) != e->dense16) throw MaError(MA_ERR_INVALID, "internal: weight " + w + " does not have the precision of the phase that uses it");
    if (e->dense16) {
        GemmTArgs t{};
        t.A = reinterpret_cast<const bf16_t*>(A); t.lda = lda; t.W = reinterpret_cast<const bf16_t*>(e->arena + en.offset); t.bias = bias;
        t.R = R; t.ldr = ldr; t.C = out.c32; t.ldc = out.ld; t.Cb = reinterpret_cast<bf16_t*>(out.act); t.ldcb = out.ld;
        t.M = M; t.N = en.rows; t.K = en.cols; t.act = act; t.r_mod = r_mod; t.cmap = out.map; t.xcd_swizzle = e->opt.gemm_xcd_swizzle; t.part = part;
        if (kv) { t.kv_k = reinterpret_cast<bf16_t*>(kv->k); t.kv_v = reinterpret_cast<bf16_t*>(kv->v); t.kv_row_stride = kv->row_stride; t.kv_max_seq = kv->max_seq; t.kv_T = kv->T; t.kv_col0 = kv->col0; }
        r = H16_CALL(e->hdt, HT, launch_gemm_dense<HT>(t, e->n_cus, s, kv ? &kv->rows_done : nullptr, sk, lnf));
    } else {
        if (part != 0) throw MaError(MA_ERR_INVALID, "internal: a GEMM by row parts needs a 16-bit phase");
        GemmArgs g{};
        g.A = reinterpret_cast<const float*>(A); g.lda = lda; g.W = e->arena + en.offset; g.bias = bias; g.R = R; g.ldr = ldr;
        g.C = out.c32 ? out.c32 : reinterpret_cast<float*>(out.act); g.ldc = out.ld; g.M = M; g.N = en.rows; g.K = en.cols; g.act = act;
        g.r_mod = r_mod; g.cmap = out.map;
        r = launch_gemm<float>(g, e->opt.gemm_impl, s);
    }
    if (r != hipSuccess) throw MaError(MA_ERR_HIP, "gemm launch failed for " + w + ": " + hipGetErrorString(r));
}
void gemm(ma_engine* e, hipStream_t s, const void* A, int lda, const std::string& w, const std::string& b, const float* R, int ldr, GemmOut out, int M,
          int act, int r_mod = 0, KvDst* kv = nullptr, GemmSplitK* sk = nullptr, GemmLnFuse* lnf = nullptr, int part = 0) {
    gemm(e, s, A, lda, w, b.c_str(), R, ldr, out, M, act, r_mod, kv, sk, lnf, part);
}

GemmOut to32(float* c, int ld, RowMap m = RowMap{0, 0, 0}) { GemmOut o; o.c32 = c; o.ld = ld; o.map = m; return o; }
GemmOut toact(void* a, int ld, RowMap m = RowMap{0, 0, 0}) { GemmOut o; o.act = a; o.ld = ld; o.map = m; return o; }

// LayerNorm rows: x fp32 (row map xin) -> y32 (fp32, optional) and ya (activation, optional), both at row map yout
// (parts > 1: the input of the first split_rows rows is the sum of `parts` buffers part_stride floats apart -- a GEMM split along K)
void lnrows(ma_engine* e, hipStream_t s, const float* x, int ldx, const std::string& prefix, float eps, float* y32, int ld32, void* ya, int lda, int rows,
            int D, RowMap xin = RowMap{0, 0, 0}, RowMap yout = RowMap{0, 0, 0}, int parts = 1, long part_stride = 0, int split_rows = 0) {
    const float* g = e->PF(prefix + "weight"); const float* b = e->PF(prefix + "bias");
    if (parts > 1 && !(e->dense16 && D == 1024 && (parts == 2 || parts == 4))) throw MaError(MA_ERR_INVALID, "internal: LayerNorm over a split input needs a 16-bit phase and 1024 columns");
    if (e->dense16) H16_DO(e->hdt, HT, launch_ln_rows2<HT>(x, ldx, xin, g, b, eps, y32, ld32, reinterpret_cast<HT*>(ya), lda, yout, rows, D, s, parts, part_stride, split_rows));
    else launch_ln_rows2<float>(x, ldx, xin, g, b, eps, y32, ld32, reinterpret_cast<float*>(ya), lda, yout, rows, D, s);
    HIP_CHECK(hipGetLastError());
}
// h = LN(h + A W^T + b) for M stacked rows, fp32 in place + 16-bit copy hb (the two post-LN sub-layers of an OPT layer, [3p] OPTDecoderLayer): the GEMM
// finishes the LayerNorm itself where it can (gemm256.hpp LNF form: whole 256-row tiles of a launch that fills the chip); the row kernel does the rest from
// the plain sums in `y`.  split: fc2 of small batches may come as partial sums along K instead (GemmSplitK), which the row kernel adds up.
// part (GemmTArgs::part): 0 = all M rows; 1 = rows [0, M - M % 256); 2 = the rows behind them (A, h, hb, y stay the addresses of row 0)
void gemm_res_ln(ma_engine* e, hipStream_t s, const void* A, int lda, const std::string& w, const std::string& b, const std::string& ln_prefix, float eps, float* h, void* hb,
                 float* y, int M, int H, bool allow_split, int part = 0) {
    const bool fuse = part == 0 && e->opt.fuse_ln && e->dense16 && e->chain_resident && e->d_ln_gran && (size_t)(M / 256) * (size_t)(H / 256) <= e->ln_gran_tiles;
    GemmSplitK sk;
    // (from 8 samples on, like the tail chain: below that a sample's prefill keeps the bits of its batch-1 run -- the GEMMs run on row-independent tiles only)
    sk.max_parts = (allow_split && e->opt.gemm_splitk && e->dense16 && H == 1024 && M >= 2048 && (long)M * H <= e->p_y_part_stride) ? 4 : 1;
    sk.part_stride = e->p_y_part_stride;
    if (fuse) {
        GemmLnFuse lf;
        lf.ln.gamma = e->PF(ln_prefix + "weight"); lf.ln.beta = e->PF(ln_prefix + "bias"); lf.ln.eps = eps; lf.ln.gran = e->d_ln_gran; lf.ln.err = e->d_chain_err;
        if (++e->ln_epoch == 0) e->ln_epoch = 1;
        lf.ln.epoch = e->ln_epoch;
        lf.tail_c = y;
        GemmOut o; o.c32 = h; o.act = hb; o.ld = H;
        gemm(e, s, A, lda, w, b, h, H, o, M, ACT_NONE, 0, nullptr, &sk, &lf);
        if (lf.rows < M) {
            const size_t r0 = (size_t)lf.rows;
            // (a split GEMM never takes the LNF form: then lf.rows == 0 and the parts cover sk.rows rows from row 0)
            lnrows(e, s, y + r0 * H, H, ln_prefix, eps, h + r0 * H, H, reinterpret_cast<char*>(hb) + r0 * H * e->act_elem, H, M - lf.rows, H, RowMap{0, 0, 0}, RowMap{0, 0, 0},
                   sk.parts, sk.part_stride, sk.rows);
        }
        return;
    }
    gemm(e, s, A, lda, w, b, h, H, to32(y, H), M, ACT_NONE, 0, nullptr, &sk, nullptr, part);
    const int Mm = M - M % 256;
    if (part == 2) {        // (the rows behind the split ones are complete in the first buffer)
        const size_t r0 = (size_t)Mm;
        if (M > Mm) lnrows(e, s, y + r0 * H, H, ln_prefix, eps, h + r0 * H, H, reinterpret_cast<char*>(hb) + r0 * H * e->act_elem, H, M - Mm, H);
        return;
    }
    const int rows = part == 1 ? Mm : M;
    if (rows > 0) lnrows(e, s, y, H, ln_prefix, eps, h, H, hb, H, rows, H, RowMap{0, 0, 0}, RowMap{0, 0, 0}, sk.parts, sk.part_stride, std::min(sk.rows, rows));
}
// attention over activation tensors; strides in elements; batch = samples (grid.z)
void attention(ma_engine* e, hipStream_t s, const void* Q, int q_rs, int q_hs, const void* K, int k_rs, int k_hs, const void* Vp, int v_rs, int v_hs, void* O,
               int o_rs, int Sq, int Sk, int H, int causal_offset, int batch = 1, size_t q_bs = 0, size_t k_bs = 0, size_t v_bs = 0, size_t o_bs = 0, bf16_t* vt = nullptr,
               size_t vt_elems = 0) {
    AttnArgs a{Q, q_rs, q_hs, K, k_rs, k_hs, Vp, v_rs, v_hs, O, o_rs, Sq, Sk, H, 0.125f, causal_offset, e->dense16 ? 3 : 0};
    a.batch = batch; a.q_bs = q_bs; a.k_bs = k_bs; a.v_bs = v_bs; a.o_bs = o_bs;
    if (e->dense16 && (e->opt.attn_impl == 2 || e->hdt == MA_DTYPE_F16)) {     // (the first-generation kernel, attn_impl 1, is bf16 only)
        if (attn2_vt_elems(Sk, H, batch) > (vt ? vt_elems : e->vt_elems)) throw MaError(MA_ERR_INVALID, "internal: V^T workspace too small");
        HIP_CHECK(H16_CALL(e->hdt, HT, launch_attention2<HT>(a, vt ? vt : e->a_vt, s)));
    } else HIP_CHECK(launch_attention(a, s));
}
// fp32 stream rows (row map in, optional row mask) -> activation tensor
void cvt_rows(ma_engine* e, hipStream_t s, const float* src, int lds, RowMap in, const unsigned char* mask, void* dst, int ldd, int rows, int cols) {
    PREC_DO(e->dense16, e->hdt, T, hipLaunchKernelGGL((cvt_rows_kernel<T>), dim3(ceil_div(rows * cols, 256)), dim3(256), 0, s, src, lds, in, mask, reinterpret_cast<T*>(dst), ldd, rows, cols));
    HIP_CHECK(hipGetLastError());
}
void add_rows(ma_engine* e, hipStream_t s, const float* in, int ld_in, const unsigned char* mask, const float* t0, const float* tab, int ld_tab, int row0,
              float* out32, int ld_out, void* outa, int ld_outa, int rows, int cols, int tab_mod = 0) {
    PREC_DO(e->dense16, e->hdt, T, hipLaunchKernelGGL((add_rows2_kernel<T>), dim3(ceil_div(rows * cols, 256)), dim3(256), 0, s, in, ld_in, mask, t0, tab, ld_tab, row0, out32, ld_out,
                                                        reinterpret_cast<T*>(outa), ld_outa, rows, cols, tab_mod));
    HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ point encoder
// ResidualAttentionBlock (transformer_blocks.py:109-112): x += proj(attn(c_qkv(ln_1 x))); x += mlp(ln_2 x), for nb samples of S
// rows each stacked in x (nb * S, W) fp32, in place.
void miche_block(ma_engine* e, hipStream_t s, float* x, int S, int nb, const std::string& p) {
    const int W = e->cfg.enc_width, Hh = e->cfg.enc_heads, rows = nb * S;
    lnrows(e, s, x, W, p + "ln_1.", 1e-5f, nullptr, 0, e->a_ln, W, rows, W);
    gemm(e, s, e->a_ln, W, p + "attn.c_qkv.weight", nullptr, nullptr, 0, toact(e->a_qkv, 3 * W), rows, ACT_NONE);
    // per-head interleaved [q|k|v] (transformer_blocks.py:61-62): head stride 192, k at +64, v at +128
    attention(e, s, e->a_qkv, 3 * W, 192, aoff(e, e->a_qkv, 64), 3 * W, 192, aoff(e, e->a_qkv, 128), 3 * W, 192, e->a_att, W, S, S, Hh, -1, nb, (size_t)S * 3 * W,
              (size_t)S * 3 * W, (size_t)S * 3 * W, (size_t)S * W);
    gemm(e, s, e->a_att, W, p + "attn.c_proj.weight", p + "attn.c_proj.bias", x, W, to32(x, W), rows, ACT_NONE);
    lnrows(e, s, x, W, p + "ln_2.", 1e-5f, nullptr, 0, e->a_ln, W, rows, W);
    gemm(e, s, e->a_ln, W, p + "mlp.c_fc.weight", p + "mlp.c_fc.bias", nullptr, 0, toact(e->a_mlp, 4 * W), rows, ACT_GELU);
    gemm(e, s, e->a_mlp, 4 * W, p + "mlp.c_proj.weight", p + "mlp.c_proj.bias", x, W, to32(x, W), rows, ACT_NONE);
}

// encode_latents (asl_pl_module.py:145-157 -> sal_perceiver.py:372-381 -> 74-99) for nb samples -> latents (nb, T, W) fp32
void encode_chunk(ma_engine* e, hipStream_t s, const void* pc, int pc_dtype, int nb, float* latents) {
    const ma_config& c = e->cfg;
    const int N = c.n_points, W = c.enc_width, T = e->T, Hh = c.enc_heads, rowsN = nb * N, rowsT = nb * T;
    {
        const int total = rowsN * 64;
        if (pc_dtype == MA_DTYPE_F16) {
            PREC_DO(e->dense16, e->hdt, T, hipLaunchKernelGGL((fourier2_kernel<_Float16, T>), dim3(ceil_div(total, 256)), dim3(256), 0, s, reinterpret_cast<const _Float16*>(pc), rowsN, c.num_freqs, reinterpret_cast<T*>(e->a_feat), 64));
        } else {
            PREC_DO(e->dense16, e->hdt, T, hipLaunchKernelGGL((fourier2_kernel<float, T>), dim3(ceil_div(total, 256)), dim3(256), 0, s, reinterpret_cast<const float*>(pc), rowsN, c.num_freqs, reinterpret_cast<T*>(e->a_feat), 64));
        }
        HIP_CHECK(hipGetLastError());
    }
    gemm(e, s, e->a_feat, 64, SM + "encoder.input_proj.weight", SM + "encoder.input_proj.bias", nullptr, 0, to32(e->w_data, W), rowsN, ACT_NONE);
    const std::string p = SM + "encoder.cross_attn.";
    const float* query = e->PF(SM + "encoder.query");
    // x = query + attn(ln_1 query, ln_2 data); x += mlp(ln_3 x)     (transformer_blocks.py:223-226).  The query side is the same
    // for every sample: computed once, attended by every sample's keys (q batch stride 0)
    lnrows(e, s, query, W, p + "ln_1.", 1e-5f, nullptr, 0, e->a_ln, W, T, W);
    gemm(e, s, e->a_ln, W, p + "attn.c_q.weight", nullptr, nullptr, 0, toact(e->a_q, W), T, ACT_NONE);
    lnrows(e, s, e->w_data, W, p + "ln_2.", 1e-5f, nullptr, 0, e->a_dataln, W, rowsN, W);
    gemm(e, s, e->a_dataln, W, p + "attn.c_kv.weight", nullptr, nullptr, 0, toact(e->a_kv, 2 * W), rowsN, ACT_NONE);
    // kv viewed (N, heads, 128) split [k|v] (transformer_blocks.py:172-174)
    attention(e, s, e->a_q, W, 64, e->a_kv, 2 * W, 128, aoff(e, e->a_kv, 64), 2 * W, 128, e->a_att, W, T, N, Hh, -1, nb, 0, (size_t)N * 2 * W, (size_t)N * 2 * W,
              (size_t)T * W);
    gemm(e, s, e->a_att, W, p + "attn.c_proj.weight", p + "attn.c_proj.bias", query, W, to32(e->w_lat, W), rowsT, ACT_NONE, /*r_mod=*/T);
    lnrows(e, s, e->w_lat, W, p + "ln_3.", 1e-5f, nullptr, 0, e->a_ln, W, rowsT, W);
    gemm(e, s, e->a_ln, W, p + "mlp.c_fc.weight", p + "mlp.c_fc.bias", nullptr, 0, toact(e->a_mlp, 4 * W), rowsT, ACT_GELU);
    gemm(e, s, e->a_mlp, 4 * W, p + "mlp.c_proj.weight", p + "mlp.c_proj.bias", e->w_lat, W, to32(e->w_lat, W), rowsT, ACT_NONE);
    for (int n = 0; n < c.enc_layers; ++n) miche_block(e, s, e->w_lat, T, nb, SM + "encoder.self_attn.resblocks." + std::to_string(n) + ".");
    lnrows(e, s, e->w_lat, W, SM + "encoder.ln_post.", 1e-5f, latents, W, nullptr, 0, rowsT, W);
}

// to_shape_latents (asl_pl_module.py:182-185 -> sal_perceiver.py:383-396 pre_kl / mode() / post_kl, 273-275 transformer) for nb
// samples: lat rows `in` of a (.., ld) fp32 tensor -> e->w_lat2 (nb * NL, W) fp32
void shape_latents_chunk(ma_engine* e, hipStream_t s, const float* lat, int ld, RowMap in, int nb) {
    const ma_config& c = e->cfg;
    const int W = c.enc_width, E = c.embed_dim, NL = c.num_latents, rows = nb * NL;
    cvt_rows(e, s, lat, ld, in, nullptr, e->a_ln, W, rows, W);
    gemm(e, s, e->a_ln, W, SM + "pre_kl.weight", SM + "pre_kl.bias", nullptr, 0, toact(e->a_mean, E), rows, ACT_NONE);      // posterior.mode(): the mean half
    gemm(e, s, e->a_mean, E, SM + "post_kl.weight", SM + "post_kl.bias", nullptr, 0, to32(e->w_lat2, W), rows, ACT_NONE);
    for (int n = 0; n < c.shape_layers; ++n) miche_block(e, s, e->w_lat2, NL, nb, SM + "transformer.resblocks." + std::to_string(n) + ".");
}

// process_point_feature (meshanything.py:125-132) incl. to_shape_latents for nb samples: latents (nb, T, W) -> prefix (nb, T, H)
void prefix_chunk(ma_engine* e, hipStream_t s, const float* latents, float* prefix, int nb) {
    const ma_config& c = e->cfg;
    const int W = c.enc_width, H = c.hidden, NL = c.num_latents, T = e->T, rows = nb * NL;
    const RowMap tail{NL, T, 1}, head{1, T, 0};                            // point_feature[:, 1:] and [:, 0] inside the T-row blocks
    shape_latents_chunk(e, s, latents, W, tail, nb);
    cvt_rows(e, s, latents, W, tail, nullptr, e->a_cat, 2 * W, rows, W);                            // cat([latents, shape_latents], -1)
    cvt_rows(e, s, e->w_lat2, W, RowMap{0, 0, 0}, nullptr, aoff(e, e->a_cat, W), 2 * W, rows, W);
    cvt_rows(e, s, latents, W, head, nullptr, e->a_ln, W, nb, W);
    gemm(e, s, e->a_ln, W, "cond_head_proj.weight", "cond_head_proj.bias", nullptr, 0, to32(prefix, H, head), nb, ACT_NONE);
    gemm(e, s, e->a_cat, 2 * W, "cond_proj.weight", "cond_proj.bias", nullptr, 0, to32(prefix, H, tail), rows, ACT_NONE);
}

// prefill of rows row0 .. row0+B-1 in ONE pass (the samples are stacked along the GEMM rows: M = B * T): ShapeOPTDecoder.forward
// inputs_embeds branch (shape_opt.py:331-364) + 24 post-LN layers, causal per sample, on the T prefix rows of every sample;
// fills the rows' KV planes and leaves each row's first logits in d_logits[row]
void prefill(ma_engine* e, hipStream_t s, const float* prefix, int row0, int B) {
    const ma_config& c = e->cfg;
    const int T = e->T, H = c.hidden, M = B * T;
    StepTimer none;
    float* h = e->p_h;                       // (B*T, H)
    add_rows(e, s, prefix, H, nullptr, e->PF(DEC + "cond_embed.weight"), e->PF(DEC + "embed_positions.weight"), H, 2, h, H, e->a_ph, H, M, H, T);
    if (e->opt.prefill_stepwise) {
        // debug path: feed the prefix rows through the decode-step kernels one position at a time, one sample at a time
        for (int b = 0; b < B; ++b) {
            const Rows rw{row0 + b, 1};
            for (int j = 0; j < T; ++j) {
                hipLaunchKernelGGL(set_pos_kernel, dim3(1), dim3(1), 0, s, e->d_st + row0 + b, 0, j, 0, 1);
                HIP_CHECK(hipGetLastError());
                for (int l = 0; l < c.layers; ++l) {
                    if (l == 0) enqueue_layer(e, s, 0, h + ((size_t)b * T + j) * H, nullptr, nullptr, -1, none, rw);
                    else enqueue_layer(e, s, l, e->d_ypre2 + (size_t)(row0 + b) * H, e->dl[l - 1].ln2_g, e->dl[l - 1].ln2_b, -1, none, rw);
                }
            }
            enqueue_lm_head(e, s, e->d_ypre2 + (size_t)(row0 + b) * H, H, e->dl[c.layers - 1].ln2_g, e->dl[c.layers - 1].ln2_b, none, rw);
        }
        return;
    }
    void* qkv = e->a_pqkv;                   // (B*T, 3H) activation
    void* att = e->a_patt;                   // (B*T, H) activation
    void* hb = e->a_ph;                      // (B*T, H) activation copy of h
    float* y = e->p_y;                       // (B*T, H)
    void* ffn = e->a_pffn;                   // (B*T, ffn) activation
    const size_t kv_row_elems = e->kv_row_bytes / e->kv_elem;
    // The last rows as a chain of their own (round 6).  M = B x 257 leaves M % 256 = B rows behind the 256-row tiles, and every GEMM of a layer ran them as a
    // launch of its own behind its tiles (the skinny GEMM: 6.5 us at 16 rows, 11 us at 64; with the K / V copy of those rows 25 - 47 us per layer = 9 - 12 % of the
    // prefill).  Those rows are the LAST B positions of the LAST sample: causal attention means no other row ever reads anything of theirs, so the rows in
    // front of them (`part 1`: exact tile rows, no tail launches) run all 24 layers without them, and they (`part 2`) follow on a second stream with the same
    // kernels the one-stream form gives them -- each of their layers needs from the main chain only that layer's K / V of the earlier positions (one event
    // per layer).  The main chain's attention still launches over all B x T query rows: the last B of them are stale rows of the q|k|v buffer, their output
    // goes to rows of `att` nobody reads (the tail chain has its own), and what they do to keys they can see but that the tail chain is still writing is
    // masked in every valid row (the planes are zeroed at creation, so a masked V is a finite number).  Same bits as the one-stream form.
    const int Mm = M - M % 256;
    const bool tail = e->opt.prefill_tail && e->bf16 && B >= 8 && M > Mm && M - Mm <= 64 && M - Mm <= T && e->a_patt_tail && attn2_vt_elems(T, c.heads, 1) <= e->vt_tail_elems;
    hipStream_t s2 = nullptr;
    if (tail) {
        if (!e->tail_stream) {
            HIP_CHECK(hipStreamCreateWithFlags(&e->tail_stream, hipStreamNonBlocking));
            HIP_CHECK(hipEventCreateWithFlags(&e->tail_fork, hipEventDisableTiming));
            HIP_CHECK(hipEventCreateWithFlags(&e->tail_join, hipEventDisableTiming));
            e->tail_kv.resize(c.layers);
            for (hipEvent_t& ev : e->tail_kv) HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        }
        s2 = e->tail_stream;
        if (e->opt.prefill_tail == 2) {
            if (!e->tail_stream_low) {
                int lo = 0, hi = 0;
                HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));            // (numerically: lo >= hi; lo = the least urgent)
                HIP_CHECK(hipStreamCreateWithPriority(&e->tail_stream_low, hipStreamNonBlocking, lo));
            }
            s2 = e->tail_stream_low;
        }
        HIP_CHECK(hipEventRecord(e->tail_fork, s));              // the embedded rows (h, hb) of every row are there
        HIP_CHECK(hipStreamWaitEvent(s2, e->tail_fork, 0));
    }
    const int mp = tail ? 1 : 0;                                     // the main chain's row part
    const int Mk = tail ? Mm : M;                                    // rows whose K / V the main chain puts into the planes
    for (int l = 0; l < c.layers; ++l) {
        const std::string p = DEC + "layers." + std::to_string(l) + ".";
        if (e->bf16) {
            // 16-bit policies: the K / V columns of the rows on the persistent 256 x 256 tiles go straight into the cache planes (gemm256.hpp, KV form);
            // the rows behind them (the 64-row tail of M = B x 257; every row when another kernel took the GEMM) are copied from the q|k|v tensor.
            // Attention then reads K, and the V^T packing V, from the planes: the cache IS the prefill's K / V operand.
            KvDst kv; kv.k = e->kplane(row0, l); kv.v = e->vplane(row0, l); kv.row_stride = kv_row_elems; kv.max_seq = e->maxseq; kv.T = T; kv.col0 = H;
            gemm(e, s, hb, H, p + "qkv.weight", p + "qkv.bias", nullptr, 0, toact(qkv, 3 * H), M, ACT_NONE, 0, e->opt.qkv_to_cache ? &kv : nullptr, nullptr, nullptr, mp);
            auto kv_fill = [&](hipStream_t st, int r_begin, int r_end) {
                const long n = (long)(r_end - r_begin) * c.heads * 8;
                hipLaunchKernelGGL((kv_fill_rows_kernel<bf16_t, bf16_t>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const bf16_t*>(qkv), 3 * H, H, 2 * H, r_begin, r_end, T,
                                   c.heads, e->maxseq, reinterpret_cast<bf16_t*>(kv.k), reinterpret_cast<bf16_t*>(kv.v), kv_row_elems);      // a copy of 16-bit words: either format
                HIP_CHECK(hipGetLastError());
            };
            if (kv.rows_done < Mk) kv_fill(s, kv.rows_done, Mk);
            if (tail) {
                // ---- the tail chain's layer l (stream s2): enqueued here, between the main chain's q|k|v and its attention ----
                HIP_CHECK(hipEventRecord(e->tail_kv[l], s));
                KvDst kv2 = kv;
                gemm(e, s2, hb, H, p + "qkv.weight", p + "qkv.bias", nullptr, 0, toact(qkv, 3 * H), M, ACT_NONE, 0, e->opt.qkv_to_cache ? &kv2 : nullptr, nullptr, nullptr, 2);
                kv_fill(s2, Mm, M);
                HIP_CHECK(hipStreamWaitEvent(s2, e->tail_kv[l], 0));
                const int nt = M - Mm;                               // its rows: positions T - nt .. T - 1 of sample B - 1
                void* att_t = e->a_patt_tail;
                attention(e, s2, aoff(e, qkv, (size_t)Mm * 3 * H), 3 * H, 64, e->kplane(row0 + B - 1, l), 64, e->maxseq * 64, e->vplane(row0 + B - 1, l), 64, e->maxseq * 64, att_t, H, nt, T,
                          c.heads, T - nt, 1, 0, 0, 0, 0, e->a_vt_tail, e->vt_tail_elems);
                // (row m of the A operand is read at A + m * lda: the address row 0 WOULD have)
                const void* att_t0 = reinterpret_cast<const char*>(att_t) - (size_t)Mm * H * e->act_elem;
                gemm_res_ln(e, s2, att_t0, H, p + "self_attn.out_proj.weight", p + "self_attn.out_proj.bias", p + "self_attn_layer_norm.", 1e-5f, h, hb, y, M, H, e->opt.gemm_splitk >= 2, 2);
                gemm(e, s2, hb, H, p + "fc1.weight", p + "fc1.bias", nullptr, 0, toact(ffn, c.ffn), M, ACT_RELU, 0, nullptr, nullptr, nullptr, 2);
                gemm_res_ln(e, s2, ffn, c.ffn, p + "fc2.weight", p + "fc2.bias", p + "final_layer_norm.", 1e-5f, h, hb, y, M, H, true, 2);
            }
            attention(e, s, qkv, 3 * H, 64, kv.k, 64, e->maxseq * 64, kv.v, 64, e->maxseq * 64, att, H, T, T, c.heads, 0, B, (size_t)T * 3 * H, kv_row_elems, kv_row_elems, (size_t)T * H);
        } else {
            gemm(e, s, hb, H, p + "qkv.weight", p + "qkv.bias", nullptr, 0, toact(qkv, 3 * H), M, ACT_NONE);
            const int n = T * c.heads * 64;
            hipLaunchKernelGGL((kv_fill2_kernel<float, float>), dim3(ceil_div(n, 256), B), dim3(256), 0, s, reinterpret_cast<const float*>(qkv), 3 * H, H, 2 * H, T, c.heads, e->maxseq,
                               reinterpret_cast<float*>(e->kplane(row0, l)), reinterpret_cast<float*>(e->vplane(row0, l)), kv_row_elems);
            HIP_CHECK(hipGetLastError());
            attention(e, s, qkv, 3 * H, 64, aoff(e, qkv, H), 3 * H, 64, aoff(e, qkv, 2 * H), 3 * H, 64, att, H, T, T, c.heads, 0, B, (size_t)T * 3 * H, (size_t)T * 3 * H,
                      (size_t)T * 3 * H, (size_t)T * H);
        }
        gemm_res_ln(e, s, att, H, p + "self_attn.out_proj.weight", p + "self_attn.out_proj.bias", p + "self_attn_layer_norm.", 1e-5f, h, hb, y, M, H, e->opt.gemm_splitk >= 2, mp);
        gemm(e, s, hb, H, p + "fc1.weight", p + "fc1.bias", nullptr, 0, toact(ffn, c.ffn), M, ACT_RELU, 0, nullptr, nullptr, nullptr, mp);
        // small batches: fc2's 256 x 256 tiles (N = hidden: four per tile row) fill a fraction of the chip while each runs 64 K-tiles -- split along K
        // into partial sums that the LayerNorm adds up (gemm256.hpp GemmSplitK; 16 samples: 64 tiles x 4 parts = one round of 16 K-tiles)
        gemm_res_ln(e, s, ffn, c.ffn, p + "fc2.weight", p + "fc2.bias", p + "final_layer_norm.", 1e-5f, h, hb, y, M, H, true, mp);
    }
    if (tail) {
        HIP_CHECK(hipEventRecord(e->tail_join, s2));
        HIP_CHECK(hipStreamWaitEvent(s, e->tail_join, 0));
    }
    // only the last prefix row of every sample feeds lm_head (the reference computes all 257 rows and discards 256, shape_opt.py:155)
    enqueue_lm_head(e, s, h + (size_t)(T - 1) * H, T * H, nullptr, nullptr, none, Rows{row0, B});
}

// ------------------------------------------------------------------------------------------------ detokenizer
// NoiseResistantDecoder.forward (meshanything.py:50-80) for nb samples stacked along the rows: X (nb, S = T + nf, Wt).
// codes != null: the caller's `input_embeds` (B, 3 nf, D) fp32 are used as the face codes (what the reference's signature
// takes); null: they are gathered from the codebook (get_codes, meshanything.py:178-212) inside the chain.
void detok_chunk(ma_engine* e, hipStream_t s, const long long* ids, const float* codes, const float* latents, float* coords, int nb) {
    const ma_config& c = e->cfg;
    const int W = c.enc_width, T = e->T, Wt = c.tok_width, nf = e->nf, S = e->S, D = c.codebook_dim, Hh = c.tok_heads;
    const int rowsS = nb * S, rowsF = nb * nf;
    float* X = e->w_x;                                               // (nb * S, Wt) fp32
    void* Xb = e->a_x;                                               // activation copy
    const RowMap head_in{1, T, 0}, tail_in{T - 1, T, 1};             // latents[:, 0] / [:, 1:] inside the T-row blocks
    const RowMap cond_out{T, S, 0}, face_out{nf, S, T};              // cond rows / face rows inside the S-row blocks of X
    // process_point_feature (meshanything.py:42-48): -> w_pf (nb * T, Wt); the projection of the encoder's latents keeps the encoder's precision
    {
        DenseScope enc(e, e->dense16 && !e->enc_exact);
        cvt_rows(e, s, latents, W, head_in, nullptr, e->a_ln, W, nb, W);
        gemm(e, s, e->a_ln, W, TOK + "cond_head_proj.weight", TOK + "cond_head_proj.bias", nullptr, 0, to32(e->w_pf, Wt, RowMap{1, T, 0}), nb, ACT_NONE);
        cvt_rows(e, s, latents, W, tail_in, nullptr, e->a_ln, W, nb * (T - 1), W);
        gemm(e, s, e->a_ln, W, TOK + "cond_proj.weight", TOK + "cond_proj.bias", nullptr, 0, to32(e->w_pf, Wt, RowMap{T - 1, T, 1}), nb * (T - 1), ACT_NONE);
    }
    add_rows(e, s, e->w_pf, Wt, nullptr, nullptr, e->PF(TOK + "point_pe.weight"), Wt, 0, e->w_pf, Wt, nullptr, 0, nb * T, Wt, T);
    lnrows(e, s, e->w_pf, Wt, TOK + "point_layernorm.", 1e-5f, X, Wt, Xb, Wt, nb * T, Wt, RowMap{0, 0, 0}, cond_out);
    // faces (meshanything.py:53-60): codes -> project_down -> zero masked -> + pos -> LN
    {
        const int total = rowsF * 3 * (D / 4);               // four consecutive d per thread
        PREC_DO(e->dense16, e->hdt, T, hipLaunchKernelGGL((codes_gather2_kernel<T>), dim3(ceil_div(total, 256)), dim3(256), 0, s, ids, e->PF(DEC + "quantize_codebooks"), D, rowsF, (float*)nullptr,
                                                            codes ? nullptr : reinterpret_cast<T*>(e->a_fein), e->w_mask));
        HIP_CHECK(hipGetLastError());
        if (codes) cvt_rows(e, s, codes, 3 * D, RowMap{0, 0, 0}, nullptr, e->a_fein, 3 * D, rowsF, 3 * D);     // 'b (nf nv) d -> b nf (nv d)' is a view
    }
    gemm(e, s, e->a_fein, 3 * D, TOK + "project_down_codebook.weight", TOK + "project_down_codebook.bias", nullptr, 0, to32(e->w_fe, Wt), rowsF, ACT_NONE);
    add_rows(e, s, e->w_fe, Wt, e->w_mask, nullptr, e->PF(TOK + "pos_embedding.weight"), Wt, 0, e->w_fe, Wt, nullptr, 0, rowsF, Wt, nf);
    lnrows(e, s, e->w_fe, Wt, TOK + "layernorm.", 1e-5f, X, Wt, Xb, Wt, rowsF, Wt, RowMap{0, 0, 0}, face_out);
    // 6 BERT post-LN layers, bidirectional, NO mask: padding faces take part as LN(pos_embedding[i]) tokens
    void* qkv = e->a_qkv; void* att = e->a_att; float* y = e->w_y; void* ffn = e->a_mlp;
    for (int n = 0; n < c.tok_layers; ++n) {
        const std::string p = TOK + "decoder.layer." + std::to_string(n) + ".";
        gemm(e, s, Xb, Wt, p + "qkv.weight", p + "qkv.bias", nullptr, 0, toact(qkv, 3 * Wt), rowsS, ACT_NONE);
        attention(e, s, qkv, 3 * Wt, 64, aoff(e, qkv, Wt), 3 * Wt, 64, aoff(e, qkv, 2 * Wt), 3 * Wt, 64, att, Wt, S, S, Hh, -1, nb, (size_t)S * 3 * Wt, (size_t)S * 3 * Wt,
                  (size_t)S * 3 * Wt, (size_t)S * Wt);
        gemm(e, s, att, Wt, p + "attention.output.dense.weight", p + "attention.output.dense.bias", X, Wt, to32(y, Wt), rowsS, ACT_NONE);
        lnrows(e, s, y, Wt, p + "attention.output.LayerNorm.", 1e-12f, X, Wt, Xb, Wt, rowsS, Wt);
        gemm(e, s, Xb, Wt, p + "intermediate.dense.weight", p + "intermediate.dense.bias", nullptr, 0, toact(ffn, c.tok_ffn), rowsS, ACT_GELU);
        gemm(e, s, ffn, c.tok_ffn, p + "output.dense.weight", p + "output.dense.bias", X, Wt, to32(y, Wt), rowsS, ACT_NONE);
        lnrows(e, s, y, Wt, p + "output.LayerNorm.", 1e-12f, X, Wt, Xb, Wt, rowsS, Wt);
    }
    // last_hidden_state[:, cond_length:], masked faces zeroed (meshanything.py:65-68) -> to_coor_logits
    cvt_rows(e, s, X, Wt, face_out, e->w_mask, e->a_ln, Wt, rowsF, Wt);
    gemm(e, s, e->a_ln, Wt, TOK + "to_coor_logits.0.weight", TOK + "to_coor_logits.0.bias", nullptr, 0, to32(e->w_logit, 9 * c.discrete_num), rowsF, ACT_NONE);
    hipLaunchKernelGGL(coords_argmax_kernel, dim3(ceil_div(rowsF * 9, 4)), dim3(256), 0, s, e->w_logit, rowsF, c.discrete_num, e->w_mask, coords);
    HIP_CHECK(hipGetLastError());
}

}  // namespace
