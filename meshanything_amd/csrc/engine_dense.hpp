// The dense phases: point encoder, prefill and detokenizer, nb <= dense_rows samples at a time stacked along the GEMM rows. (No includes of its own: compiled only inside engine.hip, in its include order.)
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------ dense-phase helpers
// Buffer kinds (dense_ops.hpp): fp32 "stream" tensors (float*) and "activation" tensors (void*: 16-bit elements in a 16-bit phase, fp32 in an
// exact one).  All dense phases run a CHUNK of nb <= e->dense_rows samples at once, stacked along the GEMM rows.  The arguments of the helpers
// are small aggregates built at the call site: a plain call passes nothing of the options, a special one names what it sets.
struct GemmOut {                       // exactly one of: fp32 stream output | activation output
    float* c32 = nullptr; void* act = nullptr; int ld = 0; RowMap map{0, 0, 0};
};
GemmOut to32(float* c, int ld, RowMap m = RowMap{0, 0, 0}) { GemmOut o; o.c32 = c; o.ld = ld; o.map = m; return o; }
GemmOut toact(void* a, int ld, RowMap m = RowMap{0, 0, 0}) { GemmOut o; o.act = a; o.ld = ld; o.map = m; return o; }
// kv (16-bit phases): the K / V columns of a fused q|k|v projection may go straight to these KV-cache planes (GemmTArgs::kv_*);
// kv->rows_done = the leading rows for which they did
struct KvDst { void* k = nullptr; void* v = nullptr; size_t row_stride = 0; int max_seq = 0, T = 0, col0 = 0; int rows_done = 0; };
// C = act(A . W^T + bias) + R.  r_mod > 0: the residual row is m % r_mod.  part (GemmTArgs::part): see gemm_res_ln
struct GemmOpts { int act = ACT_NONE; const float* R = nullptr; int ldr = 0, r_mod = 0; KvDst* kv = nullptr; GemmSplitK* sk = nullptr; GemmLnFuse* lnf = nullptr; int part = 0; };
// LayerNorm rows: x fp32 (row map xin) -> y32 (fp32, optional) and act (activation, optional), both at row map `map`
// (parts > 1: the input of the first split_rows rows is the sum of `parts` buffers part_stride floats apart -- a GEMM split along K)
struct LnDst { float* y32 = nullptr; int ld32 = 0; void* act = nullptr; int lda = 0; RowMap map{0, 0, 0}; };
struct LnOpts { RowMap xin{0, 0, 0}; int parts = 1; long part_stride = 0; int split_rows = 0; };
struct ResLnBufs { float* h; void* hb; float* y; };       // gemm_res_ln: the fp32 stream (in place), its activation copy, scratch for the plain sums
// attention operands: element strides between rows (rs), heads (hs) and samples (bs); the output's heads are 64 apart
struct AttnView { const void* p; int rs, hs; size_t bs = 0; };
struct AttnOut { void* p; int rs; size_t bs = 0; };
struct AttnShape { int Sq, Sk, heads, causal_offset, batch = 1, last_len = -1; };      // (last_len: AttnArgs, attn.hpp)
struct AttnOpts { bf16_t* vt = nullptr; size_t vt_elems = 0; };      // a V^T workspace other than the engine's (attn2.hpp)
// out = (mask ? in : 0) + t0 + tab[(i % tab_mod) + row0] -> fp32 (out32, may alias in) and activation copy (outa, optional): add_rows2_kernel
struct AddRows {
    const float* in; int ld_in; const unsigned char* mask = nullptr; const float* t0 = nullptr; const float* tab; int ld_tab, row0 = 0, tab_mod = 0;
    float* out32; int ld_out; void* outa = nullptr; int ld_outa = 0; int rows, cols;
};

// What a dense phase enqueues on and in which precision: every phase entry builds its own (the encoder phases e->bf16 && !e->enc_exact, prefill and
// the BERT stack e->bf16); which kernel a helper launches and how it offsets an activation pointer follow from it alone.
struct Dense {
    ma_engine* e; hipStream_t s; bool is16;
    size_t elem() const { return is16 ? 2 : 4; }
    Dense on(hipStream_t other) const { return Dense{e, other, is16}; }
    void* at(void* p, size_t elems) const { return reinterpret_cast<char*>(p) + elems * elem(); }
    const void* at(const void* p, size_t elems) const { return reinterpret_cast<const char*>(p) + elems * elem(); }
    // the address row 0 of an (.., ld) operand WOULD have when p is its row `rows`: a GEMM by row parts reads row m at A + m * lda
    const void* rows_back(const void* p, size_t rows, int ld) const { return reinterpret_cast<const char*>(p) - rows * ld * elem(); }

    void gemm(const void* A, int lda, const Lin& w, GemmOut out, int M, const GemmOpts& o = {}) const {
        hipError_t r;
        if ((w.dtype != MA_DTYPE_F32) != is16) throw MaError(MA_ERR_INVALID, std::string("internal: weight ").append(w.name).append(" does not have the precision of the phase that uses it"));
        if (is16) {
            GemmTArgs t{};
            t.A = reinterpret_cast<const bf16_t*>(A); t.lda = lda; t.W = reinterpret_cast<const bf16_t*>(w.w); t.bias = w.b;
            t.R = o.R; t.ldr = o.ldr; t.C = out.c32; t.ldc = out.ld; t.Cb = reinterpret_cast<bf16_t*>(out.act); t.ldcb = out.ld;
            t.M = M; t.N = w.rows; t.K = w.cols; t.act = o.act; t.r_mod = o.r_mod; t.cmap = out.map; t.xcd_swizzle = e->opt.gemm_xcd_swizzle; t.part = o.part;
            if (o.kv) { t.kv_k = reinterpret_cast<bf16_t*>(o.kv->k); t.kv_v = reinterpret_cast<bf16_t*>(o.kv->v); t.kv_row_stride = o.kv->row_stride; t.kv_max_seq = o.kv->max_seq; t.kv_T = o.kv->T; t.kv_col0 = o.kv->col0; }
            r = H16_CALL(e->hdt, HT, launch_gemm_dense<HT>(t, e->n_cus, s, o.kv ? &o.kv->rows_done : nullptr, o.sk, o.lnf, e->opt.gemm_tune()));
        } else {
            if (o.part != 0) throw MaError(MA_ERR_INVALID, "internal: a GEMM by row parts needs a 16-bit phase");
            GemmArgs g{};
            g.A = reinterpret_cast<const float*>(A); g.lda = lda; g.W = w.w; g.bias = w.b; g.R = o.R; g.ldr = o.ldr;
            g.C = out.c32 ? out.c32 : reinterpret_cast<float*>(out.act); g.ldc = out.ld; g.M = M; g.N = w.rows; g.K = w.cols; g.act = o.act;
            g.r_mod = o.r_mod; g.cmap = out.map;
            r = launch_gemm<float>(g, e->opt.gemm_impl, s);
        }
        if (r != hipSuccess) throw MaError(MA_ERR_HIP, std::string("gemm launch failed for ").append(w.name).append(": ").append(hipGetErrorString(r)));
    }
    void lnrows(const float* x, int ldx, const LnW& ln, LnDst y, int rows, int D, const LnOpts& o = {}) const {
        if (o.parts > 1 && !(is16 && D == 1024 && (o.parts == 2 || o.parts == 4))) throw MaError(MA_ERR_INVALID, "internal: LayerNorm over a split input needs a 16-bit phase and 1024 columns");
        if (is16) H16_DO(e->hdt, HT, launch_ln_rows2<HT>(x, ldx, o.xin, ln.g, ln.b, ln.eps, y.y32, y.ld32, reinterpret_cast<HT*>(y.act), y.lda, y.map, rows, D, s, o.parts, o.part_stride, o.split_rows));
        else launch_ln_rows2<float>(x, ldx, o.xin, ln.g, ln.b, ln.eps, y.y32, y.ld32, reinterpret_cast<float*>(y.act), y.lda, y.map, rows, D, s);
        HIP_CHECK(hipGetLastError());
    }
    // h = LN(h + A W^T + b) for M stacked rows of H = w.rows columns, fp32 in place + 16-bit copy hb (the two post-LN sub-layers of an OPT layer, [3p]
    // OPTDecoderLayer): the GEMM finishes the LayerNorm itself where it can (gemm256.hpp LNF form: whole 256-row tiles of a launch that fills the chip); the
    // row kernel does the rest from the plain sums in `y`.  split: fc2 of small batches may come as partial sums along K instead (GemmSplitK), which the row
    // kernel adds up.
    // part (GemmTArgs::part): 0 = all M rows; 1 = rows [0, M - M % 256); 2 = the rows behind them (A, h, hb, y stay the addresses of row 0)
    void gemm_res_ln(const void* A, int lda, const Lin& w, const LnW& ln, ResLnBufs b, int M, bool allow_split, int part = 0) const {
        const int H = w.rows;
        const bool fuse = part == 0 && e->opt.fuse_ln && is16 && e->chain_resident && e->d_ln_gran && (size_t)(M / 256) * (size_t)(H / 256) <= e->ln_gran_tiles;
        GemmSplitK sk;
        // (from 8 samples on, like the tail chain: below that a sample's prefill keeps the bits of its batch-1 run -- the GEMMs run on row-independent tiles only)
        sk.max_parts = (allow_split && e->opt.gemm_splitk && is16 && H == 1024 && M >= 2048 && (long)M * H <= e->p_y_part_stride) ? 4 : 1;
        sk.part_stride = e->p_y_part_stride;
        if (fuse) {
            GemmLnFuse lf;
            lf.ln.gamma = ln.g; lf.ln.beta = ln.b; lf.ln.eps = ln.eps; lf.ln.gran = e->d_ln_gran; lf.ln.err = e->d_chain_err;
            if (++e->ln_epoch == 0) e->ln_epoch = 1;
            lf.ln.epoch = e->ln_epoch;
            lf.tail_c = b.y;
            GemmOut out; out.c32 = b.h; out.act = b.hb; out.ld = H;
            gemm(A, lda, w, out, M, {.R = b.h, .ldr = H, .sk = &sk, .lnf = &lf});
            if (lf.rows < M) {
                const size_t r0 = (size_t)lf.rows;
                // (a split GEMM never takes the LNF form: then lf.rows == 0 and the parts cover sk.rows rows from row 0)
                lnrows(b.y + r0 * H, H, ln, {.y32 = b.h + r0 * H, .ld32 = H, .act = at(b.hb, r0 * H), .lda = H}, M - lf.rows, H, {.parts = sk.parts, .part_stride = sk.part_stride, .split_rows = sk.rows});
            }
            return;
        }
        gemm(A, lda, w, to32(b.y, H), M, {.R = b.h, .ldr = H, .sk = &sk, .part = part});
        const int Mm = M - M % 256;
        if (part == 2) {        // (the rows behind the split ones are complete in the first buffer)
            const size_t r0 = (size_t)Mm;
            if (M > Mm) lnrows(b.y + r0 * H, H, ln, {.y32 = b.h + r0 * H, .ld32 = H, .act = at(b.hb, r0 * H), .lda = H}, M - Mm, H);
            return;
        }
        const int rows = part == 1 ? Mm : M;
        if (rows > 0) lnrows(b.y, H, ln, {.y32 = b.h, .ld32 = H, .act = b.hb, .lda = H}, rows, H, {.parts = sk.parts, .part_stride = sk.part_stride, .split_rows = std::min(sk.rows, rows)});
    }
    // attention over activation tensors; sh.batch = samples (grid.z)
    void attention(AttnView q, AttnView k, AttnView v, AttnOut o, AttnShape sh, const AttnOpts& w = {}) const {
        AttnArgs a{q.p, q.rs, q.hs, k.p, k.rs, k.hs, v.p, v.rs, v.hs, o.p, o.rs, sh.Sq, sh.Sk, sh.heads, 0.125f, sh.causal_offset, is16 ? 3 : 0};
        a.batch = sh.batch; a.last_len = sh.last_len; a.q_bs = q.bs; a.k_bs = k.bs; a.v_bs = v.bs; a.o_bs = o.bs;
        if (is16 && (e->opt.attn_impl == 2 || e->hdt == MA_DTYPE_F16)) {     // (the first-generation kernel, attn_impl 1, is bf16 only)
            if (attn2_vt_elems(sh.Sk, sh.heads, sh.batch) > (w.vt ? w.vt_elems : e->vt_elems)) throw MaError(MA_ERR_INVALID, "internal: V^T workspace too small");
            HIP_CHECK(H16_CALL(e->hdt, HT, launch_attention2<HT>(a, w.vt ? w.vt : e->a_vt, s)));
        } else HIP_CHECK(launch_attention(a, s));
    }
    // fp32 stream rows (row map in, optional row mask) -> activation tensor
    void cvt_rows(const float* src, int lds, RowMap in, const unsigned char* mask, void* dst, int ldd, int rows, int cols) const {
        PREC_DO(is16, e->hdt, T, hipLaunchKernelGGL((cvt_rows_kernel<T>), dim3(ceil_div(rows * cols, 256)), dim3(256), 0, s, src, lds, in, mask, reinterpret_cast<T*>(dst), ldd, rows, cols));
        HIP_CHECK(hipGetLastError());
    }
    void add_rows(const AddRows& a) const {
        PREC_DO(is16, e->hdt, T, hipLaunchKernelGGL((add_rows2_kernel<T>), dim3(ceil_div(a.rows * a.cols, 256)), dim3(256), 0, s, a.in, a.ld_in, a.mask, a.t0, a.tab, a.ld_tab, a.row0, a.out32, a.ld_out,
                                                     reinterpret_cast<T*>(a.outa), a.ld_outa, a.rows, a.cols, a.tab_mod));
        HIP_CHECK(hipGetLastError());
    }
    // FourierEmbedder + normals of `rows` points (fp32 or fp16) -> activation tensor (rows, 64)
    template <typename PT> void fourier(const PT* pc, int rows, int num_freqs, void* out) const {
        PREC_DO(is16, e->hdt, T, hipLaunchKernelGGL((fourier2_kernel<PT, T>), dim3(ceil_div(rows * 64, 256)), dim3(256), 0, s, pc, rows, num_freqs, reinterpret_cast<T*>(out), 64));
        HIP_CHECK(hipGetLastError());
    }
};

// ------------------------------------------------------------------------------------------------ point encoder
// ResidualAttentionBlock (transformer_blocks.py:109-112): x += proj(attn(c_qkv(ln_1 x))); x += mlp(ln_2 x), for nb samples of S
// rows each stacked in x (nb * S, W) fp32, in place.
void miche_block(const Dense& d, float* x, int S, int nb, const ResBlockW& w) {
    ma_engine* e = d.e;
    const int W = e->cfg.enc_width, Hh = e->cfg.enc_heads, rows = nb * S;
    d.lnrows(x, W, w.ln1, {.act = e->a_ln, .lda = W}, rows, W);
    d.gemm(e->a_ln, W, w.qkv, toact(e->a_qkv, 3 * W), rows);
    // per-head interleaved [q|k|v] (transformer_blocks.py:61-62): head stride 192, k at +64, v at +128
    auto part = [&](int off) { return AttnView{d.at(e->a_qkv, off), 3 * W, 192, (size_t)S * 3 * W}; };
    d.attention(part(0), part(64), part(128), {e->a_att, W, (size_t)S * W}, {.Sq = S, .Sk = S, .heads = Hh, .causal_offset = -1, .batch = nb});
    d.gemm(e->a_att, W, w.proj, to32(x, W), rows, {.R = x, .ldr = W});
    d.lnrows(x, W, w.ln2, {.act = e->a_ln, .lda = W}, rows, W);
    d.gemm(e->a_ln, W, w.fc, toact(e->a_mlp, 4 * W), rows, {.act = ACT_GELU});
    d.gemm(e->a_mlp, 4 * W, w.fc_proj, to32(x, W), rows, {.R = x, .ldr = W});
}

// encode_latents (asl_pl_module.py:145-157 -> sal_perceiver.py:372-381 -> 74-99) for nb samples -> latents (nb, T, W) fp32
void encode_chunk(const Dense& d, const void* pc, int pc_dtype, int nb, float* latents) {
    ma_engine* e = d.e;
    const ma_config& c = e->cfg;
    const DenseW& w = e->dw;
    const int N = c.n_points, W = c.enc_width, T = e->T, Hh = c.enc_heads, rowsN = nb * N, rowsT = nb * T;
    if (pc_dtype == MA_DTYPE_F16) d.fourier(reinterpret_cast<const _Float16*>(pc), rowsN, c.num_freqs, e->a_feat);
    else d.fourier(reinterpret_cast<const float*>(pc), rowsN, c.num_freqs, e->a_feat);
    d.gemm(e->a_feat, 64, w.input_proj, to32(e->w_data, W), rowsN);
    // x = query + attn(ln_1 query, ln_2 data); x += mlp(ln_3 x)     (transformer_blocks.py:223-226).  The query side is the same
    // for every sample: computed once, attended by every sample's keys (q batch stride 0)
    d.lnrows(w.query, W, w.cross.ln1, {.act = e->a_ln, .lda = W}, T, W);
    d.gemm(e->a_ln, W, w.cross.q, toact(e->a_q, W), T);
    d.lnrows(e->w_data, W, w.cross.ln2, {.act = e->a_dataln, .lda = W}, rowsN, W);
    d.gemm(e->a_dataln, W, w.cross.kv, toact(e->a_kv, 2 * W), rowsN);
    // kv viewed (N, heads, 128) split [k|v] (transformer_blocks.py:172-174)
    const size_t kv_bs = (size_t)N * 2 * W;
    d.attention({e->a_q, W, 64}, {e->a_kv, 2 * W, 128, kv_bs}, {d.at(e->a_kv, 64), 2 * W, 128, kv_bs}, {e->a_att, W, (size_t)T * W}, {.Sq = T, .Sk = N, .heads = Hh, .causal_offset = -1, .batch = nb});
    d.gemm(e->a_att, W, w.cross.proj, to32(e->w_lat, W), rowsT, {.R = w.query, .ldr = W, .r_mod = T});
    d.lnrows(e->w_lat, W, w.cross.ln3, {.act = e->a_ln, .lda = W}, rowsT, W);
    d.gemm(e->a_ln, W, w.cross.fc, toact(e->a_mlp, 4 * W), rowsT, {.act = ACT_GELU});
    d.gemm(e->a_mlp, 4 * W, w.cross.fc_proj, to32(e->w_lat, W), rowsT, {.R = e->w_lat, .ldr = W});
    for (const ResBlockW& blk : w.enc) miche_block(d, e->w_lat, T, nb, blk);
    d.lnrows(e->w_lat, W, w.ln_post, {.y32 = latents, .ld32 = W}, rowsT, W);
}

// to_shape_latents (asl_pl_module.py:182-185 -> sal_perceiver.py:383-396 pre_kl / mode() / post_kl, 273-275 transformer) for nb
// samples: lat rows `in` of a (.., ld) fp32 tensor -> e->w_lat2 (nb * NL, W) fp32
void shape_latents_chunk(const Dense& d, const float* lat, int ld, RowMap in, int nb) {
    ma_engine* e = d.e;
    const ma_config& c = e->cfg;
    const int W = c.enc_width, E = c.embed_dim, NL = c.num_latents, rows = nb * NL;
    d.cvt_rows(lat, ld, in, nullptr, e->a_ln, W, rows, W);
    d.gemm(e->a_ln, W, e->dw.pre_kl, toact(e->a_mean, E), rows);      // posterior.mode(): the mean half
    d.gemm(e->a_mean, E, e->dw.post_kl, to32(e->w_lat2, W), rows);
    for (const ResBlockW& blk : e->dw.shape) miche_block(d, e->w_lat2, NL, nb, blk);
}

// process_point_feature (meshanything.py:125-132) incl. to_shape_latents for nb samples: latents (nb, T, W) -> prefix (nb, T, H)
void prefix_chunk(const Dense& d, const float* latents, float* prefix, int nb) {
    ma_engine* e = d.e;
    const ma_config& c = e->cfg;
    const int W = c.enc_width, H = c.hidden, NL = c.num_latents, T = e->T, rows = nb * NL;
    const RowMap tail{NL, T, 1}, head{1, T, 0};                            // point_feature[:, 1:] and [:, 0] inside the T-row blocks
    shape_latents_chunk(d, latents, W, tail, nb);
    d.cvt_rows(latents, W, tail, nullptr, e->a_cat, 2 * W, rows, W);                            // cat([latents, shape_latents], -1)
    d.cvt_rows(e->w_lat2, W, RowMap{0, 0, 0}, nullptr, d.at(e->a_cat, W), 2 * W, rows, W);
    d.cvt_rows(latents, W, head, nullptr, e->a_ln, W, nb, W);
    d.gemm(e->a_ln, W, e->dw.cond_head, to32(prefix, H, head), nb);
    d.gemm(e->a_cat, 2 * W, e->dw.cond, to32(prefix, H, tail), rows);
}

// prefill of rows row0 .. row0+B-1 in ONE pass (the samples are stacked along the GEMM rows: M = B * T): ShapeOPTDecoder.forward
// inputs_embeds branch (shape_opt.py:331-364) + 24 post-LN layers, causal per sample, on the T prefix rows of every sample;
// fills the rows' KV planes and leaves each row's first logits in d_logits[row]
void prefill(const Dense& d, const float* prefix, int row0, int B) {
    ma_engine* e = d.e;
    const hipStream_t s = d.s;
    const ma_config& c = e->cfg;
    const int T = e->T, H = c.hidden, M = B * T;
    StepTimer none;
    float* h = e->p_h;                       // (B*T, H)
    d.add_rows({.in = prefix, .ld_in = H, .t0 = e->dw.cond_embed, .tab = e->dw.embed_pos, .ld_tab = H, .row0 = 2, .tab_mod = T, .out32 = h, .ld_out = H, .outa = e->a_ph, .ld_outa = H, .rows = M, .cols = H});
    if (e->opt.prefill_stepwise) {
        // debug path: feed the prefix rows through the decode-step kernels one position at a time, one sample at a time
        for (int b = 0; b < B; ++b) {
            Step p(e, s, none, Rows{row0 + b, 1});
            for (int j = 0; j < T; ++j) {
                hipLaunchKernelGGL(set_pos_kernel, dim3(1), dim3(1), 0, s, p.st, 0, j, 0, 1);
                HIP_CHECK(hipGetLastError());
                gemv_chain(p, h + ((size_t)b * T + j) * H, j == T - 1);          // (lm_head behind the last position only)
            }
        }
        return;
    }
    void* qkv = e->a_pqkv;                   // (B*T, 3H) activation
    void* att = e->a_patt;                   // (B*T, H) activation
    void* hb = e->a_ph;                      // (B*T, H) activation copy of h
    void* ffn = e->a_pffn;                   // (B*T, ffn) activation
    const ResLnBufs hy{h, hb, e->p_y};       // (p_y: (B*T, H) plain sums in front of a LayerNorm)
    const size_t kv_row_elems = e->kv_row_bytes / e->kv_elem;
    // The last rows as a chain of their own (round 6).  M = B x 257 leaves M % 256 = B rows behind the 256-row tiles, and every GEMM of a layer ran them as a
    // launch of its own behind its tiles (the skinny GEMM: 6.5 us at 16 rows, 11 us at 64; with the K / V copy of those rows 25 - 47 us per layer = 9 - 12 % of the
    // prefill).  Those rows are the LAST B positions of the LAST sample: causal attention means no other row ever reads anything of theirs, so the rows in
    // front of them (`part 1`: exact tile rows, no tail launches) run all 24 layers without them, and they (`part 2`) follow on a second stream with the same
    // kernels the one-stream form gives them -- each of their layers needs from the main chain only that layer's K / V of the earlier positions (one event
    // per layer).  Neither chain touches what the other owns: the main chain's attention (and the V^T packing in front of it) takes the last sample as
    // T - nt rows and T - nt keys (AttnShape::last_len -- those rows never see a later key), so positions T - nt .. T - 1 of that sample's planes,
    // which the tail chain writes at a time of its own choosing, are read by the tail chain alone, behind its own writes, and the stale last rows of the
    // q|k|v buffer by nobody.  What a plane holds there from an earlier generation (it need not be finite: a masked probability is 0, and 0 x inf is
    // not) never reaches a kernel.  Same bits as the one-stream form: the keys left out were masked in every row that is kept.
    const int Mm = M - M % 256;
    const bool attn2 = e->opt.attn_impl == 2 || e->hdt == MA_DTYPE_F16;      // (the kernel that knows AttnShape::last_len)
    const bool tail = e->opt.prefill_tail && d.is16 && attn2 && B >= 8 && M > Mm && M - Mm <= 64 && M - Mm <= T && e->a_patt_tail && attn2_vt_elems(T, c.heads, 1) <= e->vt_tail_elems;
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
    const Dense d2 = d.on(s2);                                       // the tail chain's context
    const int mp = tail ? 1 : 0;                                     // the main chain's row part
    const int Mk = tail ? Mm : M;                                    // rows whose K / V the main chain puts into the planes
    for (int l = 0; l < c.layers; ++l) {
        const PostLnLayerW& w = e->dw.opt[l];
        const size_t q_bs = (size_t)T * 3 * H;
        const AttnShape causal{.Sq = T, .Sk = T, .heads = c.heads, .causal_offset = 0, .batch = B, .last_len = tail ? T - (M - Mm) : -1};
        if (d.is16) {
            // 16-bit policies: the K / V columns of the rows on the persistent 256 x 256 tiles go straight into the cache planes (gemm256.hpp, KV form);
            // the rows behind them (the 64-row tail of M = B x 257; every row when another kernel took the GEMM) are copied from the q|k|v tensor.
            // Attention then reads K, and the V^T packing V, from the planes: the cache IS the prefill's K / V operand.
            KvDst kv; kv.k = e->kplane(row0, l); kv.v = e->vplane(row0, l); kv.row_stride = kv_row_elems; kv.max_seq = e->maxseq; kv.T = T; kv.col0 = H;
            d.gemm(hb, H, w.qkv, toact(qkv, 3 * H), M, {.kv = e->opt.qkv_to_cache ? &kv : nullptr, .part = mp});
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
                d2.gemm(hb, H, w.qkv, toact(qkv, 3 * H), M, {.kv = e->opt.qkv_to_cache ? &kv2 : nullptr, .part = 2});
                kv_fill(s2, Mm, M);
                HIP_CHECK(hipStreamWaitEvent(s2, e->tail_kv[l], 0));
                const int nt = M - Mm;                               // its rows: positions T - nt .. T - 1 of sample B - 1
                d2.attention({d2.at(qkv, (size_t)Mm * 3 * H), 3 * H, 64}, {e->kplane(row0 + B - 1, l), 64, e->maxseq * 64}, {e->vplane(row0 + B - 1, l), 64, e->maxseq * 64}, {e->a_patt_tail, H},
                             {.Sq = nt, .Sk = T, .heads = c.heads, .causal_offset = T - nt}, {.vt = e->a_vt_tail, .vt_elems = e->vt_tail_elems});
                // (a_patt_tail holds row Mm: the GEMM by row parts wants the address of row 0)
                d2.gemm_res_ln(d2.rows_back(e->a_patt_tail, Mm, H), H, w.o, w.ln1, hy, M, e->opt.gemm_splitk >= 2, 2);
                d2.gemm(hb, H, w.fc1, toact(ffn, c.ffn), M, {.act = ACT_RELU, .part = 2});
                d2.gemm_res_ln(ffn, c.ffn, w.fc2, w.ln2, hy, M, true, 2);
            }
            d.attention({qkv, 3 * H, 64, q_bs}, {kv.k, 64, e->maxseq * 64, kv_row_elems}, {kv.v, 64, e->maxseq * 64, kv_row_elems}, {att, H, (size_t)T * H}, causal);
        } else {
            d.gemm(hb, H, w.qkv, toact(qkv, 3 * H), M);
            const int n = T * c.heads * 64;
            hipLaunchKernelGGL((kv_fill2_kernel<float, float>), dim3(ceil_div(n, 256), B), dim3(256), 0, s, reinterpret_cast<const float*>(qkv), 3 * H, H, 2 * H, T, c.heads, e->maxseq,
                               reinterpret_cast<float*>(e->kplane(row0, l)), reinterpret_cast<float*>(e->vplane(row0, l)), kv_row_elems);
            HIP_CHECK(hipGetLastError());
            d.attention({qkv, 3 * H, 64, q_bs}, {d.at(qkv, H), 3 * H, 64, q_bs}, {d.at(qkv, 2 * H), 3 * H, 64, q_bs}, {att, H, (size_t)T * H}, causal);
        }
        d.gemm_res_ln(att, H, w.o, w.ln1, hy, M, e->opt.gemm_splitk >= 2, mp);
        d.gemm(hb, H, w.fc1, toact(ffn, c.ffn), M, {.act = ACT_RELU, .part = mp});
        // small batches: fc2's 256 x 256 tiles (N = hidden: four per tile row) fill a fraction of the chip while each runs 64 K-tiles -- split along K
        // into partial sums that the LayerNorm adds up (gemm256.hpp GemmSplitK; 16 samples: 64 tiles x 4 parts = one round of 16 K-tiles)
        d.gemm_res_ln(ffn, c.ffn, w.fc2, w.ln2, hy, M, true, mp);
    }
    if (tail) {
        HIP_CHECK(hipEventRecord(e->tail_join, s2));
        HIP_CHECK(hipStreamWaitEvent(s, e->tail_join, 0));
    }
    // only the last prefix row of every sample feeds lm_head (the reference computes all 257 rows and discards 256, shape_opt.py:155)
    Step(e, s, none, Rows{row0, B}).lm_head(h + (size_t)(T - 1) * H, T * H, NO_LN);
}

// ------------------------------------------------------------------------------------------------ detokenizer
// NoiseResistantDecoder.forward (meshanything.py:50-80) for nb samples stacked along the rows: X (nb, S = T + nf, Wt).
// codes != null: the caller's `input_embeds` (B, 3 nf, D) fp32 are used as the face codes (what the reference's signature
// takes); null: they are gathered from the codebook (get_codes, meshanything.py:178-212) inside the chain.
void detok_chunk(const Dense& d, const long long* ids, const float* codes, const float* latents, float* coords, int nb) {
    ma_engine* e = d.e;
    const hipStream_t s = d.s;
    const ma_config& c = e->cfg;
    const DenseW& w = e->dw;
    const int W = c.enc_width, T = e->T, Wt = c.tok_width, nf = e->nf, S = e->S, D = c.codebook_dim, Hh = c.tok_heads;
    const int rowsS = nb * S, rowsF = nb * nf;
    float* X = e->w_x;                                               // (nb * S, Wt) fp32
    void* Xb = e->a_x;                                               // activation copy
    const RowMap head_in{1, T, 0}, tail_in{T - 1, T, 1};             // latents[:, 0] / [:, 1:] inside the T-row blocks
    const RowMap cond_out{T, S, 0}, face_out{nf, S, T};              // cond rows / face rows inside the S-row blocks of X
    // process_point_feature (meshanything.py:42-48): -> w_pf (nb * T, Wt); the projection of the encoder's latents keeps the encoder's precision
    const Dense enc{e, s, e->bf16 && !e->enc_exact};
    enc.cvt_rows(latents, W, head_in, nullptr, e->a_ln, W, nb, W);
    enc.gemm(e->a_ln, W, w.tok_cond_head, to32(e->w_pf, Wt, RowMap{1, T, 0}), nb);
    enc.cvt_rows(latents, W, tail_in, nullptr, e->a_ln, W, nb * (T - 1), W);
    enc.gemm(e->a_ln, W, w.tok_cond, to32(e->w_pf, Wt, RowMap{T - 1, T, 1}), nb * (T - 1));
    d.add_rows({.in = e->w_pf, .ld_in = Wt, .tab = w.point_pe, .ld_tab = Wt, .tab_mod = T, .out32 = e->w_pf, .ld_out = Wt, .rows = nb * T, .cols = Wt});
    d.lnrows(e->w_pf, Wt, w.point_ln, {.y32 = X, .ld32 = Wt, .act = Xb, .lda = Wt, .map = cond_out}, nb * T, Wt);
    // faces (meshanything.py:53-60): codes -> project_down -> zero masked -> + pos -> LN
    {
        const int total = rowsF * 3 * (D / 4);               // four consecutive d per thread
        PREC_DO(d.is16, e->hdt, T, hipLaunchKernelGGL((codes_gather2_kernel<T>), dim3(ceil_div(total, 256)), dim3(256), 0, s, ids, w.codebooks, D, rowsF, (float*)nullptr,
                                                            codes ? nullptr : reinterpret_cast<T*>(e->a_fein), e->w_mask));
        HIP_CHECK(hipGetLastError());
        if (codes) d.cvt_rows(codes, 3 * D, RowMap{0, 0, 0}, nullptr, e->a_fein, 3 * D, rowsF, 3 * D);     // 'b (nf nv) d -> b nf (nv d)' is a view
    }
    d.gemm(e->a_fein, 3 * D, w.project_down, to32(e->w_fe, Wt), rowsF);
    d.add_rows({.in = e->w_fe, .ld_in = Wt, .mask = e->w_mask, .tab = w.pos_emb, .ld_tab = Wt, .tab_mod = nf, .out32 = e->w_fe, .ld_out = Wt, .rows = rowsF, .cols = Wt});
    d.lnrows(e->w_fe, Wt, w.face_ln, {.y32 = X, .ld32 = Wt, .act = Xb, .lda = Wt, .map = face_out}, rowsF, Wt);
    // 6 BERT post-LN layers, bidirectional, NO mask: padding faces take part as LN(pos_embedding[i]) tokens
    void* qkv = e->a_qkv; void* att = e->a_att; float* y = e->w_y; void* ffn = e->a_mlp;
    const LnDst x_out{.y32 = X, .ld32 = Wt, .act = Xb, .lda = Wt};
    auto part = [&](int off) { return AttnView{d.at(qkv, off), 3 * Wt, 64, (size_t)S * 3 * Wt}; };      // [q|k|v] by thirds of the row
    for (const PostLnLayerW& l : w.bert) {
        d.gemm(Xb, Wt, l.qkv, toact(qkv, 3 * Wt), rowsS);
        d.attention(part(0), part(Wt), part(2 * Wt), {att, Wt, (size_t)S * Wt}, {.Sq = S, .Sk = S, .heads = Hh, .causal_offset = -1, .batch = nb});
        d.gemm(att, Wt, l.o, to32(y, Wt), rowsS, {.R = X, .ldr = Wt});
        d.lnrows(y, Wt, l.ln1, x_out, rowsS, Wt);
        d.gemm(Xb, Wt, l.fc1, toact(ffn, c.tok_ffn), rowsS, {.act = ACT_GELU});
        d.gemm(ffn, c.tok_ffn, l.fc2, to32(y, Wt), rowsS, {.R = X, .ldr = Wt});
        d.lnrows(y, Wt, l.ln2, x_out, rowsS, Wt);
    }
    // last_hidden_state[:, cond_length:], masked faces zeroed (meshanything.py:65-68) -> to_coor_logits
    d.cvt_rows(X, Wt, face_out, e->w_mask, e->a_ln, Wt, rowsF, Wt);
    d.gemm(e->a_ln, Wt, w.to_coor, to32(e->w_logit, 9 * c.discrete_num), rowsF);
    hipLaunchKernelGGL(coords_argmax_kernel, dim3(ceil_div(rowsF * 9, 4)), dim3(256), 0, s, e->w_logit, rowsF, c.discrete_num, e->w_mask, coords);
    HIP_CHECK(hipGetLastError());
}

}  // namespace
