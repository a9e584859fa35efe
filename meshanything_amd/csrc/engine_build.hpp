// Engine construction and destruction: configuration checks, the weight records of the dense phases and of the decode step (a missing name fails here), device buffers (the in-launch exchanges through xalloc), residency gates of the fused launches. (No includes of its own: compiled only inside engine.hip, in its include order.)
#pragma once

namespace {

void validate_config(const ma_config& c) {
    auto bad = [](const std::string& m) { throw MaError(MA_ERR_INVALID, "ma_config: " + m); };
    if (c.struct_size != (int32_t)sizeof(ma_config)) bad("struct_size mismatch (header/library version skew)");
    if (c.enc_width != c.enc_heads * 64 || c.hidden != c.heads * 64 || c.tok_width != c.tok_heads * 64) bad("head_dim must be 64 (width = heads*64)");
    if (c.codebook_dim != c.hidden) bad("codebook_dim must equal hidden (word_embed_proj_dim is forced to hidden_size, meshanything.py:112-113)");
    if (c.dtype != MA_DTYPE_F32 && c.dtype != MA_DTYPE_BF16 && c.dtype != MA_DTYPE_F16) bad("dtype must be MA_DTYPE_F32, MA_DTYPE_BF16 or MA_DTYPE_F16");
    const int dims[] = {c.enc_width, c.hidden, c.ffn, c.tok_width, c.tok_ffn, c.embed_dim, c.codebook_dim};
    for (int d : dims) if (d <= 0 || d % 32) bad("GEMM dimensions must be positive multiples of 32");
    if (3 * (2 * c.num_freqs + 1) + 3 > 64 || c.num_freqs < 1 || c.num_freqs > 20) bad("num_freqs out of range");
    if (c.n_points < 1 || c.num_latents < 1 || c.layers < 1 || c.enc_layers < 0 || c.shape_layers < 0 || c.tok_layers < 0) bad("non-positive size");
    if (c.n_max_faces < 1 || c.n_max_faces > c.tok_max_pos) bad("n_max_faces out of range");
    if (c.num_latents + 1 + c.n_max_faces * 9 + 2 > c.max_positions) bad("max_positions too small for cond_length + 9*n_max_faces + 2");
    if (c.max_batch < 1 || c.kv_splits < 0 || c.discrete_num < 1 || c.codebook_size < 1) bad("policy field out of range");
    // pick_kernel parks the V = codebook_size + 3 logits in dynamic LDS next to ~19 KB of static LDS (64 KB per workgroup without opt-in)
    if ((size_t)(c.codebook_size + 3) * 4 + 20 * 1024 > 64 * 1024) bad("codebook_size too large for the sampler's LDS stage (max 11261)");
}

// every matrix / bias / LayerNorm pair of the dense phases, by its arena name, into e->dw, and the decode step's tables into e->decw (engine_state.hpp)
void resolve_weights(ma_engine* e) {
    const ma_config& c = e->cfg;
    auto lin = [&](const std::string& p, bool bias = true) {
        const Entry& en = e->entry(p + ".weight");
        return Lin{e->arena + en.offset, bias ? e->PF(p + ".bias") : nullptr, en.rows, en.cols, en.dtype, en.name.c_str()};
    };
    auto ln = [&](const std::string& p, float eps = 1e-5f) { return LnW{e->PF(p + ".weight"), e->PF(p + ".bias"), eps}; };
    auto resblock = [&](const std::string& p) { return ResBlockW{ln(p + "ln_1"), ln(p + "ln_2"), lin(p + "attn.c_qkv", false), lin(p + "attn.c_proj"), lin(p + "mlp.c_fc"), lin(p + "mlp.c_proj")}; };
    DenseW& w = e->dw;
    w.query = e->PF(SM + "encoder.query"); w.input_proj = lin(SM + "encoder.input_proj");
    const std::string cp = SM + "encoder.cross_attn.";
    w.cross = CrossBlockW{ln(cp + "ln_1"), ln(cp + "ln_2"), ln(cp + "ln_3"), lin(cp + "attn.c_q", false), lin(cp + "attn.c_kv", false), lin(cp + "attn.c_proj"), lin(cp + "mlp.c_fc"), lin(cp + "mlp.c_proj")};
    for (int n = 0; n < c.enc_layers; ++n) w.enc.push_back(resblock(SM + "encoder.self_attn.resblocks." + std::to_string(n) + "."));
    w.ln_post = ln(SM + "encoder.ln_post"); w.pre_kl = lin(SM + "pre_kl"); w.post_kl = lin(SM + "post_kl");
    for (int n = 0; n < c.shape_layers; ++n) w.shape.push_back(resblock(SM + "transformer.resblocks." + std::to_string(n) + "."));
    w.cond_head = lin("cond_head_proj"); w.cond = lin("cond_proj");
    w.cond_embed = e->PF(DEC + "cond_embed.weight"); w.embed_pos = e->PF(DEC + "embed_positions.weight");
    for (int l = 0; l < c.layers; ++l) {
        const std::string p = DEC + "layers." + std::to_string(l) + ".";
        w.opt.push_back(PostLnLayerW{lin(p + "qkv"), lin(p + "self_attn.out_proj"), lin(p + "fc1"), lin(p + "fc2"), ln(p + "self_attn_layer_norm"), ln(p + "final_layer_norm")});
    }
    w.tok_cond_head = lin(TOK + "cond_head_proj"); w.tok_cond = lin(TOK + "cond_proj"); w.project_down = lin(TOK + "project_down_codebook"); w.to_coor = lin(TOK + "to_coor_logits.0");
    w.point_ln = ln(TOK + "point_layernorm"); w.face_ln = ln(TOK + "layernorm");
    w.point_pe = e->PF(TOK + "point_pe.weight"); w.pos_emb = e->PF(TOK + "pos_embedding.weight"); w.codebooks = e->PF(DEC + "quantize_codebooks");
    for (int n = 0; n < c.tok_layers; ++n) {
        const std::string p = TOK + "decoder.layer." + std::to_string(n) + ".";
        w.bert.push_back(PostLnLayerW{lin(p + "qkv"), lin(p + "attention.output.dense"), lin(p + "intermediate.dense"), lin(p + "output.dense"), ln(p + "attention.output.LayerNorm", 1e-12f), ln(p + "output.LayerNorm", 1e-12f)});
    }
    e->decw = DecW{e->P("transformer.lm_head.weight"), e->P(DEC + "input_layer.weight"), e->PF(DEC + "input_layer.bias"), w.codebooks, e->PF(DEC + "extra_embeds.weight"),
                   e->PF(DEC + "token_embed_positions.weight"), w.cond_embed, w.embed_pos, e->entry(DEC + "embed_positions.weight").rows};
}

void build_engine(ma_engine* e) {
    const ma_config& c = e->cfg;
    e->L = build_layout(c);
    pack_state_init(e->L, e->ps);
    e->T = c.num_latents + 1; e->V = c.codebook_size + 3; e->maxnew = c.n_max_faces * 9 + 2; e->maxseq = e->T + e->maxnew;
    e->nf = c.n_max_faces; e->S = e->T + e->nf;
    e->bf16 = c.dtype != MA_DTYPE_F32; e->hdt = c.dtype == MA_DTYPE_F16 ? MA_DTYPE_F16 : MA_DTYPE_BF16; e->kv_elem = e->bf16 ? 2 : 4;
    HIP_CHECK(hipMalloc(&e->arena, e->L.bytes));
    HIP_CHECK(hipMemset(e->arena, 0, e->L.bytes));
    const size_t MB = c.max_batch;
    e->kv_plane = (size_t)c.heads * e->maxseq * 64 * e->kv_elem;
    e->kv_row_bytes = e->kv_plane * 2 * c.layers;
    HIP_CHECK(hipMalloc(&e->kv, e->kv_row_bytes * MB));
    HIP_CHECK(hipMemset(e->kv, 0, e->kv_row_bytes * MB));
    const int H = c.hidden;
    // decode-step buffers: one slice per batch row
    e->d_e = e->dmalloc<float>(MB * H); e->d_q = e->dmalloc<float>(MB * H);
    e->d_ypre1 = e->dmalloc<float>(MB * H); e->d_ypre2 = e->dmalloc<float>(MB * H); e->d_h0 = e->dmalloc<float>(MB * H); e->d_h1 = e->dmalloc<float>(MB * H);
    e->d_ffn = e->dmalloc<float>(MB * c.ffn); e->d_logits = e->dmalloc<float>(MB * e->V);
    e->d_part = e->dmalloc<float>(MB * attn_workspace_floats(c.heads));
    e->n_parts = gemv_blocks(e, e->V, c.hidden);
    e->d_pval = e->dmalloc<float>(MB * e->V); e->d_pidx = e->dmalloc<int>(MB * e->V);        // row stride V >= blocks for any rows-per-block
    e->d_st = e->dmalloc<DecState>(MB);
    e->d_embtab = e->dmalloc<float>((size_t)c.codebook_size * H);      // (ensure_embtab fills it)
    // the in-launch exchanges (xalloc: zeroed here and again for every generation, because their epochs are tagged with the cache position, which restarts)
    e->d_qkv_gran = e->xalloc<u64>(MB * 3 * H);
    e->d_chain_err = e->xalloc<unsigned>(12, 1);      // [0] error bits (cleared when read, and per generation), [1] expiries ever, [2] longest slow block (ticks), [3] slow blocks ever, [4] scalar sweeps rescued by a vector look (rows_attn.hpp)
    e->d_y1_gran = e->xalloc<u64>(MB * H);
    e->d_attn_pair_gran = e->xalloc<unsigned long long>(MB * c.heads * ATTN_PAIR_GRANULES);
    e->d_y2_gran = e->xalloc<u64>(MB * H);
    e->d_ra_qkv_gran = e->xalloc<u64>(MB * RA_QKV_GRANULES); e->d_ra_out_gran = e->xalloc<u64>(MB * RA_OUT_GRANULES);
    e->d_pf_sink = e->dmalloc<unsigned>(4);
    e->d_rm_y2_gran = e->xalloc<u64>(MB * RM_Y2_GRANULES);
    e->d_ffn_gran = e->xalloc<u64>(MB * (size_t)c.ffn);
    exp_alloc_exchanges(e);
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&e->h_chain_err), sizeof(unsigned)));
    e->d_xb = e->dmalloc<bf16_t>(MB * H); e->d_ffb = e->dmalloc<bf16_t>(MB * c.ffn);
    e->d_ks_o = e->dmalloc<float>(4 * MB * H); e->d_ks_f = e->dmalloc<float>(4 * MB * H);
    HIP_CHECK(hipMemset(e->d_st, 0, MB * sizeof(DecState)));
    {   // persistent decode step: shape / device eligibility and its buffers
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, e->device));
        e->n_cus = prop.multiProcessorCount;
        {   // the fused launches spin on each other's granules: all 256 blocks of a batch row must be resident together.  The occupancy
            // API can report one block per CU too many (MI355X guide, correctness boundaries), so one block per CU is taken off and a
            // quarter is kept as margin; a partitioned device (CPX: 32 CUs) falls back to the five-launch chain.
            int occ_a = 0, occ_b = 0;
            // (the fp32 policy's instantiations hold twice the weight registers: asked about separately; the two 16-bit formats share theirs)
            const hipError_t qa = PREC_CALL(e->bf16, MA_DTYPE_BF16, T, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_a, qkv_attn_kernel<PRO_LN, T>, 256, 0));
            const hipError_t qb = PREC_CALL(e->bf16, MA_DTYPE_BF16, T, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_b, oproj_fc1_kernel<4, true, T>, 256, 0));
            if (qa != hipSuccess || qb != hipSuccess) { (void)hipGetLastError(); occ_a = occ_b = 0; }
            const int occ_c = exp_layer_pair_occupancy();
            const int occ_min = std::min(std::min(occ_a, occ_b), occ_c);
            // (a register-bound occupancy of two -- the fp32 instantiations at 171-210 VGPRs -- is exact: the over-report concerns the SGPR-limited
            // high-occupancy cases; 512 slots for the 256 blocks of batch 1 is the quarter of margin and more)
            const int usable = occ_min > 2 ? occ_min - 1 : occ_min;              // blocks per CU counted on
            e->resident_blocks = (long)e->n_cus * usable;
            e->chain_resident = e->resident_blocks * 4 >= 256L * 5;
            // the two-launch 8-row layer: 256 blocks of 8 waves at ~190-236 registers = one block per CU -- a register / wave-slot bound, where the
            // occupancy query is exact: every block must find a CU
            int occ_ra = 0, occ_rm = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_ra, rows_attn_kernel<true, 4, true, 3, 8, bf16_t>, 512, 0) != hipSuccess ||
                hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_rm, rows_mlp_kernel<bf16_t>, 512, 0) != hipSuccess) { (void)hipGetLastError(); occ_ra = occ_rm = 0; }
            e->rows_ok = (long)e->n_cus * std::min(occ_ra, occ_rm) >= 256;
        }
        exp_build_gates(e, prop);
    }
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&e->h_state), MB * sizeof(DecState)));
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&e->h_tokens), MB * e->maxnew * sizeof(long long)));
    // dense workspace: R = dense_rows samples stacked along the rows (R x 4096 point rows / R x 257 latent rows / R x 1057
    // detokenizer rows per pass)
    const int N = c.n_points, W = c.enc_width, T = e->T, Wt = c.tok_width, S = e->S, NL = c.num_latents;
    e->enc_exact = !e->bf16 || c.enc_exact != 0;
    const size_t enc_elem = e->enc_exact ? 4 : 2;                    // element size of the buffers the encoder's activations live in
    e->dense_rows = std::min(c.max_batch, 64);                        // 64 x 4096 point rows per pass: 5 GB of workspace at the 350M shape (bf16 policy)
    e->prefill_rows = e->dense_rows;
    const size_t R = e->dense_rows;
    const size_t rows_seq = R * std::max(T, S);                      // rows of the latent / token streams
    const size_t wmax = std::max(W, Wt);
    const size_t fmax = std::max(4 * W, c.tok_ffn);
    auto amalloc = [&](size_t elems) -> void* { return e->dmalloc<char>(elems * std::max<size_t>(e->bf16 ? 2 : 4, enc_elem)); };      // (buffers shared by the phases take the wider element)
    e->w_data = e->dmalloc<float>(R * N * W);
    e->w_lat = e->dmalloc<float>(R * T * W); e->w_lat2 = e->dmalloc<float>(R * NL * W);
    e->w_pf = e->dmalloc<float>(R * T * Wt); e->w_x = e->dmalloc<float>(R * S * Wt); e->w_y = e->dmalloc<float>(R * S * Wt);
    e->w_fe = e->dmalloc<float>(R * e->nf * Wt); e->w_logit = e->dmalloc<float>(R * e->nf * 9 * c.discrete_num);
    e->w_mask = e->dmalloc<unsigned char>(R * e->nf);
    e->a_feat = amalloc(R * N * 64); e->a_dataln = amalloc(R * N * W); e->a_kv = amalloc(R * N * 2 * W); e->a_q = amalloc((size_t)T * W);
    if (e->bf16) {
        size_t v = attn2_vt_elems(N, c.enc_heads, (int)R);
        v = std::max(v, attn2_vt_elems(T, c.enc_heads, (int)R)); v = std::max(v, attn2_vt_elems(T, c.heads, (int)R)); v = std::max(v, attn2_vt_elems(S, c.tok_heads, (int)R));
        e->vt_elems = v; e->a_vt = e->dmalloc<bf16_t>(v);
    }
    e->a_ln = amalloc(rows_seq * wmax); e->a_qkv = amalloc(rows_seq * 3 * wmax); e->a_att = amalloc(rows_seq * wmax); e->a_mlp = amalloc(rows_seq * fmax);
    e->a_cat = amalloc(R * NL * 2 * W); e->a_mean = amalloc(R * NL * c.embed_dim); e->a_fein = amalloc(R * e->nf * 3 * c.codebook_dim);
    e->a_x = amalloc(R * S * Wt);
    {
        const size_t PR = R * T;
        const size_t PS = std::min<size_t>(PR, 10240);           // (a split GEMM has fewer than 0.6 x CUs tiles of 256 x 256: at most ~40 tile rows)
        e->p_y_part_stride = (long)(PS * H);
        e->p_h = e->dmalloc<float>(PR * H); e->p_y = e->dmalloc<float>(std::max(PR, 4 * PS) * H);
        e->ln_gran_tiles = (PR / 256 + 1) * (size_t)((H + 255) / 256);
        e->d_ln_gran = e->xalloc<u64>(2 * e->ln_gran_tiles * 256, 0);      // (its epoch counter, ln_epoch, runs on across generations)
        e->a_ph = amalloc(PR * H); e->a_pqkv = amalloc(PR * 3 * H); e->a_patt = amalloc(PR * H); e->a_pffn = amalloc(PR * c.ffn);
        if (e->bf16) {
            e->a_patt_tail = amalloc((size_t)64 * H);
            e->vt_tail_elems = attn2_vt_elems(T, c.heads, 1); e->a_vt_tail = e->dmalloc<bf16_t>(e->vt_tail_elems);
        }
    }
    const size_t B = c.max_batch;
    e->w_latents = e->dmalloc<float>(B * T * W); e->w_prefix = e->dmalloc<float>(B * T * H);
    e->w_tokens = e->dmalloc<long long>(B * e->maxnew); e->w_ids = e->dmalloc<long long>(B * (size_t)e->nf * 9);
    resolve_weights(e);
    // per-layer decode pointers: the matrices the prefill runs, as the decode kernels take them
    e->dl.resize(c.layers);
    for (int l = 0; l < c.layers; ++l) {
        const PostLnLayerW& w = e->dw.opt[l];
        e->dl[l] = DecLayerPtrs{w.qkv.w, w.o.w, w.fc1.w, w.fc2.w, w.qkv.b, w.o.b, w.fc1.b, w.fc2.b, w.ln1.g, w.ln1.b, w.ln2.g, w.ln2.b};
    }
    exp_upload_layers(e);
}

void destroy_engine(ma_engine* e) {
    (void)hipSetDevice(e->device);
    drop_graphs(e);
    if (e->cap_stream) (void)hipStreamDestroy(e->cap_stream);
    if (e->tail_stream) (void)hipStreamDestroy(e->tail_stream);
    if (e->tail_stream_low) (void)hipStreamDestroy(e->tail_stream_low);
    if (e->tail_fork) (void)hipEventDestroy(e->tail_fork);
    if (e->tail_join) (void)hipEventDestroy(e->tail_join);
    for (hipEvent_t ev : e->tail_kv) (void)hipEventDestroy(ev);
    for (hipStream_t st : e->grp_stream) (void)hipStreamDestroy(st);
    for (hipEvent_t ev : e->grp_done) (void)hipEventDestroy(ev);
    if (e->grp_fork) (void)hipEventDestroy(e->grp_fork);
    for (void* p : e->allocs) (void)hipFree(p);
    if (e->arena) (void)hipFree(e->arena);
    if (e->stage) (void)hipFree(e->stage);
    if (e->kv) (void)hipFree(e->kv);
    if (e->h_state) (void)hipHostFree(e->h_state);
    if (e->h_err) (void)hipHostFree(e->h_err);
    if (e->h_chain_err) (void)hipHostFree(e->h_chain_err);
    if (e->h_tokens) (void)hipHostFree(e->h_tokens);
    delete e;
}

}  // namespace
