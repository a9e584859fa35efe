// Host side of the measured-and-rejected decode-step forms (MA_EXPERIMENTAL=1 libraries only): the rows-looped two-launch layer
// (rows_fused.hpp), the layer-pair launch (layer_fused.hpp) and the persistent one-launch step (persist.hpp).  Included by
// engine_decode.hpp, which gives the product build one block of stubs instead; no includes of its own.
#pragma once

namespace {

// (engine_generate.hpp)
void state_at(ma_engine* e, hipStream_t s, int B, int kv_len);

// 2 .. 8 rows on the rows-looped two-launch layer: 256 blocks whatever the batch, so the residency condition is the batch-1 one
bool use_rows_fused(ma_engine* e, int B, int len_override) {
    const ma_config& c = e->cfg;
    return e->opt.rows_fused && e->rf_ok && e->chain_resident && len_override < 0 && e->bf16 && B >= std::max(2, e->opt.rows_fused_min) && B <= RF_MAX_ROWS &&
           c.hidden == 1024 && c.ffn == 4096 && c.heads * 64 == c.hidden && c.heads * ATTN_NCHUNK == 256 && c.layers <= 30;
}

void enqueue_layer_rows_fused(ma_engine* e, hipStream_t s, int l, const float* x_in, const float* ln_g, const float* ln_b, StepTimer& tm, Rows rw) {
    const ma_config& c = e->cfg;
    const int H = c.hidden;
    const size_t r0 = rw.r0;
    RowsFusedArgs A{};
    A.q = make_qkv_attn_args(e, l, x_in, ln_g, ln_b, -1, rw);
    A.q.trace = tm.trace_slot(2, ATTN_NCHUNK * c.heads);
    const float* resid = ln_g ? e->d_h0 + r0 * H : x_in;
    A.o = make_oproj_fc1_args(e, l, resid, rw, true);
    A.o.trace = tm.trace_slot(3, H / 4);
    A.part_gran = e->d_part_gran + r0 * c.heads * ATTN_NCHUNK * RF_PART;
    A.attn_out = e->d_xb + r0 * H; A.attn_out_stride = H;
    A.B = rw.B;
    if (tm.on(1)) {
        launched(launch_qkv_attn_rows(A, c.heads, s), "qkv_attn_rows");
    }
    if (tm.on(0)) {
        launched(launch_oproj_fc1_rows(A, H, c.ffn, s), "oproj_fc1_rows");
    }
}

bool fuse_layer(ma_engine* e, int B = 1, int len_override = -1) { return e->opt.fuse_layer && e->bf16 && e->hdt == MA_DTYPE_BF16 && fuse_qkv_attn(e, B, len_override) && fuse_oproj_fc1(e, B, len_override) && e->opt.fuse_fc2; }

// second half of layer l + first half of layer l + 1 in one launch (layer_fused.hpp); belongs to the "cache" class of the profiler
void enqueue_layer_pair(ma_engine* e, hipStream_t s, int l, const float* resid, int len_override, StepTimer& tm, Rows rw) {
    const ma_config& c = e->cfg;
    LayerFusedArgs a{};
    a.o = make_oproj_fc1_args(e, l, resid, rw, true);
    a.q = make_qkv_attn_args(e, l + 1, nullptr, e->dl[l].ln2_g, e->dl[l].ln2_b, len_override, rw);
    a.gran3 = e->d_y2_gran + (size_t)rw.r0 * c.hidden;
    if (tm.on(1)) {
        launched(launch_layer_fused(a, c.hidden, c.ffn, c.heads, rw.B, s), "layer_fused");
    }
}

// ---- persistent decode step (persist.hpp) ----------------------------------------------------------------------------------
// eligible: bf16 policy, one row, greedy, the 350M layer shape, a device with exactly the 256 CUs the kernel assigns roles to
bool persist_eligible(ma_engine* e, int B, int do_sample) { return e->persist_shape && B == 1 && !do_sample; }
bool persist_selected(ma_engine* e, int B, int do_sample) { return e->opt.decode_impl == 1 && persist_eligible(e, B, do_sample); }

void enqueue_persist_step(ma_engine* e, hipStream_t s, StepTimer& tm, u64* trace = nullptr) {
    if (!tm.on(2)) return;
    const ma_config& c = e->cfg;
    PersistArgs a{};
    a.layers = e->d_layers; a.L = c.layers;
    a.lm_head = reinterpret_cast<const bf16_t*>(e->P("transformer.lm_head.weight")); a.V = e->V;
    a.embtab = e->d_embtab; a.extra = e->PF(DEC + "extra_embeds.weight"); a.tokpos = e->PF(DEC + "token_embed_positions.weight");
    a.cond = e->PF(DEC + "cond_embed.weight"); a.postab = e->PF(DEC + "embed_positions.weight"); a.T = e->T;
    a.kv = reinterpret_cast<bf16_t*>(e->kv); a.kv_plane = e->kv_plane / e->kv_elem; a.max_seq = e->maxseq;
    a.st = e->d_st; a.tokens_out = e->w_tokens; a.logits = e->d_logits;
    a.gran = e->d_gran; a.serial = e->d_serial; a.err = e->d_err; a.trace = trace;
    launched(launch_persist_decode(a, s), "persistent decode");
}

// the persistent step reports a bounded wait that expired through a device word: turn it into an error (and clear it)
void check_persist_error(ma_engine* e, hipStream_t s) {
    if (!e->persist_shape) return;
    HIP_CHECK(hipMemcpyAsync(e->h_err, e->d_err, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (*e->h_err) {
        const unsigned code = *e->h_err;
        HIP_CHECK(hipMemsetAsync(e->d_err, 0, sizeof(unsigned), s));
        throw MaError(MA_ERR_HIP, "persistent decode step: a bounded wait expired (code " + std::to_string(code) +
                                  ": 1 loader, 2 comm, 4 compute, 8 gather) -- the 256 workgroups were not all resident, or a hand-off was lost");
    }
}

// ---- the parts of init_state / build_engine that exist for these forms only (called where the blocks stood, so the order of device allocations stays)
void exp_reset_exchanges(ma_engine* e, hipStream_t s) {
    HIP_CHECK(hipMemsetAsync(e->d_part_gran, 0, (size_t)e->cfg.max_batch * e->cfg.heads * ATTN_NCHUNK * RF_PART * sizeof(u64), s));
}
void exp_alloc_exchanges(ma_engine* e) {
    const size_t n = (size_t)e->cfg.max_batch * (size_t)e->cfg.heads * ATTN_NCHUNK * RF_PART;
    e->d_part_gran = e->dmalloc<u64>(n);
    HIP_CHECK(hipMemset(e->d_part_gran, 0, n * sizeof(u64)));
}
int exp_layer_pair_occupancy() {
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, layer_fused_kernel, 256, 0) != hipSuccess) { (void)hipGetLastError(); occ = 0; }
    return occ;
}
// the residency gate of the rows-looped launches (the second one holds 66-130 KB of LDS, i.e. ONE block per CU -- an LDS bound, where the occupancy query is
// exact: 256 blocks need 256 CUs), then the persistent decode step: shape / device eligibility and its buffers
void exp_build_gates(ma_engine* e, const hipDeviceProp_t& prop) {
    const ma_config& c = e->cfg;
    int occ_r = 0;
    e->rf_ok = e->bf16 && e->hdt == MA_DTYPE_BF16 && rf_prepare() == hipSuccess &&
               hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_r, oproj_fc1_rows_kernel<8>, 256, rf_oproj_lds(8)) == hipSuccess && (long)e->n_cus * occ_r >= 256;
    if (!e->rf_ok) (void)hipGetLastError();
    e->persist_shape = e->bf16 && e->hdt == MA_DTYPE_BF16 && c.hidden == PS_H && c.ffn == PS_F && c.heads == PS_HEADS && c.codebook_dim == PS_H && c.heads * ATTN_NCHUNK == PS_CUS &&
                       e->V >= PS_CUS * 32 && e->V <= PS_CUS * 33 && e->n_cus == PS_CUS && (size_t)prop.sharedMemPerBlockOptin >= PL_TOTAL;
    if (e->persist_shape && persist_prepare() != hipSuccess) { (void)hipGetLastError(); e->persist_shape = false; }
    if (!e->persist_shape) return;
    e->d_layers = e->dmalloc<DecLayerPtrs>(c.layers);
    e->d_gran = e->dmalloc<u64>(PG_TOTAL); e->d_serial = e->dmalloc<unsigned>(1); e->d_err = e->dmalloc<unsigned>(1);
    e->d_ptrace = e->dmalloc<u64>((size_t)PS_CUS * (PS_TRACE_EVENTS + PS_TRACE2_EVENTS));
    HIP_CHECK(hipMemset(e->d_gran, 0, PG_TOTAL * sizeof(u64)));
    const unsigned one = 1u;
    HIP_CHECK(hipMemcpy(e->d_serial, &one, sizeof(unsigned), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(e->d_err, 0, sizeof(unsigned)));
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&e->h_err), sizeof(unsigned)));
}
void exp_upload_layers(ma_engine* e) {
    if (e->persist_shape) HIP_CHECK(hipMemcpy(e->d_layers, e->dl.data(), e->cfg.layers * sizeof(DecLayerPtrs), hipMemcpyHostToDevice));
}

// In-kernel timeline of ONE persistent decode step (ma_persist_trace)
void persist_trace(ma_engine* e, int kv_len, uint64_t* host_out, int32_t* n_events, hipStream_t s) {
    require_ready(e);
    if (!e->persist_shape) throw MaError(MA_ERR_STATE, "the persistent decode step is not available for this configuration / device");
    if (kv_len < e->T + 1 || kv_len + 16 > e->maxseq) throw MaError(MA_ERR_INVALID, "kv_len out of range");
    ensure_embtab(e, s);
    state_at(e, s, 1, kv_len);
    StepTimer none;
    for (int i = 0; i < 3; ++i) enqueue_persist_step(e, s, none);
    const size_t tr_words = (size_t)PS_CUS * (PS_TRACE_EVENTS + PS_TRACE2_EVENTS);
    HIP_CHECK(hipMemsetAsync(e->d_ptrace, 0, tr_words * sizeof(u64), s));
    enqueue_persist_step(e, s, none, e->d_ptrace);
    HIP_CHECK(hipMemcpyAsync(host_out, e->d_ptrace, tr_words * sizeof(u64), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    check_persist_error(e, s);
    *n_events = 2 * (6 * e->cfg.layers + 1) + 2;
}

}  // namespace
