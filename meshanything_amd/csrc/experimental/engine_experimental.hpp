// Host side of the measured-and-rejected decode-step forms (MA_EXPERIMENTAL=1 libraries only): the rows-looped two-launch layer
// (rows_fused.hpp), the layer-pair launch (layer_fused.hpp) and the persistent one-launch step (persist.hpp).  Included by
// engine_decode.hpp, which gives the product build one block of stubs instead; no includes of its own.  Like the product chains, every enqueue
// function takes the Step context of engine_decode.hpp and builds on its layer halves and argument makers.
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

// one layer as two launches that share ONE argument record: both trace slots are taken before either launch (a trace never runs with a filter)
void enqueue_layer_rows_fused(Step& p, int l, const float* x_in, const LnW& ln) {
    const ma_config& c = p.e->cfg;
    const int H = c.hidden;
    RowsFusedArgs A{};
    A.q = make_qkv_attn_args(p, l, x_in, ln);
    A.q.trace = p.tm.trace_slot(TK_ATTN, ATTN_NCHUNK * c.heads);
    A.o = make_oproj_fc1_args(p, l, ln.g ? p.h0 : x_in, true);
    A.o.trace = p.tm.trace_slot(TK_OPROJ, H / 4);
    A.part_gran = p.part_gran;
    A.attn_out = p.xb; A.attn_out_stride = H;
    A.B = p.rw.B;
    if (p.tm.on(CLS_ATTN)) launched(launch_qkv_attn_rows(A, c.heads, p.s), "qkv_attn_rows");
    if (p.tm.on(CLS_WEIGHTS)) launched(launch_oproj_fc1_rows(A, H, c.ffn, p.s), "oproj_fc1_rows");
}

bool fuse_layer(ma_engine* e, int B = 1, int len_override = -1) { return e->opt.fuse_layer && e->bf16 && e->hdt == MA_DTYPE_BF16 && fuse_qkv_attn(e, B, len_override) && fuse_oproj_fc1(e, B, len_override) && e->opt.fuse_fc2; }

// second half of layer l + first half of layer l + 1 in one launch (layer_fused.hpp); belongs to the attention class of the profiler
void enqueue_layer_pair(Step& p, int l, const float* resid) {
    const ma_config& c = p.e->cfg;
    if (!p.tm.on(CLS_ATTN)) return;
    LayerFusedArgs a{};
    a.o = make_oproj_fc1_args(p, l, resid, true);
    a.q = make_qkv_attn_args(p, l + 1, nullptr, p.ln2(l));
    a.gran3 = p.y2_gran;
    launched(launch_layer_fused(a, c.hidden, c.ffn, c.heads, p.rw.B, p.s), "layer_fused");
}
// first half of layer 0 | (second half of l + first half of l + 1) x (L - 1) | second half of layer L - 1 | lm_head
void enqueue_layer_pairs(Step& p) {
    const int L = p.e->cfg.layers;
    gemv_attn_half(p, 0, p.de, NO_LN);
    for (int l = 0; l + 1 < L; ++l) enqueue_layer_pair(p, l, l == 0 ? p.de : p.h0);
    gemv_mlp_half(p, L - 1, p.h0);
    p.lm_head(p.y2, p.H(), p.ln2(L - 1));
}

// ---- persistent decode step (persist.hpp) ----------------------------------------------------------------------------------
// eligible: bf16 policy, one row, greedy, the 350M layer shape, a device with exactly the 256 CUs the kernel assigns roles to
bool persist_eligible(ma_engine* e, int B, int do_sample) { return e->persist_shape && B == 1 && !do_sample; }
bool persist_selected(ma_engine* e, int B, int do_sample) { return e->opt.decode_impl == 1 && persist_eligible(e, B, do_sample); }

void enqueue_persist_step(Step& p, u64* trace = nullptr) {
    ma_engine* e = p.e;
    if (!p.tm.on(CLS_PERSIST)) return;
    const DecW& d = e->decw;
    PersistArgs a{};
    a.layers = e->d_layers; a.L = e->cfg.layers;
    a.lm_head = reinterpret_cast<const bf16_t*>(d.lm_head); a.V = e->V;
    a.embtab = e->d_embtab; a.extra = d.extra; a.tokpos = d.tokpos; a.cond = d.cond; a.postab = d.postab; a.T = e->T;
    a.kv = reinterpret_cast<bf16_t*>(e->kv); a.kv_plane = e->kv_plane / e->kv_elem; a.max_seq = e->maxseq;
    a.st = p.st; a.tokens_out = p.w_tokens; a.logits = p.logits;
    a.gran = e->d_gran; a.serial = e->d_serial; a.err = e->d_err; a.trace = trace;
    launched(launch_persist_decode(a, p.s), "persistent decode");
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

// ---- the parts of build_engine that exist for these forms only (called where the blocks stood, so the order of device allocations stays)
void exp_alloc_exchanges(ma_engine* e) {
    e->d_part_gran = e->xalloc<u64>((size_t)e->cfg.max_batch * (size_t)e->cfg.heads * ATTN_NCHUNK * RF_PART);
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
    e->d_gran = e->xalloc<u64>(PG_TOTAL, 0); e->d_serial = e->dmalloc<unsigned>(1); e->d_err = e->xalloc<unsigned>(1, 0);      // (zeroed once: the persistent step's exchanges are not reset per generation)
    e->d_ptrace = e->dmalloc<u64>((size_t)PS_CUS * (PS_TRACE_EVENTS + PS_TRACE2_EVENTS));
    const unsigned one = 1u;
    HIP_CHECK(hipMemcpy(e->d_serial, &one, sizeof(unsigned), hipMemcpyHostToDevice));
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
    Step p(e, s, none, Rows{0, 1});
    for (int i = 0; i < 3; ++i) enqueue_persist_step(p);
    const size_t tr_words = (size_t)PS_CUS * (PS_TRACE_EVENTS + PS_TRACE2_EVENTS);
    HIP_CHECK(hipMemsetAsync(e->d_ptrace, 0, tr_words * sizeof(u64), s));
    enqueue_persist_step(p, e->d_ptrace);
    HIP_CHECK(hipMemcpyAsync(host_out, e->d_ptrace, tr_words * sizeof(u64), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    check_persist_error(e, s);
    *n_events = 2 * (6 * e->cfg.layers + 1) + 2;
}

}  // namespace
