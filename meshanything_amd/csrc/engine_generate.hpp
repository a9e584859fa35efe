// generate(): state records and the per-generation reset of the exchange buffers (e->exchanges), prefill, bursts of decode steps, and the fall-back when an in-launch exchange times out. (No includes of its own: compiled only inside engine.hip, in its include order.)
#pragma once

namespace {

// state records of rows 0..B-1: identical except for the row id and the row's slice of the injected uniforms
void init_state(ma_engine* e, hipStream_t s, const ma_sample_cfg& sc, int B, int maxn) {
    DecState st{};
    st.t = 0; st.pos = e->T - 1; st.cur_tok = 0; st.finished = 0;
    st.suppress_eos = sc.suppress_eos; st.do_sample = sc.do_sample; st.top_k = sc.top_k; st.top_p = sc.top_p;
    st.seed = sc.seed; st.uniforms = sc.uniforms; st.row = 0; st.max_new = maxn;
    st.forced = reinterpret_cast<const long long*>(sc.forced_tokens); st.logits_out = sc.logits_out; st.logits_first = sc.logits_out ? sc.logits_first_step : 0;
    hipLaunchKernelGGL(init_state_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, s, e->d_st, st, B, e->V);
    HIP_CHECK(hipGetLastError());
    // the fused launches tag their in-launch exchanges with the cache position, which restarts here; and an error word left raised by a call that
    // threw before reading it must not make this generation's sweeps give up early (e->exchanges: filled by xalloc, engine_state.hpp)
    for (const Exchange& x : e->exchanges) HIP_CHECK(hipMemsetAsync(x.p, 0, x.reset_bytes, s));
}

ma_sample_cfg resolve_sample_cfg(ma_engine* e, const ma_sample_cfg* sc) {
    ma_sample_cfg r{};
    r.struct_size = sizeof(ma_sample_cfg);
    r.top_k = 50; r.top_p = 0.95f;
    if (sc) {
        if (sc->struct_size != (int32_t)sizeof(ma_sample_cfg)) throw MaError(MA_ERR_INVALID, "ma_sample_cfg.struct_size mismatch");
        r = *sc;
    }
    if (r.max_new_tokens <= 0 || r.max_new_tokens > e->maxnew) {
        if (r.max_new_tokens > e->maxnew) throw MaError(MA_ERR_INVALID, "max_new_tokens exceeds 9*n_max_faces+2");
        r.max_new_tokens = e->maxnew;
    }
    if (r.check_every <= 0) r.check_every = 64;
    if (!r.logits_out) r.logits_first_step = 0;                          // (no effect without logits_out: whatever the caller left there is ignored)
    else if (r.logits_first_step < 0 || r.logits_first_step >= r.max_new_tokens) throw MaError(MA_ERR_INVALID, "logits_first_step must be in [0, max_new_tokens) when logits_out is set");
    if (r.do_sample && (r.top_k < 1 || r.top_k > PICK_KMAX)) throw MaError(MA_ERR_INVALID, "top_k must be in [1,64]");
    if (r.do_sample && !(r.top_p > 0.f && r.top_p <= 1.f)) throw MaError(MA_ERR_INVALID, "top_p must be in (0,1]");
    return r;
}

// measurement entry points: the state as if kv_len - T tokens had been generated (eos suppressed) and the cache held kv_len - 1 rows
void state_at(ma_engine* e, hipStream_t s, int B, int kv_len) {
    ma_sample_cfg sc = resolve_sample_cfg(e, nullptr);
    sc.suppress_eos = 1;
    init_state(e, s, sc, B, e->maxnew);
    hipLaunchKernelGGL(set_pos_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, s, e->d_st, kv_len - e->T, kv_len - 1, 5, B);
    HIP_CHECK(hipGetLastError());
    // embed_table: no pick produced this state, so nothing wrote the layer-0 input of the step that follows: one embedding launch does
    // (ma_profile_decode, ma_trace_decode, ma_persist_trace all come through here; generate()'s first step is fed by the pick after the prefill)
    if (embed_from_table(e, B)) { StepTimer none; Step p(e, s, none, Rows{0, B}); enqueue_embed(p); }
}

// generate() for a batch of B rows: every row is prefilled, then all rows step together (they share the weight stream and
// the cache position) until every row has emitted eos or max_new_tokens ([3p] GenerationMixin: a finished row keeps
// stepping and emits pad).  tokens_out (B, maxnew) device; lengths host (B).  Returns the number of valid columns.
int generate_batch_once(ma_engine* e, hipStream_t s, const float* prefix, int B, const ma_sample_cfg& sc, long long* tokens_out, int32_t* lengths) {
    const int maxn = sc.max_new_tokens;
    const int total = B * e->maxnew;
    hipLaunchKernelGGL(fill_tokens_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, e->w_tokens, (long long)TOK_PAD, total);
    HIP_CHECK(hipGetLastError());
    // (the persistent step carries its own pick: teacher forcing / logits capture take the launch chain)
    const bool parity_aid = sc.forced_tokens || sc.logits_out;
    const int impl = (persist_selected(e, B, sc.do_sample) && !parity_aid) ? 1 : 0;
    if (impl == 1 || embed_from_table(e, B)) ensure_embtab(e, s);
    ensure_graphs(e, B, impl);
    init_state(e, s, sc, B, maxn);
    // prefill in groups of rows (bounded workspace: prefill_rows samples at a time)
    {
        RoctxRange range("ma_generate: prefill");
        for (int b0 = 0; b0 < B; b0 += e->prefill_rows) {
            const int nb = std::min(e->prefill_rows, B - b0);
            prefill(Dense{e, s, e->bf16}, prefix + (size_t)b0 * e->T * e->cfg.hidden, b0, nb);
        }
    }
    RoctxRange range_decode("ma_generate: decode steps");
    if (e->opt.prefill_stepwise) init_state(e, s, sc, B, maxn);         // the stepwise prefill used the state's pos field
    StepTimer none;
    // token 0 (expected bos; dropped later, meshanything.py:166); embed_table: this pick also writes the first decode step's layer-0 input
    Step all_rows(e, s, none, Rows{0, B});
    enqueue_pick(all_rows);
    int produced = 1;
    bool finished = false;
    while (produced < maxn && !finished) {
        // the first burst is ONE step: a grid whose blocks are not all resident (device shared with another stream / process) shows
        // in the error word after the first fused launch, not after 64 steps of zero-filled exchanges
        const int burst = std::min(produced == 1 ? 1 : sc.check_every, maxn - produced);
        launch_steps(e, s, B, impl, burst);
        produced += burst;
        HIP_CHECK(hipMemcpyAsync(e->h_state, e->d_st, (size_t)B * sizeof(DecState), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (impl == 1) check_persist_error(e, s);
        else check_chain_error(e, s);
        finished = true;
        for (int b = 0; b < B; ++b) finished = finished && e->h_state[b].finished != 0;
    }
    if (produced == 1 && impl == 0) check_chain_error(e, s);            // (no decode step ran: the prefill's own in-launch exchange -- gemm256.hpp LNF form -- is checked here)
    HIP_CHECK(hipMemcpyAsync(e->h_tokens, e->w_tokens, (size_t)total * sizeof(long long), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    int nmax = 0;
    for (int b = 0; b < B; ++b) {
        const long long* row = e->h_tokens + (size_t)b * e->maxnew;
        int len = produced;
        // (teacher forcing: the row reports the engine's picks along the GIVEN stream, every produced column counts)
        if (!sc.forced_tokens) for (int i = 0; i < produced; ++i) if (row[i] == TOK_EOS) { len = i + 1; break; }
        if (lengths) lengths[b] = len;
        nmax = std::max(nmax, len);
    }
    if (tokens_out != e->w_tokens) HIP_CHECK(hipMemcpyAsync(tokens_out, e->w_tokens, (size_t)total * sizeof(long long), hipMemcpyDeviceToDevice, s));
    return nmax;
}

// A timed-out in-launch exchange is not an error of the request: the fused launches need the whole grid resident, which another
// stream or process on the device can take away at any time.  The engine then stops using them (chain_resident = false: five
// launches per layer, no spinning, bit-identical results -- tests/test_gpu_persist.py) and runs the generation again from the prefill.
// One co-tenant blip must not cost the fused launches for the rest of the engine's life: after CHAIN_REARM_AFTER clean
// generations on the five-launch chain the engine re-arms them; if the device is still shared, the next generation pays one more
// 20 ms deadline and falls back again.  chain_fallbacks / xchg_timeouts (get_option) and the bench line show what happened.
constexpr int CHAIN_REARM_AFTER = 16;
int generate_batch(ma_engine* e, hipStream_t s, const float* prefix, int B, const ma_sample_cfg& sc, long long* tokens_out, int32_t* lengths) {
    if (!e->chain_resident && e->chain_fallbacks > 0 && e->resident_blocks * 4 >= 256L * 5 && ++e->gens_since_fallback > CHAIN_REARM_AFTER) {
        e->chain_resident = true; e->gens_since_fallback = 0;
        drop_graphs(e);
    }
    try {
        return generate_batch_once(e, s, prefix, B, sc, tokens_out, lengths);
    } catch (const ChainTimeout&) {
        if (!e->chain_resident) throw;
        e->chain_resident = false;
        e->chain_fallbacks++;
        e->gens_since_fallback = 0;
        drop_graphs(e);
    }
    return generate_batch_once(e, s, prefix, B, sc, tokens_out, lengths);
}

}  // namespace
