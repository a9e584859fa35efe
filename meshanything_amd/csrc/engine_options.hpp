// ma_engine_set_option / ma_engine_get_option: ONE table, one row per name, and the two functions that walk it.  This table is the list of
// option names: where a value lives, which values are accepted (and the message otherwise), what setting it invalidates, what reading it returns.
// (Like every engine_*.hpp: no includes of its own, compiled only inside engine.hip, after engine_state.hpp and engine_decode.hpp.)
#pragma once

namespace {

using Options = ma_engine::Options;
enum : unsigned { DROPS_GRAPHS = 1, CLEARS_EMBTAB = 2, RECOUNTS_PARTS = 4 };       // what a setter invalidates (captured steps embed grids and arguments)

// accepted values as a bit set
template <typename... A> constexpr uint32_t one_of(A... v) { return ((1u << v) | ...); }
constexpr uint32_t from_to(int lo, int hi) { uint32_t m = 0; for (int v = lo; v <= hi; ++v) m |= 1u << v; return m; }

struct Opt {
    const char* name;
    int Options::* field;                    // where the value lives: a member of ma_engine::opt ...
    void (*put)(ma_engine*, int64_t);        // ... or elsewhere (cfg, chain_resident); neither: read-only
    int64_t (*get)(ma_engine*);              // what is read back when that is not the stored value (elsewhere / effective / read-only)
    bool flag;                               // stored as value != 0
    uint32_t ok;                             // accepted values (0 = any), checked before `flag` is applied ...
    const char* bad;                         // ... and the MA_ERR_INVALID message for the others
    bool (*product)(int64_t);                // values a library without MA_EXPERIMENTAL takes (checked FIRST) ...
    const char* needs_exp;                   // ... and the MA_ERR_STATE message for the others
    void (*extra)(ma_engine*, int64_t);      // a check that needs the engine
    unsigned effects;
};

// device counters of the fused launches, never cleared (d_chain_err, build_engine): [1] sweeps that ever gave up | [3] blocks that lived > 1 ms | [2] the longest
// of them (ticks) | [4] scalar sweeps that a vector look had to finish | the first sweep that ever gave up: [5] its error bit, [6] blockIdx.x | y << 8 | z << 16 | wave << 24,
// [7] its polls | [8] sweeps that found 20 ms gone on the clock after a handful of polls (the wave was off the device: common.hpp xchg_expired) and went on
template <int I> int64_t chain_counter(ma_engine* e) {
    unsigned v[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(v, e->d_chain_err, sizeof(v), hipMemcpyDeviceToHost));
    return I == 2 ? v[2] / 100 : I == 5 ? (v[5] & 0x7fffffffu) : v[I];
}
bool zero_only(int64_t v) { return v == 0; }
#ifdef MA_EXPERIMENTAL
constexpr int64_t IS_EXPERIMENTAL = 1;
#else
constexpr int64_t IS_EXPERIMENTAL = 0;
#endif
#define MA_NEEDS_EXP " needs a library built with MA_EXPERIMENTAL=1 (the rejected decode-step forms are not part of the product build)"

const Opt OPTIONS[] = {
    // ---- dense phases
    {.name = "gemm_impl", .field = &Options::gemm_impl},
    {.name = "gemm_xcd_swizzle", .field = &Options::gemm_xcd_swizzle},
    {.name = "gemm256", .field = &Options::gemm256, .ok = from_to(0, 2), .bad = "gemm256: 0 (128-row tiles), 1 (one tile per workgroup) or 2 (1 + the persistent form)"},
    {.name = "gemm_variant", .field = &Options::gemm_variant, .product = [](int64_t v) { return v == 6; }, .needs_exp = "gemm_variant: the A/B tile variants need a library built with MA_EXPERIMENTAL=1"},
    {.name = "gemm_splitk", .field = &Options::gemm_splitk, .ok = from_to(0, 2), .bad = "gemm_splitk: 0 (never), 1 (fc2 of small prefills), 2 (+ out_proj)"},
    {.name = "attn_impl", .field = &Options::attn_impl, .ok = one_of(1, 2), .bad = "attn_impl: 1 (attn.hpp) or 2 (attn2.hpp)"},
    {.name = "qkv_to_cache", .field = &Options::qkv_to_cache, .flag = true},
    {.name = "prefill_tail", .field = &Options::prefill_tail, .ok = from_to(0, 2), .bad = "prefill_tail: 0 (one stream), 1 (the last rows as a chain on a second stream), 2 (... of the lowest priority)"},
    {.name = "prefill_stepwise", .field = &Options::prefill_stepwise},
    {.name = "fuse_ln", .field = &Options::fuse_ln, .get = [](ma_engine* e) -> int64_t { return e->opt.fuse_ln && e->chain_resident; }, .flag = true,
     .product = zero_only, .needs_exp = "fuse_ln needs a library built with MA_EXPERIMENTAL=1 (LayerNorm inside the GEMM epilogue: measured, not kept)"},
    // ---- decode step: how it is run
    {.name = "use_graph", .put = [](ma_engine* e, int64_t v) { e->cfg.use_graph = (int)v; }, .get = [](ma_engine* e) -> int64_t { return e->cfg.use_graph; }},
    {.name = "profile_batch", .field = &Options::profile_batch},
    {.name = "decode_impl", .field = &Options::decode_impl, .ok = one_of(0, 1), .bad = "decode_impl must be 0 (launch chain) or 1 (persistent step)", .product = zero_only, .needs_exp = "decode_impl" MA_NEEDS_EXP},
    // (the captured steps embed the fused 8-row launches, which rows_gates refuses beside a second row group); read back: effective, for profile_batch rows
    {.name = "decode_groups", .field = &Options::decode_groups, .get = [](ma_engine* e) -> int64_t { return decode_group_count(e, std::max(1, std::min(e->opt.profile_batch, e->cfg.max_batch)), 0); },
     .ok = from_to(1, 16), .bad = "decode_groups: 1 .. 16", .effects = DROPS_GRAPHS},
    // 0: never spin on other blocks (five-launch chain); 1: re-arm after a fallback, if the device allows
    {.name = "chain_resident", .put = [](ma_engine* e, int64_t v) { e->chain_resident = v != 0 && e->resident_blocks * 4 >= 256L * 5; },
     .get = [](ma_engine* e) -> int64_t { return e->chain_resident ? 1 : 0; }, .effects = DROPS_GRAPHS},
    // ---- decode step, GEMV chain
    {.name = "gemv_rpw", .field = &Options::gemv_rpw, .ok = one_of(1, 2, 4), .bad = "gemv_rpw must be 1, 2 or 4", .effects = DROPS_GRAPHS | RECOUNTS_PARTS},
    {.name = "gemv_small_rows", .field = &Options::gemv_small_rows, .ok = one_of(0, 1, 2, 4), .bad = "gemv_small_rows must be 0, 1, 2 or 4",
     .effects = DROPS_GRAPHS | CLEARS_EMBTAB},
    {.name = "gemv_k8_ksplit", .field = &Options::gemv_k8_ksplit, .ok = one_of(1, 2, 4), .bad = "gemv_k8_ksplit must be 1, 2 or 4", .effects = DROPS_GRAPHS},
    // (the fused launches are read back as the engine will apply them: option AND eligibility)
    {.name = "fuse_qkv_attn", .field = &Options::fuse_qkv_attn, .get = [](ma_engine* e) -> int64_t { return fuse_qkv_attn(e) ? 1 : 0; }, .flag = true, .effects = DROPS_GRAPHS},
    {.name = "fuse_oproj_fc1", .field = &Options::fuse_oproj_fc1, .get = [](ma_engine* e) -> int64_t { return fuse_oproj_fc1(e) ? 1 : 0; }, .flag = true, .effects = DROPS_GRAPHS},
    {.name = "fuse_fc2", .field = &Options::fuse_fc2, .effects = DROPS_GRAPHS},
    {.name = "qkv_xcd_local", .field = &Options::qkv_xcd_local, .flag = true, .effects = DROPS_GRAPHS},
    {.name = "oproj_fc1_sweep_waves", .field = &Options::oproj_fc1_sweep_waves, .ok = one_of(1, 2, 4), .bad = "oproj_fc1_sweep_waves must be 1, 2 or 4", .effects = DROPS_GRAPHS},
    // (read back as the engine will apply it at profile_batch rows: the matrix-core batches keep their embedding launch)
    {.name = "embed_table", .field = &Options::embed_table, .get = [](ma_engine* e) -> int64_t { return embed_from_table(e, std::max(1, std::min(e->opt.profile_batch, e->cfg.max_batch))) ? 1 : 0; },
     .flag = true, .effects = DROPS_GRAPHS},
    {.name = "fuse_layer", .field = &Options::fuse_layer, .get = [](ma_engine* e) -> int64_t { return fuse_layer(e) ? 1 : 0; }, .product = zero_only, .needs_exp = "fuse_layer" MA_NEEDS_EXP, .effects = DROPS_GRAPHS},
    // ---- decode step, matrix-core chain
    {.name = "mfma_min_batch", .field = &Options::mfma_min_batch, .effects = DROPS_GRAPHS},
    {.name = "mfma_chunks", .field = &Options::mfma_chunks, .ok = one_of(4, 8), .bad = "mfma_chunks must be 4 or 8", .effects = DROPS_GRAPHS},
    {.name = "mfma_fc2_ksplit", .field = &Options::mfma_fc2_ksplit, .ok = one_of(0, 1, 2, 4), .bad = "mfma_fc2_ksplit must be 0 (default), 1, 2 or 4",
     .extra = [](ma_engine* e, int64_t v) { if (v > 1 && e->cfg.ffn % (4 * (int)v * 32) != 0) throw MaError(MA_ERR_INVALID, "mfma_fc2_ksplit does not divide the ffn width"); }, .effects = DROPS_GRAPHS},
    {.name = "mfma_ln_waves", .field = &Options::mfma_ln_waves, .ok = one_of(0, 4, 8), .bad = "mfma_ln_waves must be 0 (by batch), 4 or 8", .effects = DROPS_GRAPHS},
    {.name = "mfma_fold_ln", .field = &Options::mfma_fold_ln, .effects = DROPS_GRAPHS},
    {.name = "mfma_fold_fc1_max", .field = &Options::mfma_fold_fc1_max, .effects = DROPS_GRAPHS},
    {.name = "mfma_fold_qkv_max", .field = &Options::mfma_fold_qkv_max, .effects = DROPS_GRAPHS},
    {.name = "attn_final_min_batch", .field = &Options::attn_final_min_batch, .effects = DROPS_GRAPHS},
    {.name = "attn_final_waves", .field = &Options::attn_final_waves, .ok = one_of(0, 4, 8, 16), .bad = "attn_final_waves: 0, 4, 8 or 16", .effects = DROPS_GRAPHS},
    {.name = "attn_rowwave", .field = &Options::attn_rowwave, .effects = DROPS_GRAPHS},
    {.name = "attn_pair", .field = &Options::attn_pair, .effects = DROPS_GRAPHS},
    // (the two 8-row launches are read back as the engine will apply them at 8 rows: the very gates of the step builder, rows_gates; the first half
    //  also needs its LayerNorm 2 folded in, or left by the previous layer's second half)
    {.name = "fuse_rows_attn", .field = &Options::fuse_rows_attn, .get = [](ma_engine* e) -> int64_t { const RowsGates rg = rows_gates(e, RA_ROWS, -1); return rg.attn && (rg.fold || (rg.mlp && e->opt.rows_mlp_ln2)); },
     .flag = true, .effects = DROPS_GRAPHS},
    {.name = "fuse_rows_mlp", .field = &Options::fuse_rows_mlp, .get = [](ma_engine* e) -> int64_t { return rows_gates(e, RA_ROWS, -1).mlp; }, .flag = true, .effects = DROPS_GRAPHS},
    // (the product refusal is checked first, so it lets the out-of-range values through: those are MA_ERR_INVALID in every library)
    {.name = "rows_attn_early", .field = &Options::rows_attn_early, .ok = from_to(0, 6), .bad = "rows_attn_early: 0 .. 6", .product = [](int64_t v) { return v < 0 || v > 6 || v == 3 || v == 5 || v == 6; },
     .needs_exp = "rows_attn_early: placements 0, 1, 2 and 4 need a library built with MA_EXPERIMENTAL=1 (measured, not kept)", .effects = DROPS_GRAPHS},
    {.name = "rows_mlp_ln2", .field = &Options::rows_mlp_ln2, .flag = true, .effects = DROPS_GRAPHS},
    {.name = "rows_mlp_prefetch", .field = &Options::rows_mlp_prefetch, .ok = from_to(0, 9), .bad = "rows_mlp_prefetch: 0 off, 1 / 2 rounds, 8 weights only, 9 half a round", .effects = DROPS_GRAPHS},
    {.name = "rows_fused", .field = &Options::rows_fused, .get = [](ma_engine* e) -> int64_t { return e->opt.rows_fused && e->rf_ok && e->chain_resident ? 1 : 0; }, .flag = true,
     .product = zero_only, .needs_exp = "rows_fused" MA_NEEDS_EXP, .effects = DROPS_GRAPHS},
    {.name = "rows_fused_min", .field = &Options::rows_fused_min, .effects = DROPS_GRAPHS},
    // ---- read-only: what the library and the device are, and the health counters
    {.name = "experimental", .get = [](ma_engine*) -> int64_t { return IS_EXPERIMENTAL; }},
    {.name = "persist_available", .get = [](ma_engine* e) -> int64_t { return e->persist_shape ? 1 : 0; }},
    {.name = "resident_blocks", .get = [](ma_engine* e) -> int64_t { return e->resident_blocks; }},
    {.name = "dense_rows", .get = [](ma_engine* e) -> int64_t { return e->dense_rows; }},
    {.name = "chain_fallbacks", .get = [](ma_engine* e) -> int64_t { return e->chain_fallbacks; }},
    {.name = "xchg_last_code", .get = [](ma_engine* e) -> int64_t { return e->xchg_last_code; }},
    {.name = "xchg_timeouts", .get = chain_counter<1>}, {.name = "slow_blocks", .get = chain_counter<3>}, {.name = "slow_block_max_us", .get = chain_counter<2>},
    {.name = "scalar_sweep_rescues", .get = chain_counter<4>}, {.name = "xchg_first_giveup_code", .get = chain_counter<5>}, {.name = "xchg_first_giveup_block", .get = chain_counter<6>},
    {.name = "xchg_first_giveup_polls", .get = chain_counter<7>}, {.name = "xchg_descheduled", .get = chain_counter<8>},
};
#undef MA_NEEDS_EXP

const Opt& find_option(const std::string& n, bool to_set) {
    for (const Opt& o : OPTIONS) if (n == o.name && (!to_set || o.field || o.put)) return o;
    throw MaError(MA_ERR_INVALID, "unknown option " + n);
}

// the refusals that need no engine (also those of ma_op_gemm_bf16_tuned's two switches)
void check_value(const Opt& o, int64_t value) {
    if (!IS_EXPERIMENTAL && o.product && !o.product(value)) throw MaError(MA_ERR_STATE, o.needs_exp);
    if (o.ok && (value < 0 || value > 31 || !(o.ok >> value & 1u))) throw MaError(MA_ERR_INVALID, o.bad);
}

void set_option(ma_engine* e, const std::string& n, int64_t value) {
    const Opt& o = find_option(n, true);
    check_value(o, value);
    if (o.extra) o.extra(e, value);
    const int64_t v = o.flag ? (value != 0) : value;
    if (o.put) o.put(e, v); else e->opt.*(o.field) = (int)v;
    if (o.effects & RECOUNTS_PARTS) e->n_parts = gemv_blocks(e, e->V, e->cfg.hidden);
    if (o.effects & CLEARS_EMBTAB) e->embtab_ready = false;
    if (o.effects & DROPS_GRAPHS) drop_graphs(e);          // the next generate() captures the step again
}

int64_t get_option(ma_engine* e, const std::string& n) {
    const Opt& o = find_option(n, false);
    return o.get ? o.get(e) : e->opt.*(o.field);
}

}  // namespace
