"""The case table of tests/test_gpu_step_forms.py: every non-default value of a decode-step (or prefill) tuning switch that a product build accepts,
with the batch size at which it selects another kernel form, the options it needs beside it, and how its logits relate to the baseline's.

A plain module (no torch, no GPU): tests/test_step_forms_host.py reads it to check that every name of csrc/engine_options.hpp is either the
switch of a case here or listed in EXEMPT with the reason.

Relations (the baseline = same batch, same prerequisites, the switch at its default):
  IDENTICAL   the form moves work between waves, blocks or launches and keeps the order of every sum: the logits of all 257 steps are
              bit-equal to the baseline's.
  REORDERED   the form splits or orders a sum differently: held to the reference's logits only (as the baseline is), and it must be seen to
              be another form (launch list, launch counts, or a bit of the logits).
The one-line reason next to each row is the place in the kernels that the relation was read from."""
from collections import namedtuple

IDENTICAL, REORDERED = "identical", "reordered"
BF16_FP16 = ("bf16", "fp16")

# prereq / switch: ((name, value), ...) in the order they are set.  needs_fused: the form (or its baseline) runs launches with in-launch
# exchanges; skipped where the device cannot hold their grids (chain_resident == 0 from the start), like tests/test_gpu_rows_attn.py.
Case = namedtuple("Case", "id policies B prereq switch relation needs_fused reason")

CASES = []


def _case(B, prereq, switch, relation, reason, policies=BF16_FP16, needs_fused=False):
    cid = f"b{B}-" + ("+".join(f"{k}={v}" for k, v in prereq) + "," if prereq else "") + "+".join(f"{k}={v}" for k, v in switch)
    if tuple(policies) != BF16_FP16:
        cid += "@" + "+".join(policies)
    CASES.append(Case(cid, tuple(policies), B, tuple(prereq), tuple(switch), relation, needs_fused, reason))


# ---- GEMV chain, batch 1 (gemv.hpp: gemv_shape picks gemv_kernel<WT, KSPLIT, LPL, RPW>) ------------------------------------------------------
for v in (1, 2):
    _case(1, (), (("gemv_rpw", v),), IDENTICAL, "lm_head (8195 x 1024, 16-bit) goes from <1, 2, 4> to <1, 2, 2>: 1025 blocks instead of 513, a wave still "
          "owns whole rows (same fmaf order, same wave_sum); n_parts follows")
# fp32 (4-byte weights: 4 pieces per row): lm_head is <2, 2, 2> whatever gemv_rpw says (N > 4096), and the fused launches take no GemvTune, so
# the switch is live only on the five-launch chain, where q/k/v (3072 rows) and fc1 (4096 rows) go from <2, 2, 2> to <2, 2, 1>.
_case(1, (("fuse_qkv_attn", 0), ("fuse_oproj_fc1", 0)), (("gemv_rpw", 1),), IDENTICAL, "fp32: q/k/v and fc1 go from <2, 2, 2> to <2, 2, 1> (1536 / 2048 blocks): "
      "the two waves of a group split K the same way, one row per group instead of two", policies=("fp32",))
_case(1, (("fuse_qkv_attn", 0), ("fuse_oproj_fc1", 0)), (("gemv_rpw", 2),), IDENTICAL, "fp32: gemv_shape gives rpw > 2 ? 2 : rpw for 4-piece rows: the value 2 "
      "selects the instantiations of the default 4 in every launch (listed in NOTHING_MOVES)", policies=("fp32",))
for v, rel, why in ((0, REORDERED, "<2, 1, 1>: two waves split K and meet in LDS (red[])"), (2, IDENTICAL, "<1, 2, 2>: whole rows per wave, 128 blocks"),
                    (4, IDENTICAL, "<1, 2, 4>: whole rows per wave, 64 blocks")):
    _case(1, (("fuse_oproj_fc1", 0),), (("gemv_small_rows", v),), rel, "out_proj (1024 x 1024, merge of the attention partials in front) as " + why)
    _case(1, (("embed_table", 0),), (("gemv_small_rows", v),), rel, "the embedding launch (1024 x 1024, EPI_EMBED) as " + why)
    # the setter clears the table (CLEARS_EMBTAB); ensure_embtab rebuilds it with the instantiation the embedding launch would use
    _case(1, (("gemv_small_rows", v),), (("embed_table", 0),), IDENTICAL, "embedding launch against the table that ensure_embtab rebuilt after the setter "
          "cleared it: the same gemv_kernel instantiation, codebook rows as batch rows")
for v in (2, 4):
    _case(1, (("fuse_fc2", 0),), (("gemv_k8_ksplit", v),), REORDERED, f"fc2 (1024 x 4096) as <{v}, {8 // v}, 1>: {v} waves split K and meet in LDS, {256 * v} blocks",
          needs_fused=True)
for v in (1, 2):
    _case(1, (("fuse_fc2", 0),), (("oproj_fc1_sweep_waves", v),), IDENTICAL, f"oproj_fc1_kernel<{v}, false>: {v} wave(s) poll the y1 granules (16 / NSW per lane and "
          "pass); what they gather and every sum behind it are the same (ignored while fc2 is fused: launch_oproj_fc1)", needs_fused=True)
_case(1, (), (("qkv_xcd_local", 0),), IDENTICAL, "qkv_block_role: (chunk, head) of a block is a bijection of blockIdx either way; the exchange does not care "
      "where a block runs", needs_fused=True)
# two rows: all five GEMV launches per layer (the fused launches hold one row's grid on a 256-CU device; switched off so that it holds anywhere)
_case(2, (("fuse_qkv_attn", 0), ("fuse_oproj_fc1", 0)), (("gemv_small_rows", 2), ("gemv_k8_ksplit", 4)), REORDERED,
      "rows in grid.y: out_proj <1, 2, 2> (same sums) and fc2 <4, 2, 1> (K split over four waves)")

# ---- matrix-core chain (gemm_decode.hpp, attn_decode.hpp, rows_attn.hpp, rows_mlp.hpp; the step builder: engine_decode.hpp) ------------------------
_case(4, (), (("mfma_ln_waves", 4),), REORDERED, "gemm_dec_ln_kernel<.., 4> for <= 8 rows: four waves split K = 1024 (red[4]) instead of eight")
_case(4, (), (("attn_rowwave", 0),), REORDERED, "attn_decode_kernel<KT, false>: the four waves of a block split one (row, head, chunk) and merge, instead of a "
      "(row, head, chunk) per wave; a quarter of the rows per block")
_case(4, (), (("mfma_fold_ln", 0),), REORDERED, "both LayerNorms in rows_prologue launches (block-level sums) and out_proj split four ways along K")
_case(4, (), (("mfma_fold_fc1_max", 0),), REORDERED, "LayerNorm 1 in a rows_prologue launch, out_proj split four ways along K (ks_o follows fold1)")
_case(4, (), (("mfma_fold_qkv_max", 0),), REORDERED, "LayerNorm 2 in a rows_prologue launch in front of q/k/v (block-level sums instead of one wave's)")
for v in (1, 2, 5, 8, 9):
    _case(8, (), (("rows_mlp_prefetch", v),), IDENTICAL, "rows_mlp.hpp step F: the 248 idle blocks only request the next launch's operands (xor into a sink "
          "that is never written); rounds past the cache are clamped to position 0", needs_fused=True)
_case(8, (), (("attn_pair", 0),), REORDERED, "pair_ok off: five launches per layer, attn_decode_final_kernel<KT, 8, false> (one block per (row, head)) instead of the "
      "two-block form inside rows_attn", needs_fused=True)
for v in (4, 16):
    _case(8, (("attn_pair", 0),), (("attn_final_waves", v),), REORDERED, f"attn_decode_final_kernel<KT, {v}, false>: {v} waves split the positions of a (row, head)")
_case(8, (), (("attn_final_min_batch", 1000),), REORDERED, "split-KV attn_decode + the PRO_ATTN rows_prologue merge instead of the final form; the fused first half "
      "drops out (rows_gates)", needs_fused=True)
for v in (1, 2):
    _case(8, (), (("mfma_fc2_ksplit", v),), REORDERED, f"fc2 over {v} block(s) along K instead of 4; rows_gates needs ks_f == 4, so the fused MLP half drops out",
          needs_fused=True)
_case(16, (), (("mfma_fold_fc1_max", 16), ("mfma_fold_qkv_max", 16)), REORDERED, "12 .. 16 rows with both LayerNorms inside gemm_dec_ln_kernel<.., 4> (rows w, w + 4 and "
      "the one-at-a-time tail), out_proj not split")
_case(16, (("mfma_fold_fc1_max", 16), ("mfma_fold_qkv_max", 16)), (("mfma_ln_waves", 8),), REORDERED, "gemm_dec_ln_kernel<.., 8> above 8 rows: rows 8 .. 15 in its "
      "`r += NW` tail, K split over eight waves")
for v in (8, 16):
    _case(16, (), (("attn_final_waves", v),), REORDERED, f"attn_decode_final_kernel<KT, {v}, false> instead of the 4 waves that 12 rows and more get")
for B in (40, 64):
    _case(B, (), (("mfma_chunks", 4),), IDENTICAL, f"gemm_dec_kernel<{(B + 15) // 16}, 4>: a wave's 256-wide k-range in two rounds of four loads; the MFMA sequence "
          "per accumulator walks k in the same order")

# ---- prefill, batch 1 (engine_dense.hpp) -----------------------------------------------------------------------------------------------------
_case(1, (), (("attn_impl", 1),), REORDERED, "attn.hpp instead of attn2.hpp for the prefix's causal attention", policies=("bf16",))
_case(1, (), (("attn_impl", 1),), IDENTICAL, "the first-generation kernel is bf16 only: a fp16 engine keeps attn2.hpp (listed in NOTHING_MOVES)", policies=("fp16",))
_case(1, (), (("gemm_xcd_swizzle", 0),), IDENTICAL, "gemm_tile.hpp: which workgroup takes which tile; a tile's arithmetic does not depend on it")

# Switches that decide only WHEN or WHERE bytes move and keep every grid: nothing observable tells their forms apart, so instead of a difference the
# test asserts the gate that makes the switch live.  name: ((option, read-back value), ...) that must hold while the form runs.
PLACEMENT_ONLY = {
    "oproj_fc1_sweep_waves": (("fuse_oproj_fc1", 1), ("fuse_fc2", 0)),
    "qkv_xcd_local": (("fuse_qkv_attn", 1),),
    "rows_mlp_prefetch": (("fuse_rows_attn", 1), ("fuse_rows_mlp", 1), ("rows_mlp_ln2", 1)),
    "mfma_chunks": (("mfma_min_batch", 4),),                 # (and 33 .. 64 rows: asserted from the case's batch)
    "gemm_xcd_swizzle": (),                                  # (a 16-bit policy: asserted from the case's policy)
}

# (policy, switch, value) at which NOTHING observable moves at this shape, with the reason read from the code.  The test then asserts exactly that
# (same launch list, same counts, every bit), so that a change which makes the value visible fails here and the entry goes.  Part a still holds.
NOTHING_MOVES = {
    # the value selects the default's own kernels
    ("fp32", "gemv_rpw", 2): "gemv_shape: 4-piece rows (fp32, K = 1024) take rpw > 2 ? 2 : rpw, and lm_head <2, 2, 2> above 4096 rows",
    ("fp16", "attn_impl", 1): "engine_dense.hpp: the first-generation attention kernel is bf16 only, a fp16 engine runs attn2.hpp for both values",
    # another kernel and another grid (not traced: the matrix-core chain's attention launches take no trace slot), the same arithmetic up to a cache of
    # 512 positions: a chunk (1/16 of the cache) then fits wave 0's 32 positions, the waves 1 .. 3 publish empty states (m = -1e30, l = 0) and the
    # block merge multiplies wave 0's state by exp(0) and theirs by exp(-1e30 - M) = 0.  The path ends at 514 positions: only its last two steps give
    # wave 1 one position per chunk.  fp16 shows that in a bit of the logits (the same row passes part c there); bf16's rounding of the attention
    # output swallows it with these weights.
    ("bf16", "attn_rowwave", 0): "attn_decode_kernel<KT, false> == <KT, true> in arithmetic while a chunk holds <= 32 positions (cache <= 512)",
}

# Every other name of the option table, with the reason why it has no row above.
EXEMPT = {
    "gemm_impl": "fp32 dense GEMM form (mfma / valu): both pinned at kernel level in test_gpu_kernels.py::test_gemm",
    "gemm256": "dense GEMM tile forms: against fp64 in test_gpu_gemm_forms.py, against each other in test_gpu_pipeline.py",
    "gemm_variant": "experimental only (the product build accepts the default alone)",
    "gemm_splitk": "split along K: against fp64 in test_gpu_gemm_forms.py, prefill with and without it in test_gpu_pipeline.py",
    "qkv_to_cache": "pinned bit for bit in test_gpu_pipeline.py (prefill forms)",
    "prefill_tail": "pinned bit for bit in test_gpu_pipeline.py (prefill forms)",
    "prefill_stepwise": "pinned in test_gpu_pipeline.py (prefill by decode steps)",
    "fuse_ln": "experimental only",
    "use_graph": "eager launches == graph replay: test_gpu_rows_attn.py, test_gpu_options.py",
    "profile_batch": "selects the batch that profile_decode / trace_decode measure; no kernel form",
    "decode_impl": "experimental only",
    "decode_groups": "row groups reproduce the ungrouped run bit for bit: test_gpu_pipeline.py",
    "chain_resident": "the fall-back chain: test_gpu_persist.py, test_gpu_rows_attn.py (*falls_back*)",
    "fuse_qkv_attn": "fused against unfused: test_gpu_persist.py; a prerequisite of rows here",
    "fuse_oproj_fc1": "fused against unfused: test_gpu_persist.py; a prerequisite of rows here",
    "fuse_fc2": "fused against unfused: test_gpu_persist.py; a prerequisite of rows here",
    "fuse_layer": "experimental only",
    "mfma_min_batch": "GEMV chain against matrix-core chain: test_gpu_pipeline.py, test_gpu_options.py",
    "fuse_rows_attn": "pinned bit for bit in test_gpu_rows_attn.py",
    "fuse_rows_mlp": "pinned bit for bit in test_gpu_rows_attn.py",
    "rows_attn_early": "pinned bit for bit in test_gpu_rows_attn.py",
    "rows_mlp_ln2": "pinned bit for bit in test_gpu_rows_attn.py",
    "rows_fused": "experimental only",
    "rows_fused_min": "experimental only (read by the rows_fused step alone)",
    "experimental": "read-only", "persist_available": "read-only", "resident_blocks": "read-only", "dense_rows": "read-only",
    "chain_fallbacks": "read-only", "xchg_last_code": "read-only", "xchg_timeouts": "read-only", "slow_blocks": "read-only",
    "slow_block_max_us": "read-only", "scalar_sweep_rescues": "read-only", "xchg_first_giveup_code": "read-only",
    "xchg_first_giveup_block": "read-only", "xchg_first_giveup_polls": "read-only", "xchg_descheduled": "read-only",
}


def covered(cases=None):
    """Names that are the switch of at least one case (a prerequisite does not count: its own numbers are not what the case is about)."""
    return {k for c in (CASES if cases is None else cases) for k, _ in c.switch}


def uncovered(option_names, cases=None, exempt=None):
    """Names of the option table that neither a case nor EXEMPT accounts for."""
    have = covered(cases) | set(EXEMPT if exempt is None else exempt)
    return sorted(n for n in option_names if n not in have)
