"""ma_engine_set_option / ma_engine_get_option, name by name (csrc/engine_options.hpp holds the table): defaults, accepted values and what
is read back, refused values with their error code and message, read-only names, the values that need an MA_EXPERIMENTAL library, and that
a setter which invalidates the captured decode steps makes the next generation capture them again."""
import pytest
import torch

from meshanything_amd._lib import MAError
from meshanything_amd.config import MAConfig, DTYPE_BF16
from conftest import cached_state_dict, load_weights_cached, mouse_variants
from test_gpu_pipeline import GREEDY_TOL

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -3
NEEDS_EXP = " needs a library built with MA_EXPERIMENTAL=1 (the rejected decode-step forms are not part of the product build)"

# name: (default, values stored as given)                      -- no range check
PLAIN = {"mfma_min_batch": (4, (1, 65, 4)), "attn_final_min_batch": (8, (0, 12, 8)), "attn_rowwave": (1, (0, 1)), "mfma_fold_ln": (1, (0, 1)),
         "attn_pair": (1, (0, 1)), "mfma_fold_fc1_max": (8, (0, 16, 8)), "mfma_fold_qkv_max": (8, (0, 16, 8)),
         "fuse_fc2": (1, (0, 1)), "rows_fused_min": (4, (2, 8, 4)), "gemm_xcd_swizzle": (1, (0, 1)), "use_graph": (1, (0, 1))}
# name: (default, accepted values, one refused value on each side, message)      -- a documented list or range; the last accepted value is the default
LISTED = {"mfma_fc2_ksplit": (0, (1, 2, 0), (-1, 3), "mfma_fc2_ksplit must be 0 (default), 1, 2 or 4"),
          "mfma_chunks": (8, (4, 8), (3, 9), "mfma_chunks must be 4 or 8"),
          "mfma_ln_waves": (0, (4, 8, 0), (-1, 9), "mfma_ln_waves must be 0 (by batch), 4 or 8"),
          "rows_mlp_prefetch": (0, (1, 2, 3, 4, 5, 6, 7, 8, 9, 0), (-1, 10), "rows_mlp_prefetch: 0 off, 1 / 2 rounds, 8 weights only, 9 half a round"),
          "attn_final_waves": (0, (4, 8, 16, 0), (-1, 17), "attn_final_waves: 0, 4, 8 or 16"),
          "prefill_tail": (2, (0, 1, 2), (-1, 3), "prefill_tail: 0 (one stream), 1 (the last rows as a chain on a second stream), 2 (... of the lowest priority)"),
          "gemm_splitk": (2, (0, 1, 2), (-1, 3), "gemm_splitk: 0 (never), 1 (fc2 of small prefills), 2 (+ out_proj)"),
          "gemm256": (2, (0, 1, 2), (-1, 3), "gemm256: 0 (128-row tiles), 1 (one tile per workgroup) or 2 (1 + the persistent form)"),
          "attn_impl": (2, (1, 2), (0, 3), "attn_impl: 1 (attn.hpp) or 2 (attn2.hpp)"),
          "gemv_rpw": (4, (1, 2, 4), (0, 3), "gemv_rpw must be 1, 2 or 4"),
          "gemv_small_rows": (1, (0, 2, 4, 1), (-1, 3), "gemv_small_rows must be 0, 1, 2 or 4"),
          "gemv_k8_ksplit": (1, (2, 4, 1), (0, 3), "gemv_k8_ksplit must be 1, 2 or 4"),
          "oproj_fc1_sweep_waves": (4, (1, 2, 4), (0, 5), "oproj_fc1_sweep_waves must be 1, 2 or 4")}
# can be set, and the parent cannot read them back (a library that can returns the stored value): name: (accepted, refused, message)
WRITE_ONLY = {"gemm_impl": ((1, 0), (), ""), "prefill_stepwise": ((1, 0), (), ""), "profile_batch": ((8, 1), (), "")}
# stored as value != 0, read back as stored
FLAGS = {"rows_mlp_ln2": 1, "qkv_xcd_local": 1, "qkv_to_cache": 1}
# stored as value != 0 (default 1), read back as the engine will apply them: option AND eligibility
EFFECTIVE = ("fuse_qkv_attn", "fuse_oproj_fc1", "fuse_rows_attn", "fuse_rows_mlp")
READ_ONLY = ("experimental", "persist_available", "chain_fallbacks", "xchg_last_code", "xchg_timeouts", "slow_blocks", "slow_block_max_us",
             "scalar_sweep_rescues", "xchg_first_giveup_code", "xchg_first_giveup_block", "xchg_first_giveup_polls", "xchg_descheduled",
             "resident_blocks", "dense_rows")


@pytest.fixture(scope="module")
def tiny():
    from meshanything_amd.engine import Engine
    cfg = MAConfig.tiny(dtype=DTYPE_BF16, max_batch=16)
    eng = Engine(cfg)
    eng.cfg = cfg
    try:
        yield eng
    finally:
        eng.close()


@pytest.fixture(scope="module")
def full8():
    """The 350M shape at 8 rows, the shape on which the fused launches are eligible (options need no weights: the last test loads them)."""
    from meshanything_amd.engine import Engine
    eng = Engine(MAConfig.full(dtype=DTYPE_BF16, max_batch=8))
    eng.cfg = MAConfig.full(dtype=DTYPE_BF16, max_batch=8)
    try:
        yield eng
    finally:
        eng.close()


def _refused(eng, name, value, code, msg):
    with pytest.raises(MAError) as ei:
        eng.set_option(name, value)
    assert ei.value.code == code and msg in str(ei.value), (name, value, str(ei.value))


def _unknown(eng, call, name):
    with pytest.raises(MAError) as ei:
        call()
    assert ei.value.code == INVALID and ("unknown option " + name) in str(ei.value), (name, str(ei.value))


def _decisive(logits, tol):
    """(rows, steps) bool: the steps at which the run's own top-1 / top-2 logit margin (eos suppressed) exceeds 2 x tol."""
    lg = logits.clone()
    lg[:, :, 1] = float("-inf")
    top2 = torch.topk(lg, 2, dim=-1).values
    return ((top2[..., 0] - top2[..., 1]) > 2 * tol).cpu()


def _agrees_where_decisive(eng, prefix, want, decisive, what, **kw):
    """A form that orders a sum differently (same_there=False below) may leave the default's stream at a near-tie, so its free-running tokens are only
    checked for their shape; its NUMBERS are held to the reference's logits in tests/test_gpu_step_forms.py.  Here: walked along the default run's
    stream (teacher forcing, so that every step has the default's context), its own pick is the default's at every step where the default run's
    margin is decisive."""
    picks, _ = eng.generate(prefix, suppress_eos=True, forced_tokens=want, **kw)
    picks = picks.cpu()
    assert picks.shape == want.shape and bool(decisive.any()), what
    bad = (picks != want) & decisive
    print(f"[options] {what}: {int(decisive.sum())} of {decisive.numel()} steps decisive, picks differ from the default's at {int((picks != want).sum())} steps")
    assert not bool(bad.any()), (what, "picks differ from the default's at decisive steps (row, step)", bad.nonzero().tolist()[:8])


def test_defaults_values_and_refusals(tiny):
    eng = tiny
    exp = eng.get_option("experimental")
    assert exp in (0, 1)
    for name, (default, values) in PLAIN.items():
        assert eng.get_option(name) == default, name
        for v in values + (default,):
            eng.set_option(name, v)
            assert eng.get_option(name) == v, (name, v)
    for name, (default, values, bad, msg) in LISTED.items():
        assert eng.get_option(name) == default, name
        for v in bad:
            _refused(eng, name, v, INVALID, msg)
            assert eng.get_option(name) == default, (name, v)
        for v in values:
            eng.set_option(name, v)
            assert eng.get_option(name) == v, (name, v)
    # (a split of fc2 along K must divide the ffn width into whole 128-column pieces: 4 does not at this shape's 256)
    assert tiny.cfg.ffn % (4 * 4 * 32) != 0
    _refused(eng, "mfma_fc2_ksplit", 4, INVALID, "mfma_fc2_ksplit does not divide the ffn width")
    for name, (values, bad, msg) in WRITE_ONLY.items():
        for v in bad:
            _refused(eng, name, v, INVALID, msg)
        for v in values:
            eng.set_option(name, v)
            try:
                got = eng.get_option(name)
            except MAError as e:
                assert e.code == INVALID and ("unknown option " + name) in str(e)
            else:
                assert got == v, (name, v)
    for name, default in FLAGS.items():
        assert eng.get_option(name) == default, name
        for v, want in ((0, 0), (2, 1), (-1, 1), (1, 1)):
            eng.set_option(name, v)
            assert eng.get_option(name) == want, (name, v)
    # decode_groups: read back as the number of groups a batch of profile_batch rows is cut into (every group keeps >= 4 rows)
    assert eng.get_option("decode_groups") == 1
    for v in (0, 17):
        _refused(eng, "decode_groups", v, INVALID, "decode_groups: 1 .. 16")
    eng.set_option("profile_batch", 16)
    for v in range(1, 17):
        eng.set_option("decode_groups", v)
        assert eng.get_option("decode_groups") == min(v, 4), v
    eng.set_option("profile_batch", 1)
    assert eng.get_option("decode_groups") == 1
    eng.set_option("decode_groups", 1)
    # rows_attn_early: 0 .. 6; the placements that were measured and not kept live in MA_EXPERIMENTAL libraries only
    assert eng.get_option("rows_attn_early") == 6
    for v in (-1, 7):
        _refused(eng, "rows_attn_early", v, INVALID, "rows_attn_early: 0 .. 6")
    for v in (0, 1, 2, 3, 4, 5, 6):
        if not exp and v in (0, 1, 2, 4):
            _refused(eng, "rows_attn_early", v, STATE, "rows_attn_early: placements 0, 1, 2 and 4 need a library built with MA_EXPERIMENTAL=1 (measured, not kept)")
            continue
        eng.set_option("rows_attn_early", v)
        assert eng.get_option("rows_attn_early") == v
    # gemm_variant: any value in an MA_EXPERIMENTAL library, 6 (the default) otherwise
    assert eng.get_option("gemm_variant") == 6
    for v in (5, 7, 0):
        if exp:
            eng.set_option("gemm_variant", v)
            assert eng.get_option("gemm_variant") == v
        else:
            _refused(eng, "gemm_variant", v, STATE, "gemm_variant: the A/B tile variants need a library built with MA_EXPERIMENTAL=1")
    eng.set_option("gemm_variant", 6)
    assert eng.get_option("gemm_variant") == 6
    # the rejected decode-step forms
    assert eng.get_option("decode_impl") == 0 and eng.get_option("rows_fused") == 0 and eng.get_option("fuse_layer") == 0 and eng.get_option("fuse_ln") == 0
    for name in ("rows_fused", "fuse_layer", "decode_impl", "fuse_ln"):
        eng.set_option(name, 0)
        assert eng.get_option(name) == 0
    if exp:
        _refused(eng, "decode_impl", 2, INVALID, "decode_impl must be 0 (launch chain) or 1 (persistent step)")
        _refused(eng, "decode_impl", -1, INVALID, "decode_impl must be 0 (launch chain) or 1 (persistent step)")
        eng.set_option("decode_impl", 1)
        assert eng.get_option("decode_impl") == 1
        eng.set_option("decode_impl", 0)
    else:
        for name in ("rows_fused", "fuse_layer", "decode_impl"):
            for v in (1, -1, 2):
                _refused(eng, name, v, STATE, name + NEEDS_EXP)
        for v in (1, -1):
            _refused(eng, "fuse_ln", v, STATE, "fuse_ln needs a library built with MA_EXPERIMENTAL=1 (LayerNorm inside the GEMM epilogue: measured, not kept)")
    # chain_resident: 0 switches the in-launch exchanges off; non-zero arms them where the device can hold the fused grids
    can = 1 if eng.get_option("resident_blocks") * 4 >= 256 * 5 else 0
    assert eng.get_option("chain_resident") == can
    for v, want in ((0, 0), (1, can), (5, can)):
        eng.set_option("chain_resident", v)
        assert eng.get_option("chain_resident") == want
    # names nobody knows, names that can only be read
    _unknown(eng, lambda: eng.set_option("no_such_option", 1), "no_such_option")
    _unknown(eng, lambda: eng.get_option("no_such_option"), "no_such_option")
    for name in READ_ONLY:
        before = eng.get_option(name)
        _unknown(eng, lambda: eng.set_option(name, 1), name)
        assert eng.get_option(name) == before, name
    assert eng.get_option("dense_rows") == 16 and eng.get_option("chain_fallbacks") == 0 and eng.get_option("xchg_timeouts") == 0


def test_effective_values_at_the_350m_shape(full8):
    """The four fused launches are read back as the engine will apply them: the stored flag (value != 0) AND the gates of the step builder."""
    eng = full8
    on = {name: eng.get_option(name) for name in EFFECTIVE}
    if eng.get_option("chain_resident") == 1:
        assert on["fuse_qkv_attn"] == 1 and on["fuse_oproj_fc1"] == 1
    assert on["fuse_rows_attn"] in (0, 1) and on["fuse_rows_mlp"] in (0, 1)
    for name in EFFECTIVE:
        eng.set_option(name, 0)
        assert eng.get_option(name) == 0, name
        for v in (2, -1, 1):                                    # any non-zero value is the default again
            eng.set_option(name, v)
            assert {n: eng.get_option(n) for n in EFFECTIVE} == on, (name, v)
    # the gates follow the other switches: without in-launch exchanges nothing is fused; a second row group, or fc2 not split four ways, un-fuses the 8-row launches
    eng.set_option("chain_resident", 0)
    assert all(eng.get_option(n) == 0 for n in EFFECTIVE)
    eng.set_option("chain_resident", 1)
    assert {n: eng.get_option(n) for n in EFFECTIVE} == on
    eng.set_option("decode_groups", 2)
    assert eng.get_option("fuse_rows_attn") == 0 and eng.get_option("fuse_rows_mlp") == 0
    eng.set_option("decode_groups", 1)
    eng.set_option("mfma_fc2_ksplit", 2)
    assert eng.get_option("fuse_rows_mlp") == 0
    eng.set_option("mfma_fc2_ksplit", 4)                        # (4096 columns: 4 divides them)
    assert eng.get_option("mfma_fc2_ksplit") == 4
    eng.set_option("mfma_fc2_ksplit", 0)
    assert {n: eng.get_option(n) for n in EFFECTIVE} == on
    assert eng.get_option("dense_rows") == 8 and eng.get_option("persist_available") in (0, 1)


def test_setters_drop_the_captured_steps(tiny):
    """generate, set, generate: a setter that changes grids or arguments of the decode step drops the captured graphs, so the next generation captures
    the step again and gives the same tokens (which also holds for a graph that was kept: it is consistent in itself -- what this part catches is a
    drop without the recount of n_parts; at this shape the GEMV switches select no other grid, the 350M shape below is their case).  The last part
    is the check that fails when a setter does not drop the graphs."""
    eng, cfg = tiny, tiny.cfg
    eng.load_weights(cached_state_dict(cfg).items())
    g = torch.Generator().manual_seed(11)
    d = torch.randn(6, cfg.n_points, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    x = torch.cat([d * (0.3 + 0.7 * torch.rand(6, cfg.n_points, 1, generator=g)), d], -1)
    _, prefix = eng.encode(x.cuda())
    try:
        for rows in (1, 6):                                     # the GEMV chain and the matrix-core chain
            p = prefix[:rows].contiguous()
            want, want_len = eng.generate(p, suppress_eos=True)
            want = want.cpu()
            assert want.shape == (rows, cfg.max_new_tokens)
            again, _, want_lg = eng.generate(p, suppress_eos=True, return_logits=True)
            assert torch.equal(again.cpu(), want)
            decisive = _decisive(want_lg, GREEDY_TOL["bf16"])

            def same(what):
                got, got_len = eng.generate(p, suppress_eos=True)
                assert torch.equal(got.cpu(), want) and list(got_len) == list(want_len), (rows, what)
            # (same_there: the other value moves work between blocks or streams without changing any sum's order)
            for name, there, back, same_there in (("gemv_rpw", 1, 4, True), ("gemv_rpw", 2, 4, True), ("gemv_small_rows", 2, 1, False),
                                                  ("gemv_k8_ksplit", 2, 1, False), ("mfma_chunks", 4, 8, True), ("mfma_min_batch", 65, 4, False),
                                                  ("use_graph", 0, 1, True)):
                eng.set_option(name, there)
                if same_there:
                    same(f"{name}={there}")
                else:
                    got, _ = eng.generate(p, suppress_eos=True)
                    assert got.shape == want.shape
                    _agrees_where_decisive(eng, p, want, decisive, (rows, f"{name}={there}"))
                eng.set_option(name, back)
                same(f"{name} back to {back}")
        # The sharp check that the graphs ARE dropped: 6 rows step on the matrix cores; with mfma_min_batch = 65 they step on the GEMV chain (another
        # order of every sum).  A graph that survived the setter would replay the matrix-core step: replay and eager launches then disagree.
        p = prefix[:6].contiguous()
        _, _, mfma = eng.generate(p, suppress_eos=True, return_logits=True)                  # (captures the matrix-core step of 6 rows)
        eng.set_option("mfma_min_batch", 65)
        _, _, replayed = eng.generate(p, suppress_eos=True, return_logits=True)
        eng.set_option("use_graph", 0)
        _, _, eager = eng.generate(p, suppress_eos=True, return_logits=True)
        eng.set_option("use_graph", 1)
        eng.set_option("mfma_min_batch", 4)
        assert not torch.equal(mfma.view(torch.int32), eager.view(torch.int32)), "the two chains give the same bits: this check sees nothing"
        assert torch.equal(replayed.view(torch.int32), eager.view(torch.int32)), "mfma_min_batch did not drop the captured step"
        _, _, back = eng.generate(p, suppress_eos=True, return_logits=True)
        assert torch.equal(back.view(torch.int32), mfma.view(torch.int32)), "mfma_min_batch (back) did not drop the captured step"
    finally:
        eng.set_option("use_graph", 1)
        eng.set_option("mfma_min_batch", 4)


def test_gemv_rpw_recaptures_the_step_at_the_350m_shape(full8, golden_dir):
    """The sharp case: gemv_rpw changes the lm_head grid (8195 rows: 2 or 4 rows per wave) and with it the number of partial maxima the pick launch
    reads (n_parts).  One row, 96 tokens: moved to another accepted value and back, every generation gives the same tokens."""
    eng = full8
    load_weights_cached(eng, eng.cfg, init="diverse")
    _, prefix = eng.encode(mouse_variants(golden_dir, 1).cuda())
    want, _ = eng.generate(prefix, max_new_tokens=96, suppress_eos=True)
    want = want.cpu()
    assert len(set(want[0].tolist())) > 8
    again, _, want_lg = eng.generate(prefix, max_new_tokens=96, suppress_eos=True, return_logits=True)
    assert torch.equal(again.cpu(), want)
    decisive = _decisive(want_lg, GREEDY_TOL["bf16"])
    for name, there, back, same_there in (("gemv_rpw", 2, 4, True), ("gemv_rpw", 1, 4, True), ("gemv_small_rows", 2, 1, False), ("gemv_k8_ksplit", 2, 1, False)):
        eng.set_option(name, there)
        got, _ = eng.generate(prefix, max_new_tokens=96, suppress_eos=True)
        assert got.shape == want.shape and (not same_there or torch.equal(got.cpu(), want)), (name, there)
        if not same_there:
            _agrees_where_decisive(eng, prefix, want, decisive, f"{name}={there}", max_new_tokens=96)
        eng.set_option(name, back)
        got, _ = eng.generate(prefix, max_new_tokens=96, suppress_eos=True)
        assert torch.equal(got.cpu(), want), (name, "back to", back)
