"""Engine option `embed_table` (default 1): the token pick writes the next decode step's layer-0 input from a table built once per set of
weights (row v = input_layer(codebook[v]) + bias), so the step has no embedding launch (csrc/misc.hpp pick_kernel<true>,
csrc/engine_decode.hpp ensure_embtab).  The table is built by the gemv_kernel instantiation the embedding launch uses and the pick adds the
positional rows in that launch's order, so every comparison here is bitwise (`view(torch.int32)` equality), never a tolerance; option 0 --
the embedding launch per step -- is the control."""
import os

import numpy as np
import pytest
import torch

from meshanything_amd.config import MAConfig, DTYPE_BF16, DTYPE_F16, DTYPE_F32
from conftest import load_weights_cached

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": DTYPE_BF16, "fp16": DTYPE_F16, "fp32": DTYPE_F32}


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.fixture(scope="module", params=["bf16", "fp16", "fp32"])
def eng(request, golden_dir):
    """The 350M shape, two rows (batch 1: the two fused launches per layer; two rows: the same launches with the rows in the grid)."""
    from meshanything_amd.engine import Engine
    cfg = MAConfig.full(dtype=DTYPES[request.param], max_batch=2)
    e = Engine(cfg)
    load_weights_cached(e, cfg, init="diverse")           # a greedy stream that depends on its own tokens (checkpoint.py)
    d = dict(np.load(os.path.join(golden_dir, "dataset.npz")))
    _, prefix = e.encode(torch.from_numpy(d["mouse_norm"])[None].cuda())
    e.prefix = prefix
    e.policy = request.param
    yield e
    e.close()


def _tiny_cfg(dtype=DTYPE_BF16):
    # 16 faces: 146 tokens at the most, so that the 130-token case of the full shape exists here too
    return MAConfig.tiny(dtype=dtype, max_batch=2, n_max_faces=16, max_positions=17 + 16 * 9 + 2 + 6)


def _tiny_prefix(cfg, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, cfg.cond_length, cfg.hidden, generator=g).cuda()


def _run(e, table, prefix, n, **kw):
    """tokens, lengths, the last step's logits of every row [, whatever else generate returns] with embed_table = `table`."""
    e.set_option("embed_table", table)
    try:
        assert e.get_option("embed_table") == table, "embed_table is not read back as set on the GEMV chain"
        out = e.generate(prefix, max_new_tokens=n, **kw)
        lg = [e.read_logits(r).clone() for r in range(prefix.shape[0])]
    finally:
        e.set_option("embed_table", 1)
    torch.cuda.synchronize()
    return (out[0].cpu(), list(out[1]), [x.cpu() for x in lg]) + tuple(o.cpu() for o in out[2:])


def _same_step(e, prefix, n, what, **kw):
    t0, l0, g0 = _run(e, 0, prefix, n, **kw)[:3]
    t1, l1, g1 = _run(e, 1, prefix, n, **kw)[:3]
    assert torch.equal(t0, t1) and l0 == l1, f"{what}: tokens differ within {n} steps: {t0.tolist()} vs {t1.tolist()}"
    for r in range(prefix.shape[0]):
        assert torch.equal(_bits(g0[r]), _bits(g1[r])), \
            f"{what}: row {r}: logits of step {n - 1} differ: max abs {float((g0[r] - g1[r]).abs().max()):.3e} at {int((g0[r] - g1[r]).abs().argmax())}"
    return t1


# ---- (a) the table's rows are what the embedding launch computes in front of its positional adds
def _check_rows(e, rows):
    rows = sorted(set(int(r) for r in rows))
    H = e.cfg.hidden
    for r in rows:
        tab = e.embed_rows(r, 1, from_table=True)
        ref = e.embed_rows(r, 1, from_table=False)
        torch.cuda.synchronize()
        assert tab.shape == ref.shape == (1, H)
        assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0, f"row {r}: the embedding launch left nothing to compare"
        assert torch.equal(_bits(tab), _bits(ref)), f"table row {r} is not the embedding launch's value for token {r + 3}: max abs {float((tab - ref).abs().max()):.3e}"


@pytest.mark.parametrize("policy", ["bf16", "fp16", "fp32"])
def test_table_rows_tiny_every_row(policy):
    from meshanything_amd.engine import Engine
    cfg = _tiny_cfg(DTYPES[policy])
    e = Engine(cfg)
    try:
        load_weights_cached(e, cfg, init="diverse")
        # all rows in one call each (the table side is one copy; the launch side runs row by row inside the library)
        tab = e.embed_rows(0, cfg.codebook_size, from_table=True)
        ref = e.embed_rows(0, cfg.codebook_size, from_table=False)
        torch.cuda.synchronize()
        assert float(ref.abs().max()) > 0
        bad = (_bits(tab) != _bits(ref)).any(dim=1).nonzero().flatten().tolist()
        assert not bad, f"table rows {bad[:8]} (of {len(bad)}) differ from the embedding launch"
    finally:
        e.close()


def test_table_rows_full_shape(eng):
    V = eng.cfg.vocab
    others = np.random.default_rng(20).choice(np.arange(2, V - 4), size=64, replace=False)
    _check_rows(eng, [0, 1, V - 4] + others.tolist())


# ---- (b) the step with the table equals the step with the embedding launch
def test_step_equality_full_shape(eng):
    assert eng.get_option("embed_table") == 1, "embed_table must be on by default on the GEMV chain"
    seen = set()
    for n in (2, 3, 12, 130):            # 2, 3: t' = 1, 2, where (t' - 2) mod 9 is negative / zero; 12 wraps the nine slots
        seen |= set(_same_step(eng, eng.prefix, n, f"{eng.policy} batch 1", suppress_eos=True).flatten().tolist())
    assert len([t for t in seen if t >= 3]) >= 3, f"the stream never left a handful of tokens ({sorted(seen)}): no probe of the table"
    two = torch.cat([eng.prefix, eng.prefix.flip(1)])
    _same_step(eng, two, 40, f"{eng.policy} two rows", suppress_eos=True)


# ---- (c) special tokens and finished rows, through teacher forcing and the captured logits of every step
def _forced_case(eng, forced, suppress_eos):
    f = torch.tensor([forced], dtype=torch.int64)
    n = f.shape[1]
    a = _run(eng, 0, eng.prefix, n, forced_tokens=f, return_logits=True, suppress_eos=suppress_eos)
    b = _run(eng, 1, eng.prefix, n, forced_tokens=f, return_logits=True, suppress_eos=suppress_eos)
    assert a[3].shape == b[3].shape == (1, n, eng.cfg.vocab), (a[3].shape, b[3].shape)
    assert torch.equal(a[0], b[0]) and a[1] == b[1], (a[0].tolist(), b[0].tolist())
    diff = (_bits(a[3][0]) != _bits(b[3][0])).any(dim=1).nonzero().flatten().tolist()
    assert not diff, f"{eng.policy}: forced stream {forced}: the logits of steps {diff} differ between embed_table 0 and 1"
    return a[0]


def test_special_tokens_and_finished_rows(eng):
    V = eng.cfg.vocab
    # 24 tokens: bos, eos and pad inside the stream next to ordinary ids (first, last and scattered codebook rows)
    stream = [0, 3, 1, 17, 2, V - 1, 4000, 0, 5, 2, 1, 812, 6011, 3, 2, 2, 1, 0, 7777, 44, V - 2, 1234, 9, 2]
    assert len(stream) == 24 and {0, 1, 2} <= set(stream)
    _forced_case(eng, stream, suppress_eos=True)
    # eos at step 5 with eos allowed: the row is finished from there on (it reports pad; the given stream goes on feeding pad, as generate() does)
    fin = [0, 3, 815, 17, 4242] + [1] + [2] * 18
    assert len(fin) == 24 and fin[5] == 1
    picks = _forced_case(eng, fin, suppress_eos=False)
    assert picks.shape[1] == 24 and (picks[0, 6:] == 2).all(), f"a finished row must report pad: {picks.tolist()}"


def test_finished_row_feeds_pad_unforced():
    """A free-running row that emits eos keeps stepping on pad: the pick writes extra_embeds[pad] + its slot row.  Tiny shape, where random
    weights reach eos within the stream; both settings must agree on tokens, lengths and the last logits."""
    from meshanything_amd.engine import Engine
    cfg = _tiny_cfg()
    e = Engine(cfg)
    try:
        load_weights_cached(e, cfg, init="diverse")
        two = torch.cat([_tiny_prefix(cfg, 3), _tiny_prefix(cfg, 4)])
        _same_step(e, two, cfg.max_new_tokens, "tiny, eos allowed", check_every=5)
    finally:
        e.close()


# ---- (d) new weights in the same engine: a stale table would keep the first checkpoint's rows
def test_weights_reloaded_rebuild_the_table():
    from meshanything_amd.engine import Engine
    cfg = _tiny_cfg()
    prefix = _tiny_prefix(cfg)
    e = Engine(cfg)
    fresh = Engine(cfg)
    try:
        load_weights_cached(e, cfg, init="diverse", seed=1234)
        first = _run(e, 1, prefix, 9, suppress_eos=True)
        tab1 = e.embed_rows(0, cfg.codebook_size, from_table=True).clone()
        load_weights_cached(e, cfg, init="diverse", seed=4321)
        again = _run(e, 1, prefix, 9, suppress_eos=True)
        tab2 = e.embed_rows(0, cfg.codebook_size, from_table=True).clone()
        load_weights_cached(fresh, cfg, init="diverse", seed=4321)
        want = _run(fresh, 1, prefix, 9, suppress_eos=True)
        tabw = fresh.embed_rows(0, cfg.codebook_size, from_table=True)
        torch.cuda.synchronize()
        assert not torch.equal(_bits(tab1), _bits(tab2)), "the two checkpoints give the same table: the test cannot see a stale one"
        assert torch.equal(_bits(tab2), _bits(tabw)), "the table was not rebuilt for the second checkpoint"
        assert torch.equal(again[0], want[0]) and torch.equal(_bits(again[2][0]), _bits(want[2][0])), \
            f"second checkpoint in a used engine {again[0].tolist()} vs in a fresh one {want[0].tolist()}"
        assert not torch.equal(_bits(first[2][0]), _bits(again[2][0])), "the two checkpoints give the same logits: no probe"
        # ... and the same through the other loader (finalize_weights instead of mark_weights_loaded)
        from conftest import cached_state_dict
        e.load_weights(cached_state_dict(cfg, init="diverse", seed=1234).items())
        back = _run(e, 1, prefix, 9, suppress_eos=True)
        assert torch.equal(back[0], first[0]) and torch.equal(_bits(back[2][0]), _bits(first[2][0]))
    finally:
        e.close()
        fresh.close()


# ---- (e) the five-launch chain of the small shapes
def test_step_equality_five_launch_chain_tiny():
    from meshanything_amd.engine import Engine
    cfg = _tiny_cfg()
    e = Engine(cfg)
    try:
        load_weights_cached(e, cfg, init="diverse")
        e.set_option("fuse_qkv_attn", 0)
        e.set_option("fuse_oproj_fc1", 0)
        prefix = _tiny_prefix(cfg)
        for n in (2, 3, 12, 130):
            _same_step(e, prefix, n, "tiny five-launch chain", suppress_eos=True)
        _same_step(e, torch.cat([prefix, prefix.flip(1)]), 40, "tiny five-launch chain, two rows", suppress_eos=True)
        # graph replay == eager launches, with the table
        base = _run(e, 1, prefix, 40, suppress_eos=True)
        e.set_option("use_graph", 0)
        try:
            eager = _run(e, 1, prefix, 40, suppress_eos=True)
        finally:
            e.set_option("use_graph", 1)
        assert torch.equal(base[0], eager[0]) and torch.equal(_bits(base[2][0]), _bits(eager[2][0]))
    finally:
        e.close()


def test_option_readback_and_scope(eng):
    """Read back as applied: on for the GEMV chain (1 .. 3 rows), off for the matrix-core batches, which keep their embedding launch."""
    assert eng.get_option("embed_table") == 1
    eng.set_option("embed_table", 0)
    try:
        assert eng.get_option("embed_table") == 0
    finally:
        eng.set_option("embed_table", 1)
    eng.set_option("embed_table", 7)                       # a flag: stored as value != 0
    assert eng.get_option("embed_table") == 1
    if eng.policy != "fp32":
        from meshanything_amd.engine import Engine
        e8 = Engine(MAConfig.full(dtype=DTYPES[eng.policy], max_batch=8))
        try:
            e8.set_option("profile_batch", 8)
            assert e8.get_option("embed_table") == 0, "8 rows of a 16-bit policy step on the matrix cores: the embedding launch stays"
            e8.set_option("profile_batch", 2)
            assert e8.get_option("embed_table") == 1
        finally:
            e8.close()


def test_step_ab_report(eng):
    """Report-only (run with -s): the decode step as a graph replay with embed_table 0 / 1 interleaved in one process, four pairs at three cache
    lengths -- the figures of DESIGN.md section 6.  The yardstick is spread against gain: slowest option-1 repeat vs fastest option-0 repeat."""
    for L in (300, 3858, eng.cfg.max_seq - 80):
        rows = {0: [], 1: []}
        launches = {}
        for rep in range(4):
            for tab in (0, 1):
                eng.set_option("embed_table", tab)
                eng.profile_decode(L, 2)
                p = eng.profile_decode(L, 16)
                rows[tab].append(p["step_ms_graph"] * 1e3)
                launches[tab] = sum(p["launches"].values()) // 16
        eng.set_option("embed_table", 1)
        m0, m1 = float(np.median(rows[0])), float(np.median(rows[1]))
        print(f"[embed_table A/B {eng.policy}] kv_len {L:5d}: launch per step ({launches[0]} launches) " + " ".join(f"{x:6.1f}" for x in rows[0]) + f" | table ({launches[1]} launches) " +
              " ".join(f"{x:6.1f}" for x in rows[1]) + f" us/step | medians {m0:.1f} -> {m1:.1f} ({100 * (m1 / m0 - 1):+.2f} %) | slowest table {max(rows[1]):.1f} "
              f"{'<' if max(rows[1]) < min(rows[0]) else '>='} fastest launch {min(rows[0]):.1f}")
        assert launches[1] == launches[0] - 1, launches
