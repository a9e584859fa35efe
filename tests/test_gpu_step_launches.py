"""Which launches a decode step consists of, pinned case by case (csrc/engine_decode.hpp decides it: the GEMV chain, the matrix-core chain, their
fused forms and the options that select among them), and the per-generation reset of the in-launch exchange buffers.

Per case two things are compared with a table recorded once from the library as it stood before the decode host was reorganised:
the launches per class that `profile_decode` counts (weights / attention / persistent / pick), and the full ordered (kind, blocks) list of
`trace_decode` (kinds: 0 embed, 1 qkv, 2 attention, 3 out_proj, 4 fc1, 5 fc2, 6 lm_head).  A host-side change that adds, drops, reorders or
regrids a launch of any covered path moves one of the two.  The table holds for a device that can keep the fused grids resident (an MI355X: 256 CUs).

Cross-check of the table against the code: batch 1, bf16, defaults is 24 x [q/k/v + attention | out_proj + fc1 + fc2] + lm_head + pick =
25 weight-class, 24 attention-class and 1 pick launch; embed_table 0 adds the embedding launch (26 + 24 + 1 = the 51 of engine.hip's header)."""
import pytest
import torch

from meshanything_amd.config import MAConfig, DTYPE_BF16, DTYPE_F32
from conftest import load_weights_cached

pytestmark = pytest.mark.gpu

FACES = 6                    # 9 * 6 + 2 = 56 new positions: the smallest cap with kv_len + 16 <= max_seq (trace_decode) at kv_len = T + 40
DEFAULTS = {"profile_batch": 1, "embed_table": 1, "fuse_qkv_attn": 1, "fuse_oproj_fc1": 1, "fuse_fc2": 1, "fuse_rows_attn": 1, "fuse_rows_mlp": 1,
            "rows_mlp_ln2": 1, "mfma_fold_ln": 1, "mfma_fc2_ksplit": 0}
EXP_DEFAULTS = {"rows_fused": 0, "fuse_layer": 0}

# case id: (policy, rows, the one option away from its default, needs an MA_EXPERIMENTAL library)
CASES = {f"bf16-b{b}": ("bf16", b, {}, False) for b in (1, 2, 4, 8, 12, 16)}
CASES.update({f"bf16-b1-{k}={v}": ("bf16", 1, {k: v}, False) for k, v in (("embed_table", 0), ("fuse_qkv_attn", 0), ("fuse_oproj_fc1", 0), ("fuse_fc2", 0))})
CASES.update({f"bf16-b8-{k}={v}": ("bf16", 8, {k: v}, False)
              for k, v in (("fuse_rows_attn", 0), ("fuse_rows_mlp", 0), ("rows_mlp_ln2", 0), ("mfma_fold_ln", 0), ("mfma_fc2_ksplit", 1))})
CASES.update({"fp32-b1": ("fp32", 1, {}, False), "fp32-b2": ("fp32", 2, {}, False),
              "bf16-b4-rows_fused=1": ("bf16", 4, {"rows_fused": 1}, True), "bf16-b1-fuse_layer=1": ("bf16", 1, {"fuse_layer": 1}, True)})

# case id: ((weights, attention, persistent, pick) launches of ONE step, the trace as runs: (repeat, ((kind, blocks), ...)))
EXPECT = {'bf16-b1': ((25, 24, 0, 1), ((24, ((2, 256), (3, 256))), (1, ((6, 513),)))),
 'bf16-b1-embed_table=0': ((26, 24, 0, 1), ((1, ((0, 256),)), (24, ((2, 256), (3, 256))), (1, ((6, 513),)))),
 'bf16-b1-fuse_fc2=0': ((49, 24, 0, 1), ((24, ((2, 256), (3, 256), (5, 256))), (1, ((6, 513),)))),
 'bf16-b1-fuse_layer=1': ((2, 24, 0, 1), ((1, ((2, 256), (3, 256), (6, 513))),)),
 'bf16-b1-fuse_oproj_fc1=0': ((73, 24, 0, 1), ((24, ((2, 256), (3, 256), (4, 256), (5, 256))), (1, ((6, 513),)))),
 'bf16-b1-fuse_qkv_attn=0': ((49, 24, 0, 1), ((24, ((1, 192), (2, 256), (3, 256))), (1, ((6, 513),)))),
 'bf16-b12': ((146, 24, 0, 1), ((1, ((0, 256),)), (24, ((1, 192), (3, 256), (4, 256), (5, 256))), (1, ((6, 513),)))),
 'bf16-b16': ((146, 24, 0, 1), ((1, ((0, 256),)), (24, ((1, 192), (3, 256), (4, 256), (5, 256))), (1, ((6, 513),)))),
 'bf16-b2': ((97, 24, 0, 1), ((24, ((1, 192), (2, 256), (3, 256), (4, 256), (5, 256))), (1, ((6, 513),)))),
 'bf16-b4': ((123, 24, 0, 1), ((1, ((0, 256),)), (24, ((1, 192), (3, 64), (4, 256), (5, 256))), (1, ((6, 513),)))),
 'bf16-b4-rows_fused=1': ((26, 24, 0, 1), ((1, ((0, 256),)), (24, ((2, 256), (3, 256))), (1, ((6, 513),)))),
 'bf16-b8': ((27, 24, 0, 1), ((1, ((0, 256),)), (24, ((2, 256), (4, 256))), (1, ((6, 513),)))),
 'bf16-b8-fuse_rows_attn=0': ((75, 24, 0, 1), ((1, ((0, 256),)), (24, ((1, 192), (3, 64), (4, 256))), (1, ((6, 513),)))),
 'bf16-b8-fuse_rows_mlp=0': ((51, 24, 0, 1), ((1, ((0, 256),)), (24, ((2, 256), (4, 256), (5, 256))), (1, ((6, 513),)))),
 'bf16-b8-mfma_fc2_ksplit=1': ((51, 24, 0, 1), ((1, ((0, 256),)), (24, ((2, 256), (4, 256), (5, 64))), (1, ((6, 513),)))),
 'bf16-b8-mfma_fold_ln=0': ((146, 24, 0, 1), ((1, ((0, 256),)), (24, ((1, 192), (3, 256), (4, 256), (5, 256))), (1, ((6, 513),)))),
 'bf16-b8-rows_mlp_ln2=0': ((27, 24, 0, 1), ((1, ((0, 256),)), (24, ((2, 256), (4, 256))), (1, ((6, 513),)))),
 'fp32-b1': ((25, 24, 0, 1), ((24, ((2, 256), (3, 256))), (1, ((6, 2049),)))),
 'fp32-b2': ((97, 24, 0, 1), ((24, ((1, 768), (2, 256), (3, 512), (4, 1024), (5, 1024))), (1, ((6, 2049),))))}


def expand(runs):
    return [pair for n, seq in runs for _ in range(n) for pair in seq]


def _engine(dtype, max_batch):
    from meshanything_amd.engine import Engine
    cfg = MAConfig.full(dtype=dtype, max_batch=max_batch, n_max_faces=FACES)
    eng = Engine(cfg)
    load_weights_cached(eng, cfg, init="diverse")
    assert eng.get_option("chain_resident") == 1, "the recorded table needs a device that holds the fused grids (MI355X, 256 CUs)"
    return eng


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(policy):
        if policy not in made:
            made[policy] = _engine(DTYPE_BF16, 16) if policy == "bf16" else _engine(DTYPE_F32, 2)
        return made[policy]
    try:
        yield get
    finally:
        for e in made.values():
            e.close()


def observe(eng, rows, flipped):
    """((weights, attention, persistent, pick) launches per step, [(kind, blocks), ...]) of the step of `rows` rows with `flipped` options set."""
    kv_len = eng.cfg.cond_length + 40
    exp = eng.get_option("experimental") == 1
    try:
        eng.set_option("profile_batch", rows)
        for k, v in flipped.items():
            eng.set_option(k, v)
        p = eng.profile_decode(kv_len, 2)
        t = eng.trace_decode(kv_len, max_launches=256)
    finally:
        for k, v in {**DEFAULTS, **(EXP_DEFAULTS if exp else {})}.items():
            eng.set_option(k, v)
    torch.cuda.synchronize()
    per_class = tuple(p["launches"][n] for n in ("gemv", "attn_decode", "persist", "pick"))
    assert all(n % 2 == 0 for n in per_class), per_class            # two steps
    return tuple(n // 2 for n in per_class), list(zip(t["kinds"].tolist(), t["blocks"].tolist()))


@pytest.mark.parametrize("case", list(CASES))
def test_step_launches(engines, case):
    policy, rows, flipped, needs_exp = CASES[case]
    eng = engines(policy)
    if needs_exp and eng.get_option("experimental") != 1:
        pytest.skip("needs a library built with MA_EXPERIMENTAL=1")
    per_class, trace = observe(eng, rows, flipped)
    print(f"[step launches] {case}: per class {per_class}, {len(trace)} traced launches: {trace}")
    want_class, want_runs = EXPECT[case]
    assert per_class == want_class, (case, per_class, want_class)
    assert trace == expand(want_runs), (case, trace, expand(want_runs))


def test_table_is_plausible():
    """The recorded table against what the code says a batch-1 step is (module docstring)."""
    assert EXPECT["bf16-b1"][0] == (25, 24, 0, 1)
    assert EXPECT["bf16-b1-embed_table=0"][0] == (26, 24, 0, 1) and sum(EXPECT["bf16-b1-embed_table=0"][0]) == 51
    assert set(EXPECT) == set(CASES)
    for case, (per_class, runs) in EXPECT.items():
        kinds = [k for k, _ in expand(runs)]
        assert kinds[-1] == 6 and kinds.count(6) == 1 and all(0 <= k <= 6 for k in kinds), case          # one lm_head, last
        policy, rows, flipped, _ = CASES[case]
        from_table = (policy == "fp32" or rows < 4) and "embed_table" not in flipped          # the GEMV chain's default: no embedding launch
        assert kinds.count(0) == (0 if from_table else 1), case


def test_exchange_buffers_reset_per_generation(engines):
    """Every in-launch exchange tags its granules with the cache position, which restarts with each generation: a buffer that the
    per-generation reset misses holds the previous generation's epochs, and the second generation reads stale data or times out.
    8 rows (the two fused 8-row launches) and 1 row (the two fused batch-1 launches) on one engine, twice each with the same inputs."""
    eng = engines("bf16")
    g = torch.Generator().manual_seed(5)
    prefix = torch.randn(8, eng.cfg.cond_length, eng.cfg.hidden, generator=g).cuda()
    counters = ("chain_fallbacks", "xchg_timeouts")
    before = {k: eng.get_option(k) for k in counters}
    first = {}
    for rnd in (0, 1):
        for rows in (8, 1):
            tok, lens = eng.generate(prefix[:rows].contiguous(), max_new_tokens=12, suppress_eos=True)
            tok = tok.cpu()
            assert tok.shape == (rows, 12)
            if rnd == 0:
                first[rows] = (tok, list(lens))
            else:
                assert torch.equal(tok, first[rows][0]) and list(lens) == first[rows][1], (rows, tok.tolist(), first[rows][0].tolist())
    assert {k: eng.get_option(k) for k in counters} == before, "an in-launch exchange gave up"
    assert eng.get_option("chain_resident") == 1
