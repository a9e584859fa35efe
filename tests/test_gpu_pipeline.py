"""End-to-end parity on MI355X: the HIP engine (through the C ABI) against the CPU oracle and the
reference-generated golden fixtures, on a tiny configuration (full-length, seconds on CPU) and on the 350M shape."""
import os

import numpy as np
import pytest
import torch

from meshanything_amd.config import MAConfig, DTYPE_BF16, DTYPE_F16, DTYPE_F32
from meshanything_amd.checkpoint import synthetic_items, synthetic_state_dict
from conftest import mouse_variants, cached_state_dict, fused_generate, load_weights_cached, oracle_device

pytestmark = pytest.mark.gpu

POLICIES = {"fp32": DTYPE_F32, "bf16": DTYPE_BF16, "fp16": DTYPE_F16}
# logit-margin below which a greedy disagreement is an ambiguous step (summation order / one 16-bit rounding flip)
GREEDY_TOL = {"fp32": 2e-4, "bf16": 2e-2, "fp16": 3e-3}


def synth_cloud(seed, n):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    r = 0.3 + 0.7 * torch.rand(n, 1, generator=g)
    return torch.cat([d * r, d], dim=-1).numpy().astype(np.float32)


def clouds(cfg, seeds):
    from oracle.meshanything_oracle import normalize_pc
    return torch.from_numpy(np.stack([normalize_pc(synth_cloud(s, cfg.n_points)) for s in seeds]))


class Env:
    def __init__(self, cfg, policy, **engine_kw):
        from meshanything_amd.engine import Engine
        from oracle.meshanything_oracle import Oracle
        self.cfg, self.policy = cfg, policy
        self.sd = cached_state_dict(cfg)
        self.oracle = Oracle(cfg, self.sd, policy, device=oracle_device())
        self.engine = Engine(cfg)
        self.engine.load_weights(self.sd.items())


@pytest.fixture(scope="module", params=["fp32", "bf16", "fp16"])
def tiny(request):
    cfg = MAConfig.tiny(dtype=POLICIES[request.param], max_batch=4)
    env = Env(cfg, request.param)
    yield env
    env.engine.close()                  # not left to the collector: ma_engine_destroy frees device memory, a device-wide sync wherever it lands


def _tol(env, fp32, bf16):
    return fp32 if env.policy == "fp32" else (bf16 if env.policy == "bf16" else bf16 / 8)          # fp16: three more mantissa bits than bf16


def test_encode_tiny(tiny):
    x = clouds(tiny.cfg, [1, 2])
    lat, prefix = tiny.engine.encode(x.cuda())
    ref_lat = tiny.oracle.encode_latents(x)
    ref_prefix = tiny.oracle.process_point_feature(ref_lat)
    e1 = float((lat.cpu() - ref_lat).abs().max())
    e2 = float((prefix.cpu() - ref_prefix).abs().max())
    # north star: 1e-5 on encoder activations -- in EVERY policy: the point encoder stays fp32 under the 16-bit ones (cfg.enc_exact)
    assert e1 < 1e-5, e1
    assert e2 < 5e-5, e2


def test_encode_tiny_matches_reference_golden(tiny, golden_dir):
    """Directly against the reference's own perceiver output (tests/golden/tiny.npz)."""
    g = dict(np.load(os.path.join(golden_dir, "tiny.npz")))
    x = torch.from_numpy(g["tiny_input"])[None]
    lat, prefix = tiny.engine.encode(x.cuda())
    e1 = float(np.abs(lat[0, g["tiny_rows"]].cpu().numpy() - g["tiny_latents_rows"]).max())
    e2 = float(np.abs(prefix[0, g["tiny_rows"]].cpu().numpy() - g["tiny_prefix_rows"]).max())
    assert e1 < 1e-5, e1
    assert e2 < 5e-5, e2


def test_all_16bit_encoder_when_enc_exact_is_off(golden_dir):
    """cfg.enc_exact = 0: the encoder follows the 16-bit policy (bf16 GEMM / attention inputs) -- the round-3 behaviour, kept reachable."""
    from meshanything_amd.engine import Engine
    from oracle.meshanything_oracle import Oracle
    g = dict(np.load(os.path.join(golden_dir, "tiny.npz")))
    cfg = MAConfig.tiny(dtype=DTYPE_BF16, max_batch=2, enc_exact=0)
    sd = cached_state_dict(cfg)
    eng = Engine(cfg)
    eng.load_weights(sd.items())
    x = torch.from_numpy(g["tiny_input"])[None]
    lat, prefix = eng.encode(x.cuda())
    e1 = float(np.abs(lat[0, g["tiny_rows"]].cpu().numpy() - g["tiny_latents_rows"]).max())
    e2 = float(np.abs(prefix[0, g["tiny_rows"]].cpu().numpy() - g["tiny_prefix_rows"]).max())
    assert 1e-5 < e1 < 3e-2 and e2 < 8e-2, (e1, e2)                 # bf16 noise: present, bounded
    ora = Oracle(cfg, sd, "bf16", device=oracle_device())              # the oracle mirrors the policy bit
    ol = ora.encode_latents(x)
    assert float((lat.cpu() - ol).abs().max()) < 2e-2
    out = eng.forward(torch.cat([x, x]).cuda(), suppress_eos=True)
    assert out["coords"].shape[0] == 2
    eng.close()


def _check_greedy(env, prefix, tokens, lengths, suppress_eos=False):
    from oracle.meshanything_oracle import verify_greedy_stream
    out = []
    for b in range(prefix.shape[0]):
        n = int(lengths[b])
        v = verify_greedy_stream(env.oracle, prefix[b:b + 1], tokens[b, :n].cpu(), GREEDY_TOL[env.policy], suppress_eos)
        assert v["hard"] == [], v
        out.append(v)
    return out


def test_generate_greedy_tiny_full_length(tiny):
    x = clouds(tiny.cfg, [3, 4, 5])
    ref_lat = tiny.oracle.encode_latents(x)
    prefix = tiny.oracle.process_point_feature(ref_lat)            # isolate the decoder: same prefix on both sides
    toks, lengths = tiny.engine.generate(prefix.cuda(), suppress_eos=True)
    assert toks.shape == (3, tiny.cfg.max_new_tokens) and (lengths == tiny.cfg.max_new_tokens).all()
    v = _check_greedy(tiny, prefix, toks, lengths, suppress_eos=True)
    ref = tiny.oracle.generate(prefix, suppress_eos=True)
    if all(r["ambiguous"] == 0 for r in v):
        assert torch.equal(toks.cpu(), ref), "token streams differ although no step was ambiguous"
    assert not (toks == 1).any()                                   # eos suppressed


def test_generate_eos_and_padding_semantics(tiny):
    x = clouds(tiny.cfg, [6, 7, 8, 9])
    prefix = tiny.oracle.process_point_feature(tiny.oracle.encode_latents(x))
    toks, lengths = tiny.engine.generate(prefix.cuda(), check_every=5)
    ref = tiny.oracle.generate(prefix)
    _check_greedy(tiny, prefix, toks, lengths)
    toks = toks.cpu()
    for b in range(4):
        n = int(lengths[b])
        if n < toks.shape[1]:
            assert toks[b, n - 1] == 1 and (toks[b, n:] == 2).all()      # eos then pad=2, like generate()
    assert toks.shape[1] == int(lengths.max())
    if torch.equal(toks[:, :ref.shape[1]], ref[:, :toks.shape[1]]):
        assert toks.shape == ref.shape


def test_batched_rows_equal_single_row_runs(tiny):
    """Rows of a batch step together and share the weight stream, but each row's arithmetic is its own: a batch of 4 must
    produce, row for row, exactly the tokens of four batch-1 generations (greedy and sampled, with and without eos)."""
    x = clouds(tiny.cfg, [30, 31, 32, 33])
    prefix = tiny.oracle.process_point_feature(tiny.oracle.encode_latents(x)).cuda()
    tiny.engine.set_option("mfma_min_batch", 65)               # row-parallel GEMV path: bit-identical to batch 1 by construction
    for kw in (dict(suppress_eos=True), dict(), dict(sampling=True, seed=7, suppress_eos=True)):
        toks, lengths = tiny.engine.generate(prefix, check_every=3, **kw)
        for b in range(4):
            if kw.get("sampling"):
                continue                                       # the hashed uniform stream is keyed by the row index
            one, l1 = tiny.engine.generate(prefix[b:b + 1], check_every=3, **kw)
            n = int(l1[0])
            assert int(lengths[b]) == n
            assert torch.equal(toks[b, :n], one[0, :n]), f"row {b} of the batch differs from its batch-1 run ({kw})"
            assert (toks[b, n:] == 2).all()
        again, _ = tiny.engine.generate(prefix, check_every=3, **kw)
        assert torch.equal(toks, again)
    # injected uniforms: row b reads its own slice, so a batched sampled run equals the per-row runs
    g = torch.Generator().manual_seed(99)
    u = torch.rand(4, tiny.cfg.max_new_tokens, generator=g)
    toks, _ = tiny.engine.generate(prefix, sampling=True, uniforms=u, suppress_eos=True)
    for b in range(4):
        one, _ = tiny.engine.generate(prefix[b:b + 1], sampling=True, uniforms=u[b:b + 1], suppress_eos=True)
        assert torch.equal(toks[b], one[0])
    tiny.engine.set_option("mfma_min_batch", 4)


def test_batched_mfma_decode_matches_oracle(tiny):
    """bf16 policy, batch >= 4: the decode step runs as skinny GEMMs on the matrix cores (different summation order than
    the batch-1 GEMV, so equality with batch-1 runs is not the criterion): every row must be a valid greedy / sampled
    decode of its own prefix under the oracle, with eos/pad semantics intact, deterministic, graph == eager."""
    if tiny.policy == "fp32":
        pytest.skip("the fp32 policy has no MFMA decode path (row-parallel GEMV, covered above)")
    from oracle.meshanything_oracle import verify_sampled_stream
    x = clouds(tiny.cfg, [40, 41, 42, 43])
    prefix = tiny.oracle.process_point_feature(tiny.oracle.encode_latents(x))
    tiny.engine.set_option("mfma_min_batch", 4)
    toks, lengths = tiny.engine.generate(prefix.cuda(), suppress_eos=True)
    assert toks.shape == (4, tiny.cfg.max_new_tokens)
    _check_greedy(tiny, prefix, toks, lengths, suppress_eos=True)
    again, _ = tiny.engine.generate(prefix.cuda(), suppress_eos=True)
    assert torch.equal(toks, again)
    tiny.engine.set_option("use_graph", 0)
    eager, _ = tiny.engine.generate(prefix.cuda(), suppress_eos=True)
    tiny.engine.set_option("use_graph", 1)
    assert torch.equal(toks, eager)
    toks, lengths = tiny.engine.generate(prefix.cuda(), check_every=4)            # natural eos
    _check_greedy(tiny, prefix, toks, lengths)
    for b in range(4):
        n = int(lengths[b])
        if n < toks.shape[1]:
            assert toks[b, n - 1] == 1 and (toks[b, n:] == 2).all()
    g = torch.Generator().manual_seed(123)
    u = torch.rand(4, tiny.cfg.max_new_tokens, generator=g)
    toks, lengths = tiny.engine.generate(prefix.cuda(), sampling=True, uniforms=u, suppress_eos=True)
    ref = tiny.oracle.generate(prefix, sampling=True, uniforms=u.numpy(), suppress_eos=True)
    for b in range(4):
        if torch.equal(toks[b].cpu(), ref[b]):
            continue                                # identical to the oracle's own incremental sampled decode
        # otherwise the streams forked at a near-boundary draw: every step must still be a draw the oracle's teacher-forced
        # distribution allows (bf16: the teacher-forced pass itself differs from the incremental one by ~1e-2 in CDF)
        v = verify_sampled_stream(tiny.oracle, prefix[b:b + 1], toks[b].cpu(), u[b].numpy(), tol=6e-2, suppress_eos=True)
        assert v["hard"] == [], v


@pytest.mark.parametrize("B", [17, 40, 64])
def test_large_batches_all_mfma_tile_counts(B):
    """Batches of 17 / 40 / 64 rows = 2 / 3 / 4 batch tiles of the skinny GEMM, prefill in several groups of 16 samples, the
    row-per-wave attention with a ragged last block: every row verified by the oracle, and compared with the row-parallel
    GEMV path (same tokens unless a near-tie resolves differently)."""
    from meshanything_amd.engine import Engine
    from oracle.meshanything_oracle import Oracle
    cfg = MAConfig.tiny(dtype=DTYPE_BF16, max_batch=64)
    env = Env.__new__(Env)
    env.cfg, env.policy = cfg, "bf16"
    env.sd = cached_state_dict(cfg)
    env.oracle = Oracle(cfg, env.sd, "bf16", device=oracle_device())
    env.engine = Engine(cfg)
    env.engine.load_weights(env.sd.items())
    x = clouds(cfg, list(range(100, 100 + B)))
    prefix = env.oracle.process_point_feature(env.oracle.encode_latents(x))
    toks, lengths = env.engine.generate(prefix.cuda(), suppress_eos=True)
    assert toks.shape == (B, cfg.max_new_tokens)
    _check_greedy(env, prefix, toks, lengths, suppress_eos=True)
    env.engine.set_option("mfma_min_batch", 65)
    ref, _ = env.engine.generate(prefix.cuda(), suppress_eos=True)
    env.engine.set_option("mfma_min_batch", 4)
    same = int((ref == toks).all(dim=1).sum())
    assert same >= int(0.75 * B), f"only {same}/{B} rows equal the GEMV path"
    # >= 8 rows: the attention launch writes the finished output (one block per (row, head)); below, split-KV partials + a
    # merge launch.  Same arithmetic per position, different grouping of the partial softmax states.
    assert env.engine.get_option("attn_final_min_batch") == 8
    env.engine.set_option("attn_final_min_batch", 1000)
    split, split_len = env.engine.generate(prefix.cuda(), suppress_eos=True)
    env.engine.set_option("attn_final_min_batch", 8)
    _check_greedy(env, prefix, split, split_len, suppress_eos=True)
    same = int((split == toks).all(dim=1).sum())
    assert same >= int(0.75 * B), f"only {same}/{B} rows equal between the final and the split attention forms"
    out = env.engine.forward(x.cuda(), suppress_eos=True)           # encode + batched prefill + decode + detokenize for the whole batch
    assert out["coords"].shape == (B, cfg.n_max_faces, 3, 3) and out["tokens"].shape == toks.shape
    # (its prefix comes from the engine's own bf16 encoder, not the oracle's: near-tie rows may differ from `toks`)
    again = env.engine.forward(x.cuda(), suppress_eos=True)
    assert torch.equal(out["tokens"], again["tokens"])


@pytest.mark.parametrize("B,G", [(8, 2), (13, 3), (24, 4), (9, 2)])
def test_large_batches_row_groups_equal_their_own_batches(B, G):
    """decode_groups (opt-in: measured slower, profiles/r03_ab_row_groups.txt): the rows of a batch are cut into G groups that step
    concurrently on their own streams (captured graph per group).  Nothing crosses a group, and on the matrix-core path a row's arithmetic depends only on the kernel forms its GROUP
    size selects -- so group g of a grouped run must reproduce, bit for bit, an ungrouped run of just its rows; greedy, with
    eos / pad bookkeeping, and sampled from injected uniforms."""
    from meshanything_amd.engine import Engine
    from oracle.meshanything_oracle import Oracle
    cfg = MAConfig.tiny(dtype=DTYPE_BF16, max_batch=32)
    sd = cached_state_dict(cfg)
    oracle = Oracle(cfg, sd, "bf16", device=oracle_device())
    eng = Engine(cfg)
    eng.load_weights(sd.items())
    x = clouds(cfg, list(range(300, 300 + B)))
    prefix = oracle.process_point_feature(oracle.encode_latents(x)).cuda()
    u = torch.rand(B, cfg.max_new_tokens, generator=torch.Generator().manual_seed(5))
    eng.set_option("profile_batch", B)
    for kw in (dict(suppress_eos=True), dict(check_every=5), dict(sampling=True, uniforms=u, suppress_eos=True)):
        eng.set_option("decode_groups", G)
        n_groups = eng.get_option("decode_groups")
        assert n_groups == G
        toks, lengths = eng.generate(prefix, **kw)
        again, _ = eng.generate(prefix, **kw)
        assert torch.equal(toks, again), "grouped generation is not deterministic"
        eng.set_option("decode_groups", 1)
        r0 = 0
        for g in range(n_groups):
            n = B // n_groups + (1 if g < B % n_groups else 0)
            kw_g = dict(kw)
            if "uniforms" in kw_g:
                kw_g["uniforms"] = u[r0:r0 + n]
            alone, len_alone = eng.generate(prefix[r0:r0 + n], **kw_g)
            w = min(alone.shape[1], toks.shape[1])
            for b in range(n):
                m = min(int(lengths[r0 + b]), int(len_alone[b]))
                assert int(lengths[r0 + b]) == int(len_alone[b]), f"group {g} row {b}: lengths differ ({kw.keys()})"
                assert torch.equal(toks[r0 + b, :m], alone[b, :m]), f"group {g} (rows {r0}..{r0 + n - 1}) row {b} differs from its own batch ({list(kw)})"
            r0 += n
    eng.set_option("decode_groups", 1)


def test_graph_eager_and_stepwise_prefill_agree(tiny):
    x = clouds(tiny.cfg, [10])
    prefix = tiny.oracle.process_point_feature(tiny.oracle.encode_latents(x)).cuda()
    base, _ = tiny.engine.generate(prefix, suppress_eos=True)
    again, _ = tiny.engine.generate(prefix, suppress_eos=True)
    assert torch.equal(base, again), "generation is not deterministic"
    tiny.engine.set_option("use_graph", 0)
    eager, _ = tiny.engine.generate(prefix, suppress_eos=True)
    tiny.engine.set_option("use_graph", 1)
    assert torch.equal(base, eager), "hipGraph replay and eager launches disagree"
    tiny.engine.set_option("prefill_stepwise", 1)
    step, lens = tiny.engine.generate(prefix, suppress_eos=True)
    tiny.engine.set_option("prefill_stepwise", 0)
    # the stepwise prefill uses the GEMV kernels (different summation order): verify instead of demanding equality
    _check_greedy(tiny, prefix.cpu(), step, lens, suppress_eos=True)


def test_sampling_with_injected_uniforms(tiny):
    from oracle.meshanything_oracle import verify_sampled_stream
    x = clouds(tiny.cfg, [11, 12])
    prefix = tiny.oracle.process_point_feature(tiny.oracle.encode_latents(x))
    maxn = tiny.cfg.max_new_tokens
    u = np.random.default_rng(5).random((2, maxn)).astype(np.float32)
    toks, lengths = tiny.engine.generate(prefix.cuda(), sampling=True, uniforms=torch.from_numpy(u), suppress_eos=True)
    for b in range(2):
        # bf16: the engine's logits sit within ~7e-3 of the bf16-policy oracle's (either dense-attention kernel, scripts/archive/diag_r3d.py); on this
        # 61-token vocabulary that moves a CDF boundary by up to a few percent -- same bound as the batched test above
        v = verify_sampled_stream(tiny.oracle, prefix[b:b + 1], toks[b].cpu(), u[b], tol=_tol(tiny, 1e-4, 5e-2), suppress_eos=True)
        assert v["hard"] == [], v
        assert v["exact"] >= (v["n"] - 3 if tiny.policy == "fp32" else int(0.8 * v["n"])), v
    # greedy and sampled streams differ (the sampler is really used)
    g, _ = tiny.engine.generate(prefix.cuda(), suppress_eos=True)
    assert not torch.equal(g, toks)
    # in-kernel uniform stream: deterministic in the seed
    a, _ = tiny.engine.generate(prefix.cuda(), sampling=True, seed=7, suppress_eos=True)
    b_, _ = tiny.engine.generate(prefix.cuda(), sampling=True, seed=7, suppress_eos=True)
    c, _ = tiny.engine.generate(prefix.cuda(), sampling=True, seed=8, suppress_eos=True)
    assert torch.equal(a, b_) and not torch.equal(a, c)


def test_postprocess_and_detokenize_tiny(tiny):
    cfg = tiny.cfg
    x = clouds(cfg, [13, 14])
    lat = tiny.oracle.encode_latents(x)
    rng = np.random.default_rng(3)
    res = torch.from_numpy(rng.integers(3, cfg.vocab, size=(2, cfg.max_new_tokens)).astype(np.int64))
    res[0, 0] = 0
    res[0, 30] = 1; res[0, 31:] = 2            # row 0 stops early
    res[1, 0] = 0
    res[1, 9 * 2 + 4] = 2                      # a special mid-sequence kills just that face
    ids = tiny.engine.postprocess_tokens(res[:, :40].cuda())
    ref_ids = tiny.oracle.postprocess_tokens(res[:, :40])
    assert torch.equal(ids.cpu(), ref_ids)
    ids = tiny.engine.postprocess_tokens(res.cuda())
    ref_ids = tiny.oracle.postprocess_tokens(res)
    assert torch.equal(ids.cpu(), ref_ids)
    coords = tiny.engine.detokenize(ids, lat.cuda()).cpu()
    ref, logits = tiny.oracle.detokenize(ref_ids, tiny.oracle.get_codes(ref_ids), lat, return_logits=True)
    assert torch.equal(torch.isnan(coords), torch.isnan(ref))
    diff = (torch.nan_to_num(coords, nan=9.0) != torch.nan_to_num(ref, nan=9.0))
    if diff.any():      # only near-ties between bins may differ
        srt = torch.sort(logits, dim=-1, descending=True).values
        gap = (srt[..., 0] - srt[..., 1]).reshape(coords.shape)
        assert float(gap[diff].max()) < _tol(tiny, 1e-4, 5e-2), float(gap[diff].max())
        assert int(diff.sum()) <= 2


def test_forward_end_to_end_tiny(tiny):
    x = clouds(tiny.cfg, [15, 16])
    out = tiny.engine.forward(x.cuda())
    ref = tiny.oracle.forward(x)
    lat_err = float((out["latents"].cpu() - ref["point_feature"]).abs().max())
    assert lat_err < 1e-5
    if torch.equal(out["tokens"].cpu(), ref["tokens"]):
        assert torch.equal(out["ids"].cpu(), ref["ids"])
        c, r = out["coords"].cpu(), ref["coords"]
        assert torch.equal(torch.isnan(c), torch.isnan(r))
        assert int((torch.nan_to_num(c, nan=9.0) != torch.nan_to_num(r, nan=9.0)).sum()) <= 2
    else:               # an ambiguous step somewhere: the stream must still be a valid greedy decode of its own prefix
        from oracle.meshanything_oracle import verify_greedy_stream
        for b in range(2):
            n = int(out["lengths"][b])
            v = verify_greedy_stream(tiny.oracle, ref["prefix"][b:b + 1], out["tokens"][b, :n].cpu(), GREEDY_TOL[tiny.policy])
            assert v["hard"] == [], v


def test_weights_are_required_and_checked():
    from meshanything_amd.engine import Engine
    from meshanything_amd._lib import MAError
    cfg = MAConfig.tiny()
    eng = Engine(cfg)
    with pytest.raises(MAError, match="MA_ERR_STATE"):
        eng.encode(torch.zeros(1, cfg.n_points, 6).cuda())
    sd = synthetic_state_dict(cfg)
    some = list(sd.items())
    eng.load_weights(some[:10], finalize=False)
    with pytest.raises(MAError, match="MA_ERR_MISSING"):
        eng.load_weights([], finalize=True)
    with pytest.raises(MAError, match="MA_ERR_UNKNOWN_TENSOR"):
        eng.load_weights([("no.such.key", np.zeros(3, np.float32))], finalize=False)
    with pytest.raises(MAError, match="MA_ERR_SHAPE"):
        eng.load_weights([("cond_proj.bias", np.zeros(3, np.float32))], finalize=False)
    eng.load_weights(some[10:])                                   # now complete
    # BetterTransformer names for the detokenizer layers land in the same arena bytes
    eng2 = Engine(cfg)
    van = sd
    fused = synthetic_state_dict(cfg, bert_fused=True)
    for n in range(cfg.tok_layers):
        p = f"tokenizer.decoder.layer.{n}."
        fused[p + "in_proj_weight"] = np.concatenate([van[p + f"attention.self.{k}.weight"] for k in ("query", "key", "value")])
        fused[p + "in_proj_bias"] = np.concatenate([van[p + f"attention.self.{k}.bias"] for k in ("query", "key", "value")])
        for a_, b_ in (("out_proj_weight", "attention.output.dense.weight"), ("out_proj_bias", "attention.output.dense.bias"),
                       ("linear1_weight", "intermediate.dense.weight"), ("linear1_bias", "intermediate.dense.bias"),
                       ("linear2_weight", "output.dense.weight"), ("linear2_bias", "output.dense.bias"),
                       ("norm1_weight", "attention.output.LayerNorm.weight"), ("norm1_bias", "attention.output.LayerNorm.bias"),
                       ("norm2_weight", "output.LayerNorm.weight"), ("norm2_bias", "output.LayerNorm.bias")):
            fused[p + a_] = van[p + b_]
    eng2.load_weights(fused.items())
    assert torch.equal(eng.arena_tensor(), eng2.arena_tensor())
    # fp16 / bf16 checkpoint tensors are accepted (converted on load)
    eng3 = Engine(cfg)
    eng3.load_weights(((k, torch.from_numpy(v).to(torch.bfloat16)) for k, v in sd.items()))
    # large tensors are converted on the device (ma_engine_load_weights), small ones on the host: both must produce the bytes of the
    # host-only packer (ma_pack_weights_host, what a DP rank 0 would broadcast) -- a 1021-entry codebook makes lm_head (-> bf16) and the
    # codebook table (-> fp32) large enough for the device path, from fp32, bf16 and fp16 storage
    from meshanything_amd import dp
    for dt in (DTYPE_BF16, DTYPE_F32):
        cfg2 = MAConfig.tiny(dtype=dt, codebook_size=1021)
        sd2 = synthetic_state_dict(cfg2)
        assert sd2["transformer.lm_head.weight"].size >= 1 << 16
        for conv in (lambda v: v, lambda v: torch.from_numpy(v).to(torch.bfloat16), lambda v: v.astype(np.float16)):
            items = [(k, conv(v)) for k, v in sd2.items()]
            host = dp.pack_host_arena(cfg2, items)
            e4 = Engine(cfg2)
            e4.load_weights(items)
            assert np.array_equal(e4.arena_tensor().cpu().numpy(), host), "device-side and host-side weight packing disagree"
            e4.close()


# ------------------------------------------------------------------------------------------------ 350M shape
# Weights: init="diverse" (checkpoint.py) -- the default synthetic checkpoint has a greedy fixed point (token 2668 for ever), on which
# "tokens identical" means "argmax == 2668 at a 0.32 margin" (VERDICT r3); with the decoder's residual branches at a fifth of their gain
# the greedy stream depends on its own tokens and positions.  Every greedy test below asserts that its stream really is diverse.
# Encoder and detokenizer weights are the default ones (same numbers), so the reference goldens of full.npz apply unchanged.
FULL_INIT = "diverse"


def assert_diverse(tokens, at_least, what=""):
    n = len(set(tokens.reshape(-1).tolist()))
    assert n >= at_least, f"{what}: only {n} distinct token ids -- a collapsed stream proves nothing"
    return n


@pytest.fixture(scope="module", params=["fp32", "bf16", "fp16"])
def full(request):
    from meshanything_amd.engine import Engine
    from oracle.meshanything_oracle import Oracle
    cfg = MAConfig.full(dtype=POLICIES[request.param], max_batch=6)
    env = Env.__new__(Env)
    env.cfg, env.policy = cfg, request.param
    env.sd = cached_state_dict(cfg, init=FULL_INIT)
    env.oracle = Oracle(cfg, env.sd, request.param, device=oracle_device())
    env.engine = Engine(cfg)
    load_weights_cached(env.engine, cfg, init=FULL_INIT)
    yield env
    env.engine.close()


def test_full_encode_and_detok_match_reference_golden(full, golden_dir):
    """350M-shape encoder + prefix + detokenizer on pc_examples/mouse.npy against the reference's own modules."""
    g = dict(np.load(os.path.join(golden_dir, "full.npz")))
    d = dict(np.load(os.path.join(golden_dir, "dataset.npz")))
    x = torch.from_numpy(d["mouse_norm"])[None]                       # fp16, exactly what Dataset.__getitem__ yields
    lat, prefix = full.engine.encode(x.cuda())
    rows = g["full_rows"]
    e_lat = float(np.abs(lat[0, rows].cpu().numpy() - g["full_latents_rows"]).max())
    e_lat8 = float(np.abs(lat[0, :, :8].cpu().numpy() - g["full_latents_cols8"]).max())
    e_pre = float(np.abs(prefix[0, rows].cpu().numpy() - g["full_prefix_rows"]).max())
    print(f"[{full.policy}] encoder max abs err vs reference: latents {e_lat:.3e}/{e_lat8:.3e}, prefix {e_pre:.3e}")
    assert max(e_lat, e_lat8) < 1e-5                                # BASELINE.json: 1e-5 on encoder activations, in the benchmarked (bf16) policy too
    assert e_pre < 1e-4
    ids = torch.from_numpy(g["full_detok_ids"])
    if full.policy == "fp32":
        ref_lat = lat
        coords = full.engine.detokenize(ids.cuda(), ref_lat).cpu().numpy()
        ref = g["full_detok_coords"]
        assert np.array_equal(np.isnan(coords), np.isnan(ref))
        mism = int((np.nan_to_num(coords, nan=9.0) != np.nan_to_num(ref, nan=9.0)).sum())
        print(f"[fp32] detokenizer: {mism} of {ref.size} coordinate bins differ from the reference")
        assert mism <= 3
    else:
        olat = full.oracle.encode_latents(x)
        coords = full.engine.detokenize(ids.cuda(), olat.cuda()).cpu()
        ref, logits = full.oracle.detokenize(ids, full.oracle.get_codes(ids), olat, return_logits=True)
        assert torch.equal(torch.isnan(coords), torch.isnan(ref))
        diff = torch.nan_to_num(coords, nan=9.0) != torch.nan_to_num(ref, nan=9.0)
        srt = torch.sort(logits, dim=-1, descending=True).values
        gap = (srt[..., 0] - srt[..., 1]).reshape(coords.shape)
        print(f"[{full.policy}] detokenizer: {int(diff.sum())} bins differ from the {full.policy}-policy oracle; worst gap {float(gap[diff].max()) if diff.any() else 0:.3e}")
        assert int(diff.sum()) <= 72 and (not diff.any() or float(gap[diff].max()) < 0.05)   # <= 1% of bins, near-ties only


def test_full_generate_matches_oracle(full, golden_dir):
    d = dict(np.load(os.path.join(golden_dir, "dataset.npz")))
    x = torch.from_numpy(d["mouse_norm"])[None]
    prefix = full.oracle.process_point_feature(full.oracle.encode_latents(x))
    n = int(os.environ.get("MA_TEST_GEN_TOKENS", "400"))
    toks, lengths = fused_generate(full.engine, f"{full.policy} batch 1", prefix.cuda(), max_new_tokens=n, suppress_eos=True)
    v = _check_greedy(full, prefix, toks, lengths, suppress_eos=True)
    nd = assert_diverse(toks, 48, "350M greedy decode")
    print(f"[{full.policy}] {n}-token greedy decode ({nd} distinct ids) vs oracle: {v}")
    # near-ties (oracle margin below the policy's noise floor) may resolve differently: the diverse stream has a few per hundred steps
    assert v[0]["ambiguous"] <= (3 if full.policy == "fp32" else max(3, n // 16))


def test_full_batched_generate_matches_oracle(full, golden_dir):
    """350M shape, a batch of 6 clouds (BASELINE.json configs 3/4 in small): bf16 runs the MFMA skinny-GEMM decode,
    fp32 the row-parallel GEMV; every row's greedy stream is verified by the oracle, and row 0 (mouse.npy) must equal its
    batch-1 stream when the batch uses the GEMV path."""
    x = mouse_variants(golden_dir, 6)                   # row 0 = mouse.npy itself
    prefix = full.oracle.process_point_feature(full.oracle.encode_latents(x))
    n = 160
    toks, lengths = fused_generate(full.engine, f"{full.policy} batch 6", prefix.cuda(), max_new_tokens=n, suppress_eos=True)
    assert toks.shape == (6, n)
    v = _check_greedy(full, prefix, toks, lengths, suppress_eos=True)
    nd = [assert_diverse(toks[b], 24, f"batch row {b}") for b in range(6)]
    assert len({tuple(r.tolist()) for r in toks.cpu()}) == 6, "rows of distinct shapes produced identical streams"
    print(f"[{full.policy}] batch-6 {n}-token greedy decode vs oracle: ambiguous {[r['ambiguous'] for r in v]}, distinct ids per row {nd}")
    # no hard disagreement (checked by _check_greedy); near-ties (oracle top-2 margin below the policy's noise floor) may
    # resolve differently -- the MFMA GEMM sums in another order than the oracle's emulation -- but must stay rare
    assert all(r["ambiguous"] <= max(2, n // 12) for r in v)
    one, _ = full.engine.generate(prefix[:1].cuda(), max_new_tokens=n, suppress_eos=True)
    if full.policy == "fp32":
        assert torch.equal(one[0], toks[0])
    else:
        full.engine.set_option("mfma_min_batch", 65)
        rowpar, _ = full.engine.generate(prefix.cuda(), max_new_tokens=n, suppress_eos=True)
        full.engine.set_option("mfma_min_batch", 4)
        assert torch.equal(one[0], rowpar[0])
        same = int((rowpar == toks).all(dim=1).sum())
        print(f"[{full.policy}] MFMA batch path vs GEMV batch path: {same}/6 rows token-identical over {n} tokens")
        # the final-form attention (default from 8 rows on; 8 waves per (row, head) block below 12 rows) at the 350M shape
        full.engine.set_option("attn_final_min_batch", 4)
        fin, fin_len = full.engine.generate(prefix.cuda(), max_new_tokens=n, suppress_eos=True)
        full.engine.set_option("attn_final_min_batch", 8)
        vf = _check_greedy(full, prefix, fin, fin_len, suppress_eos=True)
        assert all(r["ambiguous"] <= max(2, n // 12) for r in vf)
        same = int((fin == toks).all(dim=1).sum())
        # (on a diverse stream a near-tie that resolves differently forks the row for good: identity of whole rows is reported, not demanded)
        print(f"[{full.policy}] final-form vs split attention on the MFMA path: {same}/6 rows token-identical over {n} tokens")


def test_full_length_generation_properties(full, golden_dir):
    """BASELINE.json config 2 at full length (7202 tokens): deterministic, graph == eager, tokens in range,
    post-processing/detokenizer accept the stream; EVERY token of it is verified by the policy's oracle (one causal pass over 7 459 positions)."""
    cfg = full.cfg
    d = dict(np.load(os.path.join(golden_dir, "dataset.npz")))
    x = torch.from_numpy(d["mouse_norm"])[None]
    out = full.engine.forward(x.cuda(), suppress_eos=True)
    toks = out["tokens"]
    assert toks.shape == (1, cfg.max_new_tokens) and int(out["lengths"][0]) == cfg.max_new_tokens
    assert int(toks.min()) >= 0 and int(toks.max()) < cfg.vocab and not (toks == 1).any()
    nd = assert_diverse(toks, 256, "full-length generation")
    print(f"[{full.policy}] full-length stream: {nd} distinct ids in {cfg.max_new_tokens} tokens")
    again = full.engine.forward(x.cuda(), suppress_eos=True)
    assert torch.equal(toks, again["tokens"]) and torch.equal(torch.nan_to_num(out["coords"]), torch.nan_to_num(again["coords"]))
    if full.policy != "fp32":
        full.engine.set_option("use_graph", 0)
        eager = full.engine.forward(x.cuda(), suppress_eos=True, max_new_tokens=600)
        full.engine.set_option("use_graph", 1)
        assert torch.equal(eager["tokens"][0], toks[0, :600])
    coords = out["coords"].cpu()
    valid = ~torch.isnan(coords[0, :, 0, 0])
    assert float(coords[0][valid].min()) >= -0.5 and float(coords[0][valid].max()) <= 0.4921875
    nver = int(os.environ.get("MA_TEST_VERIFY_TOKENS", str(cfg.max_new_tokens)))       # ALL 7 202 tokens: one causal pass of the oracle on torch-ROCm
    from oracle.meshanything_oracle import verify_greedy_stream
    prefix = full.oracle.process_point_feature(out["latents"].cpu())
    v = verify_greedy_stream(full.oracle, prefix, toks[0, :nver].cpu(), GREEDY_TOL[full.policy], suppress_eos=True)
    print(f"[{full.policy}] full-length stream, first {nver} tokens vs oracle: {v}")
    assert v["hard"] == [], v


def test_v2_scale_1600_faces(golden_dir):
    """BASELINE.json configs[4] at its own shape (1600-face cap: 14402 new tokens, cache 14659 positions, 1.44 GB of KV per row in bf16,
    batch 8):
    the longer cache stride, position table rows and 16-chunk attention split are exercised by a short batched decode that
    the oracle verifies, plus one step profiled deep into the cache."""
    from meshanything_amd.engine import Engine
    from oracle.meshanything_oracle import Oracle
    cfg = MAConfig.full(dtype=DTYPE_BF16, n_max_faces=1600, max_batch=8)
    assert cfg.max_seq == 14659 and cfg.max_new_tokens == 14402
    env = Env.__new__(Env)
    env.cfg, env.policy = cfg, "bf16"
    env.sd = cached_state_dict(cfg, init=FULL_INIT)
    env.oracle = Oracle(cfg, env.sd, "bf16", device=oracle_device())
    env.engine = Engine(cfg)
    load_weights_cached(env.engine, cfg, init=FULL_INIT)
    x = mouse_variants(golden_dir, 8)
    prefix = env.oracle.process_point_feature(env.oracle.encode_latents(x))
    toks, lengths = fused_generate(env.engine, "1600 faces, batch 8", prefix.cuda(), max_new_tokens=96, suppress_eos=True)
    assert toks.shape == (8, 96)
    v = _check_greedy(env, prefix, toks, lengths, suppress_eos=True)
    assert all(r["ambiguous"] <= 8 for r in v), [r["ambiguous"] for r in v]
    assert len({tuple(r.tolist()) for r in toks.cpu()}) == 8 and all(assert_diverse(toks[b], 16, f"row {b}") for b in range(8))
    env.engine.set_option("profile_batch", 8)
    p = env.engine.profile_decode(cfg.max_seq - 64, 2)              # a step with ~14.6k cached positions per row
    print(f"[1600 faces, batch 8] decode step at kv_len {cfg.max_seq - 64}: {p['step_ms_graph']:.3f} ms")
    assert 0 < p["step_ms_graph"] < 50


def test_v2_scale_config3_batch64_sampling(golden_dir):
    """BASELINE.json config 3 at its own shape: 64 rows stepping together at the 350M shape with top-k 50 / top-p 0.95 sampling
    (four batch tiles of the skinny GEMM, final-form attention with 1024 (row, head) blocks, the radix-select sampler on 64 rows).
    Uniforms are injected, so every draw of every row can be checked against the oracle's own filtered distribution, teacher-forced
    on the engine's tokens (the CDF interval test of verify_sampled_stream; bf16 logits move the interval edges by a few 1e-2)."""
    from meshanything_amd.engine import Engine
    from oracle.meshanything_oracle import Oracle, verify_sampled_batch
    B, n = 64, 96
    cfg = MAConfig.full(dtype=DTYPE_BF16, max_batch=B)
    sd = cached_state_dict(cfg, init=FULL_INIT)
    oracle = Oracle(cfg, sd, "bf16", device=oracle_device())
    eng = Engine(cfg)
    load_weights_cached(eng, cfg, init=FULL_INIT)
    x = mouse_variants(golden_dir, B)
    prefix = torch.cat([oracle.process_point_feature(oracle.encode_latents(x[i:i + 16])) for i in range(0, B, 16)])
    u = torch.rand(B, n, generator=torch.Generator().manual_seed(64))
    toks, lengths = eng.generate(prefix.cuda(), sampling=True, uniforms=u, max_new_tokens=n, suppress_eos=True)
    assert toks.shape == (B, n) and (lengths == n).all()
    assert int(toks.min()) >= 0 and int(toks.max()) < cfg.vocab and not (toks == 2).any()      # no pad inside a suppressed-eos stream
    again, _ = eng.generate(prefix.cuda(), sampling=True, uniforms=u, max_new_tokens=n, suppress_eos=True)
    assert torch.equal(toks, again), "sampling from injected uniforms is not deterministic"
    v = verify_sampled_batch(oracle, prefix, toks, u, tol=6e-2, suppress_eos=True)
    d = v["distance"].flatten()
    n_out = int((~torch.isfinite(d)).sum())                         # tokens that are not even among the oracle's 64 largest scores
    d = d[torch.isfinite(d)]
    q = [float(torch.quantile(d, x)) for x in (0.5, 0.9, 0.99)]
    print(f"[config 3: batch 64, 350M, top-k/top-p] {v['n']} draws: {v['exact']} equal the oracle's own draw, {v['ambiguous']} more on the token's CDF interval "
          f"within 6e-2, {len(v['hard'])} by the strict rule outside; distance of the uniform from the token's interval on the oracle's CDF: "
          f"median {q[0]:.4f}, 90 % {q[1]:.4f}, 99 % {q[2]:.4f}, max {float(d.max()):.4f}; {n_out} tokens outside the oracle's 64 largest scores")
    # Random-init weights give a nearly flat top-50 (logit span ~1.5, neighbours ~0.03 apart: interval widths ~0.02), so the engine's
    # bf16 logits reorder neighbours and move the top-p cut by a few candidates; the draw then lands a few intervals away.  What must
    # hold -- and what a wrong uniform slice, a wrong row or a broken selection would break (mean distance ~0.25, tokens outside the
    # top-k) -- is that every token is one of the oracle's top candidates (a near-tie at the 50th score can let its neighbour in) and sits where its uniform points, within that noise:
    # measured on MI355X (profiles/r03_diag_sampling_draws.txt): 99 % within 0.044, max 0.096 for 6144 draws, the same at batch 1 / 4 / 16.
    assert n_out == 0, f"{n_out} sampled tokens far outside the oracle's top-k"
    assert v["exact"] >= 0.5 * v["n"]
    assert q[2] <= 0.07 and float(d.max()) <= 0.16, (q, float(d.max()))
    # rows are distinct shapes: their streams differ
    assert len({tuple(r.tolist()) for r in toks.cpu()}) > B // 2
    eng.close()


@pytest.mark.parametrize("policy", ["bf16", "fp16"])
def test_prefill_kv_written_by_the_qkv_gemm_equals_the_copy(golden_dir, policy):
    """Round 6: at 64 samples the prefill's q|k|v projection runs on the persistent 256 x 256 tiles, whose epilogue writes the K / V columns straight
    into the KV-cache planes (csrc/gemm256.hpp, KV form); the 64-row tail of M = 64 x 257 is copied from the tensor, and attention reads K / V from
    the planes.  Option qkv_to_cache = 0 copies every row instead (kv_fill_rows_kernel), gemm256 = 1 takes the one-tile kernel (no KV form): the three
    must give the same cache, i.e. the same logits bit for bit over the prefill's token and 24 decode steps that read every cached position."""
    from meshanything_amd.engine import Engine
    B, n = 64, 24
    cfg = MAConfig.full(dtype=POLICIES[policy], max_batch=B)
    eng = Engine(cfg)
    load_weights_cached(eng, cfg, init=FULL_INIT)
    g = torch.Generator().manual_seed(11)
    prefix = (torch.randn(B, cfg.num_latents + 1, cfg.hidden, generator=g) * 0.5).cuda()
    assert eng.get_option("qkv_to_cache") == 1 and eng.get_option("gemm256") == 2
    ref = None
    try:
        for (to_cache, g256) in ((1, 2), (0, 2), (1, 1), (1, 2)):
            eng.set_option("qkv_to_cache", to_cache); eng.set_option("gemm256", g256)
            t, _, lg = eng.generate(prefix, max_new_tokens=n, suppress_eos=True, return_logits=True)
            if ref is None:
                ref = (t.clone(), lg.clone())
                assert_diverse(t, 24, "kv-to-cache reference stream")
                continue
            assert torch.equal(ref[0], t), f"tokens differ with qkv_to_cache={to_cache} gemm256={g256}"
            assert torch.equal(ref[1].view(torch.int32), lg.view(torch.int32)), f"logits differ with qkv_to_cache={to_cache} gemm256={g256}"
    finally:
        eng.set_option("qkv_to_cache", 1); eng.set_option("gemm256", 2)
    eng.close()


@pytest.mark.parametrize("policy,B", [("bf16", 64), ("fp16", 64), ("bf16", 16), ("bf16", 24), ("bf16", 8), ("fp16", 40), ("bf16", 72)])      # (72: two row groups, 64 + 8, the second at row 64 of the cache)
def test_prefill_last_rows_as_their_own_chain_equal_the_one_stream_form(golden_dir, policy, B):
    """Round 6: M = B x 257 leaves B rows behind the 256-row tiles -- the last B positions of the last sample, which no other row ever reads (causal
    attention).  With option prefill_tail (default 2: on a stream of the lowest priority; 1: default priority) they run all 24 layers as a chain of their own on a second stream, fed per layer with the main
    chain's K / V through one event, with the kernels the one-stream form gives them (csrc/engine_dense.hpp prefill, gemm256.hpp GemmTArgs::part).  The
    logits of the prefill's token and of decode steps that read every cached position -- the last sample's most of all -- must be the one-stream
    form's bit for bit (every stretch of rows gets the kernel the one-stream form gives it: the skinny GEMM behind 256-row tiles, the 128-row tiles in
    the whole problem's shape where that form runs everything on them -- out_proj at 16 / 24 samples), and bit-stable from run to run."""
    from meshanything_amd.engine import Engine
    n = 12
    cfg = MAConfig.full(dtype=POLICIES[policy], max_batch=B)
    eng = Engine(cfg)
    load_weights_cached(eng, cfg, init=FULL_INIT)
    g = torch.Generator().manual_seed(17)
    prefix = (torch.randn(B, cfg.num_latents + 1, cfg.hidden, generator=g) * 0.5).cuda()
    assert eng.get_option("prefill_tail") == 2
    runs = {}
    try:
        for mode in (2, 0, 1, 2):
            eng.set_option("prefill_tail", mode)
            t, _, lg = eng.generate(prefix, max_new_tokens=n, suppress_eos=True, return_logits=True)
            runs.setdefault(mode, []).append((t.clone(), lg.clone()))
    finally:
        eng.set_option("prefill_tail", 2)
    two, one = runs[2] + runs[1], runs[0][0]
    assert_diverse(one[0], 8, "one-stream reference stream")
    for t, lg in two[1:]:
        assert torch.equal(two[0][0], t) and torch.equal(two[0][1].view(torch.int32), lg.view(torch.int32)), "the two-stream prefill is not bit-stable from run to run"
    assert torch.equal(one[0], two[0][0]), "tokens differ between the one-stream and the two-stream prefill"
    assert torch.equal(one[1].view(torch.int32), two[0][1].view(torch.int32)), \
        f"logits differ between the one-stream and the two-stream prefill: max {float((one[1] - two[0][1]).abs().max()):.3e}"
    eng.close()


@pytest.mark.parametrize("policy", ["bf16", "fp16"])
def test_prefill_of_16_samples_with_fc2_split_along_k(golden_dir, policy):
    """Round 6: at 16 samples (M = 4 112) the prefill's fc2 -- N = 1024: 64 tiles of 256 x 256, each 64 K-tiles deep -- and its out_proj (16 K-tiles) run as
    FOUR partial sums along K (csrc/gemm256.hpp, GemmSplitK; option gemm_splitk, default 2 = both) that the LayerNorm behind each adds up (ln_rows2_kernel,
    KS form); q|k|v takes the persistent tiles at 0.75 round.
    The summation order along K differs from the unsplit kernel's, so the two are compared the way every 16-bit path is: each against the oracle along
    its own greedy stream, and against each other on the logits of the same forced stream."""
    from meshanything_amd.engine import Engine
    from oracle.meshanything_oracle import Oracle
    B, n = 16, 12
    cfg = MAConfig.full(dtype=POLICIES[policy], max_batch=B)
    env = Env.__new__(Env)
    env.cfg, env.policy = cfg, policy
    env.sd = cached_state_dict(cfg, init=FULL_INIT)
    env.oracle = Oracle(cfg, env.sd, policy, device=oracle_device())
    env.engine = eng = Engine(cfg)
    load_weights_cached(eng, cfg, init=FULL_INIT)
    x = mouse_variants(golden_dir, B)
    prefix = env.oracle.process_point_feature(env.oracle.encode_latents(x))
    assert eng.get_option("gemm_splitk") == 2
    try:
        toks, lengths, lg = eng.generate(prefix.cuda(), max_new_tokens=n, suppress_eos=True, return_logits=True)
        v = _check_greedy(env, prefix, toks, lengths, suppress_eos=True)
        assert all(r["ambiguous"] <= 2 for r in v), [r["ambiguous"] for r in v]
        eng.set_option("gemm_splitk", 0)
        t0, _, lg0 = eng.generate(prefix.cuda(), max_new_tokens=n, suppress_eos=True, forced_tokens=toks, return_logits=True)
        err = float((lg - lg0).abs().max())
        same = float((t0 == toks).float().mean())
        print(f"[{policy}] 16-sample prefill, out_proj and fc2 as 4 partial sums along K vs unsplit: max abs logit difference over {n} steps x {B} rows {err:.5f}, same picks {same * 100:.1f} %")
        assert err <= {"bf16": 3e-2, "fp16": 4e-3}[policy] and same >= 0.9
    finally:
        eng.set_option("gemm_splitk", 2)
    eng.close()


@pytest.mark.parametrize("policy", ["bf16", "fp16"])
def test_prefill_layernorm_finished_inside_the_gemm(golden_dir, policy):
    """Round 6 (measured, not kept; MA_EXPERIMENTAL=1 builds): at 64 samples the prefill's out_proj and fc2 (N = hidden: four 256 x 256 tiles per tile row) finish the LayerNorm that follows them in
    their own epilogue -- the four workgroups of a tile row exchange per-row moments through {epoch, value} granules (csrc/gemm256.hpp, LNF form) -- and the
    row kernel only handles the 64-row tail.  The moments are the row kernel's two-pass form summed in another (fixed) order, so the two paths are compared
    like every 16-bit path: rows of the batch against the oracle along their own greedy stream, both paths on the logits of the same forced stream, and the
    fused path against itself (its result must not depend on which workgroup publishes first)."""
    from meshanything_amd.engine import Engine
    from oracle.meshanything_oracle import Oracle, verify_greedy_stream
    B, n = 64, 10
    cfg = MAConfig.full(dtype=POLICIES[policy], max_batch=B)
    sd = cached_state_dict(cfg, init=FULL_INIT)
    oracle = Oracle(cfg, sd, policy, device=oracle_device())
    eng = Engine(cfg)
    load_weights_cached(eng, cfg, init=FULL_INIT)
    x = mouse_variants(golden_dir, B)
    prefix = torch.cat([oracle.process_point_feature(oracle.encode_latents(x[i:i + 16])) for i in range(0, B, 16)])
    if not eng.get_option("experimental"):
        pytest.skip("LayerNorm inside the GEMM epilogue was measured and not kept: MA_EXPERIMENTAL=1 builds only (profiles/r06_ab_layernorm_in_gemm.txt)")
    eng.set_option("fuse_ln", 1)
    if eng.get_option("fuse_ln") != 1:
        pytest.skip("the in-launch exchanges are not in use on this device")
    try:
        toks, lengths, lg = fused_generate(eng, f"{policy} prefill with fused LayerNorm", prefix.cuda(), max_new_tokens=n, suppress_eos=True, return_logits=True)
        t2, _, lg2 = fused_generate(eng, f"{policy} prefill with fused LayerNorm, second run", prefix.cuda(), max_new_tokens=n, suppress_eos=True, return_logits=True)
        assert torch.equal(toks, t2) and torch.equal(lg.view(torch.int32), lg2.view(torch.int32)), "the fused LayerNorm is not bit-stable from launch to launch"
        for b in (0, 21, 42, 63):                                    # (63: its last 64 rows are the tail the row kernel normalises)
            v = verify_greedy_stream(oracle, prefix[b:b + 1], toks[b, :int(lengths[b])].cpu(), GREEDY_TOL[policy], True)
            assert v["hard"] == [] and v["ambiguous"] <= 2, (b, v)
        eng.set_option("fuse_ln", 0)
        t0, _, lg0 = eng.generate(prefix.cuda(), max_new_tokens=n, suppress_eos=True, forced_tokens=toks, return_logits=True)
        err = float((lg - lg0).abs().max())
        same = float((t0 == toks).float().mean())
        print(f"[{policy}] 64-sample prefill, LayerNorm inside out_proj / fc2 vs the row kernel: max abs logit difference over {n} steps x {B} rows {err:.5f}, same picks {same * 100:.1f} %")
        assert err <= {"bf16": 3e-2, "fp16": 4e-3}[policy] and same >= 0.9
    finally:
        eng.set_option("fuse_ln", 0)
    eng.close()
