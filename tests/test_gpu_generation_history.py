"""A generation must not depend on what earlier generations left in the engine (MI355X).

The KV planes, the q|k|v / attention workspaces and the exchange granules of an engine outlive a generation.  A request whose prefix is
all NaN (or all +inf) fills every one of them with non-finite values; the next, clean request on the same engine must give the tokens and
the logits of a clean engine bit for bit, and finite logits.  What this pins:

* the two-stream prefill (csrc/engine_dense.hpp prefill, option prefill_tail): the main chain's attention must not read the positions of
  the last sample that the tail chain owns -- a masked probability is exactly 0, and 0 x NaN from the previous generation is NaN in a
  valid row;
* the fused decode launches (csrc/qkv_attn.hpp, rows_attn.hpp) and the final-form decode attention: positions beyond the current length
  hold the previous generation's values and must be zeroed before the value sum, not only masked in the score;
* the shrinking batch: poison at 16 samples, clean at 8, so that the clean run's last sample sits in the middle of poisoned planes.

The stale read of the prefill was a race between two streams: every case repeats poison + clean a fixed three times per poison value.
"""
import pytest
import torch

from meshanything_amd.config import MAConfig, DTYPE_BF16, DTYPE_F16, DTYPE_F32
from conftest import load_weights_cached

pytestmark = pytest.mark.gpu

POLICIES = {"fp32": DTYPE_F32, "bf16": DTYPE_BF16, "fp16": DTYPE_F16}
FULL_INIT = "diverse"
N_CLEAN, N_POISON, REPEATS = 12, 16, 3


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def _history(eng, prefix, poison_batch, what):
    """g0 = clean run; then REPEATS x (poison run, clean run) for NaN and for +inf; every clean run must be g0 bit for bit and finite."""
    def clean():
        t, _, lg = eng.generate(prefix, max_new_tokens=N_CLEAN, suppress_eos=True, return_logits=True)
        return t.clone(), lg.clone()
    g0 = clean()
    assert bool(torch.isfinite(g0[1]).all()), f"{what}: the first clean run has non-finite logits"
    for name, value in (("nan", float("nan")), ("inf", float("inf"))):
        bad = torch.full((poison_batch,) + tuple(prefix.shape[1:]), value, device="cuda")
        for rep in range(REPEATS):
            out = eng.generate(bad, max_new_tokens=N_POISON, suppress_eos=True, return_logits=True)      # must return; its tokens mean nothing
            assert out[0].shape[0] == poison_batch
            g1 = clean()
            finite = torch.isfinite(g1[1])
            assert bool(finite.all()), (f"{what}: after a {name} generation (repeat {rep}) the clean run has {int((~finite).sum())} non-finite logits, "
                                        f"samples {sorted(set((~finite).nonzero()[:, 0].tolist()))}")
            assert _same(g0, g1), (f"{what}: after a {name} generation (repeat {rep}) the clean run differs from the first one: "
                                   f"{int((g0[0] != g1[0]).sum())} tokens, max logit difference {float((g0[1] - g1[1]).abs().max()):.3e}")


@pytest.mark.parametrize("policy,B", [("bf16", 1), ("fp32", 1), ("fp32", 4), ("bf16", 8), ("fp16", 8), ("bf16", 16), ("fp16", 16), ("bf16", 64)])
def test_clean_generation_after_a_poisoned_one_equals_the_first(policy, B):
    from meshanything_amd.engine import Engine
    cfg = MAConfig.full(dtype=POLICIES[policy], max_batch=B)
    eng = Engine(cfg)
    load_weights_cached(eng, cfg, init=FULL_INIT)
    g = torch.Generator().manual_seed(23)
    prefix = (torch.randn(B, cfg.num_latents + 1, cfg.hidden, generator=g) * 0.5).cuda()
    two_stream = policy != "fp32" and B >= 8                       # where option prefill_tail changes what runs
    assert eng.get_option("prefill_tail") == 2
    try:
        for mode in ((2, 0) if two_stream else (2,)):
            eng.set_option("prefill_tail", mode)
            _history(eng, prefix, B, f"{policy} B={B} prefill_tail={mode}")
            if (policy, B) == ("bf16", 16):                        # the shrinking batch: poison at 16, clean at 8
                _history(eng, prefix[:8].contiguous(), 16, f"{policy} poison B=16, clean B=8, prefill_tail={mode}")
    finally:
        eng.set_option("prefill_tail", 2)
    eng.close()
