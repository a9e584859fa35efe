"""The kernel tuning switches are per engine: gemv_rpw, gemv_small_rows, gemv_k8_ksplit, mfma_chunks, gemm256 and gemm_variant set on one engine change
nothing that another engine of the process reads back or launches -- not its captured steps, not its eager launches, not a step it captures afterwards.

The shape is the smallest at which the GEMV switches select anything (gemv.hpp gemv_shape: K a multiple of 512 in bf16, gemv_rpw from 2048 rows on):
hidden 512, vocabulary 2051 -- the lm_head runs 8 rows per block at gemv_rpw = 4 and 4 at gemv_rpw = 1, so the pick reads 257 or 513 partial maxima
(n_parts) -- and ffn 4096 (fc2: the K = 8 pieces case of gemv_k8_ksplit).  Hidden 512 keeps the step on the plain five-launch GEMV chain."""
import ctypes as C

import pytest
import torch

from meshanything_amd import _lib
from meshanything_amd.config import MAConfig, DTYPE_BF16
from conftest import cached_state_dict

DEFAULTS = {"gemv_rpw": 4, "gemv_small_rows": 1, "gemv_k8_ksplit": 1, "mfma_chunks": 8, "gemm256": 2, "gemm_variant": 6}
OTHER = {"gemv_rpw": 1, "gemv_small_rows": 2, "gemv_k8_ksplit": 4, "mfma_chunks": 4, "gemm256": 0, "gemm_variant": 0}      # accepted, not the default


def test_the_engine_less_gemm_checks_its_switches_like_the_options():
    """ma_op_gemm_bf16_tuned takes gemm_variant and gemm256 as arguments and refuses what ma_engine_set_option refuses, with the same code and
    message -- before anything is launched, so this needs no GPU (M = 0: an accepted pair launches nothing either)."""
    lib = _lib.load()
    buf = (C.c_char * 64)()
    p, z = C.cast(buf, C.c_void_p), C.c_void_p(0)

    def call(variant, tile256):
        return lib.ma_op_gemm_bf16_tuned(p, 32, p, z, z, 0, z, 0, p, 32, 0, 32, 32, 0, variant, tile256, z), lib.ma_last_error(None).decode()
    for tile256 in (-1, 3):
        rc, msg = call(6, tile256)
        assert rc == -1 and "gemm256: 0 (128-row tiles), 1 (one tile per workgroup) or 2 (1 + the persistent form)" in msg, (tile256, rc, msg)
    for tile256 in (0, 1, 2):
        assert call(6, tile256)[0] == 0, tile256
    rc, msg = call(0, 2)
    if _lib.LIB_PATH.endswith("_exp.so"):
        assert rc == 0, msg
    else:
        assert rc == -3 and "gemm_variant: the A/B tile variants need a library built with MA_EXPERIMENTAL=1" in msg, (rc, msg)


@pytest.mark.gpu
def test_options_set_on_one_engine_leave_the_other_alone():
    from meshanything_amd.engine import Engine
    cfg = MAConfig.tiny(hidden=512, heads=8, codebook_dim=512, codebook_size=2048, ffn=4096, dtype=DTYPE_BF16, max_batch=2)
    a, b = Engine(cfg), None
    try:
        a.load_weights(cached_state_dict(cfg, init="diverse").items())
        g = torch.Generator().manual_seed(23)
        d = torch.randn(1, cfg.n_points, 3, generator=g)
        d = d / d.norm(dim=-1, keepdim=True)
        cloud = torch.cat([d * (0.3 + 0.7 * torch.rand(1, cfg.n_points, 1, generator=g)), d], -1)
        _, prefix = a.encode(cloud.cuda())
        want_tokens, _, want_logits = a.generate(prefix, suppress_eos=True, return_logits=True)
        want_tokens, want_bits = want_tokens.cpu(), want_logits.view(torch.int32).cpu()
        assert want_tokens.shape == (1, cfg.max_new_tokens) and cfg.max_new_tokens == 74
        assert len(set(want_tokens[0].tolist())) > 8, "a generation that repeats one token would not notice a truncated argmax"

        b = Engine(MAConfig.tiny())
        stored = {name: v for name, v in OTHER.items() if name != "gemm_variant" or b.get_option("experimental")}
        for name, v in stored.items():
            b.set_option(name, v)
            assert b.get_option(name) == v, name
        for name, default in DEFAULTS.items():
            assert a.get_option(name) == default, name

        def same(what):
            tokens, _, logits = a.generate(prefix, suppress_eos=True, return_logits=True)
            assert torch.equal(tokens.cpu(), want_tokens), what
            assert torch.equal(logits.view(torch.int32).cpu(), want_bits), what
        same("the captured step, replayed")
        a.set_option("use_graph", 0)
        same("eager launches")
        a.set_option("use_graph", 1)
        same("a step captured after the other engine's options were set")

        # the converse: A's own gemv_rpw moves the lm_head's rows between blocks without changing any sum's order, and stays A's
        a.set_option("gemv_rpw", 1)
        tokens, _ = a.generate(prefix, suppress_eos=True)
        assert torch.equal(tokens.cpu(), want_tokens)
        assert a.get_option("gemv_rpw") == 1
        for name, v in stored.items():
            assert b.get_option(name) == v, name
    finally:
        a.close()
        if b is not None:
            b.close()
