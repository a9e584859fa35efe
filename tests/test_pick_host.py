"""Token pick, sampler and coordinate argmax, host side: the argument checks of ma_op_pick / ma_op_coords_argmax (which all come before
anything touches a device), and tests/pick_ref.py -- the float64 restatement the GPU tests (test_gpu_pick.py) compare the kernels with --
against the oracle's own, independently written, filter and draw.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import pick_ref as R
from meshanything_amd import _lib, build

INVALID = -1
P = C.c_void_p(16)                                                 # a non-null pointer that is never dereferenced


@pytest.fixture(scope="module")
def lib():
    build.build(force=False, verbose=False)
    return _lib.load()


def _pick_args(**kw):
    a = dict(logits=P, B=4, V=61, part_val=None, part_idx=None, nparts=0, do_sample=0, top_k=50, top_p=0.95, suppress_eos=0, uniforms=None, seed=0,
             t=0, max_new=1, forced=None, finished=P, tokens=P, cur_tok=P, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def test_pick_refuses_bad_arguments_on_the_host(lib):
    pick = lib.ma_op_pick
    for name in ("logits", "finished", "tokens", "cur_tok"):
        assert pick(*_pick_args(**{name: None})) == INVALID
        assert b"null" in lib.ma_last_error(None)
    bad = [dict(B=0), dict(B=-3), dict(B=65536), dict(V=2), dict(V=0), dict(V=-1),
           dict(V=11265), dict(V=1 << 30),                          # the sampler's LDS stage (validate_config: codebook_size + 3 <= 11264)
           dict(nparts=-1), dict(nparts=62, part_val=P, part_idx=P), dict(nparts=8), dict(nparts=8, part_val=P), dict(nparts=8, part_idx=P),
           dict(t=-1), dict(max_new=0), dict(max_new=-2),
           dict(do_sample=1, top_k=0), dict(do_sample=1, top_k=-1), dict(do_sample=1, top_k=65),
           dict(do_sample=1, top_p=0.0), dict(do_sample=1, top_p=-0.5), dict(do_sample=1, top_p=1.0000001), dict(do_sample=1, top_p=float("nan")),
           dict(do_sample=1, uniforms=P, t=1, max_new=1), dict(do_sample=1, uniforms=P, t=7, max_new=4)]
    for kw in bad:
        assert pick(*_pick_args(**kw)) == INVALID, kw
        assert b"ma_op_pick" in lib.ma_last_error(None)
    assert pick(*_pick_args(V=11265)) == INVALID and b"LDS" in lib.ma_last_error(None)
    assert pick(*_pick_args(do_sample=1, top_k=65)) == INVALID and b"top_k must be in [1,64]" in lib.ma_last_error(None)
    assert pick(*_pick_args(do_sample=1, top_p=0.0)) == INVALID and b"top_p must be in (0,1]" in lib.ma_last_error(None)


def test_coords_argmax_refuses_bad_arguments_on_the_host(lib):
    ca = lib.ma_op_coords_argmax
    good = [P, 5, 128, P, P, None]
    for i in (0, 3, 4):
        args = list(good)
        args[i] = None
        assert ca(*args) == INVALID
        assert b"null" in lib.ma_last_error(None)
    for i, v in [(1, 0), (1, -1), (1, (1 << 24) + 1), (2, 0), (2, -7)]:
        args = list(good)
        args[i] = v
        assert ca(*args) == INVALID, (i, v)
        assert b"ma_op_coords_argmax" in lib.ma_last_error(None)


def test_hash_uniform_restatement_is_pinned():
    """The hashed stream decides every sampled token: values of the Python restatement written down once (test_gpu_pick.py holds the kernel
    to the restatement), and the properties the sampler relies on."""
    known = {(0, 0, 0): 0.0, (1, 0, 0): 0.33816659450531006, (0x5EED, 3, 17): 0.23232805728912354, (2 ** 64 - 1, 63, 7201): 0.7783395051956177,
             (123456789, 1, 1): 0.268526554107666}
    for (seed, row, t), want in known.items():
        assert R.hash_uniform(seed, row, t) == want, (seed, row, t, repr(R.hash_uniform(seed, row, t)))
    u = np.array([R.hash_uniform(7, r, t) for r in range(64) for t in range(64)])
    assert u.min() >= 0.0 and u.max() < 1.0 and np.all(u * 2 ** 24 == np.round(u * 2 ** 24))
    assert len(set(u.tolist())) == u.size and abs(u.mean() - 0.5) < 0.02


def test_reference_agrees_with_the_oracle_filter_and_draw():
    """pick_ref (float64, numpy) and Oracle.topk_topp_filter / sample_from (float32, torch) are two restatements of the same warpers: on rows
    without ties, and draws whose margin is far above float32 rounding, they keep the same tokens and draw the same one."""
    from oracle.meshanything_oracle import Oracle
    rng = np.random.default_rng(5)
    n = 0
    for V, scale, k, top_p in [(61, 1.0, 50, 0.95), (61, 3.0, 61, 0.95), (300, 1.0, 50, 0.95), (300, 3.0, 7, 0.5), (8195, 1.0, 50, 0.95), (8195, 3.0, 64, 0.8),
                               (8195, 1.0, 1, 0.95), (300, 3.0, 50, 1.0)]:
        x = (rng.standard_normal(V) * scale).astype(np.float32)
        kept, probs = Oracle.topk_topp_filter(torch.from_numpy(x), k, top_p)
        idx, sc = R.candidates(x, k)
        for u in rng.random(12).astype(np.float32):
            tok, margin, alt = R.draw(idx, sc, top_p, u)
            if margin < 1e-4:
                continue
            n += 1
            assert tok == Oracle.sample_from(kept, probs, float(u)), (V, scale, k, top_p, u)
            assert tok in kept.tolist()
        # the kept set itself, read off the reference through draws at u = 1 (the last kept rank) when the cut is clear
        last, margin, _ = R.draw(idx, sc, top_p, 1.0)
        if margin >= 1e-4:
            assert last == int(kept[-1])
    assert n >= 60
    # greedy is torch.argmax with the lowest index among equals
    for _ in range(20):
        x = rng.integers(-3, 4, 40).astype(np.float32)
        assert R.greedy(x) == int(torch.argmax(torch.from_numpy(x)))
        y = x.copy()
        y[R.EOS] = -np.inf
        assert R.greedy(x, True) == int(torch.argmax(torch.from_numpy(y)))


def test_reference_on_hand_worked_rows():
    """Small cases worked by hand: ties at the k-th score stay, at most 64 survive in (score, index) order, the top-p cut, the fall-through."""
    x = np.array([0.0, 5.0, 1.0, 1.0, 1.0, -2.0], np.float32)
    idx, sc = R.candidates(x, 3)
    assert idx.tolist() == [1, 2, 3, 4] and sc.tolist() == [5.0, 1.0, 1.0, 1.0]      # three scores tie at the 2nd .. 4th place: all stay
    assert R.candidates(x, 3, suppress_eos=True)[0].tolist() == [2, 3, 4]
    idx, _ = R.candidates(np.zeros(100, np.float32), 10)
    assert idx.tolist() == list(range(64))
    x = np.full(200, -1.0, np.float32)
    x[[150, 20]] = 2.0
    idx, _ = R.candidates(x, 50)
    assert idx.tolist() == [20, 150] + list(range(20)) + list(range(21, 63))
    # masses 1/2, 1/4, 1/8, 1/8: top_p = 0.8 drops tails 1/8 (<= 0.2) and keeps 1/4 (tail 1/4 + 1/8 > 0.2) -> three kept, renormalised 4/7, 2/7, 1/7
    x = np.log(np.array([0.5, 0.25, 0.125, 0.125])).astype(np.float32)
    assert R.sample(x, 4, 0.8, 0.5)[0] == 0 and R.sample(x, 4, 0.8, 0.6)[0] == 1 and R.sample(x, 4, 0.8, 0.9)[0] == 2 and R.sample(x, 4, 0.8, 1.0)[0] == 2
    assert R.sample(x, 4, 1.0, 0.9)[0] == 3 and R.sample(x, 4, 0.4, 0.99)[0] == 0
    tok, margin, alt = R.sample(x, 4, 0.8, 4 / 7 + 1e-6)
    assert tok == 1 and margin < 2e-6 and alt == 0
    tok, margin, alt = R.sample(x, 4, 0.75 - 1e-6, 0.99)          # tail 1/4 is within 1e-6 of 1 - top_p: the other outcome keeps a candidate fewer
    assert margin < 2e-6 and {tok, alt} == {1, 2}
    assert R.greedy(np.array([1.0, 9.0, 9.0, 3.0])) == 1 and R.greedy(np.array([1.0, 9.0, 9.0, 3.0]), suppress_eos=True) == 2
    assert R.step([0.0, 9.0, 1.0, 2.0], finished=True) == (R.PAD, R.PAD, True)
    assert R.step([0.0, 9.0, 1.0, 2.0]) == (1, 1, True)
    assert R.step([0.0, 9.0, 1.0, 2.0], forced=77) == (1, 3, False)
    assert R.step([0.0, 9.0, 1.0, 2.0], t=1, max_new=1, forced=0) == (None, 1, True)
    c = R.coords(np.array([[0, 3, 3], [np.nan, -1, -2]] * 9, np.float32), [1, 0])      # (a NaN logit is no candidate)
    assert c.dtype == np.float32 and c[:9].tolist() == [float(np.float32(1) / np.float32(3) - np.float32(0.5))] * 9
    assert np.all(np.isnan(c[9:]))
