"""The token pick / sampler (csrc/misc.hpp pick_kernel, through ma_op_pick) and the detokenizer's coordinate argmax (coords_argmax_kernel,
through ma_op_coords_argmax) on logits made for the purpose, against the float64 restatement tests/pick_ref.py.  With chosen logits
every answer is exact: no "ambiguous step" allowance, except where the statistical test states one and bounds it.

Every row of a batch is different (its own noise, its own planted values), so a workgroup that read another row's logits, partials,
uniforms or state record fails."""
import ctypes as C

import numpy as np
import pytest
import torch

import pick_ref as R

pytestmark = pytest.mark.gpu

VS = [61, 257, 8192, 8195]
NINF = np.float32(-np.inf)


@pytest.fixture(scope="module")
def lib():
    from meshanything_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return _lib.load()


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def pick(lib, logits, *, parts=None, do_sample=False, top_k=50, top_p=0.95, suppress_eos=False, uniforms=None, seed=0, t=0, max_new=1, finished=None,
         forced=None, fill=-7):
    """One ma_op_pick launch over the rows of `logits` (B, V): (tokens (B, max_new) with `fill` where nothing was written, fed token (B), finished (B))."""
    from meshanything_amd import _lib
    logits = np.asarray(logits, np.float32)
    B, V = logits.shape
    d_log = _dev(logits, np.float32)
    pv = pi = None
    nparts = 0
    if parts is not None:
        pv, pi = _dev(parts[0], np.float32), _dev(parts[1], np.int32)
        nparts = parts[0].shape[1]
        assert parts[0].shape == parts[1].shape == (B, nparts)
    d_u = _dev(uniforms, np.float32)
    d_forced = _dev(forced, np.int64)
    assert uniforms is None or np.shape(uniforms) == (B, max_new)
    assert forced is None or np.shape(forced) == (B, max_new)
    d_fin = _dev(np.zeros(B) if finished is None else finished, np.int32)
    d_tok = torch.full((B, max_new), fill, dtype=torch.int64, device="cuda")
    d_cur = torch.full((B,), -9, dtype=torch.int32, device="cuda")
    rc = lib.ma_op_pick(_p(d_log), B, V, _p(pv), _p(pi), nparts, int(do_sample), top_k, top_p, int(suppress_eos), _p(d_u), seed, t, max_new, _p(d_forced),
                        _p(d_fin), _p(d_tok), _p(d_cur), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, None)
    return d_tok.cpu().numpy(), d_cur.cpu().numpy(), d_fin.cpu().numpy()


def _noise(rng, V, lo=-2.0, hi=-1.0):
    return rng.uniform(lo, hi, V).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- greedy
def _greedy_rows(V):
    """Rows whose argmax sits where the sweep can go wrong: the 32 x 256 preload and its tail (8192 ..), the clamped preload of a short row
    (V - 1), lanes / waves / thread 0 of the reduction, equal maxima across those boundaries, eos, -inf, signed zeros."""
    rng = np.random.default_rng(1000 + V)
    rows = []

    def planted(at, value=1.0, base=None):
        x = _noise(rng, V) if base is None else base
        for i in at:
            x[i] = value
        rows.append(x)

    for i in [0, 1, 2, 255, 256, V - 1, 8191, 8192, 8193, 8194, 63, 64, V - 2]:
        if i < V:
            planted([i])
    for tie in [(63, 64), (255, 256), (8190, 8193), (0, V - 1), (V - 2, V - 1), (2, 256), (63, 64, 256), (8191, 8192, 8194), (255, 8192, 8193), (1, 2), (1, V - 1),
                (1, 60, 61)]:
        if max(tie) < V:
            planted(tie)
    planted([R.EOS], 3.0, base=np.where(np.arange(V) == V - 1, np.float32(2.0), _noise(rng, V)).astype(np.float32))      # eos on top, the runner-up at V - 1
    planted([R.EOS], 3.0, base=np.where(np.arange(V) == 8192 % V, np.float32(2.0), _noise(rng, V)).astype(np.float32))
    rows.append(np.full(V, 0.5, np.float32))                                   # all equal
    x = np.full(V, 0.25, np.float32)
    x[0] = 0.0
    rows.append(x)                                                             # all equal behind a lower index 0: eos, or 2 when suppressed
    for i in [V - 1, 7, 256 % V]:
        planted([i], -5.0, base=np.full(V, NINF, np.float32))                  # all -inf except one entry
    rows.append(_noise(rng, V, -1000.0, -1.0))                                 # negative only
    rows.append(_noise(rng, V, -1e30, -1e20))
    for a, b in [(5, V - 1), (V - 3, 9), (V - 1, V - 2)]:                            # +0 and -0 are one value: the lower index wins whatever its sign
        x = _noise(rng, V)
        x[a], x[b] = np.float32(0.0), np.float32(-0.0)
        rows.append(x)
    return np.stack(rows)


def _partials(rows, rpb, suppress_eos):
    """What the lm_head GEMV's EPI_LMHEAD epilogue leaves: per block of `rpb` logits the largest value and its lowest index, eos left out
    when suppressed (a block with nothing left: -inf, INT_MAX)."""
    B, V = rows.shape
    n = -(-V // rpb)
    pv = np.full((B, n), NINF, np.float32)
    pi = np.full((B, n), 0x7fffffff, np.int32)
    for b in range(B):
        for k in range(n):
            best = None
            for i in range(k * rpb, min(V, (k + 1) * rpb)):
                if suppress_eos and i == R.EOS:
                    continue
                if best is None or rows[b, i] > rows[b, best]:
                    best = i
            if best is not None:
                pv[b, k], pi[b, k] = rows[b, best], best
    return pv, pi


_GREEDY = {}


def _greedy_case(V):
    if V not in _GREEDY:
        rows = _greedy_rows(V)
        ref = {s: np.array([R.greedy(r, s) for r in rows]) for s in (False, True)}
        _GREEDY[V] = (rows, ref)
    return _GREEDY[V]


@pytest.mark.parametrize("suppress", [False, True], ids=["eos_allowed", "eos_suppressed"])
@pytest.mark.parametrize("V", VS)
def test_greedy_plain_logits(lib, V, suppress):
    """nparts = 0: the sweep over the logits themselves (matrix-core batches).  Exact, every row."""
    rows, ref = _greedy_case(V)
    want = ref[suppress]
    n = rows.shape[0]
    assert n <= 64
    sel64 = np.arange(64) % n                                                  # B = 64: every case, some twice
    for sel in (sel64, np.arange(n)[::-1][:5], np.array([n - 1 - (V % n)])):   # B = 64, 5, 1
        tok, cur, fin = pick(lib, rows[sel], suppress_eos=suppress)
        assert tok[:, 0].tolist() == want[sel].tolist(), (V, suppress, np.flatnonzero(tok[:, 0] != want[sel]))
        assert cur.tolist() == want[sel].tolist()
        assert fin.tolist() == (want[sel] == R.EOS).astype(int).tolist()
    if not suppress:                                                           # the cases are what they claim to be
        assert R.EOS in want and (V - 1) in want and 0 in want
    else:
        assert R.EOS not in want


@pytest.mark.parametrize("suppress", [False, True], ids=["eos_allowed", "eos_suppressed"])
@pytest.mark.parametrize("V,rpb", [(61, 16), (257, 4), (257, 1), (8192, 16), (8195, 16), (8195, 3)])
def test_greedy_partials(lib, V, rpb, suppress):
    """nparts > 0: the reduction of the lm_head's per-block partials (hand-built here, as its epilogue leaves them: ties between blocks, eos
    left out when suppressed, more partials than threads at rpb = 3).  Must equal the plain-logit sweep and the reference."""
    rows, ref = _greedy_case(V)
    want = ref[suppress]
    n = rows.shape[0]
    parts = _partials(rows, rpb, suppress)
    for sel in (np.arange(64) % n, np.arange(5) * 3 % n):
        tok, cur, _ = pick(lib, rows[sel], parts=(parts[0][sel], parts[1][sel]), suppress_eos=suppress)
        plain, _, _ = pick(lib, rows[sel], suppress_eos=suppress)
        assert tok[:, 0].tolist() == want[sel].tolist()
        assert tok[:, 0].tolist() == plain[:, 0].tolist() == cur.tolist()


# ---------------------------------------------------------------------------------------------------------------- sampler, crafted rows
MARGIN_CRAFTED = 1e-3
U_LAST = float(np.float32(1.0) - np.float32(2.0 ** -24))                      # the largest float32 below 1


def _check_crafted(lib, rows, k, top_p, suppress=False, us=None, want_special=(), seed=0, launches=1):
    """Every row at the uniforms 0, just below 1, 1.0 and a few in between -- those of them that leave every decision of the reference at
    least MARGIN_CRAFTED away (`want_special`: the ones this case is there for, which must be among them on every row).  Exact."""
    rows = np.asarray(rows, np.float32)
    B, V = rows.shape
    rng = np.random.default_rng(seed)
    cands = [R.candidates(r, k, suppress) for r in rows]
    T = 8
    U = np.zeros((B, T), np.float32)
    want = np.zeros((B, T), np.int64)
    for b in range(B):
        pool = list(us if us is not None else [0.0, U_LAST, 1.0]) + rng.random(400).astype(np.float32).tolist()
        got = []
        for u in pool:
            tok, margin, _ = R.draw(*cands[b], top_p, u)
            if margin >= MARGIN_CRAFTED:
                got.append((np.float32(u), tok))
            if len(got) == T:
                break
        assert len(got) == T, f"row {b}: not enough clear draws -- the row is not what this case needs"
        for s in want_special:
            assert np.float32(s) in [g[0] for g in got], (b, s)
        U[b] = [g[0] for g in got]
        want[b] = [g[1] for g in got]
    first = None
    for _ in range(launches):
        out = np.stack([pick(lib, rows, do_sample=True, top_k=k, top_p=top_p, suppress_eos=suppress, uniforms=U, t=t, max_new=T)[0][:, t] for t in range(T)], 1)
        assert np.array_equal(out, want), (np.argwhere(out != want)[:8].tolist(), out[out != want][:8], want[out != want][:8])
        first = out if first is None else first
        assert np.array_equal(out, first)
    return cands, want


def _clear_rows(make, n, k, top_p, suppress=False):
    """n rows from make(i), i = 0, 1, ..., skipping those whose top-p cut is closer than MARGIN_CRAFTED to 1 - top_p."""
    rows, i = [], 0
    while len(rows) < n:
        x = make(i)
        i += 1
        assert i < 50 * n
        if R.sample(x, k, top_p, 0.5, suppress)[1] >= MARGIN_CRAFTED or R.draw(*R.candidates(x, k, suppress), top_p, 0.5)[2] is None:
            rows.append(x)
    return np.stack(rows)


def test_sampler_k1_and_ties_at_the_top(lib):
    rng = np.random.default_rng(11)
    rows = np.stack([_noise(rng, 8195) for _ in range(5)])
    for b, i in enumerate([0, 8194, 8192, 255, 4097]):
        rows[b, i] = 1.0
    _, want = _check_crafted(lib, rows, 1, 0.95, us=[0.0, 1.0, U_LAST], want_special=[0.0, 1.0, U_LAST])
    assert want[:, 0].tolist() == [0, 8194, 8192, 255, 4097]
    rows[0, R.EOS] = 2.0                                                       # suppressed eos above the winner
    _check_crafted(lib, rows, 1, 0.95, suppress=True)
    rows[:, [70, 8193]] = 1.5                                                  # k = 1 with two equal best scores: both stay, half each
    cands, want = _check_crafted(lib, rows, 1, 1.0, suppress=True, want_special=[0.0, 1.0])
    assert all(c[0].tolist() == [70, 8193] for c in cands) and set(want.ravel().tolist()) == {70, 8193}


def test_sampler_k_equals_v_with_suppressed_eos(lib):
    """V = 61, top_k = 61: every logit is a candidate, the suppressed eos among them with mass 0 (-inf through the radix keys)."""
    rng = np.random.default_rng(12)
    rows = _clear_rows(lambda i: (rng.standard_normal(61) * 1.5).astype(np.float32), 64, 61, 0.95, True)
    rows[::2, R.EOS] = 9.0                                                     # eos would dominate if it were not suppressed
    cands, want = _check_crafted(lib, rows, 61, 0.95, suppress=True)
    assert all(len(c[0]) == 61 and c[0][-1] == R.EOS for c in cands) and R.EOS not in want
    # top_k above V is V
    assert np.array_equal(pick(lib, rows, do_sample=True, top_k=64, top_p=0.95, suppress_eos=True, uniforms=np.full((64, 1), 0.3))[0],
                          pick(lib, rows, do_sample=True, top_k=61, top_p=0.95, suppress_eos=True, uniforms=np.full((64, 1), 0.3))[0])


@pytest.mark.parametrize("k", [50, 64])
def test_sampler_8195(lib, k):
    rng = np.random.default_rng(13 + k)

    def make(i):
        x = (rng.standard_normal(8195) * 2).astype(np.float32)
        if i % 2 == 0:
            x[[8192, 8193, 8194]] = [7.0, 6.5, 6.0]                            # candidates in the tail of the row
        return x

    rows = _clear_rows(make, 5, k, 0.95)
    cands, want = _check_crafted(lib, rows, k, 0.95)
    assert all(len(c[0]) == k for c in cands) and any(8194 in c[0] for c in cands)


@pytest.mark.parametrize("V", [257, 8195])
def test_sampler_ties_at_the_kth_score_fill_up_to_64(lib, V):
    """top_k = 50 with 45 scores above the threshold and 6 .. 19 equal ones at it: 51 .. 64 candidates, all kept."""
    rng = np.random.default_rng(14)

    def make(n_eq, i):
        x = _noise(rng, V, -9.0, -8.0)
        at = rng.permutation(V)[:45 + n_eq]
        x[at[:45]] = np.linspace(1.0, 2.0, 45, dtype=np.float32) + np.float32(0.013 * i)      # (i: until the top-p cut of the second part is clear)
        x[at[45:]] = 0.75
        return x

    rows = [_clear_rows(lambda i: make(n_eq, i), 1, 50, 0.9)[0] for n_eq in (6, 10, 15, 18, 19)]
    cands, _ = _check_crafted(lib, np.stack(rows), 50, 1.0, want_special=[1.0], launches=3)
    assert [len(c[0]) for c in cands][:4] == [51, 55, 60, 63] and len(cands[4][0]) == 64
    _check_crafted(lib, np.stack(rows), 50, 0.9)


def test_sampler_last_radix_pass_decides(lib):
    """Candidates that differ in the lowest 8 bits of the float only (200 logits share their upper 24 bits), positive and negative."""
    rng = np.random.default_rng(15)
    rows = []
    for base in (0x40400000, 0xC0400000, 0x3F800000, 0x00800000, 0x80800000):
        x = _noise(rng, 8195, -9.0, -8.0) if base < 0x80000000 else _noise(rng, 8195, -90.0, -80.0)
        at = rng.permutation(8195)[:200]
        low = rng.permutation(256)[:200].astype(np.uint32)
        x[at] = (np.uint32(base) + low).view(np.float32)
        rows.append(x)
    rows = np.stack(rows)
    cands, _ = _check_crafted(lib, rows, 50, 0.95)
    for b, (idx, sc) in enumerate(cands):
        assert len(idx) == 50 and len(set(sc.astype(np.float32).view(np.uint32) >> 8)) == 1
    _check_crafted(lib, rows, 7, 1.0, want_special=[1.0])


def test_sampler_mixed_signs_and_signed_zeros(lib):
    rng = np.random.default_rng(16)

    def make(i):
        x = -np.abs(rng.standard_normal(257)).astype(np.float32) * 2 - np.float32(0.01)
        x[rng.permutation(257)[:10]] = rng.uniform(0.01, 3.0, 10).astype(np.float32)      # ten positive scores: the 50th largest is negative
        return x

    rows = _clear_rows(make, 5, 50, 0.95)
    cands, _ = _check_crafted(lib, rows, 50, 0.95)
    assert all(c[1][0] > 0 > c[1][-1] for c in cands)
    # huge magnitudes of both signs: the order of the keys, not the masses, is what this checks (one candidate carries all the mass)
    x = (rng.standard_normal((5, 8195)) * 1e30).astype(np.float32)
    _check_crafted(lib, x, 50, 0.95)
    # +0 and -0 are one score: with the 4th largest a zero, every zero of either sign is at the threshold and stays
    rows = []
    for b in range(5):
        x = _noise(rng, 61, -3.0, -2.0)
        x[[20 + b, 40, 8]] = [1.0, 1.0, 0.5]
        x[[5, 7, 50 + b]] = [-0.0, -0.0, 0.0] if b % 2 == 0 else [0.0, -0.0, -0.0]
        rows.append(x)
    cands, want = _check_crafted(lib, np.stack(rows), 4, 1.0, want_special=[1.0])
    assert all(len(c[0]) == 6 for c in cands) and all(want[b, 2] == 50 + b for b in range(5))      # u = 1.0: the last zero


def test_sampler_top_p_edges(lib):
    rng = np.random.default_rng(17)
    # masses 1/2, 1/4, 1/8, 1/16, 1/16 (+ small per-row tilt) at scattered indices
    rows = []
    for b in range(5):
        x = _noise(rng, 257, -60.0, -50.0)
        at = rng.permutation(257)[:5]
        x[at] = np.log(np.array([0.5, 0.25, 0.125, 0.0625, 0.0625])).astype(np.float32) + np.float32([0.01 * b, 0, 0, 0.001, 0])
        rows.append(x)
    rows = np.stack(rows)
    cands, want = _check_crafted(lib, rows, 5, 1.0, want_special=[0.0, U_LAST, 1.0])            # top_p = 1: nothing goes, u = 1.0 falls through to rank 4
    assert all(want[b, 2] == cands[b][0][4] and want[b, 1] == cands[b][0][4] and want[b, 0] == cands[b][0][0] for b in range(5))
    cands, want = _check_crafted(lib, rows, 5, 0.3, want_special=[0.0, U_LAST, 1.0])            # only the largest survives
    assert all((want[b] == cands[b][0][0]).all() for b in range(5))
    cands, want = _check_crafted(lib, rows, 5, 0.8, want_special=[0.0, U_LAST, 1.0])            # ranks 3, 4 go (tail 1/8 <= 0.2 < 1/4)
    assert all(want[b, 2] == cands[b][0][2] for b in range(5))


@pytest.mark.parametrize("V", [257, 8195])
def test_more_than_64_candidates_keep_the_64_best_in_index_order(lib, V):
    """Ties at the threshold that leave more candidates than the 64 slots: the survivors are the 64 best under (score descending, index
    ascending) -- the scores above the threshold, then threshold-equal ones by ascending index -- the same in every launch."""
    rng = np.random.default_rng(18)
    rows = []
    x = _noise(rng, V, -9.0, -8.0)                                             # 30 above, 80 equal at the threshold
    at = rng.permutation(V)[:110]
    x[at[:30]] = np.linspace(1.0, 1.5, 30, dtype=np.float32)
    x[at[30:]] = 0.75
    rows.append(x)
    rows.append(np.full(V, -1.25, np.float32))                                 # all equal: tokens 0, 2 .. 64 (eos is suppressed)
    x = np.full(V, 0.0, np.float32)                                            # all equal up to the sign of zero, one score above
    x[rng.permutation(V)[:V // 2]] = -0.0
    x[V - 1] = 0.5
    rows.append(x)
    x = _noise(rng, V, -9.0, -8.0)                                             # 49 above, 200 equal from index 3 on (V = 8195: up to the row's tail)
    x[np.arange(V - 200, V)] = 2.0
    x[rng.permutation(V - 200)[:49]] = 3.0
    rows.append(x)
    x = np.full(V, 1.0, np.float32)                                            # all equal but eos, suppressed
    x[R.EOS] = 7.0
    rows.append(x)
    x = np.full(V, -4.0, np.float32)                                           # 100 equal scores in front, the ten best at the end of the row
    x[:100] = 1.0
    x[V - 10:] = np.linspace(2.0, 2.9, 10, dtype=np.float32)
    rows.append(x)
    rows = np.stack(rows)
    # 8 clear uniforms per row (0, the float below 1 and 1.0 among them), 3 x 8 launches: the same tokens every time
    cands, want = _check_crafted(lib, rows, 50, 1.0, suppress=True, want_special=[0.0, U_LAST, 1.0], launches=3)
    assert all(len(c[0]) == 64 for c in cands)
    assert cands[1][0].tolist() == cands[4][0].tolist() == [0] + list(range(2, 65)) and cands[2][0][0] == V - 1
    assert cands[5][0].tolist() == list(range(V - 1, V - 11, -1)) + [0] + list(range(2, 55))
    # u = 1.0 reports the last survivor: the 64th under (score descending, index ascending); u = 0 the best score
    assert want[:, 2].tolist() == [int(c[0][63]) for c in cands] and want[:, 0].tolist() == [int(c[0][0]) for c in cands]


# ---------------------------------------------------------------------------------------------------------------- sampler, random rows
MARGIN = 2e-5       # <= 64 float32 addends, each a few ulp off after expf and the division: 64 x 4 x 2^-24 = 1.5e-5
CAP = 0.03


@pytest.mark.parametrize("source", ["injected", "hashed"])
@pytest.mark.parametrize("scale", [1, 3])
@pytest.mark.parametrize("V", VS)
def test_sampler_random_rows(lib, V, scale, source):
    """2048 draws per case (4 batches of 64 rows of scale x randn logits, 8 steps each; top_k 50, top_p 0.95; uniforms injected or hashed from
    (seed, row, step)).  A draw whose reference margin is >= MARGIN must match exactly; one below it must be the reference's answer or the
    answer with that closest decision taken the other way; at most CAP of the draws may be of the second kind.
    Shares of draws with margin < MARGIN, from the reference alone with these seeds (injected / hashed, per cent): V 61: 0.93 / 0.98 at
    scale 1, 1.22 / 1.17 at scale 3; V 257: 0.29 / 0.15, 2.00 / 2.00; V 8192: 0.15 / 0.29, 1.81 / 1.81; V 8195: 0.24 / 0.29, 0.05 / 0.15
    (a row whose top-p cut is that close counts with all its 8 draws: the 2 % cases are five such rows).  Two launches agree bit for bit."""
    T = 8
    n = amb = 0
    for batch in range(4):
        rng = np.random.default_rng([V, scale, batch])
        rows = (rng.standard_normal((64, V)) * scale).astype(np.float32)
        seed = 0x9E3779B9 * (batch + 1) + V
        if source == "injected":
            U = rng.random((64, T)).astype(np.float32)
        else:
            U = np.array([[R.hash_uniform(seed, b, t) for t in range(T)] for b in range(64)], np.float32)
        cands = [R.candidates(r, 50) for r in rows]
        for t in range(T):
            kw = dict(do_sample=True, top_k=50, top_p=0.95, t=t, max_new=T)
            kw.update(dict(uniforms=U) if source == "injected" else dict(seed=seed))
            out = pick(lib, rows, **kw)[0][:, t]
            again = pick(lib, rows, **kw)[0][:, t]
            assert np.array_equal(out, again)
            for b in range(64):
                tok, margin, alt = R.draw(*cands[b], 0.95, U[b, t])
                n += 1
                if margin >= MARGIN:
                    assert out[b] == tok, (batch, t, b, margin, int(out[b]), tok, alt)
                else:
                    amb += 1
                    assert out[b] in (tok, alt), (batch, t, b, margin, int(out[b]), tok, alt)
    print(f"[pick V={V} scale={scale} {source}] {n} draws, {amb} with margin < {MARGIN} ({100.0 * amb / n:.2f} %)")
    assert n == 2048 and amb <= CAP * n


def test_hashed_stream_is_the_python_restatement(lib):
    """64 equal candidates, nothing dropped: the pick is candidate floor(64 u) exactly (every sum is exact), so the tokens spell the top six
    bits of hash_uniform(seed, row, t) -- three seeds, rows 0 .. 63, eight steps; each row has its own candidates."""
    rng = np.random.default_rng(19)
    rows = np.full((64, 257), -30.0, np.float32)
    at = np.stack([np.sort(rng.permutation(257)[:64]) for _ in range(64)])
    for b in range(64):
        rows[b, at[b]] = 1.0
    seen = set()
    for seed in (0, 0x5EED, 2 ** 64 - 59):
        for t in (0, 1, 2, 3, 9, 255, 7201, 65535):
            # (the fed token: the reported one is written only while t < max_new)
            got = pick(lib, rows, do_sample=True, top_k=64, top_p=1.0, seed=seed, t=t, max_new=1)[1]
            rank = np.floor(np.array([R.hash_uniform(seed, b, t) for b in range(64)]) * 64).astype(int)
            assert got.tolist() == at[np.arange(64), rank].tolist(), (seed, t)
            seen.update(rank.tolist())
    assert len(seen) == 64


# ---------------------------------------------------------------------------------------------------------------- bookkeeping
def test_bookkeeping(lib):
    rng = np.random.default_rng(20)
    V, B, T = 257, 64, 4
    rows = np.stack([_noise(rng, V) for _ in range(B)])
    top = rng.integers(3, V, B)
    top[::4] = R.EOS                                                           # every fourth row picks eos
    rows[np.arange(B), top] = 1.0
    fin_in = (np.arange(B) % 3 == 0).astype(np.int32)                          # every third row is already finished
    forced = rng.integers(0, V, (B, T))
    forced[1], forced[2], forced[4], forced[5] = -5, V, V + 1000, R.EOS        # clamped to 0 / V - 1; a forced eos finishes the row
    for kind in ("plain", "forced"):
        for t in (0, 2, 3, 4, 9):
            tok, cur, fin = pick(lib, rows, t=t, max_new=T, finished=fin_in, forced=forced if kind == "forced" else None)
            for b in range(B):
                rep, fed, f = R.step(rows[b], t=t, max_new=T, finished=bool(fin_in[b]), forced=forced[b, min(t, T - 1)] if kind == "forced" else None)
                want_row = [-7] * T
                if rep is not None:
                    want_row[t] = rep
                assert tok[b].tolist() == want_row, (kind, t, b)
                assert (cur[b], fin[b]) == (fed, int(f)), (kind, t, b)
    # the same through the sampler: a finished row reports pad whatever it would have drawn
    tok, cur, fin = pick(lib, rows, do_sample=True, top_k=1, top_p=1.0, uniforms=np.full((B, 1), 0.5), finished=fin_in)
    want = np.where(fin_in == 1, R.PAD, top)
    assert tok[:, 0].tolist() == want.tolist() == cur.tolist() and fin.tolist() == ((fin_in == 1) | (want == R.EOS)).astype(int).tolist()


# ---------------------------------------------------------------------------------------------------------------- coordinate argmax
def _coords(lib, logits, mask):
    from meshanything_amd import _lib
    nf = len(mask)
    d_log, d_mask = _dev(logits, np.float32), _dev(mask, np.uint8)
    out = torch.full((nf * 9,), 7.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.ma_op_coords_argmax(_p(d_log), nf, logits.shape[1], _p(d_mask), _p(out), C.c_void_p(torch.cuda.current_stream().cuda_stream)), None)
    return out.cpu().numpy()


@pytest.mark.parametrize("nf", [1, 5, 300])
@pytest.mark.parametrize("nd", [1, 63, 64, 65, 128, 257])
def test_coords_argmax(lib, nd, nf):
    """One wave per (face, coordinate), four per workgroup (nf * 9 is odd for odd nf: the last workgroup is ragged); 64 lanes stride the nd bins.
    Maxima at the ends of the strides, equal maxima across lanes and strides (the lowest wins), NaN in the rows next door (no row is affected
    by another), masked faces NaN.  Bit-exact coordinates."""
    rng = np.random.default_rng([nd, nf])
    n = nf * 9
    x = rng.uniform(-2.0, -1.0, (n, nd)).astype(np.float32)
    spots = [s for s in (0, 63, 64, nd - 1, 1, 62, 65, 127, 128, 191, 192, 255, 256) if s < nd]
    want_bin = np.zeros(n, np.int64)
    for i in range(n):
        kind = i % 4
        if kind == 0:                                                          # one maximum
            at = [spots[(i // 4) % len(spots)]]
        elif kind == 1:                                                        # two or three equal maxima
            at = sorted({spots[(i // 4) % len(spots)], spots[(i // 4 + 1) % len(spots)], int(rng.integers(nd))})
        elif kind == 2:                                                        # NaN all around the maximum's row-mates: this row's neighbours see none of it
            x[i, rng.permutation(nd)[:nd // 2]] = np.nan
            at = [int(rng.integers(nd))]
        else:                                                                  # an all-equal row
            x[i] = -1.5
            at = [0]
        x[i, at] = 1.0 if kind != 3 else -1.5
        want_bin[i] = min(at)
    mask = (rng.random(nf) < 0.7).astype(np.uint8)
    mask[0] = 1
    if nf > 1:
        mask[-1] = 0
    got = _coords(lib, x, mask)
    ref = R.coords(x, mask)
    keep = np.repeat(mask.astype(bool), 9)
    assert np.array_equal(np.isnan(got), ~keep)
    assert np.array_equal(got[keep].view(np.uint32), ref[keep].view(np.uint32))
    assert np.array_equal(ref[keep], (want_bin[keep].astype(np.float32) / np.float32(nd) - np.float32(0.5)))      # the planted bins are the answer
    assert np.array_equal(_coords(lib, x, mask).view(np.uint32), got.view(np.uint32))
