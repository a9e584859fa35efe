"""Attention inputs whose softmax is known in closed form, the float64 reference, and the error bound an fp32-accumulating kernel must keep.
torch / numpy only: independent of the HIP library and of oracle/.

Builder.  Head h looks at ONE dimension, d_h = (7 h + 3) % 64: the query of row i is sign_i * 8 there and zero elsewhere, key j carries its
level t_j there and asymmetric random values in the other 63 dimensions (the query is zero there, so they cannot matter -- unless a kernel
mixes dimensions, heads or operands up).  With scale 1/8 the score of (i, j) is exactly sign_i * t_j.  V is randn plus a ramp over the
dimensions.  Every tensor is rounded to the format under test before anybody sees it.

Patterns (levels change every STEP = 16 keys: 16 divides every tile (32, 64), round (32 per wave: 128, 256, 512) and chunk in use):
  stairs_up    t rises RISE = 40 per step: the running maximum moves in every tile, everything older is rescaled by e^-40 or less
  stairs_down  the mirror: the maximum is found in the first step and never moves, all later partials underflow against it
  zigzag       stairs_up keys, even rows +8, odd rows -8: rows whose maximum moves in every tile sit beside rows where it never does
  flat(+-96)   every score equal, far from 0: a maximum that starts at 0 (or is missing) overflows at +96 and flushes to 0 at -96
  spike(j)     one key SPIKE = 50 above an otherwise flat row
  twin(a, b)   two identical key rows 50 above the rest, in different tiles / rounds / chunks / halves
In every pattern the visible keys of a row that reach the row's top score weigh exactly 1 against each other and every other visible key lies
at least GAP = 30 nats below: the output is the MEAN OF V OVER THE TOP VISIBLE KEYS (closed_form), up to n e^-30.

Bound, per output element (bound()), derived from the arithmetic of ANY kernel that accumulates in fp32 -- not read off one:
    n_top * 2^-23 * max|v|        fp32 accumulation of the n_top contributions and of the row sum (one rounding each per key: 2 * 2^-24)
  + 1/2 ulp_out(|ref|) (+ 2^-24 |ref| for the normalising multiply)        the output format's rounding
  + n_vis * e^-30 * max|v|        everything that is not a top key (weight <= e^-30 each; also covers their being dropped, flushed or rounded away)
  + 2^-21 * |s_top| * max|v|      the scores are fp32 numbers of magnitude |s_top|: scale, change of base (exp2 on s log2 e) and the subtraction
                                   of the maximum are up to four roundings of 2^-24 |s| -- the exponent's argument is known to 2^-22 |s_top|, a weight
                                   to that RELATIVE error, and a normalised mean of values within max|v| to twice it.  (Whether the errors of equal
                                   scores cancel between numerator and row sum depends on where a kernel rounds P; a bound may not assume it.)
There is no P-rounding term: the top keys' p is 1 (exactly representable), the others are covered by the e^-30 term.  No element and no case is
exempt.

Batched launches (stack(), Batch): the samples of one launch (grid.z) are Cases of one shape, every sample a pattern of its own, optionally followed by a
shorter last sample (short_case) behind whose rows sits an adversarial key; the bound is per sample, unchanged.  layout_batch / last_len_batch / tail_batch
build the launches of tests/test_gpu_attention_batched.py, wrong_variants() what four wrong kernels would compute for a sample."""
import functools
import math

import numpy as np
import torch

STEP, RISE, SPIKE, GAP, QMAG, SCALE = 16, 40.0, 50.0, 30.0, 8.0, 0.125
FORMATS = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
_MANT = {"f32": 23, "bf16": 7, "fp16": 10}
_EMIN = {"f32": -126, "bf16": -126, "fp16": -14}


def head_dim(h):
    return (7 * h + 3) % 64


def rnd(x, fmt):
    return x.to(FORMATS[fmt]).to(x.dtype)


def half_ulp(x, fmt):
    """Half a unit in the last place of `fmt` at |x| (float64 tensor)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** _EMIN[fmt]))).clamp_min(_EMIN[fmt])
    return torch.exp2(e - _MANT[fmt] - 1)


# ---- levels ---------------------------------------------------------------------------------------------------------------------------
def stairs_up(Sk):
    return RISE * (torch.arange(Sk) // STEP).double()


def stairs_down(Sk):
    return RISE * ((Sk - 1) // STEP - torch.arange(Sk) // STEP).double()


def flat(Sk, level):
    return torch.full((Sk,), float(level), dtype=torch.float64)


def spike(Sk, j):
    t = torch.zeros(Sk, dtype=torch.float64)
    t[j] = SPIKE
    return t


def twin(Sk, a, b):
    t = torch.zeros(Sk, dtype=torch.float64)
    t[a] = t[b] = SPIKE
    return t


class Case:
    """q (Sq, H, 64), k, v (Sk, H, 64) float32 holding values of `fmt`; causal_offset < 0: every key visible, else row i sees keys <= offset + i."""
    def __init__(self, name, q, k, v, fmt, causal_offset, dims):
        self.name, self.q, self.k, self.v, self.fmt, self.causal_offset, self.dims = name, q, k, v, fmt, causal_offset, dims


def build(name, levels, signs, fmt, causal_offset=-1, twins=(), dims=None, seed=0, device="cpu"):
    """levels (H, Sk) float64, signs (Sq,) of +-1; twins: (h, a, b) -- key row b of head h becomes a copy of key row a (all 64 dimensions);
    dims: the dimension each head looks at (default head_dim(h))."""
    H, Sk = levels.shape
    Sq = signs.shape[0]
    dims = [head_dim(h) for h in range(H)] if dims is None else list(dims)
    g = torch.Generator().manual_seed(int(seed))
    # (host tensors of a few 10^4 elements, on ONE thread: above torch's parallel grain -- 257 keys x 2 heads x 64 -- every operation would wake the whole
    #  pool, and a session may have left it wider than the cores this process may use: seconds per case on the GPU machine)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        k = torch.randn(Sk, H, 64, generator=g) + torch.linspace(-0.3, 0.3, 64)[None, None, :]
        v = torch.randn(Sk, H, 64, generator=g) + torch.linspace(0.5, -0.5, 64)[None, None, :]
        q = torch.zeros(Sq, H, 64)
        hs = torch.arange(H)
        d = torch.tensor(dims)
        q[:, hs, d] = QMAG * signs.float()[:, None]
        k[:, hs, d] = levels.float().t()
        for (h, a, b) in twins:
            k[b, h] = k[a, h]
    finally:
        torch.set_num_threads(threads)
    q, k, v = rnd(q.to(device), fmt), rnd(k.to(device), fmt), rnd(v.to(device), fmt)      # (rounded where the tests compute: nothing large on the host's cores)
    return Case(name, q, k, v, fmt, causal_offset, dims)


# ---- what the output must be ---------------------------------------------------------------------------------------------------------------
def _visible(Sq, Sk, causal_offset, device):
    if causal_offset < 0:
        return torch.ones(Sq, Sk, dtype=torch.bool, device=device)
    return torch.arange(Sk, device=device)[None, :] <= (torch.arange(Sq, device=device)[:, None] + causal_offset)


def reference(case):
    """The softmax definition in float64 on the rounded inputs: (Sq, H, 64) float64."""
    q, k, v = case.q.double(), case.k.double(), case.v.double()
    w = torch.einsum("qhd,khd->hqk", q, k) * SCALE
    vis = _visible(q.shape[0], k.shape[0], case.causal_offset, q.device)
    w = w.masked_fill(~vis[None], float("-inf"))
    return torch.einsum("hqk,khd->qhd", torch.softmax(w, dim=-1), v)


def analyse(case):
    """The closed form and what the bound needs, from the ROUNDED tensors: dict of out (Sq, H, 64) = mean of V over the top visible keys,
    n_top, n_vis, s_top (Sq, H), gap (the smallest distance of a visible non-top key from its row's top; inf when there is none),
    clean (the score of every (row, key) comes from the head's own dimension alone)."""
    q, k, v = case.q.double(), case.k.double(), case.v.double()
    Sq, H, Sk = q.shape[0], q.shape[1], k.shape[0]
    hs, d = torch.arange(H, device=q.device), torch.tensor(case.dims, device=q.device)
    s = torch.einsum("qh,kh->hqk", q[:, hs, d], k[:, hs, d]) * SCALE              # exact: one product of small dyadic numbers
    full = torch.einsum("qhd,khd->hqk", q, k) * SCALE
    vis = _visible(Sq, Sk, case.causal_offset, q.device)[None].expand(H, Sq, Sk)
    top = s.masked_fill(~vis, float("-inf")).max(dim=-1, keepdim=True).values
    is_top = vis & (s == top)
    other = vis & ~is_top
    gap = (top - s).masked_fill(~other, float("inf")).min(dim=-1).values
    n_top = is_top.sum(-1)
    out = torch.einsum("hqk,khd->qhd", is_top.double(), v) / n_top.t()[..., None]
    return {"out": out, "n_top": n_top.t(), "n_vis": vis.sum(-1).t(), "s_top": top[..., 0].t(), "gap": gap.t(), "clean": bool((s == full).all())}


def bound(case, ref, info, out_fmt):
    """Per-element bound (module docstring) for an output stored in `out_fmt`: (Sq, H, 64) float64."""
    vmax = float(case.v.abs().max())
    row = (info["n_top"].double() * 2.0 ** -23 + info["n_vis"].double() * math.exp(-GAP) + 2.0 ** -21 * info["s_top"].abs()) * vmax
    return row[..., None] + half_ulp(ref, out_fmt) + 2.0 ** -24 * ref.abs()


def worst_ratio(got, ref, bnd):
    """max |got - ref| / bound over all elements; inf when anything is not finite.  A result passes when this is <= 1."""
    got = got.double().reshape(ref.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / bnd).max())


# ---- the case lists the host and the GPU tests share ------------------------------------------------------------------------------------------
def spike_positions_dense(Sq, Sk, causal_offset):
    pos = [0, 15, 16, 31, 32, 63, 64, Sk - 1]
    if causal_offset >= 0:                    # the diagonal key of the rows at tile / block edges and the key just beyond it
        for r in (31, 32, 63, 64, 95, 96, 127, 128):
            pos += [causal_offset + r, causal_offset + r + 1] if r < Sq else []
    return sorted({p for p in pos if 0 <= p < Sk})


def twin_positions_dense(Sk):
    return [(a, b) for (a, b) in ((5, min(70, Sk - 1)), (20, Sk - 3), (3, 40)) if 0 <= a < b < Sk]


def dense_cases(Sq, Sk, H, causal_offset, fmt, device="cpu"):
    """Every pattern for one dense shape; spike / twin positions are spread over the heads (a head is a softmax of its own)."""
    plus, alt = torch.ones(Sq), torch.where(torch.arange(Sq) % 2 == 0, 1.0, -1.0)
    rep = lambda t: t[None].expand(H, Sk).clone()
    kw = dict(fmt=fmt, causal_offset=causal_offset, device=device)
    yield build("stairs_up", rep(stairs_up(Sk)), plus, seed=1, **kw)
    yield build("stairs_down", rep(stairs_down(Sk)), plus, seed=2, **kw)
    yield build("zigzag", rep(stairs_up(Sk)), alt, seed=3, **kw)
    yield build("flat+96", rep(flat(Sk, 96)), plus, seed=4, **kw)
    yield build("flat-96", rep(flat(Sk, -96)), plus, seed=5, **kw)
    pos = spike_positions_dense(Sq, Sk, causal_offset)
    for i in range(0, len(pos), H):
        grp = [pos[min(i + h, len(pos) - 1)] for h in range(H)]
        yield build("spike" + str(tuple(grp)), torch.stack([spike(Sk, j) for j in grp]), plus, seed=10 + i, **kw)
    tw = twin_positions_dense(Sk)
    for i in range(0, len(tw), H):
        grp = [tw[min(i + h, len(tw) - 1)] for h in range(H)]
        yield build("twin" + str(tuple(grp)), torch.stack([twin(Sk, a, b) for a, b in grp]), plus, twins=[(h, a, b) for h, (a, b) in enumerate(grp)], seed=40 + i, **kw)


# ---- batched launches: the samples of ONE launch (grid.z), every sample a pattern of its own ------------------------------------------------------
ADV = SPIKE + 50.0            # level of the adversarial key behind a short last sample: GAP-dominant over every level of a spike case


class Batch:
    """The samples of one batched launch.  q (B, Sq, H, 64), k, v (B, Sk, H, 64) float32 holding values of `fmt`: what the full-length buffers of the launch
    hold; cases[b]: the Case sample b must compute (reference(), analyse() and bound() run on it).  last_len > 0: the last sample is cases[-1] of shape
    (last_len, last_len) in the leading rows of q[-1], k[-1], v[-1]; behind them sit the rows of a filler pattern, and key `last_len` is adversarial: level ADV
    in every head's dimension and V far from every other key's, so a row that wrongly saw it returns that V.  Nothing in here is modified after stack()."""
    def __init__(self, name, cases, q, k, v, causal_offset, last_len, fmt):
        self.name, self.cases, self.q, self.k, self.v, self.causal_offset, self.last_len, self.fmt = name, cases, q, k, v, causal_offset, last_len, fmt
        self.B, self.Sq, self.H = q.shape[0], q.shape[1], q.shape[2]
        self.Sk = k.shape[1]

    def rows(self, b):
        """(query rows, keys) of sample b"""
        return (self.cases[b].q.shape[0], self.cases[b].k.shape[0])


def stack(name, cases, last=None, shared_q=None, Sq=None, Sk=None):
    """Stacks Cases of one shape (Sq, Sk) into a Batch.  last: a shorter Case of shape (L, L) that becomes the last sample (see Batch); Sq, Sk are needed when
    `cases` is empty.  shared_q (Sq, H, 64): every sample takes this query instead of its own (one Q for all samples, sample stride 0): the Cases are rebuilt on it."""
    cases = list(cases)
    if shared_q is not None:
        cases = [Case(c.name, shared_q, c.k, c.v, c.fmt, c.causal_offset, c.dims) for c in cases]
    first = cases[0] if cases else last
    Sq, Sk = (cases[0].q.shape[0], cases[0].k.shape[0]) if cases else (Sq, Sk)
    assert all(c.q.shape[0] == Sq and c.k.shape[0] == Sk and c.fmt == first.fmt and c.causal_offset == first.causal_offset for c in cases)
    qs, ks, vs = [c.q for c in cases], [c.k for c in cases], [c.v for c in cases]
    last_len = -1
    if last is not None:
        L, H, dev = last.q.shape[0], last.q.shape[1], last.q.device
        assert last.k.shape[0] == L and L <= min(Sq, Sk) and last.fmt == first.fmt and last.causal_offset == first.causal_offset
        last_len = L
        fill = build("filler", stairs_down(Sk)[None].expand(H, Sk).clone(), torch.ones(Sq), last.fmt, causal_offset=last.causal_offset, dims=last.dims, seed=99, device=dev)
        q, k, v = fill.q.clone(), fill.k.clone(), fill.v.clone()
        q[:L], k[:L], v[:L] = last.q, last.k, last.v
        if L < Sk:
            k[L, torch.arange(H, device=dev), torch.tensor(last.dims, device=dev)] = ADV
            v[L] = rnd(v[L] + 4.0, last.fmt)
        qs.append(q); ks.append(k); vs.append(v)
        cases = cases + [last]
    return Batch(name, cases, torch.stack(qs), torch.stack(ks), torch.stack(vs), first.causal_offset, last_len, first.fmt)


def spike_case(Sq, Sk, positions, fmt, causal_offset, seed, device="cpu"):
    """One spike per head at positions[h] (signs all +)."""
    return build("spike" + str(tuple(positions)), torch.stack([spike(Sk, j) for j in positions]), torch.ones(Sq), fmt, causal_offset=causal_offset, seed=seed, device=device)


def short_case(L, H, fmt, causal_offset, device="cpu"):
    """The shortened last sample of a batch, shape (L, L): spikes from spike_positions_dense(L, L, .) -- head 0's at L - 1, the last key the sample has, the other
    heads' walk down the list from there."""
    pos = spike_positions_dense(L, L, causal_offset)
    assert pos[-1] == L - 1
    grp = [pos[max(len(pos) - 1 - h, 0)] for h in range(H)]
    return spike_case(L, L, grp, fmt, causal_offset, seed=70 + L, device=device)


# the launches of tests/test_gpu_attention_batched.py; tests/test_attn_cases_host.py checks every one of them on the host
LAYOUT_LAUNCHES = [      # (layout, Sq, Sk, causal_offset)
    ("interleaved", 130, 130, -1), ("interleaved", 257, 257, -1), ("interleaved", 96, 65, -1),
    ("blocks", 128, 128, -1), ("blocks", 257, 257, 0), ("blocks", 130, 130, 0),
    ("cross", 70, 300, -1), ("cross", 96, 65, -1),
    ("planes", 257, 257, 0), ("planes", 130, 130, 0), ("planes", 128, 128, 0)]
LAST_LEN_LAUNCHES = [(257, L) for L in (193, 249, 256, 257)] + [(130, L) for L in (1, 63, 64, 65, 96, 97, 129)]      # (T, last_len), each causal and not
TAIL_LAUNCHES = [(T, nt) for T in (130, 257) for nt in (1, 2, 34, 64)]                                              # (T, rows of the tail chain)
BATCH_H = 2


@functools.lru_cache(maxsize=None)
def _dense_case_list(Sq, Sk, causal_offset, fmt, device):
    """dense_cases at H = BATCH_H, built once per shape and shared by every launch that stacks them (nobody modifies a Case)."""
    return tuple(dense_cases(Sq, Sk, BATCH_H, causal_offset, fmt, device=device))


def layout_batch(layout, Sq, Sk, causal_offset, fmt, device="cpu"):
    """Every pattern of dense_cases as a sample of its own; `cross`: one Q for all samples (the zigzag's alternating signs: every pattern then has rows that
    look at its levels from both sides)."""
    cases = list(_dense_case_list(Sq, Sk, causal_offset, fmt, device))
    shared = next(c for c in cases if c.name == "zigzag").q if layout == "cross" else None
    return stack(f"{layout} {(Sq, Sk, causal_offset)} {fmt}", cases, shared_q=shared)


def _pick2(cases, i):
    """Two full-length samples for a batch of 3: the zigzag (the one pattern whose query rows differ: a launch without it cannot see a query row shifted) and
    another one of the remaining patterns for every i."""
    rest = [c for c in cases if c.name != "zigzag"]
    return [next(c for c in cases if c.name == "zigzag"), rest[i % len(rest)]]


def last_len_batch(T, L, causal_offset, fmt, device="cpu"):
    """B = 3: two full (T, T) samples and the short_case of L rows."""
    cases = list(_dense_case_list(T, T, causal_offset, fmt, device))
    return stack(f"last_len {(T, L, causal_offset)} {fmt}", _pick2(cases, L), last=short_case(L, BATCH_H, fmt, causal_offset, device=device))


def tail_batch(T, nt, fmt, device="cpu"):
    """B = 3 full causal (T, T) samples; the last one has its spikes on both sides of the cut between the main chain's rows and the tail chain's:
    key T - nt - 1 (head 0: the last key the main chain has) and key T - nt (head 1: the first one it must not read)."""
    cases = list(_dense_case_list(T, T, 0, fmt, device))
    cut = spike_case(T, T, [max(T - nt - 1, 0), T - nt], fmt, 0, seed=90 + nt, device=device)
    return stack(f"tail {(T, nt)} {fmt}", _pick2(cases, nt) + [cut])


def wrong_variants(batch, b):
    """The Cases a kernel with one of four mistakes would compute for sample b, as (name, Case) -- judged against cases[b] each must exceed the bound somewhere
    in the launch (test_attn_cases_host.py).  From the launch's full-length buffers:
      q_shift      query rows shifted by one (row i computes row i + 1)
      k_shift+-    K rows shifted by one against V (a K row stride / offset off by one row)
      sk_full      (the short last sample) every key of the full-length buffers instead of last_len; under a causal mask the rows that are kept never see
                   those keys whatever Sk is, so there the mistake is the mask letting ONE more key in (row last_len - 1 sees key last_len)."""
    c = batch.cases[b]
    nq, nk = batch.rows(b)
    q, k, v = batch.q[b], batch.k[b], batch.v[b]
    mk = lambda name, q_, k_, v_, off=c.causal_offset: (name, Case(name, q_, k_, v_, c.fmt, off, c.dims))
    out = [mk("q_shift", torch.roll(q, -1, 0)[:nq], k[:nk], v[:nk]), mk("k_shift+", q[:nq], torch.roll(k, -1, 0)[:nk], v[:nk]), mk("k_shift-", q[:nq], torch.roll(k, 1, 0)[:nk], v[:nk])]
    if batch.last_len > 0 and b == batch.B - 1 and nk < batch.Sk:
        out.append(mk("sk_full", q[:nq], k, v) if c.causal_offset < 0 else mk("sk_full", q[:nq], k, v, c.causal_offset + 1))
    return out


def decode_slots(length, chunks=16):
    """(name, levels, sign, twin) of every pattern for ONE query over `length` cached keys.  Spike positions: the tile edges, the newest two keys,
    the first key of the last step of 16, the edges of the split form's `chunks` equal chunks, one key in each of the first three rounds of 256."""
    L = length
    out = [("stairs_up", stairs_up(L), 1, None), ("stairs_down", stairs_down(L), 1, None), ("stairs_up_negq", stairs_up(L), -1, None),
           ("flat+96", flat(L, 96), 1, None), ("flat-96", flat(L, -96), 1, None), ("flat+96_negq", flat(L, 96), -1, None)]
    per = (L + chunks - 1) // chunks
    pos = [0, 15, 16, 31, 32, 63, 64, L - 1, L - 2, (L - 1) // STEP * STEP, per - 1, per, (chunks - 1) * per, ((L - 1) // per) * per, 5, 256 + 5, 512 + 5]
    for j in sorted({p for p in pos if 0 <= p < L}):
        out.append((f"spike({j})", spike(L, j), 1, None))
    for (a, b) in ((3, L - 2), (10, 256 + 10), (per - 1, per), (300, 600)):
        if 0 <= a < b < L:
            out.append((f"twin({a},{b})", twin(L, a, b), 1, (a, b)))
    return out


def decode_case(slots, n_slots, H, fmt, seed=0, device="cpu"):
    """`n_slots` independent single-query softmaxes (slot = (row, head), head = slot % H) as ONE Case with Sq = 1 and n_slots 'heads': slot i takes
    pattern i % len(slots).  Returns (case, names)."""
    pick = [slots[i % len(slots)] for i in range(n_slots)]
    levels = torch.stack([p[1] * p[2] for p in pick])                  # a negative query: the same scores as negated levels ...
    case = build("decode", levels, torch.ones(1), fmt, dims=[head_dim(i % H) for i in range(n_slots)],
                 twins=[(i, p[3][0], p[3][1]) for i, p in enumerate(pick) if p[3]], seed=seed, device=device)
    hs, d = torch.arange(n_slots, device=device), torch.tensor(case.dims, device=device)
    sg = torch.tensor([float(p[2]) for p in pick], device=device)
    case.q[0, hs, d] = case.q[0, hs, d] * sg                           # ... but carried by q = -8 against the un-negated keys
    case.k[:, hs, d] = case.k[:, hs, d] * sg[None, :]
    return case, [p[0] for p in pick]


# ---- a float32 emulation of tile-wise online softmax, written from the definition (host test) ------------------------------------------------
def emulate_online(case, tile, p_fmt, out_fmt, bug=None):
    """Online softmax over key tiles of `tile` in float32 numpy: scores and exponentials relative to the RUNNING maximum, the probabilities that
    multiply V rounded to `p_fmt`, the row sum kept in float32, the output rounded to `out_fmt`.  bug: None, or one of 'drop_newest' (the last
    visible key of every row is left out), 'mask_off_by_one' (a causal row sees one key too many), 'no_rescale' (the accumulators keep their
    scale when the maximum moves), 'max_from_zero' (the running maximum starts at 0 instead of -inf)."""
    q, k, v = case.q.cpu().numpy(), case.k.cpu().numpy(), case.v.cpu().numpy()
    Sq, H, Sk = q.shape[0], q.shape[1], k.shape[0]
    c = case.causal_offset
    last = np.minimum(np.arange(Sq) + c, Sk - 1) if c >= 0 else np.full(Sq, Sk - 1)      # last visible key of each row
    if bug == "mask_off_by_one" and c >= 0:
        last = np.minimum(last + 1, Sk - 1)
    out = np.zeros((Sq, H, 64), np.float32)
    r16 = lambda x, f: rnd(torch.from_numpy(np.ascontiguousarray(x)), f).numpy()
    with np.errstate(all="ignore"):
        for h in range(H):
            m = np.full(Sq, 0.0 if bug == "max_from_zero" else -np.inf, np.float32)
            l = np.zeros(Sq, np.float32)
            o = np.zeros((Sq, 64), np.float32)
            for k0 in range(0, Sk, tile):
                kt, vt = k[k0:k0 + tile, h], v[k0:k0 + tile, h]
                s = (q[:, h] @ kt.T).astype(np.float32) * np.float32(SCALE)
                keys = np.arange(k0, k0 + kt.shape[0])
                seen = keys[None, :] <= last[:, None]
                if bug == "drop_newest":
                    seen &= keys[None, :] != last[:, None]
                s = np.where(seen, s, -np.inf).astype(np.float32)
                m_new = np.maximum(m, s.max(axis=1))
                live = np.isfinite(m_new) | np.isnan(m_new)
                alpha = np.where(np.isfinite(m), np.exp(m - m_new), 0.0).astype(np.float32) if bug != "no_rescale" else np.ones(Sq, np.float32)
                p = np.where(seen & live[:, None], np.exp(s - np.where(live, m_new, 0.0)[:, None]), 0.0).astype(np.float32)
                l = l * alpha + p.sum(axis=1, dtype=np.float32)
                o = o * alpha[:, None] + r16(p, p_fmt) @ vt
                m = m_new
            out[:, h] = o / l[:, None]
    return rnd(torch.from_numpy(out), out_fmt)
