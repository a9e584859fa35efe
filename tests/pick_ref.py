"""Plain float64 restatement of the token pick (csrc/misc.hpp pick_kernel), its hashed uniform stream and the detokenizer's coordinate
argmax (coords_argmax_kernel).  numpy only: independent of the HIP library and of oracle/.

Greedy: argmax, lowest index among equal maxima, eos left out when suppressed.
Sampling ([3p] TopKLogitsWarper, TopPLogitsWarper, inverse-CDF draw): eos = -inf when suppressed; candidates = every score >= the k-th
largest, ordered by (score descending, index ascending), at most KMAX of them; softmax over the candidates; the ascending prefix whose
cumulative mass is <= 1 - top_p goes (never the largest); renormalise; the first rank whose cumulative mass exceeds u wins, else the last.
Every draw comes with its margin -- the distance of the closest decision (a tail mass against 1 - top_p, a partial CDF sum against u) from
flipping -- and with the answer that decision's other outcome would give."""
import numpy as np

BOS, EOS, PAD = 0, 1, 2
KMAX = 64
_M64 = (1 << 64) - 1


def greedy(logits, suppress_eos=False):
    """Index of the largest logit, the lowest index among equals; eos is not a candidate when suppressed."""
    x = np.asarray(logits, np.float64)
    idx = np.arange(x.shape[0])
    if suppress_eos:
        idx = idx[idx != EOS]
    v = x[idx]
    m = v.max()
    return int(idx[np.flatnonzero(v == m)[0]])


def candidates(logits, top_k, suppress_eos=False):
    """(indices, scores) of the sampler's candidates in (score descending, index ascending) order."""
    x = np.asarray(logits, np.float64).copy()
    if suppress_eos:
        x[EOS] = -np.inf
    V = x.shape[0]
    k = min(top_k, V, KMAX)
    order = np.argsort(-x, kind="stable")                          # stable: equal scores stay in index order
    kth = x[order[k - 1]]
    n = int(np.count_nonzero(x >= kth))
    idx = order[:min(n, KMAX)]
    return idx.astype(np.int64), x[idx]


def _draw_with_keep(p, keep, u):
    q = p[:keep] / p[:keep].sum()
    cdf = np.cumsum(q)
    hit = np.flatnonzero(cdf > u)
    pick = int(hit[0]) if hit.size else keep - 1
    return pick, cdf


def draw(idx, scores, top_p, u):
    """One draw from candidates(): (token, margin, alternative token).  top_p and u are taken as the float32 values the kernel receives.
    `alternative` is the token the closest decision's other outcome gives (the neighbouring rank for a CDF sum, one candidate more or fewer
    kept for a tail mass); None when there is no decision at all (one candidate)."""
    u = float(np.float32(u))
    thr = float(np.float32(1.0 - float(np.float32(top_p))))       # the kernel: (float)(1.0 - (double)top_p)
    nc = scores.shape[0]
    with np.errstate(invalid="ignore"):
        e = np.exp(scores - scores[0])
    p = e / e.sum()
    tail = np.cumsum(p[::-1])[::-1]                               # tail[j] = mass of ranks j .. nc - 1
    keep = nc - int(np.count_nonzero(tail[1:] <= thr))             # (the tail masses grow towards rank 0: what goes is a suffix; rank 0 stays)
    pick, cdf = _draw_with_keep(p, keep, u)
    # the closest decision
    best, alt = np.inf, None
    if nc > 1:                                                    # tail masses against 1 - top_p
        d = np.abs(tail[1:] - thr)
        j = int(np.argmin(d)) + 1                                 # (next to the cut: keep or keep - 1)
        best, alt = d[j - 1], ("keep", j + 1 if tail[j] <= thr else j)      # removed -> kept: keep = j + 1; kept -> removed: keep = j
    if keep > 1:                                                  # partial CDF sums against u (the last one decides nothing)
        d = np.abs(cdf[:keep - 1] - u)
        j = int(np.argmin(d))
        if d[j] < best:
            best, alt = d[j], ("rank", j if cdf[j] <= u else j + 1)         # <= u -> > u: rank j wins; > u -> <= u: the next rank
    if alt is None:
        alt_tok = None
    elif alt[0] == "keep":
        alt_tok = int(idx[_draw_with_keep(p, alt[1], u)[0]])
    else:
        alt_tok = int(idx[alt[1]])
    return int(idx[pick]), float(best), alt_tok


def sample(logits, top_k, top_p, u, suppress_eos=False):
    idx, sc = candidates(logits, top_k, suppress_eos)
    return draw(idx, sc, top_p, u)


def hash_uniform(seed, row, t):
    """misc.hpp hash_uniform with Python integers: splitmix64's finaliser over seed + golden * (row << 32 | t), top 24 bits / 2^24."""
    z = (seed + 0x9E3779B97F4A7C15 * (((row << 32) | (t & 0xFFFFFFFF)) & _M64)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return float(np.float32(z >> 40) * np.float32(1.0 / 16777216.0))


def step(logits, *, t=0, max_new=1, do_sample=False, top_k=50, top_p=0.95, suppress_eos=False, u=None, finished=False, forced=None):
    """One row of generate()'s bookkeeping around the pick: (reported token or None when t >= max_new, fed token, finished afterwards).
    u: this step's uniform (sampling)."""
    V = len(logits)
    tok = sample(logits, top_k, top_p, u, suppress_eos)[0] if do_sample else greedy(logits, suppress_eos)
    if finished:
        tok = PAD
    reported = tok if t < max_new else None
    if forced is not None and t < max_new:
        tok = min(max(int(forced), 0), V - 1)
    return reported, tok, bool(finished or tok == EOS)


def coords(logits, mask):
    """coords_argmax_kernel: logits (nf * 9, nd), mask (nf) -> (nf * 9) float32 = argmax / nd - 0.5 in the kernel's float32 steps, NaN for
    masked faces.  Every row needs one logit that is not NaN."""
    x = np.asarray(logits, np.float64)
    nd = x.shape[1]
    bi = np.empty(x.shape[0], np.int64)
    for i, r in enumerate(x):                                     # (a NaN logit never wins a comparison: it is no candidate)
        ok = np.flatnonzero(~np.isnan(r))
        bi[i] = ok[np.flatnonzero(r[ok] == r[ok].max())[0]]
    t = bi.astype(np.float32) / np.float32(nd)
    t = t * np.float32(1.0) + np.float32(-0.5)
    keep = np.repeat(np.asarray(mask).astype(bool), 9)
    return np.where(keep, t, np.float32(np.nan)).astype(np.float32)
