"""Plain restatement of what the dense GEMM dispatcher (csrc/gemm256.hpp launch_gemm_dense, csrc/gemm.hpp launch_gemm) and the LayerNorm row kernel
(csrc/dense_ops.hpp ln_rows2_kernel) promise, for tests/test_gpu_gemm_forms.py: row map, broadcast residual, the row ranges of a GEMM by parts, the
KV-plane address of (row, column), an fp64 GEMM with epilogue written into a canary-filled padded buffer -- and a generator of EXACT operands.

Exact operands: A, W, bias and the residual are small integers, so the 16-bit operands A and W are exact in bf16 and in fp16, every product is an integer, and every
partial sum -- in whatever order a kernel adds them up, split along K or not -- is an integer below 2^24, hence exact in fp32.  A correct kernel then
returns the fp64 result BIT FOR BIT (no tolerance that could hide one wrong small element), and its 16-bit output is the one-step round-to-nearest-even
of that integer.  The values are a hash of (row, column, seed) with different constants for A and W: a transposed, shifted or repeated fragment changes
the sums.

torch only, device-agnostic (the host test runs it on the CPU, the GPU test on the device with stock torch ops); independent of the HIP library."""
import torch

# what an untouched element holds: fixed bit patterns (finite values in every format, compared as integers)
PAT32 = 0xCAFEF00D - (1 << 32)          # as int32
PAT16 = 0xC5A7 - (1 << 16)              # as int16
A_MAX, W_MAX, BIAS_MAX, RES_MAX = 3, 3, 1000, 2000
EXACT_LIMIT = 1 << 24                   # integers below it are exact in fp32
FP16_MAX = 65504                        # the 16-bit output must stay finite in IEEE half as well

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2


# ---- addressing -------------------------------------------------------------------------------------------------------------------------------------
def row_map(m, grp, gstride, off):
    """Physical row of logical row(s) m (common.hpp RowMap): groups of `grp` rows sit `gstride` rows apart, shifted by `off`; grp 0: identity."""
    if grp <= 0:
        return m
    return (m // grp) * gstride + (m % grp) + off


def res_row(m, r_mod):
    """Row of the residual that logical row m adds: m % r_mod for a table broadcast over the batch, else m."""
    return m % r_mod if r_mod > 0 else m


def part_rows(M, part):
    """[lo, hi) of the logical rows a call computes: part 0 all, 1 the rows below M - M % 256, 2 the rows from there on."""
    mm = M - M % 256
    return {0: (0, M), 1: (0, mm), 2: (mm, M)}[part]


def kv_index(m, col, kv_T, kv_col0, kv_max_seq, kv_row_stride):
    """(plane, element) of column `col` in [kv_col0, 3 kv_col0) of logical row m: plane 0 = K, 1 = V;
    element = sample * kv_row_stride + (head * kv_max_seq + position) * 64 + d."""
    cc = col - kv_col0
    plane = cc // kv_col0
    c = cc - plane * kv_col0
    return plane, (m // kv_T) * kv_row_stride + ((c // 64) * kv_max_seq + (m % kv_T)) * 64 + (c % 64)


# ---- exact operands ---------------------------------------------------------------------------------------------------------------------------------
def _hash(r, c, seed, k1, k2):
    """32-bit mix of (r, c, seed) in int64 arithmetic that never leaves [0, 2^63): the same integers on every device."""
    m32 = 0xFFFFFFFF
    x = (r * k1 + c * k2 + seed * 0x9E3779B1 + 0x7F4A7C15) & m32
    x = ((x ^ (x >> 15)) * 0x2C1B3C6D) & m32
    x = ((x ^ (x >> 12)) * 0x297A2D39) & m32
    return x ^ (x >> 15)


def _ints(rows, cols, seed, k1, k2, amax, device):
    r = torch.arange(rows, dtype=torch.int64, device=device)[:, None]
    c = torch.arange(cols, dtype=torch.int64, device=device)[None, :]
    return (_hash(r, c, seed, k1, k2) % (2 * amax + 1) - amax).to(torch.float64)


def exact_operands(M, N, K, seed, device="cpu", r_rows=None):
    """A (M, K), W (N, K), bias (N), R (r_rows or M, N) as fp64 tensors of small integers: see the module text."""
    return dict(A=_ints(M, K, seed, 0x01000193, 0x0001F123, A_MAX, device),
                W=_ints(N, K, seed + 1, 0x00C4CEB9, 0x0000B5AD, W_MAX, device),
                bias=_ints(1, N, seed + 2, 0x0003D4D5, 0x00010DCD, BIAS_MAX, device)[0],
                R=_ints(r_rows or M, N, seed + 3, 0x0002E7A5, 0x00056B3B, RES_MAX, device))


def exact_bound(ops, K, with_bias=True, with_res=True):
    """Upper bound of |any partial sum in any order| for these operands: K |a| |w| + |bias| + |residual|."""
    b = K * float(ops["A"].abs().max()) * float(ops["W"].abs().max())
    if with_bias:
        b += float(ops["bias"].abs().max())
    if with_res:
        b += float(ops["R"].abs().max())
    return b


def is_exact_16(x):
    """Every element is an integer that bf16 AND fp16 hold exactly."""
    return bool((x == x.round()).all()) and bool((x.to(torch.bfloat16).double() == x).all()) and bool((x.to(torch.float16).double() == x).all())


def rne16(x, fmt):
    """One-step round-to-nearest-even of fp64 values to bf16 (8 significant bits) or fp16 (11; normal range, no overflow here), in integer arithmetic:
    the statement the kernels' 16-bit stores are held to.  Returned as fp64."""
    bits = 8 if fmt == "bf16" else 11
    m, e = torch.frexp(x)                               # x = m 2^e, 0.5 <= |m| < 1
    s = m * float(1 << bits)                            # exact: a scaling by a power of two
    fl = torch.floor(s)
    frac = s - fl
    up = (frac > 0.5) | ((frac == 0.5) & (fl % 2 != 0))
    return torch.ldexp(fl + up.to(x.dtype), e - bits)


# ---- the operation ----------------------------------------------------------------------------------------------------------------------------------
def gemm_ref64(A, W, bias=None, R=None, act=ACT_NONE, r_mod=0, k0=0, k1=None):
    """act(A[:, k0:k1] . W[:, k0:k1]^T + bias) + R[res_row(m)] in fp64 (the epilogue order of every kernel: bias, activation, then the residual)."""
    y = A[:, k0:k1].double() @ W[:, k0:k1].double().t()
    if bias is not None:
        y = y + bias.double()[None, :]
    if act == ACT_RELU:
        y = torch.relu(y)
    elif act == ACT_GELU:
        y = torch.nn.functional.gelu(y)
    if R is not None:
        m = torch.arange(A.shape[0], device=A.device)
        y = y + R.double()[res_row(m, r_mod)]
    return y


def split_parts_ref64(A, W, bias, R, parts, split_rows, r_mod=0):
    """The `parts` partial results of a GEMM split along K: part p holds the k-range [p K / parts, (p + 1) K / parts) of the rows below split_rows, bias and
    residual in part 0; the rows from split_rows on are complete in part 0 and absent (None rows: untouched) in the others.  -> list of (values, lo, hi)."""
    M, K = A.shape
    out = []
    for p in range(parts):
        k0, k1 = p * (K // parts), (p + 1) * (K // parts)
        y = gemm_ref64(A[:split_rows], W, bias if p == 0 else None, R[:split_rows] if (p == 0 and R is not None) else None, ACT_NONE, r_mod, k0, k1)
        if p == 0 and split_rows < M:
            m = torch.arange(split_rows, M, device=A.device)
            tail = A[split_rows:].double() @ W.double().t() + (bias.double()[None, :] if bias is not None else 0) + (R.double()[res_row(m, r_mod)] if R is not None else 0)
            y = torch.cat([y, tail])
        out.append((y, 0, y.shape[0]))
    return out


def layernorm_ref64(x, gamma, beta, eps):
    return torch.nn.functional.layer_norm(x.double(), (x.shape[-1],), gamma.double(), beta.double(), eps)


# ---- canary-filled padded buffers -------------------------------------------------------------------------------------------------------------------
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def as_int(t):
    return t.view(_INT[t.dtype])


def canvas(n_elems, dtype, device="cpu"):
    """A flat buffer of n_elems elements of `dtype` in which every element holds the pattern."""
    return torch.full((n_elems,), PAT32 if dtype == torch.float32 else PAT16, dtype=_INT[dtype], device=device).view(dtype)


def place(flat, origin, ld, phys_rows, values):
    """Write values (len(phys_rows), n) into the flat buffer as rows phys_rows of a (.., ld) matrix whose element (0, 0) is flat[origin]; values are
    converted to the buffer's format with torch's conversion (exact for the exact operands' fp32 results; one-step RNE from fp32 for 16 bits)."""
    n = values.shape[1]
    idx = origin + phys_rows.to(torch.int64)[:, None] * ld + torch.arange(n, dtype=torch.int64, device=flat.device)[None, :]
    v = values.to(torch.float32) if values.dtype == torch.float64 else values
    flat[idx.reshape(-1)] = v.to(flat.dtype).reshape(-1)
    return idx.reshape(-1)


def compare(got, want, window=None):
    """Bitwise comparison of two flat buffers of one format.  -> (elements that differ inside the window, outside it); window = the flat indices
    of the elements a kernel may write (None: everything counts as inside)."""
    diff = as_int(got) != as_int(want)
    if window is None:
        return int(diff.sum()), 0
    inside = torch.zeros_like(diff)
    inside[window] = True
    return int((diff & inside).sum()), int((diff & ~inside).sum())
