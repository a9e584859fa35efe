"""The dense GEMM's engine-only forms, host side: tests/gemm_forms_ref.py -- the reference and the exact-operand generator that
tests/test_gpu_gemm_forms.py holds the kernels to -- checked on hand-written cases and against a deliberately wrong variant of itself, the exactness
bounds asserted from the generated data at every shape of the GPU test, and the argument checks of ma_op_gemm_dense / ma_op_ln_rows / ma_op_layernorm
(which all come before anything touches a device).  No GPU needed."""
import ctypes as C

import pytest
import torch

import gemm_forms_ref as R
from meshanything_amd import _lib, build

INVALID = -1
P = 4096                                                           # a non-null, 16-byte aligned address that is never dereferenced

# (M, N, K, residual rows or None for M): every shape of tests/test_gpu_gemm_forms.py
SHAPES = [(3328, 3072, 128, None), (3345, 3072, 128, None), (3428, 3072, 128, None), (3345, 3072, 192, None),        # one-tile kernel, splittable
          (3328, 2820, 128, None), (3328, 2824, 128, None),                                                          # 16-bit only, ragged right edge
          (3341, 3072, 128, None),                                                                                   # persistent kernel (+ KV planes)
          (3100, 3072, 128, 256),                                                                                    # row map + broadcast residual
          (300, 200, 96, 100), (300, 200, 192, 100), (300, 96, 64, 100),                                             # 128- / 64-row tiles, fp32 kernels
          (512, 1024, 1024, None), (529, 1024, 1024, None), (612, 1024, 1024, None), (512, 1024, 1152, None), (4864, 1024, 1024, None),   # split along K
          (600, 512, 128, None)]                                                                                     # part 1 | 2 without a 256-row tile


@pytest.fixture(scope="module")
def lib():
    build.build(force=False, verbose=False)
    return _lib.load()


# ---- the exact-operand generator ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,r_rows", SHAPES)
def test_exact_operands_stay_exact_at_every_shape(M, N, K, r_rows):
    ops = R.exact_operands(M, N, K, seed=M + N + K, r_rows=r_rows)
    assert ops["A"].shape == (M, K) and ops["W"].shape == (N, K) and ops["bias"].shape == (N,) and ops["R"].shape == (r_rows or M, N)
    for name in ("A", "W"):
        assert R.is_exact_16(ops[name]), name                      # the 16-bit operands: exact in bf16 and in fp16
    for name in ("bias", "R"):                                     # the fp32 operands: integers
        assert bool((ops[name] == ops[name].round()).all()) and bool((ops[name].float().double() == ops[name]).all()), name
    bound = R.exact_bound(ops, K)
    assert bound < R.EXACT_LIMIT                                   # any partial sum in any order is an integer fp32 holds
    assert bound < R.FP16_MAX                                      # and the 16-bit output stays finite in IEEE half
    # the data is what the bound was computed for, and not degenerate: all values occur, rows and columns differ
    assert float(ops["A"].abs().max()) == R.A_MAX and float(ops["W"].abs().max()) == R.W_MAX
    assert len(torch.unique(ops["A"])) == 2 * R.A_MAX + 1 and len(torch.unique(ops["W"])) == 2 * R.W_MAX + 1
    assert not torch.equal(ops["A"][0], ops["A"][1]) and not torch.equal(ops["A"][:, 0], ops["A"][:, 1])
    assert not torch.equal(ops["A"][:64, :64], ops["W"][:64, :64]) and not torch.equal(ops["A"][:64, :64], ops["A"][:64, :64].t())


def test_exact_operands_depend_on_the_seed_and_not_on_the_device_arithmetic():
    a, b = R.exact_operands(40, 24, 32, seed=5), R.exact_operands(40, 24, 32, seed=6)
    assert not torch.equal(a["A"], b["A"]) and not torch.equal(a["W"], b["W"])
    assert torch.equal(a["A"], R.exact_operands(40, 24, 32, seed=5)["A"])
    # the generator of a larger matrix restricted to a corner is the smaller matrix: an element is a function of (row, column, seed) alone
    assert torch.equal(R.exact_operands(80, 24, 64, seed=5)["A"][:40, :32], a["A"])
    # the mix stays inside int64 without wrapping: the same integers with Python's unbounded ones
    def h(r, c, seed, k1, k2):
        m = 0xFFFFFFFF
        x = (r * k1 + c * k2 + seed * 0x9E3779B1 + 0x7F4A7C15) & m
        x = ((x ^ (x >> 15)) * 0x2C1B3C6D) & m
        x = ((x ^ (x >> 12)) * 0x297A2D39) & m
        return x ^ (x >> 15)
    for r, c in ((0, 0), (39, 31), (17, 5)):
        assert int(a["A"][r, c]) == h(r, c, 5, 0x01000193, 0x0001F123) % 7 - 3
    big = R._hash(torch.tensor([[1 << 20]]), torch.tensor([[1 << 20]]), 1 << 20, 0x01000193, 0x0001F123)
    assert int(big) == h(1 << 20, 1 << 20, 1 << 20, 0x01000193, 0x0001F123)


def test_one_step_rounding_to_16_bits():
    """rne16 on hand-written values, ties included, and torch's own conversion of fp32 agrees with it on every integer the exact results can take."""
    x = torch.tensor([256.0, 257.0, 258.0, 259.0, 260.0, 262.0, 263.0, -258.0, -262.0, 1000.0, 2049.0, 2050.0, 2051.0, 4099.0, 0.0, 3.0])
    # bf16: 8 significant bits -- steps of 2 from 256, 4 from 512, 8 from 1024, 16 from 2048; a tie goes to the even significand
    assert R.rne16(x.double(), "bf16").tolist() == [256.0, 256.0, 258.0, 260.0, 260.0, 262.0, 264.0, -258.0, -262.0, 1000.0, 2048.0, 2048.0, 2048.0, 4096.0, 0.0, 3.0]
    assert R.rne16(torch.tensor([1026.0, 1028.0, 1036.0, 1037.0, -1028.0, -1036.0], dtype=torch.float64), "bf16").tolist() == [1024.0, 1024.0, 1040.0, 1040.0, -1024.0, -1040.0]
    # fp16: 11 significant bits -- steps of 2 from 2048, 4 from 4096
    assert R.rne16(x.double(), "fp16").tolist() == [256.0, 257.0, 258.0, 259.0, 260.0, 262.0, 263.0, -258.0, -262.0, 1000.0, 2048.0, 2050.0, 2052.0, 4100.0, 0.0, 3.0]
    n = torch.arange(-R.FP16_MAX, R.FP16_MAX + 1, dtype=torch.float64)
    assert torch.equal(n.float().to(torch.bfloat16).double(), R.rne16(n, "bf16"))
    assert torch.equal(n.float().to(torch.float16).double(), R.rne16(n, "fp16"))


# ---- addressing helpers, hand-written cases ---------------------------------------------------------------------------------------------------------
def test_row_map_residual_row_and_parts():
    assert [R.row_map(m, 0, 0, 0) for m in (0, 5, 300)] == [0, 5, 300]
    assert [R.row_map(m, 256, 257, 1) for m in (0, 255, 256, 511, 512, 3099)] == [1, 256, 258, 513, 515, 12 * 257 + 28]
    assert [R.row_map(m, 100, 130, 7) for m in (0, 99, 100, 299)] == [7, 106, 137, 366]
    assert R.row_map(torch.tensor([0, 99, 100, 299]), 100, 130, 7).tolist() == [7, 106, 137, 366]
    # the physical rows a (256, 257, 1) map skips: one per 257, the first of each block
    used = set(R.row_map(torch.arange(3100), 256, 257, 1).tolist())
    assert [r for r in range(3113) if r not in used] == [257 * b for b in range(13)]
    assert [R.res_row(m, 256) for m in (0, 255, 256, 700)] == [0, 255, 0, 188] and R.res_row(700, 0) == 700
    assert R.part_rows(3341, 0) == (0, 3341) and R.part_rows(3341, 1) == (0, 3328) and R.part_rows(3341, 2) == (3328, 3341)
    assert R.part_rows(600, 1) == (0, 512) and R.part_rows(600, 2) == (512, 600)
    assert R.part_rows(512, 2) == (512, 512) and R.part_rows(200, 1) == (0, 0)


def test_kv_plane_address():
    T, col0, ms, stride = 257, 1024, 300, 16 * 300 * 64 + 64
    assert R.kv_index(0, 1024, T, col0, ms, stride) == (0, 0)                                   # first K element of sample 0, position 0
    assert R.kv_index(0, 2048, T, col0, ms, stride) == (1, 0)                                   # first V element
    assert R.kv_index(5, 1024 + 64 * 3 + 9, T, col0, ms, stride) == (0, (3 * 300 + 5) * 64 + 9)
    assert R.kv_index(257, 3071, T, col0, ms, stride) == (1, stride + (15 * 300 + 0) * 64 + 63)  # sample 1 starts at row 257
    assert R.kv_index(3327, 2047, T, col0, ms, stride) == (0, 12 * stride + (15 * 300 + 243) * 64 + 63)
    m, c = torch.tensor([5, 257]), torch.tensor([1024 + 201, 3071])
    plane, el = R.kv_index(m, c, T, col0, ms, stride)
    assert plane.tolist() == [0, 1] and el.tolist() == [(3 * 300 + 5) * 64 + 9, stride + 15 * 300 * 64 + 63]
    # all addresses of a sample's rows are distinct and inside its plane
    mm = torch.arange(257)[:, None].expand(257, 1024).reshape(-1)
    cc = (1024 + torch.arange(1024))[None, :].expand(257, 1024).reshape(-1)
    _, el = R.kv_index(mm, cc, T, col0, ms, stride)
    assert len(torch.unique(el)) == 257 * 1024 and int(el.max()) < 16 * 300 * 64


# ---- the reference against itself -------------------------------------------------------------------------------------------------------------------
def _small_case(act=R.ACT_RELU):
    M, N, K, grp, gstride, off, r_mod, ldc = 70, 24, 64, 20, 26, 3, 20, 32
    ops = R.exact_operands(M, N, K, seed=11, r_rows=r_mod)
    ref = R.gemm_ref64(ops["A"], ops["W"], ops["bias"], ops["R"], act, r_mod)
    rows = R.row_map(torch.arange(M), grp, gstride, off)
    n_phys = int(rows.max()) + 1
    origin = 2 * ldc
    want = R.canvas((n_phys + 4) * ldc, torch.float32)
    window = R.place(want, origin, ldc, rows, ref)
    return ops, ref, rows, want, window, (M, N, K, grp, gstride, off, r_mod, ldc, origin, n_phys, act)


def test_reference_gemm_by_hand_and_in_a_canary_buffer():
    ops, ref, rows, want, window, (M, N, K, grp, gstride, off, r_mod, ldc, origin, n_phys, act) = _small_case()
    for m, n in ((0, 0), (19, 23), (20, 1), (69, 5)):               # element by element, in Python integers
        s = sum(int(ops["A"][m, k]) * int(ops["W"][n, k]) for k in range(K)) + int(ops["bias"][n])
        assert int(ref[m, n]) == max(s, 0) + int(ops["R"][m % r_mod, n])
        assert float(want[origin + int(rows[m]) * ldc + n]) == float(ref[m, n])
    assert float(ref.abs().max()) <= R.exact_bound(ops, K)
    assert (ref < 0).any() and (ref > 0).any()
    # the canvas: every element outside the window still holds the pattern, every element inside holds a value
    ints = R.as_int(want)
    inside = torch.zeros(want.shape, dtype=torch.bool)
    inside[window] = True
    assert int(inside.sum()) == M * N and bool((ints[~inside] == R.PAT32).all()) and not bool((ints[inside] == R.PAT32).any())
    assert R.compare(want, want.clone(), window) == (0, 0)
    # a GEMM split along K adds up to the unsplit one, with bias and residual in part 0 only
    full = R.gemm_ref64(ops["A"], ops["W"], ops["bias"], ops["R"][R.res_row(torch.arange(M), r_mod)], R.ACT_NONE)
    Rfull = ops["R"][R.res_row(torch.arange(M), r_mod)]
    parts = R.split_parts_ref64(ops["A"], ops["W"], ops["bias"], Rfull, 4, 50)
    assert [p[0].shape[0] for p in parts] == [70, 50, 50, 50]
    total = parts[0][0].clone()
    for y, lo, hi in parts[1:]:
        total[lo:hi] += y
    assert torch.equal(total, full)
    assert torch.equal(parts[1][0], ops["A"][:50, 16:32] @ ops["W"][:, 16:32].t())


@pytest.mark.parametrize("wrong", ["row_map_off_by_one", "residual_not_broadcast", "transposed_fragment", "shifted_k", "dropped_k_tile", "relu_after_residual",
                                   "one_small_element", "overrun_past_the_right_edge", "overrun_into_a_skipped_row", "rounding_truncates"])
def test_a_wrong_variant_fails_the_comparison(wrong):
    """What the GPU test's comparison must catch: each deliberately wrong variant of the reference differs from the right one in the bits."""
    ops, ref, rows, want, window, (M, N, K, grp, gstride, off, r_mod, ldc, origin, n_phys, act) = _small_case()
    A, W, b, Rr = ops["A"], ops["W"], ops["bias"], ops["R"]
    got = R.canvas(want.numel(), torch.float32)
    if wrong == "row_map_off_by_one":
        R.place(got, origin, ldc, R.row_map(torch.arange(M), grp, gstride, off + 1), ref)
    elif wrong == "residual_not_broadcast":
        R.place(got, origin, ldc, rows, R.gemm_ref64(A, W, b, R.exact_operands(M, N, K, seed=11)["R"], act, 0))
    elif wrong == "transposed_fragment":
        A2 = A.clone(); A2[:16, :16] = A[:16, :16].t()
        R.place(got, origin, ldc, rows, R.gemm_ref64(A2, W, b, Rr, act, r_mod))
    elif wrong == "shifted_k":
        R.place(got, origin, ldc, rows, R.gemm_ref64(torch.roll(A, 8, dims=1), W, b, Rr, act, r_mod))
    elif wrong == "dropped_k_tile":
        R.place(got, origin, ldc, rows, R.gemm_ref64(A, W, b, Rr, act, r_mod, 0, K - 32))
    elif wrong == "relu_after_residual":
        R.place(got, origin, ldc, rows, torch.relu(R.gemm_ref64(A, W, b, Rr, R.ACT_NONE, r_mod)))
    elif wrong == "one_small_element":
        r2 = ref.clone(); r2[33, 7] += 1                            # one unit in one element: 1e-4 of the largest value, invisible to a max-norm tolerance
        assert 1 / float(ref.abs().max()) < 6e-3
        R.place(got, origin, ldc, rows, r2)
    elif wrong == "overrun_past_the_right_edge":
        R.place(got, origin, ldc, rows, torch.cat([ref, ref[:, :1]], dim=1))
    elif wrong == "overrun_into_a_skipped_row":
        R.place(got, origin, ldc, rows, ref)
        got[origin + 23 * ldc] = 0.0                                # physical row 23 = the gap behind the first group (rows 3 .. 22)
        assert 23 not in rows.tolist()
    elif wrong == "rounding_truncates":
        w16, g16 = R.canvas(want.numel(), torch.bfloat16), R.canvas(want.numel(), torch.bfloat16)
        win = R.place(w16, origin, ldc, rows, ref)
        trunc = (R.as_int(ref.float().contiguous()) >> 16).to(torch.int16).view(torch.bfloat16)
        R.place(g16, origin, ldc, rows, trunc)
        assert torch.equal(w16[win].double(), R.rne16(ref, "bf16").reshape(-1))       # the right one IS the one-step rounding
        bad_in, bad_out = R.compare(g16, w16, win)
        assert bad_in > 0 and bad_out == 0
        return
    bad_in, bad_out = R.compare(got, want, window)
    assert bad_in + bad_out > 0
    if wrong.startswith("overrun"):
        assert bad_in == 0 and bad_out >= 1                         # the window itself is right: only the canary shows it
    if wrong == "one_small_element":
        assert (bad_in, bad_out) == (1, 0)


def test_layernorm_reference():
    x = torch.tensor([[1.0, 2.0, 3.0, 6.0]])
    y = R.layernorm_ref64(x, torch.tensor([1.0, 1.0, 2.0, 1.0]), torch.tensor([0.0, 0.5, 0.0, 0.0]), 0.0)
    sd = (3.5) ** 0.5
    assert torch.allclose(y, torch.tensor([[-2 / sd, -1 / sd + 0.5, 0.0, 3 / sd]], dtype=torch.float64), atol=1e-15)


# ---- argument checks: all before the first launch ---------------------------------------------------------------------------------------------------
def _ln_rows_args(**kw):
    a = dict(x=P, ldx=1024, xin_grp=0, xin_gstride=0, xin_off=0, g=P, b=P, eps=1e-5, y32=P + 64, ld32=1024, act=None, lda=0, act_dtype=0,
             yout_grp=0, yout_gstride=0, yout_off=0, rows=8, D=1024, parts=1, part_stride=0, split_rows=0, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


LN_BAD = [dict(D=1026, ldx=1028, ld32=1028), dict(D=4100, ldx=4100, ld32=4100), dict(D=0), dict(D=-4), dict(rows=0), dict(rows=-1),
          dict(parts=3, part_stride=8192), dict(parts=0), dict(parts=8, part_stride=8192), dict(parts=2, part_stride=8192, D=768, ldx=768, ld32=768),
          dict(parts=4, part_stride=8192, D=512, ldx=512, ld32=512), dict(split_rows=-1), dict(split_rows=9), dict(parts=2, part_stride=8192, split_rows=9)]


def test_ln_rows_refuses_what_the_kernel_cannot_compute(lib):
    f = lib.ma_op_ln_rows
    for bad in LN_BAD:
        assert f(*_ln_rows_args(**bad)) == INVALID, bad
        assert b"ma_op_ln_rows" in lib.ma_last_error(None)
    more = [dict(x=None), dict(g=None), dict(b=None), dict(y32=None), dict(ldx=1020), dict(ldx=1026), dict(ld32=1000), dict(act=P, lda=1000, act_dtype=1),
            dict(act_dtype=2), dict(x=P + 4), dict(xin_grp=-1), dict(yout_grp=4, yout_gstride=3), dict(parts=2, part_stride=0), dict(parts=2, part_stride=8190),
            dict(y32=P, ld32=1028, ldx=1024), dict(y32=P, yout_off=1)]
    for bad in more:
        assert f(*_ln_rows_args(**bad)) == INVALID, bad


def test_layernorm_refuses_what_the_kernel_cannot_compute(lib):
    f = lib.ma_op_layernorm
    def call(rows=8, D=1024, ldx=None, ldy=None, x=P):
        return f(x, ldx or D, P, P, 1e-5, P + 64, ldy or D, rows, D, None)
    for kw in (dict(D=1026), dict(D=4100), dict(D=0), dict(D=-4), dict(rows=0), dict(rows=-1), dict(D=1024, ldx=1000), dict(D=1024, ldy=1022), dict(x=None)):
        assert call(**kw) == INVALID, kw
        assert b"ma_op_layernorm" in lib.ma_last_error(None)


def _dense_args(**kw):
    a = dict(precision=1, impl=0, M=300, N=256, K=128, act=0, lda=136, ldr=260, ldc=264, ldcb=272, r_mod=0, cmap_grp=0, cmap_gstride=0, cmap_off=0, part=0,
             max_parts=0, kv_max_seq=0, kv_T=0, kv_col0=0, variant=6, tile256=2, part_stride=0, kv_row_stride=0, A=P, W=P, bias=P, R=None, C=P, Cb=P,
             kv_k=None, kv_v=None)
    assert set(kw) <= set(a) | {"struct_size"}
    a.update(kw)
    size = a.pop("struct_size", None)
    s = _lib.GemmDenseArgs(**a)
    if size is not None:
        s.struct_size = size
    return s


def test_gemm_dense_refuses_bad_arguments_on_the_host(lib):
    f = lib.ma_op_gemm_dense
    assert C.sizeof(_lib.GemmDenseArgs) == 26 * 4 + 2 * 8 + 8 * 8
    assert f(None, None) == INVALID
    kvok = dict(N=768, ldc=772, ldcb=776, kv_k=P, kv_v=P, kv_col0=256, kv_T=10, kv_max_seq=12, kv_row_stride=4 * 12 * 64)
    bad = [dict(struct_size=0), dict(struct_size=100), dict(precision=2), dict(precision=-1), dict(A=None), dict(W=None), dict(C=None, Cb=None),
           dict(M=0), dict(N=-1), dict(K=0), dict(K=100, lda=104), dict(act=3), dict(act=-1), dict(lda=120), dict(lda=132), dict(ldc=252), dict(ldc=262),
           dict(R=P, ldr=250), dict(R=P, ldr=258), dict(ldcb=250), dict(ldcb=258), dict(A=P + 8), dict(C=P + 4), dict(bias=P + 4),
           dict(cmap_grp=-1), dict(cmap_grp=8, cmap_gstride=7), dict(cmap_grp=8, cmap_gstride=8, cmap_off=-1), dict(r_mod=-1),
           dict(part=3), dict(part=-1), dict(part=1, cmap_grp=100, cmap_gstride=130), dict(part=2, r_mod=100, R=P), dict(part=1, r_mod=100, R=P),
           dict(max_parts=5), dict(max_parts=-1), dict(max_parts=4, part_stride=0, Cb=None), dict(max_parts=4, part_stride=1 << 20, C=None), dict(max_parts=2, part_stride=1002, Cb=None),
           dict(kv_k=P), dict(kv_v=P), dict(kvok, kv_col0=250), dict(kvok, N=512, ldc=516, ldcb=520), dict(kvok, kv_T=0), dict(kvok, kv_T=13),
           dict(kvok, kv_row_stride=4 * 12 * 64 - 8), dict(kvok, kv_row_stride=4 * 12 * 64 + 4), dict(kvok, Cb=None), dict(kvok, kv_k=P + 2),
           dict(tile256=3), dict(tile256=-1),
           dict(precision=0, Cb=None, lda=130), dict(precision=0), dict(precision=0, Cb=None, part=1), dict(precision=0, Cb=None, max_parts=2, part_stride=1 << 20),
           dict(precision=0, Cb=None, impl=2), dict(precision=0, C=None)]
    for kw in bad:
        s = _dense_args(**kw)
        assert f(C.byref(s), None) == INVALID, kw
        assert b"ma_op_gemm_dense" in lib.ma_last_error(None) or b"gemm256" in lib.ma_last_error(None), kw
        assert (s.out_parts, s.out_split_rows, s.out_kv_rows, s.out_rows256) in ((0, 0, 0, 0), (1, 0, 0, 0)), kw
