"""The dense GEMM dispatcher's engine-only forms and the LayerNorm row kernel at kernel level (MI355X), through the test aids ma_op_gemm_dense and
ma_op_ln_rows: split along K, row map and broadcast residual on every tile, the 16-bit-only ragged right edge of the 256-row tile, the persistent kernel's
KV epilogue, a GEMM by row parts -- each with padded leading dimensions inside a buffer pre-filled with a fixed bit pattern.

Method (tests/gemm_forms_ref.py): on EXACT operands every correct kernel returns the fp64 result bit for bit, whatever its summation order, and its 16-bit
output is the one-step round-to-nearest-even of it; so the comparison is equality of bits on the window and of the pattern everywhere else.  Each form
also runs once on seeded-normal data with GELU, held to the tolerances of test_gpu_kernels.py.  Every case asserts what the dispatcher reports it chose
(rows256, parts, split_rows, kv_rows): the shapes are the smallest that select each branch at 256 CUs, and a case cannot quietly test another kernel.
Tensors and fp64 references are computed on the device with stock torch ops."""
import ctypes as C
import math

import pytest
import torch

import gemm_forms_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 2                                                          # pattern rows in front of and behind every output window
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from meshanything_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    torch.backends.cuda.matmul.allow_tf32 = False
    return _lib.load()


class _H16:
    def __init__(self, name):
        self.name, self.tdt, self.code = name, (torch.bfloat16 if name == "bf16" else torch.float16), (1 if name == "bf16" else 2)


@pytest.fixture(params=["bf16", "fp16"])
def h16(request, lib):
    h = _H16(request.param)
    assert lib.ma_op_set_half_dtype(h.code) == 0
    yield h
    lib.ma_op_set_half_dtype(1)


@pytest.fixture(scope="module")
def cus256():
    """The shapes of the path-dependent cases select their branch by the number of CUs (a round counts as reasonably full from 154 of 256 tiles)."""
    def need():
        n = torch.cuda.get_device_properties(0).multi_processor_count
        if n != 256:
            pytest.skip(f"the shapes of this case select the dispatcher branch under test at 256 CUs; this device reports {n}")
    return need


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _up(n, a):
    return (n + a - 1) // a * a


# modes of a case: (data, act)
EXACT, EXACT_RELU, NORMAL_GELU = ("exact", R.ACT_NONE), ("exact", R.ACT_RELU), ("normal", R.ACT_GELU)
MODES = pytest.mark.parametrize("mode", [EXACT, EXACT_RELU, NORMAL_GELU], ids=["exact", "exact_relu", "normal_gelu"])


class Problem:
    """One GEMM problem on the device: operands in padded buffers (lda > K; ldc, ldr, ldcb all different), the fp64 reference, and pattern-filled output
    buffers whose window starts GUARD rows in."""

    def __init__(self, h, M, N, K, out, mode=EXACT, bias=True, res=False, cmap=(0, 0, 0), r_mod=0, prec=1, impl=0, ldcb=None, max_parts=0, seed=0, tile256=2):
        self.h, self.M, self.N, self.K, self.out, self.cmap, self.r_mod, self.prec, self.impl, self.tile256 = h, M, N, K, out, cmap, r_mod, prec, impl, tile256
        self.data, self.act = mode
        self.max_parts = max_parts
        in_dt = h.tdt if prec == 1 else torch.float32
        r_rows = r_mod if r_mod > 0 else M
        if self.data == "exact":
            ops = R.exact_operands(M, N, K, seed=seed + M + 3 * N + 5 * K, device=DEV, r_rows=r_rows)
            assert R.exact_bound(ops, K) < min(R.EXACT_LIMIT, R.FP16_MAX)
            A, W, b, Rr = ops["A"], ops["W"], ops["bias"], ops["R"]
        else:
            g = torch.Generator(device=DEV).manual_seed(seed + M + 3 * N + 5 * K)
            A = torch.randn(M, K, generator=g, device=DEV) + torch.linspace(-1, 1, K, device=DEV)[None, :] * 0.5
            W = torch.randn(N, K, generator=g, device=DEV) / math.sqrt(K) + torch.linspace(0, 1, N, device=DEV)[:, None] * 0.02
            b = torch.randn(N, generator=g, device=DEV) * 0.1
            Rr = torch.randn(r_rows, N, generator=g, device=DEV)
        self.A = A.to(in_dt)                                       # (what the kernel reads: exact for the exact operands, rounded for the normal ones)
        self.W = W.to(in_dt).contiguous()
        self.bias = b.float().contiguous() if bias else None
        self.R = Rr.float() if res else None
        self.ref = R.gemm_ref64(self.A, self.W, self.bias, self.R, self.act, r_mod)
        self.lda = K + (8 if prec == 1 else 4)
        self.ldc, self.ldr, self.ldcb = _up(N, 4) + 4, _up(N, 4) + 8, (ldcb or _up(N, 8) + 16)
        self.Abuf = R.canvas(M * self.lda, in_dt, DEV)
        R.place(self.Abuf, 0, self.lda, torch.arange(M, device=DEV), self.A)
        self.Rbuf = None
        if res:
            self.Rbuf = R.canvas(r_rows * self.ldr, torch.float32, DEV)
            R.place(self.Rbuf, 0, self.ldr, torch.arange(r_rows, device=DEV), self.R)
        self.rows = R.row_map(torch.arange(M, device=DEV), *cmap)
        self.n_phys = int(self.rows.max()) + 1
        self.part_stride = (self.n_phys + GUARD) * self.ldc + 68 if max_parts >= 2 else 0
        self.kv = None
        self.fresh()

    # ---- buffers
    def c_elems(self):
        return (self.n_phys + 2 * GUARD) * self.ldc + (3 * self.part_stride if self.max_parts >= 2 else 0)

    def blank_c(self):
        return R.canvas(self.c_elems(), torch.float32, DEV)

    def blank_cb(self):
        return R.canvas((self.n_phys + 2 * GUARD) * self.ldcb, self.h.tdt, DEV)

    def fresh(self):
        self.C = self.blank_c() if self.out in ("f32", "both") else None
        self.Cb = self.blank_cb() if self.out in ("h16", "both") else None
        if self.kv:
            self.kv["k"], self.kv["v"] = self.blank_plane(), self.blank_plane()

    def with_kv(self, T, col0, max_seq):
        stride = (col0 // 64) * max_seq * 64 + 64                  # (a padded sample stride: the gap must stay untouched)
        self.kv = dict(T=T, col0=col0, max_seq=max_seq, stride=stride, samples=(self.M + T - 1) // T)
        self.fresh()
        return self

    def blank_plane(self):
        return R.canvas(64 + self.kv["samples"] * self.kv["stride"] + 64, self.h.tdt, DEV)

    # ---- the call
    def call(self, lib, part=0, max_parts=None, act=None):
        from meshanything_amd import _lib
        isz = 2 if self.prec == 1 else 4
        a = _lib.GemmDenseArgs(precision=self.prec, impl=self.impl, M=self.M, N=self.N, K=self.K, act=self.act if act is None else act, lda=self.lda, ldr=self.ldr,
                               ldc=self.ldc, ldcb=self.ldcb, r_mod=self.r_mod, cmap_grp=self.cmap[0], cmap_gstride=self.cmap[1], cmap_off=self.cmap[2], part=part,
                               max_parts=self.max_parts if max_parts is None else max_parts, variant=6, tile256=self.tile256, part_stride=self.part_stride,
                               A=self.Abuf.data_ptr(), W=self.W.data_ptr(), bias=None if self.bias is None else self.bias.data_ptr(),
                               R=None if self.Rbuf is None else self.Rbuf.data_ptr(),
                               C=None if self.C is None else self.C.data_ptr() + GUARD * self.ldc * 4,
                               Cb=None if self.Cb is None else self.Cb.data_ptr() + GUARD * self.ldcb * 2)
        assert isz * self.lda % 16 == 0
        if self.kv:
            a.kv_k, a.kv_v = self.kv["k"].data_ptr() + 128, self.kv["v"].data_ptr() + 128
            a.kv_row_stride, a.kv_max_seq, a.kv_T, a.kv_col0 = self.kv["stride"], self.kv["max_seq"], self.kv["T"], self.kv["col0"]
        _lib.check(lib.ma_op_gemm_dense(C.byref(a), _stream()), None)
        torch.cuda.synchronize()
        return dict(rows256=a.out_rows256, parts=a.out_parts, split_rows=a.out_split_rows, kv_rows=a.out_kv_rows)

    # ---- the comparison
    def window(self, ld, lo=0, hi=None, n0=0, n1=None, origin=None):
        """Flat indices of columns [n0, n1) of logical rows [lo, hi) in an output buffer of leading dimension ld."""
        hi, n1 = self.M if hi is None else hi, self.N if n1 is None else n1
        origin = GUARD * ld if origin is None else origin
        idx = origin + self.rows[lo:hi, None] * ld + torch.arange(n0, n1, device=DEV)[None, :]
        return idx.reshape(-1)

    def _check(self, got, want, win, ref, tol, what):
        bad_in, bad_out = R.compare(got, want, win)
        assert bad_out == 0, f"{what}: {bad_out} elements outside the window no longer hold the pattern"
        if self.data == "exact":
            assert bad_in == 0, f"{what}: {bad_in} of {win.numel()} window elements differ from the exact result in the bits"
        else:
            scale = max(1e-6, float(ref.abs().max()))
            err = float((got[win].double() - ref.reshape(-1)).abs().max()) / scale
            assert err < tol, f"{what}: off by {err:.3e} of the largest value"

    def verify(self, lo=0, hi=None, kv_rows=0):
        """Rows [lo, hi) of the outputs hold the reference, everything else the pattern (kv_rows: the K | V columns of the leading rows left for the planes)."""
        hi = self.M if hi is None else hi
        ref = self.ref[lo:hi]
        if self.C is not None:
            want = self.blank_c()
            win = self.window(self.ldc, lo, hi)
            want[win] = ref.float().reshape(-1)
            self._check(self.C, want, win, ref, 3e-5, "fp32 output")
        if self.Cb is not None:
            r16 = (R.rne16(ref, self.h.name) if self.data == "exact" else ref).float().to(self.h.tdt)
            want = self.blank_cb()
            kvr = min(max(kv_rows, lo), hi)
            c0 = self.kv["col0"] if kv_rows else self.N
            wins = [self.window(self.ldcb, lo, kvr, 0, c0), self.window(self.ldcb, kvr, hi)]
            want[wins[0]] = r16[:kvr - lo, :c0].reshape(-1)
            want[wins[1]] = r16[kvr - lo:].reshape(-1)
            refs = torch.cat([ref[:kvr - lo, :c0].reshape(-1), ref[kvr - lo:].reshape(-1)])
            self._check(self.Cb, want, torch.cat(wins), refs, 6e-3, "16-bit output")
            if self.C is not None:                                 # where both exist the 16-bit copy is the rounded fp32 output, exactly
                w32, w16 = self.window(self.ldc, lo, hi), self.window(self.ldcb, lo, hi)
                assert torch.equal(R.as_int(self.Cb[w16]), R.as_int(self.C[w32].to(self.h.tdt))), "16-bit copy is not the rounded fp32 output"

    def verify_planes(self, kv_rows):
        kv = self.kv
        m = torch.arange(kv_rows, device=DEV)[:, None]
        col = torch.arange(kv["col0"], 3 * kv["col0"], device=DEV)[None, :]
        plane, el = R.kv_index(m, col, kv["T"], kv["col0"], kv["max_seq"], kv["stride"])
        ref = self.ref[:kv_rows, kv["col0"]:]
        r16 = (R.rne16(ref, self.h.name) if self.data == "exact" else ref).float().to(self.h.tdt)
        for p, name in ((0, "k"), (1, "v")):
            sel = (plane == p).expand(kv_rows, 2 * kv["col0"])
            want = self.blank_plane()
            win = (64 + el.expand(kv_rows, 2 * kv["col0"])[sel]).reshape(-1)
            assert len(torch.unique(win)) == win.numel() == kv_rows * kv["col0"]
            want[win] = r16[sel]
            self._check(kv[name], want, win, ref[sel], 6e-3, f"KV plane {name}")


def _expect(got, **want):
    assert {k: got[k] for k in want} == want, f"the dispatcher chose {got}, the case is written for {want}"


# ---- the one-tile 256 x 256 kernel, splittable ------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("out", ["f32", "both"])
@pytest.mark.parametrize("rest,K", [(0, 128), (17, 128), (100, 128), (17, 192)], ids=["whole", "skinny_tail", "tile_tail", "tile_tail_k192"])
def test_one_tile_kernel_with_the_rest_on_the_small_kernels(lib, h16, cus256, rest, K, out, mode):
    """13 tile rows x 12 tiles on the one-tile kernel (fp32 output with residual), the rows behind them on the skinny GEMM through its strided form
    (<= 64 rows, K % 128 == 0) or on the 128- / 64-row tiles."""
    cus256()
    p = Problem(h16, 13 * 256 + rest, 3072, K, out, mode, res=True)
    _expect(p.call(lib), rows256=3328, parts=1, split_rows=0, kv_rows=0)
    p.verify()


@MODES
@pytest.mark.parametrize("N", [2820, 2824])
def test_one_tile_kernel_16_bit_only_ragged_right_edge(lib, h16, cus256, N, mode):
    """Cp == nullptr with element stores where a lane's 8 columns cross N (N = 2820) and whole chunks up to a ragged edge (N = 2824)."""
    cus256()
    p = Problem(h16, 3328, N, 128, "h16", mode, ldcb=2832)
    _expect(p.call(lib), rows256=3328, parts=1, split_rows=0, kv_rows=0)
    p.verify()


# ---- the persistent kernel and its KV epilogue ------------------------------------------------------------------------------------------------------
@MODES
def test_persistent_kernel(lib, h16, cus256, mode):
    cus256()
    p = Problem(h16, 13 * 257, 3072, 128, "h16", mode)
    _expect(p.call(lib), rows256=3328, parts=1, split_rows=0, kv_rows=0)
    p.verify()


@pytest.mark.parametrize("mode", [EXACT, ("normal", R.ACT_NONE)], ids=["exact", "normal"])          # (the KV epilogue exists without an activation only)
def test_persistent_kernel_kv_epilogue(lib, h16, cus256, mode):
    """The K | V columns of the leading kv_rows rows sit at plane[b * stride + (head * max_seq + pos) * 64 + d] and nowhere else; Cb keeps the pattern there;
    the 13 rows behind them arrive in Cb whole."""
    cus256()
    p = Problem(h16, 13 * 257, 3072, 128, "h16", mode).with_kv(T=257, col0=1024, max_seq=300)
    _expect(p.call(lib), rows256=3328, parts=1, split_rows=0, kv_rows=3328)
    p.verify(kv_rows=3328)
    p.verify_planes(3328)
    # with an activation the dispatcher must not take the KV form (and then reports no rows)
    p.fresh()
    _expect(p.call(lib, act=R.ACT_RELU), rows256=3328, kv_rows=0)
    for name in ("k", "v"):
        assert R.compare(p.kv[name], p.blank_plane()) == (0, 0)


# ---- row map and broadcast residual -----------------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("out", ["f32", "both"])
def test_row_map_and_broadcast_residual_on_the_256_tile(lib, h16, cus256, out, mode):
    """The !can_split branch: a ragged 13th tile row computed with clamped rows, the guarded epilogue through cmap and r_mod.  The physical rows the map
    skips (one per 257) keep the pattern."""
    cus256()
    p = Problem(h16, 3100, 3072, 128, out, mode, res=True, cmap=(256, 257, 1), r_mod=256)
    _expect(p.call(lib), rows256=3100, parts=1, split_rows=0, kv_rows=0)
    p.verify()


@MODES
def test_row_map_with_16_bit_output_and_residual_stays_on_the_128_row_tiles(lib, h16, mode):
    p = Problem(h16, 3100, 3072, 128, "h16", mode, res=True, cmap=(256, 257, 1), r_mod=256)
    _expect(p.call(lib), rows256=0, parts=1, split_rows=0, kv_rows=0)
    p.verify()


@MODES
@pytest.mark.parametrize("out", ["f32", "h16", "both"])
@pytest.mark.parametrize("K", [96, 192], ids=["tile64", "tile128"])
def test_row_map_and_broadcast_residual_on_the_small_tiles(lib, h16, K, out, mode):
    p = Problem(h16, 300, 200, K, out, mode, res=True, cmap=(100, 130, 7), r_mod=100)
    _expect(p.call(lib), rows256=0, parts=1, split_rows=0, kv_rows=0)
    p.verify()


@MODES
@pytest.mark.parametrize("impl", [0, 1], ids=["mfma", "valu"])
def test_row_map_and_broadcast_residual_on_the_fp32_kernels(lib, impl, mode):
    p = Problem(_H16("bf16"), 300, 96, 64, "f32", mode, res=True, cmap=(100, 130, 7), r_mod=100, prec=0, impl=impl)
    _expect(p.call(lib), rows256=0, parts=1, split_rows=0, kv_rows=0)
    p.verify()


# ---- split along K ----------------------------------------------------------------------------------------------------------------------------------
def _verify_split(p, parts, split_rows):
    """Every part window holds its k-range of the rows below split_rows (bias and residual in part 0, the rows behind complete in part 0); nothing is
    written between or behind the windows; the parts add up to the unsplit reference."""
    want = p.blank_c()
    wins = []
    total = torch.zeros_like(p.ref)
    for q, (y, lo, hi) in enumerate(R.split_parts_ref64(p.A, p.W, p.bias, p.R, parts, split_rows)):
        win = p.window(p.ldc, lo, hi, origin=GUARD * p.ldc + q * p.part_stride)
        want[win] = y.float().reshape(-1)
        wins.append(win)
        got = p.C[win].double().reshape(hi - lo, p.N)
        total[lo:hi] += got
        if p.data != "exact":
            scale = max(1e-6, float(p.ref.abs().max()))
            assert float((got - y).abs().max()) / scale < 3e-5, f"part {q}"
    bad_in, bad_out = R.compare(p.C, want, torch.cat(wins))
    assert bad_out == 0, f"{bad_out} elements between or behind the part windows no longer hold the pattern"
    if p.data == "exact":
        assert bad_in == 0, f"{bad_in} elements of the part windows differ in the bits"
        assert torch.equal(total, p.ref)
    else:
        assert float((total - p.ref).abs().max()) / max(1e-6, float(p.ref.abs().max())) < 3e-5


def _ln_of_the_parts(lib, p, h16, parts, split_rows):
    """The very buffers of the split GEMM through ma_op_ln_rows, against the fp64 LayerNorm of the unsplit reference."""
    g = torch.Generator(device=DEV).manual_seed(p.M)
    gamma, beta = 1 + 0.1 * torch.randn(p.N, generator=g, device=DEV), 0.1 * torch.randn(p.N, generator=g, device=DEV)
    ld32, lda = p.N + 12, p.N + 8
    y32, ya = R.canvas((p.M + 2 * GUARD) * ld32, torch.float32, DEV), R.canvas((p.M + 2 * GUARD) * lda, h16.tdt, DEV)
    from meshanything_amd import _lib
    _lib.check(lib.ma_op_ln_rows(p.C.data_ptr() + GUARD * p.ldc * 4, p.ldc, 0, 0, 0, gamma.data_ptr(), beta.data_ptr(), 1e-5, y32.data_ptr() + GUARD * ld32 * 4, ld32,
                                 ya.data_ptr() + GUARD * lda * 2, lda, 1, 0, 0, 0, p.M, p.N, parts, p.part_stride, split_rows, _stream()), None)
    torch.cuda.synchronize()
    ref = R.layernorm_ref64(p.ref, gamma, beta, 1e-5)
    w32, w16 = p.window(ld32), p.window(lda)
    assert R.compare(y32, R.canvas(y32.numel(), torch.float32, DEV), w32)[1] == 0 and R.compare(ya, R.canvas(ya.numel(), h16.tdt, DEV), w16)[1] == 0
    err = float((y32[w32].double() - ref.reshape(-1)).abs().max())
    assert err < 2e-5 * max(1.0, float(ref.abs().max())), err
    assert torch.equal(R.as_int(ya[w16]), R.as_int(y32[w32].to(h16.tdt)))


@pytest.mark.parametrize("mode", [EXACT, ("normal", R.ACT_NONE)], ids=["exact", "normal"])
@pytest.mark.parametrize("M,K,parts,split_rows", [(512, 1024, 4, 512), (529, 1024, 4, 512), (612, 1024, 4, 512), (512, 1152, 2, 512), (4864, 1024, 2, 4864)])
def test_split_along_k_and_its_layernorm(lib, h16, cus256, M, K, parts, split_rows, mode):
    cus256()
    p = Problem(h16, M, 1024, K, "f32", mode, res=True, max_parts=4)
    _expect(p.call(lib), rows256=split_rows, parts=parts, split_rows=split_rows, kv_rows=0)
    _verify_split(p, parts, split_rows)
    _ln_of_the_parts(lib, p, h16, parts, split_rows)


@pytest.mark.parametrize("why", ["max_parts_1", "relu"])
def test_no_split_without_leave_or_with_an_activation(lib, h16, why):
    p = Problem(h16, 512, 1024, 1024, "f32", EXACT_RELU if why == "relu" else EXACT, res=True, max_parts=4)
    got = p.call(lib, max_parts=1 if why == "max_parts_1" else 4)
    _expect(got, parts=1, split_rows=0, kv_rows=0)
    p.verify()                                                     # (whole-buffer comparison: the windows of parts 1 .. 3 keep the pattern)


# ---- a GEMM by row parts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["persistent", "persistent_kv", "one_tile_f32_res", "small_tiles", "split"])
def test_parts_1_and_2_write_their_rows_only_and_together_equal_part_0(lib, h16, cus256, case):
    """Seeded-normal data, so that a different kernel choice for a stretch of rows would show up in the bits."""
    cus256()
    mode = ("normal", R.ACT_NONE)
    p = {"persistent": lambda: Problem(h16, 3341, 3072, 128, "h16", mode),
         "persistent_kv": lambda: Problem(h16, 3341, 3072, 128, "h16", mode).with_kv(T=257, col0=1024, max_seq=300),
         "one_tile_f32_res": lambda: Problem(h16, 3345, 3072, 128, "f32", mode, res=True),
         "small_tiles": lambda: Problem(h16, 600, 512, 128, "both", mode, res=True),
         "split": lambda: Problem(h16, 529, 1024, 1024, "f32", mode, res=True, max_parts=4)}[case]()
    want = {"persistent": dict(rows256=3328, parts=1, kv_rows=0), "persistent_kv": dict(rows256=3328, parts=1, kv_rows=3328),
            "one_tile_f32_res": dict(rows256=3328, parts=1, kv_rows=0), "small_tiles": dict(rows256=0, parts=1, kv_rows=0),
            "split": dict(rows256=512, parts=4, split_rows=512, kv_rows=0)}[case]
    Mm = p.M - p.M % 256
    res = {}
    for part in (0, 1, 2):
        p.fresh()
        _expect(p.call(lib, part=part), **want)                    # the kernels are chosen as for the whole problem, whichever part is computed
        res[part] = dict(C=p.C, Cb=p.Cb, k=p.kv["k"] if p.kv else None, v=p.kv["v"] if p.kv else None)
    nparts = want["parts"]
    for name, ld, blank in (("C", p.ldc, p.blank_c), ("Cb", p.ldcb, p.blank_cb)):
        if res[0][name] is None:
            continue
        wins = {1: [], 2: []}
        for q in range(nparts if name == "C" else 1):
            o = GUARD * ld + q * p.part_stride
            wins[1].append(p.window(ld, 0, Mm, origin=o)); wins[2].append(p.window(ld, Mm, p.M, origin=o))
        for part in (1, 2):
            assert R.compare(res[part][name], blank(), torch.cat(wins[part]))[1] == 0, f"part {part} wrote {name} outside its rows"
        x1, x2 = R.as_int(res[1][name]), R.as_int(res[2][name])
        pat = R.PAT32 if name == "C" else R.PAT16
        assert torch.equal(torch.where(x1 != pat, x1, x2), R.as_int(res[0][name])), f"{name}: parts 1 and 2 together differ from part 0 in the bits"
    if p.kv:
        for name in ("k", "v"):
            assert R.compare(res[2][name], p.blank_plane()) == (0, 0), "part 2 wrote to the KV planes"
            assert R.compare(res[1][name], res[0][name]) == (0, 0)
    # ... and part 0 itself is right
    p.C, p.Cb = res[0]["C"], res[0]["Cb"]
    if case == "split":
        _verify_split(p, 4, 512)
    else:
        p.verify(kv_rows=want["kv_rows"])
    if p.kv:
        p.kv["k"], p.kv["v"] = res[0]["k"], res[0]["v"]
        p.verify_planes(want["kv_rows"])


def test_parts_take_no_row_map_and_no_broadcast_residual(lib, h16):
    p = Problem(h16, 300, 200, 96, "f32", EXACT, res=True, cmap=(100, 130, 7), r_mod=100)
    q = Problem(h16, 300, 200, 96, "f32", EXACT, res=True, r_mod=100)
    from meshanything_amd import _lib
    for prob in (p, q):
        for part in (1, 2):
            with pytest.raises(_lib.MAError) as e:
                prob.call(lib, part=part)
            assert e.value.code == INVALID
            assert R.compare(prob.C, prob.blank_c()) == (0, 0)


# ---- ma_op_ln_rows ----------------------------------------------------------------------------------------------------------------------------------
ROWS = 11                                                          # four rows per block: the last block is ragged


def _ln_case(lib, h16, D, form, parts=1, split_rows=0):
    from meshanything_amd import _lib
    g = torch.Generator(device=DEV).manual_seed(D + 7 * parts + split_rows)
    xin, yout = (4, 6, 1), ((4, 6, 1) if form == "inplace" else (3, 5, 2))
    ldx = D + 4
    ld32, lda = (ldx if form == "inplace" else D + 8), D + 12
    rin, rout = R.row_map(torch.arange(ROWS, device=DEV), *xin), R.row_map(torch.arange(ROWS, device=DEV), *yout)
    nin, nout = int(rin.max()) + 1 + 2 * GUARD, int(rout.max()) + 1 + 2 * GUARD
    part_stride = nin * ldx + 36
    xparts = torch.randn(parts, ROWS, D, generator=g, device=DEV) * 3 + 1
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g, device=DEV), 0.1 * torch.randn(D, generator=g, device=DEV)
    xsum = xparts[0].double().clone()
    xsum[:split_rows] += xparts[1:, :split_rows].double().sum(dim=0)
    ref = R.layernorm_ref64(xsum, gamma, beta, 1e-5)
    xbuf = R.canvas(nin * ldx + (parts - 1) * part_stride, torch.float32, DEV)
    cols = torch.arange(D, device=DEV)[None, :]
    xwin = (GUARD * ldx + rin[:, None] * ldx + cols).reshape(-1)
    for q in range(parts):
        v = xparts[q].clone()
        if q > 0:
            v[split_rows:] = 1e30                                  # rows at and behind split_rows must ignore parts 1 and above
        xbuf[xwin + q * part_stride] = v.reshape(-1)
    x_before = xbuf.clone()
    y32 = xbuf if form == "inplace" else (R.canvas(nout * ld32, torch.float32, DEV) if form != "act32" else None)
    a_dt = torch.float32 if form == "act32" else h16.tdt
    ya = R.canvas(nout * lda, a_dt, DEV)
    ptr = lambda t, ld: None if t is None else t.data_ptr() + GUARD * ld * t.element_size()
    _lib.check(lib.ma_op_ln_rows(ptr(xbuf, ldx), ldx, *xin, gamma.data_ptr(), beta.data_ptr(), 1e-5, ptr(y32, ld32), ld32, ptr(ya, lda), lda, 0 if form == "act32" else 1,
                                 *yout, ROWS, D, parts, part_stride, split_rows, _stream()), None)
    torch.cuda.synchronize()
    tol = 2e-5 * max(1.0, float(ref.abs().max()))
    ywin = lambda ld: (GUARD * ld + rout[:, None] * ld + cols).reshape(-1)
    if y32 is not None:
        # outside the window: the pattern, or -- in place -- whatever the input buffer held there (its other parts included)
        before = x_before if form == "inplace" else R.canvas(y32.numel(), torch.float32, DEV)
        assert R.compare(y32, before, ywin(ld32))[1] == 0
        assert float((y32[ywin(ld32)].double() - ref.reshape(-1)).abs().max()) < tol
    assert R.compare(ya, R.canvas(ya.numel(), a_dt, DEV), ywin(lda))[1] == 0
    if form == "act32":
        assert float((ya[ywin(lda)].double() - ref.reshape(-1)).abs().max()) < tol
    else:
        assert torch.equal(R.as_int(ya[ywin(lda)]), R.as_int(y32[ywin(ld32)].to(h16.tdt))), "the 16-bit output is not the rounded fp32 output"
    if form != "inplace":
        assert R.compare(xbuf, x_before) == (0, 0)


@pytest.mark.parametrize("form", ["maps", "act32", "inplace"])
@pytest.mark.parametrize("D", [36, 128, 256, 512, 768, 1024, 1028, 4096])
def test_ln_rows(lib, h16, D, form):
    _ln_case(lib, h16, D, form)


@pytest.mark.parametrize("form", ["maps", "inplace"])
@pytest.mark.parametrize("split_rows", [0, 1, 6, 10, 11])
@pytest.mark.parametrize("parts", [2, 4])
def test_ln_rows_of_a_split_input(lib, h16, parts, split_rows, form):
    _ln_case(lib, h16, 1024, form, parts, split_rows)


REFUSED = [dict(D=1026), dict(D=4100), dict(D=0), dict(D=-4), dict(rows=0), dict(rows=-2), dict(parts=3), dict(parts=0), dict(parts=8),
           dict(parts=2, D=768), dict(parts=4, D=512), dict(split_rows=-1), dict(split_rows=9), dict(parts=2, split_rows=9)]


def test_layernorm_entry_points_refuse_what_the_kernel_cannot_compute(lib):
    """Before this check ma_op_layernorm returned 0 with wrong values for D % 4 != 0 or D > 4096 (a lane holds at most 16 float4 chunks of a row)."""
    x = torch.randn(4 * 8 * 4104, device=DEV)
    gamma = torch.ones(4104, device=DEV)
    y = R.canvas(8 * 4104, torch.float32, DEV)
    for kw in REFUSED:
        a = dict(rows=8, D=1024, parts=1, split_rows=0)
        a.update(kw)
        ld = max(4, _up(a["D"], 4))
        rc = lib.ma_op_ln_rows(x.data_ptr(), ld, 0, 0, 0, gamma.data_ptr(), gamma.data_ptr(), 1e-5, y.data_ptr(), ld, None, 0, 1, 0, 0, 0,
                               a["rows"], a["D"], a["parts"], 8 * 4104, a["split_rows"], _stream())
        assert rc == INVALID, kw
        if a["parts"] == 1 and a["split_rows"] == 0:
            assert lib.ma_op_layernorm(x.data_ptr(), ld, gamma.data_ptr(), gamma.data_ptr(), 1e-5, y.data_ptr(), ld, a["rows"], a["D"], _stream()) == INVALID, kw
        torch.cuda.synchronize()
        assert R.compare(y, R.canvas(y.numel(), torch.float32, DEV)) == (0, 0), kw
