"""Dense attention as the dense phases launch it (MI355X), through the test aid ma_op_attention_dense: a batch of samples along grid.z with sample strides,
the engine's operand layouts (per-head [q|k|v], q|k|v blocks, cross-attention with ONE query for all samples, K / V in KV-cache planes), a shortened last
sample (last_len), the caller's V^T workspace, and the prefill's main chain + tail chain against the one-stream launch.  Every sample of a launch is a
closed-form pattern of its own (tests/attn_cases.py: stack(), layout_batch(), last_len_batch(), tail_batch()): every element of every sample against the
float64 softmax within attn_cases.bound() -- no tolerance of this file's own --, outputs pre-filled with a NaN bit pattern, what a launch must not write
compared bit for bit, what it must not read non-finite, two launches bit for bit, a batch bit for bit against its samples launched one by one.
tests/test_attn_cases_host.py proves on the host that each of these launches tells a wrong sample, a shifted row and a key behind last_len from the truth."""
import ctypes as C
import functools

import pytest
import torch

import attn_cases as A

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CODE = {"f32": 0, "bf16": 1, "fp16": 2}
H = A.BATCH_H
W = H * 64
GUARD_ROWS = 3                          # rows of every sample's output behind its Sq rows: never written
VT_GUARD = 4096                         # 16-bit elements behind the V^T workspace: never written
KERNELS = [(0, "f32"), (3, "bf16"), (4, "bf16"), (4, "fp16")]
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from meshanything_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    lib = _lib.load()
    yield lib
    lib.ma_op_set_half_dtype(1)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _sentinel(shape, tdt, pattern=None):
    """A buffer of one NaN bit pattern (0x7fc1.... is a NaN in fp32, bf16 and fp16)."""
    if tdt == torch.float32:
        return torch.full(shape, 0x7FC10001 if pattern is None else pattern, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full(shape, 0x7FC1 if pattern is None else pattern, dtype=torch.int16, device="cuda").view(tdt)


def _nan(shape, tdt):
    return torch.full(shape, float("nan"), dtype=tdt, device="cuda")


class Operand:
    """A tensor that holds an operand, the element offset of (sample 0, row 0, head 0) in it, and the row / head / sample strides in elements."""
    def __init__(self, t, off, rs, hs, bs):
        self.t, self.off, self.rs, self.hs, self.bs = t, off, rs, hs, bs

    def ptr(self, b=0, row=0):
        return self.t.data_ptr() + (self.off + b * self.bs + row * self.rs) * self.t.element_size()

    def check(self, rows, B):
        """The last element a launch of B samples x `rows` rows may touch lies inside the tensor."""
        assert self.off + (B - 1) * self.bs + (rows - 1) * self.rs + (H - 1) * self.hs + 64 <= self.t.numel(), "operand outside its buffer"


def _launch(lib, kernel, q, k, v, o, Sq, Sk, causal, batch, last_len=-1, vt=None, b0=None, q_row0=0, expect=0, vt_elems=None):
    """One ma_op_attention_dense call.  b0: launch sample b0 alone (batch 1, its own addresses); the extent of every operand is checked here first."""
    from meshanything_amd import _lib
    nb = 1 if b0 is not None else batch
    sb = b0 or 0
    for x, rows in ((q, q_row0 + Sq), (k, Sk), (v, Sk), (o, Sq)):
        x.check(rows, sb + nb)
    a = _lib.AttnDenseArgs(kernel=kernel, Sq=Sq, Sk=Sk, H=H, causal_offset=causal, batch=nb, last_len=last_len, scale=0.125,
                           q_rs=q.rs, q_hs=q.hs, k_rs=k.rs, k_hs=k.hs, v_rs=v.rs, v_hs=v.hs, o_rs=o.rs, q_bs=q.bs, k_bs=k.bs, v_bs=v.bs, o_bs=o.bs,
                           Q=q.ptr(sb, q_row0), K=k.ptr(sb), V=v.ptr(sb), O=o.ptr(sb))
    if vt is not None:
        need = lib.ma_attention_vt_workspace_elems(Sk, H, nb)
        assert need == nb * H * 64 * ((Sk + 63) // 64 * 64) and vt.numel() >= need + VT_GUARD
        a.vt, a.vt_elems = vt.data_ptr(), need if vt_elems is None else vt_elems
    rc = lib.ma_op_attention_dense(C.byref(a), _stream())
    torch.cuda.synchronize()
    if expect == 0:
        _lib.check(rc, None)
    else:
        assert rc == expect, (rc, lib.ma_last_error(None))
        assert b"ma_op_attention_dense" in lib.ma_last_error(None)
    return rc


def _workspace(lib, kernel, Sk, batch, tdt):
    """Kernel 4's V^T workspace: exactly ma_attention_vt_workspace_elems elements of NaN (the stale columns of an earlier, longer launch) + a guard."""
    if kernel != 4:
        return None
    need = lib.ma_attention_vt_workspace_elems(Sk, H, batch)
    vt = _sentinel((need + VT_GUARD,), tdt, 0x5A5A)
    vt[:need] = float("nan")
    return vt


def _guard_ok(vt, Sk, batch):
    need = batch * H * 64 * ((Sk + 63) // 64 * 64)
    return vt is None or bool((_bits(vt[need:]) == 0x5A5A).all())


def _output(B, Sq, tdt):
    t = _sentinel((B, Sq + GUARD_ROWS, W), tdt)
    return Operand(t, 0, W, 64, (Sq + GUARD_ROWS) * W)


def _layout(layout, bt, tdt, poison=True):
    """The launch's q, k, v (attn_cases.Batch) in one of the engine's layouts -> (q, k, v) Operands.  What the launch has no business reading is NaN."""
    B, Sq, Sk = bt.B, bt.Sq, bt.Sk
    q, k, v = bt.q.to(tdt), bt.k.to(tdt), bt.v.to(tdt)
    if layout == "interleaved":         # MiCHe self-attention: per head [q|k|v], one stride for all three; the rows a side does not have hold NaN
        n = max(Sq, Sk)
        buf = _nan((B, n, H, 192), tdt)
        buf[:, :Sq, :, :64] = q; buf[:, :Sk, :, 64:128] = k; buf[:, :Sk, :, 128:] = v
        return tuple(Operand(buf, off, H * 192, 192, n * H * 192) for off in (0, 64, 128))
    if layout == "blocks":              # BERT / the fp32 prefill: q | k | v by thirds of the row of one stacked buffer
        n = max(Sq, Sk)
        buf = _nan((B, n, 3, H, 64), tdt)
        buf[:, :Sq, 0] = q; buf[:, :Sk, 1] = k; buf[:, :Sk, 2] = v
        return tuple(Operand(buf, off, 3 * W, 64, n * 3 * W) for off in (0, W, 2 * W))
    if layout == "cross":               # encoder cross-attention: ONE query (sample stride 0), per head [k|v] per sample
        assert all(torch.equal(bt.q[b], bt.q[0]) for b in range(B))
        qb = q[0].reshape(Sq, W).contiguous()
        kv = torch.cat([k, v], dim=-1).contiguous()                  # (B, Sk, H, 128)
        return Operand(qb, 0, W, 64, 0), Operand(kv, 0, H * 128, 128, Sk * H * 128), Operand(kv, 64, H * 128, 128, Sk * H * 128)
    assert layout == "planes" and Sq == Sk
    # the 16-bit prefill: q from the stacked q|k|v tensor (its k and v columns are not read: NaN), K and V from cache planes [B][layer][H][max_seq][64] -- the
    # second of two layers, so that a sample stride of one layer's size lands in NaN -- with max_seq > T and NaN behind position T
    T, max_seq = Sk, Sk + 43
    qkv = _nan((B, T, 3, H, 64), tdt)
    qkv[:, :, 0] = q
    planes = []
    for x in (k, v):
        p = _nan((B, 2, H, max_seq, 64), tdt)
        p[:, 1, :, :T] = x.permute(0, 2, 1, 3)
        planes.append(Operand(p, H * max_seq * 64, 64, max_seq * 64, 2 * H * max_seq * 64))
    return Operand(qkv, 0, 3 * W, 64, T * 3 * W), planes[0], planes[1]


@functools.lru_cache(maxsize=None)
def _judged(kind, key, fmt):
    """A launch's Batch on the device with the float64 reference and bound of every sample: built once, shared, never modified."""
    make = {"layout": A.layout_batch, "last_len": A.last_len_batch, "tail": A.tail_batch}[kind]
    bt = make(*key, fmt, device="cuda")
    out = []
    for case in bt.cases:
        ref, info = A.reference(case), A.analyse(case)
        out.append((ref, A.bound(case, ref, info, fmt)))
    return bt, out


def _judge(bt, judged, O, worst, what=""):
    """Every element of every sample of the output tensor O.t (B, rows + guard, W) against its reference; the guard rows and, behind a short last sample, the rows
    it does not have must still hold the sentinel."""
    fresh = _bits(_sentinel((1,), O.t.dtype))[0]
    for b, (ref, bnd) in enumerate(judged):
        nq = bt.rows(b)[0]
        worst.append((A.worst_ratio(O.t[b, :nq].float().reshape(nq, H, 64), ref, bnd), f"{what}sample {b} {bt.cases[b].name}"))
        assert bool((_bits(O.t[b, nq:]) == fresh).all()), f"{what}sample {b}: a row behind its {nq} rows was written"


def _report(name, worst):
    worst.sort(reverse=True)
    print(f"{name}: worst |err| / bound = {worst[0][0]:.3f} at {worst[0][1]}; over the bound: {[(w, f'{r:.3g}') for r, w in worst if not r <= 1.0]}")
    assert worst[0][0] <= 1.0, [(w, r) for r, w in worst if not r <= 1.0]


def _set_format(lib, kernel, fmt):
    assert lib.ma_op_set_half_dtype(CODE[fmt] if kernel != 0 else 1) == 0


# ---- a. the engine's layouts at batch > 1 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,fmt", KERNELS)
@pytest.mark.parametrize("layout,Sq,Sk,causal", A.LAYOUT_LAUNCHES)
def test_batched_layouts(lib, layout, Sq, Sk, causal, kernel, fmt):
    """Every pattern a sample of ONE launch (11 - 19 samples), in each layout the dense phases use: within the bound, two launches and the samples one by one
    bit for bit (a block is independent of every other (sample, head, row block))."""
    _set_format(lib, kernel, fmt)
    tdt = TDT[fmt]
    bt, judged = _judged("layout", (layout, Sq, Sk, causal), fmt)
    q, k, v = _layout(layout, bt, tdt)
    outs, worst = [], []
    for it in range(2):
        O, vt = _output(bt.B, Sq, tdt), _workspace(lib, kernel, Sk, bt.B, tdt)
        _launch(lib, kernel, q, k, v, O, Sq, Sk, causal, bt.B, vt=vt)
        assert _guard_ok(vt, Sk, bt.B), "written behind the V^T workspace"
        outs.append(O)
    assert torch.equal(_bits(outs[0].t), _bits(outs[1].t)), "two launches differ"
    _judge(bt, judged, outs[0], worst)
    single = _output(bt.B, Sq, tdt)
    for b in range(bt.B):
        vt = _workspace(lib, kernel, Sk, 1, tdt)
        _launch(lib, kernel, q, k, v, single, Sq, Sk, causal, bt.B, vt=vt, b0=b)
        assert _guard_ok(vt, Sk, 1)
    assert torch.equal(_bits(single.t), _bits(outs[0].t)), "the batch differs from its samples launched one by one"
    _report(f"batched {layout} {(Sq, Sk, causal)} kernel {kernel} {fmt} B {bt.B}", worst)


# ---- b. a shortened last sample -------------------------------------------------------------------------------------------------------------------------
def _poison_behind(q, k, v, b, L, T):
    """Behind row L of sample b: Q rows NaN; K row L stays (the adversarial dominant key), V row L is +inf, every later K / V row NaN, +inf, NaN, -inf, ..."""
    def rows(x, r0, all_nan=False):
        view = x.t.view(-1)
        for h in range(H):
            for j in range(r0, T):
                o = x.off + b * x.bs + j * x.rs + h * x.hs
                d = j - L
                view[o:o + 64] = float("nan") if d % 2 or all_nan else (float("inf") if d % 4 == 0 else float("-inf"))
    rows(q, L, all_nan=True)
    rows(k, L + 1)
    rows(v, L)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("causal", [0, -1])
@pytest.mark.parametrize("T,L", A.LAST_LEN_LAUNCHES)
def test_short_last_sample(lib, T, L, causal, fmt):
    """last_len = L on a batch of 3 in the prefill's plane layout: nothing behind row L of the last sample is read (Q NaN, K / V NaN and +-inf, the key at L
    dominant) or written (sentinel rows), the V^T workspace has exactly its size and starts as NaN; the last sample's rows equal a batch-1 launch with
    Sq = Sk = L bit for bit, whichever of the 96- / 128-row kernels either launch takes (a fully masked round leaves a row as it was: alpha == 1 exactly)."""
    _set_format(lib, 4, fmt)
    tdt = TDT[fmt]
    bt, judged = _judged("last_len", (T, L, causal), fmt)
    assert bt.B == 3 and bt.last_len == L
    q, k, v = _layout("planes", bt, tdt)
    _poison_behind(q, k, v, bt.B - 1, L, T)
    outs, worst = [], []
    for it in range(2):
        O, vt = _output(bt.B, T, tdt), _workspace(lib, 4, T, bt.B, tdt)
        _launch(lib, 4, q, k, v, O, T, T, causal, bt.B, last_len=L, vt=vt)
        assert _guard_ok(vt, T, bt.B), "written behind the V^T workspace"
        outs.append(O)
    assert torch.equal(_bits(outs[0].t), _bits(outs[1].t)), "two launches differ"
    _judge(bt, judged, outs[0], worst)
    single = _output(bt.B, T, tdt)
    for b in range(bt.B):
        n = bt.rows(b)[0]
        vt = _workspace(lib, 4, n, 1, tdt)
        _launch(lib, 4, q, k, v, single, n, n, causal, bt.B, vt=vt, b0=b)
        assert _guard_ok(vt, n, 1)
    assert torch.equal(_bits(single.t), _bits(outs[0].t)), "the batch differs from its samples launched one by one (the last one with Sq = Sk = last_len)"
    _report(f"last_len {(T, L, causal)} {fmt}", worst)


# ---- c. the prefill's main chain + tail chain = the one-stream launch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("T,nt", A.TAIL_LAUNCHES)
def test_main_chain_plus_tail_chain_is_the_one_stream_launch(lib, T, nt, fmt):
    """Launch 1: the batch with last_len = T - nt while positions T - nt .. T - 1 of the last sample's planes and q rows hold NaN.  Launch 2, after they are
    filled in: batch 1, Sq = nt, Sk = T, causal_offset = T - nt, q from stacked row B T - nt, the last sample's planes, its own output and workspace.
    Together: the bits of the launch with last_len = -1, and every row within the bound."""
    _set_format(lib, 4, fmt)
    tdt = TDT[fmt]
    bt, judged = _judged("tail", (T, nt), fmt)
    B, cut = bt.B, T - nt
    assert B == 3 and bt.last_len < 0
    q, k, v = _layout("planes", bt, tdt)
    one, vt = _output(B, T, tdt), _workspace(lib, 4, T, B, tdt)
    _launch(lib, 4, q, k, v, one, T, T, 0, B, vt=vt)
    assert _guard_ok(vt, T, B)
    worst = []
    _judge(bt, judged, one, worst, "one stream: ")
    # launch 1 on buffers whose tail rows are not there yet
    q1, k1, v1 = (Operand(x.t.clone(), x.off, x.rs, x.hs, x.bs) for x in (q, k, v))
    for x in (q1, k1, v1):
        flat = x.t.view(-1)
        for h in range(H):
            for j in range(cut, T):
                o = x.off + (B - 1) * x.bs + j * x.rs + h * x.hs
                flat[o:o + 64] = float("nan")
    main, vt = _output(B, T, tdt), _workspace(lib, 4, T, B, tdt)
    _launch(lib, 4, q1, k1, v1, main, T, T, 0, B, last_len=cut, vt=vt)
    assert _guard_ok(vt, T, B)
    fresh = _bits(_sentinel((1,), tdt))[0]
    assert bool((_bits(main.t[B - 1, cut:]) == fresh).all()), "the main chain wrote a row of the tail chain"
    # launch 2: the tail form, on the complete buffers
    tail_t = _sentinel((nt + GUARD_ROWS, W), tdt)
    tail, vt2 = Operand(tail_t, 0, W, 64, 0), _workspace(lib, 4, T, 1, tdt)
    qt = Operand(q.t, q.off, q.rs, q.hs, 0)                          # (one sample: rows B T - nt .. B T - 1 of the stacked tensor)
    assert q.bs == T * q.rs
    kt, vtail = (Operand(x.t, x.off + (B - 1) * x.bs, x.rs, x.hs, 0) for x in (k, v))
    _launch(lib, 4, qt, kt, vtail, tail, nt, T, cut, 1, vt=vt2, q_row0=B * T - nt)
    assert _guard_ok(vt2, T, 1)
    assert bool((_bits(tail_t[nt:]) == fresh).all())
    both = main.t.clone()
    both[B - 1, cut:T] = tail_t[:nt]
    assert torch.equal(_bits(both), _bits(one.t)), "main chain + tail chain differ from the one-stream launch"
    _judge(bt, judged, Operand(both, 0, W, 64, main.bs), worst, "two chains: ")
    _report(f"main + tail {(T, nt)} {fmt}", worst)


# ---- d. what the launchers refuse comes back as an error, and nothing was launched ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_refusals_launch_nothing(lib, fmt):
    Sq, Sk, B = 96, 65, 3
    bt, _ = _judged("layout", ("blocks", Sq, Sk, -1), fmt)
    bt = A.stack("three", bt.cases[:B])

    def refused(kernel, kfmt, layout="blocks", tweak=None, **kw):
        _set_format(lib, kernel, kfmt)
        tdt = TDT["f32" if kernel == 0 else kfmt]
        q, k, v = _layout(layout, bt, tdt)
        O, vt = _output(B, Sq, tdt), _workspace(lib, kernel, Sk, B, tdt)
        if tweak:
            tweak(q, k, v, O)
        before = (O.t.clone(), None if vt is None else vt.clone())
        _launch(lib, kernel, q, k, v, O, Sq, Sk, -1, B, vt=vt, expect=INVALID, **kw)
        assert torch.equal(_bits(before[0]), _bits(O.t)) and (vt is None or torch.equal(_bits(before[1]), _bits(vt))), (kernel, kfmt, kw)

    for last_len in (0, 1, Sk, Sq):                                   # the first-generation kernels know no last_len
        refused(0, fmt, last_len=last_len)
        refused(3, "bf16", last_len=last_len)
    for last_len in (0, Sq + 1, Sk + 1, Sq):                           # (Sk + 1 <= Sq: more rows than the sample has keys)
        refused(4, fmt, last_len=last_len)
    for name in ("q.rs", "k.rs", "v.rs", "o.rs", "q.hs", "k.hs", "v.hs", "q.bs", "k.bs", "v.bs", "o.bs"):      # 16-byte accesses: every stride a multiple of 8 elements
        def tweak(q, k, v, o, name=name):
            x = {"q": q, "k": k, "v": v, "o": o}[name[0]]
            setattr(x, name[2:], getattr(x, name[2:]) - 4)             # (smaller: still inside the buffer)
        refused(4, fmt, tweak=tweak)
    refused(4, fmt, vt_elems=lib.ma_attention_vt_workspace_elems(Sk, H, B) - 1)
    if fmt == "fp16":
        refused(3, "fp16")
