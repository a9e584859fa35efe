"""The attention kernels on scores that are not benign (MI355X): tests/attn_cases.py -- a running maximum that moves in every tile, rescales
by e^-40, partials that underflow before the merge, scores at +-96, rows of one wave whose maxima move in different tiles, a dominant key
exactly on a mask / tile / round / chunk / hand-over edge -- where the output is known in closed form (the mean of V over a row's top visible
keys) to about one ulp of the output.  Every element of every case against the float64 softmax of the same rounded inputs within the bound
DERIVED in attn_cases.py (fp32 accumulation + the output's rounding + e^-30 leakage + fp32 score arithmetic; nothing read off a kernel),
outputs pre-filled with NaN, cache rows beyond the length NaN, two launches bit for bit.  test_attn_cases_host.py checks the cases, the
bound and the checker on the host."""
import ctypes as C

import pytest
import torch

import attn_cases as A

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CODE = {"f32": 0, "bf16": 1, "fp16": 2}


@pytest.fixture(scope="module")
def lib():
    from meshanything_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    lib = _lib.load()
    yield lib
    lib.ma_op_set_half_dtype(1)


def _chk(rc):
    from meshanything_amd import _lib
    _lib.check(rc, None)


def _p(t, byte_off=0):
    return C.c_void_p(t.data_ptr() + byte_off)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _judge(what, case, out, out_fmt, worst):
    ref, info = A.reference(case), A.analyse(case)
    r = A.worst_ratio(out.float(), ref, A.bound(case, ref, info, out_fmt))
    worst.append((r, what))
    return r


def _report(name, worst):
    worst.sort(reverse=True)
    print(f"{name}: worst |err| / bound = {worst[0][0]:.3f} at {worst[0][1]}; cases over the bound: {[(w, f'{r:.3g}') for r, w in worst if not r <= 1.0]}")
    assert worst[0][0] <= 1.0, [(w, r) for r, w in worst if not r <= 1.0]


# mode 0: the fp32 kernel; 1: the first MFMA kernel on fp32 tensors (q, k, v, P rounded to bf16 inside); 2: the fp32 kernel on bf16-valued inputs;
# 4: the engine's 16-bit kernel (attn2.hpp: V^T packing + swapped operands), 16-bit tensors in, 16-bit out, in both formats
@pytest.mark.parametrize("mode,fmt", [(0, "f32"), (1, "bf16"), (2, "bf16"), (4, "bf16"), (4, "fp16")])
@pytest.mark.parametrize("Sq,Sk,H,layout,causal", [(257, 257, 2, "std", 0), (130, 300, 2, "cross", -1), (70, 130, 2, "std", 60), (96, 65, 3, "interleaved", -1)])
def test_attention_on_closed_form_scores(lib, mode, fmt, Sq, Sk, H, layout, causal):
    tdt = TDT[fmt] if mode == 4 else torch.float32
    out_fmt = fmt if mode == 4 else "f32"
    es = 2 if mode == 4 else 4
    if mode == 4:
        assert lib.ma_op_set_half_dtype(CODE[fmt]) == 0
    worst = []
    for case in A.dense_cases(Sq, Sk, H, causal, fmt, device="cuda"):
        q, k, v = case.q.to(tdt), case.k.to(tdt), case.v.to(tdt)
        if layout == "std":
            keep = (q.reshape(Sq, H * 64).contiguous(), k.reshape(Sk, H * 64).contiguous(), v.reshape(Sk, H * 64).contiguous())
            ptrs = (_p(keep[0]), H * 64, 64, _p(keep[1]), H * 64, 64, _p(keep[2]), H * 64, 64)
        elif layout == "interleaved":          # per head [q|k|v], Sq and Sk rows in one buffer; the rows a side does not have hold NaN
            n = max(Sq, Sk)
            buf = torch.full((n, H, 192), float("nan"), dtype=tdt, device="cuda")
            buf[:Sq, :, :64] = q; buf[:Sk, :, 64:128] = k; buf[:Sk, :, 128:] = v
            keep = (buf,)
            ptrs = (_p(buf), H * 192, 192, _p(buf, 64 * es), H * 192, 192, _p(buf, 128 * es), H * 192, 192)
        else:                                  # cross: q (Sq, H*64); kv per head [k|v]
            keep = (q.reshape(Sq, H * 64).contiguous(), torch.cat([k, v], dim=-1).reshape(Sk, H * 128).contiguous())
            ptrs = (_p(keep[0]), H * 64, 64, _p(keep[1]), H * 128, 128, _p(keep[1], 64 * es), H * 128, 128)
        outs = []
        for it in range(2):
            O = torch.full((Sq, H * 64), float("nan"), dtype=tdt, device="cuda")
            _chk(lib.ma_op_attention(*ptrs, _p(O), H * 64, Sq, Sk, H, 0.125, causal, mode, _stream()))
            torch.cuda.synchronize()
            outs.append(O)
        del keep
        assert torch.equal(outs[0].view(torch.int16 if es == 2 else torch.int32), outs[1].view(torch.int16 if es == 2 else torch.int32)), f"{case.name}: two launches differ"
        _judge(case.name, case, outs[0].reshape(Sq, H, 64), out_fmt, worst)
    _report(f"attention mode {mode} {fmt} {(Sq, Sk, H, layout, causal)}", worst)


@pytest.mark.parametrize("fmt", ["f32", "bf16", "fp16"])
@pytest.mark.parametrize("length", [1, 17, 129, 1000, 2500])
def test_decode_attention_on_closed_form_scores(lib, fmt, length):
    """Split-KV decode attention (16 equal chunks per head + the merge of the partials), H = 2: two patterns per launch."""
    H, max_seq = 2, length + 3
    slots = A.decode_slots(length)
    n = len(slots) + len(slots) % 2
    case, names = A.decode_case(slots, n, H, fmt, seed=length, device="cuda")
    ws = torch.empty(lib.ma_decode_attention_workspace_bytes(H) // 4, device="cuda")
    got = torch.empty(1, n, 64, device="cuda")
    for g in range(0, n, 2):
        kd = torch.full((H, max_seq, 64), float("nan"), dtype=TDT[fmt], device="cuda")
        vd = torch.full((H, max_seq, 64), float("nan"), dtype=TDT[fmt], device="cuda")
        kd[:, :length] = case.k[:, g:g + 2].permute(1, 0, 2).to(TDT[fmt]); vd[:, :length] = case.v[:, g:g + 2].permute(1, 0, 2).to(TDT[fmt])
        qd = case.q[0, g:g + 2].reshape(H * 64).contiguous()
        outs = []
        for it in range(2):
            out = torch.full((H * 64,), float("nan"), device="cuda")
            _chk(lib.ma_op_decode_attention(CODE[fmt], _p(qd), _p(kd), _p(vd), H, max_seq, length, _p(out), _p(ws), _stream()))
            torch.cuda.synchronize()
            outs.append(out)
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"{names[g:g + 2]}: two launches differ"
        got[0, g:g + 2] = outs[0].reshape(2, 64)
    ref, info = A.reference(case), A.analyse(case)
    ratio = ((got.double() - ref).abs() / A.bound(case, ref, info, "f32")).amax(dim=-1)[0]
    ratio = torch.where(torch.isfinite(got).all(dim=-1)[0], ratio, torch.full_like(ratio, float("inf")))
    _report(f"decode attention {fmt} len {length}", [(float(r), names[i]) for i, r in enumerate(ratio)])


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("waves", [4, 8, 16, 82])        # 82: 8 waves, two blocks per (row, head) with the in-launch hand-over
@pytest.mark.parametrize("B,length", [(8, 700), (16, 257), (17, 130)])
def test_decode_attention_rows_on_closed_form_scores(lib, fmt, B, length, waves):
    """Final-form batched decode attention: every (row, head) of ONE launch is a pattern of its own (H = 4: 32 - 68 slots for ~ 30 patterns)."""
    H, max_seq = 4, length + 3
    assert lib.ma_op_set_half_dtype(CODE[fmt]) == 0
    slots = A.decode_slots(length)
    case, names = A.decode_case(slots, B * H, H, fmt, seed=B + length, device="cuda")
    assert B * H >= len(slots)
    kd = torch.full((B, H, max_seq, 64), float("nan"), dtype=TDT[fmt], device="cuda")
    vd = torch.full((B, H, max_seq, 64), float("nan"), dtype=TDT[fmt], device="cuda")
    kd[:, :, :length] = case.k.permute(1, 0, 2).reshape(B, H, length, 64).to(TDT[fmt])
    vd[:, :, :length] = case.v.permute(1, 0, 2).reshape(B, H, length, 64).to(TDT[fmt])
    qd = case.q[0].reshape(B, H * 64).contiguous()
    outs = []
    for it in range(2):
        out = torch.full((B, H * 64), float("nan"), device="cuda", dtype=TDT[fmt])
        _chk(lib.ma_op_decode_attention_rows(_p(qd), _p(kd), _p(vd), H, max_seq, length, B, H * max_seq * 64, 8 if waves == 82 else waves, 2 if waves == 82 else 1, _p(out), _stream()))
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "two launches differ"
    got = outs[0].reshape(1, B * H, 64)
    ref, info = A.reference(case), A.analyse(case)
    ratio = ((got.double() - ref).abs() / A.bound(case, ref, info, fmt)).amax(dim=-1)[0]
    ratio = torch.where(torch.isfinite(got.float()).all(dim=-1)[0], ratio, torch.full_like(ratio, float("inf")))
    _report(f"decode attention rows {fmt} B {B} len {length} waves {waves}", [(float(r), f"slot {i} {names[i]}") for i, r in enumerate(ratio)])
