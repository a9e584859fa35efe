"""tests/attn_cases.py on the host: the builder's promises, the closed forms against the float64 softmax, a float32 emulation of tile-wise
online softmax inside HALF the bound the GPU tests (test_gpu_attention_scores.py) hold the kernels to, and four deliberately wrong emulations
that the same checker must reject.  The stacked launches of test_gpu_attention_batched.py: every sample keeps the builder's promises and the half bound,
every pair of samples of a launch and three emulated addressing mistakes are told apart by the bound (a condition on the cases), and
ma_op_attention_dense's argument checks (which all come before anything touches a device).  No GPU needed."""
import functools
import math

import pytest
import torch

import attn_cases as A

DENSE_SHAPES = [(257, 257, 2, 0), (130, 300, 2, -1), (70, 130, 2, 60), (96, 65, 3, -1)]       # the GPU test's (Sq, Sk, H, causal_offset)
DECODE_LENGTHS = [1, 17, 129, 1000, 2500]
FMT_OUT = [("f32", "f32"), ("bf16", "bf16"), ("fp16", "fp16"), ("bf16", "f32")]                # (inputs and P, output)


@functools.lru_cache(maxsize=None)
def _judged(fmt):
    """(name, case, float64 reference, analysis) of every case in `fmt`: built once, shared by the tests below, never modified."""
    return [(what, case, A.reference(case), A.analyse(case)) for what, case in _all_cases(fmt)]


def _all_cases(fmt):
    for (Sq, Sk, H, c) in DENSE_SHAPES:
        for case in A.dense_cases(Sq, Sk, H, c, fmt):
            yield f"{(Sq, Sk, H, c)} {case.name}", case
    for L in DECODE_LENGTHS:
        slots = A.decode_slots(L)
        case, names = A.decode_case(slots, len(slots), 2, fmt, seed=L)
        yield f"decode {L}", case


@pytest.mark.parametrize("fmt", ["f32", "bf16", "fp16"])
def test_builder_keeps_its_promises_after_rounding(fmt):
    """Scores come from the head's own dimension alone and are exactly sign * level; distinct levels of a row stay >= 30 nats apart after rounding to
    the format, equal ones bit-identical (they are the row's top keys: at least one, and exactly the pattern's count)."""
    for what, case, _, info in _judged(fmt):
        assert info["clean"], what
        assert float(info["gap"].min()) >= A.GAP, (what, float(info["gap"].min()))
        assert int(info["n_top"].min()) >= 1, what
        for t in (case.q, case.k, case.v):
            assert torch.equal(A.rnd(t, fmt), t) and bool(torch.isfinite(t).all()), what
    # the levels themselves: 16 equal keys per step, bit-identical after rounding, steps >= 30 apart even where the format's spacing is 32 (bf16 above 4096)
    t = A.rnd(A.stairs_up(2500).float(), fmt)
    assert bool((t.view(-1)[: 2496].view(-1, 16) == t[: 2496 : 16, None]).all())
    assert float((t[16::16] - t[:-16:16]).min()) >= A.GAP
    assert torch.equal(A.stairs_down(257) + A.stairs_up(257), torch.full((257,), 640.0, dtype=torch.float64))      # the mirror, on the same grid of 16
    assert A.head_dim(0) == 3 and A.head_dim(1) == 10 and len({A.head_dim(h) for h in range(16)}) == 16


def test_closed_forms_are_the_float64_softmax():
    """mean of V over the top visible keys == the softmax definition to n e^-30; and the table of the patterns, spelled out."""
    for fmt in ("f32", "bf16", "fp16"):
        for what, case, ref, info in _judged(fmt):
            tol = info["n_vis"].double().max() * math.exp(-A.GAP) * float(case.v.abs().max()) + 1e-12
            assert float((ref - info["out"]).abs().max()) <= float(tol), what
    Sq, Sk, H, c = 257, 257, 2, 0
    v = lambda case: case.v.double()
    cases = {x.name: x for x in A.dense_cases(Sq, Sk, H, c, "bf16")}
    up, down, zig = A.analyse(cases["stairs_up"])["out"], A.analyse(cases["stairs_down"])["out"], A.analyse(cases["zigzag"])["out"]
    for i in (0, 15, 16, 100, 256):                                   # causal: row i sees keys 0 .. i
        lo = i // 16 * 16
        assert torch.allclose(up[i], v(cases["stairs_up"])[lo:i + 1].mean(0), atol=1e-12)              # the visible keys of the top visible step
        assert torch.allclose(down[i], v(cases["stairs_down"])[0:min(i, 15) + 1].mean(0), atol=1e-12)   # ... of the first step
    assert torch.allclose(zig[100], v(cases["zigzag"])[96:101].mean(0), atol=1e-12) and torch.allclose(zig[101], v(cases["zigzag"])[0:16].mean(0), atol=1e-12)
    assert torch.allclose(A.analyse(cases["flat-96"])["out"][200], v(cases["flat-96"])[:201].mean(0), atol=1e-12)
    sp = A.build("spike(31, 32)", torch.stack([A.spike(Sk, 31), A.spike(Sk, 32)]), torch.ones(Sq), "bf16", causal_offset=c)      # head 0: key 31, head 1: key 32
    out = A.analyse(sp)["out"]
    assert torch.equal(out[31, 0], v(sp)[31, 0]) and torch.equal(out[32, 1], v(sp)[32, 1]) and torch.equal(out[200, 0], v(sp)[31, 0])
    assert torch.allclose(out[30, 0], v(sp)[:31, 0].mean(0), atol=1e-12) and torch.allclose(out[31, 1], v(sp)[:32, 1].mean(0), atol=1e-12)   # the row before does not see it
    tw = next(x for x in cases.values() if x.name.startswith("twin"))
    assert torch.equal(A.analyse(tw)["out"][256, 0], (v(tw)[5, 0] + v(tw)[70, 0]) / 2) and torch.equal(tw.k[5, 0], tw.k[70, 0])
    assert torch.equal(A.analyse(tw)["out"][69, 0], v(tw)[5, 0])


def test_half_ulp():
    x = torch.tensor([1.0, 1.5, 2.0, 0.75, 3e-6, 0.0], dtype=torch.float64)
    assert A.half_ulp(x, "bf16").tolist()[:4] == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9]
    assert A.half_ulp(x, "fp16").tolist() == [2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -12, 2.0 ** -25, 2.0 ** -25]      # (fp16 subnormals: spacing 2^-24)
    assert A.half_ulp(x, "f32").tolist()[:3] == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23]


@pytest.mark.parametrize("tile", [32, 64])
@pytest.mark.parametrize("fmt,out_fmt", FMT_OUT)
def test_online_softmax_emulation_stays_inside_half_the_bound(fmt, out_fmt, tile):
    worst = ("", 0.0)
    for what, case, ref, info in _judged(fmt):
        r = A.worst_ratio(A.emulate_online(case, tile, fmt, out_fmt), ref, A.bound(case, ref, info, out_fmt))
        worst = max(worst, (what, r), key=lambda x: x[1])
        # (the output's own rounding alone uses the bound's half-ulp term in full: "half the bound" holds for everything else)
        rest = A.worst_ratio(A.emulate_online(case, tile, fmt, "f32"), ref, A.bound(case, ref, info, "f32")) if out_fmt != "f32" else r
        assert r <= 1.0 and rest <= 0.5, (what, r, rest)
    print(f"emulation {fmt}->{out_fmt} tile {tile}: worst |err| / bound = {worst[1]:.3f} at {worst[0]}")


# ---- the batched launches of test_gpu_attention_batched.py ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batches(fmt):
    """Every stacked launch of the GPU tests in `fmt`, each sample judged once: [(batch, [(reference, analysis, bound in the kernel's output format)] per sample)]."""
    bs = [A.layout_batch(*launch, fmt) for launch in A.LAYOUT_LAUNCHES]
    if fmt != "f32":                                                  # (last_len exists in the 16-bit kernel only)
        bs += [A.last_len_batch(T, L, c, fmt) for (T, L) in A.LAST_LEN_LAUNCHES for c in (0, -1)]
        bs += [A.tail_batch(T, nt, fmt) for (T, nt) in A.TAIL_LAUNCHES]
    out = []
    for bt in bs:
        judged = []
        for case in bt.cases:
            ref, info = A.reference(case), A.analyse(case)
            judged.append((ref, info, A.bound(case, ref, info, fmt)))
        out.append((bt, judged))
    return out


@pytest.mark.parametrize("fmt", ["f32", "bf16", "fp16"])
def test_stacked_samples_keep_the_builders_promises(fmt):
    """Every sample of every launch is a closed-form case (clean scores, gaps >= 30 nats, finite values of the format) -- the shared query of the cross
    layout and the short last sample included -- and sits unchanged in the leading rows of the launch's buffers; the key behind a short sample dominates."""
    n = 0
    for bt, judged in _batches(fmt):
        assert bt.B == len(bt.cases) >= 3 and bt.H == A.BATCH_H and len({c.name for c in bt.cases}) == bt.B, bt.name
        for b, (case, (ref, info, bnd)) in enumerate(zip(bt.cases, judged)):
            nq, nk = bt.rows(b)
            assert info["clean"] and float(info["gap"].min()) >= A.GAP and int(info["n_top"].min()) >= 1, (bt.name, case.name)
            assert torch.equal(bt.q[b, :nq], case.q) and torch.equal(bt.k[b, :nk], case.k) and torch.equal(bt.v[b, :nk], case.v), (bt.name, case.name)
            assert (nq, nk) == ((bt.Sq, bt.Sk) if b < bt.B - 1 or bt.last_len < 0 else (bt.last_len, bt.last_len)), bt.name
            n += 1
        for t in (bt.q, bt.k, bt.v):
            assert torch.equal(A.rnd(t, fmt), t) and bool(torch.isfinite(t).all()), bt.name
        if 0 < bt.last_len < bt.Sk:
            L, last = bt.last_len, bt.cases[-1]
            hs, d = torch.arange(bt.H), torch.tensor(last.dims)
            assert float(last.k[:, hs, d].max()) == A.SPIKE and bool((last.k[L - 1, 0, d[0]] == A.SPIKE).all()), bt.name      # a dominant key exactly at last_len - 1
            assert bool((bt.k[-1, L, hs, d] - last.k[:, hs, d].max(dim=0).values >= A.GAP).all()), bt.name
            assert float((bt.v[-1, L] - last.v).abs().min(dim=0).values.mean()) > 1.0, bt.name
    assert n >= (100 if fmt == "f32" else 200)                         # (11 layout launches of 11 - 19 samples; 22 + 8 launches of 3)


@pytest.mark.parametrize("fmt", ["f32", "bf16", "fp16"])
def test_stacked_launches_discriminate(fmt):
    """A condition on the cases, not a measurement.  (1) Wrong sample: the exact result of sample b' judged as sample b is over the bound for EVERY pair
    b != b' of every launch (a short last sample: on the rows both have; for the cross layout's shared Q this is 'the wrong K / V').  (2) Every launch
    catches a query shifted by one row and K shifted by one row either way, and the short last sample ITSELF catches the keys behind last_len let in."""
    for bt, judged in _batches(fmt):
        for b in range(bt.B):
            ref, info, bnd = judged[b]
            for b2 in range(bt.B):
                if b2 == b:
                    continue
                if bt.rows(b2) == bt.rows(b):
                    other = judged[b2][0]
                else:                   # (a short sample on one side: sample b' read with sample b's lengths, from the launch's full-length buffers)
                    nq, nk = bt.rows(b)
                    c = bt.cases[b]
                    other = A.reference(A.Case("other", bt.q[b2, :nq], bt.k[b2, :nk], bt.v[b2, :nk], c.fmt, c.causal_offset, c.dims))
                r = A.worst_ratio(other, ref, bnd)
                assert r > 1.0, (bt.name, bt.cases[b].name, bt.cases[b2].name, r)
        caught = {}
        for b in range(bt.B):
            ref, info, bnd = judged[b]
            for name, wrong in A.wrong_variants(bt, b):
                r = A.worst_ratio(A.reference(wrong), ref, bnd)
                caught[name] = max(caught.get(name, 0.0), r)
                if name == "sk_full":
                    assert r > 1.0, (bt.name, name, r)
        assert set(caught) >= {"q_shift", "k_shift+", "k_shift-"} and all(r > 1.0 for r in caught.values()), (bt.name, caught)
        assert ("sk_full" in caught) == (0 < bt.last_len < bt.Sk), bt.name


@pytest.mark.parametrize("fmt", ["f32", "bf16", "fp16"])
def test_online_softmax_emulation_stays_inside_half_the_bound_on_stacked_samples(fmt):
    """The half-bound check above over every sample of every stacked launch (tile 64, the kernels' output formats)."""
    worst, seen = ("", 0.0), []
    for bt, judged in _batches(fmt):
        for case, (ref, info, bnd) in zip(bt.cases, judged):
            if any(c.name == case.name and c.q.shape == case.q.shape and c.k.shape == case.k.shape and torch.equal(c.q, case.q) and torch.equal(c.k, case.k) and torch.equal(c.v, case.v) for c in seen):
                continue                # (the same tensors in another launch: the layouts share their samples)
            seen.append(case)
            out32 = A.emulate_online(case, 64, fmt, "f32")            # (the output format is one rounding of this)
            r = A.worst_ratio(A.rnd(out32, fmt), ref, bnd)
            rest = A.worst_ratio(out32, ref, A.bound(case, ref, info, "f32")) if fmt != "f32" else r
            worst = max(worst, (f"{bt.name} {case.name}", r), key=lambda x: x[1])
            assert r <= 1.0 and rest <= 0.5, (bt.name, case.name, r, rest)
    print(f"emulation {fmt} on stacked samples: worst |err| / bound = {worst[1]:.3f} at {worst[0]}")


def test_attention_dense_refuses_bad_arguments_on_the_host():
    """ma_op_attention_dense checks every argument, and the launchers refuse what they refuse, before anything touches a device."""
    import ctypes as C
    from meshanything_amd import _lib, build
    build.build(force=False, verbose=False)
    lib = _lib.load()
    P, INVALID = 4096, -1                                             # a non-null, 16-byte aligned address that is never dereferenced
    assert C.sizeof(_lib.AttnDenseArgs) == 16 * 4 + 5 * 8 + 5 * 8
    assert lib.ma_attention_vt_workspace_elems(257, 2, 3) == 3 * 2 * 64 * 320 and lib.ma_attention_vt_workspace_elems(64, 1, 1) == 64 * 64
    assert lib.ma_attention_vt_workspace_elems(0, 2, 3) == 0 and lib.ma_attention_vt_workspace_elems(65, 2, -1) == 0
    assert lib.ma_op_attention_dense(None, None) == INVALID
    ok = dict(kernel=4, Sq=96, Sk=65, H=2, causal_offset=-1, batch=3, last_len=-1, scale=0.125, q_rs=384, q_hs=64, k_rs=384, k_hs=64, v_rs=384, v_hs=64, o_rs=128,
              q_bs=96 * 384, k_bs=96 * 384, v_bs=96 * 384, o_bs=96 * 128, vt_elems=3 * 2 * 64 * 128, Q=P, K=P, V=P, O=P, vt=P)
    bad = [dict(struct_size=0), dict(struct_size=100), dict(kernel=1), dict(kernel=2), dict(kernel=5), dict(kernel=-1), dict(Q=None), dict(K=None), dict(V=None), dict(O=None),
           dict(Q=P + 8), dict(O=P + 2), dict(vt=P + 4), dict(Sq=0), dict(Sk=-1), dict(H=0), dict(batch=0), dict(scale=0.0), dict(scale=float("nan")), dict(scale=float("inf")),
           dict(q_rs=32), dict(o_rs=64), dict(k_hs=-64), dict(v_hs=32), dict(k_bs=0), dict(v_bs=0), dict(o_bs=0), dict(q_bs=1 << 41), dict(vt=None),
           dict(vt_elems=3 * 2 * 64 * 128 - 1), dict(vt_elems=0), dict(Sk=129),
           dict(last_len=0), dict(last_len=97), dict(last_len=66), dict(last_len=96), dict(q_rs=388), dict(k_hs=68), dict(v_rs=380), dict(o_rs=132), dict(q_bs=96 * 384 + 4),
           dict(k_bs=96 * 384 - 4), dict(o_bs=96 * 128 + 4),
           dict(kernel=0, last_len=0), dict(kernel=0, last_len=1), dict(kernel=0, last_len=65), dict(kernel=3, last_len=0), dict(kernel=3, last_len=65),
           dict(kernel=0, q_rs=386), dict(kernel=0, v_bs=96 * 384 + 2), dict(kernel=3, k_rs=388), dict(kernel=3, q_bs=96 * 384 + 4)]
    for kw in bad:
        a = dict(ok, **kw)
        size = a.pop("struct_size", None)
        s = _lib.AttnDenseArgs(**a)
        if size is not None:
            s.struct_size = size
        assert lib.ma_op_attention_dense(C.byref(s), None) == INVALID, kw
        assert b"ma_op_attention_dense" in lib.ma_last_error(None), kw
    try:
        assert lib.ma_op_set_half_dtype(2) == 0
        assert lib.ma_op_attention_dense(C.byref(_lib.AttnDenseArgs(**dict(ok, kernel=3))), None) == INVALID and b"bf16 only" in lib.ma_last_error(None)
    finally:
        lib.ma_op_set_half_dtype(1)


@pytest.mark.parametrize("bug,where", [("drop_newest", "spike"), ("mask_off_by_one", "spike"), ("no_rescale", "stairs_up"), ("max_from_zero", "flat")])
@pytest.mark.parametrize("fmt,out_fmt", FMT_OUT)
def test_the_checker_rejects_wrong_emulations(fmt, out_fmt, bug, where):
    """Each wrong emulation must exceed the bound on at least one case of the pattern built to catch it -- and the correct one on none (above)."""
    caught = []
    for what, case, ref, info in _judged(fmt):
        if bug == "mask_off_by_one" and case.causal_offset < 0:
            continue
        if A.worst_ratio(A.emulate_online(case, 64, fmt, out_fmt, bug=bug), ref, A.bound(case, ref, info, out_fmt)) > 1.0:
            caught.append(what)
    assert any(where in c for c in caught), (bug, caught)
    assert len(caught) >= 2, (bug, caught)
