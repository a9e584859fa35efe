"""tests/attn_cases.py on the host: the builder's promises, the closed forms against the float64 softmax, a float32 emulation of tile-wise
online softmax inside HALF the bound the GPU tests (test_gpu_attention_scores.py) hold the kernels to, and four deliberately wrong emulations
that the same checker must reject.  No GPU needed."""
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
