"""Alignment to the tightest box on the MI355X (csrc/pc_align.hpp, meshanything_amd/pc_align.py): extents, volumes and best against the
numpy restatement `pc_align_ref.extents_ref`, and a turned box through `Dataset(..., align_iters=...)`.  Every GPU step runs in a fresh
interpreter under a time limit; the comparisons run here.

Min and max do not depend on the order of the rows and the workgroups combine through integer atomics on a monotone key: the outputs are a
function of the inputs alone, so they must EQUAL the restatement's, a second run's, and a run on a workspace full of 0xFF.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import pc_align_ref as R

if R.REPO not in sys.path:
    sys.path.insert(0, R.REPO)

from meshanything_amd import pc_align                             # noqa: E402

pytestmark = pytest.mark.gpu

REPO = R.REPO
TESTS = os.path.dirname(os.path.abspath(__file__))
ROWS_PER_GROUP = R.ROWS_PER_GROUP                                  # the rows of one workgroup (pca::ROWS = 256 threads x 32 rows)
HYP_TILE = R.HYP_TILE                                              # the hypotheses of one workgroup (pca::TILE)
TAU = 2 * 4.13e-4                                                  # tests/test_pc_align_host.py: twice the worst volume excess measured there
E2E_ROWS = 16384

_PRELUDE = f"""
import sys
sys.path[:0] = [{REPO!r}, {TESTS!r}]
import ctypes as C
import numpy as np
import torch
import pc_align_ref as R
import test_gpu_pc_align as T
from meshanything_amd import _lib, pc_align
out = {{}}
"""


def _gpu(tmp_path, body, timeout=300):
    """Run `body` (after _PRELUDE) in a fresh interpreter; it fills the dict `out`, which comes back as a dict of arrays, and its stdout."""
    script = tmp_path / "job.py"
    res = tmp_path / "out.npz"
    script.write_text(_PRELUDE + body + f"\nnp.savez({str(res)!r}, **out)\n")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=timeout, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with np.load(res) as z:
        return {k: z[k] for k in z.files}, r.stdout


def test_the_shapes_are_the_ones_the_kernel_can_go_wrong_at():
    got = set(R.SHAPES)
    assert {(1, 3, 1)} <= got and {(257, ld, H) for ld in (3, 6) for H in (1, 3, 65)} <= got
    assert {N for N, _, _ in got} >= {ROWS_PER_GROUP - 1, ROWS_PER_GROUP, ROWS_PER_GROUP + 1, 2 * ROWS_PER_GROUP - 1, 2 * ROWS_PER_GROUP, 2 * ROWS_PER_GROUP + 1}
    assert {H for _, _, H in got} >= {HYP_TILE - 1, HYP_TILE, HYP_TILE + 1} and ROWS_PER_GROUP == 8192 and HYP_TILE == 8


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
_KERNEL = """
lib = _lib.load()
def same(a, b):
    return all(a[w].cpu().numpy().tobytes() == b[w].cpu().numpy().tobytes() for w in a)
def raw(p, r, c, fill, want=pc_align.WANT, nbytes=None, N=None, H=None, ld=None, null=()):
    # the C ABI itself, on a workspace filled with `fill` and outputs filled with a sentinel -> (rc, message, outputs)
    N, H, ld = p.shape[0] if N is None else N, r.shape[0] if H is None else H, p.shape[1] if ld is None else ld
    need = lib.ma_pc_align_workspace_bytes(p.shape[0], r.shape[0])
    ws = torch.full((max(need, 1),), fill, dtype=torch.uint8, device="cuda")
    outs = {"extents": torch.full((r.shape[0], 6), -7.0, dtype=torch.float32, device="cuda"), "volumes": torch.full((r.shape[0],), -7.0, dtype=torch.float64, device="cuda"),
            "best": torch.full((1,), -7, dtype=torch.int32, device="cuda")}
    ptr = lambda w: outs[w].data_ptr() if w in want else None
    arg = lambda name, t: None if name in null else t
    rc = lib.ma_op_pc_align_extents(arg("ref", p.data_ptr()), N, ld, arg("centre", (C.c_float * 3)(*c.tolist())), arg("rot", r.data_ptr()), H, ptr("extents"), ptr("volumes"), ptr("best"),
                                    arg("workspace", ws.data_ptr()), need if nbytes is None else nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, (lib.ma_last_error(None) or b"").decode(), outs
def run(name, cloud, rot, centre):
    p, r = torch.from_numpy(cloud).cuda(), torch.from_numpy(rot).cuda()
    got = pc_align.box_extents(p, r, centre, want=pc_align.WANT)
    out[name + "_twice"] = np.array(same(got, pc_align.box_extents(p, r.reshape(-1, 3, 3), torch.from_numpy(centre), want=pc_align.WANT)))
    alone = [pc_align.box_extents(p, r, centre, want=w) for w in pc_align.WANT]      # each output with the other two NULL
    out[name + "_alone"] = np.array(all(list(a) == [w] and same(a, {w: got[w]}) for a, w in zip(alone, pc_align.WANT)))
    default = pc_align.box_extents(p, r, centre)
    out[name + "_default"] = np.array(sorted(default) == ["best", "volumes"] and same(default, {w: got[w] for w in default}))
    rc, _, filled = raw(p, r, centre, 0xFF)
    out[name + "_ff"] = np.array(rc == 0 and same(got, filled))
    for w in got:
        out[name + "_" + w] = got[w].cpu().numpy()
for N, ld, H in R.SHAPES:
    run(f"n{N}_ld{ld}_h{H}", *R.uniform_case(N, ld, H)[:3])
for name, case in R.content_cases().items():
    run(name, *case[:3])
# the (N, 6) cloud against its (N, 3) copy, and a strided view
cloud, rot, centre, _ = R.uniform_case(257, 6, 65)
p, r = torch.from_numpy(cloud).cuda(), torch.from_numpy(rot).cuda()
six, three = pc_align.box_extents(p, r, centre, want=pc_align.WANT), pc_align.box_extents(p[:, :3].contiguous(), r, centre, want=pc_align.WANT)
wide = torch.cat([p, p], 1)
view = pc_align.box_extents(wide[:, 6:], torch.cat([r, r], 1)[:, 9:], centre, want=pc_align.WANT)
out["six_is_three"], out["view"] = np.array(same(six, three)), np.array(same(six, view))
# refusals of the C ABI with real device pointers: non-zero, a message, and nothing launched (the sentinels stand)
p3 = p[:, :3].contiguous()
untouched = lambda outs: bool((outs["extents"] == -7).all() and (outs["volumes"] == -7).all() and (outs["best"] == -7).all())
abi = []
for kw in (dict(null=("ref",)), dict(null=("centre",)), dict(null=("rot",)), dict(null=("workspace",)), dict(want=()), dict(N=0), dict(N=(1 << 22) + 1), dict(H=0),
           dict(H=(1 << 16) + 1), dict(ld=4), dict(ld=2), dict(nbytes=0), dict(nbytes=lib.ma_pc_align_workspace_bytes(257, 65) - 1)):
    rc, msg, outs = raw(p3, r, centre, 0, **kw)
    abi.append(f"{rc}|{int(untouched(outs))}|{msg}")
out["abi"] = np.array(abi)
rc, msg, outs = raw(p3, r, centre, 0)
out["abi_good"] = np.array(rc == 0 and same(six, outs))
# refusals of the Python op with tensors on the device
def refused(fn):
    try:
        fn()
        return ""
    except ValueError as e:
        return str(e)
out["errors"] = np.array([refused(lambda: pc_align.box_extents(p3[:0], r, centre)), refused(lambda: pc_align.box_extents(p3, r[:0], centre)),
                          refused(lambda: pc_align.box_extents(p3, torch.zeros(((1 << 16) + 1, 9), device="cuda"), centre)), refused(lambda: pc_align.box_extents(p3.cpu(), r.cpu(), centre)),
                          refused(lambda: pc_align.box_extents(p3, r.cpu(), centre)), refused(lambda: pc_align.box_extents(p3, r, centre[:2])),
                          refused(lambda: pc_align.box_extents(p3, r, centre, want=("volume",))), refused(lambda: pc_align.box_extents(p3.double(), r, centre))])
"""


@pytest.fixture(scope="module")
def kernel_out(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_align"), _KERNEL)[0]


def _check(out, name, case):
    cloud, rot, _, (ext, vol, best) = case
    H = rot.shape[0]
    got_e, got_v, got_b = out[name + "_extents"], out[name + "_volumes"], out[name + "_best"]
    assert got_e.dtype == np.float32 and got_e.shape == (H, 6) and got_v.dtype == np.float64 and got_v.shape == (H,) and got_b.dtype == np.int32 and got_b.shape == (1,), name
    assert np.array_equal(got_e, ext, equal_nan=True), name
    assert not (np.signbit(got_e) & (got_e == 0)).any(), name        # a zero extent is +0
    assert (got_v == vol).all(), name
    assert int(got_b[0]) == best, name
    assert bool(out[name + "_twice"]) and bool(out[name + "_alone"]) and bool(out[name + "_default"]) and bool(out[name + "_ff"]), name


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "n%d_ld%d_h%d" % s)
def test_extents_volumes_and_best_equal_the_restatement(kernel_out, shape):
    N, ld, H = shape
    case = R.uniform_case(N, ld, H)
    assert case[0].shape == (N, ld) and case[1].shape == (H, 9)
    _check(kernel_out, f"n{N}_ld{ld}_h{H}", case)
    if N == 1:
        ext = kernel_out[f"n{N}_ld{ld}_h{H}_extents"]
        assert np.array_equal(ext[:, :3], ext[:, 3:]) and (kernel_out[f"n{N}_ld{ld}_h{H}_volumes"] == 0).all() and int(kernel_out[f"n{N}_ld{ld}_h{H}_best"][0]) == 0


@pytest.mark.parametrize("name", ["at_centre", "minus_zero", "twin", "nan_entry", "overflow", "all_bad"])
def test_zeros_twins_and_bad_hypotheses(kernel_out, name):
    case = R.content_cases()[name]
    _check(kernel_out, name, case)
    ext, vol, best = kernel_out[name + "_extents"], kernel_out[name + "_volumes"], int(kernel_out[name + "_best"][0])
    if name == "at_centre":
        assert (ext == 0).all() and (vol == 0).all() and best == 0
    if name == "twin":
        assert best == 4 and vol[4] == vol[13] == vol.min()          # of two identical hypotheses at the top the lower index
    if name == "nan_entry":
        assert np.isnan(ext[[2, 5]]).all() and (vol[[2, 5]] == np.inf).all() and best not in (2, 5) and np.isfinite(np.delete(vol, [2, 5])).all()
    if name == "overflow":
        bad = np.isinf(vol)
        assert bad[3] and not bad[[1, 6]].any() and np.isnan(ext[bad]).all() and np.isfinite(ext[~bad]).all() and (vol[bad] > 0).all() and not bad[best]
    if name == "all_bad":
        assert best == -1 and (vol == np.inf).all() and np.isnan(ext).all()


def test_six_columns_are_three_and_a_strided_view(kernel_out):
    assert bool(kernel_out["six_is_three"]) and bool(kernel_out["view"])


def test_refusals(kernel_out):
    abi = [e.split("|", 2) for e in kernel_out["abi"].tolist()]
    assert len(abi) == 13 and bool(kernel_out["abi_good"])
    for (rc, untouched, msg), word in zip(abi, ["null"] * 4 + ["at least one"] + ["N <="] * 2 + ["H <="] * 2 + ["ref_ld"] * 2 + ["workspace"] * 2):
        assert int(rc) != 0 and untouched == "1" and msg.startswith("ma_op_pc_align_extents:") and word in msg, (rc, untouched, msg)
    errors = kernel_out["errors"].tolist()
    assert len(errors) == 8 and all(errors), errors
    assert "N = 0" in errors[0] and "H = 0" in errors[1] and "2^16" in errors[2] and "CUDA tensor" in errors[3] and "device" in errors[4]
    assert "centre" in errors[5] and "want" in errors[6] and "float32" in errors[7]


# ---- the input side --------------------------------------------------------------------------------------------------------------------
def e2e_file():
    """-> (rows (16 384, 6) float32): the 1 x 0.6 x 0.3 box's surface with its normals, turned 25 degrees about (1, 2, 3) / sqrt(14) and shifted"""
    xyz, normals = R.box_surface(E2E_ROWS, 9)
    return np.concatenate([R.turn(xyz, R.R_25, (3.0, -2.0, 5.0)), normals @ R.R_25.T], 1).astype(np.float32)


_E2E = """
import os
from meshanything_amd.data import Dataset
tmp = os.path.dirname(os.path.abspath(__file__))
path = os.path.join(tmp, "box.npy")
np.save(path, T.e2e_file())
for kind in ("pc_normal", "pc_xyz"):
    for tag, kw in (("on", dict(align_iters=4096)), ("off", {})):
        np.random.seed(3)
        ds = Dataset(kind, [path], **kw)
        item = ds[0]
        out[f"{kind}_{tag}_n"], out[f"{kind}_{tag}_keys"], out[f"{kind}_{tag}_item"], out[f"{kind}_{tag}_raw"] = np.array(len(ds)), np.array(sorted(item)), item["pc_normal"], ds.data[0]["pc_normal"]
        if tag == "on":
            out[kind + "_R"], out[kind + "_c"] = item["pose"]
"""


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_align_e2e"), _E2E)


def _half_extents(item):
    return np.sort(np.abs(item[:, :3].astype(np.float64)).max(0))[::-1]


@pytest.mark.parametrize("kind", ["pc_normal", "pc_xyz"])
def test_dataset_aligns_a_turned_box(e2e, kind):
    out, stdout = e2e
    want = 0.9995 * np.array(R.BOX)
    on, off = out[kind + "_on_item"], out[kind + "_off_item"]
    assert on.shape == (4096, 6) and on.dtype == np.float16 and int(out[kind + "_on_n"]) == 1
    assert out[kind + "_on_keys"].tolist() == ["pc_normal", "pose", "uid"] and out[kind + "_off_keys"].tolist() == ["pc_normal", "uid"]
    got_on, got_off = _half_extents(on), _half_extents(off)
    print(f"{kind}: per-axis max |coordinate| on {got_on.tolist()}, off {got_off.tolist()}, wanted {want.tolist()}; relative errors on {(got_on / want - 1).tolist()}")
    assert (np.abs(got_on / want - 1) <= TAU).all()
    assert (np.abs(got_off / want - 1) > TAU).any()
    Rp, c = out[kind + "_R"], out[kind + "_c"]
    assert Rp.shape == (3, 3) and Rp.dtype == np.float64 and c.shape == (3,) and c.dtype == np.float64 and np.abs(Rp @ Rp.T - np.eye(3)).max() < 1e-12
    assert R.angle_to_cube(Rp @ R.R_25, pc_align.cube_rotations()) < 1e-3
    assert stdout.count("box: alignment turned the cloud ") == 2 and stdout.count(", 20480 hypotheses") == 2
    if kind == "pc_normal":
        n = on[:, 3:].astype(np.float64)
        assert (np.abs(np.abs(n).max(1) - 1) < 1e-2).all() and (np.sort(np.abs(n), 1)[:, :2] < 1e-2).all()   # within 1e-2 of +- an axis
        # the pose undoes the turn: the aligned raw rows, taken back, are rows of the file
        raw = out["pc_normal_on_raw"].astype(np.float64)
        back = c + (raw[:, :3] - c) @ Rp
        np.random.seed(3)
        rows = e2e_file()[np.random.choice(E2E_ROWS, 4096, replace=False)]   # alignment draws nothing from the numpy RNG: the rows of the run without it
        assert np.abs(back - rows[:, :3]).max() < 1e-5 and _same_bytes(rows, out["pc_normal_off_raw"])


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
