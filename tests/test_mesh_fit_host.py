"""The mesh fit without a GPU (meshanything_amd/mesh_fit.py, main.py --fit_iters): every argument refusal, the
float32 restatement (b) of the kernel against the float64 definition (a) of tests/mesh_fit_ref.py on the inputs of the GPU tests, the
host's assembly and solve against (a)'s dense system, and the whole fit of the crafted cases through (a) alone.

MEASURED on (a) (`test_the_definition_alone_meets_the_end_to_end_conditions` prints them): the jittered cube's largest vertex error
1.50e-02 falls to 2.04e-03, 4.25e-05, 1.13e-06 and 3.75e-08 after 1, 2, 3 and 4 iterations with the defaults (4.0e5 x after four);
against float16 rows it settles at 9.77e-05, the rounding of 0.4.  (b) against (a): see tests/test_gpu_mesh_fit.py.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_fit_ref as R
import mesh_score_ref as SR

from meshanything_amd import _lib, build, mesh_fit                  # noqa: E402

REPO = R.REPO


def _cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ma_main_cli_fit", os.path.join(REPO, "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
def test_check_fit_args():
    assert mesh_fit.check_fit_args(0) == (0, 4.0, 2.0, 1.0, 0.0)
    assert mesh_fit.check_fit_args(32, 64, 64, 0.5, 0.99) == (32, 64.0, 64.0, 0.5, 0.99)
    assert mesh_fit.check_fit_args(3, fit_max_move=4) == (3, 4.0, 4.0, 1.0, 0.0)
    nan, inf = float("nan"), float("inf")
    for bad, word in (((-1,), "fit_iters"), ((33,), "fit_iters"), ((1.5,), "fit_iters"), ((True,), "fit_iters"),
                      ((2, 0.0), "fit_dist"), ((2, 64.5), "fit_dist"), ((2, nan), "fit_dist"), ((2, inf), "fit_dist"), ((2, -1.0), "fit_dist"),
                      ((2, None, 0.0), "fit_max_move"), ((2, None, nan), "fit_max_move"), ((2, None, 4.5), "at most fit_dist"), ((2, 1.0, 2.0), "at most fit_dist"),
                      ((2, None, None, 0.0), "fit_stiffness"), ((2, None, None, inf), "fit_stiffness"), ((2, None, None, nan), "fit_stiffness"),
                      ((2, None, None, None, 1.0), "fit_normal_cos"), ((2, None, None, None, -0.1), "fit_normal_cos"), ((2, None, None, None, nan), "fit_normal_cos"),
                      ((0, 4.0), "fit_dist needs fit_iters > 0"), ((0, None, 2.0), "fit_max_move needs fit_iters > 0"),
                      ((0, None, None, 1.0), "fit_stiffness needs fit_iters > 0"), ((0, None, None, None, 0.5), "fit_normal_cos needs fit_iters > 0"),
                      ((0, 4.0, 2.0), "fit_dist, fit_max_move need fit_iters > 0")):
        with pytest.raises(ValueError, match=word):
            mesh_fit.check_fit_args(*bad)
    with pytest.raises(ValueError, match="fit_iters"):
        mesh_fit.fit_mesh(*R.jittered_cube(), R.cube_cloud(64), 0)


def test_cli_flags(capsys):
    cli = _cli()
    base = ["--input_type", "pc_normal", "--input_path", "x.npy"]
    a = cli.get_args(base)
    assert (a.fit_iters, a.fit_dist, a.fit_max_move, a.fit_stiffness, a.fit_normal_cos) == (0, None, None, None, None)
    a = cli.get_args(base + ["--fit_iters", "3"])
    assert (a.fit_iters, a.fit_dist, a.fit_max_move, a.fit_stiffness, a.fit_normal_cos) == (3, 4.0, 2.0, 1.0, 0.0)
    a = cli.get_args(["--input_type", "mesh", "--input_path", "x.obj", "--fit_iters", "32", "--fit_dist", "64", "--fit_max_move", "64", "--fit_stiffness", "0.25",
                      "--fit_normal_cos", "0.5"])                       # every input type
    assert (a.fit_iters, a.fit_dist, a.fit_max_move, a.fit_stiffness, a.fit_normal_cos) == (32, 64.0, 64.0, 0.25, 0.5)
    for bad, msg in ((["--fit_iters", "33"], "--fit_iters must be 0 (off) or in 1..32"), (["--fit_iters", "-1"], "--fit_iters must be 0 (off) or in 1..32"),
                     (["--fit_dist", "3"], "--fit_dist needs --fit_iters > 0"), (["--fit_max_move", "1"], "--fit_max_move needs --fit_iters > 0"),
                     (["--fit_stiffness", "2"], "--fit_stiffness needs --fit_iters > 0"), (["--fit_normal_cos", "0.5"], "--fit_normal_cos needs --fit_iters > 0"),
                     (["--fit_dist", "3", "--fit_stiffness", "2"], "--fit_dist and --fit_stiffness need --fit_iters > 0"),
                     (["--fit_iters", "2", "--fit_dist", "0"], "--fit_dist must be finite, > 0 and at most 64"),
                     (["--fit_iters", "2", "--fit_dist", "65"], "--fit_dist must be finite, > 0 and at most 64"),
                     (["--fit_iters", "2", "--fit_dist", "nan"], "--fit_dist must be finite, > 0 and at most 64"),
                     (["--fit_iters", "2", "--fit_max_move", "0"], "--fit_max_move must be finite and > 0"),
                     (["--fit_iters", "2", "--fit_max_move", "inf"], "--fit_max_move must be finite and > 0"),
                     (["--fit_iters", "2", "--fit_max_move", "5"], "--fit_max_move must be at most --fit_dist"),
                     (["--fit_iters", "2", "--fit_dist", "1", "--fit_max_move", "2"], "--fit_max_move must be at most --fit_dist"),
                     (["--fit_iters", "2", "--fit_stiffness", "0"], "--fit_stiffness must be finite and > 0"),
                     (["--fit_iters", "2", "--fit_stiffness", "inf"], "--fit_stiffness must be finite and > 0"),
                     (["--fit_iters", "2", "--fit_normal_cos", "1"], "--fit_normal_cos must be in [0, 1)"),
                     (["--fit_iters", "2", "--fit_normal_cos", "-0.5"], "--fit_normal_cos must be in [0, 1)")):
        with pytest.raises(SystemExit):
            cli.get_args(base + bad)
        assert msg in capsys.readouterr().err, bad
    assert "--fit_iters" in cli.__doc__ and "mesh_fit.py" in cli.__doc__
    # the CLI's ranges are the module's
    for name, (default, _, _) in cli.FIT_FLAGS.items():
        assert mesh_fit.DEFAULTS[name] == default
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "--fit_iters" in readme


def test_cli_help_lists_the_flags():
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--fit_iters", "--fit_dist", "--fit_max_move", "--fit_stiffness", "--fit_normal_cos"):
        assert flag in r.stdout


def test_the_switch_off_imports_nothing():
    """In a fresh interpreter: parsing a command line without the flag, and with it, leaves mesh_fit unimported (main() imports it only
    inside the branch that fits), and the flag never reaches CloudPrep or Dataset."""
    code = f"""
import sys
sys.path.insert(0, {REPO!r})
import main
from meshanything_amd.cloud_prep import CloudPrep
import meshanything_amd.data, meshanything_amd.mesh_export, meshanything_amd.model
args = main.get_args(["--input_type", "pc_normal", "--input_path", "x.npy"])
assert not any("fit" in k for k in vars(CloudPrep.from_args(args)))
args = main.get_args(["--input_type", "pc_normal", "--input_path", "x.npy", "--fit_iters", "2"])
assert not any("fit" in k for k in vars(CloudPrep.from_args(args)))
assert "meshanything_amd.mesh_fit" not in sys.modules
print("off: ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.splitlines() == ["off: ok"], r.stdout + r.stderr
    src = open(os.path.join(REPO, "main.py")).read()
    assert src.count("mesh_fit import") == 1
    at = src.index("mesh_fit import")
    assert "if args.fit_iters > 0" in src[at - 300:at]


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def test_input_refusals():
    v, f = R.jittered_cube()
    cl = R.cube_cloud(64)
    mesh_fit.check_fit_inputs(v, f, cl)
    mesh_fit.check_fit_inputs(torch.from_numpy(v), torch.from_numpy(f).int(), torch.from_numpy(cl).half())
    for args, word in (((v, f, cl[:, :3]), "needs the cloud's normals"), ((v, f, cl.astype(np.float64)), "float16 or float32"),
                       ((v[:, :2], f, cl), "verts must be"), ((v, f[:, :2], cl), "faces must be"), ((v, f.astype(np.float32), cl), "faces must be"),
                       ((v, f, cl, 0.0), "mesh_scale"), ((v, f, cl, float("inf")), "mesh_scale")):
        with pytest.raises(ValueError, match=word):
            mesh_fit.check_fit_inputs(*args)
    bad = v.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="verts has non-finite"):
        mesh_fit.check_fit_inputs(bad, f, cl)
    for col in (2, 4):
        bad = cl.copy()
        bad[5, col] = np.inf
        with pytest.raises(ValueError, match="cloud has non-finite"):
            mesh_fit.check_fit_inputs(v, f, bad)
    for idx in (8, -1):
        bad = f.copy()
        bad[11, 2] = idx
        with pytest.raises(ValueError, match="faces must index the 8 vertices"):
            mesh_fit.check_fit_inputs(v, bad, cl)
    # the limits: M <= 4096, V <= 3 M, P <= 2^22
    many = np.zeros((4097, 3), np.int64)
    with pytest.raises(ValueError, match="outside the limits"):
        mesh_fit.check_fit_inputs(v, many, cl)
    with pytest.raises(ValueError, match="outside the limits"):
        mesh_fit.check_fit_inputs(np.zeros((37, 3), np.float32), f, cl)                       # 12 faces: at most 36 vertices
    with pytest.raises(ValueError, match="outside the limits"):
        mesh_fit.check_fit_inputs(v, f, torch.zeros(((1 << 22) + 1, 6), dtype=torch.float16))
    mesh_fit.check_fit_inputs(np.zeros((36, 3), np.float32), f, cl)
    # a host tensor is refused, as in score_meshes; and so are a bad dist and cosine, before any device is looked for
    with pytest.raises(ValueError, match="CUDA tensor"):
        mesh_fit.fit_pairs(torch.from_numpy(v), f, cl, 0.05)
    for d in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="dist must be"):
            mesh_fit.fit_pairs(torch.from_numpy(v), f, cl, d)
    with pytest.raises(ValueError, match="normal_cos"):
        mesh_fit.fit_pairs(torch.from_numpy(v), f, cl, 0.05, 1.0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mesh_fit.fit_mesh(v, f, cl, 2)
    with pytest.raises(ValueError, match="at most 1"):
        mesh_fit.fit_mesh(v, f, cl, 2, dist=64.0, mesh_scale=4.0)


def test_c_abi_refuses_bad_arguments_without_a_gpu():
    build.build(force=False, verbose=False)
    lib = _lib.load()
    assert lib.ma_mesh_fit_workspace_bytes(8, 12, 4096) == 2 * 4096 * 4 + 256
    assert lib.ma_mesh_fit_workspace_bytes(3, 1, 1) == 2 * 256 + 256
    assert lib.ma_mesh_fit_workspace_bytes(3 * 4096, 4096, 1 << 22) > 0
    for V, M, P in ((8, 4097, 64), (37, 12, 64), (8, 12, (1 << 22) + 1), (0, 12, 64), (8, 0, 64), (8, 12, 0)):
        assert lib.ma_mesh_fit_workspace_bytes(V, M, P) == 0
    p = 4096                                                           # never dereferenced: every call below is refused before a HIP call
    ok = dict(V=8, M=12, ld=6, P=64, dist=0.05, cos=0.0, flat=mesh_fit.FLAT, ws=1 << 20)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.ma_op_mesh_fit_pairs(p, a["V"], p, a["M"], p, a["ld"], a["P"], a["dist"], a["cos"], a["flat"], p, p, a.get("sums", p), p, a["ws"], None)
        return rc, lib.ma_last_error(None).decode()
    for kw, word in ((dict(M=4097), "M <= 4096"), (dict(V=37), "V <= 3 M"), (dict(P=(1 << 22) + 1), "P <= 2^22"), (dict(ld=3), "cloud_ld must be 6"),
                     (dict(dist=0.0), "dist"), (dict(dist=1.5), "dist"), (dict(dist=float("nan")), "dist"), (dict(cos=1.0), "min_cos"),
                     (dict(cos=-0.5), "min_cos"), (dict(flat=-1.0), "flat"), (dict(ws=100), "workspace smaller"), (dict(sums=None), "null pointer")):
        rc, msg = call(**kw)
        assert rc == -1 and "ma_op_mesh_fit_pairs" in msg and word in msg, (kw, msg)


# ---- (b) against (a) ------------------------------------------------------------------------------------------------------------------
def test_the_restatement_agrees_with_the_definition():
    pt, fc, mism = R.figures()
    print(f"(b) against (a) on kernel_cases(): per point {pt:.3e}, per face {fc:.3e}; differently paired {mism}")
    from test_gpu_mesh_fit import RESOLUTION
    for name, rows in mism.items():
        for q, fa, fb, gap in rows:
            assert gap <= RESOLUTION, (name, q, fa, fb, gap)
    assert sum(len(r) for r in mism.values()) <= 16                     # ties on shared edges, not a habit
    assert 0 < pt < 1e-4                                                 # float32 on coordinates below 1: far below the lattice's 7.8e-3
    # the hand-made points
    v, f, cl, d = R.quad_case(63)
    for res in (R.pairs_f32(v, f, cl, d), R.pairs_ref(v, f, cl, d)):
        assert res["face"][:5].tolist() == [0, 0, 0, -1, -1]
        assert np.allclose(res["w"][0], [0.5, 0, 0.5]) and np.allclose(res["w"][1], [1, 0, 0])


def _dense_from_blocks(A, g, faces, V, stiffness):
    H, b = stiffness * np.eye(3 * V), np.zeros(3 * V)
    for i, t in enumerate(np.asarray(faces)):
        cols = (3 * t[:, None] + np.arange(3)[None]).reshape(-1)
        H[np.ix_(cols, cols)] += A[i]
        b[cols] += g[i]
    return H, b


@pytest.mark.parametrize("name", ["cube_p4096", "quad_p63", "m255_p65"])
def test_host_assembly_and_step_agree_with_the_dense_definition(name):
    """normal_equations + solve_step on (b)'s integer sums against (a)'s dense system and numpy.linalg.solve.  The per-face figure is a
    deviation per paired point, so an assembled entry is within the figure times the number of pairs; the step solves (H + I) x = g, and with the smallest eigenvalue at 1 (the
    stiffness) an error E in H and e in g moves x by at most |e| + |E| |x| (2-norms, first order)."""
    pt, fc, mism = R.figures()
    v, f, cl, d, mc = R.kernel_cases()[name]
    cl32 = np.asarray(cl).astype(np.float32)
    b = R.pairs_f32(v, f, cl, d, mc)
    A, g, n, _, _ = mesh_fit.normal_equations(b["sums"], f)
    assert np.array_equal(n, np.bincount(b["face"][b["face"] >= 0], minlength=len(f)))
    assert np.array_equal(A, A.transpose(0, 2, 1))
    V = len(v)
    Hb, gb = _dense_from_blocks(A, g, f, V, 1.0)
    want, pr = R.step_ref(v, f, cl32, d, 1.0, mc)
    Ha, ga = R.dense_system(pr, f, cl32, V, 1.0)
    npair = int(n.sum())
    assert not mism[name] or name == "cube_p4096"
    extra = sum(1 for _ in mism[name]) * 2.0                            # a differently paired point moves its (whole, <= 1) term to another block
    assert np.abs(Hb - Ha).max() <= fc * npair + extra and np.abs(gb - ga).max() <= fc * npair + extra * d
    got = mesh_fit.solve_step(A, g, f, V, 1.0)
    assert np.abs(np.linalg.solve(Hb, gb).reshape(-1, 3) - got).max() <= 1e-9          # the conjugate gradients solve what was assembled
    if not mism[name]:
        e, E = np.linalg.norm(gb - ga), np.linalg.norm(Hb - Ha, 2)
        assert np.linalg.norm(got - want) <= 1.01 * (e + E * np.linalg.norm(want)) + 1e-9
    print(f"{name}: {npair} pairs, step against (a): {np.abs(got - want).max():.3e} of {np.abs(want).max():.3e}")
    assert np.abs(got - want).max() <= 8 * pt + 1e-9 or name != "cube_p4096"
    assert mesh_fit.solve_step(np.zeros_like(A), np.zeros_like(g), f, V, 1.0).tolist() == np.zeros((V, 3)).tolist()


def test_clamp():
    x0 = np.zeros((3, 3))
    x = np.array([[3.0, 4.0, 0.0], [0.3, 0.4, 0.0], [0.0, 0.0, 0.0]])
    out = mesh_fit.clamp_moves(x, x0, 1.0)
    assert np.allclose(out[0], [0.6, 0.8, 0.0]) and np.array_equal(out[1:], x[1:])


# ---- the whole fit through (a) ---------------------------------------------------------------------------------------------------------
def _err(x):
    return float(np.abs(np.asarray(x, np.float64) * 2.0 - R.cube_mesh()[0]).max())


def test_the_definition_alone_meets_the_end_to_end_conditions():
    v, f = R.jittered_cube()
    cl = R.cube_cloud()
    start = _err(v)
    errs = [_err(R.fit_ref(v, f, cl, k)[0]) for k in (1, 2, 3, 4)]
    half = _err(R.fit_ref(v, f, R.cube_cloud(dtype=np.float16), 4)[0])
    print(f"jittered cube through (a): {start:.3e} -> " + ", ".join(f"{e:.3e}" for e in errs) + f"; float16 rows: {half:.3e}")
    assert errs[3] * 100 <= start and errs[1] * 100 <= start and half <= 2.0 ** -12
    # out of reach: nothing pairs, nothing moves
    x, its = R.fit_ref(v, f, R.shifted_cloud(10.0), 4)
    assert its == [(0.0, 0.0, 0.0)] and np.array_equal(x, v.astype(np.float64))
    # the pulled vertex goes the cap toward its place, nobody further
    pv, pf = R.pulled_cube(6.0)
    x, _ = R.fit_ref(pv, pf, cl, 4, max_move=2.0)
    d = (x - pv.astype(np.float64)) * 2.0
    ln, cap = np.linalg.norm(d, axis=1), 2.0 * R.STEP
    print(f"pulled vertex through (a): moved {ln[7] / R.STEP:.6f} steps, {d[7] @ (-np.ones(3) / np.sqrt(3.0)) / R.STEP:.6f} of them along the diagonal")
    assert abs(ln[7] - cap) <= 1e-12 and (ln <= cap + 1e-12).all()
    assert d[7] @ (-np.ones(3) / np.sqrt(3.0)) >= cap * (1 - 1e-6)
    # the fin's apex has no support
    fv, ff = R.fin_cube()
    x, _ = R.fit_ref(fv, ff, cl, 4)
    assert np.array_equal(x[8], fv[8].astype(np.float64)) and _err(x[:8]) * 100 <= _err(fv[:8])
    # a side without mesh: the two scores exist before and after; whether their mean fell is the guard's to say
    ov, of = R.open_cube()
    x, its = R.fit_ref(ov, of, cl, 4)
    before, after = (SR.score_ref(m[of].astype(np.float32), cl[:, :3])["scores"][:2] for m in (ov, x))
    print(f"open cube through (a): paired {its[0][0]:.3f}, scores {before} -> {after}")
    assert np.isfinite(before).all() and np.isfinite(after).all() and 0 < its[0][0] < 1
