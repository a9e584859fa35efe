"""Generate csrc/mc_table.hpp: the 256-case marching-cubes triangle table of the watertight remeshing step (csrc/watertight.hpp).

    python scripts/gen_mc_table.py            # rewrites meshanything_amd/csrc/mc_table.hpp
    python scripts/gen_mc_table.py --check    # exits 1 if the committed file differs from what this script makes

Conventions (the kernel and tests/watertight_ref.py read them from the library through ma_mc_table()):

* corner c of a cell sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) from the cell's origin grid point; bit c of the cube index is
  set when that corner's value is >= level ("above").
* edge e = (corner offset dx, dy, dz, axis) joins that corner to the next one along `axis`; the edge's vertex belongs to the grid
  point at the corner (each grid point owns its +x, +y and +z edges).  Edges are numbered by axis, then by corner index.
* Each cube face is cut into oriented segments between its crossing edges.  A face whose four corners alternate above / below
  (ambiguous) is resolved by one rule that depends on that face's corners only, so both cells that share it draw the same
  segments: the above-level corners are cut off one by one (the below-level corners stay connected across the face).
* Segments run with the above-level corners on their left, seen from outside the cell.  The segments of a case form closed loops;
  each loop is triangulated in loop order, which makes every triangle's normal (b - a) x (c - a) point toward increasing values
  (scikit-image's gradient_direction='descent'), and no triangulation diagonal joins two vertices of one face, so the diagonals
  of neighbouring cells never coincide.  Together: the output of a field whose border is above level is a closed, consistently
  oriented surface (every directed edge once, every undirected edge in exactly two triangles).
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "meshanything_amd", "csrc", "mc_table.hpp")


def corner_pos(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=float)


def edges():
    """12 edges (corner, axis), ordered by axis, then by corner index."""
    out = []
    for axis in range(3):
        for c in range(8):
            if not (c >> axis) & 1:
                out.append((c, axis))
    return out


EDGES = edges()


def edge_corners(e):
    c, axis = EDGES[e]
    return c, c | (1 << axis)


def faces():
    """6 faces: (axis, side, corners in cyclic order, edges of the face)."""
    out = []
    for axis in range(3):
        for side in range(2):
            cs = [c for c in range(8) if ((c >> axis) & 1) == side]
            u, v = [a for a in range(3) if a != axis]
            # cyclic order around the face: (0,0) (1,0) (1,1) (0,1) in the (u, v) plane
            ring = []
            for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                ring.append(next(c for c in cs if ((c >> u) & 1) == du and ((c >> v) & 1) == dv))
            fe = [e for e in range(12) if set(edge_corners(e)) <= set(cs)]
            out.append((axis, side, ring, fe))
    return out


FACES = faces()


def edge_between(a, b):
    return next(e for e in range(12) if set(edge_corners(e)) == {a, b})


def mid(e):
    a, b = edge_corners(e)
    return 0.5 * (corner_pos(a) + corner_pos(b))


def face_segments(case, face):
    axis, side, ring, _ = face
    above = [bool((case >> c) & 1) for c in ring]
    n = np.zeros(3)
    n[axis] = 1.0 if side else -1.0
    cross = [edge_between(ring[i], ring[(i + 1) % 4]) for i in range(4) if above[i] != above[(i + 1) % 4]]
    pairs = []
    if len(cross) == 2:
        pairs.append((cross[0], cross[1], [ring[i] for i in range(4) if above[i]]))
    elif len(cross) == 4:                   # ambiguous: cut off each above-level corner on its own
        for i in range(4):
            if above[i]:
                pairs.append((edge_between(ring[i], ring[(i - 1) % 4]), edge_between(ring[i], ring[(i + 1) % 4]), [ring[i]]))
    segs = []
    for p, q, ups in pairs:
        t = mid(q) - mid(p)
        left = np.cross(n, t)
        s = np.dot(left, corner_pos(ups[0]) - mid(p))
        assert abs(s) > 1e-9
        segs.append((p, q) if s > 0 else (q, p))
    return segs


def cofacial(a, b):
    return any(a in f[3] and b in f[3] for f in FACES)


def triangulate(loop, segset):
    """Triangles of a polygon (vertex list in loop order) whose diagonals never join two vertices of one face."""
    n = len(loop)
    if n == 3:
        return [tuple(loop)]

    def ok(a, b):
        return (a, b) in segset or (b, a) in segset or not cofacial(a, b)

    # base edge loop[0] -> loop[1], apex loop[k]; sub-polygons loop[1..k] and loop[k..n-1] + loop[0]
    for k in range(2, n):
        a, b, c = loop[0], loop[1], loop[k]
        if k > 2 and not ok(b, c):
            continue
        if k < n - 1 and not ok(c, a):
            continue
        try:
            left = triangulate(loop[1:k + 1], segset | {(b, c)}) if k > 2 else []
            right = triangulate(loop[k:] + [loop[0]], segset | {(c, a)}) if k < n - 1 else []
        except ValueError:
            continue
        return [(a, b, c)] + left + right
    raise ValueError("no valid triangulation")


def case_triangles(case):
    segs = [s for f in FACES for s in face_segments(case, f)]
    nxt = {}
    for p, q in segs:
        assert p not in nxt
        nxt[p] = q
    assert sorted(nxt) == sorted(nxt.values())
    seen, tris = set(), []
    segset = set(segs)
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        # try every rotation: the first that triangulates wins (rotation 0 nearly always does)
        for r in range(len(loop)):
            try:
                tris += triangulate(loop[r:] + loop[:r], segset)
                break
            except ValueError:
                continue
        else:
            raise AssertionError(f"case {case}: loop {loop} cannot be triangulated")
    return tris


def make():
    table = [case_triangles(c) for c in range(256)]
    max_tris = max(len(t) for t in table)
    lines = [
        "// GENERATED by scripts/gen_mc_table.py -- do not edit; rerun the script instead.",
        "// Marching-cubes triangle table of the watertight remeshing step (conventions: the script's header).",
        "#pragma once",
        "#include <cstdint>",
        "#include <hip/hip_runtime.h>",
        "",
        "namespace ma {",
        "namespace wt {",
        "",
        f"constexpr int MC_MAX_TRIS = {max_tris};",
        "// edge e: (corner dx, corner dy, corner dz, axis); the edge's vertex belongs to that corner's grid point",
        "#define MA_MC_EDGES_INIT {" + ", ".join("{%d, %d, %d, %d}" % (c & 1, (c >> 1) & 1, (c >> 2) & 1, a) for c, a in EDGES) + "}",
        "// number of triangles of case `cube index`",
        "#define MA_MC_NTRIS_INIT {" + ", ".join(str(len(t)) for t in table) + "}",
        "// triangles of case `cube index` as edge ids, -1 padded",
        "#define MA_MC_TRIS_INIT { \\",
    ]
    for c, t in enumerate(table):
        flat = [e for tri in t for e in tri] + [-1] * (3 * max_tris - 3 * len(t))
        lines.append("    {" + ", ".join(str(x) for x in flat) + "}, \\")
    lines += ["}", "",
              "// one table, two copies of it: the host's (ma_mc_table) and the kernels' (constant memory)",
              "static const int8_t MC_EDGES_HOST[12][4] = MA_MC_EDGES_INIT;",
              "static const int8_t MC_TRIS_HOST[256][3 * MC_MAX_TRIS] = MA_MC_TRIS_INIT;",
              "__constant__ int8_t MC_EDGES[12][4] = MA_MC_EDGES_INIT;",
              "__constant__ uint8_t MC_NTRIS[256] = MA_MC_NTRIS_INIT;",
              "__constant__ int8_t MC_TRIS[256][3 * MC_MAX_TRIS] = MA_MC_TRIS_INIT;",
              ]
    lines += ["", "}  // namespace wt", "}  // namespace ma", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    text = make()
    if "--check" in sys.argv:
        same = open(OUT).read() == text
        print("up to date" if same else f"{OUT} differs from the generator's output")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {OUT}")
