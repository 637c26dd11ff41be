#!/usr/bin/env python3
"""Generates mc_tables.h: the marching-cubes triangulation of tl3d_extract_mesh.

Cube corners: corner c sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) from the cell's lowest voxel; case bit c is set
when corner c is inside (t < 0).  Edge e = 4 * axis + q runs along `axis` from its lower corner, whose two other offsets are
(q & 1, q >> 1) in axis order (x edges: q = y | z << 1; y edges: q = x | z << 1; z edges: q = x | y << 1).

Method, per case:
  1. On each cube face join the crossing points into segments.  A face with two crossings has one segment; a face with four
     (two diagonal inside corners) always separates the inside corners: one segment cuts off each of them.
  2. Direct every segment so that, seen from outside the cube, the face's inside corners lie to its right.
  3. Chain the directed segments into closed loops: every crossing is the end of exactly one segment and the start of one.
  4. Fan-triangulate each loop.  The direction of step 2 winds every triangle so that (v1 - v0) x (v2 - v0) points to the
     outside (t > 0).  The fan starts at the first loop position whose fan has no triangle lying in one cube face.

Because a face's segments depend only on its four corners, two cells that share a face cut it the same way: closed
surfaces come out without cracks.

Usage: gen_mc_tables.py [OUTPUT]   (default: mc_tables.h next to this script)
"""
import os
import sys

MAX_TRIS = 10                 # a cell has at most 12 crossings

# face: (axis normal to it, side 0/1) -> its four corners in cyclic order
FACES = []
for _ax in range(3):
    _u, _v = [a for a in range(3) if a != _ax]
    for _side in (0, 1):
        cyc = []
        for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
            cyc.append((_side << _ax) | (du << _u) | (dv << _v))
        FACES.append((_ax, _side, cyc))


def corner_pos(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_of(a, b):
    """edge id joining corners a and b (adjacent)"""
    d = a ^ b
    ax = {1: 0, 2: 1, 4: 2}[d]
    lo = a & b
    o = [a for a in range(3) if a != ax]
    q = ((lo >> o[0]) & 1) | (((lo >> o[1]) & 1) << 1)
    return 4 * ax + q


def edge_corners(e):
    ax, q = divmod(e, 4)
    o = [a for a in range(3) if a != ax]
    lo = ((q & 1) << o[0]) | ((q >> 1) << o[1])
    return lo, lo | (1 << ax)


def edge_mid(e):
    a, b = edge_corners(e)
    pa, pb = corner_pos(a), corner_pos(b)
    return tuple(0.5 * (pa[i] + pb[i]) for i in range(3))


def _sub(p, q):
    return tuple(p[i] - q[i] for i in range(3))


def _cross(p, q):
    return (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])


def _dot(p, q):
    return sum(p[i] * q[i] for i in range(3))


def face_segments(case, face):
    """directed segments (edge, edge) the face rule draws on one face of one case"""
    ax, side, cyc = face
    inside = [bool(case >> c & 1) for c in cyc]
    n_in = sum(inside)
    if n_in in (0, 4):
        return []
    segs = []
    if n_in == 2 and inside[0] == inside[2]:               # ambiguous: cut off each inside corner
        for k in range(4):
            if inside[k]:
                segs.append((cyc[k], [edge_of(cyc[k - 1], cyc[k]), edge_of(cyc[k], cyc[(k + 1) % 4])]))
    else:
        cross = [edge_of(cyc[k], cyc[(k + 1) % 4]) for k in range(4) if inside[k] != inside[(k + 1) % 4]]
        assert len(cross) == 2
        ref = next(cyc[k] for k in range(4) if inside[k])
        segs.append((ref, cross))
    normal = [0, 0, 0]
    normal[ax] = 1 if side else -1
    out = []
    for ref, (e0, e1) in segs:
        p, q = edge_mid(e0), edge_mid(e1)
        s = _dot(_cross(_sub(q, p), _sub(corner_pos(ref), p)), normal)
        assert s != 0
        out.append((e0, e1) if s < 0 else (e1, e0))     # inside corner to the right, seen from outside
    return out


def edge_faces(e):
    a, b = edge_corners(e)
    return {f for f, (_, _, cyc) in enumerate(FACES) if a in cyc and b in cyc}


def case_triangles(case):
    segs = [s for f in FACES for s in face_segments(case, f)]
    nxt = {}
    for a, b in segs:
        assert a not in nxt
        nxt[a] = b
    tris = []
    seen = set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop = [start]
        seen.add(start)
        while nxt[loop[-1]] != start:
            loop.append(nxt[loop[-1]])
            seen.add(loop[-1])
        best = None
        for r in range(len(loop)):
            lp = loop[r:] + loop[:r]
            fan = [(lp[0], lp[i], lp[i + 1]) for i in range(1, len(lp) - 1)]
            if all(not (edge_faces(a) & edge_faces(b) & edge_faces(c)) for a, b, c in fan):
                best = fan
                break
        assert best is not None, (case, loop)
        tris.extend(best)
    assert len(tris) <= MAX_TRIS
    return tris


def build_tables():
    return [case_triangles(c) for c in range(256)]


def render_header(tables):
    width = max(len(t) for t in tables)              # the face rule above never needs more than 5
    lines = [
        "// mc_tables.h -- GENERATED by gen_mc_tables.py; do not edit.  Marching-cubes triangulation of tl3d_extract_mesh.",
        "// Case bit c: corner c = (c & 1, c >> 1 & 1, c >> 2 & 1) is inside (t < 0).  Edge e = 4 * axis + q runs along `axis` from its",
        "// lower corner, whose other two offsets are (q & 1, q >> 1) in axis order.  MC_TRI_EDGES[case] lists the cell's triangles",
        "// as edge triples, wound so that (v1 - v0) x (v2 - v0) points to t > 0; MC_TRI_COUNT[case] triangles are valid.",
        "#pragma once",
        "#include <stdint.h>",
        "",
        "#ifndef MC_CONST",
        "#define MC_CONST static const   // kernels_mesh.hip: static __device__ const",
        "#endif",
        "",
        "#define MC_MAX_TRIS %d" % width,
        "",
        "MC_CONST uint8_t MC_TRI_COUNT[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join("%d" % len(tables[c]) for c in range(r, r + 32)) + ",")
    lines.append("};")
    lines.append("")
    lines.append("MC_CONST uint8_t MC_TRI_EDGES[256][3 * MC_MAX_TRIS] = {")
    for c in range(256):
        flat = [e for t in tables[c] for e in t]
        flat += [255] * (3 * width - len(flat))
        lines.append("    {" + ", ".join("%d" % e for e in flat) + "},   // %d" % c)
    lines.append("};")
    return "\n".join(lines) + "\n"


def main(argv):
    out = argv[1] if len(argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "mc_tables.h")
    text = render_header(build_tables())
    with open(out, "w", newline="\n") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
