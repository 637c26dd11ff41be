"""Inputs the quadric placement tests share (CPU and GPU): meshes with known answers (a roof, a cube corner, a tilted plane), the
edge rules' hand-made meshes, the carry case, and the reference results computed once."""
import numpy as np

import mesh_simplify_quadric_reference as mqr
import mesh_simplify_reference as msr
import mesh_simplify_common as msc

NO_TRIS = np.zeros((0, 3), np.uint32)
# Every known-answer mesh lies on the lattice of 1/1024 cell: cell 1 (a power of two), origin 0, coordinates multiples of 1/1024


def _grid_tris(nu, nv, flip=False):
    """the two triangles of every quad of an nu x nv grid whose vertex (a, b) has index a * nv + b"""
    a, b = np.meshgrid(np.arange(nu - 1), np.arange(nv - 1), indexing="ij")
    v = (a * nv + b).reshape(-1)
    t = np.concatenate([np.stack([v, v + nv, v + 1], axis=1), np.stack([v + 1, v + nv, v + nv + 1], axis=1)], axis=1).reshape(-1, 3)
    return t[:, ::-1] if flip else t


ROOFS = ((1.0, 1.0), (0.5, 2.0), (1.0, 0.25))          # slopes left / right of the crease; the first two creases are 90 degrees
ROOF_CREASE = (2.25, 5.5)                               # x and z of the crease line (y is free): a quarter cell from the face x = 2


def roof(slopes):
    """(xyz, tris, cell): a roof over x in [0, 4.5], y in [0, 3] at a spacing of 1/8 cell, z = 5.5 - slope * |x - 2.25|, so the
    crease is a grid line a quarter cell from a cell face"""
    xc, zc = ROOF_CREASE
    x, y = np.arange(37) / 8.0, np.arange(25) / 8.0
    z = zc - np.where(x < xc, slopes[0] * (xc - x), slopes[1] * (x - xc))
    xyz = np.stack([np.repeat(x, len(y)), np.tile(y, len(x)), np.repeat(z, len(y))], axis=1).astype(np.float32)
    assert np.array_equal(xyz.astype(np.float64) * 1024, np.rint(xyz.astype(np.float64) * 1024))
    return xyz, _grid_tris(len(x), len(y)).astype(np.uint32), 1.0


def roof_crease_clusters(xyz, vert_map):
    """the output vertices whose clusters contain crease vertices"""
    return np.unique(vert_map[xyz[:, 0] == np.float32(ROOF_CREASE[0])])


def roof_distance(pos):
    """distance of positions to the crease line, in cells"""
    p = np.asarray(pos, np.float64)
    return np.hypot(p[:, 0] - ROOF_CREASE[0], p[:, 2] - ROOF_CREASE[1])


CORNER = (2.25, 2.25, 2.25)


def cube_corner():
    """(xyz, tris, cell): the three faces that meet in CORNER, each 2 x 2 cells at a spacing of 1/16 cell (the faces do not share
    vertices: the edges and the corner are there two and three times)"""
    g = np.arange(33) / 16.0
    u, v = np.repeat(g, len(g)), np.tile(g, len(g))
    parts, tris = [], []
    for axis in range(3):
        p = np.zeros((len(u), 3))
        p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = u, v
        parts.append(p + np.array(CORNER))
        tris.append(_grid_tris(len(g), len(g)) + axis * len(u))
    return np.concatenate(parts).astype(np.float32), np.concatenate(tris).astype(np.uint32), 1.0


PLANE = (0.25, 0.5, 1.375)                              # z = 0.25 x + 0.5 y + 1.375


def tilted_plane():
    """(xyz, tris, cell): one plane over 3 x 3 cells at a spacing of 1/8 cell"""
    g = np.arange(25) / 8.0 + 0.0625
    x, y = np.repeat(g, len(g)), np.tile(g, len(g))
    xyz = np.stack([x, y, PLANE[0] * x + PLANE[1] * y + PLANE[2]], axis=1).astype(np.float32)
    return xyz, _grid_tris(len(g), len(g)).astype(np.uint32), 1.0


def spans():
    """(xyz, tris, cell): ONE triangle whose corners sit in the cells 0, 3 and 4 along x: the corner in cell 3 sees spans of 3 and 1
    and contributes; the corners in cells 0 and 4 see a span of 4 and are skipped"""
    xyz = np.array([(0.5, 0.25, 0.5), (3.5, 0.75, 0.5), (4.5, 0.25, 0.75)], np.float32)
    return xyz, np.array([(0, 1, 2)], np.uint32), 1.0


def without_area():
    """(xyz, rgb, tris, cell): clusters without a triangle, with a triangle that names a vertex twice, with three collinear vertices
    and with three equal positions: every cluster follows the mean rule"""
    rng = np.random.default_rng(31)
    free = rng.random((40, 3)) * 3.0                                                  # no triangle names these
    line = np.array([(5.125, 0.25, 0.5), (5.375, 0.5, 0.5), (5.875, 1.0, 0.5)])       # collinear, over two cells
    same = np.tile([(7.25, 7.5, 7.75)], (3, 1))
    twice = np.array([(9.25, 0.5, 0.5), (9.75, 0.25, 0.125)])
    xyz = np.concatenate([free, line, same, twice]).astype(np.float32)
    tris = np.array([(40, 41, 42), (43, 44, 45), (46, 47, 46), (46, 46, 46)], np.uint32)
    return xyz, rng.integers(0, 256, size=(len(xyz), 3), dtype=np.uint8), tris, 1.0


def crease_outside():
    """(xyz, tris, cell): cell (0, 0, 0) holds a vertex of the plane z = 0.25 and a vertex of the plane z = 0.5 x + 0.5; the planes
    meet in x = -0.5, half a cell outside: the solve is clamped to x = 0"""
    xyz = np.array([(0.5, 0.25, 0.25), (1.5, 0.25, 0.25), (0.5, 1.25, 0.25),
                    (0.5, 0.75, 0.75), (1.5, 0.75, 1.25), (0.5, 2.75, 0.75)], np.float32)
    return xyz, np.array([(0, 1, 2), (3, 4, 5)], np.uint32), 1.0


CARRY_TRIS, CARRY_FILL = 4096, 1 << 16


def carry():
    """(xyz, rgb, tris, cell): 4096 triangles with one corner each in cell (0, 0, 0) and the other two 3 cells away: one along two
    axes, one along the third, so the plane runs diagonally past the cell and the foot of the cell's corner on it, which gives
    d N_a its sign, falls on either side.  The terms seen from that cell are about as large as a triangle with a corner in the
    frame's own cell gives (|d N_a| above 2^56; the 2^68 of the rules bounds every triangle the span rule lets through).  Every other triangle is mirrored in the cell's centre and reversed.  The low words of the one record
    wrap thousands of times and the high words of b go negative and come back.  2^16 more vertices in that cell, as the
    contention case of the clustering tests has them."""
    rng = np.random.default_rng(41)
    n, rows = CARRY_TRIS, np.arange(CARRY_TRIS)
    a = rng.integers(64, 1024, size=(n, 3)) / 1024.0                                  # in cell (0, 0, 0)
    axis = rng.integers(0, 3, size=n)
    # (the other corners follow a, up to a jitter: the normal, and with it the weight of a term, does not depend on where a sits)
    b, c = a - rng.integers(0, 64, size=(n, 3)) / 1024.0, a - rng.integers(0, 64, size=(n, 3)) / 1024.0
    b[rows, axis] += 3.0
    b[rows, (axis + 1) % 3] += 3.0
    c[rows, (axis + 2) % 3] += 3.0
    tri_xyz = np.stack([a, b, c], axis=1)                                             # [n, 3, 3]
    odd = rows % 2 == 1
    tri_xyz[odd] = (1023.0 / 1024.0 - tri_xyz[odd])[:, ::-1]                          # mirrored (corner a stays in the cell), reversed
    fill = (0.25 + 0.5 * rng.random((CARRY_FILL, 3)))
    xyz = np.concatenate([tri_xyz.reshape(-1, 3), fill]).astype(np.float32)
    tris = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    return xyz, rng.integers(0, 256, size=(len(xyz), 3), dtype=np.uint8), tris, 1.0


_REFERENCES = {}


def reference(name):
    """((xyz, rgb, tris, cell, origin), quadric reference, mean reference) of a named case, computed once and shared (read-only).
    Names: "roof 0" .. "roof 2", "corner", "plane", "spans", "without area", "crease outside", "carry", or a topology of
    mesh_simplify_common."""
    if name not in _REFERENCES:
        if name.startswith("roof "):
            xyz, tris, cell = roof(ROOFS[int(name.split()[1])])
            inp = (xyz, None, tris, cell, None)
        elif name in ("corner", "plane", "spans", "crease outside"):
            xyz, tris, cell = {"corner": cube_corner, "plane": tilted_plane, "spans": spans, "crease outside": crease_outside}[name]()
            inp = (xyz, None, tris, cell, None)
        elif name in ("without area", "carry"):
            inp = (without_area if name == "without area" else carry)() + (None,)
        else:
            inp, mean = msc.reference(name)                         # (shared with the clustering tests)
        if name not in msc.TOPOLOGIES + msc.WRAPPED:
            mean = msr.simplify(*inp)
        want = mqr.simplify(*inp, mean=mean)
        for a in inp[:3] + want[:3] + mean[:3] + (want[3]["vert_map"],):
            if a is not None:
                a.setflags(write=False)
        _REFERENCES[name] = (inp, want, mean)
    return _REFERENCES[name]
