"""Inputs of the compaction edge tests (CPU and GPU): the "beads" mesh with exactly T triangles, for the T at which the bounds of the
shared compaction loop (csrc/compact.h: chunks of 2048 elements, walked 256 at a time) can go wrong, with the figures both
references give for it."""
import numpy as np

MIN_TRIANGLES = 2                                       # filter_mesh: the beads of one triangle go
CELL = 0.01                                             # simplify_mesh: every fifth vertex shares its cell with the one before it
# T -> (vertices in, filter: (vertices, triangles) out, simplify: (vertices, triangles, degenerate, duplicate) out)
FIGURES = {1: (3, (0, 0), (3, 1, 0, 0)), 255: (511, (382, 212), (409, 153, 102, 0)), 256: (516, (382, 212), (413, 154, 102, 0)),
           257: (516, (386, 214), (413, 154, 103, 0)), 2047: (4095, (3069, 1705), (3276, 1227, 820, 0)),
           2048: (4099, (3069, 1705), (3280, 1228, 820, 0)), 2049: (4099, (3073, 1707), (3280, 1229, 820, 0)),
           4097: (8196, (6146, 3414), (6557, 2458, 1639, 0))}
SIZES = tuple(sorted(FIGURES))


def beads(n_tri):
    """(xyz f32 [V,3], rgb u8 [V,3], tris u32 [T,3]): bead k is a strip of s = 1 + k % 3 triangles (v + j, v + j + 1, v + j + 2)
    over its own s + 2 vertices; beads are appended until n_tri triangles exist, the last strip cut short (its vertices stay)"""
    tris, v, k = [], 0, 0
    while len(tris) < n_tri:
        s = 1 + k % 3
        tris += [(v + j, v + j + 1, v + j + 2) for j in range(min(s, n_tri - len(tris)))]
        v += s + 2
        k += 1
    j = np.arange(v)
    late = (j % 5 == 4).astype(np.int64)
    xyz = np.stack([(j - late) * 0.01 + 0.005 + late * 0.001, (j % 7) * 0.001, np.zeros(v)], axis=1).astype(np.float32)
    rgb = np.stack([j % 251, j % 241, j % 239], axis=1).astype(np.uint8)
    return xyz, rgb, np.array(tris, np.uint32).reshape(-1, 3)


_REFERENCES = {}


def reference(n_tri):
    """(mesh, filter_mesh result, simplify result) of beads(n_tri) with both references, computed once and shared (read-only)"""
    import mesh_components_reference as mcr
    import mesh_simplify_reference as msr
    if n_tri not in _REFERENCES:
        mesh = beads(n_tri)
        filt = mcr.filter_mesh(*mesh, MIN_TRIANGLES)
        simp = msr.simplify(*mesh, CELL)
        for a in (*mesh, *filt[:3], filt[3]["keep_vert"], *simp[:3], simp[3]["vert_map"]):
            a.setflags(write=False)
        _REFERENCES[n_tri] = (mesh, filt, simp)
    return _REFERENCES[n_tri]


def figures(n_tri):
    """the row of FIGURES as the references give it"""
    mesh, filt, simp = reference(n_tri)
    assert len(mesh[2]) == n_tri
    return (len(mesh[0]), (len(filt[0]), len(filt[2])),
            (len(simp[0]), len(simp[2]), simp[3]["degenerate_dropped"], simp[3]["duplicates_dropped"]))
