"""Inputs the mesh simplification tests share (CPU and GPU): the crafted mesh of the component tests with its pinned figures, the
topologies on which hashed vertex clustering goes wrong, and the speck scene of the component tests."""
import numpy as np

import keytab_common as kt
from mesh_components_common import SPECK_GRID, SPECK_MIN_TRIANGLES, crafted_mesh, speck_scene  # noqa: F401  (shared with the tests)

# crafted_mesh(0): 5135 vertices, 9188 triangles.  By cell size, origin 0: (vertices, triangles, duplicates dropped) out
CRAFTED = {0.01: (3918, 7158, 0), 0.02: (2566, 4567, 0), 0.04: (1003, 1612, 0), 0.05: (762, 1209, 1), 0.16: (92, 134, 1),
           10.0: (4, 4, 0)}
CRAFTED_ORIGIN = (0.0137, -0.271, 1.0 / 3.0)           # no multiple of any cell above


def _lattice(n, step):
    """an n x n plane lattice in z = step / 2 and the two triangles of each of its quads, row by row"""
    g = (np.arange(n, dtype=np.float64) * step).astype(np.float32)
    xyz = np.stack([np.repeat(g, n), np.tile(g, n), np.full(n * n, np.float32(step / 2))], axis=1)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).reshape(-1)
    tris = np.concatenate([np.stack([a, a + n, a + 1], axis=1), np.stack([a + 1, a + n, a + n + 1], axis=1)], axis=1).reshape(-1, 3)
    return np.ascontiguousarray(xyz), tris.astype(np.uint32)


def _colours(rng, n):
    return rng.integers(0, 256, size=(n, 3), dtype=np.uint8)


def _axis_lines(cell):
    """per axis the values f32(k * cell), k = -50..50, and their two f32 neighbours, permuted; the other two coordinates at cell / 2"""
    rng = np.random.default_rng(5)
    v = (np.arange(-50, 51, dtype=np.float64) * cell).astype(np.float32)
    v = np.concatenate([v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))])
    parts = []
    for a in range(3):
        p = np.full((len(v), 3), np.float32(cell / 2), np.float32)
        p[:, a] = rng.permutation(v)
        parts.append(p)
    xyz = np.concatenate(parts)
    ids = rng.permutation(len(xyz)).astype(np.uint32)
    tris = np.stack([ids[:-2], ids[1:-1], ids[2:]], axis=1)
    return xyz, _colours(rng, len(xyz)), np.ascontiguousarray(tris)


WRAPPED = ("wrapped chains", "wrapped chains shared")
WRAPPED_VERTS = 512                                       # n_vert of both: half of the smallest vertex table


def cell_keys(i):
    """ms_key of kernels_meshsimplify.hip for cell indices i [N, 3] within +-2^20"""
    u = (np.asarray(i, np.int64) + (1 << 20)).astype(np.uint64)
    return (u[:, 0] << np.uint64(42)) | (u[:, 1] << np.uint64(21)) | u[:, 2]


def _wrapped_chains(shared):
    """The vertex table at its smallest capacity, every probe sequence running into the end of the array: cells (cell 1, origin 0,
    indices anywhere within +-2^20) whose keys' sequences start in the last 8 of 1024 slots (keytab_common.wrapping).
    "wrapped chains": WRAPPED_VERTS vertices at the centres of as many distinct cells; the table is filled to exactly half.
    "wrapped chains shared": the first half of those cells, and then as many vertices again a quarter cell off the centre of cells
    already taken, which find their key at the end of a wrapped chain.  (The table is sized by n_vert, so vertices that share cells
    cannot come on top of WRAPPED_VERTS distinct ones without doubling it: they take the place of half of them.)
    400 triangles among all vertices.  Every coordinate is a multiple of 1/4 below 2^20: exact in f32."""
    rng = np.random.default_rng(25)

    def draw(rng, count):
        i = rng.integers(-(1 << 20), 1 << 20, size=(count, 3))
        return cell_keys(i), i
    i = kt.wrapping(rng, WRAPPED_VERTS, draw)
    xyz = i + 0.5
    if shared:
        half = WRAPPED_VERTS // 2
        xyz = np.concatenate([xyz[:half], i[rng.integers(0, half, size=half)] + rng.choice([0.25, 0.75], size=(half, 3))])
    xyz = xyz.astype(np.float32)
    tris = rng.integers(0, len(xyz), size=(400, 3)).astype(np.uint32)
    return xyz, _colours(rng, len(xyz)), tris, 1.0, None


def topology(name):
    """(xyz f32 [V,3], rgb u8 [V,3], tris u32 [T,3], cell, origin or None)"""
    if name in WRAPPED:
        return _wrapped_chains(name.endswith("shared"))
    if name == "one hot cluster":                               # every add lands on one record
        rng = np.random.default_rng(21)
        xyz = (0.25 + 0.5 * rng.random((1 << 16, 3))).astype(np.float32)
        tris = rng.integers(0, 1 << 16, size=(1 << 17, 3)).astype(np.uint32)
        return xyz, _colours(rng, len(xyz)), tris, 1.0, None
    if name == "doubled sheet":                                 # the list, the list rotated by one position, the list reversed
        xyz, tris = _lattice(257, 0.01)
        tris = np.concatenate([tris, tris[:, [1, 2, 0]], tris[:, ::-1]])
        return xyz, _colours(np.random.default_rng(22), len(xyz)), np.ascontiguousarray(tris), 0.02, None
    if name == "soup":                                          # long probe chains in both tables, leaders far out of order
        rng = np.random.default_rng(23)
        n, t = 1 << 18, 1 << 19
        xyz = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32)
        xyz[xyz >= 1.0] = np.nextafter(np.float32(1.0), np.float32(0.0))
        box = np.floor((xyz.astype(np.float64) + 1.0) * 4.0).astype(np.int64)          # neighbours: the vertices of one 0.25 m box
        order = np.lexsort((rng.random(n), box[:, 2], box[:, 1], box[:, 0]))          # ids are random within a box and across boxes
        per = n // 512
        base = rng.integers(0, n, size=t)
        lo = np.minimum(base // per * per, n - per)
        tris = np.stack([order[base], order[lo + rng.integers(0, per, size=t)], order[lo + rng.integers(0, per, size=t)]], axis=1)
        return xyz, _colours(rng, n), tris.astype(np.uint32), 1.0 / 16.0, None
    if name.startswith("axis lines"):                           # "axis lines 0.25", "axis lines 0.25 shifted"
        cell = float(name.split()[2])
        xyz, rgb, tris = _axis_lines(cell)
        return xyz, rgb, tris, cell, ((0.3 * cell, -1.7 * cell, 1.0 / 3.0) if name.endswith("shifted") else None)
    if name == "cell finer than the spacing":                   # nothing merges
        xyz, tris = _lattice(65, 0.01)
        return xyz, _colours(np.random.default_rng(24), len(xyz)), tris, 0.001, None
    raise KeyError(name)


AXIS_LINES = tuple(f"axis lines {c}{s}" for c in ("0.25", "0.1", "0.005") for s in ("", " shifted"))
TOPOLOGIES = ("one hot cluster", "doubled sheet", "soup") + AXIS_LINES + ("cell finer than the spacing",)
# (vertices, triangles, degenerate, duplicates) out, with the reference on the CPU (test_mesh_simplify_reference_cpu.py); the soup's
# depend on its generator's draws
FIGURES = {"one hot cluster": (1, 0, 131072, 0), "doubled sheet": (16384, 64516, 296442, 32258), "soup": (32759, 502853, 19714, 1721),
           "axis lines 0.25": (304, 902, 3, 2), "axis lines 0.25 shifted": (301, 902, 3, 2), "axis lines 0.1": (304, 900, 5, 2),
           "axis lines 0.1 shifted": (301, 902, 3, 2), "axis lines 0.005": (304, 899, 5, 3), "axis lines 0.005 shifted": (301, 902, 3, 2),
           "cell finer than the spacing": (4225, 8192, 0, 0), "wrapped chains": (512, 397, 3, 0), "wrapped chains shared": (256, 395, 5, 0)}

_REFERENCES = {}


def reference(name):
    """(inputs, reference result) of a topology, computed once and shared (read-only)"""
    import mesh_simplify_reference as msr
    if name not in _REFERENCES:
        xyz, rgb, tris, cell, origin = topology(name)
        want = msr.simplify(xyz, rgb, tris, cell, origin)
        for a in (xyz, rgb, tris, want[0], want[1], want[2], want[3]["vert_map"]):
            a.setflags(write=False)
        _REFERENCES[name] = ((xyz, rgb, tris, cell, origin), want)
    return _REFERENCES[name]
