"""The rules of the mesh component filter restated with scipy's connected_components.

Two vertices are connected when one triangle names both; a component is a connected set of vertices; label[v] is the smallest
vertex index of v's component; a vertex no triangle names is a component of its own with 0 triangles; a triangle belongs to the
component of its vertices, and (a, a, b) counts as one and connects a and b."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def components(tris, n_vert):
    """(labels u32 [n_vert], counts u32 [n_vert] with a component's triangle count at index = label and 0 elsewhere, n)"""
    n_vert = int(n_vert)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    if n_vert == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0
    rows = np.concatenate([t[:, 0], t[:, 1]])
    cols = np.concatenate([t[:, 1], t[:, 2]])
    graph = coo_matrix((np.ones(len(rows), np.uint8), (rows, cols)), shape=(n_vert, n_vert))
    n, comp = connected_components(graph, directed=False)
    smallest = np.full(n, n_vert, np.int64)
    np.minimum.at(smallest, comp, np.arange(n_vert))              # re-base every component to its smallest vertex index
    labels = smallest[comp]
    counts = np.bincount(labels[t[:, 0]], minlength=n_vert) if len(t) else np.zeros(n_vert, np.int64)
    return labels.astype(np.uint32), counts.astype(np.uint32), int(n)


def filter_mesh(xyz, rgb, tris, min_triangles=0, largest_only=False):
    """(xyz, rgb, tris, info): the kept vertices and re-indexed triangles in their original order; info as
    FusionContext.filter_mesh gives it (components, components_kept, vertices_dropped, triangles_dropped, keep_vert)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    tris = np.asarray(tris, np.uint32).reshape(-1, 3)
    nv = len(xyz)
    labels, counts, n = components(tris, nv)
    roots = np.flatnonzero(labels == np.arange(nv))
    kept = np.ones(len(roots), bool) if min_triangles <= 0 else counts[roots] >= min_triangles
    if largest_only:
        only = np.zeros(len(roots), bool)
        if len(roots) and counts[roots].max() > 0:
            only[np.argmax(counts[roots])] = True                 # the first maximum: ties go to the smaller label
        kept &= only
    keep_label = np.zeros(nv, bool)
    keep_label[roots[kept]] = True
    keep_vert = keep_label[labels] if nv else np.zeros(0, bool)
    keep_tri = keep_vert[tris[:, 0]] if len(tris) else np.zeros(0, bool)
    remap = (np.cumsum(keep_vert) - 1).astype(np.uint32)
    info = dict(components=n, components_kept=int(kept.sum()), vertices_dropped=int(nv - keep_vert.sum()),
                triangles_dropped=int(len(tris) - keep_tri.sum()), keep_vert=keep_vert)
    return xyz[keep_vert], (None if rgb is None else np.asarray(rgb, np.uint8).reshape(-1, 3)[keep_vert]), remap[tris[keep_tri]], info
