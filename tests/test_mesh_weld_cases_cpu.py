"""CPU: the crafted cases of the mesh weld (tests/mesh_weld_common.py) against the host weld, the conditions that keep them honest,
and everything of the device weld that needs no GPU: the argument checks of tl3d_mesh_weld_keyed, the
binding's structure, the configuration and command-line refusals, and where the fusion body calls FusionContext.weld_meshes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import keytab_common as kt
import mesh_weld_common as mw
from tl3d import _cabi as abi
from tl3d import pipeline as pl
from tl3d.config import ReconstructionConfig
from tl3d.fusion import GridSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", mw.CASES)
def test_constructed_result_is_the_host_welds(name):
    L, parts, want, _info = mw.case(name)
    assert mw.same_bytes(pl.weld_meshes(parts, L), want)


@pytest.mark.parametrize("name", mw.SOUPS + ("sized",))
def test_cases_have_what_they_are_for(name):
    L, parts, want, info = mw.case(name)
    kept = len(want[0])
    assert sum(len(p[0]) for p in parts) > kept                              # halo copies exist
    named = np.zeros(kept, bool)
    named[want[2].reshape(-1).astype(np.int64)] = True
    assert (~named).sum() >= 1                                               # a kept vertex no triangle names
    if name in mw.SOUPS:
        for p, owner in enumerate(info["corner_owner"]):
            assert (owner != p).sum() >= 100, (name, p)                      # halo corners ...
            if p > 0:
                assert (owner < p).sum() >= 1, (name, p)                     # ... pointing to earlier ...
            if p < len(parts) - 1:
                assert (owner > p).sum() >= 1, (name, p)                     # ... and to later parts
    else:
        sizes = [(int((info["part"][info["order"]] == p).sum()), len(parts[p][0]), len(parts[p][2])) for p in range(len(parts))]
        assert sizes == [(o, o + h, t) for o, h, t in mw.SIZED]
        assert np.all(info["corner_owner"][3] != 3) and parts[4][2].tolist() == [[0, 0, 0]]


def test_wrap_case_fills_the_smallest_table_to_half_with_chains_that_wrap():
    """the two conditions that keep the case from going hollow, by the Python copy of the mixer and of the sizing rule"""
    L, parts, want, info = mw.case("wrap")
    keys = want[3]
    assert len(keys) == len(np.unique(keys)) == mw.WRAP_KEPT == 512 and keys.min() >= 0 and keys.max() < 3 * L[0] * L[1] * L[2]
    assert kt.kt_slots(len(keys)) == 1024 and kt.kt_slots(len(keys) + 1) == 2048      # exactly half of the smallest table
    assert kt.start_slot(keys, 1024).min() >= 1016                                    # more keys than slots to the end: every chain wraps
    assert [int((info["part"][info["order"]] == p).sum()) for p in (0, 1)] == [512, 0]          # part 1 owns nothing ...
    assert len(parts[1][0]) == 512 and np.array_equal(np.sort(parts[1][3]), np.sort(keys))      # ... lists a halo copy of every key ...
    assert np.array_equal(np.unique(parts[1][2]), np.arange(512)) and np.all(info["corner_owner"][1] == 0)     # ... and names each
    assert np.all(info["corner_owner"][0] == 0) and len(parts[0][2]) > 0


def test_host_weld_refuses_the_broken_cases_with_both_messages():
    L, parts, _want, _info = mw.case("soup_small")
    x, r, t, k, lo, hi = parts[0]
    own = mw.owner_part(k, L, [(lo, hi)]) == 0
    v = int(np.flatnonzero(own)[0])
    twice = (np.concatenate([x, x[v:v + 1]]), np.concatenate([r, r[v:v + 1]]), t, np.concatenate([k, k[v:v + 1]]), lo, hi)
    with pytest.raises(ValueError, match="owned by two block cores"):
        pl.weld_meshes([twice] + parts[1:], L)
    with pytest.raises(ValueError, match="references a vertex no block core owns"):
        pl.weld_meshes(parts[:-1], L)


# ---- the raw ABI: every refusal that is decided before any device call, the null ctx last ----------------------------------------

def _raw(parts, L, **kw):
    """tl3d_mesh_weld_keyed on host arrays with a NULL ctx: (code, message)"""
    return mw.raw_call(None, parts, L, **kw)[:2]


def test_raw_abi_refusals_and_the_null_ctx_last():
    L, parts, _want = mw.seam_case()
    assert _raw(parts, L) == (abi.E_INVALID, "null ctx")                     # everything else is in order
    lib = abi.load()
    rc, msg = _raw(parts, None)
    assert rc == abi.E_INVALID and msg == "null argument"
    rc, msg = _raw(parts, L, counts=False)
    assert rc == abi.E_INVALID and msg == "null argument"
    c = C.c_int64(0)
    assert lib.tl3d_mesh_weld_keyed(None, None, 2, (C.c_int64 * 3)(16, 8, 8), None, None, None, 0, None, 0, C.byref(c), C.byref(c), C.byref(c),
                                    C.byref(c)) == abi.E_INVALID and lib.tl3d_last_error() == b"null argument"
    rc, msg = _raw(parts, L, n_parts=-1)
    assert rc == abi.E_INVALID and "n_parts -1 is negative" in msg
    for kw in (dict(vert_cap=-1), dict(tri_cap=-1)):
        rc, msg = _raw(parts, L, **kw)
        assert rc == abi.E_INVALID and msg == "negative capacity"

    def setter(field, value, part=1):
        def fix(arr):
            setattr(arr[part], field, value)
        return fix
    for field, value, text in (("n_vert", -1, "negative size"), ("n_tri", -1, "negative size"), ("n_vert", 1 << 31, "fewer than 2^31 vertices"),
                               ("n_tri", 1 << 32, "fewer than 2^32 triangles"), ("xyz_hd", None, "null argument"),
                               ("key_hd", None, "null argument"), ("tri_hd", None, "null argument"),
                               ("rgb_hd", None, "rgb given in some parts only")):
        rc, msg = _raw(parts, L, fix=setter(field, value))
        assert rc == abi.E_INVALID and text in msg, (field, value, msg)

    def many_triangles(arr):                                                 # each part below 2^32, the sum not
        arr[0].n_tri = arr[1].n_tri = 1 << 31
    rc, msg = _raw(parts, L, fix=many_triangles)
    assert rc == abi.E_INVALID and "fewer than 2^32 triangles" in msg and "in all" in msg
    for dims, text in (((16, 0, 8), "lattice of 0 voxels on axis 1"), ((16, 8, -8), "lattice of -8 voxels on axis 2"),
                       ((1 << 21, 1 << 20, 1 << 20), "2^61 voxels or more"), ((1 << 62, 1 << 62, 1 << 62), "2^61 voxels or more")):
        rc, msg = _raw(parts, dims)
        assert rc == abi.E_INVALID and text in msg, (dims, msg)
    assert _raw([p[:4] + ((0, 0, 0), (1 << 21, 1 << 20, (1 << 20) - 8)) for p in parts], (1 << 21, 1 << 20, (1 << 20) - 8))[1] == "null ctx"
    for lo, hi in (((-1, 0, 0), (8, 8, 8)), ((0, 5, 0), (8, 4, 8)), ((0, 0, 0), (8, 8, 9)), ((0, 0, 0), (17, 8, 8))):
        rc, msg = _raw([parts[0][:4] + (lo, hi), parts[1]], L)
        assert rc == abi.E_INVALID and "must be a range within the lattice" in msg, (lo, hi, msg)
    assert _raw([parts[0][:4] + ((3, 3, 3), (3, 8, 8)), parts[1]], L)[1] == "null ctx"          # an empty core, no multiple of 8
    assert _raw([p[:1] + (None,) + p[2:] for p in parts], L)[1] == "null ctx"                   # no rgb anywhere
    # an output that overlaps an input
    x, r, t, k = (np.ascontiguousarray(a) for a in parts[0][:4])
    nv, nt = 8, 2
    fresh = (np.empty((nv, 3), np.float32), np.empty((nv, 3), np.uint8), np.empty(nv, np.int64), np.empty((nt, 3), np.uint32))
    for slot, a in ((0, x), (1, r), (2, k), (3, t)):
        outs = list(fresh)
        outs[slot] = a
        rc, msg = _raw([(x, r, t, k) + parts[0][4:], parts[1]], L, outs=tuple(outs))
        assert rc == abi.E_INVALID and "an output aliases an input" in msg, (slot, msg)
    # a null output with a capacity
    rc, msg = _raw(parts, L, outs=(None,) + fresh[1:], vert_cap=nv, tri_cap=nt)
    assert rc == abi.E_INVALID and msg == "null output with a capacity"
    rc, msg = _raw(parts, L, outs=(fresh[0], None) + fresh[2:], vert_cap=nv, tri_cap=nt)
    assert rc == abi.E_INVALID and msg == "null output with a capacity"
    assert _raw(parts, L, outs=(fresh[0], fresh[1], None, fresh[3]), vert_cap=nv, tri_cap=nt)[1] == "null ctx"       # out_key may be NULL
    # nothing to weld still wants a context
    assert _raw([], L) == (abi.E_INVALID, "null ctx")


def test_mesh_part_matches_the_header():
    with open(os.path.join(ROOT, "include", "tl3d.h")) as f:
        m = re.search(r"typedef struct tl3d_mesh_part \{(.*?)\} tl3d_mesh_part;", f.read(), re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            tail = re.sub(r"^(const\s+)?\w+\s+", "", decl)                   # the declarators behind the type
            fields += [re.sub(r"[\*\[\]0-9 ]", "", n) for n in tail.split(",")]
    assert fields == [f for f, _ in abi.MeshPart._fields_]
    assert C.sizeof(abi.MeshPart) == 6 * 8 + 6 * 8 and abi.MeshPart.core_lo.offset == 48
    assert "tl3d_mesh_weld_keyed" in abi.SYMBOLS and hasattr(abi.load(), "tl3d_mesh_weld_keyed")


# ---- configuration, command line --------------------------------------------------------------------------------------------------

def test_config_and_command_line_refusals(capsys):
    assert ReconstructionConfig().mesh_weld == "host"
    for cfg, text in ((dict(mesh_weld="gpu", extract_mesh=True), "must be 'host' or 'device'"),
                      (dict(mesh_weld="device"), "needs extract_mesh")):
        with pytest.raises(ValueError, match=text):
            pl.DepthToReconstructionPipeline(ReconstructionConfig(**cfg)).reconstruct()
    import depth_to_reconstruction as cli
    with pytest.raises(SystemExit):
        cli.main(["--rgb-folder", "a", "--depth-folder", "b", "--mesh-weld", "device"])
    assert "--mesh-weld device welds the mesh: it needs --mesh-output" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["--rgb-folder", "a", "--depth-folder", "b", "--mesh-output", "m.ply", "--mesh-weld", "gpu"])
    assert "invalid choice" in capsys.readouterr().err


# ---- the fusion body with a recording stand-in for FusionContext -----------------------------------------------------------------

class _Recorder:
    """Logs (method, args, kwargs).  Every block has one triangle on three vertices its own core owns; weld_meshes answers with the
    host weld of what it was given."""

    def __init__(self):
        self.log, self.grid, self.core, self.fused = [], None, None, 0

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*a, **k):
            self.log.append((name, a, k))
            answer = getattr(type(self), "_" + name, None)
            return answer(self, *a, **k) if answer else None
        return call

    def _attach_grid(self, grid):
        self.grid = grid

    def _set_block_core(self, lattice_dims, lo, hi):
        self.core = (lattice_dims, lo, hi)

    def _fuse_frames(self, *a, **k):
        self.fused += 1

    def _stats(self):
        return dict(centroid_points=1, centroid_dropped=1, pool_slots_tsdf=0, pool_slots_centroid=0, pool_refused=0)

    def _extract(self, *a, **k):
        return np.full((2, 3), self.fused, np.float32), np.full((2, 3), self.fused, np.uint8)

    def _extract_mesh(self, min_weight=0, keys=False):
        assert keys
        L, off = self.core[0], np.asarray(self.grid.voxel_offset) + np.asarray(self.core[1])
        return (np.arange(9, dtype=np.float32).reshape(3, 3) + 100 * self.fused, np.full((3, 3), self.fused, np.uint8),
                np.array([[2, 0, 1]], np.uint32), np.array([mw.key_of(*off, axis, L) for axis in range(3)], np.int64))

    def _statistical_outlier(self, xyz, *a, **k):
        return np.ones(len(xyz), bool)

    def _weld_meshes(self, parts, lattice_dims):
        return pl.weld_meshes(parts, lattice_dims)


_LATTICE = GridSpec((256, 200, 96), (0.0, 0.0, 0.0), 0.01, 0.04)


def _run(monkeypatch, **cfg):
    monkeypatch.setattr(pl, "device_free_bytes", lambda device: 1 << 40)
    pipe = pl.DepthToReconstructionPipeline(ReconstructionConfig(extract_mesh=True, **cfg))
    pipe.frame_index, pipe.scales, pipe.image_names = [0, 1], [1.0, 1.0], ["a.png", "b.png"]
    pipe.camera_poses = [(np.eye(3), np.zeros((3, 1)))] * 2
    ctx, blocks = _Recorder(), pl.plan_blocks(_LATTICE, 136 ** 3)
    assert len(blocks) == 3
    pipe._fuse_blocks(ctx, _LATTICE, blocks)
    return pipe, ctx, blocks


def test_fusion_body_welds_on_the_device_once_after_the_last_detach(monkeypatch):
    pipe, ctx, blocks = _run(monkeypatch, mesh_weld="device")
    names = [n for n, _a, _k in ctx.log]
    assert names.count("weld_meshes") == 1
    at = names.index("weld_meshes")
    assert names.count("detach_grid") == 3 and max(i for i, n in enumerate(names) if n == "detach_grid") < at
    parts, dims = ctx.log[at][1]
    assert tuple(dims) == _LATTICE.dims and len(parts) == 3
    for k, (b, part) in enumerate(zip(blocks, parts)):                       # block order, cores in lattice voxels
        off = np.asarray(b.grid.voxel_offset)
        assert np.array_equal(part[4], off + np.asarray(b.lo)) and np.array_equal(part[5], off + np.asarray(b.hi))
        assert part[0][0, 0] == 100 * (k + 1) and len(part) == 6
    assert pipe.stats["mesh_weld"] == dict(parts=3, vertices_in=9, vertices=9, triangles=3)
    assert "mesh_weld_s" in pipe.timings and "mesh_s" in pipe.timings
    host, hctx, _ = _run(monkeypatch)                                        # the default: the host weld, and no new key anywhere
    assert "weld_meshes" not in [n for n, _a, _k in hctx.log]
    assert "mesh_weld" not in host.stats and "mesh_weld_s" not in host.timings
    for a, b in zip(pipe.mesh, host.mesh):
        assert np.array_equal(a, b)


def test_one_block_welds_nothing_in_device_mode(monkeypatch):
    monkeypatch.setattr(pl, "device_free_bytes", lambda device: 1 << 40)
    pipe = pl.DepthToReconstructionPipeline(ReconstructionConfig(extract_mesh=True, mesh_weld="device"))
    pipe.frame_index, pipe.scales, pipe.image_names = [0], [1.0], ["a.png"]
    pipe.camera_poses = [(np.eye(3), np.zeros((3, 1)))]

    class One(_Recorder):
        def _extract_mesh(self, min_weight=0, keys=False):
            assert not keys
            return np.zeros((3, 3), np.float32), np.zeros((3, 3), np.uint8), np.array([[0, 1, 2]], np.uint32)
    ctx = One()
    pipe._fuse_blocks(ctx, _LATTICE, pl.plan_blocks(_LATTICE))
    assert "weld_meshes" not in [n for n, _a, _k in ctx.log] and "mesh_weld" not in pipe.stats
