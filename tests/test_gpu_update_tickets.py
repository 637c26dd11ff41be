"""The TSDF update's work distribution (kernels_tsdf.hip: tsdf_update_pairs_kernel) on a grid whose launch has more workgroups
than the chip holds at once, against the C oracle bit for bit.  Every wave starts on the static list entry of its place in the
launch and goes on by ticket; the workgroups the chip cannot hold start one by one as waves retire.  A brick handed out twice or
not at all changes integer sums, so the equal grid says that every list entry was handed out exactly once.  The small-grid tests
never launch more workgroups than fit; only the 512^3 headline-shape test did.

Shape: 24 x 24 x 24 bricks (192 x 192 x 192 voxels, 13 824 bricks, 3456 workgroups) on a part of 256 CUs, which holds 2048
workgroups of the kernel (8 per CU); more slabs of bricks on a larger part.  Frames of 160 x 120 pixels: fronto-parallel walls,
frame f's wall through the middle of slab f of bricks (24 x 24 bricks), so a batch of 1 / 2 / 32 frames lists one slab, two
slabs, every brick.  L = the length of the batch list (counting mode: stats()["tsdf_batch_bricks"]), W = 4 x the workgroups of
the launch (a wave each):

  none     L = 0: every pixel out of range; every wave leaves at once
  one      L = 1: a long lens on the middle of one brick
  walls    1 frame: L = 576, 2 frames: L = 1152, far below W (most waves, and every late workgroup, find nothing);
           32 frames: L = every brick = W with the shipped library (a wave per entry, the late workgroups' entries live, no ticket);
           with 9 workgroups per CU (the experiments flavour of the library in a child process) L > W = 9216: tickets run
           and the late workgroups meet a live list, and with 1 frame they meet a list that is used up

each with batches of 1, 2 and 32 frames, f32 and 16-bit frames, dense and sparse layout; three passes into a grid that is reset
in between (classify, replay + refine, replay) and a fourth in counting mode, which reads L."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import tl3d
from oracle import c_oracle

from test_gpu_update_groups import _with_env

W_PX, H_PX = 160, 120
VOXEL, TRUNC = 1.0 / 64, 2.0 / 64
MIND, MAXD = 0.05, 16.0
Z0 = 1.5
NBXY = 24
SLAB_MM = 125                                   # a brick: 8 voxels of 15.625 mm
WALL_MM = 1562                                  # frame 0's wall: inside slab 0 with its truncation band (1531 .. 1593 of 1500 .. 1625)
I3 = np.eye(3)
CAM_WIDE = dict(fx=60.0, fy=60.0, cx=79.5, cy=59.5)      # sees every brick of every slab
CAM_LONG = dict(fx=4000.0, fy=4000.0, cx=79.5, cy=59.5)  # the image is 6 cm wide at the wall: the middle of one 12.5 cm brick
POSE_WIDE = (I3, np.zeros(3))
POSE_LONG = (I3, np.array([-(0.0 + 0.0625), -(0.0 + 0.0625), 0.0]))   # the optical axis through the centre of brick (12, 12, 0)
RESIDENT_PER_CU = 8                             # workgroups of the update kernel a CU holds (61 vector registers, 256 threads)
CHILD_PER_CU = 9                                # the child's launch: the chip's fill and a ninth on top
KINDS = ("none", "one", "walls")
BATCHES = (1, 2, 32)


def slabs_for(cus):
    """slabs of 24 x 24 bricks so that a wave per brick takes at least half as many workgroups again as the chip holds"""
    need = RESIDENT_PER_CU * cus * 4 * 3 // 2
    return max(24, -(-need // (NBXY * NBXY)))


def dims_for(nbz):
    return (8 * NBXY, 8 * NBXY, 8 * nbz)


ORIGIN = (-1.5, -1.5, Z0)


def frames_mm(kind, n, nbz):
    """whole millimetres (a 16-bit twin exists)"""
    if kind == "none":
        return [np.zeros((H_PX, W_PX), np.int32) for _ in range(n)]
    if kind == "one":
        return [np.full((H_PX, W_PX), WALL_MM, np.int32) for _ in range(n)]
    return [np.full((H_PX, W_PX), WALL_MM + SLAB_MM * (f % nbz), np.int32) for f in range(n)]


def as_f32(mm):
    return (mm.astype(np.float32) / np.float32(1000.0)).astype(np.float32)          # as a 16-bit upload is converted


def cam_of(kind):
    return (CAM_LONG, POSE_LONG) if kind == "one" else (CAM_WIDE, POSE_WIDE)


@functools.lru_cache(maxsize=None)
def oracle_grid(kind, n, nbz):
    """one pass of the batch into an empty grid; shared by every test that needs it, never written to"""
    cam, pose = cam_of(kind)
    orc = c_oracle.Oracle(W_PX, H_PX, cam["fx"], cam["fy"], cam["cx"], cam["cy"], min_depth=MIND, max_depth=MAXD, dims=dims_for(nbz),
                          origin=ORIGIN, voxel_size=VOXEL, sdf_trunc=TRUNC)
    for mm in frames_mm(kind, n, nbz):
        orc.tsdf_integrate(as_f32(mm), *pose, 1.0)
    out = orc.tsdf.copy()
    out.setflags(write=False)
    return out


def surface_bricks(grid):
    """bricks with a record between the walls' truncation bands' ends (updated, and not all of its updates tsdf == 1): each of them is
    on the batch list, whatever the classification's margins"""
    g = grid.reshape(-1, 512, 2).astype(np.int64)
    return int(((g[..., 1] > 0) & (g[..., 0] != 32767 * g[..., 1])).any(axis=1).sum())


# ---- on the CPU, with the oracle alone: the walls reach the brick counts the cases are named for (the 256-CU shape) ---------------
def test_the_walls_reach_the_intended_brick_counts():
    nbz = slabs_for(256)
    assert nbz == 24 and (NBXY * NBXY * nbz + 3) // 4 == 3456 > RESIDENT_PER_CU * 256
    assert not oracle_grid("none", 2, nbz).any()
    assert surface_bricks(oracle_grid("one", 1, nbz)) == 1
    assert surface_bricks(oracle_grid("walls", 1, nbz)) == NBXY * NBXY
    assert surface_bricks(oracle_grid("walls", 2, nbz)) == 2 * NBXY * NBXY
    every = surface_bricks(oracle_grid("walls", 32, nbz))
    assert every == NBXY * NBXY * nbz > 4 * CHILD_PER_CU * 256


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _ctx(kind, n, nbz, sparse, blocks=None):
    cam, _ = cam_of(kind)
    nbricks = NBXY * NBXY * nbz
    spec = tl3d.GridSpec(dims_for(nbz), ORIGIN, VOXEL, TRUNC, tl3d.CH_TSDF, pool_tsdf=nbricks if sparse else 0)
    env = {"TL3D_CLASS_CACHE": None, "TL3D_TILE_CACHE": None, "TL3D_CLASS_CACHE_ENTRIES": None, "TL3D_CLASS_REFINE": None,
           "TL3D_UPDATE_BLOCKS": None if blocks is None else str(blocks)}
    return _with_env(env, lambda: tl3d.FusionContext(W_PX, H_PX, cam["fx"], cam["fy"], cam["cx"], cam["cy"], min_depth=MIND, max_depth=MAXD,
                                                     n_slots=n, grid=spec))


def run_case(kind, n, u16, sparse, nbz, want, blocks=None):
    """three passes into a grid reset in between, then one in counting mode; returns L"""
    _, pose = cam_of(kind)
    slots, poses = list(range(n)), [pose] * n
    with _ctx(kind, n, nbz, sparse, blocks) as ctx:
        for i, mm in enumerate(frames_mm(kind, n, nbz)):
            ctx.upload(i, mm.astype(np.uint16) if u16 else as_f32(mm))
        for k in range(3):
            ctx.fuse_frames(slots, poses)
            got = ctx.download_grid(tl3d.CH_TSDF)
            assert np.array_equal(got, want), (kind, n, u16, sparse, blocks, "pass", k, int((got != want).any(axis=-1).sum()))
            ctx.reset()
        ctx.reset_stats()
        ctx.set_profile(count_records=True)
        ctx.fuse_frames(slots, poses)
        got = ctx.download_grid(tl3d.CH_TSDF)
        assert np.array_equal(got, want), (kind, n, u16, sparse, blocks, "counting", int((got != want).any(axis=-1).sum()))
        st = ctx.stats()
        assert st["tsdf_launches"] == 1, st
        return int(st["tsdf_batch_bricks"])


def intended(kind, n, nbz, L, waves):
    """where the case means L to fall against the waves of the launch"""
    slab = NBXY * NBXY
    if kind == "none":
        return L == 0
    if kind == "one":
        return L == 1
    lo = slab * min(n, nbz)                     # the bricks the walls cut are listed; the margins of the classification may add neighbours
    if n <= 2:
        return lo <= L <= 2 * lo and 4 * L < waves
    return L == slab * nbz and L >= waves


@pytest.mark.gpu
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_more_workgroups_than_the_chip_holds(kind, n, u16, sparse):
    nbz = slabs_for(_cus())
    blocks = (NBXY * NBXY * nbz + 3) // 4
    assert RESIDENT_PER_CU * _cus() < blocks <= 32 * _cus(), "the launch must exceed the chip's fill and be a wave per brick"
    L = run_case(kind, n, u16, sparse, nbz, oracle_grid(kind, n, nbz))
    assert intended(kind, n, nbz, L, 4 * blocks), (kind, n, L, 4 * blocks)


CHILD_CASES = [("walls", 32, False, False), ("walls", 32, True, True), ("walls", 1, False, True), ("walls", 2, True, False),
               ("one", 2, False, False), ("none", 1, True, True)]


@pytest.mark.gpu
def test_tickets_run_and_late_workgroups_meet_a_live_and_a_used_up_list(tmp_path):
    """Nine workgroups per CU: the number is a knob of the experiments flavour of the library (TL3D_UPDATE_BLOCKS, read when the
    context is created), so the cases run in one child process that loads that flavour -- the same kernel source."""
    cus = _cus()
    nbz = slabs_for(cus)
    np.save(tmp_path / "walls_32.npy", oracle_grid("walls", 32, nbz))          # the dear one: computed once, here
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exp = os.path.join(root, "textureless-3d-reconstruction_amd", "libtl3d_exp.so")
    if not os.path.exists(exp):
        subprocess.check_call(["bash", os.path.join(root, "textureless-3d-reconstruction_amd", "csrc", "build.sh")],
                              env=dict(os.environ, TL3D_FLAVOUR="experiments"))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_update_tickets as t; t._child(%r, %d, %d)" % (
        root, os.path.join(root, "tests"), str(tmp_path), nbz, CHILD_PER_CU * cus)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, TL3D_LIB=exp), timeout=300)
    assert r.returncode == 0 and "tickets ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


def _child(folder, nbz, blocks):
    assert blocks < (NBXY * NBXY * nbz + 3) // 4
    for kind, n, u16, sparse in CHILD_CASES:
        want = np.load(os.path.join(folder, "walls_32.npy")) if (kind, n) == ("walls", 32) else oracle_grid(kind, n, nbz)
        L = run_case(kind, n, u16, sparse, nbz, want, blocks=blocks)
        print(kind, n, u16, sparse, "L", L, "waves", 4 * blocks)
        if kind == "walls" and n == 32:
            assert L == NBXY * NBXY * nbz > 4 * blocks, (L, blocks)          # tickets run; the ninth workgroup of a CU starts on a live entry
        else:
            assert intended(kind, n, nbz, L, 4 * blocks), (kind, n, L)       # ... and here on an entry beyond the list
    print("tickets ok")
