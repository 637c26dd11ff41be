"""CPU: the numpy ray caster of tests/raycast_reference.py against analytic answers -- an exactly linear
field (a tilted plane), a truncated sphere, a camera inside a surface, an unobserved slab and the weight gate -- and the
command line's --render-output flag."""
import os
import subprocess
import sys

import numpy as np

import raycast_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = dict(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5)
DIMS, VOXEL = (64, 64, 64), 0.02
ORIGIN = tuple(-0.5 * d * VOXEL for d in DIMS)
TRUNC = 4 * VOXEL
POSE = (np.eye(3), np.array([0.0, 0.0, 2.0]))          # camera at z = -2, looking along +z
NPLANE, EPLANE, SLOPE = np.array([1.0, 2.0, 8.0]), 352.0, 256


def _grid_coords():
    return np.meshgrid(*[np.arange(n) for n in DIMS], indexing="ij")


def plane_volume(weights=None):
    """t = -(i + 2j + 8k - 352) * 256 / 32767 (clipped to +-1): exactly linear inside the band, positive towards the camera"""
    ii, jj, kk = _grid_coords()
    q = np.clip(-(ii + 2 * jj + 8 * kk - int(EPLANE)) * SLOPE, -32767, 32767).astype(np.int64)
    w = np.ones(DIMS, np.int64) if weights is None else weights
    return q * w, w


def _rays(pose):
    R, t = (np.asarray(p, np.float64) for p in pose)
    vv, uu = np.meshgrid(np.arange(CAM["height"]), np.arange(CAM["width"]), indexing="ij")
    dc = np.stack([(uu - CAM["cx"]) / CAM["fx"], (vv - CAM["cy"]) / CAM["fy"], np.ones(uu.shape)], axis=-1)
    C = -R.T @ t
    D = dc @ R                                           # rows: R^T (xf, yf, 1)
    return C, D


def plane_truth(pose):
    """analytic depth and grid-coordinate hit point of every pixel's ray on the plane"""
    C, D = _rays(pose)
    x0 = (C - np.array(ORIGIN)) / VOXEL - 0.5
    dx = D / VOXEL
    z = (EPLANE - x0 @ NPLANE) / (dx @ NPLANE)
    return z, x0 + z[..., None] * dx


def _interior(x, margin):
    return np.all((x >= margin) & (x <= np.array(DIMS) - 1 - margin), axis=-1)


def _cast(s, w, pose=POSE, **kw):
    rec = rr.records_from_volume(s, w)
    return rr.raycast(rec, DIMS, ORIGIN, VOXEL, TRUNC, CAM, pose, **kw)


def _plane_normal_cam(pose):
    R = np.asarray(pose[0], np.float64)
    n = -NPLANE / np.linalg.norm(NPLANE)                 # the field grows towards -n: the camera side
    return R @ n


def test_plane_depth_and_normals_are_exact():
    s, w = plane_volume()
    for pose in (POSE, (np.array([[0.98, 0.0, -0.2], [0.0, 1.0, 0.0], [0.2, 0.0, 0.98]]), np.array([0.1, -0.05, 1.9]))):
        R = pose[0] / np.linalg.norm(pose[0], axis=1, keepdims=True)
        u_, _, vt = np.linalg.svd(R)
        pose = (u_ @ vt, pose[1])
        depth, nrm, bgr, steps = _cast(s, w, pose)
        z, x = plane_truth(pose)
        inner = _interior(x, 1.0)
        assert inner.sum() > 500
        assert np.abs(depth[inner] - z[inner]).max() < 1e-5
        assert (depth[~_interior(x, -1e-3)] == 0).all()
        want = _plane_normal_cam(pose)
        assert np.abs(nrm[inner] - want).max() < 1e-5
        assert (bgr == 128).all()
        assert steps[inner].max() < 200


def sphere_volume(centre=(0.03, -0.02, 0.05), radius=0.3, w=3):
    ii, jj, kk = _grid_coords()
    p = np.stack([ORIGIN[a] + (g + 0.5) * VOXEL for a, g in enumerate((ii, jj, kk))], axis=-1)
    sdf = np.linalg.norm(p - np.array(centre), axis=-1) - radius
    q = np.rint(np.clip(sdf / TRUNC, -1.0, 1.0) * 32767.0).astype(np.int64)
    return q * w, np.full(DIMS, w, np.int64)


def test_sphere_depth_misses_and_normals_face_the_camera():
    centre, radius = np.array([0.03, -0.02, 0.05]), 0.3
    s, w = sphere_volume(tuple(centre), radius)
    depth, nrm, _, _ = _cast(s, w)
    C, D = _rays(POSE)
    # analytic intersection of C + z D with the sphere
    oc = C - centre
    a = np.einsum("...i,...i", D, D)
    b = 2 * np.einsum("...i,i", D, oc)
    c = oc @ oc - radius ** 2
    disc = b * b - 4 * a * c
    z = np.where(disc >= 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0.0)
    p = C + z[..., None] * D
    nrm_true = (p - centre) / radius
    cosang = -np.einsum("...i,...i", nrm_true, D) / np.sqrt(a)
    frontal = (disc >= 0) & (cosang > 0.3)
    # closest approach of the ray to the centre: clear misses
    dist = np.linalg.norm(np.cross(D, oc[None, None, :] * np.ones_like(D)), axis=-1) / np.sqrt(a)
    miss = dist > radius + 2 * VOXEL
    assert frontal.sum() > 150 and miss.sum() > 300
    assert np.abs(depth[frontal] - z[frontal]).max() < 0.05 * VOXEL
    assert (depth[miss] == 0).all()
    hit = depth > 0
    dots = nrm[..., 0] * D[..., 0] + nrm[..., 1] * D[..., 1] + nrm[..., 2] * D[..., 2]
    assert (np.linalg.norm(nrm[hit], axis=-1) > 0.999).all()
    assert (dots[hit] < 0).all()
    assert np.abs(nrm[frontal] - nrm_true[frontal]).max() < 0.05          # (gradient of the trilinear field: within ~3 degrees)


def test_camera_inside_a_surface_sees_nothing():
    centre = (0.03, -0.02, 0.05)
    s, w = sphere_volume(centre, 0.3)
    inside = (np.eye(3), -np.array(centre))             # camera at the sphere's centre
    depth, nrm, _, steps = _cast(s, w, inside)
    assert (depth == 0).all() and (nrm == 0).all()
    assert (steps == 1).all()                           # the first sample is defined and negative


def test_unobserved_slab_in_front_does_not_stop_the_ray():
    s, w = plane_volume()
    s[:, :, 8:13] = 0
    w[:, :, 8:13] = 0                                   # between the camera and every point of the plane
    depth, _, _, _ = _cast(s, w)
    z, x = plane_truth(POSE)
    inner = _interior(x, 1.0)
    assert inner.sum() > 500
    assert np.abs(depth[inner] - z[inner]).max() < 1e-5


def test_min_weight_gates():
    ii, _, _ = _grid_coords()
    wv = np.where(ii < 32, 1, 3).astype(np.int64)
    s, w = plane_volume(wv)
    z, x = plane_truth(POSE)
    inner = _interior(x, 1.0)
    low, high = inner & (x[..., 0] < 30), inner & (x[..., 0] > 33)
    assert low.sum() > 100 and high.sum() > 100
    for mw in (0, 1):
        d, _, _, _ = _cast(s, w, min_weight=mw)
        assert np.abs(d[inner] - z[inner]).max() < 1e-5
    for mw in (2, 3):
        d, n, _, _ = _cast(s, w, min_weight=mw)
        assert (d[low] == 0).all() and (n[low] == 0).all()
        assert np.abs(d[high] - z[high]).max() < 1e-5
    d, _, _, _ = _cast(s, w, min_weight=4)
    assert (d == 0).all()


def test_colour_of_the_hit_voxel():
    s, w = plane_volume()
    rec = rr.records_from_volume(s, w)
    cen = np.zeros((rec.shape[0], 4), np.uint64)
    ii, jj, kk = _grid_coords()
    idx = rr.rec_index(ii.ravel(), jj.ravel(), kk.ravel(), DIMS)
    n = 3
    r, g, b = (ii.ravel() * 4) % 256, (jj.ravel() * 4) % 256, np.full(ii.size, 77)
    cen[idx, 1] = np.uint64(n) << np.uint64(32)
    cen[idx, 2] = (r * n + 1).astype(np.uint64) | ((g * n + 2).astype(np.uint64) << np.uint64(32))
    cen[idx, 3] = (b * n).astype(np.uint64)
    depth, _, bgr, _ = rr.raycast(rec, DIMS, ORIGIN, VOXEL, TRUNC, CAM, POSE, centroid=cen)
    z, x = plane_truth(POSE)
    inner = _interior(x, 1.0)
    vox = np.floor(x + 0.5).astype(np.int64)
    want = np.stack([np.full(vox.shape[:2], 77), (vox[..., 1] * 4) % 256, (vox[..., 0] * 4) % 256], axis=-1)
    # (the analytic hit and the ray cast's differ by far less than a voxel, away from voxel faces)
    far = inner & np.all(np.abs(x + 0.5 - np.round(x + 0.5)) > 1e-3, axis=-1)
    assert far.sum() > 500
    assert np.array_equal(bgr[far], want[far].astype(np.uint8))
    assert (bgr[depth == 0] == 128).all()


def test_cli_help_lists_render_output():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "depth_to_reconstruction.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0
    assert "--render-output" in r.stdout


def test_cli_refuses_render_output_on_several_gpus(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "depth_to_reconstruction.py"), "--rgb-folder", str(tmp_path),
                        "--depth-folder", str(tmp_path), "--fx", "1", "--fy", "1", "--cx", "0", "--cy", "0", "--gpus", "2",
                        "--render-output", str(tmp_path / "views")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "--render-output" in r.stderr and "single GPU" in r.stderr
    assert not (tmp_path / "views").exists()
