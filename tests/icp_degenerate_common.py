"""Shared by the degenerate-geometry registration tests (CPU and GPU): scenes whose normal equations leave some motion
unobserved, one start pose per case, the fp64 reference of ONE update step, and the bound a correct device step must keep to it.
Not a test.

The solve of every registration (reg_solve.h: solve6_wave / solve_n_serial) is x = -(M + lam I)^+ b over
the eigen-directions of M + lam I whose eigenvalue exceeds eig_rel * the largest.  The reference here is that sentence in numpy
(track_reference.solve for 6 unknowns, solve_n below for Sim(3)'s 7), fed with sums that never come from the device: the C oracle's
icp_sums / icp_sums_scale for the pairwise paths, track_reference.sums for tracking.

step_bound: how far a correct device step may lie from the reference step
---------------------------------------------------------------------------
The device adds the reference's very terms in another order, so its sums differ from the reference's by at most the reordering
bound the evaluation tests assert (tests/test_gpu_icp_eval.py, tests/test_gpu_track.py): with delta = n_corr 2^-52,
|dM_ij| <= delta sum|J_i J_j| <= delta sqrt(M_ii M_jj) and |db_i| <= delta sum|J_i r| <= delta sqrt(M_ii e) (Cauchy-Schwarz), hence
    |dM|_F <= delta trace(M),        |db|_2 <= delta sqrt(trace(M) e).
An eigen-solver (LAPACK's in the reference, cyclic Jacobi on the device) returns the exact decomposition of a matrix a small
multiple of n 2^-52 |M|_2 away (n unknowns); both are covered by adding EIG_FEW n 2^-52 |M|_2 to |dM|:
    dA := delta trace(M) + EIG_FEW n 2^-52 lmax.
Let (l_i, v_i) be the reference spectrum of M + lam I, K the kept set, D the dropped one, P the projector on span(v_K),
lK = min l_K, lD = max l_D (0 when nothing is dropped) and x = -P (M + lam I)^-1 P b the reference step.  To first order in dA, db:
  * inside the kept subspace the step is the solution of a linear system with smallest eigenvalue lK:
        |dx|_kept <= (dA |x| + db) / lK;
  * the kept subspace itself turns towards the dropped one by an angle phi <= dA / (lK - lD) (Davis-Kahan, first order).  The
    turn moves x by phi |x| (x leaves the old subspace) and brings in the part of b that lay in the dropped subspace, divided by an
    eigenvalue of at least lK: phi |P_D b| / lK.  With nothing dropped there is no such term.
        |dx|_turn <= dA / (lK - lD) * (|x| + |P_D b| / lK).
step_bound = |dx|_kept + |dx|_turn.  It is meaningful only while no eigenvalue is near the cutoff (the device and the reference
must agree on K): tests/test_icp_degenerate_reference_cpu.py checks a factor-2 hole around eig_rel * lmax on every case.
The pose: |exp(x) T - exp(x_ref) T|_F <= |dx| (1 + |T|_F) to first order, plus the rounding of the update itself (sin, cos, a 3 x 3
by 3 x 4 product in fp64 on both sides): POSE_ULPS 2^-52 |T|_F."""
import math

import numpy as np

import raycast_reference as rr
import track_reference as tr
from tl3d import synth

CAM = dict(width=160, height=120, fx=140.0, fy=140.0, cx=79.5, cy=59.5)
W, H = CAM["width"], CAM["height"]
EPS = 2.0 ** -52
EIG_FEW = 4.0                                  # "a few": the backward error of an eigen-solver in units of n 2^-52 |M|
POSE_ULPS = 16.0                               # rounding of se3_apply itself, in units of 2^-52 |T|_F
PRM = dict(damping=1e-6, eig_rel=1e-4, max_dist=0.1, eps=1e-9)
TRACK_PRM = dict(damping=1e-6, eig_rel=1e-4, max_dist=0.05, eps=1e-9)
STRIDES, RADII = (1, 2), (0, 1)
SIM3_CASES = ("plane", "sphere", "tube", "control")
PLANE_LEAK = 1e-4                              # the bar tests/test_track_reference_cpu.py holds the reference to on a plane


def oracle():
    from oracle import c_oracle
    return c_oracle.Oracle(W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], 0.1, 50.0, dims=(8, 8, 8), origin=(0.0, 0.0, 0.0), voxel_size=0.02,
                           sdf_trunc=0.08)


# ---- scenes and start poses -----------------------------------------------------------------------------------------------
def twist(rot_deg, trans, axis, direction):
    a, d = np.asarray(axis, np.float64), np.asarray(direction, np.float64)
    return np.concatenate([np.radians(rot_deg) * a / np.linalg.norm(a), trans * d / np.linalg.norm(d)])


MOTION = twist(1.0, 0.03, (0.2, 1.0, 0.1), (1.0, 0.3, 0.2))                 # target camera -> source camera, every case
OFFSET = twist(0.5, 0.008, (0.3, -0.5, 0.8), (0.6, -0.3, 0.74))             # the start's error: track_common.offset_pose's axes
_TILT = np.array([0.3, 0.2, -1.0]) / np.linalg.norm([0.3, 0.2, -1.0])
_EYE = (np.eye(3), np.zeros((3, 1)))


def _scenes():
    """name -> (scene, world->camera pose of the target frame)"""
    return {
        "plane": (synth.Scene(planes=[((0.0, 0.0, -1.0), -1.5)]), _EYE),                                    # z = 1.5
        "tilted_plane": (synth.Scene(planes=[(tuple(_TILT), float(_TILT @ [0.0, 0.0, 1.5]))]), _EYE),
        "sphere": (synth.Scene(spheres=[((0.0, 0.0, 1.2), 0.45)]), _EYE),
        "cylinder": (synth.cylinder_scene(ground=False), synth.orbit_poses(1, 1.0, 0.0)[0]),
        "tube": (synth.Scene(room=((-1.0, -1.2, -50.0), (1.0, 1.2, 200.0))), _EYE),                          # its ends beyond max_depth
        "corridor": (synth.corridor_scene(), _EYE),
        "control": (synth.object_scene(True), synth.orbit_poses(1, 1.0, 0.0)[0]),
    }


PAIR_CASES = tuple(_scenes())
EXPECTED_KEPT = dict(plane=3, tilted_plane=3, sphere=3, cylinder=4, tube=4, corridor=6, control=6)          # of 6 unknowns
# of Sim(3)'s 7: a plane's distance is one constraint on (translation along the normal, scale), a sphere's radius observes the
# scale (weakly), the tube's width observes it well
EXPECTED_KEPT_SIM3 = dict(plane=3, sphere=4, tube=5, control=7)
LEAK_CASES = ("plane", "tilted_plane", "sphere", "cylinder", "tube")
# The start of the leak checks.  A plane's unobserved twists are exact null vectors of every J = [p x n, n] (n is constant), so
# its start is T_init.  On a sphere and a cylinder they are null only for p ON the surface: p is the transformed source point,
# which the projective association pairs with the target point of the nearest pixel -- up to half a pixel (4 mm at 1.2 m) beside
# it, and off the surface by the observed part of the start's error.  The reference step leans into the unobserved twists by
# that much, so these two start closer in the observed directions (2.5 mm along z; the step stays above 1e-3) and further in the
# unobserved ones: (coefficients of the twists of unobserved(), metres along the target camera's z).  These two starts were
# moved until the bar -- twice the reference's own lean, about 4e-4 |x| -- came under the 1e-3 the CPU test asks for; with a
# bar that close to the reference's own value, the leak check adds little on these two cases to the comparison with the
# reference step that runs beside it.  On the planes and the tube it stands on its own.
LEAK_START = dict(sphere=((0.006, 0.006, 0.006), 0.0025), cylinder=((0.0005, 0.008), 0.0025))


def plane_twists(n):
    """what a plane with normal n (camera frame) leaves free: the rotation about the normal, the in-plane translations"""
    t1 = np.cross(n, [1.0, 0.0, 0.0]); t1 /= np.linalg.norm(t1)
    z3 = np.zeros(3)
    return [np.r_[n, z3], np.r_[z3, t1], np.r_[z3, np.cross(n, t1)]]


def axis_twists(a, c):
    """what a cylinder about the axis a through c (camera frame) leaves free: the spin about and the slide along the axis"""
    return [np.r_[a, np.cross(c, a)], np.r_[np.zeros(3), a]]


def orthonormal(cols):
    return np.linalg.qr(np.stack(cols, axis=1))[0]


def unobserved(name, T_tgt):
    """orthonormal twists [6, k] (target-camera frame, the frame the update acts in) that the geometry of `name` leaves free, or None.
    A twist (w, v) moves p by w x p + v; J = [p x n, n]."""
    R, t = T_tgt[:3, :3], T_tgt[:3, 3]
    if name in ("plane", "tilted_plane"):
        cols = plane_twists(R @ (np.array([0.0, 0.0, -1.0]) if name == "plane" else _TILT))
    elif name == "sphere":                                                   # the rotations about its centre c: (w, c x w)
        c = R @ np.array([0.0, 0.0, 1.2]) + t
        cols = [np.r_[w, np.cross(c, w)] for w in np.eye(3)]
    elif name == "cylinder":                                                 # the axis: world y through 0
        cols = axis_twists(R @ np.array([0.0, 1.0, 0.0]), t)
    elif name == "tube":
        # slide along the axis (world z) only.  A rectangular tube does observe the spin about its axis; the second direction its
        # spectrum drops (a mix of the rotation about x and the translation along y) is no symmetry: floor and ceiling come into
        # view at 2.8 m, where neighbouring rows are already a depth_jump apart, so hardly any of their pixels has a normal.  That
        # direction has no leak assertion of its own: the comparison with the reference step within step_bound holds it (a solve
        # that keeps it misses the bound by more than 1e7: the no_cutoff mutant of the CPU test)
        cols = [np.r_[np.zeros(3), R @ np.array([0.0, 0.0, 1.0])]]
    else:
        return None
    return orthonormal(cols)


_PAIRS = {}


def pair_frames():
    """name -> dict(src, tgt: depth images; T_true: source camera -> target camera; T_init; T_tgt).  Computed once."""
    if not _PAIRS:
        for name, (scene, pose) in _scenes().items():
            T_tgt = tr.pose_matrix(pose)
            T_src = tr.se3_apply(MOTION, T_tgt)
            tgt = synth.render(scene, (T_tgt[:3, :3], T_tgt[:3, 3]), **CAM, want_color=False)[0]
            src = synth.render(scene, (T_src[:3, :3], T_src[:3, 3]), **CAM, want_color=False)[0]
            T_true = T_tgt @ np.linalg.inv(T_src)
            T_leak = tr.se3_apply(OFFSET, T_true)
            if name in LEAK_START:
                coef, dz = LEAK_START[name]
                T_leak = tr.se3_apply(unobserved(name, T_tgt) @ np.asarray(coef) + np.r_[np.zeros(5), dz], T_true)
            _PAIRS[name] = dict(name=name, src=src, tgt=tgt, T_true=T_true, T_init=tr.se3_apply(OFFSET, T_true), T_tgt=T_tgt, T_leak=T_leak)
    return _PAIRS


_MAPS = {}


def maps(orc, name, radius):
    """(source depth a registration reads, target normal map) of a pair under smoothing radius `radius`: the C oracle's"""
    key = (name, radius)
    if key not in _MAPS:
        f = pair_frames()[name] if name in PAIR_CASES else pixel_frames()[name]
        if radius:
            _MAPS[key] = (orc.normals_smooth(f["src"], radius=radius)[0], orc.normals_smooth(f["tgt"], radius=radius)[1])
        else:
            _MAPS[key] = (f["src"], orc.normals(f["tgt"]))
    return _MAPS[key]


# ---- the N-pixel frames of the count gates -----------------------------------------------------------------------------------
# even coordinates (on the stride-2 grid too), spread over the control scene's image; the first N of them are kept
PIXELS = ((10, 8), (150, 12), (80, 60), (24, 100), (140, 104), (60, 30), (110, 84), (40, 64))
_PIXEL_FRAMES = {}


def pixel_frames():
    """'pixels5', 'pixels6': the control pair with the source depth zeroed except at the first N of PIXELS"""
    if not _PIXEL_FRAMES:
        base = pair_frames()["control"]
        for n in (5, 6):
            src = np.zeros_like(base["src"])
            for u, v in PIXELS[:n]:
                src[v, u] = base["src"][v, u]
            _PIXEL_FRAMES[f"pixels{n}"] = dict(base, name=f"pixels{n}", src=src)
    return _PIXEL_FRAMES


# ---- reference: one step ---------------------------------------------------------------------------------------------------
def system7(s37):
    """(M [7, 7], b [7]) from orc.icp_sums_scale's 37 doubles, in solve7_serial's layout: the pose block with the scale column
    c appended to every row, cc in the corner, bc as b's last entry"""
    s = np.asarray(s37, np.float64)
    M = np.zeros((7, 7))
    M[:6, :6] = tr.sym6(s[:21])
    M[:6, 6] = M[6, :6] = s[29:35]
    M[6, 6] = s[35]
    return M, np.concatenate([s[21:27], [s[36]]])


def spectrum(M, damping=PRM["damping"], eig_rel=PRM["eig_rel"]):
    """(eigenvalues ascending, eigenvectors, kept mask) of M + damping trace(M) / n I, as the solves cut it"""
    n = len(M)
    lam, V = np.linalg.eigh(M + damping * (np.trace(M) / n) * np.eye(n))
    return lam, V, (lam > eig_rel * lam.max()) & (lam > 0.0)


def solve_n(M, b, damping=PRM["damping"], eig_rel=PRM["eig_rel"], keep=None):
    """track_reference.solve for any n (Sim(3): 7): x = -(M + lam I)^+ b over the kept eigen-directions; None when there is none.
    keep: a mask to use instead of the cutoff's (the mutants of the CPU test)."""
    if not np.trace(M) > 0.0:
        return None
    lam, V, k = spectrum(M, damping, eig_rel)
    k = k if keep is None else keep
    if not lam.max() > 0.0 or not k.any():
        return None
    return -(V[:, k] @ ((V[:, k].T @ np.asarray(b)) / lam[k]))


def step_bound(M, b, e, n_corr, x, damping=PRM["damping"], eig_rel=PRM["eig_rel"]):
    """|x_device - x| allowed (module docstring).  M, b, e, n_corr: the reference sums; x: the reference step."""
    n = len(M)
    lam, V, k = spectrum(M, damping, eig_rel)
    delta = n_corr * EPS
    dA = delta * np.trace(M) + EIG_FEW * n * EPS * lam.max()
    db = delta * math.sqrt(np.trace(M) * e)
    lK = lam[k].min()
    xn = float(np.linalg.norm(x))
    kept = (dA * xn + db) / lK
    turn = 0.0
    if (~k).any():
        lD = max(lam[~k].max(), 0.0)
        bD = float(np.linalg.norm(V[:, ~k].T @ np.asarray(b)))
        turn = dA / (lK - lD) * (xn + bD / lK)
    return kept + turn


def pose_bound(dx, T):
    nT = float(np.linalg.norm(T))
    return dx * (1.0 + nT) + POSE_ULPS * EPS * nT


def reference_step(orc, name, stride, radius, sim3=False, T=None, scale=1.0, prm=PRM):
    """dict(x, T, scale, M, b, e, n_corr, n_src, bound, pose_bound, status, iters_run) of one step of the pair `name` from its T_init
    (or T).  status / iters_run: what a run with iters=1 reports (2 / 0 when the step cannot be taken)."""
    f = pair_frames()[name] if name in PAIR_CASES else pixel_frames()[name]
    T = f["T_init"] if T is None else T
    src, nmap = maps(orc, name, radius)
    if sim3:
        s, cnt, nsrc = orc.icp_sums_scale(src, nmap, T, stride=stride, max_dist=prm["max_dist"], scale_src=scale)
        M, b = system7(s)
    else:
        s, cnt, nsrc = orc.icp_sums(src, nmap, T, stride=stride, max_dist=prm["max_dist"], scale_src=scale)
        M, b = tr.sym6(s[:21]), s[21:27].copy()
    out = dict(M=M, b=b, e=float(s[27]), n_corr=cnt, n_src=nsrc, x=None, T=T.copy(), scale=scale, status=2, iters_run=0, bound=0.0, pose_bound=0.0)
    if cnt < 6:
        return out
    x = solve_n(M, b, prm["damping"], prm["eig_rel"]) if sim3 else tr.solve(s[:21], b, prm["damping"], prm["eig_rel"])
    if x is None:
        return out
    bound = step_bound(M, b, out["e"], cnt, x, prm["damping"], prm["eig_rel"])
    T1 = tr.se3_apply(x[:6], T)
    return dict(out, x=x, T=T1, scale=scale * math.exp(x[6]) if sim3 else scale, status=int(np.abs(x).max() < prm["eps"]), iters_run=1, bound=bound,
                pose_bound=pose_bound(bound, T))


def leak(Q, x):
    """largest component of the step x along the unobserved twists Q, relative to |x|"""
    return float(np.abs(Q.T @ np.asarray(x)[:6]).max() / np.linalg.norm(np.asarray(x)[:6]))


def step_of(T1, T0):
    """the twist x with T1 = se3_apply(x, T0), to first order beyond the rotation (exact rotation vector): what a one-step result
    moved by, for the leak checks"""
    D = T1[:3, :3] @ T0[:3, :3].T
    ang = math.acos(min(1.0, max(-1.0, (np.trace(D) - 1.0) / 2.0)))
    w = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) / 2.0
    w = w * (ang / math.sin(ang)) if ang > 1e-12 else w
    return np.concatenate([w, T1[:3, 3] - D @ T0[:3, 3]])


# ---- tracking: crafted TSDF records ----------------------------------------------------------------------------------------
T_DIMS, T_VOXEL = (64, 64, 64), 0.02
T_ORIGIN, T_TRUNC = tuple(-0.5 * d * T_VOXEL for d in T_DIMS), 4 * T_VOXEL
T_SPEC = (T_DIMS, T_ORIGIN, T_VOXEL, T_TRUNC)
T_POSE = (np.eye(3), np.array([0.0, 0.0, 2.0]))                              # the camera at z = -2, looking at the grid
T_NRM = np.array([1.0, 2.0, 8.0]) / np.linalg.norm([1.0, 2.0, 8.0])
T_CYL_R = 0.35
TRACK_CASES = ("track_plane", "track_cylinder")
TRACK_KEPT = dict(track_plane=3, track_cylinder=4)
_TRACK = {}


def _voxel_centres():
    ii, jj, kk = np.meshgrid(*[np.arange(n) for n in T_DIMS], indexing="ij")
    return np.stack([T_ORIGIN[a] + (g + 0.5) * T_VOXEL for a, g in enumerate((ii, jj, kk))], axis=-1)


def track_cases():
    """name -> dict(rec, depth, start: (R, t), T0, Q): the plane of tests/test_track_reference_cpu.py and a cylinder about the y axis,
    both seen from T_POSE through their own ray cast; start = the view 0.5 degrees and 8 mm off"""
    if not _TRACK:
        p = _voxel_centres()
        sdfs = dict(track_plane=-(p @ T_NRM - 0.1), track_cylinder=np.hypot(p[..., 0], p[..., 2]) - T_CYL_R)
        for name, sdf in sdfs.items():
            rec = rr.records_from_volume(np.rint(np.clip(sdf / T_TRUNC, -1.0, 1.0) * 32767.0).astype(np.int64), np.ones(T_DIMS, np.int64))
            depth = rr.raycast(rec, *T_SPEC, CAM, T_POSE)[0]
            T0 = tr.se3_apply(OFFSET, tr.pose_matrix(T_POSE))
            # the step acts on the points in the camera frame of the start pose: the unobserved twists there
            R, t = T0[:3, :3], T0[:3, 3]
            cols = plane_twists(R @ T_NRM) if name == "track_plane" else axis_twists(R @ np.array([0.0, 1.0, 0.0]), t)
            _TRACK[name] = dict(name=name, rec=rec, depth=depth, start=(T0[:3, :3].copy(), T0[:3, 3].copy()), T0=T0, Q=orthonormal(cols))
    return _TRACK


def track_pixels():
    """8 pixels of the plane's frame that are correspondences at its start pose, on the stride-2 grid, spread over the image:
    evenly spaced in the row-major list of the stride-2 pass's correspondences"""
    c = track_cases()["track_plane"]
    if "pixels" not in c:
        s = tr.sums(c["rec"], *T_SPEC, CAM, c["depth"], c["start"], stride=2, max_dist=TRACK_PRM["max_dist"], min_weight=1, detail=True)
        pick = np.rint(np.linspace(0, s["n_corr"] - 1, 10)).astype(int)[1:9]
        c["pixels"] = tuple((int(s["u"][i]), int(s["v"][i])) for i in pick)
    return c["pixels"]


def track_pixel_depth(n):
    """the plane's depth image zeroed except at the first n of track_pixels()"""
    full = track_cases()["track_plane"]["depth"]
    d = np.zeros_like(full)
    for u, v in track_pixels()[:n]:
        d[v, u] = full[v, u]
    return d


def track_reference_step(name, stride, depth=None, prm=TRACK_PRM, T0=None):
    """as reference_step, for one tracking step of `name` from its start or T0 (the camera moves by -x: track_reference.track)"""
    c = track_cases()[name]
    c = c if T0 is None else dict(c, T0=T0, start=(T0[:3, :3], T0[:3, 3]))
    depth = c["depth"] if depth is None else depth
    s = tr.sums(c["rec"], *T_SPEC, CAM, depth, c["start"], stride=stride, max_dist=prm["max_dist"], min_weight=1)
    M = tr.sym6(s["A"])
    out = dict(M=M, b=s["b"], e=s["e"], n_corr=s["n_corr"], n_src=s["n_src"], x=None, T=c["T0"].copy(), status=2, iters_run=0, bound=0.0, pose_bound=0.0)
    x = tr.solve(s["A"], s["b"], prm["damping"], prm["eig_rel"]) if s["n_corr"] >= 8 else None
    if x is None:
        return out
    bound = step_bound(M, s["b"], s["e"], s["n_corr"], x, prm["damping"], prm["eig_rel"])
    return dict(out, x=x, T=tr.se3_apply(-x, c["T0"]), status=int(np.abs(x).max() < prm["eps"]), iters_run=1, bound=bound,
                pose_bound=pose_bound(bound, c["T0"]))


# ---- the grid of cases, and a few iterations ----------------------------------------------------------------------------------
def combos():
    """every (name, stride, radius, sim3) of the one-step tests"""
    return [(name, stride, radius, sim3) for name in PAIR_CASES for stride in STRIDES for radius in RADII
            for sim3 in ((False, True) if name in SIM3_CASES else (False,))]


# The steps of the reference runs fall to the noise floor of the f32 pass (1e-10 .. 1e-7) by the third iteration and stay there;
# this eps lies more than 10 times below every one of them (checked on the CPU for every run the GPU test makes), so no run
# stops early and iters_run can be compared
FEW_ITERS, FEW_EPS = 5, 1e-11


def few_reference(orc, name, stride, radius, sim3=False):
    """(largest |x_i| of each of FEW_ITERS reference steps, T, scale): the numpy reference iterated, to show that no step of the
    few-iteration runs comes near FEW_EPS"""
    T, scale, sizes = pair_frames()[name]["T_init"], 1.0, []
    for _ in range(FEW_ITERS):
        r = reference_step(orc, name, stride, radius, sim3, T=T, scale=scale)
        assert r["x"] is not None
        sizes.append(float(np.abs(r["x"]).max()))
        T, scale = r["T"], r["scale"]
    return sizes, T, scale


def track_few_sizes(name, stride):
    """largest |x_i| of each of FEW_ITERS reference tracking steps"""
    T0, sizes = track_cases()[name]["T0"], []
    for _ in range(FEW_ITERS):
        r = track_reference_step(name, stride, T0=T0)
        sizes.append(float(np.abs(r["x"]).max()))
        T0 = r["T"]
    return sizes


def track_few_reference(name, stride):
    c = track_cases()[name]
    return tr.track(c["rec"], *T_SPEC, CAM, c["depth"], c["start"], [dict(TRACK_PRM, iters=FEW_ITERS, stride=stride, eps=FEW_EPS)])


def scale_bound(r):
    """of a Sim(3) step's scale = scale_0 exp(x[6]): the step's bound, and the rounding of exp"""
    return r["scale"] * (r["bound"] + 4.0 * EPS)


# ---- leak bars ---------------------------------------------------------------------------------------------------------------
def leak_reference(orc, name, stride, radius):
    """(reference step from the leak start of `name`, leak bar): PLANE_LEAK on a plane, elsewhere twice the reference's own leak"""
    f = pair_frames()[name]
    r = reference_step(orc, name, stride, radius, T=f["T_leak"])
    return r, PLANE_LEAK if "plane" in name else 2.0 * leak(unobserved(name, f["T_tgt"]), r["x"])


def track_leak_reference(name, stride):
    r = track_reference_step(name, stride)
    return r, PLANE_LEAK if name == "track_plane" else 2.0 * leak(track_cases()[name]["Q"], r["x"])
