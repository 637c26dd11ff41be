"""An fp64 model of the two readers of the TSDF cell -- the ray caster and the point-to-SDF tracker (section
12) -- written from the rules, not from the kernels, for the crafted cases of cell_edges_common.  Not a test.

Its formulation is its own: plain Python floats, one ray or one sample at a time;
  t(v)      = sum / (32767 * w), an fp64 quotient; a voxel is usable when w >= max(1, min_weight);
  F(x)      = sum over the 8 corners c of t_c * w_c(f), w_c the product over the axes of f or 1 - f;
  grad F    = the same sum with one factor of w_c replaced by its derivative (+1 / -1);
  ray range = the intersection of [z_near, z_far] with one interval per axis (the whole line or nothing where the ray does not move
              along that axis), not a running min / max;
  x(z)      = (C + z d - origin) / voxel - 1/2 with C = -R^T t and d = R^T (xf, yf, 1); the tracker's x = (R^T (p_c - t) - origin) /
              voxel - 1/2.
Every ray and every sample also reports the EVENTS it went through (which decision ended it, which edges it touched) and how close
it came to a decision (margin): cell_edges_common.counters() adds the events up, the CPU test sets rays aside by the margin.
"""
import math

import numpy as np

MAX_STEPS = 4096
# |grad F| <= 2 sqrt(3) < 4 per voxel for corner values in [-1, 1]: a point that moves by delta voxels changes F by less than 4 delta, so a
# margin of F against 0 or the gate is |F - limit| / SLOPE voxels
SLOPE = 4.0


def rec_index(i, j, k, dims):
    """record of voxel (i, j, k): bricks of 8^3 x-fastest, inside a brick 4^3 sub-bricks, inside those x fastest"""
    nbx, nby = dims[0] // 8, dims[1] // 8
    brick = ((k // 8) * nby + (j // 8)) * nbx + (i // 8)
    sub = ((k % 8) // 4) * 4 + ((j % 8) // 4) * 2 + ((i % 8) // 4)
    return brick * 512 + sub * 64 + (k % 4) * 16 + (j % 4) * 4 + (i % 4)


class Volume:
    """the records behind a cell look-up; reads are counted by kind for the counters"""

    def __init__(self, rec, dims, min_weight):
        rec = np.asarray(rec).reshape(-1, 2)
        self.s = rec[:, 0].astype(np.int64).tolist()
        self.w = rec[:, 1].astype(np.int64).tolist()
        self.dims = tuple(int(d) for d in dims)
        self.mw = max(1, int(min_weight))

    def cell(self, x, ev=None):
        """(defined, corner values [8] or None, fractions, margin): margin = the distance of x, in voxels, to the nearest boundary
        across which the answer `defined` changes (a box face, or the wall to a neighbouring cell of the other definedness)"""
        n = self.dims
        if not all(0.0 <= x[a] < n[a] - 1 for a in range(3)):
            return False, None, None, self._margin(x, False)
        base = [int(math.floor(x[a])) for a in range(3)]
        f = [x[a] - base[a] for a in range(3)]
        ok, t = self._corners(base, ev)
        return ok, t, f, self._margin(x, ok, base)

    def _corners(self, base, ev=None):
        ok, t = True, []
        for c in range(8):
            r = rec_index(base[0] + (c & 1), base[1] + ((c >> 1) & 1), base[2] + ((c >> 2) & 1), self.dims)
            s, w = self.s[r], self.w[r]
            if ev is not None:
                if w == self.mw:
                    ev["w_eq_mw"] = ev.get("w_eq_mw", 0) + 1
                if w == self.mw - 1:
                    ev["w_eq_mw_minus_1"] = ev.get("w_eq_mw_minus_1", 0) + 1
                if w == 0 and s != 0:
                    ev["w0_sum_nonzero"] = ev.get("w0_sum_nonzero", 0) + 1
                if w > 0 and abs(s) > 2 ** 24 and float(np.float32(s)) != float(s):
                    ev["sum_not_f32"] = ev.get("sum_not_f32", 0) + 1
            if w >= self.mw:
                t.append(s / (32767.0 * w))
            else:
                ok = False
                t.append(0.0)
        return ok, t

    def _defined_at(self, base):
        n = self.dims
        if not all(0 <= base[a] < n[a] - 1 for a in range(3)):
            return False
        return self._corners(base)[0]

    def _margin(self, x, ok, base=None):
        n = self.dims
        if base is None:                              # outside (or on the open end of) the box of cells: distance back into it
            return max(max(-x[a], x[a] - (n[a] - 1)) for a in range(3))
        m = math.inf
        for a in range(3):
            for step, dist in ((-1, x[a] - base[a]), (1, base[a] + 1 - x[a])):
                nb = list(base)
                nb[a] += step
                if self._defined_at(nb) != ok:
                    m = min(m, dist)
        return m


def field(t, f):
    return sum(t[c] * ((f[0] if c & 1 else 1.0 - f[0]) * (f[1] if c & 2 else 1.0 - f[1]) * (f[2] if c & 4 else 1.0 - f[2])) for c in range(8))


def gradient(t, f):
    g = []
    for a in range(3):
        tot = 0.0
        for c in range(8):
            w = 1.0
            for b in range(3):
                bit = (c >> b) & 1
                w *= (1.0 if bit else -1.0) if b == a else (f[b] if bit else 1.0 - f[b])
            tot += t[c] * w
        g.append(tot)
    return g


def _camera_in_grid(pose, origin, voxel):
    R = np.asarray(pose[0], np.float64).reshape(3, 3)
    t = np.asarray(pose[1], np.float64).reshape(3)
    C = -(R.T @ t)
    return R, t, [(C[a] - origin[a]) / voxel - 0.5 for a in range(3)]


def ray_range(cg, dg, dims, z_near, z_far):
    """(z0, z1, stationary axes): the intersection of [z_near, z_far] with the per-axis intervals in which 0 <= x_a(z) <= n_a - 1"""
    lo, hi, still = [z_near], [z_far], []
    for a in range(3):
        top = dims[a] - 1
        if dg[a] == 0.0:
            still.append((a, 0.0 <= cg[a] <= top, math.copysign(1.0, dg[a]) < 0))
            if not 0.0 <= cg[a] <= top:
                lo.append(math.inf)
                hi.append(-1.0)
            continue
        za, zb = (0.0 - cg[a]) / dg[a], (top - cg[a]) / dg[a]
        lo.append(min(za, zb))
        hi.append(max(za, zb))
    return max(lo), min(hi), still


def cast(vol, origin, voxel, trunc, cam, pose, z_near, z_far, u, v, centroid=None):
    """one ray: dict(depth, normal, bgr, samples, events, margin)"""
    R, _, cg = _camera_in_grid(pose, origin, voxel)
    xf, yf = (u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"]
    # (written out so that a zero keeps the sign IEEE gives it: -0.0 entries of R make dg == -0.0, which must still count as zero)
    dg = [((float(R[0, a]) * xf + float(R[1, a]) * yf) + float(R[2, a])) / voxel for a in range(3)]
    ev = {}
    z0, z1, still = ray_range(cg, dg, vol.dims, z_near, z_far)
    for a, inside, negative in still:
        ev["axis_parallel_inside" if inside else "axis_parallel_outside"] = 1
        if negative:
            ev["axis_parallel_negative_zero"] = 1
    margin = math.inf                                  # in voxels (F: / SLOPE): how close the march came to a decision
    point = lambda z: [cg[a] + z * dg[a] for a in range(3)]
    speed = math.sqrt(sum(q * q for q in dg))          # voxels per unit of z
    z, prev, hit, samples = z0, False, 0.0, 0
    zp = dzp = fp = 0.0
    end = "range_empty" if not z0 <= z1 else None
    if z_near > z_far:
        ev["z_near_gt_z_far"] = 1
    while end is None:
        if samples == MAX_STEPS:
            end = "cap"
            break
        if not z <= z1:
            end = "z1"
            margin = min(margin, (z - z1) * speed)
            break
        margin = min(margin, (z1 - z) * speed if z1 > z else math.inf)
        x = point(z)
        if samples == 0:
            if any(x[a] == 0.0 or x[a] == vol.dims[a] - 1 for a in range(3)):
                ev["first_sample_on_face"] = 1
        if any(x[a] == vol.dims[a] - 1 for a in range(3)):
            ev["sample_on_open_end"] = ev.get("sample_on_open_end", 0) + 1
        ok, t, f, m = vol.cell(x, ev)
        margin = min(margin, m)
        samples += 1
        dz = voxel
        F = 0.0
        if ok:
            F = field(t, f)
            margin = min(margin, abs(F) / SLOPE)
            if F <= 0.0:
                if F == 0.0:
                    ev["F_eq_0_prev_defined" if prev else "F_eq_0_prev_undefined"] = 1
                elif samples == 1:
                    ev["first_sample_negative"] = 1
                elif not prev:
                    ev["negative_after_undefined"] = 1
                if prev:
                    hit = zp + (dzp * fp) / (fp - F)
                    end = "hit"
                else:
                    end = "behind"
                break
            dz = max(0.5 * voxel, 0.8 * trunc * F)
            if dz == 0.5 * voxel:
                ev["half_voxel_steps"] = ev.get("half_voxel_steps", 0) + 1
        prev, fp, zp, dzp = ok, F, z, dz
        z = z + dz
    ev["end_" + end] = 1
    if end == "z1":
        ev["ended_by_z_far" if z1 == z_far else "ended_by_box_exit"] = 1
    normal, bgr = [0.0, 0.0, 0.0], [128, 128, 128]
    if hit > 0.0:
        x = point(hit)
        ok, t, f, m = vol.cell(x)
        margin = min(margin, m)
        if ok:
            g = gradient(t, f)
            len2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2]
            if len2 > 1e-30:
                nw = np.array(g) / math.sqrt(len2)
                nc = R @ nw
                if nc[0] * xf + nc[1] * yf + nc[2] > 0.0:
                    nc = -nc
                normal = [float(q) + 0.0 for q in nc]
            else:
                ev["hit_normal_zero_gradient"] = 1
        else:
            ev["hit_normal_cell_undefined"] = 1
        if centroid is not None:
            vox = [int(math.floor(x[a] + 0.5)) for a in range(3)]
            margin = min(margin, min(abs(x[a] + 0.5 - round(x[a] + 0.5)) for a in range(3)))
            if all(0 <= vox[a] < vol.dims[a] for a in range(3)):
                if any(vox[a] == vol.dims[a] - 1 for a in range(3)):
                    ev["colour_last_voxel"] = 1
                r = centroid[rec_index(vox[0], vox[1], vox[2], vol.dims)]
                cnt = int(r[1]) >> 32
                if cnt > 0:
                    rgb = [(int(r[2]) & 0xffffffff) // cnt, (int(r[2]) >> 32) // cnt, (int(r[3]) & 0xffffffff) // cnt]
                    if any(((int(r[2]) >> s) & 0xffffffff) % cnt for s in (0, 32)) or (int(r[3]) & 0xffffffff) % cnt:
                        ev["colour_division_rounds"] = 1
                    bgr = [q & 0xff for q in rgb[::-1]]
                    ev["colour_mean"] = 1
                else:
                    ev["colour_count_0"] = 1
    return dict(depth=hit, normal=normal, bgr=bgr, samples=samples, events=ev, margin=margin)


def raycast(tsdf, dims, origin, voxel, trunc, cam, pose, min_weight, z_near, z_far, centroid=None):
    """every ray of the camera: (depth f64 [H,W], normals [H,W,3], bgr u8 [H,W,3], samples [H,W], margin [H,W], events: list per ray)"""
    vol = Volume(tsdf, dims, min_weight)
    cen = None if centroid is None else np.asarray(centroid).reshape(-1, 4)
    W, H = int(cam["width"]), int(cam["height"])
    depth, nrm, bgr = np.zeros((H, W)), np.zeros((H, W, 3)), np.zeros((H, W, 3), np.uint8)
    samples, margin, events = np.zeros((H, W), np.int64), np.zeros((H, W)), []
    for v in range(H):
        for u in range(W):
            r = cast(vol, origin, voxel, trunc, cam, pose, float(z_near), float(z_far), u, v, cen)
            depth[v, u], nrm[v, u], bgr[v, u], samples[v, u], margin[v, u] = r["depth"], r["normal"], r["bgr"], r["samples"], r["margin"]
            events.append(r["events"])
    return depth, nrm, bgr, samples, margin, events


def track_sums(tsdf, dims, origin, voxel, trunc, cam, depth, pose, stride, max_dist, min_weight, min_depth, max_depth, scale=1.0,
               pixels=None):
    """one tracking pass: dict(n_src, n_corr, terms: the 28 lists of fp64 products in the order A (upper triangle by rows), b, e,
    J [n][6], r [n], uv [n][2], events (totals), margin: per sampled pixel in image order, or inf)"""
    vol = Volume(tsdf, dims, min_weight)
    R = np.asarray(pose[0], np.float64).reshape(3, 3)
    t = np.asarray(pose[1], np.float64).reshape(3)
    W, H = int(cam["width"]), int(cam["height"])
    depth = np.asarray(depth, np.float32).reshape(H, W)
    gate = min(float(max_dist) / trunc, 0.98)
    ev = {"gate_capped": int(float(max_dist) / trunc > 0.98)}
    bump = lambda k: ev.__setitem__(k, ev.get(k, 0) + 1)
    n_src, Js, rs, uvs, xs, margins = 0, [], [], [], [], []
    lo32, hi32 = np.float32(min_depth), np.float32(max_depth)
    for v in range(0, H, stride):
        for u in range(0, W, stride):
            if pixels is not None and (u, v) not in pixels:
                continue
            raw = depth[v, u]
            d = float(raw * np.float32(scale)) if np.isfinite(raw) else float(raw)     # the slot holds f32 depth; the product is the frame's unit change
            bump("n_samples")
            if math.isnan(d):
                bump("d_nan")
            elif math.isinf(d):
                bump("d_inf")
            elif d == 0.0:
                bump("d_zero")
            elif d < 0.0:
                bump("d_negative")
            for name, lim in (("min", float(lo32)), ("max", float(hi32))):
                if d == lim:
                    bump("d_eq_" + name)
                elif d == float(np.nextafter(np.float32(lim), np.float32(np.inf))):
                    bump("d_next_above_" + name)
                elif d == float(np.nextafter(np.float32(lim), np.float32(-np.inf))):
                    bump("d_next_below_" + name)
                if math.isfinite(d) and float(raw) > 0.0 and (float(raw) > lim) != (d > lim):
                    bump("scale_crosses_" + name)
            if not (d > float(lo32) and d < float(hi32)):
                margins.append(math.inf)
                continue
            n_src += 1
            m = math.inf                               # (d is the f32 product the kernel forms: no deviation, so no margin against the limits)
            xf, yf = (u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"]
            p = np.array([xf * d, yf * d, d])
            pw = R.T @ (p - t)
            x = [(pw[a] - origin[a]) / voxel - 0.5 for a in range(3)]
            ok, tc, f, mc = vol.cell(x, ev)
            m = min(m, mc)
            if not ok:
                bump("cell_undefined")
                margins.append(m)
                continue
            F = field(tc, f)
            m = min(m, abs(abs(F) - gate) / SLOPE)
            margins.append(m)
            if abs(F) == gate:
                bump("F_eq_gate")
            if not abs(F) <= gate:
                bump("gated")
                continue
            g = gradient(tc, f)
            n = R @ (np.array(g) * (trunc / voxel))
            Js.append(list(np.cross(p, n)) + list(n))
            rs.append(F * trunc)
            uvs.append((u, v))
            xs.append(x)
    J = np.array(Js, np.float64).reshape(-1, 6)
    r = np.array(rs, np.float64)
    return dict(n_src=n_src, n_corr=len(rs), J=J, r=r, uv=uvs, x=np.array(xs, np.float64).reshape(-1, 3), events=ev, margin=np.array(margins))


def sum_three_ways(p):
    """(forwards, backwards, exactly rounded) sums of a list of floats"""
    fwd = bwd = 0.0
    for q in p:
        fwd += q
    for q in reversed(p):
        bwd += q
    return fwd, bwd, math.fsum(p)
