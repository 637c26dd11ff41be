"""The weld of the blocks' keyed meshes on the device against the host weld (DESIGN.md sections 4.2.4 and 7.9).  No fusion needed.

Builds a synthetic keyed sheet mesh at the corridor's scale (--vertices, default 53 M: a height field over an nx x ny lattice floor,
one z-edge vertex per column, two triangles per cell: 2.0 triangles per vertex, 53 M / 106 M where the corridor has 53 M / 96 M), cuts it along
x into 2 and into 8 parts as blocks would be (a part holds the triangles of the cells of its core and, as halo copies, the vertices
of the next part's first column, in a shuffled vertex order), and welds each cut
  on the host    lattice.weld_meshes (numpy: argsort + searchsorted), the yardstick;
  on the device  FusionContext.weld_meshes with the same host arrays (uploads and downloads inside the time, as the pipeline calls
                 it), and with device tensors in and out (the kernels and their three waits alone).
Asserts that all three give the same bytes, then times whole calls on the host clock with a device synchronise inside the timed
region: one warm-up each, then --reps rounds that take host and device in turn.  Prints median, smallest and largest of each cut as
soon as it has them; --out FILE also writes them there behind a two-line header (profiles/mesh_weld.txt is made that way).

    python tools/bench_mesh_weld.py [--vertices 53000000] [--reps 3] [--parts 2,8] [--out profiles/mesh_weld.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sheet(np, nx, ny):
    """(key [nx, ny], pos [nx, ny, 3], col [nx, ny, 3]) of the welded sheet: what every cut is made from"""
    i, j = np.meshgrid(np.arange(nx, dtype=np.int64), np.arange(ny, dtype=np.int64), indexing="ij")
    k = (32 + 12 * np.sin(i / 37.0) * np.cos(j / 53.0)).astype(np.int64)
    key = 3 * ((k * ny + j) * nx + i) + 2
    pos = np.stack([i, j, k], axis=-1).astype(np.float32) * np.float32(0.005)
    col = np.stack([i % 251, j % 241, k], axis=-1).astype(np.uint8)
    return key, pos, col


def sheet_parts(np, nx, ny, n_parts, seed=0, base=None):
    """[(xyz, rgb, tris, keys, core_lo, core_hi)] of the sheet cut into n_parts along x, and the lattice dims"""
    rng = np.random.default_rng(seed)
    L = (nx, ny, 64)
    key, pos, col = base if base is not None else sheet(np, nx, ny)
    cuts = [(nx * p) // n_parts for p in range(n_parts + 1)]
    parts = []
    for p in range(n_parts):
        x0, x1 = cuts[p], cuts[p + 1]
        xe = min(x1 + 1, nx)                                                # the next part's first column: halo copies
        w = xe - x0
        perm = rng.permutation(w * ny)                                      # local vertex (column, row) -> its place in the part
        place = np.empty(w * ny, np.int64)
        place[perm] = np.arange(w * ny)
        xyz = pos[x0:xe].reshape(-1, 3)[perm]
        rgb = col[x0:xe].reshape(-1, 3)[perm]
        keys = key[x0:xe].reshape(-1)[perm]
        ci, cj = np.meshgrid(np.arange(min(x1, nx - 1) - x0, dtype=np.int64), np.arange(ny - 1, dtype=np.int64), indexing="ij")
        place = place.astype(np.uint32)
        a, b, c, d = (place[v.reshape(-1)] for v in (ci * ny + cj, (ci + 1) * ny + cj, ci * ny + cj + 1, (ci + 1) * ny + cj + 1))
        del ci, cj
        tris = np.concatenate([np.stack([a, b, c], -1), np.stack([b, d, c], -1)])
        parts.append((np.ascontiguousarray(xyz), np.ascontiguousarray(rgb), tris, np.ascontiguousarray(keys), (x0, 0, 0), (x1, ny, 64)))
    return parts, L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=53_000_000, help="vertices of the welded mesh (a small number rehearses)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parts", type=str, default="2,8")
    ap.add_argument("--out", type=str, default=None, help="also write the result to this file")
    args = ap.parse_args()
    assert args.reps >= 3, "at least three repetitions"
    import numpy as np
    import torch
    import tl3d
    from tl3d import pipeline as pl

    nx = ny = max(16, int(round(args.vertices ** 0.5)))
    ctx = tl3d.FusionContext(64, 48, 50.0, 50.0, 32.0, 24.0, n_slots=1, grid=None, device=0)
    base = sheet(np, nx, ny)
    lines = [f"sheet {nx} x {ny}: {nx * ny} vertices, {2 * (nx - 1) * (ny - 1)} triangles; whole calls, host clock, device synchronised inside;",
             f"one warm-up, then {args.reps} rounds taking host and device in turn; seconds as median (smallest .. largest)"]
    header = ("# tools/bench_mesh_weld.py: the device weld of keyed block meshes against lattice.weld_meshes (DESIGN.md section 7.9)\n"
              f"# MI355X, --vertices {args.vertices} --reps {args.reps} --parts {args.parts}\n")

    def report(first):
        """the lines from `first` on, to the terminal and (the whole text so far) to --out: a cut's figures survive a later one"""
        print("\n".join(lines[first:]), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(header + "\n".join(lines) + "\n")
    report(0)

    def same(a, b):
        return all(np.asarray(x).dtype == np.asarray(y).dtype and np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for n_parts in [int(v) for v in args.parts.split(",")]:
        print(f"[{n_parts} parts: building the sheet]", flush=True)
        parts, L = sheet_parts(np, nx, ny, n_parts, base=base)
        first = len(lines)
        v_in = sum(len(p[0]) for p in parts)
        dparts = [(torch.from_numpy(x).cuda(), torch.from_numpy(r).cuda(), torch.from_numpy(t.view(np.int32)).cuda(), torch.from_numpy(k).cuda(),
                   lo, hi) for x, r, t, k, lo, hi in parts]
        runs = dict(host=lambda: pl.weld_meshes(parts, L), device_host_arrays=lambda: ctx.weld_meshes(parts, L),
                    device_tensors=lambda: ctx.weld_meshes(dparts, L))
        ref = None
        for name, fn in runs.items():                                       # warm-up, and the bytes
            _, out = timed(fn)
            if name == "device_tensors":
                out = (out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy().view(np.uint32), out[3].cpu().numpy())
            if ref is None:
                ref = out
            assert same(out, ref), f"{name} differs from the host weld ({n_parts} parts)"
            print(f"[{n_parts} parts: {name} warmed up, bytes equal]", flush=True)
            del out
        times = {name: [] for name in runs}
        for _ in range(args.reps):
            for name, fn in runs.items():
                dt, out = timed(fn)
                times[name].append(dt)
                del out
        lines.append(f"{n_parts} parts: {v_in} vertices in, {len(ref[0])} kept, {len(ref[2])} triangles; device = host bytes: yes")
        for name, ts in times.items():
            ts = sorted(ts)
            lines.append(f"  {name:<20s} {ts[len(ts) // 2]:8.3f} s  ({ts[0]:.3f} .. {ts[-1]:.3f})")
        med = {name: sorted(ts)[len(ts) // 2] for name, ts in times.items()}
        lines.append(f"  host / device: {med['host'] / med['device_host_arrays']:.1f} x with host arrays, "
                     f"{med['host'] / med['device_tensors']:.1f} x with device tensors")
        report(first)
        del parts, dparts, ref
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
