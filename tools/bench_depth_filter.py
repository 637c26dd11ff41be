"""The depth-frame filter on resident frames (tl3d_filter_depth_slots) against the time a plain copy of the same
images takes, and against the numpy / scipy reference on one frame.

--frames resident 1080 x 1920 frames: one render of synth.object_scene at that size through a 3 x 3 box blur (the ramps a depth
network leaves at every occlusion edge), shifted sideways by one column per frame; as f32 metres and as u16 millimetres; with the
default parameters (stage B off) and with --min-region (stage B on).  The filter is destructive, so every timed call is preceded by
an untimed re-upload of all frames from device tensors.  Timed by device events on the context's stream around ONE whole
filter_depth_slots call over all slots (no counts read back inside the window), after one warm-up call, [median, min] of --reps;
the copy (ONE hipMemcpyAsync device to device of the same f32 images, a [frames, H, W] tensor onto another, by device events on its
own stream) is timed in turn with the filter, in the same run.  floor_ms = the bytes of one read and one write of the filtered images at the copy's measured rate; the
passes' own traffic, from the shapes, is listed beside it (bytes_per_pixel).  The reference: wall clock of
tests/depth_filter_reference.py filter_shifted on frame 0, whose bytes the GPU's frame 0 must equal.
Prints one JSON line; --out FILE also writes it there behind a header (profiles/depth_filter.txt is made that way).

    python tools/bench_depth_filter.py [--frames 64] [--reps 20] [--min-region 200] [--out profiles/depth_filter.txt]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def box3(np, d):
    p = np.pad(d.astype(np.float64), 1, mode="edge")
    h, w = d.shape
    return (sum(p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0).astype(np.float32)


def traffic_bytes_per_pixel(kind_bytes, regions):
    """compulsory bytes per pixel of the passes, from the shapes alone (halo re-reads, the union-find's walks and the few zeros written
    come on top): support reads the image and writes the mask; init writes parent and size; hook reads mask, image and parent; count
    reads mask and parent and adds to size; apply reads the mask (and parent and size)"""
    b = kind_bytes + 1 + 1
    if regions:
        b += 8 + (1 + kind_bytes + 4) + (1 + 4) + (4 + 4)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--min-region", type=int, default=200)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import depth_filter_reference as dr
    import tl3d
    from tl3d import synth

    n, w, h = args.frames, args.width, args.height
    dev = torch.device("cuda", 0)
    f = 0.52 * w
    depth, _colour = synth.render(synth.object_scene(), synth.orbit_poses(1, 1.0, 2.0)[0], w, h, f, f, 0.5 * (w - 1), 0.5 * (h - 1))
    base = box3(np, depth)
    frames32 = [np.ascontiguousarray(np.roll(base, i, axis=1)) for i in range(n)]
    frames16 = [np.rint(a * 1000.0).astype(np.uint16) for a in frames32]
    d32 = [torch.from_numpy(a).to(dev) for a in frames32]
    d16 = [torch.from_numpy(a.view(np.int16)).to(dev) for a in frames16]
    npx = w * h
    src = torch.stack(d32)
    dst = torch.empty_like(src)

    def copy_ms():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    configs = [("f32", "A", d32, frames32, 0), ("f32", "A+B", d32, frames32, args.min_region),
               ("u16", "A", d16, frames16, 0), ("u16", "A+B", d16, frames16, args.min_region)]
    rows = []
    with tl3d.FusionContext(w, h, f, f, 0.5 * (w - 1), 0.5 * (h - 1), n_slots=n, grid=None) as ctx:
        slots = list(range(n))

        def upload(tensors):
            for i, t in enumerate(tensors):
                ctx.upload(i, t)

        def window(fn):
            ctx.sync()
            ctx.event_record(0)
            fn()
            ctx.event_record(1)
            return ctx.event_elapsed_ms()
        for kind, stages, tensors, host, min_region in configs:
            prm = dict(jump_rel=0.05, radius=1, min_support=4, min_region=min_region)
            upload(tensors)
            counts = ctx.filter_depth_slots(slots, **prm)                     # warm-up, and the counts
            first = ctx.download_depth(0)
            ctx.sync()
            copy_ms()
            filt, copy = [], []
            for _ in range(args.reps):                                        # in turn: copy, filter
                ctx.sync()
                copy.append(copy_ms())
                upload(tensors)
                filt.append(window(lambda: ctx.filter_depth_slots(slots, counts=False, **prm)))
            t0 = time.perf_counter()
            ref, ref_counts = dr.filter_shifted(host[0], **prm)
            ref_s = time.perf_counter() - t0
            want = ref if kind == "f32" else (ref.astype(np.float32) / np.float32(1000.0))
            same = bool(np.array_equal(first.view(np.uint32), want.view(np.uint32))) and counts[0].tolist() == ref_counts.tolist()
            kb = 4 if kind == "f32" else 2
            cp_ms = float(np.median(copy))
            rate = 2.0 * n * npx * 4 / (cp_ms * 1e-3) / 1e9                 # GB/s, read + write
            image_bytes = n * npx * (kb + (4 if kind == "u16" else 0))        # a u16 slot's f32 copy is zeroed with it, but only where a pixel goes
            floor_ms = 2.0 * n * npx * kb / (rate * 1e9) * 1e3
            bpp = traffic_bytes_per_pixel(kb, min_region > 1)
            med = float(np.median(filt))
            rows.append(dict(kind=kind, stages=stages, frames=n, width=w, height=h, **prm, filter_ms=[round(med, 3), round(float(np.min(filt)), 3)],
                             copy_f32_ms=[round(cp_ms, 3), round(float(np.min(copy)), 3)], copy_GBps=round(rate, 1), floor_ms=round(floor_ms, 3),
                             ratio_to_floor=round(med / floor_ms, 2), bytes_per_pixel=bpp, passes_traffic_ms=round(n * npx * bpp / (rate * 1e9) * 1e3, 3),
                             resident_image_MB=round(image_bytes / 1e6, 1), ms_per_frame=round(med / n, 4),
                             counts_total=counts.sum(axis=0).tolist(), reference_frame0_s=round(ref_s, 3), frame0_equals_reference=same,
                             speedup_over_reference=round(ref_s * 1e3 / (med / n), 0)))
    line = json.dumps(dict(reps=args.reps, configs=rows))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(f"# python tools/bench_depth_filter.py --frames {n} --reps {args.reps} --min-region {args.min_region}  (one MI355X; device events on the\n"
                     f"# context's stream, [median, min] of {args.reps} whole filter_depth_slots calls over all slots after one warm-up; the f32 copy in turn; the\n"
                     f"# reference: wall clock of numpy / scipy on frame 0; ms unless named)\n{line}\n")
    if not all(r["frame0_equals_reference"] for r in rows):
        sys.exit("frame 0 differs from the reference")


if __name__ == "__main__":
    main()
