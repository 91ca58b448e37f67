"""Device time of the dense flow unit next to a plain device-to-device copy.

    python tools/flow_probe.py [--reps 60] [--warmup 10] [--out profiles/flow_kernels.json]

For 1920x1080 and 3840x2160 on the moving value-noise pattern (flow_model.translated_pattern), frame
and flow in device memory, default options (2 warps, 10 iterations): ms per frame (wall clock of the
call and the sum of the stage times), the stages as vsg_flow_last_stats times them with HIP events on
the handle's stream, launches per frame, and for the iteration kernel its algorithmic bytes per pixel
(from shapes: reads g 16 + u 8 + Px 8 + Py 8, writes u 8 + Px 8 + Py 8 = 64; neighbours and the apron
come from cache), its time per executed iteration over all scales and its GB/s.  In the same run a
device-to-device copy moving as many bytes as one full-resolution iteration (32 per pixel read, 32
written) is timed with torch events.  Medians over the repetitions after a warm-up, with the 10th and
90th percentile as the spread.  Not a test; no threshold.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ITER_BYTES_PER_PIXEL = 64
DENSE_UNIT_MS_1080P = 4.9   # BENCH_r06: the dense unit's time per 1080p frame


def pct(values):
    a = np.asarray(values, np.float64)
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_kernels.json"))
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    args = ap.parse_args()

    import torch
    import flow_model as fm
    from video_segment_amd import _lib, flow
    if _lib.lib().vsg_device_count() <= 0:
        sys.exit("flow_probe needs a HIP device: a time from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "cases": []}
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        px = W * H
        sizes = fm.pyramid_sizes(W, H)
        # 8 distinct frames of the moving pattern, cycled (the wrap-around pair is one more motion)
        frames = [torch.from_numpy(fm.gray_to_bgr(g)).to(dev) for g in fm.translated_pattern(W, H, 8, seed=7)]
        src = torch.empty(ITER_BYTES_PER_PIXEL // 2 * px, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        d = flow.DenseFlow(W, H)
        keys = ("pyramid_us", "warp_us", "iterate_us", "export_us")
        rows = {k: [] for k in keys + ("call_ms", "device_ms", "copy_us", "iter_us_each", "iter_GBps")}
        st = None
        for it in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            out = d.process_frame_device(frames[it % len(frames)])
            call_ms = (time.perf_counter() - t0) * 1e3
            st = d.last_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            e1.synchronize()
            if it >= args.warmup and out is not None:
                for k in keys:
                    rows[k].append(st[k])
                rows["call_ms"].append(call_ms)
                rows["device_ms"].append(sum(st[k] for k in keys) / 1e3)
                rows["copy_us"].append(e0.elapsed_time(e1) * 1e3)
                # every scale runs the same number of launches; executed ones may be fewer
                per_scale = st["iterations_run"] / float(len(sizes))
                moved = sum(w * h for w, h in sizes) * per_scale * ITER_BYTES_PER_PIXEL
                rows["iter_us_each"].append(st["iterate_us"] / max(st["iterations_run"], 1))
                rows["iter_GBps"].append(moved / st["iterate_us"] / 1e3)
        d.close()
        med = {k: pct(v) for k, v in rows.items()}
        case = {
            "size": size, "scales": st["scales"], "launches_per_frame": st["launches"],
            "iterations_run_last_frame": st["iterations_run"], "host_syncs": st["host_syncs"],
            "call_wall_ms": med["call_ms"], "device_ms": med["device_ms"],
            "stages_us": {k: med[k] for k in keys},
            "iterate": dict(med["iter_us_each"], unit="us per executed iteration, mean over scales",
                            bytes_per_pixel=ITER_BYTES_PER_PIXEL, GBps=med["iter_GBps"]),
            "copy_same_bytes_as_one_full_iteration": dict(
                med["copy_us"], unit="us", bytes_per_pixel=ITER_BYTES_PER_PIXEL,
                GBps=ITER_BYTES_PER_PIXEL * px / med["copy_us"]["median"] / 1e3),
        }
        if size == "1920x1080":
            case["dense_unit_ms_per_frame"] = DENSE_UNIT_MS_1080P
            case["flow_bound"] = med["device_ms"]["median"] > DENSE_UNIT_MS_1080P
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
