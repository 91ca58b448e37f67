"""Device time of the downscale stage next to a plain device-to-device copy.

    python tools/resize_probe.py [--reps 60] [--warmup 10] [--out profiles/resize_kernels.json]

For 1920x1080 and 3840x2160 to 640x360 (TO_MIN_SIZE 360, the --run_on_server shape) on noise frames,
frame and result in device memory: the two kernels as vsg_resize_last_stats times them with HIP events
on the handle's stream, the wall clock of the call, and each kernel's algorithmic bytes (from shapes:
k_resize_h reads in_w*in_h*3 and writes out_w*3*4*in_h, k_resize_v reads that once and writes
out_w*out_h*3; table reads and the re-reads of intermediate rows come from cache) over its time.  In
the same run a device-to-device copy moving the same total bytes (half read, half written) is timed
with torch events, and the host-memory variant (numpy in and out: upload, kernels, download) with its
stage times.  Medians over the repetitions after a warm-up, with the 10th and 90th percentile as the
spread.  Not a test; no threshold.
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


def pct(values):
    a = np.asarray(values, np.float64)
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_kernels.json"))
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    args = ap.parse_args()

    import torch
    from video_segment_amd import _lib, resize
    if _lib.lib().vsg_device_count() <= 0:
        sys.exit("resize_probe needs a HIP device: a time from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "cases": []}
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(W)
        host_frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(4)]
        frames = [torch.from_numpy(f).to(dev) for f in host_frames]
        d = resize.Downscaler(W, H, mode=resize.DOWNSCALE_TO_MIN_SIZE, size=360)
        ow, oh = d.out_size
        bytes_h = {"read": W * H * 3, "written": ow * 3 * 4 * H}
        bytes_v = {"read": ow * 3 * 4 * H, "written": ow * oh * 3}
        total = sum(bytes_h.values()) + sum(bytes_v.values())
        src = torch.empty(total // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        keys = ("horizontal_us", "vertical_us")
        host_keys = ("upload_us", "horizontal_us", "vertical_us", "download_us")
        rows = {k: [] for k in keys + ("call_ms", "copy_us", "host_call_ms") + tuple("host_" + k for k in host_keys)}
        st = None
        for it in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            d.process_frame_device(frames[it % len(frames)])
            call_ms = (time.perf_counter() - t0) * 1e3
            st = d.last_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            e1.synchronize()
            t0 = time.perf_counter()
            d.process_frame(host_frames[it % len(host_frames)])
            host_call_ms = (time.perf_counter() - t0) * 1e3
            hst = d.last_stats()
            if it >= args.warmup:
                for k in keys:
                    rows[k].append(st[k])
                for k in host_keys:
                    rows["host_" + k].append(hst[k])
                rows["call_ms"].append(call_ms)
                rows["host_call_ms"].append(host_call_ms)
                rows["copy_us"].append(e0.elapsed_time(e1) * 1e3)
        d.close()
        med = {k: pct(v) for k, v in rows.items()}
        copy_gbps = total / med["copy_us"]["median"] / 1e3

        def kernel(name, nbytes):
            gbps = sum(nbytes.values()) / med[name]["median"] / 1e3
            return dict(med[name], unit="us", bytes=nbytes, GBps=gbps, share_of_copy_rate=gbps / copy_gbps)

        host_stage = {k: med["host_" + k] for k in host_keys}
        others = sum(host_stage[k]["median"] for k in host_keys if k != "upload_us")
        case = {
            "size": size, "out_size": "%dx%d" % (ow, oh), "taps_h": st["taps_h"], "taps_v": st["taps_v"],
            "launches_per_frame": st["launches"], "host_syncs": st["host_syncs"],
            "device_allocations": st["device_allocations"],
            "call_wall_ms": med["call_ms"],
            "k_resize_h": kernel("horizontal_us", bytes_h),
            "k_resize_v": kernel("vertical_us", bytes_v),
            "copy_same_total_bytes": dict(med["copy_us"], unit="us", bytes=total, GBps=copy_gbps),
            "host_memory_variant": {
                "call_wall_ms": med["host_call_ms"], "stages_us": host_stage,
                "upload_GBps": W * H * 3 / host_stage["upload_us"]["median"] / 1e3,
                "upload_bound": host_stage["upload_us"]["median"] > others,
            },
        }
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
