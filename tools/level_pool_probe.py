"""Device time of the stages of vsg_render_level_pool.

    python tools/level_pool_probe.py [--reps 60] [--warmup 10] [--size 1920x1080] [--inputs checker,noise]
                                     [--channels 1,4,16,64] [--index_add_reps 3]
                                     [--out profiles/level_pool.json]

On the checker-like (synth.bench_frame) and the many-region (synth.noise_frame) chunk results that
tools/level_colors_probe.py uses, at level 0 and at the top level, connectedness 0: vsg_render_level_pool of C
channels, f32 and bf16, planar and channels-last, features and outputs in device memory, once for the sum alone
and once for all four statistics, with the stage times of vsg_render_pool_stats.  HIP events on the handle's
stream; medians over the repetitions after a warm-up, with the 10th and 90th percentile as the spread.  Measured
against, in the same run and on the same handle:

  a device-to-device copy of the bytes the sums stage has to move (feature_bytes, half of them read and half
  written by the copy): sums_over_copy = sums_us / copy_us;

  what a user writes today: torch index_add_ of the float64 features over the dense record plane (the plane is
  vsg_render_level_unpool of the record numbers, made once and not timed; neither the conversion to a contiguous
  (H * W, C) float64 matrix nor the clear of the target is timed): call_over_index_add = call_ms / index_add_ms.
  It takes seconds per call at 64 channels and few groups, so it is repeated --index_add_reps times only.

No pass or fail threshold.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

ALL = ("sum", "sum_sq", "min", "max")


def pct(values):
    a = np.asarray(values, np.float64)
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--inputs", default="checker,noise")
    ap.add_argument("--channels", default="1,4,16,64")
    ap.add_argument("--index_add_reps", type=int, default=3,
                    help="index_add_ takes seconds per call at 64 channels: fewer of its repetitions shorten a run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level_pool.json"))
    args = ap.parse_args()

    import torch
    import synth
    import video_segment_amd as vsg
    from video_segment_amd import _lib
    from level_colors_probe import chunk_result
    if _lib.lib().vsg_device_count() <= 0:
        sys.exit("level_pool_probe needs a HIP device: a time from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    W, H = (int(v) for v in args.size.split("x"))
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "size": args.size,
              "cases": []}
    generators = {"checker": synth.bench_frame, "noise": synth.noise_frame}
    gen = torch.Generator(device=dev).manual_seed(1)
    for kind in args.inputs.split(","):
        t0 = time.perf_counter()
        seg, height, _ = chunk_result(vsg, synth, generators[kind], W, H)
        print("%s: chunk result in %.1f s, %d levels" % (kind, time.perf_counter() - t0, height), flush=True)
        r = vsg.SegmentationRenderer(W, H)
        for level in sorted({0, max(height - 1, 0)}):
            groups, _ = r.level_pool(seg, level, torch.zeros((1, H, W), device=dev), 0, ())
            R = len(groups)
            numbers = torch.arange(R, dtype=torch.float32, device=dev).reshape(R, 1)
            assert R < 1 << 24
            plane = r.level_unpool(seg, level, numbers, 0, fill=float(R)).reshape(-1).to(torch.int64)
            for channels in (int(c) for c in args.channels.split(",")):
                base = torch.randn((channels, H, W), generator=gen, device=dev)
                f64 = base.to(torch.float64).reshape(channels, -1).t().contiguous()   # (HW, C), rows contiguous
                table = torch.zeros((R + 1, channels), dtype=torch.float64, device=dev)
                for kind_name, kind_t in (("f32", torch.float32), ("bf16", torch.bfloat16)):
                    for layout in ("planar", "channels_last"):
                        x = base.to(kind_t)
                        if layout == "channels_last":
                            x = x.permute(1, 2, 0).contiguous().permute(2, 0, 1)
                        keys = ["plane_us", "sums_us", "table_us", "call_ms", "sums_all_us", "table_all_us",
                                "call_all_ms", "copy_us", "index_add_ms"]
                        rows = {k: [] for k in keys}
                        for it in range(args.warmup + args.reps):
                            t0 = time.perf_counter()
                            r.level_pool(seg, level, x, 0, ("sum",), capacity=R)
                            st = dict(r.last_pool_stats(), call_ms=(time.perf_counter() - t0) * 1e3)
                            t0 = time.perf_counter()
                            r.level_pool(seg, level, x, 0, ALL, capacity=R)
                            st["call_all_ms"] = (time.perf_counter() - t0) * 1e3
                            st_all = r.last_pool_stats()
                            st["sums_all_us"], st["table_all_us"] = st_all["sums_us"], st_all["table_us"]
                            moved = st["feature_bytes"]
                            src = torch.empty(max(moved // 2, 1), dtype=torch.uint8, device=dev)
                            dst = torch.empty_like(src)
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            dst.copy_(src)
                            e1.record()
                            e1.synchronize()
                            st["copy_us"] = e0.elapsed_time(e1) * 1e3
                            yardstick = it >= args.warmup + args.reps - args.index_add_reps
                            if yardstick:
                                table.zero_()
                                torch.cuda.synchronize()
                                t0 = time.perf_counter()
                                table.index_add_(0, plane, f64)
                                torch.cuda.synchronize()
                                st["index_add_ms"] = (time.perf_counter() - t0) * 1e3
                            if it >= args.warmup:
                                for k in keys:
                                    if k != "index_add_ms" or yardstick:
                                        rows[k].append(st[k])
                        med = {k: pct(v) for k, v in rows.items()}
                        case = {"input": kind, "level": level, "hierarchy_levels": height, "channels": channels,
                                "dtype": kind_name, "layout": layout, "groups": st["groups"],
                                "intervals": st["intervals"], "covered": st["covered"],
                                "largest_group_intervals": st["largest_group_intervals"],
                                "launches": st["launches"], "feature_bytes": moved,
                                "sums_GBps": moved / med["sums_us"]["median"] / 1e3,
                                "copy_GBps": moved / med["copy_us"]["median"] / 1e3,
                                "sums_over_copy": med["sums_us"]["median"] / med["copy_us"]["median"],
                                "sums_all_over_copy": med["sums_all_us"]["median"] / med["copy_us"]["median"],
                                "call_over_index_add": med["call_ms"]["median"] / med["index_add_ms"]["median"]}
                        case.update({k: dict(v, unit=k.rsplit("_", 1)[1]) for k, v in med.items()})
                        result["cases"].append(case)
                        print(json.dumps({k: case[k] for k in ("input", "level", "channels", "dtype", "layout",
                                                               "groups", "intervals", "sums_over_copy",
                                                               "sums_all_over_copy", "call_over_index_add")}
                                         | {"sums_us": med["sums_us"]["median"], "copy_us": med["copy_us"]["median"],
                                            "call_ms": med["call_ms"]["median"],
                                            "index_add_ms": med["index_add_ms"]["median"]}), flush=True)
                        with open(args.out, "w") as f:
                            json.dump(result, f, indent=1)
                            f.write("\n")
                del base, f64, table
        r.close()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
