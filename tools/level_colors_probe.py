"""Device time of the colour stages of vsg_render_level_colors and vsg_render_mean_frame.

    python tools/level_colors_probe.py [--reps 60] [--warmup 10] [--sizes 1920x1080,3840x2160]
                                       [--inputs checker,noise] [--out profiles/level_colors.json]

For every size, on a checker-like (synth.bench_frame) and a many-region (synth.noise_frame) chunk result of
the dense over-segmentation given a hierarchy by RegionSegmentation, at level 0 and at the top level, of the
regions (connectedness 0) and of their N4 components: vsg_render_level_colors (frame and table in device
memory) with the stage times of vsg_render_color_stats, and vsg_render_mean_frame (picture in device memory)
with its paint stage.  HIP events on the handle's stream; medians over the repetitions after a warm-up, with
the 10th and 90th percentile as the spread.  Measured against, in the same run and on the same handle:

  vsg_render_level_regions on the same desc and level (outputs in device memory): the new call contains that
  pipeline up to its table, so colours_over_level_regions = (plane + sums + table) / (clear + fill + runs +
  sort + table + moments) is the price of the colour stages;

  a device-to-device copy of the bytes k_color_runs has to move, 3 per pixel read, 16 read and 32 written per
  interval (the copy reads half of them and writes half): runs_over_copy = sums_us / copy_us.

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


def pct(values):
    a = np.asarray(values, np.float64)
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90))}


def chunk_result(vsg, synth, frame_fn, W, H):
    """(a dense-unit desc that carries a hierarchy, its height, its frame)."""
    from test_proto_wire import build_schema
    N = 3
    fl = synth.const_flow(W, H)
    frames = [frame_fn(W, H, k) for k in range(N)]
    d = vsg.DenseSegmentation(W, H, vsg.default_options(chunk_size=20), has_flow=True)
    reg = vsg.RegionSegmentation(W, H, vsg.default_region_options())
    over, segs = [], []
    for k in range(N):
        n = d.process_frame(frames[k], fl if k > 0 else None, flush=(k == N - 1))
        over += [d.result_bytes(i) for i in range(n)]
    for k, seg in enumerate(over):
        n = reg.process_frame(seg, frames[k], fl if k > 0 else None, flush=(k == N - 1))
        segs += [reg.result_bytes(i) for i in range(n)]
    d.close()
    reg.close()
    m = build_schema()()
    m.ParseFromString(segs[0])          # the chunk's first frame carries the hierarchy
    return segs[0], len(m.hierarchy), frames[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--inputs", default="checker,noise")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level_colors.json"))
    args = ap.parse_args()

    import torch
    import synth
    import video_segment_amd as vsg
    from video_segment_amd import _lib, render
    if _lib.lib().vsg_device_count() <= 0:
        sys.exit("level_colors_probe needs a HIP device: a time from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "cases": []}
    generators = {"checker": synth.bench_frame, "noise": synth.noise_frame}
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        px = W * H
        for kind in args.inputs.split(","):
            t0 = time.perf_counter()
            seg, height, frame = chunk_result(vsg, synth, generators[kind], W, H)
            print("%s %s: chunk result in %.1f s, %d levels" % (size, kind, time.perf_counter() - t0, height), flush=True)
            d_frame = torch.from_numpy(frame).to(dev)
            picture = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
            r = vsg.SegmentationRenderer(W, H)
            for level in sorted({0, max(height - 1, 0)}):
                nr, ni = (len(a) for a in r.level_regions(seg, level))
                regions = torch.empty((nr, render.LEVEL_REGION_WORDS), dtype=torch.int32, device=dev)
                intervals = torch.empty((ni, 4), dtype=torch.int32, device=dev)
                # the copy moving the bytes of k_color_runs: half of them read, half written
                moved = 3 * px + (16 + 32) * ni
                src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
                dst = torch.empty_like(src)
                for mode, connect in (("regions", 0), ("components_N4", render.N4)):
                    n = len(r.level_colors(seg, level, d_frame, connect))
                    table = torch.empty((n, render.LEVEL_COLOR_WORDS), dtype=torch.int32, device=dev)
                    keys = ["plane_us", "sums_us", "table_us", "paint_us", "call_ms", "mean_frame_call_ms",
                            "level_regions_us", "level_regions_call_ms", "copy_us"]
                    rows = {k: [] for k in keys}
                    for it in range(args.warmup + args.reps):
                        t0 = time.perf_counter()
                        r.level_colors(seg, level, d_frame, connect, colors_out=table)
                        st = dict(r.last_color_stats(), call_ms=(time.perf_counter() - t0) * 1e3)
                        t0 = time.perf_counter()
                        r.mean_frame(seg, level, d_frame, connect, out=picture)
                        st["mean_frame_call_ms"] = (time.perf_counter() - t0) * 1e3
                        st["paint_us"] = r.last_color_stats()["paint_us"]
                        t0 = time.perf_counter()
                        r.level_regions(seg, level, regions_out=regions, intervals_out=intervals)
                        st["level_regions_call_ms"] = (time.perf_counter() - t0) * 1e3
                        ls, rs = r.last_level_stats(), r.last_stats()
                        st["level_regions_us"] = (rs["clear_us"] + rs["fill_us"] + ls["runs_us"] + ls["sort_us"]
                                                  + ls["table_us"] + ls["moments_us"])
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        dst.copy_(src)
                        e1.record()
                        e1.synchronize()
                        st["copy_us"] = e0.elapsed_time(e1) * 1e3
                        if it >= args.warmup:
                            for k in keys:
                                rows[k].append(st[k])
                    med = {k: pct(v) for k, v in rows.items()}
                    colours_us = med["plane_us"]["median"] + med["sums_us"]["median"] + med["table_us"]["median"]
                    case = {"size": size, "input": kind, "level": level, "hierarchy_levels": height, "mode": mode,
                            "groups": st["groups"], "intervals": st["intervals"], "covered": st["covered"],
                            "largest_group_intervals": st["largest_group_intervals"], "launches": st["launches"],
                            "runs_bytes_moved": moved,
                            "runs_GBps": moved / med["sums_us"]["median"] / 1e3,
                            "copy_GBps": moved / med["copy_us"]["median"] / 1e3,
                            "colours_over_level_regions": colours_us / med["level_regions_us"]["median"],
                            "runs_over_copy": med["sums_us"]["median"] / med["copy_us"]["median"]}
                    case.update({k: dict(v, unit=k.rsplit("_", 1)[1]) for k, v in med.items()})
                    result["cases"].append(case)
                    print(json.dumps(case), flush=True)
                    with open(args.out, "w") as f:
                        json.dump(result, f, indent=1)
                        f.write("\n")
            r.close()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
