"""Device time of the stages of vsg_render_level_contours.

    python tools/level_contours_probe.py [--reps 40] [--warmup 8] [--sizes 1920x1080,3840x2160]
                                         [--inputs checker,noise] [--out profiles/level_contours.json]

For every size, on a checker-like (synth.bench_frame) and a many-region (synth.noise_frame) chunk result of
the dense over-segmentation given a hierarchy by RegionSegmentation, at level 0 and at the top level, of the
regions (connectedness 0) and of their N4 components: vsg_render_level_contours (both lists in device memory)
with the four stage times, the rounds, the launches and the counts of vsg_render_contour_stats, and the
call's wall time.  HIP events on the handle's stream; medians over the repetitions after a warm-up, with the
10th and 90th percentile as the spread.  Measured against, in the same run, on the same handle and input,
alternating with it:

  vsg_render_level_boundaries (inner points, same connectedness, outputs in device memory), the nearest
  sibling: it makes the same plane and classifies, sorts and tabulates one key per boundary pixel.
  contours_over_boundaries = (classify + trace + table) / (count + emit + sort + table) compares the device
  time after the plane, call_over_boundaries_call the wall times.

  per_round_us = trace_us / rounds, and the bytes a doubling round moves (a launch does two rounds: 32 read,
  8 written per crack) over it: what the random gathers of the doubling achieve.

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
    """(a dense-unit desc that carries a hierarchy, its height)."""
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
    return segs[0], len(m.hierarchy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--inputs", default="checker,noise")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level_contours.json"))
    args = ap.parse_args()

    import torch
    import synth
    import video_segment_amd as vsg
    from video_segment_amd import _lib, render
    if _lib.lib().vsg_device_count() <= 0:
        sys.exit("level_contours_probe needs a HIP device: a time from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "cases": []}
    generators = {"checker": synth.bench_frame, "noise": synth.noise_frame}
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        for kind in args.inputs.split(","):
            t0 = time.perf_counter()
            seg, height = chunk_result(vsg, synth, generators[kind], W, H)
            print("%s %s: chunk result in %.1f s, %d levels" % (size, kind, time.perf_counter() - t0, height), flush=True)
            r = vsg.SegmentationRenderer(W, H, has_video=False)
            for level in sorted({0, max(height - 1, 0)}):
                for mode, connect in (("regions", 0), ("components_N4", render.N4)):
                    nc, nv = (len(a) for a in r.level_contours(seg, level, connect))
                    nb, npts = (len(a) for a in r.level_boundaries(seg, level, connect))
                    contours = torch.empty((nc, render.LEVEL_CONTOUR_WORDS), dtype=torch.int32, device=dev)
                    vertices = torch.empty((nv, 2), dtype=torch.int32, device=dev)
                    records = torch.empty((nb, render.LEVEL_BOUNDARY_WORDS), dtype=torch.int32, device=dev)
                    points = torch.empty((npts, 2), dtype=torch.int32, device=dev)
                    keys = ["plane_us", "classify_us", "trace_us", "table_us", "call_ms", "boundaries_us",
                            "boundaries_plane_us", "boundaries_call_ms"]
                    rows = {k: [] for k in keys}
                    for it in range(args.warmup + args.reps):
                        t0 = time.perf_counter()
                        r.level_contours(seg, level, connect, contours_out=contours, vertices_out=vertices)
                        st = dict(r.last_contour_stats(), call_ms=(time.perf_counter() - t0) * 1e3)
                        t0 = time.perf_counter()
                        r.level_boundaries(seg, level, connect, boundaries_out=records, points_out=points)
                        st["boundaries_call_ms"] = (time.perf_counter() - t0) * 1e3
                        bs = r.last_boundary_stats()
                        st["boundaries_us"] = bs["count_us"] + bs["emit_us"] + bs["sort_us"] + bs["table_us"]
                        st["boundaries_plane_us"] = bs["plane_us"]
                        if it >= args.warmup:
                            for k in keys:
                                rows[k].append(st[k])
                    med = {k: pct(v) for k, v in rows.items()}
                    after_plane = sum(med[k]["median"] for k in ("classify_us", "trace_us", "table_us"))
                    per_round = med["trace_us"]["median"] / st["rounds"] if st["rounds"] else 0.0
                    case = {"size": size, "input": kind, "level": level, "hierarchy_levels": height, "mode": mode,
                            "cracks": st["cracks"], "vertices": st["vertices"], "contours": st["contours"],
                            "holes": st["holes"], "largest_contour_cracks": st["largest_contour_cracks"],
                            "rounds": st["rounds"], "launches": st["launches"],
                            "boundary_points": bs["points"], "boundaries_launches": bs["launches"],
                            "per_round_us": per_round,
                            "round_GBps": 20 * st["cracks"] / per_round / 1e3 if per_round else 0.0,
                            "contours_over_boundaries": after_plane / med["boundaries_us"]["median"],
                            "call_over_boundaries_call": med["call_ms"]["median"] / med["boundaries_call_ms"]["median"]}
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
