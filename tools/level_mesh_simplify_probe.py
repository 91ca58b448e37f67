"""Device time of the stages of vsg_render_level_mesh_simplified.

    python tools/level_mesh_simplify_probe.py [--reps 40] [--warmup 8] [--sizes 1920x1080,3840x2160]
                                              [--inputs checker,noise] [--max_error 1.0] [--min_segment_points 4]
                                              [--out profiles/level_mesh_simplify.json]

The inputs of tools/level_mesh_probe.py: for every size, a checker-like (synth.bench_frame) and a many-region
(synth.noise_frame) chunk result of the dense over-segmentation given a hierarchy by RegionSegmentation, at
level 0 and at the top level, of the regions (connectedness 0) and of their N4 components.  Per input:
vsg_render_level_mesh_simplified at (max_error, min_segment_points), all four lists in device memory, with
dp_us, clean_us, table_us, the counts (vertices_in, vertices_kept, vertices_out, max_rounds, the longest
segment), the launches and the call's wall time.  HIP events on the handle's stream; medians over the
repetitions after a warm-up, with the 10th and 90th percentile as the spread.  Measured against, in the same
run, on the same handle and input, alternating with it:

  vsg_render_level_mesh (all four lists in device memory), whose stages the simplified call runs first:
  its split_us, table_us and wall time.  simplify_over_mesh_tables = (dp + clean + table) / the mesh call's
  (split + table) compares the added device time with the stages it is added to, call_over_mesh_call the wall
  times.

With --worst it adds the test suite's comb_8192 and long_zigzag_640 planes at max_error 0 and 0.5, where ties
make the recursion as deep as a segment is long: what a round costs when the rounds are many.

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

KEYS = ("dp_us", "clean_us", "table_us", "call_ms", "mesh_split_us", "mesh_table_us", "mesh_call_ms")
COUNTS = ("segments", "collapsed_segments", "vertices_in", "vertices_kept", "vertices_out", "single_vertex_closed",
          "longest_segment_vertices_in", "max_rounds", "launches")


def pct(values):
    a = np.asarray(values, np.float64)
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90))}


def measure(r, render, torch, dev, seg, level, connect, max_error, min_points, warmup, reps):
    """One input: the medians of the simplified call and of the mesh call alternating with it."""
    sizes = [len(a) for a in r.level_mesh(seg, level, connect)]
    widths = (render.MESH_SEGMENT_WORDS, 2, render.MESH_LOOP_WORDS, 0)
    outs = [torch.empty((n, w) if w else (n,), dtype=torch.int32, device=dev) for n, w in zip(sizes, widths)]
    rows = {k: [] for k in KEYS}
    st = ms = None
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        r.level_mesh_simplified(seg, level, connect, max_error, min_points, *outs)   # never longer than the mesh's
        row = {"call_ms": (time.perf_counter() - t0) * 1e3}
        st = r.last_simplify_stats()
        t0 = time.perf_counter()
        r.level_mesh(seg, level, connect, *outs)
        row["mesh_call_ms"] = (time.perf_counter() - t0) * 1e3
        ms = r.last_mesh_stats()
        row.update(dp_us=st["dp_us"], clean_us=st["clean_us"], table_us=st["table_us"],
                   mesh_split_us=ms["split_us"], mesh_table_us=ms["table_us"])
        if it >= warmup:
            for k in KEYS:
                rows[k].append(row[k])
    med = {k: pct(v) for k, v in rows.items()}
    added = sum(med[k]["median"] for k in ("dp_us", "clean_us", "table_us"))
    case = {"level": level, "mode": "regions" if connect == 0 else "components_N4", "max_error": max_error,
            "min_segment_points": min_points, "mesh_launches": ms["launches"], "cracks": ms["cracks"],
            "longest_segment_cracks": ms["longest_segment_cracks"],
            "simplify_over_mesh_tables": added / (med["mesh_split_us"]["median"] + med["mesh_table_us"]["median"]),
            "call_over_mesh_call": med["call_ms"]["median"] / med["mesh_call_ms"]["median"]}
    case.update({k: st[k] for k in COUNTS})
    case.update({k: dict(v, unit=k.rsplit("_", 1)[1]) for k, v in med.items()})
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--inputs", default="checker,noise")
    ap.add_argument("--max_error", type=float, default=1.0)
    ap.add_argument("--min_segment_points", type=int, default=4)
    ap.add_argument("--worst", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level_mesh_simplify.json"))
    args = ap.parse_args()

    import torch
    import synth
    import video_segment_amd as vsg
    from level_contours_probe import chunk_result
    from video_segment_amd import _lib, render
    if _lib.lib().vsg_device_count() <= 0:
        sys.exit("level_mesh_simplify_probe needs a HIP device: a time from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "cases": []}

    def record(case):
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    if args.worst:
        import level_mesh_simplify_cases as sc
        for c in (sc.long_zigzag(), sc.mc.tc.comb_8192()):
            r = vsg.SegmentationRenderer(c.W, c.H, has_video=False)
            for max_error in (0.0, 0.5, 1.0):
                case = measure(r, render, torch, dev, c.msg.SerializeToString(), 0, 0, max_error, 0, args.warmup,
                               args.reps)
                record(dict(case, size="%dx%d" % (c.W, c.H), input=c.name))
            r.close()
    generators = {"checker": synth.bench_frame, "noise": synth.noise_frame}
    for size in [s for s in args.sizes.split(",") if s]:
        W, H = (int(v) for v in size.split("x"))
        for kind in args.inputs.split(","):
            t0 = time.perf_counter()
            seg, height = chunk_result(vsg, synth, generators[kind], W, H)
            print("%s %s: chunk result in %.1f s, %d levels" % (size, kind, time.perf_counter() - t0, height), flush=True)
            r = vsg.SegmentationRenderer(W, H, has_video=False)
            for level in sorted({0, max(height - 1, 0)}):
                for connect in (0, render.N4):
                    case = measure(r, render, torch, dev, seg, level, connect, args.max_error,
                                   args.min_segment_points, args.warmup, args.reps)
                    record(dict(case, size=size, input=kind, hierarchy_levels=height))
            r.close()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
