"""Device time of the stages of vsg_render_level_mesh.

    python tools/level_mesh_probe.py [--reps 40] [--warmup 8] [--sizes 1920x1080,3840x2160]
                                     [--inputs checker,noise] [--out profiles/level_mesh.json]

For every size, on a checker-like (synth.bench_frame) and a many-region (synth.noise_frame) chunk result of
the dense over-segmentation given a hierarchy by RegionSegmentation, at level 0 and at the top level, of the
regions (connectedness 0) and of their N4 components: vsg_render_level_mesh (all four lists in device memory)
with the five stage times, the rounds, the launches and the counts of vsg_render_mesh_stats, and the call's
wall time.  HIP events on the handle's stream; medians over the repetitions after a warm-up, with the 10th
and 90th percentile as the spread.  Measured against, in the same run, on the same handle and input,
alternating with it:

  vsg_render_level_contours (same connectedness, both lists in device memory), whose stages the mesh call
  runs first.  mesh_over_contours = (classify + trace + split + table) / (classify + trace + table) compares
  the device time after the plane, call_over_contours_call the wall times.  The mesh adds a third doubling
  (split_us holds it with the junction bits and the halves) and the tables of the four lists, and a second
  wait for the host between them: split_over_trace = split_us / the contour call's trace_us says what the one
  doubling costs next to the contour call's two.

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


def pct(values):
    a = np.asarray(values, np.float64)
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--inputs", default="checker,noise")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level_mesh.json"))
    args = ap.parse_args()

    import torch
    import synth
    import video_segment_amd as vsg
    from level_contours_probe import chunk_result
    from video_segment_amd import _lib, render
    if _lib.lib().vsg_device_count() <= 0:
        sys.exit("level_mesh_probe needs a HIP device: a time from anywhere else says nothing")
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
                    ns, nv, nl, nr = (len(a) for a in r.level_mesh(seg, level, connect))
                    nc, ncv = (len(a) for a in r.level_contours(seg, level, connect))
                    outs = [torch.empty((ns, render.MESH_SEGMENT_WORDS), dtype=torch.int32, device=dev),
                            torch.empty((nv, 2), dtype=torch.int32, device=dev),
                            torch.empty((nl, render.MESH_LOOP_WORDS), dtype=torch.int32, device=dev),
                            torch.empty((nr,), dtype=torch.int32, device=dev)]
                    contours = torch.empty((nc, render.LEVEL_CONTOUR_WORDS), dtype=torch.int32, device=dev)
                    vertices = torch.empty((ncv, 2), dtype=torch.int32, device=dev)
                    keys = ["plane_us", "classify_us", "trace_us", "split_us", "table_us", "call_ms", "contours_us",
                            "contours_trace_us", "contours_plane_us", "contours_call_ms"]
                    rows = {k: [] for k in keys}
                    for it in range(args.warmup + args.reps):
                        t0 = time.perf_counter()
                        r.level_mesh(seg, level, connect, *outs)
                        st = dict(r.last_mesh_stats(), call_ms=(time.perf_counter() - t0) * 1e3)
                        t0 = time.perf_counter()
                        r.level_contours(seg, level, connect, contours_out=contours, vertices_out=vertices)
                        st["contours_call_ms"] = (time.perf_counter() - t0) * 1e3
                        ts = r.last_contour_stats()
                        st["contours_us"] = ts["classify_us"] + ts["trace_us"] + ts["table_us"]
                        st["contours_trace_us"] = ts["trace_us"]
                        st["contours_plane_us"] = ts["plane_us"]
                        if it >= args.warmup:
                            for k in keys:
                                rows[k].append(st[k])
                    med = {k: pct(v) for k, v in rows.items()}
                    after_plane = sum(med[k]["median"] for k in ("classify_us", "trace_us", "split_us", "table_us"))
                    case = {"size": size, "input": kind, "level": level, "hierarchy_levels": height, "mode": mode,
                            "rounds": st["rounds"], "launches": st["launches"], "contours_launches": ts["launches"],
                            "contours": ts["contours"], "contour_vertices": ts["vertices"],
                            "mesh_over_contours": after_plane / med["contours_us"]["median"],
                            "split_over_trace": med["split_us"]["median"] / med["contours_trace_us"]["median"],
                            "call_over_contours_call": med["call_ms"]["median"] / med["contours_call_ms"]["median"]}
                    case.update({k: st[k] for k in ("cracks", "segments", "closed_segments", "shared_segments",
                                                    "vertices", "loops", "refs", "junctions",
                                                    "longest_segment_cracks")})
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
