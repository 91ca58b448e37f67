"""Device time of vsg_render_boundary_distance and vsg_render_boundary_benchmark.

    python tools/boundary_distance_probe.py [--reps 20] [--warmup 5] [--sizes 1920x1080,3840x2160]
                                            [--inputs checker,noise,grid12,corner] [--heights 1,5,20]
                                            [--tolerance_sq 25] [--out profiles/boundary_distance.json]

Everything is in device memory.  The inputs: a checker-like (synth.bench_frame) and a value-noise
(synth.noise_frame) frame of the dense over-segmentation; `grid12`, 48 blocks that a top level merges into 12
regions; `corner`, one region but for the last pixel, the row pass's longest searches.  Every desc gets a
hierarchy of L levels for each L of --heights (level l + 1 merges the regions of level l in pairs while more
than 12 are left), a handle of its own, and as ground truth its own level-0 id image moved by (3, 4), the first row
and column repeated into the border.

Per desc and L: vsg_render_boundary_distance at level 0 and at the top level, and vsg_render_boundary_benchmark,
each with the stage times and the launches of vsg_render_distance_stats and the call's wall time; medians over
the repetitions after a warm-up, with the 10th and 90th percentile as the spread.  Measured against, in the same
run, on the same handle and desc, alternating with it: `per_level`, the route without the benchmark call, L calls
of vsg_render_boundary_distance with the two thresholds and sums of every level in torch on the device
(seg_edges and gt_matched; seg_matched would need the ground truth's distance transform on top).
benchmark_over_per_level compares the wall times.

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


def dense_desc(vsg, synth, frame_fn, W, H):
    """The first frame of a dense over-segmentation, rasters only."""
    N = 2
    fl = synth.const_flow(W, H)
    d = vsg.DenseSegmentation(W, H, vsg.default_options(chunk_size=20), has_flow=True)
    segs = []
    for k in range(N):
        n = d.process_frame(frame_fn(W, H, k), fl if k > 0 else None, flush=(k == N - 1))
        segs += [d.result_bytes(i) for i in range(n)]
    d.close()
    return segs[0]


def plane_desc(lc, ids):
    return lc.desc_from_ids(ids).SerializeToString()


def with_height(Msg, lc, seg, L):
    """The desc with a hierarchy of L levels: level 1 numbers the regions by rank and merges them in pairs, every
    further level merges pairs again; a level of 12 regions or fewer is repeated as it is."""
    m = Msg()
    m.ParseFromString(seg)
    ids = sorted({r.id for r in m.region})
    maps = []
    if L > 1:
        step = 2 if len(ids) > 12 else 1
        maps.append({rid: k // step for k, rid in enumerate(ids)})
        n = (len(ids) + step - 1) // step
        for _ in range(L - 2):
            step = 2 if n > 12 else 1
            maps.append({k: k // step for k in range(n)})
            n = (n + step - 1) // step
    lc.add_hierarchy(m, maps)
    return m.SerializeToString()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--inputs", default="checker,noise,grid12,corner")
    ap.add_argument("--heights", default="1,5,20")
    ap.add_argument("--tolerance_sq", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_distance.json"))
    args = ap.parse_args()

    import torch
    import level_regions_cases as lc
    import synth
    import video_segment_amd as vsg
    from video_segment_amd import _lib, render
    if _lib.lib().vsg_device_count() <= 0:
        sys.exit("boundary_distance_probe needs a HIP device: a time from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    T = args.tolerance_sq
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "tolerance_sq": T, "cases": []}
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        for kind in args.inputs.split(","):
            t0 = time.perf_counter()
            if kind == "grid12":
                yy, xx = np.mgrid[0:H, 0:W]
                seg = plane_desc(lc, (8 * (yy * 6 // H) + xx * 8 // W).astype(np.int32))
            elif kind == "corner":
                ids = np.ones((H, W), np.int32)
                ids[H - 1, W - 1] = 0
                seg = plane_desc(lc, ids)
            else:
                seg = dense_desc(vsg, synth, {"checker": synth.bench_frame, "noise": synth.noise_frame}[kind], W, H)
            print("%s %s: desc in %.1f s" % (size, kind, time.perf_counter() - t0), flush=True)
            for L in (int(v) for v in args.heights.split(",")):
                if kind == "grid12" and L not in (1, 3):
                    L = 3                                   # 48 blocks, 24, 12 regions
                desc = with_height(lc.Msg, lc, seg, L)
                r = vsg.SegmentationRenderer(W, H, has_video=False)   # a handle of its own: no kept hierarchy
                ids0 = torch.empty((H, W), dtype=torch.int32, device=dev)
                r.id_image(desc, 0, out=ids0)
                ys = torch.clamp(torch.arange(H, device=dev) - 4, min=0)
                xs = torch.clamp(torch.arange(W, device=dev) - 3, min=0)
                other = ids0[ys][:, xs].contiguous()          # the first row and column repeated, as the tests do
                other_edges = torch.zeros((H, W), dtype=torch.bool, device=dev)
                other_edges[:, :-1] |= other[:, :-1] != other[:, 1:]
                other_edges[:-1] |= other[:-1] != other[1:]
                plane = torch.empty((H, W), dtype=torch.int32, device=dev)
                scores = torch.empty((L, render.BOUNDARY_SCORE_WORDS), dtype=torch.int64, device=dev)
                stage_keys = ["plane_us", "classify_us", "columns_us", "rows_us", "match_us"]
                legs = {"distance_level0": lambda: r.boundary_distance(desc, 0, out=plane),
                        "distance_top": lambda: r.boundary_distance(desc, L - 1, out=plane),
                        "benchmark": lambda: r.boundary_benchmark(desc, other, T, out=scores)}

                def per_level():
                    out = []
                    for l in range(L):
                        r.boundary_distance(desc, l, out=plane)
                        out.append(((plane == 0).sum(), ((plane <= T) & other_edges).sum()))
                    return [(int(a), int(b)) for a, b in out]

                rows, counts = {}, {}
                for it in range(args.warmup + args.reps):
                    for name, call in legs.items():
                        t0 = time.perf_counter()
                        call()
                        st = dict(r.last_distance_stats(), call_ms=(time.perf_counter() - t0) * 1e3)
                        counts[name] = {k: st[k] for k in ("levels", "edge_pixels", "other_edge_pixels", "max_distance",
                                                           "launches")}
                        if it >= args.warmup:
                            for k in stage_keys + ["call_ms"]:
                                rows.setdefault(name + "_" + k, []).append(st[k])
                    t0 = time.perf_counter()
                    levels = per_level()
                    if it >= args.warmup:
                        rows.setdefault("per_level_call_ms", []).append((time.perf_counter() - t0) * 1e3)
                got = scores.cpu().numpy()
                assert [(int(a), int(b)) for a, b in zip(got[:, 0], got[:, 3])] == levels, (got, levels)
                med = {k: pct(v) for k, v in rows.items()}
                case = {"size": size, "input": kind, "hierarchy_levels": L, "counts": counts,
                        "benchmark_over_per_level": med["benchmark_call_ms"]["median"] / med["per_level_call_ms"]["median"]}
                case.update({k: dict(v, unit=k.rsplit("_", 1)[1]) for k, v in med.items()})
                result["cases"].append(case)
                print(json.dumps(case), flush=True)
                with open(args.out, "w") as f:
                    json.dump(result, f, indent=1)
                    f.write("\n")
                r.close()
                if kind == "grid12" and L == 3:
                    break
    print("wrote", args.out)


if __name__ == "__main__":
    main()
