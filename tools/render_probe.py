"""Device time of the renderer's two kernels next to a plain device-to-device copy.

    python tools/render_probe.py [--reps 60] [--warmup 10] [--out profiles/render_kernels.json]

For 1920x1080 and 3840x2160, on a checker-like (synth.bench_frame) and a many-region
(synth.noise_frame) chunk result of the dense over-segmentation: k_render_fill and k_render_compose
are timed with HIP events on the handle's stream (vsg_render_last_stats), frame and output in device
memory, default options (edges, blend 0.5).  In the same run a device-to-device copy of 7 bytes per
pixel is timed with torch events: it reads and writes as many bytes as the two kernels have to move
(plane write 4 + plane read 4 + frame read 3 + frame write 3 = 14 per pixel).  Medians over the
repetitions after a warm-up, with the 10th and 90th percentile as the spread.

    python tools/render_probe.py --vector [--out profiles/vector_raster.json]

The vector leg: the same four chunk results computed with compute_vectorization, once as they are
(rasters: the path above) and once as the reference's writer leaves them (rasters cleared,
rasterization_removed set).  For the vector-only desc the three scan conversion stages (k_vec_walk,
radix sort, k_vec_pairs; vsg_render_last_vector_stats), host decode and upload and the fill are
recorded, for the desc with rasters decode, upload and fill: the yardstick beside them.

    python tools/render_probe.py --level-regions [--reps 30] [--out profiles/level_regions.json]

The level leg: a dense-unit chunk result given a hierarchy by RegionSegmentation, asked for its regions
(vsg_render_level_regions, outputs in device memory) at the lowest, a middle and the top level.  Per
call the four stage times of vsg_render_level_stats, the launch count and the runs of the frame are
recorded; in the same run vsg_render_id_image on the same desc and level is timed, which is what
painting the plane the answer is read from costs.  No pass or fail threshold.

    python tools/render_probe.py --level-components [--reps 30] [--out profiles/level_components.json]

The component leg: the same descs and levels asked for their connected components
(vsg_render_level_components, N4 and N8, lists and label image in device memory).  Per call the six
stage times of vsg_render_component_stats, launches, runs, links and components are recorded; in the
same run vsg_render_level_regions on the same desc and handle is timed with its four stage times: the
yardstick.  No pass or fail threshold.

    python tools/render_probe.py --level-boundaries [--reps 30] [--out profiles/level_boundaries.json]

The boundary leg: the same descs and levels asked for their boundary point lists
(vsg_render_level_boundaries, outputs in device memory): of the regions (connectedness 0) and of their N4
components, inner and outer.  Per call the five stage times of vsg_render_boundary_stats, launches, points
and boundaries are recorded; in the same run vsg_render_level_components (N4, lists and label image in
device memory) on the same desc and handle is timed with its six stage times: the yardstick.  No pass or
fail threshold.

    python tools/render_probe.py --level-adjacency [--reps 30] [--out profiles/level_adjacency.json]

The adjacency leg: the same descs and levels asked for their adjacency graph (vsg_render_level_adjacency,
outputs in device memory): of the regions (connectedness 0) and of their N4 components, with pixel sides
only (N4) and with diagonal contacts (N8).  Per call the five stage times of vsg_render_adjacency_stats,
launches, sides, keys, nodes, edges and the largest degree are recorded; in the same run
vsg_render_level_boundaries (inner, same connectedness, outputs in device memory) on the same desc and
handle is timed: a point of comparison, nothing more.  No pass or fail threshold.

    python tools/render_probe.py --level-overlap [--reps 30] [--out profiles/level_overlap.json]

The overlap leg: the same descs at their lowest and top level asked for their overlap table
(vsg_render_level_overlap, outputs in device memory) of the regions (connectedness 0) and of their N4
components, with the same level's id image shifted right by 8 pixels, in device memory, as the other plane.
Per call the five stage times of vsg_render_overlap_stats, launches, runs, rows, cols and pairs are recorded;
in the same run vsg_render_level_adjacency (N4 sides, same connectedness, outputs in device memory) on the
same desc and handle is timed: the yardstick, which makes the same plane, reads it twice and sorts.  No pass
or fail threshold.

    python tools/render_probe.py --persistence [--reps 30] [--out profiles/persistence.json]

The persistence leg: the same descs with their hierarchy cut to 1, 2, 5 and all of its levels, asked for the
persistence plane (vsg_render_persistence_image, device memory), the picture (vsg_render_persistence_frame,
source and picture in device memory) and the graph (vsg_render_persistence_graph, N4, device memory).  Per call
the stage times of vsg_render_persistence_stats and launches are recorded; in the same run, on the same handle
and desc, the yardstick for the same information: L calls of vsg_render_id_image, one per level, for the plane,
and L calls of vsg_render_level_adjacency, one per level, for the graph.  No pass or fail threshold.
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--vector", action="store_true", help="the vector leg instead (profiles/vector_raster.json)")
    ap.add_argument("--level-regions", action="store_true",
                    help="the level leg instead (profiles/level_regions.json)")
    ap.add_argument("--level-components", action="store_true",
                    help="the component leg instead (profiles/level_components.json)")
    ap.add_argument("--level-boundaries", action="store_true",
                    help="the boundary leg instead (profiles/level_boundaries.json)")
    ap.add_argument("--level-adjacency", action="store_true",
                    help="the adjacency leg instead (profiles/level_adjacency.json)")
    ap.add_argument("--level-overlap", action="store_true",
                    help="the overlap leg instead (profiles/level_overlap.json)")
    ap.add_argument("--persistence", action="store_true",
                    help="the persistence leg instead (profiles/persistence.json)")
    args = ap.parse_args()
    if ((args.level_regions or args.level_components or args.level_boundaries or args.level_adjacency
         or args.level_overlap or args.persistence) and "--reps" not in sys.argv):
        args.reps = 30
    if args.out is None:
        name = ("persistence.json" if args.persistence else
                "level_overlap.json" if args.level_overlap else
                "level_adjacency.json" if args.level_adjacency else
                "level_boundaries.json" if args.level_boundaries else
                "level_components.json" if args.level_components else "level_regions.json" if args.level_regions
                else "vector_raster.json" if args.vector else "render_kernels.json")
        args.out = os.path.join(ROOT, "profiles", name)

    import torch
    import synth
    import video_segment_amd as vsg
    from video_segment_amd import _lib
    if _lib.lib().vsg_device_count() <= 0:
        sys.exit("render_probe needs a HIP device: a time from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "cases": []}
    if args.vector:
        return vector_leg(args, result, dev)
    if args.persistence:
        return persistence_leg(args, result, dev)
    if args.level_overlap:
        return overlap_leg(args, result, dev)
    if args.level_adjacency:
        return adjacency_leg(args, result, dev)
    if args.level_boundaries:
        return boundaries_leg(args, result, dev)
    if args.level_components:
        return components_leg(args, result, dev)
    if args.level_regions:
        return level_leg(args, result, dev)
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        px = W * H
        # the copy moving the same bytes: 7 * px read + 7 * px written
        src = torch.empty(7 * px, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        for kind, frame_fn in (("checker", synth.bench_frame), ("noise", synth.noise_frame)):
            N = 3
            fl = torch.from_numpy(synth.const_flow(W, H)).to(dev)
            d = vsg.DenseSegmentation(W, H, vsg.default_options(chunk_size=20), has_flow=True)
            frames, segs = [], []
            for k in range(N):
                frames.append(torch.from_numpy(frame_fn(W, H, k)).to(dev))
                n = d.process_frame(frames[k], fl if k > 0 else None, flush=(k == N - 1))
                segs += [d.result_bytes(i) for i in range(n)]
            d.close()
            seg, frame = segs[1], frames[1]
            r = vsg.SegmentationRenderer(W, H)
            out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
            rows = {k: [] for k in ("clear_us", "fill_us", "compose_us", "decode_ms", "upload_ms", "call_ms", "copy_us")}
            for it in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                r.render(seg, frame, out=out)
                call_ms = (time.perf_counter() - t0) * 1e3
                st = r.last_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dst.copy_(src)
                e1.record()
                e1.synchronize()
                if it >= args.warmup:
                    for k in ("clear_us", "fill_us", "compose_us", "decode_ms", "upload_ms"):
                        rows[k].append(st[k])
                    rows["call_ms"].append(call_ms)
                    rows["copy_us"].append(e0.elapsed_time(e1) * 1e3)
            st = r.last_stats()
            r.close()
            med = {k: pct(v) for k, v in rows.items()}
            fill_bytes = 4 * px + 16 * st["intervals"]          # plane write + interval list read
            compose_bytes = (4 + 3 + 3) * px                    # plane read + frame read + frame write
            kernels_us = med["fill_us"]["median"] + med["compose_us"]["median"]
            case = {
                "size": size, "input": kind, "intervals": st["intervals"], "distinct_ids": st["distinct_ids"],
                "launches_per_frame": st["launches"],
                "fill": dict(med["fill_us"], unit="us", bytes_per_pixel=fill_bytes / px,
                             GBps=fill_bytes / med["fill_us"]["median"] / 1e3),
                "compose": dict(med["compose_us"], unit="us", bytes_per_pixel=compose_bytes / px,
                                GBps=compose_bytes / med["compose_us"]["median"] / 1e3),
                "clear": dict(med["clear_us"], unit="us"),
                "copy_same_bytes": dict(med["copy_us"], unit="us", bytes_per_pixel=14.0,
                                        GBps=14 * px / med["copy_us"]["median"] / 1e3),
                "kernels_over_copy": kernels_us / med["copy_us"]["median"],
                "host_decode_colour_table_ms": med["decode_ms"],
                "host_upload_ms": med["upload_ms"],
                "call_wall_ms": med["call_ms"],
            }
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    print("wrote", args.out)


def vector_leg(args, result, dev):
    import torch
    import synth
    import vector_raster_model as vm
    import video_segment_amd as vsg
    from test_proto_wire import build_schema
    Msg = build_schema()
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        for kind, frame_fn in (("checker", synth.bench_frame), ("noise", synth.noise_frame)):
            N = 3
            fl = torch.from_numpy(synth.const_flow(W, H)).to(dev)
            d = vsg.DenseSegmentation(W, H, vsg.default_options(chunk_size=20, compute_vectorization=1), has_flow=True)
            frames, segs = [], []
            for k in range(N):
                frames.append(torch.from_numpy(frame_fn(W, H, k)).to(dev))
                n = d.process_frame(frames[k], fl if k > 0 else None, flush=(k == N - 1))
                segs += [d.result_bytes(i) for i in range(n)]
            d.close()
            m = Msg()
            m.ParseFromString(segs[1])
            stripped = vm.remove_rasterization(m)
            stripped.frame_width, stripped.frame_height = W, H
            frame = frames[1]
            out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
            case = {"size": size, "input": kind, "regions": len(m.region)}
            for leg, seg in (("raster", segs[1]), ("vector", stripped.SerializeToString())):
                r = vsg.SegmentationRenderer(W, H)
                keys = ["decode_ms", "upload_ms", "clear_us", "fill_us", "compose_us", "call_ms"]
                if leg == "vector":
                    keys += ["walk_us", "sort_us", "pairs_us"]
                rows = {k: [] for k in keys}
                for it in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    r.render(seg, frame, out=out)
                    call_ms = (time.perf_counter() - t0) * 1e3
                    st = dict(r.last_stats(), call_ms=call_ms, **r.last_vector_stats())
                    if it >= args.warmup:
                        for k in keys:
                            rows[k].append(st[k])
                st = dict(r.last_stats(), **r.last_vector_stats())
                r.close()
                entry = {k: dict(pct(v), unit=k.rsplit("_", 1)[1]) for k, v in rows.items()}
                entry.update(seg_bytes=len(seg), intervals=st["intervals"], launches_per_frame=st["launches"])
                if leg == "vector":
                    entry.update(lines=st["lines"], crossings=st["crossings"], groups=st["groups"],
                                 largest_group=st["largest_group"])
                case[leg] = entry
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    print("wrote", args.out)


def level_descs(args):
    """Per size: (size, W, H, a dense-unit desc that carries a hierarchy, its height)."""
    import synth
    import video_segment_amd as vsg
    from test_proto_wire import build_schema
    Msg = build_schema()
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        N = 3
        fl = synth.const_flow(W, H)
        frames = [synth.bench_frame(W, H, k) for k in range(N)]
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
        m = Msg()
        m.ParseFromString(segs[0])          # the chunk's first frame carries the hierarchy
        yield size, W, H, segs[0], len(m.hierarchy)


def level_leg(args, result, dev):
    import torch
    import video_segment_amd as vsg
    from video_segment_amd import render
    for size, W, H, seg0, height in level_descs(args):
        r = vsg.SegmentationRenderer(W, H, has_video=False)
        ids = torch.empty((H, W), dtype=torch.int32, device=dev)
        for level in sorted({0, height // 2, max(height - 1, 0)}):
            nr, ni = (len(a) for a in r.level_regions(seg0, level))
            regions = torch.empty((nr, render.LEVEL_REGION_WORDS), dtype=torch.int32, device=dev)
            intervals = torch.empty((ni, 4), dtype=torch.int32, device=dev)
            keys = ["runs_us", "sort_us", "table_us", "moments_us", "call_ms", "id_image_call_ms", "id_image_fill_us",
                    "id_image_clear_us"]
            rows = {k: [] for k in keys}
            for it in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                r.level_regions(seg0, level, regions_out=regions, intervals_out=intervals)
                st = dict(r.last_level_stats(), call_ms=(time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                r.id_image(seg0, level, out=ids)
                ist = r.last_stats()
                st.update(id_image_call_ms=(time.perf_counter() - t0) * 1e3, id_image_fill_us=ist["fill_us"],
                          id_image_clear_us=ist["clear_us"])
                if it >= args.warmup:
                    for k in keys:
                        rows[k].append(st[k])
            case = {"size": size, "level": level, "hierarchy_levels": height, "runs": st["runs"],
                    "regions": st["regions"], "largest_region_intervals": st["largest_region_intervals"],
                    "launches": st["launches"]}
            case.update({k: dict(pct(v), unit=k.rsplit("_", 1)[1]) for k, v in rows.items()})
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
        r.close()
    print("wrote", args.out)


def components_leg(args, result, dev):
    import torch
    import video_segment_amd as vsg
    from video_segment_amd import render
    for size, W, H, seg, height in level_descs(args):
        r = vsg.SegmentationRenderer(W, H, has_video=False)
        labels = torch.empty((H, W), dtype=torch.int32, device=dev)
        for level in sorted({0, height // 2, max(height - 1, 0)}):
            nr, ni = (len(a) for a in r.level_regions(seg, level))
            regions = torch.empty((nr, render.LEVEL_REGION_WORDS), dtype=torch.int32, device=dev)
            intervals = torch.empty((ni, 4), dtype=torch.int32, device=dev)
            for name, connect in (("N4", render.N4), ("N8", render.N8)):
                nc = len(r.level_components(seg, level, connect)[0])
                comps = torch.empty((nc, render.LEVEL_COMPONENT_WORDS), dtype=torch.int32, device=dev)
                stage_keys = ["runs_us", "sort_us", "link_us", "order_us", "moments_us", "label_us"]
                region_keys = ["runs_us", "sort_us", "table_us", "moments_us"]
                rows = {k: [] for k in stage_keys + ["call_ms", "level_regions_call_ms"]
                        + ["level_regions_" + k for k in region_keys]}
                for it in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    r.level_components(seg, level, connect, components_out=comps, intervals_out=intervals,
                                       labels_out=labels)
                    st = dict(r.last_component_stats(), call_ms=(time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    r.level_regions(seg, level, regions_out=regions, intervals_out=intervals)
                    st["level_regions_call_ms"] = (time.perf_counter() - t0) * 1e3
                    lst = r.last_level_stats()
                    st.update({"level_regions_" + k: lst[k] for k in region_keys})
                    if it >= args.warmup:
                        for k in rows:
                            rows[k].append(st[k])
                case = {"size": size, "level": level, "hierarchy_levels": height, "connectedness": name,
                        "runs": st["runs"], "regions": st["regions"], "components": st["components"],
                        "links": st["links"], "largest_component_intervals": st["largest_component_intervals"],
                        "largest_region_intervals": lst["largest_region_intervals"], "launches": st["launches"],
                        "level_regions_launches": lst["launches"]}
                case.update({k: dict(pct(v), unit=k.rsplit("_", 1)[1]) for k, v in rows.items()})
                result["cases"].append(case)
                print(json.dumps(case), flush=True)
                with open(args.out, "w") as f:
                    json.dump(result, f, indent=1)
                    f.write("\n")
        r.close()
    print("wrote", args.out)


def boundaries_leg(args, result, dev):
    import torch
    import video_segment_amd as vsg
    from video_segment_amd import render
    for size, W, H, seg, height in level_descs(args):
        r = vsg.SegmentationRenderer(W, H, has_video=False)
        labels = torch.empty((H, W), dtype=torch.int32, device=dev)
        for level in sorted({0, height // 2, max(height - 1, 0)}):
            nc, ni = (len(a) for a in r.level_components(seg, level, render.N4))
            comps = torch.empty((nc, render.LEVEL_COMPONENT_WORDS), dtype=torch.int32, device=dev)
            intervals = torch.empty((ni, 4), dtype=torch.int32, device=dev)
            for mode, connect in (("regions", 0), ("components_N4", render.N4)):
                for which, outer in (("inner", False), ("outer", True)):
                    nb, npts = (len(a) for a in r.level_boundaries(seg, level, connect, outer))
                    records = torch.empty((nb, render.LEVEL_BOUNDARY_WORDS), dtype=torch.int32, device=dev)
                    points = torch.empty((npts, 2), dtype=torch.int32, device=dev)
                    stage_keys = ["plane_us", "count_us", "emit_us", "sort_us", "table_us"]
                    comp_keys = ["runs_us", "sort_us", "link_us", "order_us", "moments_us", "label_us"]
                    rows = {k: [] for k in stage_keys + ["call_ms", "level_components_call_ms"]
                            + ["level_components_" + k for k in comp_keys]}
                    for it in range(args.warmup + args.reps):
                        t0 = time.perf_counter()
                        r.level_boundaries(seg, level, connect, outer, boundaries_out=records, points_out=points)
                        st = dict(r.last_boundary_stats(), call_ms=(time.perf_counter() - t0) * 1e3)
                        t0 = time.perf_counter()
                        r.level_components(seg, level, render.N4, components_out=comps, intervals_out=intervals,
                                           labels_out=labels)
                        st["level_components_call_ms"] = (time.perf_counter() - t0) * 1e3
                        cst = r.last_component_stats()
                        st.update({"level_components_" + k: cst[k] for k in comp_keys})
                        if it >= args.warmup:
                            for k in rows:
                                rows[k].append(st[k])
                    case = {"size": size, "level": level, "hierarchy_levels": height, "mode": mode, "which": which,
                            "points": st["points"], "boundaries": st["boundaries"],
                            "largest_boundary_points": st["largest_boundary_points"], "launches": st["launches"],
                            "runs": cst["runs"], "components": cst["components"],
                            "level_components_launches": cst["launches"]}
                    case.update({k: dict(pct(v), unit=k.rsplit("_", 1)[1]) for k, v in rows.items()})
                    result["cases"].append(case)
                    print(json.dumps(case), flush=True)
                    with open(args.out, "w") as f:
                        json.dump(result, f, indent=1)
                        f.write("\n")
        r.close()
    print("wrote", args.out)


def adjacency_leg(args, result, dev):
    import torch
    import video_segment_amd as vsg
    from video_segment_amd import render
    for size, W, H, seg, height in level_descs(args):
        r = vsg.SegmentationRenderer(W, H, has_video=False)
        for level in sorted({0, height // 2, max(height - 1, 0)}):
            for mode, connect in (("regions", 0), ("components_N4", render.N4)):
                nb, npts = (len(a) for a in r.level_boundaries(seg, level, connect, False))
                records = torch.empty((nb, render.LEVEL_BOUNDARY_WORDS), dtype=torch.int32, device=dev)
                points = torch.empty((npts, 2), dtype=torch.int32, device=dev)
                for name, hood in (("N4", render.ADJACENT_N4), ("N8", render.ADJACENT_N8)):
                    nn, ne = (len(a) for a in r.level_adjacency(seg, level, connect, hood))
                    nodes = torch.empty((nn, render.LEVEL_NODE_WORDS), dtype=torch.int32, device=dev)
                    edges = torch.empty((ne, render.LEVEL_EDGE_WORDS), dtype=torch.int32, device=dev)
                    stage_keys = ["plane_us", "count_us", "emit_us", "sort_us", "table_us"]
                    rows = {k: [] for k in stage_keys + ["call_ms", "level_boundaries_call_ms"]}
                    for it in range(args.warmup + args.reps):
                        t0 = time.perf_counter()
                        r.level_adjacency(seg, level, connect, hood, nodes_out=nodes, edges_out=edges)
                        st = dict(r.last_adjacency_stats(), call_ms=(time.perf_counter() - t0) * 1e3)
                        t0 = time.perf_counter()
                        r.level_boundaries(seg, level, connect, False, boundaries_out=records, points_out=points)
                        st["level_boundaries_call_ms"] = (time.perf_counter() - t0) * 1e3
                        if it >= args.warmup:
                            for k in rows:
                                rows[k].append(st[k])
                    case = {"size": size, "level": level, "hierarchy_levels": height, "mode": mode,
                            "neighbourhood": name, "sides": st["sides"], "keys": st["keys"], "nodes": st["nodes"],
                            "edges": st["edges"], "largest_node_edges": st["largest_node_edges"],
                            "launches": st["launches"]}
                    case.update({k: dict(pct(v), unit=k.rsplit("_", 1)[1]) for k, v in rows.items()})
                    result["cases"].append(case)
                    print(json.dumps(case), flush=True)
                    with open(args.out, "w") as f:
                        json.dump(result, f, indent=1)
                        f.write("\n")
        r.close()
    print("wrote", args.out)


def overlap_leg(args, result, dev):
    import torch
    import video_segment_amd as vsg
    from video_segment_amd import render
    shift = 8
    for size, W, H, seg, height in level_descs(args):
        r = vsg.SegmentationRenderer(W, H, has_video=False)
        ids = torch.empty((H, W), dtype=torch.int32, device=dev)
        for level in sorted({0, max(height - 1, 0)}):
            r.id_image(seg, level, out=ids)
            other = torch.full((H, W), -1, dtype=torch.int32, device=dev)
            other[:, shift:] = ids[:, :W - shift]
            for mode, connect in (("regions", 0), ("components_N4", render.N4)):
                nn, ne = (len(a) for a in r.level_adjacency(seg, level, connect, render.ADJACENT_N4))
                nodes = torch.empty((nn, render.LEVEL_NODE_WORDS), dtype=torch.int32, device=dev)
                edges = torch.empty((ne, render.LEVEL_EDGE_WORDS), dtype=torch.int32, device=dev)
                sizes = [len(a) for a in r.level_overlap(seg, level, other, connect)]
                words = (render.OVERLAP_ROW_WORDS, render.OVERLAP_COL_WORDS, render.OVERLAP_PAIR_WORDS)
                outs = [torch.empty((n, w), dtype=torch.int32, device=dev) for n, w in zip(sizes, words)]
                stage_keys = ["plane_us", "count_us", "emit_us", "sort_us", "table_us"]
                rows = {k: [] for k in stage_keys + ["call_ms", "level_adjacency_call_ms"]
                        + ["level_adjacency_" + k for k in stage_keys]}
                for it in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    r.level_overlap(seg, level, other, connect, rows_out=outs[0], cols_out=outs[1], pairs_out=outs[2])
                    st = dict(r.last_overlap_stats(), call_ms=(time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    r.level_adjacency(seg, level, connect, render.ADJACENT_N4, nodes_out=nodes, edges_out=edges)
                    st["level_adjacency_call_ms"] = (time.perf_counter() - t0) * 1e3
                    ast = r.last_adjacency_stats()
                    st.update({"level_adjacency_" + k: ast[k] for k in stage_keys})
                    if it >= args.warmup:
                        for k in rows:
                            rows[k].append(st[k])
                case = {"size": size, "level": level, "hierarchy_levels": height, "mode": mode, "shift": shift,
                        "runs": st["runs"], "rows": st["rows"], "cols": st["cols"], "pairs": st["pairs"],
                        "largest_row_pairs": st["largest_row_pairs"], "covered": st["covered"],
                        "labelled": st["labelled"], "both": st["both"], "launches": st["launches"],
                        "level_adjacency_keys": ast["keys"], "level_adjacency_launches": ast["launches"]}
                case.update({k: dict(pct(v), unit=k.rsplit("_", 1)[1]) for k, v in rows.items()})
                result["cases"].append(case)
                print(json.dumps(case), flush=True)
                with open(args.out, "w") as f:
                    json.dump(result, f, indent=1)
                    f.write("\n")
        r.close()
    print("wrote", args.out)


def persistence_leg(args, result, dev):
    import torch
    import synth
    import video_segment_amd as vsg
    from video_segment_amd import render
    from test_proto_wire import build_schema
    Msg = build_schema()
    for size, W, H, seg, height in level_descs(args):
        src = torch.from_numpy(synth.bench_frame(W, H, 0)).to(dev)
        for L in sorted({1, 2, 5, height} & set(range(1, height + 1))):
            m = Msg()
            m.ParseFromString(seg)
            del m.hierarchy[(L if L > 1 else 0):]       # the top level's parents are never looked up
            cut = m.SerializeToString()
            r = vsg.SegmentationRenderer(W, H)          # a handle of its own: no kept hierarchy from another height
            plane = torch.empty((H, W), dtype=torch.int32, device=dev)
            ids = torch.empty((H, W), dtype=torch.int32, device=dev)
            picture = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
            assert r.persistence_image(cut, out=plane)[1] == L
            nn, ne = (len(a) for a in r.level_adjacency(cut, 0))
            nodes = torch.empty((nn, render.LEVEL_NODE_WORDS), dtype=torch.int32, device=dev)
            edges = torch.empty((ne, render.LEVEL_EDGE_WORDS), dtype=torch.int32, device=dev)
            persistence = torch.empty((ne,), dtype=torch.int32, device=dev)
            level_sides = torch.empty((L,), dtype=torch.int64, device=dev)
            keys = ["image_call_ms", "image_plane_us", "image_persist_us", "frame_call_ms", "frame_plane_us",
                    "frame_persist_us", "frame_compose_us", "graph_call_ms", "graph_plane_us", "graph_graph_us",
                    "graph_persist_us", "id_image_per_level_call_ms", "level_adjacency_per_level_call_ms"]
            rows = {k: [] for k in keys}
            launches = {}
            for it in range(args.warmup + args.reps):
                st = {}
                t0 = time.perf_counter()
                r.persistence_image(cut, out=plane)
                st["image_call_ms"] = (time.perf_counter() - t0) * 1e3
                ps = r.last_persistence_stats()
                st.update({"image_" + k: ps[k] for k in ("plane_us", "persist_us")})
                launches["image"] = ps["launches"]
                t0 = time.perf_counter()
                r.persistence_frame(cut, src, out=picture)
                st["frame_call_ms"] = (time.perf_counter() - t0) * 1e3
                ps = r.last_persistence_stats()
                st.update({"frame_" + k: ps[k] for k in ("plane_us", "persist_us", "compose_us")})
                launches["frame"] = ps["launches"]
                t0 = time.perf_counter()
                r.persistence_graph(cut, render.ADJACENT_N4, nodes, edges, persistence, level_sides)
                st["graph_call_ms"] = (time.perf_counter() - t0) * 1e3
                ps = r.last_persistence_stats()
                st.update({"graph_" + k: ps[k] for k in ("plane_us", "graph_us", "persist_us")})
                launches["graph"] = ps["launches"]
                # the yardsticks: one call per level
                t0 = time.perf_counter()
                for level in range(L):
                    r.id_image(cut, level, out=ids)
                st["id_image_per_level_call_ms"] = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                for level in range(L):
                    r.level_adjacency(cut, level, 0, render.ADJACENT_N4, nodes_out=nodes, edges_out=edges)
                st["level_adjacency_per_level_call_ms"] = (time.perf_counter() - t0) * 1e3
                if it >= args.warmup:
                    for k in rows:
                        rows[k].append(st[k])
            case = {"size": size, "hierarchy_levels": L, "regions": ps["regions"], "nodes": ps["nodes"],
                    "edges": ps["edges"], "edge_pixels": int((plane > 0).sum()), "top_pixels": int((plane == L).sum()),
                    "image_launches": launches["image"], "frame_launches": launches["frame"],
                    "graph_launches": launches["graph"]}
            case.update({k: dict(pct(v), unit=k.rsplit("_", 1)[1]) for k, v in rows.items()})
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
            r.close()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
