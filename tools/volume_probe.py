"""Device and call time of a volume session: vsg_render_volume_add and vsg_render_volume_table.

    python tools/volume_probe.py [--reps 5] [--warmup 1] [--frames 20] [--sizes 1920x1080,3840x2160]
                                 [--inputs checker,noise] [--out profiles/volume.json]

For every size, on a checker-like (synth.bench_frame) and a many-region (synth.noise_frame) chunk result of the
dense over-segmentation given a hierarchy by RegionSegmentation, at level 0 and at the top level: a session with
colours and labels over `frames` adds.  The chunk result has three descs; add k takes desc k mod 3, its frame in
device memory, and as labels the id image (device memory) of the desc before it at the same level, so the first
three adds bring every key and the others bring none.  A repetition is one whole session; medians over the adds
of all repetitions after the warm-up sessions, with the 10th and 90th percentile as the spread, separately for
the adds that brought keys (`new`) and for those that did not (`steady`).  Reported:

  add_call_ms and the stages of vsg_render_volume_stats (frame_us, geometry_us, merge_us, sort_us);
  table_call_ms and table_us of a read-out after the last add (host outputs);
  siblings_call_ms: in the same run and on the same handle, vsg_render_level_overlap + vsg_render_level_colors on
  the same desc, frame and labels with outputs in device memory: add_over_siblings = add_call_ms / siblings_call_ms
  (steady adds) is the price of the geometry and the merge;
  host_merge_ms_per_add: the same session done the only way there was before: vsg_render_level_regions,
  _colors and _overlap on the same desc, with the same frame and labels in device memory and with host outputs,
  for every frame, the records summed into Python dicts keyed by id and by (id, label):
  host_merge_over_add = host_merge_ms_per_add / add_call_ms (steady adds).  Only the tables cross to the host.
  One session, not repeated.

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
    if not len(a):
        return None
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90))}


def chunk_result(vsg, synth, frame_fn, W, H):
    """(the chunk's descs, the first of which carries the hierarchy; its height; the frames)."""
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
    m.ParseFromString(segs[0])
    return segs, len(m.hierarchy), frames


def host_merge(r, segs, level, frames, labels, n_adds):
    """The session on the host: every frame's tables fetched and summed into dicts.  frames, labels: in device
    memory, as the timed adds get them."""
    rows, pairs = {}, {}
    t0 = time.perf_counter()
    for k in range(n_adds):
        seg, F, B = segs[k % len(segs)], frames[k % len(segs)], labels[k % len(segs)]
        regions, _ = r.level_regions(seg, level)
        colors = r.level_colors(seg, level, F)
        orows, _, opairs = r.level_overlap(seg, level, B)
        sums = colors["sum"].tolist()
        for i, (rid, area, un) in enumerate(zip(regions["id"].tolist(), regions["area"].tolist(),
                                                orows["unlabelled"].tolist())):
            acc = rows.get(rid)
            if acc is None:
                acc = rows[rid] = [k, k, 0, 0, 0, 0, 0, 0]
            acc[1] = k
            acc[2] += 1
            acc[3] += area
            acc[4] += un
            acc[5] += sums[i][0]
            acc[6] += sums[i][1]
            acc[7] += sums[i][2]
        ids = regions["id"][opairs["row"]].tolist()
        for rid, label, count in zip(ids, opairs["label"].tolist(), opairs["count"].tolist()):
            key = (rid, label)
            pairs[key] = pairs.get(key, 0) + count
    return (time.perf_counter() - t0) * 1e3 / n_adds, len(rows), len(pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--inputs", default="checker,noise")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume.json"))
    args = ap.parse_args()

    import torch
    import synth
    import video_segment_amd as vsg
    from video_segment_amd import _lib, render
    if _lib.lib().vsg_device_count() <= 0:
        sys.exit("volume_probe needs a HIP device: a time from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "frames": args.frames, "cases": []}
    generators = {"checker": synth.bench_frame, "noise": synth.noise_frame}
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        for kind in args.inputs.split(","):
            t0 = time.perf_counter()
            segs, height, frames = chunk_result(vsg, synth, generators[kind], W, H)
            print("%s %s: chunk result in %.1f s, %d levels" % (size, kind, time.perf_counter() - t0, height),
                  flush=True)
            d_frames = [torch.from_numpy(f).to(dev) for f in frames]
            r = vsg.SegmentationRenderer(W, H)
            for level in sorted({0, max(height - 1, 0)}):
                r.id_image(segs[0], level)            # the hierarchy is kept from here on
                planes = [r.id_image(s, level) for s in segs]
                labels = [planes[k - 1] for k in range(len(segs))]
                d_labels = [torch.from_numpy(b).to(dev) for b in labels]
                sizes = [len(a) for a in r.level_overlap(segs[0], level, labels[0])]
                outs = [torch.empty((3 * sizes[0] + 64, render.OVERLAP_ROW_WORDS), dtype=torch.int32, device=dev),
                        torch.empty((3 * sizes[1] + 64, render.OVERLAP_COL_WORDS), dtype=torch.int32, device=dev),
                        torch.empty((4 * sizes[2] + 64, render.OVERLAP_PAIR_WORDS), dtype=torch.int32, device=dev)]
                table = torch.empty((3 * sizes[0] + 64, render.LEVEL_COLOR_WORDS), dtype=torch.int32, device=dev)
                keys = ["add_call_ms", "frame_us", "geometry_us", "merge_us", "sort_us", "siblings_call_ms"]
                rows = {"new": {k: [] for k in keys}, "steady": {k: [] for k in keys}}
                tables = {"table_call_ms": [], "table_us": []}
                st = {}
                for it in range(args.warmup + args.reps):
                    r.volume_begin(level, True, True)
                    for k in range(args.frames):
                        j = k % len(segs)
                        t0 = time.perf_counter()
                        r.volume_add(segs[j], k, d_frames[j], d_labels[j])
                        st = dict(r.last_volume_stats(), add_call_ms=(time.perf_counter() - t0) * 1e3)
                        t0 = time.perf_counter()
                        r.level_overlap(segs[j], level, d_labels[j], rows_out=outs[0], cols_out=outs[1],
                                        pairs_out=outs[2])
                        r.level_colors(segs[j], level, d_frames[j], colors_out=table)
                        st["siblings_call_ms"] = (time.perf_counter() - t0) * 1e3
                        if it >= args.warmup:
                            which = rows["new" if st["resorts"] else "steady"]
                            for name in keys:
                                which[name].append(st[name])
                    t0 = time.perf_counter()
                    got = r.volume_table()
                    if it >= args.warmup:
                        tables["table_call_ms"].append((time.perf_counter() - t0) * 1e3)
                        tables["table_us"].append(r.last_volume_stats()["table_us"])
                host_ms, host_rows, host_pairs = host_merge(r, segs, level, d_frames, d_labels, args.frames)
                assert (host_rows, host_pairs) == (len(got[0]), len(got[2])), "the host merge has other keys"
                steady = {k: pct(v) for k, v in rows["steady"].items()}
                case = {"size": size, "input": kind, "level": level, "hierarchy_levels": height,
                        "rows": st["rows"], "cols": st["cols"], "pairs": st["pairs"], "launches_steady": st["launches"],
                        "new": {k: pct(v) for k, v in rows["new"].items()}, "steady": steady,
                        "table_call_ms": pct(tables["table_call_ms"]), "table_us": pct(tables["table_us"]),
                        "host_merge_ms_per_add": host_ms,
                        "add_over_siblings": steady["add_call_ms"]["median"] / steady["siblings_call_ms"]["median"],
                        "host_merge_over_add": host_ms / steady["add_call_ms"]["median"]}
                result["cases"].append(case)
                print(json.dumps(case), flush=True)
                with open(args.out, "w") as f:
                    json.dump(result, f, indent=1)
                    f.write("\n")
            r.close()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
