"""Device time of vsg_render_tree_cut, with both DP paths forced, against the route without it.

    python tools/tree_cut_probe.py [--reps 20] [--warmup 5] [--sizes 1920x1080,3840x2160]
                                   [--inputs checker,noise,grid12,blocks8] [--heights 1,5,20] [--penalty 50]
                                   [--out profiles/tree_cut.json]

Everything is in device memory.  The inputs are those of boundary_distance_probe.py: a checker-like and a
value-noise frame of the dense over-segmentation and `grid12`, 48 blocks that a top level merges into 12
regions; `blocksN` adds a plane of N x N pixel blocks, whose tree sizes bracket the crossover of the two DP
paths.  Every desc gets a hierarchy of L levels for each L of --heights, a handle of its own, and as ground truth
its own level-0 id image moved by (3, 4), the first row and column repeated into the border.

Per desc and L: vsg_render_tree_cut with labels, once with the one-workgroup DP forced (`block`) and once with
the per-level DP (`level`), each with the stage times and launches of vsg_render_cut_stats and the call's wall
time; medians over the repetitions after a warm-up, with the 10th and 90th percentile as the spread.  Measured
against, in the same run, on the same handle and desc, alternating with it: `host_route`, L calls of
vsg_render_level_overlap into device memory, the rows' best counts copied to the host, the hierarchy's parents
looked up with numpy and the dynamic programme run there; it paints nothing, so the comparison flatters it.
Its total has to equal the call's.  cut_over_host_route compares the wall times of the default-path call and
the route.

`crossover` at the end: the tree sizes between which the faster DP path changes, from dp_us of all cases; null
where one path was faster at every measured size.  No pass or fail threshold.
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

ONE_BLOCK = (1 << 63) - 1


def pct(values):
    a = np.asarray(values, np.float64)
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90))}


def parents_of(msg):
    """Per level below the top: (sorted ids, their parents' ids) as int64 arrays."""
    out = []
    for level in list(msg.hierarchy)[:-1]:
        pairs = sorted((c.id, c.parent_id) for c in level.region)
        out.append((np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64)))
    return out


def host_dp(tables, parents, penalty):
    """The model's dynamic programme on the rows (id, best_count) of every level's overlap table: the total."""
    ids, opt = tables[0][0], tables[0][1] - penalty
    for l in range(1, len(tables)):
        child_ids, parent_ids = parents[l - 1]
        up = parent_ids[np.searchsorted(child_ids, ids)]
        at = np.searchsorted(tables[l][0], up)
        split = np.zeros(len(tables[l][0]), np.int64)
        np.add.at(split, at, opt)
        ids, opt = tables[l][0], np.maximum(tables[l][1] - penalty, split)
    return int(opt.sum())


def crossover(cases):
    """Between which tree sizes the faster DP path changes."""
    points = sorted((c["counts"]["tree_nodes"], c["block_dp_us"]["median"], c["level_dp_us"]["median"])
                    for c in cases if c["counts"]["tree_nodes"])
    block_wins = [n for n, b, l in points if b <= l]
    level_wins = [n for n, b, l in points if b > l]
    out = {"points": [{"tree_nodes": n, "block_dp_us": b, "level_dp_us": l} for n, b, l in points],
           "largest_tree_where_block_is_faster": max(block_wins) if block_wins else None,
           "smallest_tree_where_level_is_faster": min(level_wins) if level_wins else None, "block_nodes": None}
    if block_wins and level_wins and max(block_wins) < min(level_wins):
        out["block_nodes"] = int(round((max(block_wins) * min(level_wins)) ** 0.5))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--inputs", default="checker,noise,grid12,blocks8")
    ap.add_argument("--heights", default="1,5,20")
    ap.add_argument("--penalty", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_cut.json"))
    args = ap.parse_args()

    import torch
    import boundary_distance_probe as bdp
    import level_regions_cases as lc
    import synth
    import video_segment_amd as vsg
    from video_segment_amd import _lib, render
    if _lib.lib().vsg_device_count() <= 0:
        sys.exit("tree_cut_probe needs a HIP device: a time from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "penalty": args.penalty, "cases": []}
    stage_keys = ["plane_us", "table_us", "lift_us", "dp_us", "paint_us"]
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        for kind in args.inputs.split(","):
            t0 = time.perf_counter()
            yy, xx = np.mgrid[0:H, 0:W]
            if kind == "grid12":
                seg = bdp.plane_desc(lc, (8 * (yy * 6 // H) + xx * 8 // W).astype(np.int32))
            elif kind.startswith("blocks"):
                b = int(kind[6:])
                seg = bdp.plane_desc(lc, ((yy // b) * ((W + b - 1) // b) + xx // b).astype(np.int32))
            else:
                seg = bdp.dense_desc(vsg, synth, {"checker": synth.bench_frame, "noise": synth.noise_frame}[kind], W, H)
            print("%s %s: desc in %.1f s" % (size, kind, time.perf_counter() - t0), flush=True)
            for L in (int(v) for v in args.heights.split(",")):
                if kind == "grid12" and L not in (1, 3):
                    L = 3                                   # 48 blocks, 24, 12 regions
                desc = bdp.with_height(lc.Msg, lc, seg, L)
                msg = lc.Msg()
                msg.ParseFromString(desc)
                parents = parents_of(msg)
                r = vsg.SegmentationRenderer(W, H, has_video=False)   # a handle of its own: no kept hierarchy
                ids0 = torch.empty((H, W), dtype=torch.int32, device=dev)
                r.id_image(desc, 0, out=ids0)
                ys = torch.clamp(torch.arange(H, device=dev) - 4, min=0)
                xs = torch.clamp(torch.arange(W, device=dev) - 3, min=0)
                other = ids0[ys][:, xs].contiguous()          # the first row and column repeated, as the tests do
                rows0, cols0, pairs0 = r.level_overlap(desc, 0, other)
                n_rows, n_cols, n_pairs = len(rows0), len(cols0), len(pairs0)
                d_rows = torch.empty((n_rows + 1, render.OVERLAP_ROW_WORDS), dtype=torch.int32, device=dev)
                d_cols = torch.empty((n_cols + 1, render.OVERLAP_COL_WORDS), dtype=torch.int32, device=dev)
                d_pairs = torch.empty((n_pairs + 1, render.OVERLAP_PAIR_WORDS), dtype=torch.int32, device=dev)
                d_nodes = torch.empty((n_rows + 1, render.CUT_NODE_WORDS), dtype=torch.int32, device=dev)
                d_plane = torch.empty((H, W), dtype=torch.int32, device=dev)

                def cut(block_nodes):
                    r.tree_cut_tuning(block_nodes)
                    return r.tree_cut(desc, labels=other, penalty=args.penalty, nodes_out=d_nodes, plane_out=d_plane)

                def host_route():
                    tables = []
                    for l in range(L):
                        rows, _, _ = r.level_overlap(desc, l, other, rows_out=d_rows, cols_out=d_cols,
                                                     pairs_out=d_pairs)
                        t = rows.cpu().numpy()
                        tables.append((t[:, 0].astype(np.int64), t[:, 7].astype(np.int64)))
                    return host_dp(tables, parents, args.penalty)

                legs = {"block": lambda: cut(ONE_BLOCK), "level": lambda: cut(0), "default": lambda: cut(-1)}
                samples, counts, totals = {}, {}, set()
                for it in range(args.warmup + args.reps):
                    for name, call in legs.items():
                        t0 = time.perf_counter()
                        nodes, _, total = call()
                        st = dict(r.last_cut_stats(), call_ms=(time.perf_counter() - t0) * 1e3)
                        totals.add(total)
                        counts[name] = {k: st[k] for k in ("levels", "leaves", "tree_nodes", "pairs", "entries",
                                                           "cut_nodes", "dp_path", "dp_launches", "launches")}
                        if it >= args.warmup:
                            for k in stage_keys + ["call_ms"]:
                                samples.setdefault(name + "_" + k, []).append(st[k])
                    t0 = time.perf_counter()
                    totals.add(host_route())
                    if it >= args.warmup:
                        samples.setdefault("host_route_call_ms", []).append((time.perf_counter() - t0) * 1e3)
                assert len(totals) == 1, totals                 # both paths and the host route agree
                med = {k: pct(v) for k, v in samples.items()}
                case = {"size": size, "input": kind, "hierarchy_levels": L, "counts": counts["block"],
                        "level_counts": counts["level"], "default_dp_path": counts["default"]["dp_path"],
                        "total": totals.pop(),
                        "cut_over_host_route": med["default_call_ms"]["median"] / med["host_route_call_ms"]["median"]}
                case.update({k: dict(v, unit=k.rsplit("_", 1)[1]) for k, v in med.items()})
                result["cases"].append(case)
                result["crossover"] = crossover(result["cases"])
                print(json.dumps(case), flush=True)
                with open(args.out, "w") as f:
                    json.dump(result, f, indent=1)
                    f.write("\n")
                r.close()
                if kind == "grid12" and L == 3:
                    break
    print("crossover", json.dumps(result.get("crossover")))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
