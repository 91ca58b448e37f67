"""bench.py contract: one JSON line with the required keys; the N > 1 control flow (barriers,
reductions, chunk-chain hand-off) exercised with two ranks sharing the one GPU of the test box
(gloo instead of RCCL, which refuses two ranks on one device)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
            "scaling", "vs_baseline", "dtype", "data", "config", "roofline"]


def last_json_line(text):
    for line in reversed(text.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError(text)


def check(out, n_gpus, steps, warmup):
    for k in REQUIRED:
        assert k in out, k
    assert out["n_gpus"] == n_gpus and out["steps"] == steps and out["warmup"] == warmup
    assert out["value"] > 0 and out["higher_is_better"] is True and out["scaling"] == "weak"
    assert out["unit"] == "frames/s" and out["dtype"] == "f32" and out["data"] == "synthetic"
    assert "workload" in out["config"] and "model" not in out["config"]
    r = out["roofline"]
    for k in ["bound", "achieved", "peak", "unit", "frac", "traffic"]:
        assert k in r, k
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12


# what only `bench.py --full` measures or checks; a plain run leaves these keys out
FULL_ONLY = ["cpu_baseline", "cpu_baseline_threaded", "parity_checked", "pcie_inclusive", "configs",
             "workloads", "streams_sweep", "pipelined"]


def test_full_is_off_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--pipelined-leg"])
    assert bench.parse().full is True
    # the pipelined leg is one of the information-only legs: without --full it would silently not run
    monkeypatch.setattr(sys, "argv", ["bench.py", "--pipelined-leg"])
    with pytest.raises(SystemExit):
        bench.parse()


@pytest.mark.gpu
def test_plain_line_is_the_headline_only():
    """A plain run sets up, warms up, times the steps and prints the line: the contract keys and
    what the timed steps themselves give (roofline, stages), none of the --full legs."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--width", "320", "--height", "240"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    out = last_json_line(p.stdout)
    check(out, 1, 2, 1)
    assert out["value"] * out["ms_per_step"] * out["steps"] / 1e3 == pytest.approx(2 * 19)
    assert out["stage_ms_per_step"]["merge"] > 0 and out["roofline"]["achieved"] >= 0
    for k in FULL_ONLY:
        assert k not in out, k
    assert out["roofline"]["peak_measured"] is None and out["chain"] is None


@pytest.mark.gpu
def test_single_gpu_line_and_cpu_baseline():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2",
                        "--warmup", "1", "--width", "320", "--height", "240", "--cpu-frames", "20"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    out = last_json_line(p.stdout)
    check(out, 1, 2, 1)
    c = out["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and "sample" in c
    assert out["parity_checked"] is True and out["pcie_inclusive"]["value"] > 0
    assert out["roofline"]["peak_measured"] > 0


@pytest.mark.gpu
def test_dump_outputs_hold_the_last_timed_step(tmp_path):
    """--dump-outputs writes what the last timed step returned, within 64 MB: the same arrays as the
    oracle's last chunk boundary over the same frames (two timed steps after one warm-up step)."""
    import numpy as np
    W, H, chunk, boundaries = 320, 240, 20, 3
    d = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1",
                        "--width", str(W), "--height", str(H), "--no-cpu-baseline", "--no-pcie-leg",
                        "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    out = last_json_line(p.stdout)
    check(out, 1, 2, 1)
    assert out["dump_outputs"]["frames"] == chunk - 1
    names = sorted(os.listdir(d))
    assert names == sorted(n + ".npy" for n in out["dump_outputs"]["arrays"])
    assert sum(os.path.getsize(d / n) for n in names) <= 64e6

    import bench
    import oracle_lib as ol
    import synth
    o = ol.OracleStream(W, H, ol.default_options(chunk_size=chunk), has_flow=True)
    fl = synth.const_flow(W, H)
    seen = 0
    for k in range(chunk + (chunk - 1) * (boundaries - 1)):
        n = o.process_frame(synth.bench_frame(W, H, k), fl if k > 0 else None)
        if n:
            seen += 1
            last = n
    assert seen == boundaries
    bench.dump_outputs(o, last, W, H, str(tmp_path / "oracle"))
    o.close()
    for n in names:
        got, want = np.load(d / n), np.load(tmp_path / "oracle" / n)
        assert got.dtype in (np.float32, np.float64) and got.dtype == want.dtype, n
        assert got.shape == want.shape and np.array_equal(got, want), n


@pytest.mark.gpu
@pytest.mark.parametrize("mode,port", [("streams", "29611"), ("chain", "29612")])
def test_two_ranks_control_flow(mode, port):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", port, os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "2", "--warmup", "1", "--width", "256", "--height", "144",
           "--mode", mode, "--dist-backend", "gloo", "--share-gpu", "--no-cpu-baseline", "--full"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=360, cwd=ROOT, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    out = last_json_line(p.stdout)
    check(out, 2, 2, 1)
    # two ranks x two timed steps x 19 frames (streams) or one 4-chunk video (chain: 20 + 3 x 19)
    frames = out["value"] * out["ms_per_step"] * out["steps"] / 1e3
    assert abs(frames - (76 if mode == "streams" else 77)) < 1e-6
    if mode == "streams":
        # the N > 1 line says by itself how many ranks the collective backend spanned and what
        # every one of them measured
        rk = out["ranks"]
        assert rk["world_size"] == 2 and rk["allreduce_sum_of_ones"] == 2.0 and rk["backend"] == "gloo"
        assert len(rk["per_rank_frames_per_s"]) == 2 and all(v > 0 for v in rk["per_rank_frames_per_s"])
        assert out["value"] <= sum(rk["per_rank_frames_per_s"]) * (1 + 1e-9)   # MAX over ranks of the time
        # ... and carries the other partition of SURVEY 8(e) as well: a short chunk-chain leg (ONE
        # video over the ranks, the halo handed on through the transport: RCCL inside the library
        # on a multi-GPU node, torch.distributed/gloo in this one-GPU control-flow test)
        ch = out["chain"]
        assert "error" not in ch, ch
        assert ch["value"] > 0 and ch["chunks_per_rank"] == 2 and ch["rccl_ranks"] == 0
        assert ch["handoff_ms"] >= 0 and ch["recv_wait_ms"] >= 0 and ch["bytes_per_handoff"] == 2 * 256 * 144 * 4 + 32
        assert "expected" in ch and ch["vs_one_stream"] > 0


@pytest.mark.gpu
def test_two_ranks_plain_line():
    """A plain N > 1 run: the replicas leg and what every rank measured, no chunk-chain leg."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29613", os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "2", "--warmup", "1", "--width", "256", "--height", "144",
           "--dist-backend", "gloo", "--share-gpu"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=360, cwd=ROOT, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    out = last_json_line(p.stdout)
    check(out, 2, 2, 1)
    assert abs(out["value"] * out["ms_per_step"] * out["steps"] / 1e3 - 76) < 1e-6
    assert out["ranks"]["world_size"] == 2 and out["ranks"]["allreduce_sum_of_ones"] == 2.0
    assert out["chain"] is None
    for k in FULL_ONLY:
        assert k not in out, k


def test_committed_round_line_carries_every_key():
    """The full bench line of the round (what `bench.py --full` prints, a plain run before that option
    existed; profiles/, produced on an MI355X by tools/measure_round.sh): the contract keys plus what
    the headline depends on -- the other single-GPU configs, the other inputs (each with its own
    oracle check), the streams sweep, the memory a stream holds -- and counters that belong to the
    kernel sources of the same commit."""
    import glob
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r6_*_bench_1080p.json")))
    assert paths, "no round-6 bench line under profiles/"
    out = last_json_line(open(paths[-1]).read())
    check(out, 1, out["steps"], out["warmup"])
    assert out["vs_baseline"] is None and out["parity_checked"] is True
    c = out["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0
    assert out["roofline"]["bound"] == "hbm" and out["roofline"]["peak"] == 8000.0
    cfg = out["configs"]
    assert cfg["configs[1]"]["cpu_baseline"]["value"] > 0 and cfg["configs[1]"]["parity_checked"] is True
    assert set(cfg["configs[1]"]["phase_ms_per_window"]) == {"create", "add_frames", "segment", "read_out", "close"}
    assert cfg["3840x2160"]["value"] > 0 and cfg["configs[4]"]["value"] > 0
    # four 3840x2160 streams fit the 288 GB of the device
    assert (1 << 30) < cfg["3840x2160"]["device_bytes_per_stream"] < 72e9
    wl = out["workloads"]
    assert set(wl) >= {"checker (headline input)", "blobs", "noise"}
    assert wl["blobs"]["parity_checked"] is True and wl["noise"]["parity_checked"] is True
    assert [s["streams"] for s in out["streams_sweep"]] == [1, 2, 4, 8]
    assert "pipelined" not in out          # (only with --pipelined-leg)
    r = out["roofline"]
    assert r["peak_measured"] > 1000 and 0 < r["frac_of_measured"] < 1
    assert len(r["kernels"]["top"]) == 8 and all(k["ms_per_step"] > 0 for k in r["kernels"]["top"])
    assert 0.9 < r["traffic_vs_algorithmic_same_run"] < 1.5
    assert (1 << 30) < out["device_bytes_per_stream"] < 24e9
    # the counters the line quotes were taken from the kernel sources that are committed with it
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from source_hash import source_hash
    assert r["kernels"]["source_hash"] == source_hash(ROOT)
    for name in ("r6_pmc_wave.json", "r6_pmc_spine.json", "r6_kernel_table.json"):
        assert json.load(open(os.path.join(ROOT, "profiles", name)))["source_hash"] == source_hash(ROOT), name
