"""EVPLP_PARTITION_ITERATIONS: what the device reduction of a written frame costs, and what sharing out the iterations buys.  JSON to stdout.

(a) reduce_shards_kernel alone (one plane: n source planes of W x local_rows float4 -> one), 1080p and 1024^2 at n = 2, 4, 8 virtual ranks
    (all planes on GPU 0), launched through the library's own launcher on torch-allocated planes:
      * "events": HIP events (torch.cuda.Event) around `reps` back-to-back launches on one stream, mean per launch;
      * "rocprofv3": the same launches in a child process under `rocprofv3 --kernel-trace --stats` (a run of its own), mean kernel time.
    Bytes per plane = (n + 1) x W x local_rows x 16 (n reads, one write); GB/s = bytes / time.  The n source planes of one case are at most
    267 MB and were just read by the previous launch: much of them may be served by the 256 MiB Infinity Cache, so the rate can exceed
    what HBM alone gives (~6.3 TB/s achievable).  A written frame runs the kernel three times (VPL, photon, light).
(b) One written frame under ITERATIONS, host-clocked (perf_counter) around Group.resolve of a 1080p group of n virtual ranks (the sums made
    stale before every call, so each one exchanges and reduces), against the path the technique loop used before, reproduced in Python in the
    same process: download the VPL and photon planes of every rank, sum them in float32 in rank order, upload the sums into rank 0, resolve
    rank 0's context, upload rank 0's own planes back.  Median of `reps`.
(c) Iterations completed by the config #4 technique block (tools/run_cfg4.py's shape: 1920x1080, pure progressive photon mapping, 300 000
    light paths) with timeLimitMs 3000 and numMaxIteration -1, on 1 GPU and on 2 / 4 virtual ranks of the same GPU sharing out the
    iterations (and on 2 / 4 distinct GPUs when more than one is visible): the stat file's numIterations and time.

usage: python tools/shard_reduce_times.py [--parts abc] [--reps N]"""
import argparse
import ctypes as C
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import evplp_amd as ev  # noqa: E402

CASES = [(1920, 1080, n) for n in (2, 4, 8)] + [(1024, 1024, n) for n in (2, 4, 8)]
# evplp::launch_reduce_shards(const ShardPlanes &, int n, int first_nonzero, size_t count, float4 *out, int num_cus, hipStream_t)
LAUNCH = "_ZN5evplp20launch_reduce_shardsERKNS_11ShardPlanesEiimP15HIP_vector_typeIfLj4EEiP12ihipStream_t"


class ShardPlanes(C.Structure):
    _fields_ = [("p", C.c_void_p * 64)]


def local_rows(H):
    return (H + 15) // 16 * 16          # a whole-image rank of the group (16-row blocks)


def launcher():
    fn = getattr(ev.lib(), LAUNCH)
    fn.restype = None
    fn.argtypes = [C.POINTER(ShardPlanes), C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
    return fn


def kernel_launches(reps):
    """(a), the launches: returns {case: ms per launch by HIP events}"""
    fn = launcher()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    stream = torch.cuda.current_stream()
    out = {}
    for W, H, n in CASES:
        px = W * local_rows(H)
        planes = [torch.rand(px * 4, device="cuda", dtype=torch.float32) for _ in range(n)]
        dst = torch.empty(px * 4, device="cuda", dtype=torch.float32)
        src = ShardPlanes()
        for r, t in enumerate(planes):
            src.p[r] = t.data_ptr()
        for _ in range(3):
            fn(C.byref(src), n, 0, px, dst.data_ptr(), cus, stream.cuda_stream)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn(C.byref(src), n, 0, px, dst.data_ptr(), cus, stream.cuda_stream)
        e1.record(stream)
        torch.cuda.synchronize()
        ref = planes[0]
        for t in planes[1:]:
            ref = ref + t
        assert torch.equal(ref, dst), "reduce_shards_kernel disagrees with torch's rank-order float32 sum"
        out[f"{W}x{H} n={n}"] = e0.elapsed_time(e1) / reps
        del planes, dst
    return out


def rate(W, H, n, ms):
    b = (n + 1) * W * local_rows(H) * 16
    return {"bytes_per_plane": b, "gb_per_s": b / (ms * 1e-3) / 1e9 if ms > 0 else None}


def part_a(reps):
    ev_ms = kernel_launches(reps)
    res = {"what": "reduce_shards_kernel, one plane (sum mode), mean per launch; x3 for a written frame", "events": {}, "rocprofv3": {}}
    for W, H, n in CASES:
        k = f"{W}x{H} n={n}"
        res["events"][k] = {"ms": ev_ms[k], **rate(W, H, n, ev_ms[k])}
    # the same launches under rocprofv3 in a run of their own
    with tempfile.TemporaryDirectory() as d:
        cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--kernel-only", "--reps", str(reps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
            if p.returncode != 0 or not traces:
                res["rocprofv3"] = {"error": f"exit {p.returncode}: {(p.stderr or p.stdout)[-400:]}"}
            else:
                import csv
                rows = [r for r in csv.DictReader(open(traces[0])) if "reduce_shards_kernel" in r.get("Kernel_Name", "")]
                # launch order = CASES order, 3 warm-up launches + reps each
                per = 3 + reps
                for i, (W, H, n) in enumerate(CASES):
                    mine = rows[i * per + 3:(i + 1) * per]
                    if len(mine) != reps:
                        res["rocprofv3"][f"{W}x{H} n={n}"] = {"error": f"{len(mine)} launches traced"}
                        continue
                    ms = statistics.mean((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in mine)
                    res["rocprofv3"][f"{W}x{H} n={n}"] = {"ms": ms, **rate(W, H, n, ms)}
        except (OSError, subprocess.TimeoutExpired) as e:
            res["rocprofv3"] = {"error": str(e)}
    return res


def part_b(reps):
    W, H = 1920, 1080
    res = {"what": "one written frame at 1080p, host-clocked around the call, median ms", "cases": {}}
    for n in (2, 4):
        with ev.Group(W, H, 1024, 0, 4, n, devices=[0] * n, partition="iterations") as g:
            g.clear_accumulators()
            ctxs = [g.context(r) for r in range(n)]
            for r, c in enumerate(ctxs):                     # (some content: rank r's planes = r + 1)
                for b in (ev.BUF_VPL_ACCUM, ev.BUF_PHOTON_ACCUM):
                    c.upload(b, np.full((c.local_rows, W, 4), r + 1, np.float32))
            g.synchronize()
            dev = []
            for i in range(reps + 2):
                g.context(0)                                 # (the sums are stale: every resolve exchanges and reduces)
                t = time.perf_counter(); img = g.resolve(0.5, 0.5, 1.0); dt = time.perf_counter() - t
                if i >= 2:
                    dev.append(dt * 1e3)
            assert float(img[0, 0, 0]) == n * (n + 1) / 2
            host = []
            for i in range(reps + 2):
                t = time.perf_counter()
                own, acc = [], []
                for b in (ev.BUF_VPL_ACCUM, ev.BUF_PHOTON_ACCUM):
                    s = ctxs[0].download(b); own.append(s.copy())
                    for c in ctxs[1:]:
                        s += c.download(b)
                    acc.append(s)
                for b, s in zip((ev.BUF_VPL_ACCUM, ev.BUF_PHOTON_ACCUM), acc):
                    ctxs[0].upload(b, s)
                img_h = ctxs[0].resolve(0.5, 0.5, 1.0)
                for b, s in zip((ev.BUF_VPL_ACCUM, ev.BUF_PHOTON_ACCUM), own):
                    ctxs[0].upload(b, s)
                dt = time.perf_counter() - t
                if i >= 2:
                    host.append(dt * 1e3)
            assert np.array_equal(img_h[:H], img)
            res["cases"][f"n={n}"] = {"device_ms": statistics.median(dev), "host_path_ms": statistics.median(host),
                                      "host_path_bytes": 2 * n * W * local_rows(H) * 16 + 4 * W * local_rows(H) * 16}
    return res


def part_c():
    d = tempfile.mkdtemp(prefix="evplp_shard_cfg4_")
    jp = ev.synth_scene(d, "conf", 331000, 1234, 1920, 1080)
    runs = {"1 GPU": dict(gpus=1), "2 virtual": dict(gpus=2, virtual=True, partition="iterations"),
            "4 virtual": dict(gpus=4, virtual=True, partition="iterations")}
    ndev = torch.cuda.device_count()
    for k in (2, 4):
        if ndev >= k:
            runs[f"{k} GPUs"] = dict(gpus=k, partition="iterations")
    res = {"what": "config #4 block, timeLimitMs 3000, numMaxIteration -1: iterations completed", "visible_gpus": ndev, "runs": {}}
    for name, dev in runs.items():
        over = dict(numLightPaths=300000, numVplLightPaths=0, radiusPercentage=0.003, DoProgressive=True, AlphaProgressive=0.7, numMaxIteration=-1,
                    timeLimitMs=3000, frameMode="accumulate", run={"photonSplat": True}, combinedFilename="c.pfm", weightedVplFilename="v.pfm",
                    weightedPhotonFilename="p.pfm", statFilename="stat.json", useStat=True, device=dev)
        ev.render_json(jp, json.dumps(over))
        st = json.load(open(os.path.join(d, "stat.json")))
        res["runs"][name] = {"numIterations": st["numIterations"], "time_ms": st["time"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true", help="(a)'s launches alone: the child process rocprofv3 traces")
    a = ap.parse_args()
    if a.kernel_only:
        kernel_launches(a.reps)
        return
    # the library's progress lines (numIter: ..) go to stderr: stdout carries the JSON alone
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    out = {"device": torch.cuda.get_device_name(0)}
    if "a" in a.parts:
        out["a_kernel"] = part_a(a.reps)
    if "b" in a.parts:
        out["b_written_frame"] = part_b(a.reps)
    if "c" in a.parts:
        out["c_iterations_in_3s"] = part_c()
    sys.stdout.flush()
    json_out.write(json.dumps(out, indent=1) + "\n")
    json_out.flush()


if __name__ == "__main__":
    main()
