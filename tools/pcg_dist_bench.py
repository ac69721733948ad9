#!/usr/bin/env python3
"""What diagonal preconditioning costs per body on a partitioned matrix
(DESIGN.md §5b "partitioned"): 2 ranks on one GPU over the host transport
with the device peer transport for the iteration (`host-peer`), 3-D Poisson
nx x ny x nz (default 256 x 256 x 64: each rank a 256 x 256 x 32 block, the
256^3 / 8 per-rank slab) scaled symmetrically as tests/test_pcg_cpu.py's
case() scales, A' = S A S with s_i = 10^U(0, 2).

The yardstick is the plain mode-3 partitioned body on the same matrix in the
same processes: the plain solver and the Jacobi solver take turns `--rounds`
times, `--steps` bodies after `--warmup`, graph replay; medians and every
round are printed, with the byte model's ratio (94 N + matrix) / (78 N +
matrix) per rank (matrix bytes: cgx_csr_stream_bytes) beside the measured one.

    python tools/pcg_dist_bench.py [--rounds 3] [--steps 400] [--warmup 20]
        [--grid 256 256 64] [--ranks 2] [--trace DIR]

--trace DIR adds the launch count per body from rocprofv3 kernel traces
(every rank under `rocprofv3 --kernel-trace --stats`, counters off): each
solver alone, eagerly launched, for B and 2 B bodies on a small grid; the
difference of the kernel call counts over B is the launches per body, free
of the setup's and the autotune's launches. The all-reduce kernels among
them (k_peer_allreduce, k_peer_allreduce2) are the tags per body.

This file is the driver and the worker: the driver starts each GPU step as
a child of its own under `timeout`, and stops at the first that fails.
Prints one JSON line and a table.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import re
import shutil
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NONE, JACOBI = 0, 1


# ---- worker (one per rank, under torch.distributed.run) ----------------------
def worker(a):
    import ctypes as C

    import numpy as np
    import torch.distributed as dist

    import conjugategradient_amd as cga
    from conjugategradient_amd._native import F64, check, lib
    from conjugategradient_amd.hostcomm import HostTransport
    from oracle import oracle as O

    world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist.init_process_group("gloo")
    L = lib()
    q = cga.Queue(local % max(1, cga.device_count()))
    transport = HostTransport()
    transport.attach(q, overlap=False)
    nx, ny, nz = a.grid
    n = nx * ny * nz
    base, extra = divmod(n, world)
    counts = [base + (r < extra) for r in range(world)]
    begin, nl = sum(counts[:rank]), counts[rank]
    # this rank's rows of the global matrix, generated with global columns and
    # scaled on the host (the scale vector is global and seeded)
    rp, cl, vl = (np.asarray(v) for v in O.poisson(3, nx, ny, nz))
    lo, hi = int(rp[begin]), int(rp[begin + nl])
    lrp = (rp[begin:begin + nl + 1] - lo).astype(np.int32)
    lcl = np.ascontiguousarray(cl[lo:hi], np.int32)
    s = 10.0 ** np.random.default_rng(9).uniform(0, 2.0, n)
    lvl = np.asarray(vl[lo:hi], np.float64) * np.repeat(s[begin:begin + nl], np.diff(lrp)) * s[lcl]
    del rp, cl, vl
    rows = cga.DeviceArray(q, nl + 1, np.int32).upload(lrp)
    cols = cga.DeviceArray(q, hi - lo, np.int32).upload(lcl)
    vals = cga.DeviceArray(q, hi - lo, np.float64).upload(lvl)
    A = C.c_void_p()
    check(L.cgx_csr_create_dist(q.handle, n, begin, nl, hi - lo, rows.ptr, cols.ptr, vals.ptr,
                                F64, C.byref(A)))
    peer = C.c_int(0)
    check(L.cgx_dist_peer_enable(A, C.byref(peer)))
    if not peer.value:
        raise SystemExit(f"rank {rank}: peer transport unavailable: {L.cgx_last_error().decode()}")
    coloc, onew, sb, var = C.c_int(), C.c_int(), C.c_int64(), C.c_int()
    check(L.cgx_dist_peer_form(A, C.byref(coloc), C.byref(onew)))
    check(L.cgx_csr_stream_bytes(A, C.byref(sb)))
    check(L.cgx_csr_variant(A, C.byref(var)))
    b = cga.DeviceArray(q, nl, np.float64)
    x = cga.DeviceArray(q, nl, np.float64)
    check(L.cgx_iota(q.handle, F64, b.ptr, nl, float(begin)))

    def solver(kind, graph):
        h = C.c_void_p()
        check(L.cgx_cg_create(q.handle, A, C.byref(h)))
        check(L.cgx_cg_config(h, 64, 1 if graph else 0))
        check(L.cgx_cg_set_mode(h, 3))
        check(L.cgx_cg_set_precond(h, kind, None))  # collective
        return h

    def body_us(h, steps, warmup, prepare=True):
        tot, st = C.c_int64(), C.c_int()
        x.fill(0.0)
        check(L.cgx_cg_begin(h, b.ptr, x.ptr, 0.0, warmup + steps + 1))
        check(L.cgx_cg_run(h, warmup, C.byref(tot), C.byref(st)))
        if prepare:
            check(L.cgx_cg_prepare(h, steps))
        check(L.cgx_sync(q.handle))
        dist.barrier()
        t = time.perf_counter()
        check(L.cgx_cg_run(h, steps, C.byref(tot), C.byref(st)))
        check(L.cgx_sync(q.handle))
        dt = time.perf_counter() - t
        if tot.value != warmup + steps:
            raise SystemExit(f"the timed window ended early: {tot.value} bodies, "
                             f"stopped {st.value}")
        return dt / steps * 1e6

    out = {"rank": rank, "rows": nl, "matrix_stream_bytes": int(sb.value),
           "spmv_variant": int(var.value), "peer_form": [int(coloc.value), int(onew.value)]}
    if a.only:  # a trace run: one solver alone, eager launches
        h = solver(JACOBI if a.only == "jacobi" else NONE, graph=False)
        body_us(h, a.steps, 0, prepare=False)
        L.cgx_cg_destroy(h)
    else:
        cfgs = {"plain": solver(NONE, True), "jacobi": solver(JACOBI, True)}
        us = {k: [] for k in cfgs}
        for _ in range(a.rounds):  # the two take turns: drift hits them alike
            for k, h in cfgs.items():
                us[k].append(round(body_us(h, a.steps, a.warmup), 2))
        for h in cfgs.values():
            L.cgx_cg_destroy(h)
        out["rounds_us_per_body"] = us
    everyone = [None] * world
    dist.all_gather_object(everyone, out)
    if rank == 0:
        print("RANKS " + json.dumps(everyone), flush=True)
    L.cgx_csr_destroy(A)
    q.close()
    dist.destroy_process_group()


# ---- driver -----------------------------------------------------------------
def port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def step(a, limit, extra, grid, trace_dir=None):
    """One GPU step: the ranks under torchrun, the whole under `timeout`."""
    me = os.path.abspath(__file__)
    prog = [sys.executable, me, "--worker", "--grid", *map(str, grid), *extra]
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "torch.distributed.run",
           "--nproc-per-node", str(a.ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port())]
    if trace_dir:  # the profiler starts the rank's program, not the other way round
        cmd += ["--no-python", shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3",
                "--kernel-trace", "--stats", "--output-format", "csv",
                "-d", trace_dir, "--"]
    else:
        cmd += ["--no-python"]
    print("step:", " ".join(extra), "grid", *grid, file=sys.stderr, flush=True)
    p = subprocess.run(cmd + prog, capture_output=True, text=True, cwd=ROOT)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"step failed with status {p.returncode}: nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RANKS ")][-1]
    return json.loads(line[6:])


def kernel_calls(trace_dir):
    """kernel name -> [calls, total ns], summed over the ranks' *kernel_stats.csv."""
    calls = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                m = re.search(r"\bk_\w+", row["Name"])
                name = m.group(0) if m else row["Name"]
                c = calls.setdefault(name, [0, 0])
                c[0] += int(row["Calls"])
                c[1] += int(row["TotalDurationNs"])
    return calls


def launches_per_body(a):
    """From two traces per solver (B and 2 B bodies): calls(2B) - calls(B) over
    B and over the ranks, per kernel name."""
    B, grid, out = 100, a.trace_grid, {}
    for only in ("plain", "jacobi"):
        got = []
        for bodies in (B, 2 * B):
            d = os.path.join(a.trace, f"{only}_{bodies}")
            os.makedirs(d, exist_ok=True)
            step(a, 240, ["--only", only, "--steps", str(bodies)], grid, d)
            got.append(kernel_calls(d))
        zero = [0, 0]
        per = {k: (got[1].get(k, zero)[0] - got[0].get(k, zero)[0]) / (B * a.ranks)
               for k in sorted(set(got[0]) | set(got[1]))}
        per = {k: v for k, v in per.items() if v}
        # the kernels' own durations per body (the 2 B run, setup launches included
        # for the names the setup shares): where the time of a body goes
        dur = {k: round(got[1][k][1] / (2 * B * a.ranks) / 1e3, 2) for k in per}
        out[only] = {"grid": list(grid), "kernels": per, "kernel_us_per_body": dur,
                     "launches_per_body": sum(per.values()),
                     "allreduce_tags_per_body": sum(v for k, v in per.items()
                                                    if "k_peer_allreduce" in k)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--grid", type=int, nargs=3, default=[256, 256, 64])
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--trace", default=None, help="directory for the rocprofv3 kernel traces")
    ap.add_argument("--trace-grid", type=int, nargs=3, default=[128, 128, 32],
                    help="grid of the trace runs (launch counts do not depend on it; the "
                         "kernels' durations do)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--only", choices=["plain", "jacobi"], default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    ranks = step(a, 900, ["--rounds", str(a.rounds), "--steps", str(a.steps),
                          "--warmup", str(a.warmup)], a.grid)
    # a body ends when the slowest rank's does: per round the maximum over the ranks
    us = {k: [max(r["rounds_us_per_body"][k][i] for r in ranks) for i in range(a.rounds)]
          for k in ("plain", "jacobi")}
    med = {k: statistics.median(v) for k, v in us.items()}
    ratios = [j / p for j, p in zip(us["jacobi"], us["plain"])]
    model = [(94.0 * r["rows"] + r["matrix_stream_bytes"]) /
             (78.0 * r["rows"] + r["matrix_stream_bytes"]) for r in ranks]
    res = {"grid": a.grid, "ranks": a.ranks, "transport": "host-peer",
           "peer_form": ranks[0]["peer_form"], "rows_per_rank": [r["rows"] for r in ranks],
           "spmv_variant": [r["spmv_variant"] for r in ranks],
           "matrix_stream_bytes": [r["matrix_stream_bytes"] for r in ranks],
           "bodies_timed": a.steps, "rounds_us_per_body": us,
           "per_rank_rounds_us_per_body": [r["rounds_us_per_body"] for r in ranks],
           "us_per_body": med, "ratio_jacobi_to_plain": round(med["jacobi"] / med["plain"], 4),
           "ratio_by_round": [round(v, 4) for v in ratios],
           "ratio_byte_model": round(max(model), 4)}
    res["excess_over_model_points"] = round(
        100.0 * (res["ratio_jacobi_to_plain"] - res["ratio_byte_model"]), 2)
    res["round_spread_points"] = round(100.0 * (max(ratios) - min(ratios)), 2)
    if a.trace:
        print(json.dumps(res), file=sys.stderr, flush=True)  # kept should a trace step fail
        res["trace"] = launches_per_body(a)
    print(json.dumps(res), flush=True)
    print("\n| grid | ranks | plain µs/body | Jacobi µs/body | Jacobi / plain | byte model | "
          "excess (points) | round spread (points) |")
    print("|---|---|---|---|---|---|---|---|")
    print(f"| {'x'.join(map(str, a.grid))} | {a.ranks} | {med['plain']} | {med['jacobi']} | "
          f"{res['ratio_jacobi_to_plain']} | {res['ratio_byte_model']} | "
          f"{res['excess_over_model_points']} | {res['round_spread_points']} |")
    if a.trace:
        for k, t in res["trace"].items():
            print(f"{k}: {t['launches_per_body']} launches and {t['allreduce_tags_per_body']} "
                  f"all-reduce kernels per body: {t['kernels']}; kernel µs per body on "
                  f"{'x'.join(map(str, t['grid']))}: {t['kernel_us_per_body']}")


if __name__ == "__main__":
    main()
