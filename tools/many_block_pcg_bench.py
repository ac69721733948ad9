#!/usr/bin/env python3
"""What block-Jacobi inside the many-systems kernels
(cgx_many_set_block_precond) buys in time, not in bodies,
against the in-kernel Jacobi (cgx_many_set_precond) and the plain loop on the
same object. The systems are leading principal submatrices of
workloads.node_mixed(nx, ny, bs, 1.5, 7) cut to n rows, system s scaled
D A D with d = 10^(0.25 U(0,1)) as tools/many_bench.py scales its own, every b
random with ||b|| = 1, x0 = 0, tol = 1e-8:

  n60b3     5 x 4 nodes x 3, 60 rows, 65,536 systems: the wave form (AUTO)
  n396b3    12 x 11 nodes x 3, 396 rows, 4,096 systems: 2 rows per thread
  n392b8    7 x 7 nodes x 8, 392 rows, 4,096 systems: bs = 8
  n3000b3   32 x 32 nodes x 3 cut to 3,000 rows, 4,096 systems: 16 rows per thread

Contenders, taking turns `--rounds` times in one process after an untimed pass
each; one blocking cgx_many_solve call, wall time around it, X zeroed before
the clock starts:

  plain    no preconditioner
  jacobi   cgx_many_set_precond(JACOBI)
  block    cgx_many_set_block_precond(JACOBI, bs): the fill launch that forms W
           from the values is inside the timed solve

Beside them `fill`: a blocking cgx_many_block_inv into an array of the
caller's, the same launch plus its verdicts' copy and wait, as a bound on the
fill's share of the block solve.

Per contender: µs per system, ns per system-body and the bodies per system,
medians and every round; whether every block round lies below every jacobi
round. No ratio is asserted.

    python tools/many_block_pcg_bench.py [--rounds 3] [--small] [--only NAME]

Prints one JSON line per workload and a table, and writes both to
profiles/many_block_pcg_bench.log.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import conjugategradient_amd as cga  # noqa: E402
import many_bench as MB  # noqa: E402
from conjugategradient_amd._native import F64, check, lib  # noqa: E402
from conjugategradient_amd.workloads import node_mixed  # noqa: E402

TOL = MB.TOL
NONE, JACOBI = 0, 1
# name: (nx, ny, bs, n, nsys)
WORKLOADS = {"n60b3": (5, 4, 3, 60, 65536), "n396b3": (12, 11, 3, 396, 4096),
             "n392b8": (7, 7, 8, 392, 4096), "n3000b3": (32, 32, 3, 3000, 4096)}
LOG = os.path.join(ROOT, "profiles", "many_block_pcg_bench.log")
_lines = []


def say(s=""):
    print(s, flush=True)
    _lines.append(s)


def cut(rp, cl, vl, n):
    """The leading principal n x n submatrix of a CSR matrix."""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    keep = (rows < n) & (cl < n)
    cnt = np.bincount(rows[keep], minlength=len(rp) - 1)[:n]
    return (np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32), cl[keep].astype(np.int32),
            vl[keep].astype(np.float64))


def systems(rp, cl, vl, nsys, width, seed, chunk=256):
    """MB.systems' scaling and right-hand sides, formed `chunk` systems at a time."""
    n = len(rp) - 1
    rng = np.random.default_rng(seed)
    row = np.repeat(np.arange(n), np.diff(rp))
    vals = np.empty((nsys, len(vl)))
    B = np.empty((nsys, n))
    for s0 in range(0, nsys, chunk):
        k = min(chunk, nsys - s0)
        D = 10.0 ** (width * rng.uniform(0.0, 1.0, (k, n)))
        vals[s0:s0 + k] = D[:, row] * vl[None, :] * D[:, cl]
        b = rng.standard_normal((k, n))
        B[s0:s0 + k] = b / np.linalg.norm(b, axis=1)[:, None]
    return vals, B


def stats(b):
    return [int(b.min()), int(np.median(b)), int(b.max())]


def measure(q, name, nx, ny, bs, n, nsys, a):
    L = lib()
    rp, cl, vl = cut(*node_mixed(nx, ny, bs, 1.5, 7), n)
    nnz = len(vl)
    vals, B = systems(rp, cl, vl, nsys, 0.25, seed=2024)
    d_rp = cga.DeviceArray(q, n + 1, np.int32).upload(rp)
    d_cl = cga.DeviceArray(q, nnz, np.int32).upload(cl)
    d_v = cga.DeviceArray(q, nsys * nnz, np.float64).upload(vals.ravel())
    dB = cga.DeviceArray(q, nsys * n, np.float64).upload(B.ravel())
    dX = cga.DeviceArray(q, nsys * n, np.float64)
    dW = cga.DeviceArray(q, nsys * n * bs, np.float64)
    del vals, B
    m = C.c_void_p()
    check(L.cgx_many_create(q.handle, F64, nsys, n, nnz, d_rp.ptr, d_cl.ptr, d_v.ptr, nnz,
                            C.byref(m)))

    def shape():
        wg, rpt, lds, eff = C.c_int(), C.c_int(), C.c_int64(), C.c_int()
        check(L.cgx_many_info(m, C.byref(wg), C.byref(rpt), C.byref(lds)))
        check(L.cgx_many_get_form(m, None, C.byref(eff)))
        return {"form": "wave" if eff.value == 2 else "workgroup", "rows_per_thread": rpt.value,
                "workgroups": wg.value, "lds_bytes": lds.value}

    def many(c):
        if c == "block":
            check(L.cgx_many_set_block_precond(m, JACOBI, bs, None, 0))
        else:
            check(L.cgx_many_set_precond(m, JACOBI if c == "jacobi" else NONE, None, 0))
        return MB.time_many(q, m, dB, dX, nsys, n)

    def fill():
        nb = C.c_int64()
        check(L.cgx_sync(q.handle))
        t = time.perf_counter()
        check(L.cgx_many_block_inv(m, bs, dW.ptr, n * bs, C.byref(nb), None))
        return time.perf_counter() - t, nb.value

    contenders = ["plain", "jacobi", "block"]
    shapes, rounds, out = {}, {c: [] for c in contenders + ["fill"]}, {}
    for c in contenders:  # an untimed pass of each: code objects loaded
        many(c)
        shapes[c] = shape()
    fill()
    for _ in range(a.rounds):  # the contenders take turns: drift hits them alike
        for c in contenders:
            dt, out[c + "_bodies"], out[c + "_stopped"] = many(c)
            rounds[c].append(dt)
        dt, out["bad_systems"] = fill()
        rounds["fill"].append(dt)
    L.cgx_many_destroy(m)
    us = lambda xs: [round(x / nsys * 1e6, 4) for x in xs]  # noqa: E731
    r = {"workload": name, "nsys": nsys, "n": n, "nnz": nnz, "bs": bs, "tol": TOL, "shape": shapes,
         "bad_systems": out["bad_systems"], "us_per_system": {}, "ns_per_system_body": {},
         "bodies_min_med_max": {}, "stop_codes": {}}
    for c in contenders:
        b = out[c + "_bodies"]
        r["us_per_system"][c] = us(rounds[c])
        r["ns_per_system_body"][c] = [round(x / max(int(b.sum()), 1) * 1e9, 2) for x in rounds[c]]
        r["bodies_min_med_max"][c] = stats(b)
        r["stop_codes"][c] = {int(k): int((out[c + "_stopped"] == k).sum())
                              for k in np.unique(out[c + "_stopped"])}
    r["us_per_system"]["fill"] = us(rounds["fill"])
    med = {c: statistics.median(v) for c, v in r["us_per_system"].items()}
    r["median_us_per_system"] = {c: round(v, 4) for c, v in med.items()}
    r["fill_share_of_block_solve"] = round(med["fill"] / med["block"], 4)
    r["jacobi_over_block_time"] = round(med["jacobi"] / med["block"], 3)
    r["jacobi_over_block_bodies"] = round(float(out["jacobi_bodies"].sum()) /
                                          float(out["block_bodies"].sum()), 3)
    u = r["us_per_system"]
    r["every_block_round_below_every_jacobi_round"] = max(u["block"]) < min(u["jacobi"])
    r["every_block_round_below_every_plain_round"] = max(u["block"]) < min(u["plain"])
    say(json.dumps(r))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a quick pass: 64 systems each")
    ap.add_argument("--only", default=None, help="one workload by name")
    a = ap.parse_args()
    q = cga.Queue(0)
    out = []
    for name, (nx, ny, bs, n, nsys) in WORKLOADS.items():
        if a.only in (None, name):
            out.append(measure(q, name, nx, ny, bs, n, 64 if a.small else nsys, a))
    say("\n| workload | contender | µs per system (median; rounds) | ns per system-body "
        "(median) | bodies min, median, max | stop codes |")
    say("|---|---|---|---|---|---|")
    med = lambda v: round(statistics.median(v), 4)  # noqa: E731
    for r in out:
        u, b = r["us_per_system"], r["ns_per_system_body"]
        for c in ("plain", "jacobi", "block"):
            sh = r["shape"][c]
            say(f"| {r['workload']} ({r['nsys']} x {r['n']}, bs {r['bs']}) | {c} ({sh['form']}, "
                f"R = {sh['rows_per_thread']}, {sh['workgroups']} workgroups, "
                f"{sh['lds_bytes']} B LDS) | {med(u[c])}; {u[c]} | {med(b[c])} | {r['bodies_min_med_max'][c]} | "
                f"{r['stop_codes'][c]} |")
        say(f"| | fill alone (cgx_many_block_inv, blocking) | {med(u['fill'])}; {u['fill']} | | | "
            f"{r['fill_share_of_block_solve']} of the block solve |")
        say(f"| | jacobi / block: time {r['jacobi_over_block_time']}, bodies "
            f"{r['jacobi_over_block_bodies']}; every block round below every jacobi round: "
            f"{r['every_block_round_below_every_jacobi_round']}, below every plain round: "
            f"{r['every_block_round_below_every_plain_round']} | | | | |")
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "w") as f:
        f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
