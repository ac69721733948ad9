#!/usr/bin/env python3
"""What Jacobi inside the many-systems kernel (cgx_many_set_precond, DESIGN.md
§5e) buys in time, not in bodies, on `--nsys` (4096) systems of one pattern:

  poisson32     tools/many_bench.py's: 2-D 5-point Poisson 32 x 32 (n = 1,024),
                system s scaled D A D with d = 10^U(0,1)
  irregular     tools/many_bench.py's: irregular_spd(1000, seed=12345),
                d = 10^U(0,0.25)
  poisson32w2   the same Poisson scaled by d = 10^U(0,2), where the plain loop
                is expected to end at its cap of n + 1 bodies

every b random with ||b|| = 1, x0 = 0, tol = 1e-8, generated as many_bench
does (same seed, so the first two are its very systems).

Contenders, taking turns `--rounds` times in one process after an untimed
pass each. `single` is launch-bound and leaves the device nearly idle, and the
17 ms plain call that follows it then runs 9 % slow (measured: 4.20 against
3.85 µs per system), which would flatter jacobi; so every round begins with
one more untimed plain call:

  plain    one cgx_many_solve call, no preconditioner (blocking; wall time
           around it, X zeroed before the clock starts)
  jacobi   the same call after cgx_many_set_precond(JACOBI): the diagonal is
           formed in the kernel at every solve, so its cost is inside
  single   per system a cgx_csr, a cgx_cg, cgx_cg_set_precond(JACOBI) and one
           blocking cgx_cg_solve in auto mode (3 under a preconditioner), on
           the first `--single` (256) systems. The solve is timed per system;
           the creates and cgx_cg_set_precond (which builds 1 / diag) are
           timed beside, not inside.

Per contender: µs per system, ns per system-body (time over the bodies its
systems ran) and the bodies per system, medians and every round; the ratio of
the medians plain / jacobi, and whether every jacobi round lies below every
plain round. No ratio is asserted.

    python tools/many_pcg_bench.py [--nsys 4096] [--single 256] [--rounds 3] [--small]
    python tools/many_pcg_bench.py --plain-only [--rounds 3]

--plain-only times the plain contender alone on many_bench's two workloads
and calls nothing a library without cgx_many_set_precond lacks: run it
through tools/ab_lib.py against a parent build, alternating with this one, to
see that the plain path did not move.

Prints one JSON line per workload and a table.
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
from conjugategradient_amd.workloads import irregular_spd  # noqa: E402

TOL = MB.TOL
JACOBI = 1


def time_single_jacobi(q, rp, cl, vals, B, count):
    """-> (solve seconds, create + set_precond seconds, bodies, X, mode) over
    the first `count` systems"""
    L = lib()
    n = len(rp) - 1
    t_solve = t_create = 0.0
    bodies, X = [], []
    mode = C.c_int()
    for s in range(count):
        A = cga.Matrix(q, vals[s], cl, rp)
        db = cga.DeviceArray(q, n, np.float64).upload(B[s])
        dx = cga.DeviceArray(q, n, np.float64)
        dx.fill(0.0)
        check(L.cgx_sync(q.handle))
        t = time.perf_counter()
        sched = A.schedule()
        h = C.c_void_p()
        check(L.cgx_cg_create(q.handle, sched, C.byref(h)))
        check(L.cgx_cg_set_precond(h, JACOBI, None))
        t_create += time.perf_counter() - t
        k, rr = C.c_int64(), C.c_double()
        t = time.perf_counter()
        check(L.cgx_cg_solve(h, db.ptr, dx.ptr, TOL, -1, C.byref(k), C.byref(rr)))
        t_solve += time.perf_counter() - t
        check(L.cgx_cg_get_mode(h, C.byref(mode)))
        bodies.append(k.value)
        X.append(dx.download())
        L.cgx_cg_destroy(h)
    return t_solve, t_create, np.array(bodies), np.stack(X), mode.value


def stats(b):
    return [int(b.min()), int(np.median(b)), int(b.max())]


def measure(q, name, rp, cl, vl, width, a):
    L = lib()
    nsys, n, nnz = a.nsys, len(rp) - 1, len(vl)
    vals, B = MB.systems(rp, cl, vl, nsys, width, seed=2024)
    d_rp = cga.DeviceArray(q, n + 1, np.int32).upload(rp)
    d_cl = cga.DeviceArray(q, nnz, np.int32).upload(cl)
    d_v = cga.DeviceArray(q, nsys * nnz, np.float64).upload(vals.ravel())
    dB = cga.DeviceArray(q, nsys * n, np.float64).upload(B.ravel())
    dX = cga.DeviceArray(q, nsys * n, np.float64)
    m = C.c_void_p()
    check(L.cgx_many_create(q.handle, F64, nsys, n, nnz, d_rp.ptr, d_cl.ptr, d_v.ptr, nnz,
                            C.byref(m)))
    cus = 256
    try:
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
    except Exception:
        pass

    def shape():
        wg, rpt, lds = C.c_int(), C.c_int(), C.c_int64()
        check(L.cgx_many_info(m, C.byref(wg), C.byref(rpt), C.byref(lds)))
        return {"rows_per_thread": rpt.value, "workgroups": wg.value, "lds_bytes": lds.value,
                "workgroups_per_cu": round(wg.value / cus, 2)}

    def many(kind):
        if not a.plain_only:
            check(L.cgx_many_set_precond(m, kind, None, 0))
        return MB.time_many(q, m, dB, dX, nsys, n)

    contenders = ["plain"] if a.plain_only else ["plain", "jacobi", "single"]
    ns = min(a.single, nsys)
    shapes = {"plain": shape()}
    many(0)  # untimed pass of each contender: code objects loaded
    if not a.plain_only:
        many(JACOBI)
        shapes["jacobi"] = shape()
        time_single_jacobi(q, rp, cl, vals, B, min(ns, 8))
    rounds = {c: [] for c in contenders + ["single_create"]}
    out = {}
    for _ in range(a.rounds):  # the contenders take turns: drift hits them alike
        many(0)  # untimed: the device busy again after `single` (module docstring)
        dt, out["plain_bodies"], out["plain_stopped"] = many(0)
        rounds["plain"].append(dt)
        if a.plain_only:
            continue
        dt, out["jacobi_bodies"], out["jacobi_stopped"] = many(JACOBI)
        Xj = dX.download().reshape(nsys, n)
        rounds["jacobi"].append(dt)
        ts, tc, sb, Xs, smode = time_single_jacobi(q, rp, cl, vals, B, ns)
        rounds["single"].append(ts)
        rounds["single_create"].append(tc)
    L.cgx_many_destroy(m)
    us = lambda xs, k: [round(x / k * 1e6, 3) for x in xs]  # noqa: E731
    nsb = lambda xs, k: [round(x / k * 1e9, 2) for x in xs]  # noqa: E731
    pb = out["plain_bodies"]
    r = {"workload": name, "nsys": nsys, "n": n, "nnz": nnz, "tol": TOL, "shape": shapes,
         "plain_bodies_min_med_max": stats(pb),
         "plain_at_cap": int((out["plain_stopped"] == 2).sum()),
         "us_per_system": {"plain": us(rounds["plain"], nsys)},
         "ns_per_system_body": {"plain": nsb(rounds["plain"], int(pb.sum()))}}
    if not a.plain_only:
        jb = out["jacobi_bodies"]
        r["jacobi_bodies_min_med_max"] = stats(jb)
        r["jacobi_stop_codes"] = {int(c): int((out["jacobi_stopped"] == c).sum())
                                  for c in np.unique(out["jacobi_stopped"])}
        r["single_systems"], r["single_auto_mode"] = ns, smode
        r["single_bodies_min_med_max"] = stats(sb)
        r["us_per_system"].update(jacobi=us(rounds["jacobi"], nsys), single=us(rounds["single"], ns),
                                  single_create=us(rounds["single_create"], ns))
        r["ns_per_system_body"].update(jacobi=nsb(rounds["jacobi"], int(jb.sum())),
                                       single=nsb(rounds["single"], int(sb.sum())))
        r["x_max_rel_diff_jacobi_vs_single"] = float(
            np.max(np.linalg.norm(Xj[:ns] - Xs, axis=1) / np.linalg.norm(Xs, axis=1)))
        r["bodies_identical_to_single"] = int((jb[:ns] == sb).sum())
    u = r["us_per_system"]
    r["median_us_per_system"] = {c: round(statistics.median(v), 3) for c, v in u.items()}
    if not a.plain_only:
        med = r["median_us_per_system"]
        r["plain_over_jacobi_time"] = round(med["plain"] / med["jacobi"], 3)
        r["plain_over_jacobi_bodies"] = round(float(pb.sum()) / float(jb.sum()), 3)
        r["every_jacobi_round_below_every_plain_round"] = max(u["jacobi"]) < min(u["plain"])
        r["every_jacobi_round_below_every_single_round"] = max(u["jacobi"]) < min(u["single"])
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsys", type=int, default=4096)
    ap.add_argument("--single", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a quick pass: 64 systems, 8 single")
    ap.add_argument("--plain-only", action="store_true",
                    help="the plain contender alone, for an A/B of two libraries")
    a = ap.parse_args()
    if a.small:
        a.nsys, a.single = 64, 8
    q = cga.Queue(0)
    out = [measure(q, "poisson32", *MB.poisson2d(32, 32), 1.0, a),
           measure(q, "irregular", *irregular_spd(1000, seed=12345), 0.25, a)]
    if not a.plain_only:
        out.append(measure(q, "poisson32w2", *MB.poisson2d(32, 32), 2.0, a))
    print("\n| workload | contender | µs per system (median; rounds) | ns per system-body "
          "(median) | bodies min, median, max |")
    print("|---|---|---|---|---|")
    med = lambda v: round(statistics.median(v), 3)  # noqa: E731
    for r in out:
        u, b = r["us_per_system"], r["ns_per_system_body"]
        for c in ("plain", "jacobi"):
            if c not in u:
                continue
            sh = r["shape"][c]
            print(f"| {r['workload']} | many {c} (R = {sh['rows_per_thread']}, {sh['workgroups']} "
                  f"workgroups, {sh['workgroups_per_cu']} per CU, {sh['lds_bytes']} B LDS) | "
                  f"{med(u[c])}; {u[c]} | {med(b[c])} | {r[c + '_bodies_min_med_max']}"
                  + (f", {r['plain_at_cap']} at the cap" if c == "plain" else "") + " |")
        if "single" in u:
            print(f"| | single, JACOBI, auto mode {r['single_auto_mode']} ({r['single_systems']} "
                  f"systems); create + set_precond beside | {med(u['single'])}; {u['single']}; "
                  f"beside {med(u['single_create'])} | {med(b['single'])} | "
                  f"{r['single_bodies_min_med_max']} |")
            print(f"| | plain / jacobi: time {r['plain_over_jacobi_time']}, bodies "
                  f"{r['plain_over_jacobi_bodies']}; every jacobi round below every plain round: "
                  f"{r['every_jacobi_round_below_every_plain_round']}, below every single round: "
                  f"{r['every_jacobi_round_below_every_single_round']} | | | |")


if __name__ == "__main__":
    main()
