#!/usr/bin/env python3
"""A workgroup per system against a wave per system (cgx_many_set_form,
DESIGN.md §5e "A wave per system") on many systems of at most 256 rows:

  poisson8      2-D 5-point Poisson 8 x 8     n = 64   R = 1   65,536 systems
  irregular60   irregular_spd(60, seed=12345) n = 60   R = 1   65,536 systems
  poisson11     Poisson 11 x 11               n = 121  R = 2   16,384 systems
  poisson16     Poisson 16 x 16               n = 256  R = 4   16,384 systems

every system scaled D A D with d = 10^U(0,0.25), b random with ||b|| = 1,
x0 = 0, tol = 1e-8, generated as tools/many_bench.py does (seed 2024). The
counts fill the wave form several times over (it can hold up to 32 waves on
each of 256 CUs at once).

Contenders, on ONE object, taking turns `--rounds` times in one process after
an untimed pass each (tools/many_bench.py's protocol: a blocking
cgx_many_solve, host clock around it, X zeroed before the clock starts):

  workgroup / wave            the plain loop in either form
  workgroup-j / wave-j        the same under cgx_many_set_precond(JACOBI)

Per contender: µs per system, ns per system-body and the bodies per system,
medians and every round. Per pair: whether every wave round lies below every
workgroup round, whether the medians differ by more than the workgroup form's
own round spread (max - min), and whether x and the bodies of the two forms
are identical. The two n <= 64 workloads decide what auto does;
no ratio is asserted here.

    python tools/many_wave_bench.py [--rounds 3] [--small] [--only NAME]

Prints one JSON line per workload and a table.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import conjugategradient_amd as cga  # noqa: E402
import many_bench as MB  # noqa: E402
from conjugategradient_amd._native import F64, check, lib  # noqa: E402
from conjugategradient_amd.workloads import irregular_spd  # noqa: E402

WORKGROUP, WAVE = 1, 2
JACOBI = 1
CONTENDERS = [("workgroup", WORKGROUP, 0), ("wave", WAVE, 0),
              ("workgroup-j", WORKGROUP, JACOBI), ("wave-j", WAVE, JACOBI)]


def measure(q, name, rp, cl, vl, nsys, a):
    L = lib()
    n, nnz = len(rp) - 1, len(vl)
    vals, B = MB.systems(rp, cl, vl, nsys, 0.25, seed=2024)
    d_rp = cga.DeviceArray(q, n + 1, np.int32).upload(rp)
    d_cl = cga.DeviceArray(q, nnz, np.int32).upload(cl)
    d_v = cga.DeviceArray(q, nsys * nnz, np.float64).upload(vals.ravel())
    dB = cga.DeviceArray(q, nsys * n, np.float64).upload(B.ravel())
    dX = cga.DeviceArray(q, nsys * n, np.float64)
    m = C.c_void_p()
    check(L.cgx_many_create(q.handle, F64, nsys, n, nnz, d_rp.ptr, d_cl.ptr, d_v.ptr, nnz,
                            C.byref(m)))
    req, eff = C.c_int(), C.c_int()
    check(L.cgx_many_get_form(m, C.byref(req), C.byref(eff)))
    auto_form = eff.value
    cus = 256
    try:
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
    except Exception:
        pass

    def run(form, kind):
        check(L.cgx_many_set_form(m, form))
        check(L.cgx_many_set_precond(m, kind, None, 0))
        dt, bodies, st = MB.time_many(q, m, dB, dX, nsys, n)
        wg, rpt, lds = C.c_int(), C.c_int(), C.c_int64()
        check(L.cgx_many_info(m, C.byref(wg), C.byref(rpt), C.byref(lds)))
        shape = {"rows": rpt.value, "workgroups": wg.value, "lds_bytes": lds.value,
                 "workgroups_per_cu": round(wg.value / cus, 2)}
        return dt, bodies, st, shape

    shapes, last = {}, {}
    for c, form, kind in CONTENDERS:  # untimed pass of each contender: code objects loaded
        shapes[c] = run(form, kind)[3]
    rounds = {c: [] for c, _, _ in CONTENDERS}
    for _ in range(a.rounds):  # the contenders take turns: drift hits them alike
        for c, form, kind in CONTENDERS:
            dt, bodies, st, _ = run(form, kind)
            rounds[c].append(dt)
            if c not in last:  # (first round: what it computed, to compare the two forms)
                last[c] = (dX.download().reshape(nsys, n), bodies, st)
    L.cgx_many_destroy(m)
    us = lambda xs, k: [round(x / k * 1e6, 4) for x in xs]  # noqa: E731
    nsb = lambda xs, k: [round(x / k * 1e9, 3) for x in xs]  # noqa: E731
    r = {"workload": name, "nsys": nsys, "n": n, "nnz": nnz, "tol": MB.TOL, "auto_form": auto_form,
         "shape": shapes, "us_per_system": {}, "ns_per_system_body": {}, "bodies_min_med_max": {},
         "stop_codes": {}}
    for c, _, _ in CONTENDERS:
        X, bodies, st = last[c]
        r["us_per_system"][c] = us(rounds[c], nsys)
        r["ns_per_system_body"][c] = nsb(rounds[c], int(bodies.sum()))
        r["bodies_min_med_max"][c] = [int(bodies.min()), int(np.median(bodies)), int(bodies.max())]
        r["stop_codes"][c] = {int(k): int((st == k).sum()) for k in np.unique(st)}
    u = r["us_per_system"]
    r["median_us_per_system"] = {c: round(statistics.median(v), 4) for c, v in u.items()}
    med = r["median_us_per_system"]
    for tag, wg, wv in (("plain", "workgroup", "wave"), ("jacobi", "workgroup-j", "wave-j")):
        spread = round(max(u[wg]) - min(u[wg]), 4)
        r[tag] = {
            "workgroup_over_wave_time": round(med[wg] / med[wv], 3),
            "every_wave_round_below_every_workgroup_round": max(u[wv]) < min(u[wg]),
            "workgroup_round_spread_us": spread,
            "medians_differ_by_more_than_that_spread": abs(med[wg] - med[wv]) > spread,
            "x_identical": bool(np.array_equal(last[wg][0], last[wv][0], equal_nan=True)),
            "bodies_identical": bool(np.array_equal(last[wg][1], last[wv][1])),
            "systems_with_other_bodies": int((last[wg][1] != last[wv][1]).sum()),
        }
    print(json.dumps(r), flush=True)
    return r


WORKLOADS = {
    "poisson8": (lambda: MB.poisson2d(8, 8), 65536),
    "irregular60": (lambda: irregular_spd(60, seed=12345), 65536),
    "poisson11": (lambda: MB.poisson2d(11, 11), 16384),
    "poisson16": (lambda: MB.poisson2d(16, 16), 16384),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a quick pass: 256 systems each")
    ap.add_argument("--only", choices=list(WORKLOADS), action="append")
    a = ap.parse_args()
    q = cga.Queue(0)
    out = []
    for name, (pattern, nsys) in WORKLOADS.items():
        if a.only and name not in a.only:
            continue
        out.append(measure(q, name, *pattern(), 256 if a.small else nsys, a))
    print("\n| workload | contender | µs per system (median; rounds) | ns per system-body "
          "(median) | bodies min, median, max |")
    print("|---|---|---|---|---|")
    med = lambda v: round(statistics.median(v), 4)  # noqa: E731
    for r in out:
        u, b = r["us_per_system"], r["ns_per_system_body"]
        for c, _, _ in CONTENDERS:
            sh = r["shape"][c]
            print(f"| {r['workload']} (n = {r['n']}, {r['nsys']} systems) | {c} (R = {sh['rows']}, "
                  f"{sh['workgroups']} workgroups, {sh['workgroups_per_cu']} per CU, "
                  f"{sh['lds_bytes']} B LDS) | {med(u[c])}; {u[c]} | {med(b[c])} | "
                  f"{r['bodies_min_med_max'][c]} |")
        for tag in ("plain", "jacobi"):
            t = r[tag]
            print(f"| | {tag}: workgroup / wave time {t['workgroup_over_wave_time']}; every wave "
                  f"round below every workgroup round: "
                  f"{t['every_wave_round_below_every_workgroup_round']}; medians apart by more than "
                  f"the workgroup spread ({t['workgroup_round_spread_us']} µs): "
                  f"{t['medians_differ_by_more_than_that_spread']}; x identical: "
                  f"{t['x_identical']}, bodies identical: {t['bodies_identical']} | | | |")


if __name__ == "__main__":
    main()
