#!/usr/bin/env python3
"""What many small systems cost through cgx_many_solve against
the two routes a caller had before it, on `--nsys` (4096) systems of one
pattern each:

  poisson32    2-D 5-point Poisson 32 x 32 (n = 1,024), system s scaled
               symmetrically D A D with d = 10^U(0,1)
  irregular    irregular_spd(1000, seed=12345), d = 10^U(0,0.25)

every b random with ||b|| = 1, x0 = 0, tol = 1e-8 (so 1e-8 ||b|| per system).

Contenders, taking turns `--rounds` times in one process:

  many     one cgx_many_solve call on all systems (blocking; wall time around
           it, X zeroed before the clock starts)
  single   (a) the route without it: per system a cgx_csr and a cgx_cg in auto
           mode and one blocking cgx_cg_solve, on the first `--single` (256)
           systems. The solve is timed per system, first launch of that solver
           included (a caller with a new matrix pays it); cgx_csr_create +
           cgx_cg_create are timed separately and reported beside, not inside.
  blockdiag (b) one cgx_cg_solve in auto mode on the block-diagonal assembly
           of all systems, run for the K bodies after which every block's own
           true residual ||b_s - A_s x_s|| is at most its tol. K is found
           before the timed rounds (bodies in chunks of 20, A x by cgx_spmv,
           the norms on the host) and handed to the timed solve as its cap
           with tol = 0: (b) is timed with a perfect stop rule that costs
           nothing, the create is not timed.

Per contender: µs per system and ns per system-body (time over the bodies its
systems ran; for (b) nsys K), medians and every round, and whether every many
round lies below every round of (a) and of (b). Also the instantiation (rows
per thread), the grid and the workgroups per CU it ran at, and the largest
relative difference between many's x and (a)'s.

    python tools/many_bench.py [--nsys 4096] [--single 256] [--rounds 3] [--small]

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

import numpy as np  # noqa: E402

import conjugategradient_amd as cga  # noqa: E402
from conjugategradient_amd._native import F64, check, lib  # noqa: E402
from conjugategradient_amd.workloads import irregular_spd  # noqa: E402

TOL = 1e-8
CHUNK = 20


def poisson2d(nx, ny):
    n = nx * ny
    i = np.arange(n)
    ix, iy = i % nx, i // nx
    rows = [i[iy > 0], i[ix > 0], i, i[ix < nx - 1], i[iy < ny - 1]]
    cols = [i[iy > 0] - nx, i[ix > 0] - 1, i, i[ix < nx - 1] + 1, i[iy < ny - 1] + nx]
    vals = [np.full(len(r), -1.0) for r in rows]
    vals[2] = np.full(n, 4.0)
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((c, r))
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, r + 1, 1)
    return np.cumsum(rp).astype(np.int32), c[order].astype(np.int32), v[order]


def systems(rp, cl, vl, nsys, width, seed):
    n = len(rp) - 1
    rng = np.random.default_rng(seed)
    row = np.repeat(np.arange(n), np.diff(rp))
    D = 10.0 ** (width * rng.uniform(0.0, 1.0, (nsys, n)))
    vals = D[:, row] * vl[None, :] * D[:, cl]
    B = rng.standard_normal((nsys, n))
    B /= np.linalg.norm(B, axis=1)[:, None]
    return vals, B


def time_many(q, m, dB, dX, nsys, n):
    L = lib()
    dX.fill(0.0)
    check(L.cgx_sync(q.handle))
    bodies, rxr, st = (C.c_int64 * nsys)(), (C.c_double * nsys)(), (C.c_int * nsys)()
    t = time.perf_counter()
    check(L.cgx_many_solve(m, dB.ptr, n, dX.ptr, n, TOL, -1, bodies, rxr, st))
    dt = time.perf_counter() - t
    return dt, np.array(bodies[:]), np.array(st[:])


def time_single(q, rp, cl, vals, B, count):
    """-> (solve seconds, create seconds, bodies, X) over the first `count` systems"""
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


class BlockDiag:
    def __init__(self, q, rp, cl, vals, B):
        L = lib()
        nsys, nnz = vals.shape
        n = len(rp) - 1
        self.q, self.nsys, self.n, self.N = q, nsys, n, nsys * n
        off = np.arange(nsys, dtype=np.int64)
        brp = np.concatenate([(rp[:-1][None, :] + off[:, None] * nnz).ravel(), [nsys * nnz]])
        bcl = (cl[None, :].astype(np.int64) + off[:, None] * n).ravel()
        self.A = cga.Matrix(q, vals.ravel(), bcl.astype(np.int32), brp.astype(np.int32))
        self.h = C.c_void_p()
        check(L.cgx_cg_create(q.handle, self.A.schedule(), C.byref(self.h)))
        check(L.cgx_cg_config(self.h, CHUNK, 1))
        self.mode = C.c_int()
        check(L.cgx_cg_get_mode(self.h, C.byref(self.mode)))
        self.B = B
        self.b = cga.DeviceArray(q, self.N, np.float64).upload(B.ravel())
        self.x = cga.DeviceArray(q, self.N, np.float64)
        self.Ax = cga.DeviceArray(q, self.N, np.float64)

    def bodies_needed(self, limit):
        """The first multiple of CHUNK bodies after which every block's true
        residual is at most TOL (||b_s|| = 1); None past `limit`."""
        L = lib()
        self.x.fill(0.0)
        check(L.cgx_cg_begin(self.h, self.b.ptr, self.x.ptr, 0.0, limit))
        tot, st = C.c_int64(), C.c_int()
        while tot.value < limit:
            check(L.cgx_cg_run(self.h, CHUNK, C.byref(tot), C.byref(st)))
            check(L.cgx_spmv(self.q.handle, self.A.schedule(), self.x.ptr, self.Ax.ptr, self.N))
            res = (self.B - self.Ax.download().reshape(self.nsys, self.n))
            worst = float(np.max(np.linalg.norm(res, axis=1)))
            if worst <= TOL:
                return tot.value, worst
            if st.value:
                break
        return None, worst

    def timed(self, K):
        L = lib()
        self.x.fill(0.0)
        check(L.cgx_sync(self.q.handle))
        k, rr = C.c_int64(), C.c_double()
        t = time.perf_counter()
        check(L.cgx_cg_solve(self.h, self.b.ptr, self.x.ptr, 0.0, K, C.byref(k), C.byref(rr)))
        dt = time.perf_counter() - t
        if k.value != K:
            raise SystemExit(f"blockdiag: {k.value} bodies, expected {K}")
        return dt

    def close(self):
        lib().cgx_cg_destroy(self.h)


def measure(q, name, rp, cl, vl, width, a):
    L = lib()
    nsys, n, nnz = a.nsys, len(rp) - 1, len(vl)
    vals, B = systems(rp, cl, vl, nsys, width, seed=2024)
    d_rp = cga.DeviceArray(q, n + 1, np.int32).upload(rp)
    d_cl = cga.DeviceArray(q, nnz, np.int32).upload(cl)
    d_v = cga.DeviceArray(q, nsys * nnz, np.float64).upload(vals.ravel())
    dB = cga.DeviceArray(q, nsys * n, np.float64).upload(B.ravel())
    dX = cga.DeviceArray(q, nsys * n, np.float64)
    m = C.c_void_p()
    t = time.perf_counter()
    check(L.cgx_many_create(q.handle, F64, nsys, n, nnz, d_rp.ptr, d_cl.ptr, d_v.ptr, nnz,
                            C.byref(m)))
    many_create_ms = (time.perf_counter() - t) * 1e3
    wg, rpt, lds = C.c_int(), C.c_int(), C.c_int64()
    check(L.cgx_many_info(m, C.byref(wg), C.byref(rpt), C.byref(lds)))
    cus = 256
    try:
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
    except Exception:
        pass
    ns = min(a.single, nsys)
    bd = BlockDiag(q, rp, cl, vals, B)
    K, worst = bd.bodies_needed(limit=20 * n)
    # untimed pass of each contender: code objects loaded, (b)'s graphs built
    time_many(q, m, dB, dX, nsys, n)
    time_single(q, rp, cl, vals, B, min(ns, 8))
    if K:
        bd.timed(K)
    rounds = {"many": [], "single": [], "single_create": [], "blockdiag": []}
    for _ in range(a.rounds):  # the contenders take turns: drift hits them alike
        dt, bodies, st = time_many(q, m, dB, dX, nsys, n)
        Xm = dX.download().reshape(nsys, n)
        rounds["many"].append(dt)
        ts, tc, sb, Xs, smode = time_single(q, rp, cl, vals, B, ns)
        rounds["single"].append(ts)
        rounds["single_create"].append(tc)
        if K:
            rounds["blockdiag"].append(bd.timed(K))
    bd.close()
    L.cgx_many_destroy(m)
    diff = float(np.max(np.linalg.norm(Xm[:ns] - Xs, axis=1) / np.linalg.norm(Xs, axis=1)))
    mb, tot_sb = int(bodies.sum()), int(sb.sum())
    us = lambda xs, k: [round(x / k * 1e6, 3) for x in xs]  # noqa: E731
    nsb = lambda xs, k: [round(x / k * 1e9, 2) for x in xs]  # noqa: E731
    r = {"workload": name, "nsys": nsys, "n": n, "nnz": nnz, "tol": TOL,
         "rows_per_thread": rpt.value, "workgroups": wg.value, "lds_bytes": lds.value,
         "workgroups_per_cu": round(wg.value / cus, 2), "many_create_ms": round(many_create_ms, 2),
         "many_bodies_min_med_max": [int(bodies.min()), int(np.median(bodies)), int(bodies.max())],
         "many_all_stopped_by_rule": bool((st == 1).all()),
         "single_systems": ns, "single_auto_mode": smode,
         "single_bodies_min_med_max": [int(sb.min()), int(np.median(sb)), int(sb.max())],
         "blockdiag_auto_mode": bd.mode.value, "blockdiag_bodies": K,
         "blockdiag_worst_residual": worst,
         "us_per_system": {"many": us(rounds["many"], nsys), "single": us(rounds["single"], ns),
                           "single_create": us(rounds["single_create"], ns),
                           "blockdiag": us(rounds["blockdiag"], nsys)},
         "ns_per_system_body": {"many": nsb(rounds["many"], mb),
                                "single": nsb(rounds["single"], tot_sb),
                                "blockdiag": nsb(rounds["blockdiag"], nsys * K) if K else []},
         "x_max_rel_diff_many_vs_single": diff}
    u = r["us_per_system"]
    r["median_us_per_system"] = {c: round(statistics.median(v), 3) if v else None
                                 for c, v in u.items()}
    r["every_many_round_below_every_single_round"] = max(u["many"]) < min(u["single"])
    r["every_many_round_below_every_blockdiag_round"] = (
        bool(u["blockdiag"]) and max(u["many"]) < min(u["blockdiag"]))
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsys", type=int, default=4096)
    ap.add_argument("--single", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a quick pass: 64 systems, 8 single")
    a = ap.parse_args()
    if a.small:
        a.nsys, a.single = 64, 8
    q = cga.Queue(0)
    out = [measure(q, "poisson32", *poisson2d(32, 32), 1.0, a),
           measure(q, "irregular", *irregular_spd(1000, seed=12345), 0.25, a)]
    print("\n| workload | contender | µs per system (median; rounds) | ns per system-body "
          "(median) | bodies |")
    print("|---|---|---|---|---|")
    for r in out:
        u, b = r["us_per_system"], r["ns_per_system_body"]
        med = lambda v: round(statistics.median(v), 3) if v else "not measured"  # noqa: E731
        print(f"| {r['workload']} | many (R = {r['rows_per_thread']}, {r['workgroups']} workgroups, "
              f"{r['workgroups_per_cu']} per CU) | {med(u['many'])}; {u['many']} | {med(b['many'])} | "
              f"{r['many_bodies_min_med_max']} |")
        print(f"| | (a) single, auto mode {r['single_auto_mode']} ({r['single_systems']} systems); "
              f"create beside | {med(u['single'])}; {u['single']}; create {med(u['single_create'])} "
              f"| {med(b['single'])} | {r['single_bodies_min_med_max']} |")
        print(f"| | (b) block diagonal, auto mode {r['blockdiag_auto_mode']} | {med(u['blockdiag'])}; "
              f"{u['blockdiag']} | {med(b['blockdiag'])} | {r['blockdiag_bodies']} |")
        print(f"| | every many round below every round of (a): "
              f"{r['every_many_round_below_every_single_round']}, of (b): "
              f"{r['every_many_round_below_every_blockdiag_round']} | | | |")


if __name__ == "__main__":
    main()
