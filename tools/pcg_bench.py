#!/usr/bin/env python3
"""What diagonal preconditioning (cgx_cg_set_precond) costs per
body and what it buys to a tolerance, on the G3_circuit stand-in and on the
stand-in scaled symmetrically, A' = S A S with s_i = 10^U(0, 1.5) (seed 8):
the badly scaled system plain CG does not solve.

  * per body: µs over 400 bodies after 20, graph replay, for plain mode 3, for
    Jacobi in mode 3 with m read by plain loads (the default), and with m read
    by non-temporal loads ($CGX_PCG_M_NT=1, read by cgx_cg_set_precond). The
    three solvers take turns, `--rounds` times; the median and every round are
    printed. The byte model (94 N + matrix against 78 N + matrix) predicts the
    ratio printed beside the measured one.
  * to 1e-8 ||b||: bodies and wall time for Jacobi and for plain CG. Plain's
    body count is capped at 10 x Jacobi's (it would otherwise run to N + 1 on
    the scaled matrix); the line says whether it stopped by the rule.

    python tools/pcg_bench.py [--rounds 3] [--steps 400] [--warmup 20] [--rows N]

Prints one JSON line per matrix and two tables.
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
from conjugategradient_amd._native import check, lib  # noqa: E402
from conjugategradient_amd.workloads import G3_MEAN_DEG, G3_ROWS, irregular_spd  # noqa: E402

NONE, JACOBI = 0, 1


class Solver:
    """One cgx_cg in mode 3 on A, with or without Jacobi."""

    def __init__(self, q, A, b, x, kind, m_nt=False):
        self.L, self.q, self.b, self.x = lib(), q, b, x
        self.h = C.c_void_p()
        check(self.L.cgx_cg_create(q.handle, A.schedule(), C.byref(self.h)))
        check(self.L.cgx_cg_config(self.h, 64, 1))
        check(self.L.cgx_cg_set_mode(self.h, 3))
        if m_nt:
            os.environ["CGX_PCG_M_NT"] = "1"
        try:
            check(self.L.cgx_cg_set_precond(self.h, kind, None))
        finally:
            os.environ.pop("CGX_PCG_M_NT", None)

    def body_us(self, steps, warmup):
        L, tot, st = self.L, C.c_int64(), C.c_int()
        self.x.fill(0.0)
        check(L.cgx_cg_begin(self.h, self.b.ptr, self.x.ptr, 0.0, warmup + steps + 1))
        check(L.cgx_cg_run(self.h, warmup, C.byref(tot), C.byref(st)))
        check(L.cgx_cg_prepare(self.h, steps))
        check(L.cgx_sync(self.q.handle))
        t = time.perf_counter()
        check(L.cgx_cg_run(self.h, steps, C.byref(tot), C.byref(st)))
        check(L.cgx_sync(self.q.handle))
        dt = time.perf_counter() - t
        if tot.value != warmup + steps:
            raise SystemExit(f"the timed window ended early: {tot.value} bodies, stopped {st.value}")
        return dt / steps * 1e6

    def to_tolerance(self, tol, cap):
        L, tot, rxr = self.L, C.c_int64(), C.c_double()
        self.x.fill(0.0)
        check(L.cgx_sync(self.q.handle))
        t = time.perf_counter()
        check(L.cgx_cg_solve(self.h, self.b.ptr, self.x.ptr, tol, cap, C.byref(tot), C.byref(rxr)))
        check(L.cgx_sync(self.q.handle))
        return tot.value, time.perf_counter() - t, rxr.value

    def close(self):
        self.L.cgx_cg_destroy(self.h)


def measure(q, name, rp, cl, vl, a):
    n, nnz = len(rp) - 1, len(vl)
    A = cga.Matrix(q, vl, cl, rp)
    b = cga.DeviceArray(q, n, np.float64)
    x = cga.DeviceArray(q, n, np.float64)
    check(lib().cgx_iota(q.handle, 0, b.ptr, n, 0.0))
    bnorm = float(np.sqrt(n * (n + 1) * (2 * n + 1) / 6.0))
    sb, v = C.c_int64(), C.c_int()
    check(lib().cgx_csr_stream_bytes(A.schedule(), C.byref(sb)))
    check(lib().cgx_csr_variant(A.schedule(), C.byref(v)))
    cfgs = {"plain": Solver(q, A, b, x, NONE), "jacobi": Solver(q, A, b, x, JACOBI),
            "jacobi_m_nt": Solver(q, A, b, x, JACOBI, m_nt=True)}
    us = {k: [] for k in cfgs}
    for _ in range(a.rounds):  # the three take turns: drift hits them alike
        for k, s in cfgs.items():
            us[k].append(round(s.body_us(a.steps, a.warmup), 2))
    med = {k: statistics.median(vs) for k, vs in us.items()}
    # mode 3's body: 78 N + matrix bytes; m read twice adds 16 N
    model = (94.0 * n + sb.value) / (78.0 * n + sb.value)
    tol = 1e-8 * bnorm
    jb, jt, jr = cfgs["jacobi"].to_tolerance(tol, -1)
    cap = 10 * jb
    pb, pt, pr = cfgs["plain"].to_tolerance(tol, cap)
    for s in cfgs.values():
        s.close()
    return {"matrix": name, "rows": n, "nnz": nnz, "spmv_variant": v.value,
            "matrix_stream_bytes": sb.value, "bodies_timed": a.steps, "rounds_us_per_body": us,
            "us_per_body": med,
            "ratio_jacobi_to_plain": round(med["jacobi"] / med["plain"], 4),
            "ratio_jacobi_m_nt_to_plain": round(med["jacobi_m_nt"] / med["plain"], 4),
            "ratio_byte_model": round(model, 4),
            "to_1e-8": {"jacobi": {"bodies": jb, "wall_ms": round(jt * 1e3, 2),
                                   "rel_residual": float(np.sqrt(jr)) / bnorm},
                        "plain": {"bodies": pb, "wall_ms": round(pt * 1e3, 2),
                                  "rel_residual": float(np.sqrt(pr)) / bnorm,
                                  "body_cap": cap, "stopped_by_rule": pb < cap}}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", type=int, default=G3_ROWS, help="rows of the stand-in")
    a = ap.parse_args()
    q = cga.Queue(0)
    rp, cl, vl = irregular_spd(a.rows, mean_deg=G3_MEAN_DEG, seed=12345)
    s = 10.0 ** np.random.default_rng(8).uniform(0, 1.5, a.rows)
    rows = np.repeat(np.arange(a.rows), np.diff(rp))
    out = [measure(q, "g3_standin", rp, cl, vl, a),
           measure(q, "g3_standin scaled 10^U(0,1.5)", rp, cl, vl * s[rows] * s[cl], a)]
    for r in out:
        print(json.dumps(r), flush=True)
    print("\n| matrix | plain µs/body | Jacobi µs/body | Jacobi, m non-temporal | "
          "Jacobi / plain | byte model |")
    print("|---|---|---|---|---|---|")
    for r in out:
        u = r["us_per_body"]
        print(f"| {r['matrix']} | {u['plain']} | {u['jacobi']} | {u['jacobi_m_nt']} | "
              f"{r['ratio_jacobi_to_plain']} | {r['ratio_byte_model']} |")
    print("\nto 1e-8 ||b|| (plain CG's bodies capped at 10 x Jacobi's; residual: the loop's "
          "sqrt(r.r) / ||b||)\n")
    print("| matrix | plain bodies | plain ms | plain residual | Jacobi bodies | Jacobi ms | "
          "Jacobi residual |")
    print("|---|---|---|---|---|---|---|")
    for r in out:
        p, j = r["to_1e-8"]["plain"], r["to_1e-8"]["jacobi"]
        pb = f"{p['bodies']}" + ("" if p["stopped_by_rule"] else " (cap)")
        print(f"| {r['matrix']} | {pb} | {p['wall_ms']} | {p['rel_residual']:.1e} | "
              f"{j['bodies']} | {j['wall_ms']} | {j['rel_residual']:.1e} |")


if __name__ == "__main__":
    main()
