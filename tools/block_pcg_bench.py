#!/usr/bin/env python3
"""What block-Jacobi preconditioning (cgx_cg_set_block_precond)
costs per body and what it buys to a tolerance, on node_mixed matrices
(conjugategradient_amd.workloads): a 5-point Laplacian on nx x ny nodes with bs
unknowns per node, mixed inside each node by a matrix with singular values
10^U(0, e). b_i = i + 1, x0 = 0. One process, graph replay.

  * per body: µs over `--steps` bodies after `--warmup`, mode 3, for plain CG,
    Jacobi and block-Jacobi (block size = the node's unknowns). The three
    solvers take turns `--rounds` times after one untimed pass; the median and
    every round are printed, and the block body as a ratio to Jacobi's beside
    the byte model's ((86 + 8 bs) N + matrix against 94 N + matrix).
  * to 1e-8 ||b||: bodies, wall time and final residual for Jacobi and
    block-Jacobi, taking turns `--rounds` times, and for plain CG once, its
    bodies capped at 10 x Jacobi's.
  * setup: cgx_csr_block_inv and cgx_csr_diag_inv timed on their own (median
    of `--rounds`), beside the solves, not inside them.

    python tools/block_pcg_bench.py [--rounds 3] [--steps 400] [--warmup 20]
                                    [--configs 512x512x3,627x627x2,313x314x8]
                                    [--bodies-only]

--bodies-only runs the per-body part alone, one round (for a kernel trace).
Prints one JSON line per matrix and three tables.
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
from conjugategradient_amd.workloads import node_mixed  # noqa: E402

E, SEED = 1.5, 7


class Solver:
    """One cgx_cg in mode 3 on A: plain, Jacobi or block-Jacobi."""

    def __init__(self, q, A, b, x, kind, bs=0):
        self.L, self.q, self.b, self.x = lib(), q, b, x
        self.h = C.c_void_p()
        check(self.L.cgx_cg_create(q.handle, A.schedule(), C.byref(self.h)))
        check(self.L.cgx_cg_config(self.h, 64, 1))
        check(self.L.cgx_cg_set_mode(self.h, 3))
        if kind == "jacobi":
            check(self.L.cgx_cg_set_precond(self.h, 1, None))
        elif kind == "block":
            check(self.L.cgx_cg_set_block_precond(self.h, 1, bs, None))

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
            raise SystemExit(f"the timed window ended early: {tot.value} bodies, "
                             f"stopped {st.value}")
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


def timed_ms(q, call, rounds):
    out = []
    for _ in range(rounds + 1):  # the first pass untimed
        check(lib().cgx_sync(q.handle))
        t = time.perf_counter()
        check(call())
        check(lib().cgx_sync(q.handle))
        out.append(round((time.perf_counter() - t) * 1e3, 3))
    return out[1:]


def measure(q, nx, ny, bs, a):
    L = lib()
    rp, cl, vl = node_mixed(nx, ny, bs, E, SEED)
    n, nnz = len(rp) - 1, len(vl)
    name = f"node_mixed({nx}, {ny}, {bs}, {E})"
    A = cga.Matrix(q, vl, cl, rp)
    b = cga.DeviceArray(q, n, np.float64)
    x = cga.DeviceArray(q, n, np.float64)
    check(L.cgx_iota(q.handle, 0, b.ptr, n, 0.0))
    bnorm = float(np.sqrt(n * (n + 1) * (2 * n + 1) / 6.0))
    sb, v = C.c_int64(), C.c_int()
    check(L.cgx_csr_stream_bytes(A.schedule(), C.byref(sb)))
    check(L.cgx_csr_variant(A.schedule(), C.byref(v)))
    cfgs = {"plain": Solver(q, A, b, x, "plain"), "jacobi": Solver(q, A, b, x, "jacobi"),
            "block": Solver(q, A, b, x, "block", bs)}
    rounds = 1 if a.bodies_only else a.rounds
    us = {k: [] for k in cfgs}
    for r in range(rounds + 1):  # the three take turns: drift hits them alike
        for k, s in cfgs.items():
            t = round(s.body_us(a.steps, a.warmup), 2)
            if r:  # (the first pass is untimed)
                us[k].append(t)
    med = {k: statistics.median(vs) for k, vs in us.items()}
    out = {"matrix": name, "rows": n, "nnz": nnz, "block_size": bs, "spmv_variant": v.value,
           "matrix_stream_bytes": sb.value, "bodies_timed": a.steps, "rounds_us_per_body": us,
           "us_per_body": med,
           "ratio_jacobi_to_plain": round(med["jacobi"] / med["plain"], 4),
           "ratio_block_to_jacobi": round(med["block"] / med["jacobi"], 4),
           "ratio_block_to_jacobi_byte_model":
               round(((86.0 + 8 * bs) * n + sb.value) / (94.0 * n + sb.value), 4)}
    if not a.bodies_only:
        tol = 1e-8 * bnorm
        tt = {"jacobi": [], "block": []}
        for _ in range(rounds):
            for k in tt:
                kb, kt, kr = cfgs[k].to_tolerance(tol, -1)
                tt[k].append({"bodies": kb, "wall_ms": round(kt * 1e3, 2),
                              "rel_residual": float(np.sqrt(kr)) / bnorm})
        cap = 10 * tt["jacobi"][0]["bodies"]
        pb, pt, pr = cfgs["plain"].to_tolerance(tol, cap)
        tt["plain"] = [{"bodies": pb, "wall_ms": round(pt * 1e3, 2),
                        "rel_residual": float(np.sqrt(pr)) / bnorm, "body_cap": cap,
                        "stopped_by_rule": pb < cap}]
        out["to_1e-8"] = tt
        out["every_block_round_below_every_jacobi_round"] = (
            max(r["wall_ms"] for r in tt["block"]) < min(r["wall_ms"] for r in tt["jacobi"]))
        w = cga.DeviceArray(q, n * bs, np.float64)
        d = cga.DeviceArray(q, n, np.float64)
        out["setup_ms"] = {
            "cgx_csr_block_inv": timed_ms(q, lambda: L.cgx_csr_block_inv(A.schedule(), bs, w.ptr),
                                          rounds),
            "cgx_csr_diag_inv": timed_ms(q, lambda: L.cgx_csr_diag_inv(A.schedule(), d.ptr),
                                         rounds)}
    for s in cfgs.values():
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--configs", default="512x512x3,627x627x2,313x314x8",
                    help="nx x ny x bs, comma-separated")
    ap.add_argument("--bodies-only", action="store_true")
    a = ap.parse_args()
    q = cga.Queue(0)
    out = []
    for cfg in a.configs.split(","):
        nx, ny, bs = (int(t) for t in cfg.split("x"))
        out.append(measure(q, nx, ny, bs, a))
        print(json.dumps(out[-1]), flush=True)
    print("\n| matrix | rows | plain µs/body | Jacobi µs/body | block µs/body | block rounds | "
          "block / Jacobi | byte model |")
    print("|---|---|---|---|---|---|---|---|")
    for r in out:
        u = r["us_per_body"]
        print(f"| {r['matrix']} | {r['rows']} | {u['plain']} | {u['jacobi']} | {u['block']} | "
              f"{r['rounds_us_per_body']['block']} | {r['ratio_block_to_jacobi']} | "
              f"{r['ratio_block_to_jacobi_byte_model']} |")
    if a.bodies_only:
        return
    print("\nto 1e-8 ||b|| (plain CG's bodies capped at 10 x Jacobi's; residual: the loop's "
          "sqrt(r.r) / ||b||; ms per round)\n")
    print("| matrix | plain bodies | plain ms | plain residual | Jacobi bodies | Jacobi ms | "
          "Jacobi residual | block bodies | block ms | block residual | every block round below "
          "every Jacobi round |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in out:
        t = r["to_1e-8"]
        p, j, k = t["plain"][0], t["jacobi"], t["block"]
        pb = f"{p['bodies']}" + ("" if p["stopped_by_rule"] else " (cap)")
        print(f"| {r['matrix']} | {pb} | {p['wall_ms']} | {p['rel_residual']:.1e} | "
              f"{j[0]['bodies']} | {[q_['wall_ms'] for q_ in j]} | {j[0]['rel_residual']:.1e} | "
              f"{k[0]['bodies']} | {[q_['wall_ms'] for q_ in k]} | {k[0]['rel_residual']:.1e} | "
              f"{r['every_block_round_below_every_jacobi_round']} |")
    print("\n| matrix | cgx_csr_block_inv ms | cgx_csr_diag_inv ms |")
    print("|---|---|---|")
    for r in out:
        s = r["setup_ms"]
        print(f"| {r['matrix']} | {s['cgx_csr_block_inv']} | {s['cgx_csr_diag_inv']} |")


if __name__ == "__main__":
    main()
