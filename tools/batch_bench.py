#!/usr/bin/env python3
"""What the fused batch form (cgx_cg_solve_batch) costs per body
and per column against single solves, on the G3_circuit stand-in and on a
denser irregular matrix, irregular_spd(400_000, mean_deg=26, seed=12345).

For k in {1, 2, 4, 8} columns three contenders take turns, `--rounds` times in
one process, each timing `--steps` bodies after `--warmup`, all graph replay
(the poll interval divides both, so every timed chunk is a captured graph that
an untimed pass has built before):

  fused     cgx_cg_begin_batch / cgx_cg_run_batch with k columns
            (b_c = i + 1 + c): µs per body, and that over k per column
  single_1  cgx_cg_begin / cgx_cg_run in mode 1 on one column
  single_a  the same in the solver's auto mode: the yardstick, since k auto
            solves are what a caller runs without the batch

Medians and every round are printed, and beside each case the byte model's
ratio (S + k 80 N) / (k (S + 80 N)), S from cgx_csr_stream_bytes. `verdict`
is "fused" where every fused run's µs per body per column lies below every
single run's µs per body, single_a's and single_1's alike (the auto mode is
not always the faster single solve: a caller could pick mode 1), else
"sequential".

    python tools/batch_bench.py [--rounds 3] [--steps 400] [--warmup 20] [--small]

Prints one JSON line per case and a table. (No per-kernel times are recorded
for it: DESIGN.md §5c says why.)
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

POLL = 20  # divides the warm-up and the timed bodies; a multiple of 4 (the slot ring)


class Single:
    def __init__(self, q, A, n, mode):
        self.L, self.q, self.n = lib(), q, n
        self.h = C.c_void_p()
        check(self.L.cgx_cg_create(q.handle, A.schedule(), C.byref(self.h)))
        check(self.L.cgx_cg_config(self.h, POLL, 1))
        check(self.L.cgx_cg_set_mode(self.h, mode))
        m = C.c_int()
        check(self.L.cgx_cg_get_mode(self.h, C.byref(m)))
        self.mode = m.value
        self.b = cga.DeviceArray(q, n, np.float64)
        self.x = cga.DeviceArray(q, n, np.float64)
        check(self.L.cgx_iota(q.handle, 0, self.b.ptr, n, 0.0))

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
            raise SystemExit(f"single: the timed window ended early: {tot.value} bodies")
        return dt / steps * 1e6

    def close(self):
        self.L.cgx_cg_destroy(self.h)


class Fused:
    def __init__(self, q, A, n, k):
        self.L, self.q, self.n, self.k = lib(), q, n, k
        self.h = C.c_void_p()
        check(self.L.cgx_cg_create(q.handle, A.schedule(), C.byref(self.h)))
        check(self.L.cgx_cg_config(self.h, POLL, 1))
        check(self.L.cgx_cg_set_batch_form(self.h, 1))
        self.B = cga.DeviceArray(q, n * k, np.float64)
        self.X = cga.DeviceArray(q, n * k, np.float64)
        for c in range(k):
            check(self.L.cgx_iota(q.handle, 0, self.B.ptr + 8 * n * c, n, float(c)))

    def body_us(self, steps, warmup):
        L, tot, st, n, k = self.L, (C.c_int64 * 8)(), C.c_int(), self.n, self.k
        self.X.fill(0.0)
        check(L.cgx_cg_begin_batch(self.h, k, self.B.ptr, n, self.X.ptr, n, 0.0,
                                   warmup + steps + 1))
        check(L.cgx_cg_run_batch(self.h, warmup, tot, C.byref(st)))
        check(L.cgx_sync(self.q.handle))
        t = time.perf_counter()
        check(L.cgx_cg_run_batch(self.h, steps, tot, C.byref(st)))
        check(L.cgx_sync(self.q.handle))
        dt = time.perf_counter() - t
        if [tot[c] for c in range(k)] != [warmup + steps] * k:
            raise SystemExit(f"fused: the timed window ended early: {list(tot)[:k]}")
        return dt / steps * 1e6

    def close(self):
        self.L.cgx_cg_destroy(self.h)


def measure(q, name, rp, cl, vl, a):
    n, nnz = len(rp) - 1, len(vl)
    A = cga.Matrix(q, vl, cl, rp)
    sb, v = C.c_int64(), C.c_int()
    check(lib().cgx_csr_stream_bytes(A.schedule(), C.byref(sb)))
    check(lib().cgx_csr_variant(A.schedule(), C.byref(v)))
    s1, sa = Single(q, A, n, 1), Single(q, A, n, 0)
    out = []
    for k in a.columns:
        f = Fused(q, A, n, k)
        cfgs = {"fused": f, "single_1": s1, "single_a": sa}
        for s in cfgs.values():  # untimed: every graph of the timed windows is built
            s.body_us(a.steps, a.warmup)
        us = {c: [] for c in cfgs}
        for _ in range(a.rounds):  # the contenders take turns: drift hits them alike
            for c, s in cfgs.items():
                us[c].append(round(s.body_us(a.steps, a.warmup), 2))
        f.close()
        med = {c: statistics.median(vs) for c, vs in us.items()}
        S = float(sb.value)
        model = (S + k * 80.0 * n) / (k * (S + 80.0 * n))
        per_col = [u / k for u in us["fused"]]
        r = {"matrix": name, "rows": n, "nnz": nnz, "spmv_variant": v.value,
             "matrix_stream_bytes": sb.value, "k": k, "single_auto_mode": sa.mode,
             "bodies_timed": a.steps, "rounds_us_per_body": us, "us_per_body": med,
             "fused_us_per_body_per_column": round(med["fused"] / k, 2),
             "ratio_fused_per_column_to_single_1": round(med["fused"] / k / med["single_1"], 4),
             "ratio_fused_per_column_to_single_a": round(med["fused"] / k / med["single_a"], 4),
             "ratio_byte_model": round(model, 4),
             "verdict": "fused" if max(per_col) < min(us["single_a"] + us["single_1"])
             else "sequential"}
        print(json.dumps(r), flush=True)
        out.append(r)
    s1.close()
    sa.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--columns", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--small", action="store_true", help="a quick pass on 1/16 of the rows")
    a = ap.parse_args()
    if a.steps % POLL or a.warmup % POLL:
        raise SystemExit(f"--steps and --warmup must be multiples of {POLL}")
    q = cga.Queue(0)
    d = 16 if a.small else 1
    out = measure(q, "g3_standin", *irregular_spd(G3_ROWS // d, mean_deg=G3_MEAN_DEG, seed=12345),
                  a)
    out += measure(q, "irregular mean_deg 26", *irregular_spd(400_000 // d, mean_deg=26,
                                                              seed=12345), a)
    print("\n| matrix | k | fused µs/body | fused µs/body/column | single mode 1 µs/body | "
          "single auto µs/body (mode) | fused per column / auto | byte model | verdict |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in out:
        u = r["us_per_body"]
        print(f"| {r['matrix']} | {r['k']} | {u['fused']} | {r['fused_us_per_body_per_column']} | "
              f"{u['single_1']} | {u['single_a']} ({r['single_auto_mode']}) | "
              f"{r['ratio_fused_per_column_to_single_a']} | {r['ratio_byte_model']} | "
              f"{r['verdict']} |")


if __name__ == "__main__":
    main()
