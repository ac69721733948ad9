#!/usr/bin/env python3
"""The mixed-precision solve (cgx_mixed_solve) against the f64
auto-mode cgx_cg_solve, time to the same solution: A x = b, b_i = i + 1, to
1e-8 ||b|| on the true residual, on

  poisson 256^3, poisson 4096^2, the G3_circuit stand-in and
  irregular_spd(400_000, mean_deg=26, seed=12345).

Both solvers live in one process on one matrix. After one untimed solve each
(every graph captured) they take turns `--rounds` times; a round is the wall
time of the blocking solve call from x = 0. Medians and every round are
reported, with the bodies, the outer steps, cgx_mixed_bytes and, measured
separately over `--steps` graph-replayed bodies at tol 0, the µs per body of
the inner f32 solver (through cgx_mixed_inner) and of the f64 solver. `verdict`
is "mixed" only where the mixed solve reached the tolerance (status 1) and
every mixed round is below every f64 round.

    python tools/mixed_bench.py [--rounds 3] [--steps 200] [--small] [--log PATH]

Prints one JSON line per case and a table; the same text goes to the log
(default profiles/mixed_bench.log).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
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

POLL = 20   # divides the warm-up and the timed bodies; a multiple of 4 (the slot ring)
WARMUP = 20
_log = None


def say(text=""):
    print(text, flush=True)
    if _log:
        _log.write(text + "\n")
        _log.flush()


def body_us(q, cg, dtype, n, steps):
    """µs per body of `steps` graph-replayed bodies after WARMUP, b_i = i + 1,
    tol 0; None when the solver stops inside the window."""
    L = lib()
    code = 0 if dtype == np.float64 else 1
    b, x = cga.DeviceArray(q, n, dtype), cga.DeviceArray(q, n, dtype)
    check(L.cgx_iota(q.handle, code, b.ptr, n, 0.0))
    x.fill(0.0)
    tot, st = C.c_int64(), C.c_int()
    check(L.cgx_cg_config(cg, POLL, 1))
    check(L.cgx_cg_begin(cg, b.ptr, x.ptr, 0.0, WARMUP + steps + 1))
    check(L.cgx_cg_run(cg, WARMUP, C.byref(tot), C.byref(st)))
    check(L.cgx_cg_prepare(cg, steps))
    check(L.cgx_sync(q.handle))
    t = time.perf_counter()
    check(L.cgx_cg_run(cg, steps, C.byref(tot), C.byref(st)))
    check(L.cgx_sync(q.handle))
    dt = time.perf_counter() - t
    check(L.cgx_cg_config(cg, 32, 1))  # back to the defaults
    if tot.value != WARMUP + steps:
        return None
    return round(dt / steps * 1e6, 2)


def measure(q, name, A, a):
    L = lib()
    n, nnz = A.N(), A.NNZ()
    tol = 1e-8 * math.sqrt(n * (n + 1) * (2 * n + 1) / 6.0)  # ||1..n||
    b, x = cga.DeviceArray(q, n, np.float64), cga.DeviceArray(q, n, np.float64)
    check(L.cgx_iota(q.handle, 0, b.ptr, n, 0.0))
    cg, mx, cg32, a32 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    check(L.cgx_cg_create(q.handle, A.schedule(), C.byref(cg)))
    t = time.perf_counter()
    check(L.cgx_mixed_create(q.handle, A.schedule(), C.byref(mx)))
    create_s = time.perf_counter() - t
    check(L.cgx_mixed_inner(mx, C.byref(a32), C.byref(cg32)))
    m64, m32, v64, v32, by = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    check(L.cgx_cg_get_mode(cg, C.byref(m64)))
    check(L.cgx_cg_get_mode(cg32, C.byref(m32)))
    check(L.cgx_csr_variant(A.schedule(), C.byref(v64)))
    check(L.cgx_csr_variant(a32, C.byref(v32)))
    check(L.cgx_mixed_bytes(mx, C.byref(by)))

    def f64():
        x.fill(0.0)
        k, rxr = C.c_int64(), C.c_double()
        check(L.cgx_sync(q.handle))
        t = time.perf_counter()
        check(L.cgx_cg_solve(cg, b.ptr, x.ptr, tol, -1, C.byref(k), C.byref(rxr)))
        return time.perf_counter() - t, dict(bodies=k.value, rxr=rxr.value)

    def mixed():
        x.fill(0.0)
        o, k, rxr, st = C.c_int(), C.c_int64(), C.c_double(), C.c_int()
        check(L.cgx_sync(q.handle))
        t = time.perf_counter()
        check(L.cgx_mixed_solve(mx, b.ptr, x.ptr, tol, -1, C.byref(o), C.byref(k), C.byref(rxr),
                                C.byref(st)))
        dt = time.perf_counter() - t
        cnt = C.c_int()
        ib = (C.c_int64 * 64)()
        check(L.cgx_mixed_history(mx, None, ib, None, 64, C.byref(cnt)))
        return dt, dict(bodies=k.value, outer=o.value, status=st.value, rxr=rxr.value,
                        inner=list(ib[1:cnt.value]))

    runs = {"f64": f64, "mixed": mixed}
    info = {c: run()[1] for c, run in runs.items()}  # untimed: the graphs are captured
    acc = C.c_double()
    check(L.cgx_accuracy(q.handle, A.schedule(), b.ptr, x.ptr, C.byref(acc)))  # of the mixed x
    secs = {c: [] for c in runs}
    for _ in range(a.rounds):  # the solvers take turns: drift hits them alike
        for c, run in runs.items():
            dt, inf = run()
            assert inf == info[c], (inf, info[c])
            secs[c].append(round(dt, 5))
    us32 = body_us(q, cg32, np.float32, n, a.steps)
    us64 = body_us(q, cg, np.float64, n, a.steps)
    med = {c: statistics.median(v) for c, v in secs.items()}
    r = {"matrix": name, "rows": n, "nnz": nnz, "tol": tol,
         "f64": {"mode": m64.value, "spmv_variant": v64.value, **info["f64"]},
         "mixed": {"inner_mode": m32.value, "spmv_variant_f32": v32.value, **info["mixed"]},
         "true_residual_ok": bool(math.sqrt(info["mixed"]["rxr"]) <= tol),
         "accuracy_of_mixed_x": acc.value,  # cgx_accuracy: sum (b - A x)^2 / sum x^2
         "body_ratio": round(info["mixed"]["bodies"] / info["f64"]["bodies"], 3),
         "us_per_f32_body": us32, "us_per_f64_body": us64,
         "rounds_s": secs, "median_s": med,
         "speedup_mixed_over_f64": round(med["f64"] / med["mixed"], 3),
         "mixed_bytes": by.value, "mixed_create_s": round(create_s, 3),
         "verdict": "mixed" if info["mixed"]["status"] == 1 and max(secs["mixed"]) < min(secs["f64"])
         else "f64"}
    say(json.dumps(r))
    L.cgx_mixed_destroy(mx)
    L.cgx_cg_destroy(cg)
    return r


def main():
    global _log
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--small", action="store_true", help="a quick pass on small matrices")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "mixed_bench.log"))
    a = ap.parse_args()
    if a.steps % POLL:
        raise SystemExit(f"--steps must be a multiple of {POLL}")
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    _log = open(a.log, "w")
    say(f"# tools/mixed_bench.py --rounds {a.rounds} --steps {a.steps}{' --small' if a.small else ''}")
    q = cga.Queue(0)
    d, e = (16, 4) if a.small else (1, 1)  # rows / d; edges / e
    out = []
    cases = [(f"poisson {256 // e}^3",
              lambda: cga.Matrix.poisson(q, 3, 256 // e, 256 // e, 256 // e)),
             (f"poisson {4096 // e}^2", lambda: cga.Matrix.poisson(q, 2, 4096 // e, 4096 // e)),
             ("g3_standin", lambda: _host(q, irregular_spd(G3_ROWS // d, mean_deg=G3_MEAN_DEG,
                                                           seed=12345))),
             ("irregular mean_deg 26", lambda: _host(q, irregular_spd(400_000 // d, mean_deg=26,
                                                                      seed=12345)))]
    for name, make in cases:
        A = make()
        out.append(measure(q, name, A, a))
        del A
    say("\n| matrix | rows | f64 bodies (mode) | mixed bodies = inner solves (inner mode) | outer "
        "(status) | body ratio | µs / f64 body | µs / f32 body | f64 s | mixed s | f64 / mixed | "
        "mixed MB | verdict |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in out:
        f, m = r["f64"], r["mixed"]
        say(f"| {r['matrix']} | {r['rows']} | {f['bodies']} ({f['mode']}) | {m['bodies']} = "
            f"{' + '.join(map(str, m['inner']))} ({m['inner_mode']}) | {m['outer']} ({m['status']}) | "
            f"{r['body_ratio']} | {r['us_per_f64_body']} | {r['us_per_f32_body']} | "
            f"{r['median_s']['f64']} | {r['median_s']['mixed']} | {r['speedup_mixed_over_f64']} | "
            f"{r['mixed_bytes'] / 1e6:.1f} | {r['verdict']} |")
    _log.close()


def _host(q, csr):
    rp, cl, vl = csr
    return cga.Matrix(q, vl, cl, rp)


if __name__ == "__main__":
    main()
