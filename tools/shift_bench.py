#!/usr/bin/env python3
"""What multi-shift CG (cgx_cg_solve_shifted) costs against S
separate solves on explicitly shifted matrices, on the G3_circuit stand-in,
irregular_spd(400_000, mean_deg=26, seed=12345) and the 128^3 Poisson matrix.

Per body, S in {1, 2, 4, 8}: the contenders take turns, `--rounds` times in one
process, all graph replay. The shifted solve is blocking, so a body's time is
the difference of two solves at tol 0, with caps `--warmup` and `--warmup` +
`--steps`, over `--steps` (init and the host's share cancel); the single
solves are timed the same way, so both sides carry the same method.

  shifted   cgx_cg_solve_shifted with S shifts k * 1e-6 * (mean diagonal),
            small enough that no zeta leaves the normal range over the window
  single_1  cgx_cg_solve in mode 1 on S matrices A + sigma_k I, one after the
            other (the ladder's matrices below: a body's traffic does not
            depend on the value added to the diagonal), summed
  single_a  the same in each solver's auto mode

To 1e-8 ||b|| for a geometric ladder of 8 shifts, 1e-4 .. 1 times the mean
diagonal: one shifted solve against the 8 single solves (mode 1 and auto,
summed), the 8 cgx_csr_create calls reported separately (`create_ms`).

    python tools/shift_bench.py [--rounds 3] [--steps 200] [--warmup 40] [--small]

Prints one JSON line per case and a table.
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

POLL = 20


def poisson3d(nx):
    """7-point Poisson matrix of an nx^3 grid, rows in x-fastest order."""
    n = nx ** 3
    idx = np.arange(n)
    x, y, z = idx % nx, (idx // nx) % nx, idx // (nx * nx)
    cols = [(z > 0, idx - nx * nx), (y > 0, idx - nx), (x > 0, idx - 1), (x >= 0, idx),
            (x < nx - 1, idx + 1), (y < nx - 1, idx + nx), (z < nx - 1, idx + nx * nx)]
    keep = np.stack([c[0] for c in cols], axis=1)
    cl = np.stack([c[1] for c in cols], axis=1)[keep].astype(np.int32)
    vl = np.broadcast_to(np.array([-1.0, -1, -1, 6, -1, -1, -1]), (n, 7))[keep].copy()
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    return rp, cl, vl


class Solver:
    def __init__(self, q, A, n, mode):
        self.L, self.q, self.n = lib(), q, n
        self.h = C.c_void_p()
        check(self.L.cgx_cg_create(q.handle, A.schedule(), C.byref(self.h)))
        check(self.L.cgx_cg_config(self.h, POLL, 1))
        check(self.L.cgx_cg_set_mode(self.h, mode))
        m = C.c_int()
        check(self.L.cgx_cg_get_mode(self.h, C.byref(m)))
        self.mode = m.value

    def single(self, b, x, tol, cap):
        """seconds, bodies of cgx_cg_solve from x = 0"""
        tot, rxr = C.c_int64(), C.c_double()
        x.fill(0.0)
        check(self.L.cgx_sync(self.q.handle))
        t = time.perf_counter()
        check(self.L.cgx_cg_solve(self.h, b.ptr, x.ptr, tol, cap, C.byref(tot), C.byref(rxr)))
        check(self.L.cgx_sync(self.q.handle))
        return time.perf_counter() - t, tot.value

    def shifted(self, b, X, sig, tol, cap):
        k = len(sig)
        bo, ro, co = (C.c_int64 * 8)(), (C.c_double * 8)(), (C.c_int * 8)()
        check(self.L.cgx_sync(self.q.handle))
        t = time.perf_counter()
        check(self.L.cgx_cg_solve_shifted(self.h, k, (C.c_double * 8)(*sig), b.ptr, X.ptr, self.n,
                                          tol, cap, bo, ro, co))
        check(self.L.cgx_sync(self.q.handle))
        return time.perf_counter() - t, list(bo[:k]), list(co[:k])

    def close(self):
        self.L.cgx_cg_destroy(self.h)


def measure(q, name, rp, cl, vl, a):
    n, nnz = len(rp) - 1, len(vl)
    rows = np.repeat(np.arange(n), np.diff(rp))
    diag = np.nonzero(rows == cl)[0]
    assert len(diag) == n
    d = float(vl[diag].mean())
    ladder = [d * 10.0 ** (-4 + 4 * k / 7) for k in range(8)]
    small = [d * 1e-6 * (k + 1) for k in range(8)]
    bh = np.random.default_rng(21).standard_normal(n)
    b = cga.DeviceArray(q, n, np.float64).upload(bh)
    x = cga.DeviceArray(q, n, np.float64)
    X = cga.DeviceArray(q, 8 * n, np.float64)
    A = cga.Matrix(q, vl, cl, rp)
    sb = C.c_int64()
    check(lib().cgx_csr_stream_bytes(A.schedule(), C.byref(sb)))
    sh = Solver(q, A, n, 1)
    mats, create_ms = [], []
    for sg in ladder:
        vs = vl.copy()
        vs[diag] += sg
        t = time.perf_counter()
        m = cga.Matrix(q, vs, cl, rp)
        m.schedule()
        check(lib().cgx_sync(q.handle))
        create_ms.append(round((time.perf_counter() - t) * 1e3, 2))
        mats.append(m)
    s1 = [Solver(q, m, n, 1) for m in mats]
    sa = [Solver(q, m, n, 0) for m in mats]
    w, st = a.warmup, a.steps
    out = []

    def body_shift(S):
        t0, b0, _ = sh.shifted(b, X, small[:S], 0.0, w)
        t1, b1, _ = sh.shifted(b, X, small[:S], 0.0, w + st)
        if b0 != [w] * S or b1 != [w + st] * S:
            raise SystemExit(f"shifted: a shift froze inside the window: {b0} {b1}")
        return (t1 - t0) / st * 1e6

    def body_single(solvers, S):
        tot = 0.0
        for s in solvers[:S]:
            t0, k0 = s.single(b, x, 0.0, w)
            t1, k1 = s.single(b, x, 0.0, w + st)
            if (k0, k1) != (w, w + st):
                raise SystemExit(f"single: the window ended early: {k0} {k1}")
            tot += (t1 - t0) / st * 1e6
        return tot

    for S in a.shifts:
        cfgs = {"shifted": lambda: body_shift(S), "single_1": lambda: body_single(s1, S),
                "single_a": lambda: body_single(sa, S)}
        for f in cfgs.values():  # untimed: every graph of the timed windows is built
            f()
        us = {c: [] for c in cfgs}
        for _ in range(a.rounds):
            for c, f in cfgs.items():
                us[c].append(round(f(), 2))
        med = {c: statistics.median(v) for c, v in us.items()}
        Sb = float(sb.value)
        model = (Sb + 64.0 * n + 32.0 * n * S) / (S * (Sb + 80.0 * n))
        r = {"part": "per_body", "matrix": name, "rows": n, "nnz": nnz, "S": S,
             "single_auto_mode": sa[0].mode, "bodies_timed": st, "rounds_us_per_body": us,
             "us_per_body": med,
             "ratio_shifted_to_single_1": round(med["shifted"] / med["single_1"], 4),
             "ratio_shifted_to_single_a": round(med["shifted"] / med["single_a"], 4),
             "ratio_byte_model": round(model, 4)}
        print(json.dumps(r), flush=True)
        out.append(r)
    # the ladder to 1e-8 ||b||
    tol = 1e-8 * float(np.linalg.norm(bh))
    ms = {"shifted": [], "single_1": [], "single_a": []}
    info = {}
    for rnd in range(a.rounds + 1):  # the first pass untimed
        t, bodies, codes = sh.shifted(b, X, ladder, tol, -1)
        info["shifted_bodies"], info["shifted_codes"] = bodies, codes
        t1 = [s.single(b, x, tol, -1) for s in s1]
        ta = [s.single(b, x, tol, -1) for s in sa]
        info["single_bodies"] = [k for _, k in t1]
        if rnd:
            ms["shifted"].append(round(t * 1e3, 3))
            ms["single_1"].append(round(sum(v for v, _ in t1) * 1e3, 3))
            ms["single_a"].append(round(sum(v for v, _ in ta) * 1e3, 3))
    med = {c: statistics.median(v) for c, v in ms.items()}
    r = {"part": "ladder", "matrix": name, "rows": n, "shifts": ladder, "tol": tol, **info,
         "rounds_ms": ms, "ms": med, "create_ms": create_ms,
         "create_ms_total": round(sum(create_ms), 2),
         "ratio_shifted_to_single_1": round(med["shifted"] / med["single_1"], 4),
         "ratio_shifted_to_single_a": round(med["shifted"] / med["single_a"], 4)}
    print(json.dumps(r), flush=True)
    out.append(r)
    for s in [sh] + s1 + sa:
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--shifts", type=int, nargs="+", default=[1, 2, 4, 8])
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
    out += measure(q, "poisson 128^3" if d == 1 else "poisson 48^3",
                   *poisson3d(128 if d == 1 else 48), a)
    print("\n| matrix | S | shifted µs/body | S single mode 1 µs/body | S single auto µs/body "
          "(mode) | shifted / mode 1 | shifted / auto | byte model |")
    print("|---|---|---|---|---|---|---|---|")
    for r in out:
        if r["part"] != "per_body":
            continue
        u = r["us_per_body"]
        print(f"| {r['matrix']} | {r['S']} | {u['shifted']} | {u['single_1']} | {u['single_a']} "
              f"({r['single_auto_mode']}) | {r['ratio_shifted_to_single_1']} | "
              f"{r['ratio_shifted_to_single_a']} | {r['ratio_byte_model']} |")
    print("\n| matrix | shifted ms (bodies) | 8 single mode 1 ms | 8 single auto ms | "
          "8 cgx_csr_create ms | shifted / mode 1 | shifted / auto |")
    print("|---|---|---|---|---|---|---|")
    for r in out:
        if r["part"] != "ladder":
            continue
        print(f"| {r['matrix']} | {r['ms']['shifted']} ({max(r['shifted_bodies'])}) | "
              f"{r['ms']['single_1']} | {r['ms']['single_a']} | {r['create_ms_total']} | "
              f"{r['ratio_shifted_to_single_1']} | {r['ratio_shifted_to_single_a']} |")


if __name__ == "__main__":
    main()
