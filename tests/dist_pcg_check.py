#!/usr/bin/env python3
"""Multi-rank check of diagonal preconditioning on partitioned matrices
(cgx_cg_set_precond on a cgx_csr_create_dist matrix; DESIGN.md §5b
"partitioned"), one process per rank, launched with torch.distributed.run:

  python -m torch.distributed.run --nproc-per-node W --master-addr 127.0.0.1 \
      --master-port P tests/dist_pcg_check.py --case p3d --transport host-peer \
      --steps jacobi@1@30,jacobi@3@30

The Python classes have no partitioned constructor: the ctypes level used
here (and by tests/dist_check.py) is the partitioned surface.

One launch runs several steps on the same partitioned matrix, so process
start-up is paid once per configuration. A step is kind[@mode[@bodies[@runs]]]:

  kind    jacobi   CGX_PRECOND_JACOBI
          plain    no preconditioner
          ones     CGX_PRECOND_DIAGONAL with m == 1
          diag     CGX_PRECOND_DIAGONAL with m = 10^U(-1, 1), seeded
          diagjac  CGX_PRECOND_DIAGONAL with the caller's m = 1 / diag(A)
          f32jac   Jacobi on an f32 copy of the matrix, to 1e-3 ||b||
          mode4    mode 4 with a preconditioner is refused, both call orders
          errors   the collective error paths, on a small matrix of its own
  mode    cgx_cg_set_mode; a+b+... gives rank r the r-th entry (default --mode)
  bodies  >= 0: that many bodies at tol 0; -1: to 1e-8 ||b|| (default -1)
  runs    split the solve into this many cgx_cg_run calls (default --runs)

The matrices are tests.test_pcg_cpu.case(name), the project's scaled
matrices, or "poisson": the unscaled 3-D Poisson 128 x 128 x 48 (constant
coefficients, so the lean interior walk applies). Every rank slices its
contiguous row block from the global CSR on the host and uploads it with
global column indices. Rank 0 gathers x and checks it against
tests.test_pcg_cpu.pcg / jacobi_ref on the global matrix, and prints one JSON
line: per step the bodies, the modes run, r.r and r.z as every rank read
them, x's sha256, the distance to the checker and the true residual.
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401
import torch.distributed as dist  # noqa: E402

import conjugategradient_amd as cga  # noqa: E402
from conjugategradient_amd._native import F32, F64, check, lib  # noqa: E402
from tests import test_pcg_cpu as K  # noqa: E402

NONE, JACOBI, DIAGONAL = 0, 1, 2
DIAG_SEED = 11


def global_case(name):
    if name == "poisson":
        from oracle import oracle as O
        rp, cl, vl = O.poisson(3, 128, 128, 48)
        rp, cl = np.asarray(rp, np.int32), np.asarray(cl, np.int32)
        vl = np.asarray(vl, np.float64)
        return rp, cl, vl, np.arange(1, len(rp), dtype=np.float64)
    return K.case(name)


def random_m(n):
    return 10.0 ** np.random.default_rng(DIAG_SEED).uniform(-1, 1, n)


class Ranked:
    """This rank's block of a global CSR as a partitioned device matrix."""

    def __init__(self, q, rp, cl, vl, dtype=np.float64):
        self.q, self.dtype = q, np.dtype(dtype)
        self.code = F32 if self.dtype == np.float32 else F64
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.n = len(rp) - 1
        base, extra = divmod(self.n, self.world)
        self.counts = [base + (r < extra) for r in range(self.world)]
        self.begin = sum(self.counts[:self.rank])
        self.nl = self.counts[self.rank]
        a, b = self.begin, self.begin + self.nl
        lrp = (rp[a:b + 1] - rp[a]).astype(np.int32)
        nnz = int(lrp[-1])
        self.rows = cga.DeviceArray(q, self.nl + 1, np.int32).upload(lrp)
        self.cols = cga.DeviceArray(q, max(nnz, 1), np.int32)
        self.vals = cga.DeviceArray(q, max(nnz, 1), self.dtype)
        if nnz:
            self.cols.upload(np.ascontiguousarray(cl[rp[a]:rp[b]], np.int32))
            self.vals.upload(np.ascontiguousarray(vl[rp[a]:rp[b]], self.dtype))
        self.A = C.c_void_p()
        check(lib().cgx_csr_create_dist(q.handle, self.n, a, self.nl, nnz, self.rows.ptr,
                                        self.cols.ptr, self.vals.ptr, self.code,
                                        C.byref(self.A)))

    def local(self, v):
        return np.ascontiguousarray(v[self.begin:self.begin + self.nl], self.dtype)

    def vec(self, v=None):
        d = cga.DeviceArray(self.q, self.nl, self.dtype)
        if v is None:
            d.fill(0.0)
        else:
            d.upload(self.local(v))
        return d

    def gather(self, dev):
        """The global vector on rank 0 (None elsewhere)."""
        mx = max(self.counts)
        xl = torch.zeros(mx, dtype=torch.float64)
        xl[:self.nl] = torch.from_numpy(dev.download().astype(np.float64))
        if self.world == 1:
            return xl[:self.nl].numpy().astype(self.dtype)
        xs = [torch.empty(mx, dtype=torch.float64) for _ in self.counts] if self.rank == 0 else None
        dist.gather(xl, xs, dst=0)
        if self.rank:
            return None
        return torch.cat([t[:c] for t, c in zip(xs, self.counts)]).numpy().astype(self.dtype)

    def destroy(self):
        lib().cgx_csr_destroy(self.A)


def everyone(value):
    out = [None] * dist.get_world_size()
    dist.all_gather_object(out, value)
    return out


def solve(M, cg, b, x, tol, bodies, runs):
    """-> bodies run, stopped, r.r, r.z (nan without a preconditioner)."""
    L = lib()
    done, stopped = C.c_int64(), C.c_int(0)
    check(L.cgx_cg_begin(cg, b.ptr, x.ptr, tol, bodies))
    if runs > 1:
        per = max(1, (bodies if bodies >= 0 else 120) // runs)
        while not stopped.value:
            check(L.cgx_cg_run(cg, per, C.byref(done), C.byref(stopped)))
    else:
        check(L.cgx_cg_run(cg, M.n + 1, C.byref(done), C.byref(stopped)))
    rxr, rz, kind = C.c_double(), C.c_double(float("nan")), C.c_int()
    check(L.cgx_cg_rxr(cg, C.byref(rxr)))
    check(L.cgx_cg_get_precond(cg, C.byref(kind)))
    if kind.value != NONE:
        check(L.cgx_cg_rz(cg, C.byref(rz)))
    return int(done.value), int(stopped.value), rxr.value, rz.value


def run_step(M, name, gc, kind, modes, bodies, runs):
    L = lib()
    rp, cl, vl, bg = gc
    dt = M.dtype
    tol_rel = 1e-3 if kind == "f32jac" else 1e-8
    tol = 0.0 if bodies >= 0 else tol_rel * float(np.linalg.norm(bg))
    cg = C.c_void_p()
    check(L.cgx_cg_create(M.q.handle, M.A, C.byref(cg)))
    check(L.cgx_cg_set_mode(cg, modes[M.rank % len(modes)]))
    m_dev, m_glob = None, None
    if kind in ("jacobi", "f32jac"):
        check(L.cgx_cg_set_precond(cg, JACOBI, None))
        m_glob = 1.0 / K.diag_of(rp, cl, vl)
    elif kind in ("ones", "diag", "diagjac"):
        m_glob = (np.ones(M.n) if kind == "ones" else random_m(M.n) if kind == "diag"
                  else 1.0 / K.diag_of(rp, cl, vl))
        m_dev = M.vec(m_glob)
        check(L.cgx_cg_set_precond(cg, DIAGONAL, m_dev.ptr))
    b, x = M.vec(bg), M.vec()
    done, stopped, rxr, rz = solve(M, cg, b, x, tol, bodies, runs)
    mode_run = C.c_int()
    check(L.cgx_cg_get_mode(cg, C.byref(mode_run)))
    seen = everyone((done, stopped, rxr, rz, int(mode_run.value)))
    xg = M.gather(x)
    L.cgx_cg_destroy(cg)
    if M.rank:
        return None
    out = {"kind": kind, "mode": "+".join(map(str, modes)), "bodies": done, "stopped": stopped,
           "rxr": rxr, "rz": None if np.isnan(rz) else rz, "runs": runs,
           "modes_run": [s[4] for s in seen],
           # every rank read the same bodies, stop and world values
           "ranks_agree": all(s[:2] == seen[0][:2] and s[2] == seen[0][2] and
                              (s[3] == seen[0][3] or (np.isnan(s[3]) and np.isnan(seen[0][3])))
                              for s in seen),
           "x_sha": hashlib.sha256(xg.tobytes()).hexdigest()[:16],
           "finite": bool(np.isfinite(xg).all())}
    x64 = xg.astype(np.float64)
    out["residual"] = float(np.linalg.norm(bg - K.spmv(rp, cl, vl, x64)) / np.linalg.norm(bg))
    if kind in ("jacobi", "diagjac", "diag") and dt == np.float64:
        if name in K.CASES and kind != "diag":
            xr, kr, rr, rzr = K.jacobi_ref(name, 0.0 if bodies >= 0 else 1e-8, bodies)
        else:
            xr, kr, rr, rzr = K.pcg(rp, cl, vl, bg, m_glob, tol, False, bodies)
        out.update(ref_bodies=kr, ref_rxr=rr, ref_rz=rzr,
                   rel=float(np.linalg.norm(x64 - xr) / np.linalg.norm(xr)))
    return out


def mode4_step(M):
    """Mode 4 with a preconditioner on this partitioned matrix: refused in
    both call orders, with the supported modes in the message."""
    L = lib()
    out = {"kind": "mode4"}
    got = C.c_int(-1)
    cg = C.c_void_p()
    check(L.cgx_cg_create(M.q.handle, M.A, C.byref(cg)))
    out["set_mode4"] = L.cgx_cg_set_mode(cg, 4)  # the mode itself runs on this matrix
    rc = L.cgx_cg_set_precond(cg, JACOBI, None)
    msg = L.cgx_last_error().decode()
    check(L.cgx_cg_get_precond(cg, C.byref(got)))
    out["mode_then_precond"] = everyone((rc, msg, got.value))
    L.cgx_cg_destroy(cg)
    cg = C.c_void_p()
    check(L.cgx_cg_create(M.q.handle, M.A, C.byref(cg)))
    check(L.cgx_cg_set_precond(cg, JACOBI, None))
    check(L.cgx_cg_get_mode(cg, C.byref(got)))
    auto = got.value
    rc = L.cgx_cg_set_mode(cg, 4)
    msg = L.cgx_last_error().decode()
    check(L.cgx_cg_get_mode(cg, C.byref(got)))
    out["precond_then_mode"] = everyone((rc, msg, auto, got.value))
    L.cgx_cg_destroy(cg)
    return None if M.rank else out


def errors_step(q):
    """The collective error paths on 2-D Poisson 6 x 5, scaled: a zero
    diagonal in a row of the last rank, then a non-positive entry in the last
    rank's d_minv. Every rank must return the same code and message (with the
    GLOBAL index), keep CGX_PRECOND_NONE, and a plain solve on the same
    handles must complete afterwards: no collective was left half-entered."""
    from oracle import oracle as O
    L = lib()
    rp, cl, vl = (np.array(a) for a in O.poisson(2, 6, 5, 1))
    rp, cl, vl = rp.astype(np.int32), cl.astype(np.int32), vl.astype(np.float64)
    n = len(rp) - 1
    s = 10.0 ** np.random.default_rng(5).uniform(0, 2.0, n)
    vl = vl * s[K.rows_of(rp)] * s[cl]
    world, rank = dist.get_world_size(), dist.get_rank()
    out = {"kind": "errors", "n": n}

    def plain_solve(M, cg):
        b, x = M.vec(np.arange(1, n + 1, dtype=np.float64)), M.vec()
        check(L.cgx_cg_set_mode(cg, 3))
        return solve(M, cg, b, x, 0.0, 8, 1)[:2]

    # (a) a zero diagonal in a row the last rank owns
    bad_row = n - 3
    va = vl.copy()
    k = rp[bad_row] + int(np.nonzero(cl[rp[bad_row]:rp[bad_row + 1]] == bad_row)[0][0])
    va[k] = 0.0
    M = Ranked(q, rp, cl, va)
    if rank == world - 1:
        assert M.begin <= bad_row < M.begin + M.nl
    d = cga.DeviceArray(q, M.nl + 1, np.float64)
    rc = L.cgx_csr_diag_inv(M.A, d.ptr)
    out["bad_row"] = bad_row
    out["diag_inv"] = everyone((rc, L.cgx_last_error().decode()))
    cg = C.c_void_p()
    check(L.cgx_cg_create(q.handle, M.A, C.byref(cg)))
    rc = L.cgx_cg_set_precond(cg, JACOBI, None)
    msg = L.cgx_last_error().decode()
    kind = C.c_int(-1)
    check(L.cgx_cg_get_precond(cg, C.byref(kind)))
    out["jacobi"] = everyone((rc, msg, kind.value))
    out["plain_after_jacobi"] = everyone(plain_solve(M, cg))
    L.cgx_cg_destroy(cg)
    M.destroy()
    # (b) one non-positive entry in the last rank's d_minv
    M = Ranked(q, rp, cl, vl)
    bad_entry = n - 5
    mv = np.ones(n)
    mv[bad_entry] = -1.0
    md = M.vec(mv)
    cg = C.c_void_p()
    check(L.cgx_cg_create(q.handle, M.A, C.byref(cg)))
    rc = L.cgx_cg_set_precond(cg, DIAGONAL, md.ptr)
    msg = L.cgx_last_error().decode()
    check(L.cgx_cg_get_precond(cg, C.byref(kind)))
    out["bad_entry"] = bad_entry
    out["diagonal"] = everyone((rc, msg, kind.value))
    out["plain_after_diagonal"] = everyone(plain_solve(M, cg))
    # ... and the good diagonal is still taken on the same handles
    good = M.vec(np.ones(n))  # caller-owned: alive until the solver lets go of it
    rc = L.cgx_cg_set_precond(cg, DIAGONAL, good.ptr)
    check(L.cgx_cg_get_precond(cg, C.byref(kind)))
    out["good_after"] = everyone((rc, kind.value))
    check(L.cgx_cg_set_precond(cg, NONE, None))
    L.cgx_cg_destroy(cg)
    M.destroy()
    return None if rank else out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["p2d", "irr", "p3d", "poisson"], default="p3d")
    ap.add_argument("--transport", choices=["rccl", "host", "host-async", "host-peer", "rccl-peer"],
                    default="host")
    ap.add_argument("--mode", default="3",
                    help="default mode of a step; a comma list gives rank r the r-th entry")
    ap.add_argument("--runs", type=int, default=1, help="default cgx_cg_run calls of a step")
    ap.add_argument("--steps", default="jacobi",
                    help="comma list of kind[@mode[@bodies[@runs]]], see the module docstring")
    a = ap.parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist.init_process_group("gloo")
    L = lib()
    q = cga.Queue(local % max(1, cga.device_count()))
    if a.transport.startswith("host"):
        from conjugategradient_amd.hostcomm import HostTransport
        transport = HostTransport()
        transport.attach(q, overlap=a.transport == "host-async")
    else:
        uid = C.create_string_buffer(128)
        if rank == 0:
            check(L.cgx_nccl_unique_id(uid, 128))
        obj = [bytes(uid.raw) if rank == 0 else None]
        dist.broadcast_object_list(obj, src=0)
        check(L.cgx_dist_init(q.handle, rank, world, obj[0], 128))
    gc = global_case(a.case)
    mats = {}

    def matrix(dtype):
        if dtype not in mats:
            M = Ranked(q, gc[0], gc[1], gc[2], dtype)
            peer = C.c_int(0)
            if a.transport.endswith("-peer"):
                check(L.cgx_dist_peer_enable(M.A, C.byref(peer)))
                if not peer.value:
                    raise SystemExit(f"rank {rank}: peer transport unavailable: "
                                     f"{L.cgx_last_error().decode()}")
            mats[dtype] = M
        return mats[dtype]

    M = matrix(np.float64)
    coloc, onew, var, peer = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    check(L.cgx_dist_peer_info(M.A, C.byref(peer)))
    if peer.value:
        check(L.cgx_dist_peer_form(M.A, C.byref(coloc), C.byref(onew)))
    check(L.cgx_csr_variant(M.A, C.byref(var)))
    forms = everyone((int(peer.value), [int(coloc.value), int(onew.value)], int(var.value)))
    results = []
    for step in a.steps.split(","):
        f = step.split("@")
        kind = f[0]
        modes = [int(m) for m in (f[1].split("+") if len(f) > 1 and f[1] else a.mode.split(","))]
        bodies = int(f[2]) if len(f) > 2 and f[2] else -1
        runs = int(f[3]) if len(f) > 3 and f[3] else a.runs
        if kind == "errors":
            results.append(errors_step(q))
        elif kind == "mode4":
            results.append(mode4_step(M))
        else:
            Mk = matrix(np.float32 if kind == "f32jac" else np.float64)
            results.append(run_step(Mk, a.case, gc, kind, modes, bodies, runs))
    if rank == 0:
        print(json.dumps({"world": world, "transport": a.transport, "case": a.case, "n": M.n,
                          "peer": [f[0] for f in forms], "peer_form": [f[1] for f in forms],
                          "variant": [f[2] for f in forms], "steps": results}), flush=True)
    for Mk in mats.values():
        Mk.destroy()
    q.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
