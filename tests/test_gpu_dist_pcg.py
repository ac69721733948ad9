"""Diagonal preconditioning on partitioned matrices (DESIGN.md §5b
"partitioned"): cgx_csr_diag_inv and cgx_cg_set_precond on cgx_csr_create_dist
matrices, modes 1 and 3, over the host-staged transport (synchronous and
asynchronous), RCCL (world size 1 on this box) and the device peer transport
in both iteration forms. Every launch is a tests/dist_pcg_check.py job under
torch.distributed.run with all ranks on this one GPU; one launch runs several
steps and is shared by the tests that read it.

The bounds are the single-device ones of tests/test_gpu_pcg.py: x within
1e-13 of the checker after 30 bodies (the per-rank rounded sums of the host
and RCCL paths are no worse than the checker's np.dot variant, which
tests/test_pcg_cpu.py holds to 1e-13 of the exact one), r.r and r.z within
1e-9, and bit-identity wherever the sums are the same sums: mode 3 against
mode 1, the peer transport against any split and against one device (every
dot a double-length sum rounded once), both peer forms, m == 1 against the
plain partitioned solver."""
import functools
import hashlib
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import conjugategradient_amd as cga
from tests.test_pcg_cpu import CASES, case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAN = (("CGX_SPMV_VARIANT", "33554432:0"),)
FUSED = (("CGX_PEER_ONE_WAITER", "0"),)
EINVAL, EUNSUPPORTED = 1, 6
J30 = "jacobi@1@30,jacobi@3@30"


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@functools.lru_cache(maxsize=None)
def _launch(nproc, transport, name, steps, env=()):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(_port()),
           os.path.join(ROOT, "tests", "dist_pcg_check.py"), "--case", name,
           "--transport", transport, "--steps", steps]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env={**os.environ, **dict(env)})
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert r["world"] == nproc
    assert r["peer"] == [int(transport.endswith("-peer"))] * nproc
    for s in r["steps"]:
        if "ranks_agree" in s:  # the readers report the world values on every rank
            assert s["ranks_agree"] and s["finite"], s
    return r


def _bits(s):
    return s["x_sha"], s["bodies"], s["rxr"], s["rz"]


# the launches several tests share
def _p3d_peer(nproc):
    steps = J30 + ",jacobi@1+3@30,diagjac@3@30" if nproc == 2 else J30
    return _launch(nproc, "host-peer", "p3d", steps)


# 1 -------------------------------------------------------------------------
@pytest.mark.parametrize("nproc,transport,name", [(2, "host", "p3d"), (3, "host-peer", "p3d"),
                                                  (8, "host-peer", "p3d"), (1, "rccl", "p3d"),
                                                  (2, "host-async", "p2d")])
def test_jacobi_30_bodies_against_checker(nproc, transport, name):
    r = _p3d_peer(nproc) if transport == "host-peer" else _launch(nproc, transport, name, J30)
    one, three = r["steps"][:2]
    for s, mode in ((one, 1), (three, 3)):
        print(f"{name} x{nproc} {transport} mode {mode}: rel {s['rel']:.3e}, r.r {s['rxr']:.17g} "
              f"(checker {s['ref_rxr']:.17g}), r.z {s['rz']:.17g} (checker {s['ref_rz']:.17g})")
        assert s["modes_run"] == [mode] * nproc
        assert s["bodies"] == s["ref_bodies"] == 30
        assert s["rel"] <= 1e-13
        assert s["rxr"] == pytest.approx(s["ref_rxr"], rel=1e-9)
        assert s["rz"] == pytest.approx(s["ref_rz"], rel=1e-9)
    assert _bits(three) == _bits(one)


# 2 -------------------------------------------------------------------------
def test_peer_transport_independent_of_the_split(queue):
    """x, r.r and r.z after 30 Jacobi bodies: the same bits on 2, 3 and 8 ranks
    and on one device (the plain solver's property, extended to r.z)."""
    rp, cl, vl, b = case("p3d")
    cg = cga.CG(queue)
    cg.mode = 3
    cg.setMatrix(cga.Matrix(queue, vl, cl, rp))
    cg.setTarget(b)
    cg.setPreconditioner(cga.Preconditioner.Jacobi)
    cg.setInital(np.zeros(len(b)))
    cg.solve(0.0, max_iter=30)
    single = (hashlib.sha256(cg.extract().tobytes()).hexdigest()[:16], cg.iterations,
              cg.final_rxr, cg.final_rz)
    got = {n: _bits(_p3d_peer(n)["steps"][1]) for n in (2, 3, 8)}
    print("single", single, got)
    assert single[1] == 30
    for n, bits in got.items():
        assert bits == single, (n, bits, single)


# 3 -------------------------------------------------------------------------
@pytest.mark.parametrize("nproc", [2, 8])
def test_both_peer_forms(nproc):
    ro = _p3d_peer(nproc)
    rf = _launch(nproc, "host-peer", "p3d", "jacobi@3@30", FUSED)
    assert ro["peer_form"] == [[nproc, 1]] * nproc, ro["peer_form"]
    assert rf["peer_form"] == [[nproc, 0]] * nproc, rf["peer_form"]
    assert rf["steps"][0]["bodies"] == 30
    assert _bits(rf["steps"][0]) == _bits(ro["steps"][1])


def test_fused_peer_form_with_odd_local_rows():
    """p2d (33 x 31 = 1,023 rows) on 3 ranks: 341 rows each, so the vector
    kernels' odd-n tail runs in the peer transport's fused form in modes 1 and
    3 (p3d splits into even blocks on 2, 3 and 8 ranks; the ring form has odd
    blocks in test_jacobi_30_bodies_against_checker's p2d x 2, 512 + 511, and
    in test_to_tolerance_where_plain_cg_hits_the_cap). The checker and bounds
    of test_jacobi_30_bodies_against_checker."""
    r = _launch(3, "host-peer", "p2d", J30, FUSED)
    assert r["peer_form"] == [[3, 0]] * 3, r["peer_form"]
    one, three = r["steps"][:2]
    for s, mode in ((one, 1), (three, 3)):
        print(f"p2d x3 fused peer mode {mode}: rel {s['rel']:.3e}, r.r {s['rxr']:.17g} "
              f"(checker {s['ref_rxr']:.17g}), r.z {s['rz']:.17g} (checker {s['ref_rz']:.17g})")
        assert s["modes_run"] == [mode] * 3
        assert s["bodies"] == s["ref_bodies"] == 30
        assert s["rel"] <= 1e-13
        assert s["rxr"] == pytest.approx(s["ref_rxr"], rel=1e-9)
        assert s["rz"] == pytest.approx(s["ref_rz"], rel=1e-9)
    assert _bits(three) == _bits(one)


# 4, 5 ----------------------------------------------------------------------
ID45 = "plain@1@45,ones@1@45,plain@3@45,ones@3@45"


def _lean_launch():
    return _launch(2, "host-peer", "poisson", ID45 + ",diag@3@30,mode4", LEAN)


@pytest.mark.parametrize("where", ["poisson-lean-peer", "p3d-host"])
def test_unit_diagonal_is_the_plain_partitioned_solver(where):
    r = _lean_launch() if where == "poisson-lean-peer" else _launch(3, "host", "p3d", ID45)
    if where == "poisson-lean-peer":
        assert all(v & 33554432 for v in r["variant"]), r["variant"]
    for plain, ones in (r["steps"][0:2], r["steps"][2:4]):
        assert plain["kind"] == "plain" and ones["kind"] == "ones"
        assert plain["modes_run"] == ones["modes_run"]
        assert plain["bodies"] == ones["bodies"] == 45
        assert ones["x_sha"] == plain["x_sha"]
        assert ones["rxr"] == plain["rxr"] and ones["rz"] == ones["rxr"]
    assert r["steps"][2]["x_sha"] == r["steps"][0]["x_sha"]


def test_real_diagonal_behind_the_lean_interior():
    r = _lean_launch()
    s = r["steps"][4]
    assert all(v & 33554432 for v in r["variant"]), r["variant"]
    print(f"poisson 128x128x48, m = 10^U(-1,1): rel {s['rel']:.3e}, r.z {s['rz']:.17g} "
          f"(checker {s['ref_rz']:.17g})")
    assert s["kind"] == "diag" and s["bodies"] == s["ref_bodies"] == 30
    assert s["rel"] <= 1e-13


def test_callers_diagonal_gives_jacobis_bits():
    r = _p3d_peer(2)
    assert r["steps"][3]["kind"] == "diagjac"
    assert _bits(r["steps"][3]) == _bits(r["steps"][1])


# 6 -------------------------------------------------------------------------
@pytest.mark.parametrize("name,nproc", [("p2d", 2), ("irr", 3)])
def test_to_tolerance_where_plain_cg_hits_the_cap(name, nproc):
    r = _launch(nproc, "host-peer", name, "jacobi@0@-1,jacobi@0@-1@3,plain@0@-1")
    jac, split, plain = r["steps"]
    n = r["n"]
    print(f"{name} x{nproc}: Jacobi {jac['bodies']} bodies (checker {jac['ref_bodies']}), rel "
          f"{jac['rel']:.3e}, residual {jac['residual']:.3e}; plain {plain['bodies']} bodies, "
          f"residual {plain['residual']:.3e}")
    assert jac["modes_run"] == [3] * nproc  # auto with a preconditioner
    assert jac["ref_bodies"] == CASES[name]
    assert abs(jac["bodies"] - CASES[name]) <= 2
    assert jac["stopped"] == 1
    assert jac["rel"] <= 1e-10
    assert jac["residual"] <= 2e-8
    # split into three runs: the deferred-x flush at every run's end
    assert split["runs"] == 3 and _bits(split) == _bits(jac)
    # the same ranks without the preconditioner: the cap, far from solved
    assert plain["bodies"] == n + 1 and plain["stopped"] == 2
    assert plain["residual"] > 1e-4


# 7 -------------------------------------------------------------------------
def test_mixed_modes():
    r = _p3d_peer(2)
    mixed, three = r["steps"][2], r["steps"][1]
    assert mixed["modes_run"] == [1, 3] and three["modes_run"] == [3, 3]
    assert _bits(mixed) == _bits(three)


# 8 -------------------------------------------------------------------------
def _host_p2d():
    return _launch(2, "host", "p2d", "f32jac@3@-1,errors")


def test_collective_errors():
    e = _host_p2d()["steps"][1]
    row, entry = e["bad_row"], e["bad_entry"]
    codes = [rc for rc, _ in e["diag_inv"]]
    msgs = [m for _, m in e["diag_inv"]]
    assert codes == [EINVAL, EINVAL], e["diag_inv"]
    assert msgs[0] == msgs[1] and f"row {row}" in msgs[0] and "1 row" in msgs[0], msgs
    for rc, msg, kind in e["jacobi"]:
        assert rc == EINVAL and f"row {row}" in msg and kind == 0, e["jacobi"]
    assert e["jacobi"][0][1] == e["jacobi"][1][1]
    assert e["plain_after_jacobi"] == [[8, 2], [8, 2]], e["plain_after_jacobi"]
    for rc, msg, kind in e["diagonal"]:
        assert rc == EINVAL and f"entry {entry}" in msg and kind == 0, e["diagonal"]
    assert e["diagonal"][0][1] == e["diagonal"][1][1]
    assert e["plain_after_diagonal"] == [[8, 2], [8, 2]], e["plain_after_diagonal"]
    assert e["good_after"] == [[0, 2], [0, 2]], e["good_after"]


def test_mode4_refuses_a_preconditioner_on_a_partitioned_matrix():
    m = _lean_launch()["steps"][5]
    assert m["set_mode4"] == 0  # the mode itself runs on this matrix
    for rc, msg, kind in m["mode_then_precond"]:
        assert rc == EUNSUPPORTED and "modes 1 and 3" in msg and kind == 0, m
        assert "single device" not in msg
    for rc, msg, auto, mode in m["precond_then_mode"]:
        assert rc == EUNSUPPORTED and "modes 1 and 3" in msg and auto == mode == 3, m


# 9 -------------------------------------------------------------------------
def test_f32_jacobi():
    s = _host_p2d()["steps"][0]
    print(f"f32 x2 host: Jacobi {s['bodies']} bodies, f64 residual {s['residual']:.3e}")
    assert s["modes_run"] == [3, 3]
    assert s["stopped"] == 1 and s["bodies"] < 200
    assert s["residual"] <= 3e-3
