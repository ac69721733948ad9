"""Block-Jacobi preconditioning of the many-systems solve
(cgx_many_set_block_precond), the parts that need no device:
the entry points are declared, exported and bound, the C ABI and the Python
class refuse bad arguments before they touch a device, the C++ example
compiles, every system the GPU tests compare bit for bit
(tests/many_block_systems.py) has, in the numpy restatement of the loop
(tests/bj_model.cg), no dot closer than its guard to a rounding boundary, and
the convergence record: block bodies are fewer than Jacobi bodies.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd import _native
from conjugategradient_amd.workloads import node_mixed
from tests import bj_model, cg_model
from tests import many_block_systems as S
from tests import many_pcg_systems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
NEW_SYMBOLS = ["cgx_many_set_block_precond", "cgx_many_get_block_precond", "cgx_many_block_inv",
               "cgx_many_block_bad"]

# bodies over a set's systems, (JACOBI, GIVEN): the model's, recorded
BODIES = {
    "n257b3": ((39, 47), (44, 57)), "n396b3": ((40, 49), (47, 60)),
    "n1023b7": ((49, 66), (57, 79)), "n4096b8": ((12, 12), (12, 12)),
    "n4096b5": ((12, 12), (12, 12)), "n60b3": ((16, 17), (19, 21)),
    "n65b3": ((20, 23), (25, 28)), "n255b8": ((26, 31), (29, 36)),
    "n256b8": ((21, 24), (24, 29)), "n1b3": ((2, 2), (2, 2)), "n2b3": ((2, 2), (2, 2)),
    "n7b8": ((2, 2), (2, 2)), "multi11": ((16, 17), (18, 21)), "n396b3x0": ((5, 5), (5, 5)),
}


def test_new_symbols_exported_and_bound():
    syms = cga.header_symbols()
    L = cga.lib()
    for s in NEW_SYMBOLS:
        assert s in syms, f"{s} not declared in include/cgx.h"
        assert hasattr(L, s), f"{s} not exported by libcgx.so"
        assert s in _native._SIGS, f"{s} has no ctypes signature"
    assert hasattr(cga.ManyCG, "set_block_preconditioner") and hasattr(cga.ManyCG, "block_inv")
    header = open(os.path.join(ROOT, "include", "CGMany.hpp")).read()
    for name in ("setBlockPreconditioner", "blockPreconditioner", "blockInverse"):
        assert name in header


def _err():
    return cga.lib().cgx_last_error().decode()


def test_set_block_precond_refusals_need_no_device():
    """The handle is NULL or made up: a refusal must come before anything
    reads it. (ldw < n bs needs a real object: tests/test_gpu_many_block_pcg.py.)"""
    L = cga.lib()
    fake = 0x5000  # never dereferenced: every call below is refused first
    for kind in (-1, 3, 17):
        assert L.cgx_many_set_block_precond(fake, kind, 3, 0x1000, 100) == EINVAL
        assert f"unknown kind {kind}" in _err()
    for kind in (S.JACOBI, S.GIVEN):
        for bs in (0, 9, -2):
            assert L.cgx_many_set_block_precond(fake, kind, bs, 0x1000, 100) == EINVAL
            assert "outside 1..8" in _err()
    assert L.cgx_many_set_block_precond(fake, S.GIVEN, 3, None, 100) == EINVAL
    assert "NULL" in _err() and "d_W" in _err()
    assert L.cgx_many_set_block_precond(fake, S.GIVEN, 3, 0x1004, 100) == EINVAL
    assert "8-byte aligned" in _err()
    for kind, bs, w in ((S.NONE, 0, None), (S.JACOBI, 3, None), (S.GIVEN, 3, 0x1000)):
        assert L.cgx_many_set_block_precond(None, kind, bs, w, 100) == EINVAL
        assert "NULL handle" in _err()


def test_get_block_precond_and_block_inv_refuse_before_any_device_call():
    L = cga.lib()
    kind, bs = C.c_int(7), C.c_int(7)
    assert L.cgx_many_get_block_precond(None, C.byref(kind), C.byref(bs)) == EINVAL
    assert (kind.value, bs.value) == (7, 7)
    fake = 0x5000
    for b in (0, 9):
        assert L.cgx_many_block_inv(fake, b, 0x1000, 100, None, None) == EINVAL
        assert "outside 1..8" in _err()
    assert L.cgx_many_block_inv(fake, 3, None, 100, None, None) == EINVAL
    assert L.cgx_many_block_inv(fake, 3, 0x1004, 100, None, None) == EINVAL
    assert L.cgx_many_block_inv(None, 3, 0x1000, 100, None, None) == EINVAL
    assert "NULL handle" in _err()
    assert L.cgx_many_block_bad(None, (C.c_int * 3)()) == EINVAL
    assert L.cgx_many_block_bad(fake, None) == EINVAL


def test_python_class_refuses_before_any_device_call():
    m = object.__new__(cga.ManyCG)
    m.nsys, m.n, m.nnz, m._h = 3, 12, 40, None  # no queue, no handle: a device call would raise
    B = cga.BlockPreconditioner
    with pytest.raises(ValueError, match="unknown block preconditioner kind"):
        m.set_block_preconditioner(5, 3)
    with pytest.raises(ValueError, match="block_size"):
        m.set_block_preconditioner(B.Jacobi, 9)
    with pytest.raises(ValueError, match="block_size"):
        m.set_block_preconditioner(B.Given, 0, np.ones((3, 12, 3)))
    with pytest.raises(ValueError, match="needs blocks"):
        m.set_block_preconditioner(B.Given, 3)
    with pytest.raises(ValueError, match="blocks has shape"):
        m.set_block_preconditioner(B.Given, 3, np.ones((3, 12, 2)))
    with pytest.raises(ValueError, match="blocks has shape"):
        m.set_block_preconditioner(B.Given, 3, np.ones((12, 3)))
    with pytest.raises(ValueError, match="block_size"):
        m.block_inv(0)


def test_many_block_pcg_check_compiles(tmp_path):
    out = str(tmp_path / "many_block_pcg_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                        "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "many_block_pcg_check.cpp"), "-o", out,
                        "-L" + os.path.join(ROOT, "conjugategradient_amd"), "-lcgx",
                        "-Wl,-rpath," + os.path.join(ROOT, "conjugategradient_amd")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "many_block_pcg_check" in open(os.path.join(ROOT, "examples", "Makefile")).read()


def test_cut_is_a_leading_principal_submatrix():
    rp, cl, vl = node_mixed(3, 2, 3, S.E, 7)
    n = 14
    rp2, cl2, vl2 = S.cut(rp, cl, vl, n)
    full = np.zeros((18, 18))
    full[np.repeat(np.arange(18), np.diff(rp)), cl] = vl
    part = np.zeros((n, n))
    part[np.repeat(np.arange(n), np.diff(rp2)), cl2] = vl2
    np.testing.assert_array_equal(part, full[:n, :n])
    assert (part == part.T).all() and np.linalg.eigvalsh(part).min() > 0


def test_small_seeds_are_the_first_clear_ones():
    """The search many_block_systems.SEEDS records, run again for n = 1, 2 and 7."""
    for name in ("n1b3", "n2b3", "n7b8"):
        assert S.SEEDS[name] == S.search(name), name


@pytest.mark.parametrize("kind", list(S.KINDS))
@pytest.mark.parametrize("name", S.ALL_SETS)
def test_committed_systems_have_no_unclear_dot(name, kind):
    rp, cl, vals, B, tol, X0, max_bodies, bs = S.system_set(name)
    n = len(rp) - 1
    assert n == S.SETS[name][3] and bs == S.SETS[name][2] and len(vals) == S.SETS[name][4]
    W = S.precond(name, S.KINDS[kind])
    assert W.shape == (len(vals), n, bs) and np.isfinite(W).all()
    if n % bs:  # the columns past the partial last block are +0.0
        pad = W[:, n // bs * bs:, n % bs:]
        assert not pad.any() and not np.signbit(pad).any()
    bodies, nan_x = [], []
    for s, run in enumerate(S.model_runs(name, kind)):
        assert not run.unclear, f"{name}[{s}] {kind}: {len(run.unclear)} dots are not clear"
        assert len(run.rz) == run.bodies
        if np.isnan(run.x).any():
            nan_x.append(s)
        began = ([run.rr0] + run.rr)[-2]  # the r.r the last body began with
        by_rule = bool(np.isnan(began)) or bool(np.sqrt(began) <= tol)
        if max_bodies >= 0:
            assert run.bodies == max_bodies and not by_rule, f"{name}[{s}]: not ended by the cap"
        else:
            assert by_rule, f"{name}[{s}] {kind}: not ended by the stop rule"
            assert run.bodies < n + 1 or n <= 2, f"{name}[{s}]: {run.bodies} bodies, the cap"
        bodies.append(run.bodies)
    assert tuple(nan_x) == S.NAN_X.get((name, kind), ()), (name, kind, nan_x)
    k = 0 if kind == "jacobi" else 1
    assert (min(bodies), max(bodies)) == BODIES[name][k], bodies


def _jacobi_bodies(rp, cl, vl, b, tol):
    d = P.diagonal_of(rp, cl, vl)[0]
    return cg_model.cg(rp, cl, vl, b, tol, -1, minv=1.0 / d, dtype=np.float64).bodies


def test_convergence_record():
    """By the model: on the 396-row node_mixed(12, 11, 3, 1.5, 7) plain CG ends
    at its cap, Jacobi takes 308 bodies and block-Jacobi 49; on the 60-row set
    every system takes fewer block bodies than Jacobi bodies."""
    rp, cl, vl = node_mixed(12, 11, 3, S.E, 7)
    n = len(rp) - 1
    b = np.arange(1, n + 1, dtype=np.float64)
    b /= np.linalg.norm(b)
    plain = cg_model.cg(rp, cl, vl, b, 1e-8, -1, dtype=np.float64).bodies
    jac = _jacobi_bodies(rp, cl, vl, b, 1e-8)
    blk = bj_model.cg(rp, cl, vl, b, 1e-8, -1, bj_model.csr_block_inverse(rp, cl, vl, 3)[0]).bodies
    assert (plain, jac, blk) == (397, 308, 49)
    rp, cl, vals, B, tol, _, _, bs = S.system_set("n60b3")
    for s, run in enumerate(S.model_runs("n60b3", "jacobi")):
        assert run.bodies < _jacobi_bodies(rp, cl, vals[s], B[s], tol), s
