"""The preconditioner extension of the C++ drop-in (include/CG.hpp:
CGSolver::Preconditioner, CG::setPreconditioner), driven from C++ by
examples/pcg_check.cpp: the scaled 1,023-row matrix solved to 1e-8 ||b|| with
Jacobi and with the same diagonal moved in as a Vector, held to the numpy
checker of tests/test_pcg_cpu.py as tests/test_gpu_pcg.py holds the Python
mirror."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_pcg_cpu import CASES, case, diag_of, jacobi_ref, residual
from tests.util import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "examples", "pcg_check")


@pytest.mark.gpu
def test_cpp_preconditioners_against_checker(tmp_path):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples")], check=True)
    rp, cl, vl, b = case("p2d")
    n = len(b)
    tol = 1e-8 * float(np.linalg.norm(b))
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        np.array([n, len(vl)], np.int64).tofile(f)
        rp.astype(np.int32).tofile(f)
        cl.astype(np.int32).tofile(f)
        vl.astype(np.float64).tofile(f)
        b.tofile(f)
        (1.0 / diag_of(rp, cl, vl)).tofile(f)
        np.array([tol], np.float64).tofile(f)
    p = subprocess.run([EXE, str(inp), str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = np.fromfile(out, np.float64)
    assert res.size == 2 * (2 + n)
    xr, kr, _, _ = jacobi_ref("p2d", 1e-8, -1)
    assert kr == CASES["p2d"]
    runs = res.reshape(2, 2 + n)
    for name, run in zip(("Jacobi", "Diagonal"), runs):
        k, rxr, x = int(run[0]), run[1], run[2:]
        print(f"{name}: {k} bodies (checker {kr}), rel {rel(x, xr):.3e}, "
              f"residual {residual('p2d', x):.3e}, r.r {rxr:.3e}")
        assert abs(k - kr) <= 2
        assert rel(x, xr) <= 1e-10
        assert residual("p2d", x) <= 2e-8
    # the moved-in 1 / diag(A) is Jacobi's m: the same bits
    np.testing.assert_array_equal(runs[1], runs[0])
