"""Diagonal preconditioning on partitioned matrices, the parts that need no
device (DESIGN.md §5b "partitioned"): the row partition's local numbering
that k_diag_inv relies on, and the partitioned PCG loop itself in numpy.

The partition is libcgx's own: cgx_plan_ghosts / cgx_plan_remap, as
cgx_csr_create_dist and tests/dist_emul.py call them. After the remap a
rank's columns are local: own rows first (global - row_begin), then the
ghosts, so the diagonal entry of local row i is the one with col == i.

The ranks run in this one process (the halo is a gather from the global
vector, an all-reduce a sum of the ranks' np.dot values in rank order): the
partitioned loop of cgx_abi.cpp, per rank z = m o r never stored beyond the
body, r.r and r.z all-reduced together, the stop rule on the true r.r."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd._native import lib
from tests.dist_emul import partition
from tests.test_pcg_cpu import case, diag_of, pcg, rows_of
from tests.util import rel


def plan(rank, world, rp, cl):
    """Rank's local rowptr, remapped columns, ghost ids (global), row range."""
    L = lib()
    n = len(rp) - 1
    begins, counts = partition(n, world)
    a, b = int(begins[rank]), int(begins[rank] + counts[rank])
    lrp = (rp[a:b + 1] - rp[a]).astype(np.int32)
    lcol = cl[rp[a]:rp[b]].astype(np.int32).copy()
    ng = C.c_int64()
    gp = C.POINTER(C.c_int64)()
    recv = np.zeros(world, np.int64)
    assert L.cgx_plan_ghosts(counts[rank], a, len(lcol), lcol.ctypes.data, world,
                             begins.ctypes.data, counts.ctypes.data, C.byref(ng), C.byref(gp),
                             recv.ctypes.data) == 0
    ghosts = np.ctypeslib.as_array(gp, shape=(max(ng.value, 1),))[:ng.value].copy()
    assert L.cgx_plan_remap(counts[rank], a, len(lcol), lcol.ctypes.data, ng.value, gp) == 0
    L.cgx_free_host(C.cast(gp, C.c_void_p))
    return dict(a=a, b=b, rowptr=lrp, col=lcol, ghosts=ghosts)


def partitioned_pcg(rp, cl, vl, b, m, world, bodies):
    """x, r.r, r.z after `bodies` bodies at tol 0 over a `world`-way partition."""
    n = len(b)
    ranks = [plan(r, world, rp, cl) for r in range(world)]
    for k in ranks:
        k["val"] = vl[rp[k["a"]]:rp[k["b"]]]
        k["rows"] = rows_of(k["rowptr"])
        k["m"] = m[k["a"]:k["b"]]

    def spmv(k, v_glob):
        nl = k["b"] - k["a"]
        ext = np.concatenate([v_glob[k["a"]:k["b"]], v_glob[k["ghosts"]]])  # the halo
        y = np.zeros(nl)
        np.add.at(y, k["rows"], k["val"] * ext[k["col"]])
        return y

    def allreduce(parts):  # rank order
        s = 0.0
        for v in parts:
            s += v
        return s

    sl = [slice(k["a"], k["b"]) for k in ranks]
    x = np.zeros(n)
    r = np.concatenate([b[s] - spmv(k, x) for k, s in zip(ranks, sl)])
    p = np.concatenate([k["m"] * r[s] for k, s in zip(ranks, sl)])
    rxr = allreduce(float(np.dot(r[s], r[s])) for s in sl)
    rz = allreduce(float(np.dot(r[s], k["m"] * r[s])) for k, s in zip(ranks, sl))
    for _ in range(bodies):
        Ap = np.concatenate([spmv(k, p) for k in ranks])
        alpha = rz / allreduce(float(np.dot(p[s], Ap[s])) for s in sl)
        r = r - alpha * Ap
        z = np.concatenate([k["m"] * r[s] for k, s in zip(ranks, sl)])
        rr_new = allreduce(float(np.dot(r[s], r[s])) for s in sl)  # the two values of
        rz_new = allreduce(float(np.dot(r[s], z[s])) for s in sl)  # the one all-reduce
        x = x + alpha * p
        p = z + (rz_new / rz) * p
        assert not (math.isnan(rxr) or math.sqrt(rxr) <= 0.0)  # tol 0: the cap stops it
        rxr, rz = rr_new, rz_new
    return x, rxr, rz


@pytest.mark.parametrize("world", [2, 3])
def test_local_diagonal_is_col_equal_local_row(world):
    """After cgx_plan_remap the entries with col == local row are exactly the
    global diagonal's, for every case's partition: what k_diag_inv sums."""
    for name in ("p2d", "irr", "p3d"):
        rp, cl, vl, _ = case(name)
        want = diag_of(rp, cl, vl)
        got = []
        for rank in range(world):
            k = plan(rank, world, rp, cl)
            nl = k["b"] - k["a"]
            rows = rows_of(k["rowptr"])
            on = rows == k["col"]
            # own columns map to [0, nl), ghosts behind them
            glob = cl[rp[k["a"]]:rp[k["b"]]]
            own = (glob >= k["a"]) & (glob < k["b"])
            np.testing.assert_array_equal(k["col"][own], glob[own] - k["a"])
            assert (k["col"][~own] >= nl).all()
            np.testing.assert_array_equal(k["ghosts"][k["col"][~own] - nl], glob[~own])
            d = np.zeros(nl)
            np.add.at(d, rows[on], vl[rp[k["a"]]:rp[k["b"]]][on])
            got.append(d)
        np.testing.assert_array_equal(np.concatenate(got), want)


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_pcg_equals_the_single_process_checker(world):
    rp, cl, vl, b = case("p2d")
    m = 1.0 / diag_of(rp, cl, vl)
    xr, kr, rr, rzr = pcg(rp, cl, vl, b, m, 0.0, False, 30)
    x, rxr, rz = partitioned_pcg(rp, cl, vl, b, m, world, 30)
    d = rel(x, xr)
    print(f"p2d over {world} ranks, 30 bodies: rel {d:.3e}, r.r {rxr:.17g} / {rr:.17g}, "
          f"r.z {rz:.17g} / {rzr:.17g}")
    assert kr == 30
    assert d <= 1e-14
