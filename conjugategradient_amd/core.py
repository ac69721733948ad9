"""Python mirror of the reference's C++ API, on top of libcgx.so.

Same class and method names, argument meaning and error behaviour as
/root/reference/src (cited per method), so parity tests read like the
reference's own driver (test/Tester.cpp). The C++ drop-in for the same API is
include/CG.hpp, include/VectorOperations.hpp, include/LinearAlgebraTypes.hpp.

Everything here is a thin wrapper: every computation runs in libcgx.so's HIP
kernels on a gfx950 device; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import enum

import numpy as np

from . import _native as N
from ._native import CgxError, check, lib

_vp = C.c_void_p


class Debuglevel(enum.IntEnum):
    """LinearAlgebraTypes.hpp:26-30"""
    None_ = 0
    Verbose = 1


class Preconditioner(enum.IntEnum):
    """Extension (cgx.h CGX_PRECOND_*): diagonal preconditioning of CG.solve."""
    None_ = 0
    Jacobi = 1     # 1 / diag(A), built on the device
    Diagonal = 2   # a positive vector the caller supplies


class BlockPreconditioner(enum.IntEnum):
    """Extension (cgx.h CGX_BLOCK_*): block-Jacobi preconditioning of CG.solve
    with dense diagonal blocks of 1 to 8 rows."""
    None_ = 0
    Jacobi = 1     # the inverses of A's diagonal blocks, built on the device
    Given = 2      # an (n, block_size) array of blocks the caller supplies


MAX_BLOCK_SIZE = 8


def _dtype_code(dtype) -> int:
    dt = np.dtype(dtype)
    if dt == np.float64:
        return N.F64
    if dt == np.float32:
        return N.F32
    raise TypeError(f"unsupported dtype {dt} (float64 or float32)")


class Queue:
    """The sycl::queue of the reference (CG.hpp:61,70-77): one device, one
    in-order HIP stream. ``wait()`` is ``executeQueue`` (CG.hpp:561-578)."""

    def __init__(self, device: int = 0):
        h = _vp()
        check(lib().cgx_create(device, C.byref(h)))
        self._h = h
        self.device = device

    @property
    def handle(self):
        return self._h

    def wait(self) -> None:
        check(lib().cgx_sync(self._h))

    wait_and_throw = wait

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().cgx_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass


class DeviceArray:
    """A device allocation released when the last reference goes away (the
    shared_ptr + Asycl_deleter of LinearAlgebraTypes.hpp:43-49)."""

    def __init__(self, queue: Queue, n: int, dtype=np.float64):
        self.queue = queue
        self.n = int(n)
        self.dtype = np.dtype(dtype)
        p = _vp()
        check(lib().cgx_alloc(queue.handle, max(self.n, 1) * self.dtype.itemsize, C.byref(p)))
        self.ptr = p.value

    @property
    def nbytes(self) -> int:
        return self.n * self.dtype.itemsize

    def upload(self, host) -> "DeviceArray":
        a = np.ascontiguousarray(host, dtype=self.dtype)
        if a.size != self.n:
            raise ValueError(f"size {a.size} != {self.n}")
        check(lib().cgx_h2d(self.queue.handle, self.ptr, a.ctypes.data, a.nbytes))
        return self

    def download(self) -> np.ndarray:
        out = np.empty(self.n, self.dtype)
        check(lib().cgx_d2h(self.queue.handle, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def fill(self, value: float) -> None:
        check(lib().cgx_fill(self.queue.handle, _dtype_code(self.dtype), self.ptr,
                             float(value), self.n))

    def __del__(self):  # pragma: no cover
        try:
            if self.ptr and self.queue.handle:
                lib().cgx_free(self.queue.handle, self.ptr)
        except Exception:
            pass
        self.ptr = None


class Matrix:
    """CSR matrix on the device (LinearAlgebraTypes.hpp:57-132)."""

    def __init__(self, queue: Queue, data=None, cols=None, rows=None, dtype=np.float64):
        self._queue = queue
        self.dtype = np.dtype(dtype)
        self._N = 0
        self._NNZ = 0
        self._data = self._columns = self._rows = None
        self._csr = None
        self._host_rows = None
        if data is not None:
            self.init(data, cols, rows)

    def init(self, data, cols, rows) -> None:
        """LinearAlgebraTypes.hpp:101-121: upload a CSR triple."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        data = np.ascontiguousarray(data, dtype=self.dtype)
        self._N = len(rows) - 1
        self._NNZ = len(data)
        self._data = DeviceArray(self._queue, self._NNZ, self.dtype).upload(data)
        self._columns = DeviceArray(self._queue, self._NNZ, np.int32).upload(cols)
        self._rows = DeviceArray(self._queue, self._N + 1, np.int32).upload(rows)
        self._host_rows = rows
        self._drop_schedule()

    @classmethod
    def poisson(cls, queue: Queue, dim: int, nx: int, ny: int, nz: int = 1,
                dtype=np.float64) -> "Matrix":
        """Dirichlet Poisson CSR generated on the device."""
        m = cls(queue, dtype=dtype)
        zz = nz if dim == 3 else 1
        n = nx * ny * zz
        nnz = lib().cgx_poisson_nnz(dim, nx, ny, zz, 0, n)
        m._N, m._NNZ = n, nnz
        m._data = DeviceArray(queue, nnz, dtype)
        m._columns = DeviceArray(queue, nnz, np.int32)
        m._rows = DeviceArray(queue, n + 1, np.int32)
        check(lib().cgx_poisson_fill(queue.handle, _dtype_code(dtype), dim, nx, ny, zz, 0, n,
                                     m._rows.ptr, m._columns.ptr, m._data.ptr))
        queue.wait()
        return m

    def _drop_schedule(self):
        # libcgx refcounts the context from the handle, so this is valid after
        # the queue was closed (interpreter shutdown, a fixture closing first)
        if self._csr:
            lib().cgx_csr_destroy(self._csr)
        self._csr = None

    def schedule(self):
        """The cgx_csr handle (row-block schedule), built on first use."""
        if self._csr is None:
            if self._rows is None:
                raise CgxError("No Matrix given")
            h = _vp()
            hr = self._host_rows.ctypes.data if self._host_rows is not None else None
            check(lib().cgx_csr_create(self._queue.handle, self._N, self._NNZ, self._rows.ptr,
                                       self._columns.ptr, self._data.ptr,
                                       _dtype_code(self.dtype), hr, C.byref(h)))
            self._csr = h
        return self._csr

    def diag_inv(self) -> np.ndarray:
        """Extension: 1 / a_ii (a row's entries with col == row summed), formed
        on the device by cgx_csr_diag_inv — Jacobi's m. Raises CgxError when a
        row has no positive, finite diagonal."""
        out = DeviceArray(self._queue, self._N, self.dtype)
        check(lib().cgx_csr_diag_inv(self.schedule(), out.ptr))
        return out.download()

    def block_inv(self, block_size: int) -> np.ndarray:
        """Extension: the inverses of the diagonal blocks of ``block_size``
        rows (1..8) as an (N, block_size) array, row i holding its row of its
        block's inverse (cgx_csr_block_inv; the columns past a partial last
        block are 0) — block-Jacobi's W. ValueError for a block size outside
        1..8, before any device call; CgxError when a block has a pivot that is
        not positive and finite."""
        bs = int(block_size)
        if not 1 <= bs <= MAX_BLOCK_SIZE:
            raise ValueError(f"block_size {block_size!r} must be 1..{MAX_BLOCK_SIZE}")
        out = DeviceArray(self._queue, max(self._N * bs, 1), self.dtype)
        check(lib().cgx_csr_block_inv(self.schedule(), bs, out.ptr))
        return out.download()[:self._N * bs].reshape(self._N, bs)

    def data(self):
        return self._data

    def columns(self):
        return self._columns

    def rows(self):
        return self._rows

    def N(self) -> int:
        return self._N

    def NNZ(self) -> int:
        return self._NNZ

    def __del__(self):  # pragma: no cover
        try:
            self._drop_schedule()
        except Exception:
            pass


class Vector:
    """Vector on the device (LinearAlgebraTypes.hpp:143-203)."""

    def __init__(self, queue: Queue, arg=None, dtype=np.float64):
        self._q = queue
        self.dtype = np.dtype(dtype)
        self._N = 0
        self._ptr = None
        if isinstance(arg, (int, np.integer)):
            self._N = int(arg)
            self.init_empty(self._N)
        elif arg is not None:
            self.init(arg)

    def init_empty(self, size: int = 0) -> None:
        """:160-171 — allocate and zero (asserts a non-zero size)."""
        if size != 0 and self._N == 0:
            self._N = int(size)
        assert self._N != 0
        self._ptr = DeviceArray(self._q, self._N, self.dtype)
        self._ptr.fill(0.0)

    def init(self, data) -> None:
        """:177-183 — copy a host vector (the size is not recorded, as in the
        reference, unless it was never set)."""
        a = np.ascontiguousarray(data, dtype=self.dtype)
        self._ptr = DeviceArray(self._q, a.size, self.dtype).upload(a)
        if self._N == 0:
            self._N = a.size

    def data(self):
        return self._ptr

    def ptr(self):
        return self._ptr.ptr if self._ptr is not None else None

    def N(self) -> int:
        return self._N

    def to_numpy(self) -> np.ndarray:
        return self._ptr.download()


class Scalar:
    """Device-resident scalar (LinearAlgebraTypes.hpp:210-250)."""

    def __init__(self, queue: Queue, value: float = 0.0, dtype=np.float64):
        self._q = queue
        self.dtype = np.dtype(dtype)
        self.init(value)

    def init(self, value: float) -> None:
        self._v = DeviceArray(self._q, 1, self.dtype).upload(np.array([value], self.dtype))

    def ptr(self):
        return self._v.ptr

    def get(self) -> float:
        return float(self._v.download()[0])


class Event:
    """Stand-in for sycl::event: the queue is in order, so an event only
    names the point in the stream (VectorOperations methods return one)."""

    def __init__(self, queue: Queue):
        self.queue = queue

    def wait(self) -> None:
        self.queue.wait()


class VectorOperations:
    """src/VectorOperations.hpp:39-488. Methods are asynchronous and return an
    Event; scalars are device pointers (Scalar.ptr()) as in the reference."""

    def __init__(self, queue: Queue, dtype=np.float64, debug=Debuglevel.None_):
        self._queue = queue
        self.dtype = np.dtype(dtype)
        self._dt = _dtype_code(dtype)
        self.vector_size = 0
        self.workgroupsize = 128  # calculateWorkgroupSize :478-487 (min(128, max))

    def setVectorSize(self, size: int) -> None:
        self.vector_size = int(size)

    @staticmethod
    def _p(x):
        if isinstance(x, (Vector, Scalar)):
            return x.ptr()
        if isinstance(x, DeviceArray):
            return x.ptr
        return x

    def spmv(self, A: Matrix, vec, Result, NNZ=None, events=(), count=0) -> Event:
        """:438-466 — ignores NNZ, honours count, asserts A.N() == count."""
        self.vector_size = count if count else self.vector_size
        assert self.vector_size != 0 and A.N() == self.vector_size
        check(lib().cgx_spmv(self._queue.handle, A.schedule(), self._p(vec), self._p(Result),
                             self.vector_size))
        return Event(self._queue)

    def dot_product_trivial(self, left, right, result, dependencies=(), size=0) -> Event:
        """:287-309 — *result += left.right over vector_size (size ignored, Q7)."""
        check(lib().cgx_dot_acc(self._queue.handle, self._dt, self.vector_size, self._p(left),
                                self._p(right), self._p(result)))
        return Event(self._queue)

    def norm(self, vector, result, dependencies=(), size=0) -> Event:
        """:311-331 — *result += sum x^2 (no sqrt)."""
        check(lib().cgx_norm_acc(self._queue.handle, self._dt, self.vector_size,
                                 self._p(vector), self._p(result)))
        return Event(self._queue)

    def dot_product(self, left, right, result, dependencies=(), vec_size=0) -> Event:
        """:212-285 (deprecated in the reference) — *result += left.right."""
        self.vector_size = vec_size if vec_size else self.vector_size
        assert self.vector_size != 0
        return self.dot_product_trivial(left, right, result)

    def dot_product_optimised(self, Left, Right, result, dependencies=(), count=0) -> Event:
        """:110-208 — *result += Left.Right. The reference's multi-level tree
        indexes the wrong offsets beyond wg^2 groups (SURVEY §2 C2'); this one
        is the exact deterministic reduction for every size."""
        self.vector_size = count if count else self.vector_size
        assert self.vector_size != 0
        return self.dot_product_trivial(Left, Right, result)

    def saxpby(self, X, Y, a, b, Result, events=(), vec_size=0) -> Event:
        """:349-367 — Result = (*a) X + (*b) Y."""
        self.vector_size = vec_size if vec_size else self.vector_size
        check(lib().cgx_saxpby(self._queue.handle, self._dt, self.vector_size, self._p(X),
                               self._p(Y), self._p(a), self._p(b), self._p(Result)))
        return Event(self._queue)

    def sambx(self, X, Y, b, Result, events=(), count=0) -> Event:
        """:380-397 — Result = X - (*b) Y over vector_size (count ignored, Q7)."""
        check(lib().cgx_sambx(self._queue.handle, self._dt, self.vector_size, self._p(X),
                              self._p(Y), self._p(b), self._p(Result)))
        return Event(self._queue)

    def sapbx(self, X, Y, b, Result, events=(), count=0) -> Event:
        """:410-428 — Result = X + (*b) Y over vector_size (count ignored, Q7)."""
        check(lib().cgx_sapbx(self._queue.handle, self._dt, self.vector_size, self._p(X),
                              self._p(Y), self._p(b), self._p(Result)))
        return Event(self._queue)


class CG:
    """CGSolver::CG<DT, Debuglevel> (src/CG.hpp:53-601)."""

    def __init__(self, queue: Queue, dtype=np.float64, debug=Debuglevel.None_):
        self._queue = queue
        self.dtype = np.dtype(dtype)
        self.debug = debug
        self.A = Matrix(queue, dtype=dtype)
        self.x = Vector(queue, dtype=dtype)
        self.b = Vector(queue, dtype=dtype)
        self.is_solved = False
        self._cg = None
        self._cg_for = None
        self.iterations = 0       # extension: loop bodies of the last solve
        self.final_rxr = float("nan")  # extension: rxr after the last body
        self.final_rz = float("nan")   # extension: r.z after the last body (preconditioned)
        self._precond = Preconditioner.None_
        self._minv = None  # the caller's diagonal (a Vector), kept alive for the solver
        self._blk = BlockPreconditioner.None_  # setBlockPreconditioner: kind, block size and
        self._blk_bs = 0                       # the caller's blocks (host; the solver copies)
        self._blk_w = None
        self.poll_every = 32
        self.use_graph = True
        self.mode = 0  # cgx_cg_set_mode: 0 auto (5, 4, 6 or 3), 1 three kernels, 2 fused,
        # 3 deferred x, 4 fused + deferred x, 5 persistent body, 6 deferred x with Ap
        # recomputed (lean walk), 7 fused + deferred x with Ap recomputed (tile walk)
        self.batch_form = 0  # cgx_cg_set_batch_form: 0 auto, 1 fused, 2 sequential
        self.iterations_batch = None  # extension (solve_batch): loop bodies per column
        self.final_rxr_batch = None   # r.r after each column's last body
        self.stopped_batch = None     # 1 stop rule / NaN, 2 cap reached, per column
        self.iterations_shifted = None  # extension (solve_shifted): loop bodies per shift
        self.residual_shifted = None    # |zeta_s| ||r|| after each shift's last body
        self.stopped_shifted = None     # 1 frozen by the rule, 2 cap reached, per shift
        self._mixed = None        # cgx_mixed handle (solve_mixed), built on first use
        self._mixed_for = None
        self._mixed_cfg = None    # the (mode, preconditioner) its inner solver was given
        self.outer_steps = 0      # extension (solve_mixed): corrections applied
        self.mixed_status = None  # 1 tolerance, 2 cap, 3 stagnated, 4 NaN
        self.mixed_history = None  # [(f64 r.r, inner bodies, inner final f32 r.r)]

    @classmethod
    def createCG(cls, dtype=np.float64, debug=Debuglevel.None_, device: int = 0) -> "CG":
        """:70-77 — a CG with its own default queue."""
        return cls(Queue(device), dtype, debug)

    # -- inputs ---------------------------------------------------------
    def setMatrix(self, data, columns=None, rows=None) -> None:
        """:87-93 (host CSR triple) and :102 (a device Matrix, moved)."""
        if isinstance(data, Matrix):
            self.A = data
        else:
            self.A.init(data, columns, rows)
        self._drop_solver()
        self._drop_mixed()

    def getDimension(self) -> int:
        """:156"""
        return self.A.N()

    def setTarget(self, data) -> None:
        """:164-170 (host vector) and :206 (a device Vector)."""
        if isinstance(data, Vector):
            self.b = data
        else:
            self.b.init(data)
            self._queue.wait()

    def setInital(self, data) -> None:
        """:215-219 (sic) — initial guess from a host vector."""
        self.x.init(data)
        self._queue.wait()

    def setInitial(self, V) -> None:
        """:244 — initial guess from a device Vector (moved)."""
        if isinstance(V, Vector):
            self.x = V
        else:
            self.setInital(V)

    def calculateExpectedStepCount(self, accuracy) -> None:
        """:235 (empty in the reference)."""
        return None

    def setPreconditioner(self, kind, diag=None) -> None:
        """Extension: diagonal preconditioning of the following solves (modes
        1 and 3; auto resolves to 3; the stop rule still tests the true r.r).
        ``Jacobi`` builds 1 / diag(A) on the device, from the matrix in place
        at each solve; ``Diagonal`` takes ``diag``, N positive finite values
        as a numpy array or a device Vector, kept alive by this object.
        ValueError for an unknown kind, a missing ``diag`` or a wrong length."""
        try:
            kind = Preconditioner(kind)
        except (ValueError, TypeError):
            raise ValueError(f"unknown preconditioner kind {kind!r}") from None
        minv = None
        if kind == Preconditioner.Diagonal:
            if diag is None:
                raise ValueError("Preconditioner.Diagonal needs diag")
            n = diag.N() if isinstance(diag, Vector) else int(np.size(diag))
            if self.A.N() and n != self.A.N():
                raise ValueError(f"diag has {n} entries, the matrix {self.A.N()} rows")
            if n == 0:
                raise ValueError("diag is empty")
            minv = diag if isinstance(diag, Vector) else Vector(self._queue, np.asarray(diag),
                                                                dtype=self.dtype)
        self._precond, self._minv = kind, minv
        self._blk, self._blk_bs, self._blk_w = BlockPreconditioner.None_, 0, None  # replaced
        if self._cg is not None and self._cg_for == self.A._csr:
            self._apply_precond()

    def setBlockPreconditioner(self, kind, block_size: int = 0, blocks=None) -> None:
        """Extension: block-Jacobi preconditioning of the following solves
        (cgx_cg_set_block_precond; float64, modes 1 and 3, auto resolves to 3;
        the stop rule still tests the true r.r). ``Jacobi`` inverts A's
        diagonal blocks of ``block_size`` rows (1..8) on the device, from the
        matrix in place at each solve; ``Given`` takes ``blocks``, an
        (N, block_size) array whose row i is row i of its block's matrix — each
        block symmetric positive definite, which is the caller's duty (only
        finite entries and a positive diagonal are checked). It replaces a
        preconditioner set by ``setPreconditioner`` and is replaced by it.
        ValueError, before any device call, for an unknown kind, a block size
        outside 1..8, missing ``blocks`` or a wrong shape; TypeError on a
        float32 CG."""
        try:
            kind = BlockPreconditioner(kind)
        except (ValueError, TypeError):
            raise ValueError(f"unknown block preconditioner kind {kind!r}") from None
        bs, w = 0, None
        if kind != BlockPreconditioner.None_:
            if self.dtype != np.float64:
                raise TypeError(f"block preconditioning is float64; this CG is {self.dtype}")
            bs = int(block_size)
            if not 1 <= bs <= MAX_BLOCK_SIZE:
                raise ValueError(f"block_size {block_size!r} must be 1..{MAX_BLOCK_SIZE}")
        if kind == BlockPreconditioner.Given:
            if blocks is None:
                raise ValueError("BlockPreconditioner.Given needs blocks")
            arr = np.ascontiguousarray(blocks, dtype=np.float64)
            if arr.ndim != 2 or arr.shape[1] != bs or arr.shape[0] == 0:
                raise ValueError(f"blocks has shape {arr.shape}, expected (N, {bs})")
            if self.A.N() and arr.shape[0] != self.A.N():
                raise ValueError(f"blocks has {arr.shape[0]} rows, the matrix {self.A.N()}")
            w = arr
        self._blk, self._blk_bs, self._blk_w = kind, bs, w
        self._precond, self._minv = Preconditioner.None_, None  # replaced
        if self._cg is not None and self._cg_for == self.A._csr:
            self._apply_precond()

    def _apply_precond(self) -> None:
        if self._blk != BlockPreconditioner.None_:
            d_w = None
            if self._blk == BlockPreconditioner.Given:
                if self._blk_w.shape[0] != self.A.N():
                    raise ValueError(f"blocks has {self._blk_w.shape[0]} rows, the matrix "
                                     f"{self.A.N()}")
                d_w = DeviceArray(self._queue, self._blk_w.size, np.float64)
                d_w.upload(self._blk_w.ravel())  # the solver keeps a copy of its own
            check(lib().cgx_cg_set_block_precond(self._cg, int(self._blk), self._blk_bs,
                                                 d_w.ptr if d_w is not None else None))
            return
        if self._precond == Preconditioner.Diagonal and self._minv.N() != self.A.N():
            raise ValueError(f"diag has {self._minv.N()} entries, the matrix {self.A.N()} rows")
        check(lib().cgx_cg_set_precond(
            self._cg, int(self._precond),
            self._minv.ptr() if self._precond == Preconditioner.Diagonal else None))

    # -- solve ----------------------------------------------------------
    def _drop_solver(self):
        if self._cg:  # valid after Queue.close (see Matrix._drop_schedule)
            lib().cgx_cg_destroy(self._cg)
        self._cg = None
        self._cg_for = None

    def _solver(self):
        sched = self.A.schedule()
        if self._cg is None or self._cg_for != sched:
            self._drop_solver()
            h = _vp()
            check(lib().cgx_cg_create(self._queue.handle, sched, C.byref(h)))
            self._cg = h
            self._cg_for = sched
            check(lib().cgx_cg_config(self._cg, self.poll_every, 1 if self.use_graph else 0))
            check(lib().cgx_cg_set_mode(self._cg, self.mode))
            if self._precond != Preconditioner.None_ or self._blk != BlockPreconditioner.None_:
                self._apply_precond()
        return self._cg

    def solve(self, improvement: float = 0.0, max_iter: int = -1) -> None:
        """:255-454. Throws RuntimeError for a missing b or A (:266-272).
        max_iter caps the loop bodies (extension; -1 keeps the cap N+1)."""
        if self.b.ptr() is None:
            raise RuntimeError("No right hand side to solve for")
        if self.A.columns() is None:
            raise RuntimeError("No Matrix given")
        n = self.A.N()
        if self.x.ptr() is None:  # :291-297
            self.x = Vector(self._queue, n, dtype=self.dtype)
        bodies = C.c_int64(0)
        rxr = C.c_double(0)
        check(lib().cgx_cg_solve(self._solver(), self.b.ptr(), self.x.ptr(), float(improvement),
                                 int(max_iter), C.byref(bodies), C.byref(rxr)))
        self.iterations = bodies.value
        self.final_rxr = rxr.value
        self.final_rz = float("nan")
        if self._precond != Preconditioner.None_ or self._blk != BlockPreconditioner.None_:
            rz = C.c_double(0)
            check(lib().cgx_cg_rz(self._cg, C.byref(rz)))
            self.final_rz = rz.value
        self.is_solved = True

    def _drop_mixed(self):
        if self._mixed:
            lib().cgx_mixed_destroy(self._mixed)
        self._mixed = None
        self._mixed_for = None
        self._mixed_cfg = None

    def solve_mixed(self, improvement: float = 0.0, max_iter: int = -1,
                    inner_reduction: float = 0, max_outer: int = 0, inner_cap: int = 0,
                    fallback: bool = True) -> None:
        """Extension (cgx_mixed_solve): the f64 system solved to
        ``improvement`` on the true f64 residual with the loop bodies run by
        the f32 solver on a cast copy of the matrix (iterative refinement).
        f64 ``CG`` only (TypeError otherwise, before any device call).
        ``mode`` is the inner solver's mode and ``setPreconditioner`` its
        preconditioner (a caller's diagonal is cast to f32). ``max_iter`` caps
        the inner bodies of the whole call; ``inner_reduction``, ``max_outer``
        and ``inner_cap``: 0 keeps the default (1e-5, 8, N + 1), ValueError
        for a negative or non-finite value. Sets ``iterations`` (inner
        bodies), ``outer_steps``, ``final_rxr`` (the last true r.r),
        ``mixed_status`` (1 tolerance reached, 2 cap, 3 stagnated, 4 NaN) and
        ``mixed_history`` ([(r.r, inner bodies, inner final r.r)] per residual
        evaluation). With ``fallback`` a status 3 or 4 continues with the
        ordinary f64 ``solve`` from the current x; its bodies are added to
        ``iterations`` and ``mixed_status`` keeps the 3 or 4."""
        if self.dtype != np.float64:
            raise TypeError(f"solve_mixed refines a float64 system; this CG is {self.dtype}")
        if not (np.isfinite(inner_reduction) and inner_reduction >= 0):
            raise ValueError(f"inner_reduction {inner_reduction!r} must be finite and not negative")
        if int(max_outer) < 0:
            raise ValueError(f"max_outer {max_outer!r} must not be negative")
        if int(inner_cap) < 0:
            raise ValueError(f"inner_cap {inner_cap!r} must not be negative")
        if self.b.ptr() is None:
            raise RuntimeError("No right hand side to solve for")
        if self.A.columns() is None:
            raise RuntimeError("No Matrix given")
        n = self.A.N()
        if self.x.ptr() is None:
            self.x = Vector(self._queue, n, dtype=self.dtype)
        L = lib()
        sched = self.A.schedule()
        if self._mixed is None or self._mixed_for != sched:
            self._drop_mixed()
            h = _vp()
            check(L.cgx_mixed_create(self._queue.handle, sched, C.byref(h)))
            self._mixed, self._mixed_for = h, sched
        m = self._mixed
        inner = _vp()
        check(L.cgx_mixed_inner(m, None, C.byref(inner)))
        if self._blk != BlockPreconditioner.None_:
            # refused, whatever the kind: the inner solver is f32 (CGX_EUNSUPPORTED)
            check(L.cgx_cg_set_block_precond(inner, int(BlockPreconditioner.Jacobi),
                                             self._blk_bs, None))
        check(L.cgx_cg_config(inner, self.poll_every, 1 if self.use_graph else 0))
        # (mode before the preconditioner, and NONE first: whichever of the two
        # comes second refuses a mode that runs no preconditioner)
        cfg = (self.mode, self._precond, self._minv)
        if cfg != self._mixed_cfg:  # (setting either drops the inner solver's captured graphs)
            self._mixed_cfg = None
            check(L.cgx_mixed_set_precond(m, int(Preconditioner.None_), None))
            check(L.cgx_mixed_set_mode(m, self.mode))
            if self._precond != Preconditioner.None_:
                if self._precond == Preconditioner.Diagonal and self._minv.N() != n:
                    raise ValueError(f"diag has {self._minv.N()} entries, the matrix {n} rows")
                check(L.cgx_mixed_set_precond(
                    m, int(self._precond),
                    self._minv.ptr() if self._precond == Preconditioner.Diagonal else None))
            self._mixed_cfg = cfg
        check(L.cgx_mixed_config(m, float(inner_reduction), int(max_outer), int(inner_cap)))
        outer, bodies, rxr, status = C.c_int(0), C.c_int64(0), C.c_double(0), C.c_int(0)
        check(L.cgx_mixed_solve(m, self.b.ptr(), self.x.ptr(), float(improvement), int(max_iter),
                                C.byref(outer), C.byref(bodies), C.byref(rxr), C.byref(status)))
        cnt = C.c_int(0)
        check(L.cgx_mixed_history(m, None, None, None, 0, C.byref(cnt)))
        k = cnt.value
        rr, ib, ir = (C.c_double * k)(), (C.c_int64 * k)(), (C.c_double * k)()
        check(L.cgx_mixed_history(m, rr, ib, ir, k, C.byref(cnt)))
        self.mixed_history = [(rr[i], ib[i], ir[i]) for i in range(k)]
        self.iterations = bodies.value
        self.outer_steps = outer.value
        self.final_rxr = rxr.value
        self.final_rz = float("nan")
        self.mixed_status = status.value
        self.is_solved = True
        if fallback and status.value in (3, 4):
            self.solve(improvement, max_iter)
            self.iterations += bodies.value

    MAX_BATCH = 8  # cgx.h: a batch has 1 to 8 right-hand sides

    def solve_batch(self, B, X0=None, improvement: float = 0.0, max_iter: int = -1) -> np.ndarray:
        """Extension (cgx_cg_solve_batch): k independent solves A x_c = b_c,
        k = 1..8, the columns of ``B`` (n, k) in any memory order; ``X0`` (same
        shape) holds the initial guesses (default 0). Returns X (n, k) and sets
        ``iterations_batch``, ``final_rxr_batch`` and ``stopped_batch``. Every
        column is the single solve's in mode 1, bit for bit, when the fused
        form runs (``batch_form``: 0 auto, 1 fused, 2 sequential). ValueError,
        before any device call, for a wrong row count, k outside 1..8 or an
        X0 whose shape is not B's."""
        B = np.asarray(B)
        n = self.A.N()
        if B.ndim != 2:
            raise ValueError(f"B must be a 2-D (n, k) array, got {B.ndim} dimension(s)")
        if B.shape[0] != n:
            raise ValueError(f"B has {B.shape[0]} rows, the matrix {n}")
        k = B.shape[1]
        if not 1 <= k <= self.MAX_BATCH:
            raise ValueError(f"a batch has 1 to {self.MAX_BATCH} right-hand sides, got {k}")
        if X0 is not None:
            X0 = np.asarray(X0)
            if X0.shape != B.shape:
                raise ValueError(f"X0 has shape {X0.shape}, B {B.shape}")
        if self.A.columns() is None:
            raise RuntimeError("No Matrix given")
        # column-major on the device: column c at element c * n
        dB = DeviceArray(self._queue, n * k, self.dtype).upload(
            np.asarray(B, dtype=self.dtype).T.ravel())
        dX = DeviceArray(self._queue, n * k, self.dtype)
        if X0 is None:
            dX.fill(0.0)
        else:
            dX.upload(np.asarray(X0, dtype=self.dtype).T.ravel())
        bodies = (C.c_int64 * k)()
        rxr = (C.c_double * k)()
        stopped = (C.c_int * k)()
        cg = self._solver()
        check(lib().cgx_cg_set_batch_form(cg, int(self.batch_form)))
        check(lib().cgx_cg_solve_batch(cg, k, dB.ptr, n, dX.ptr, n, float(improvement),
                                       int(max_iter), bodies, rxr, stopped))
        self.iterations_batch = np.array(bodies[:], dtype=np.int64)
        self.final_rxr_batch = np.array(rxr[:], dtype=np.float64)
        self.stopped_batch = np.array(stopped[:], dtype=np.int32)
        return np.ascontiguousarray(dX.download().reshape(k, n).T)

    def batch_info(self):
        """(form in effect: 1 fused or 2 sequential, instantiated width of the
        fused form's buffers or 0) for ``batch_form`` on this matrix."""
        cg = self._solver()
        check(lib().cgx_cg_set_batch_form(cg, int(self.batch_form)))
        form, width = C.c_int(0), C.c_int(0)
        check(lib().cgx_cg_batch_info(cg, C.byref(form), C.byref(width)))
        return form.value, width.value

    MAX_SHIFTS = 8  # cgx.h CGX_SHIFT_MAX

    def solve_shifted(self, sigmas, improvement: float = 0.0, max_iter: int = -1) -> np.ndarray:
        """Extension (cgx_cg_solve_shifted): (A + sigma_s I) x_s = b for
        S = 1..8 shifts sigma_s >= 0 on ``setTarget``'s b, every x_s from zero,
        all from one Krylov space (one SpMV and one pair of dots per body).
        Returns X (n, S) and sets ``iterations_shifted``, ``residual_shifted``
        (|zeta_s| ||r|| after each shift's last body) and ``stopped_shifted``
        (1 frozen by the rule, 2 cap reached). A sigma = 0 column is the single
        mode-1 solve from a zero initial guess, bit for bit. ValueError, before
        any device call, for S outside 1..8 or a shift that is negative or not
        finite."""
        sg = np.atleast_1d(np.asarray(sigmas, dtype=np.float64))
        if sg.ndim != 1 or not 1 <= sg.size <= self.MAX_SHIFTS:
            raise ValueError(f"a shifted solve has 1 to {self.MAX_SHIFTS} shifts, got "
                             f"{sg.size if sg.ndim == 1 else sg.shape}")
        if not np.all(np.isfinite(sg)) or np.any(sg < 0):
            raise ValueError(f"a shift is finite and not negative, got {sg.tolist()}")
        if self.b.ptr() is None:
            raise RuntimeError("No right hand side to solve for")
        if self.A.columns() is None:
            raise RuntimeError("No Matrix given")
        n, k = self.A.N(), int(sg.size)
        dX = DeviceArray(self._queue, n * k, self.dtype)
        bodies = (C.c_int64 * k)()
        res = (C.c_double * k)()
        stopped = (C.c_int * k)()
        check(lib().cgx_cg_solve_shifted(self._solver(), k, (C.c_double * k)(*sg.tolist()),
                                         self.b.ptr(), dX.ptr, n, float(improvement),
                                         int(max_iter), bodies, res, stopped))
        self.iterations_shifted = np.array(bodies[:], dtype=np.int64)
        self.residual_shifted = np.array(res[:], dtype=np.float64)
        self.stopped_shifted = np.array(stopped[:], dtype=np.int32)
        return np.ascontiguousarray(dX.download().reshape(k, n).T)

    # -- outputs --------------------------------------------------------
    def accuracy(self) -> float:
        """:463-515 — |sum (b - A x)^2 / sum x^2| (squared norms, Q6)."""
        out = C.c_double(0)
        check(lib().cgx_accuracy(self._queue.handle, self.A.schedule(), self.b.ptr(),
                                 self.x.ptr(), C.byref(out)))
        return out.value

    def extract(self) -> np.ndarray:
        """:517-523"""
        return self.x.data().download()[: self.A.N()]

    def extractTo(self, result: list) -> None:
        """:529-532 — resizes `result` to N and copies x into it."""
        v = self.extract()
        result[:] = v.tolist()

    def memoryFootprint(self) -> int:
        """:555-558"""
        it = self.dtype.itemsize
        return (2 * self.A.NNZ() + 4 * self.A.N()) * it + 2 * self.A.N() * 4

    def __del__(self):  # pragma: no cover
        try:
            self._drop_mixed()
            self._drop_solver()
        except Exception:
            pass


class ManyCG:
    """Extension (cgx_many): ``nsys`` small SPD systems on one
    sparsity pattern, each solved by one workgroup that runs the whole CG loop.

    ``rows`` (n + 1) and ``cols`` (nnz) are the shared CSR pattern, ``vals``
    (nsys, nnz) each system's values; n <= 4096, float64. Every system's
    result is the single solve's in mode 1, bit for bit (cgx.h). ValueError /
    TypeError, before any device call, for a float32 ``vals``, a shape that
    does not fit, n outside 1..4096 or a malformed ``rows``. ``set_values``
    overwrites the values in place for the next solve (no new create).
    ``set_preconditioner`` turns on Jacobi or a caller's diagonal inside the
    kernel (cgx_many_set_precond), ``set_block_preconditioner`` block-Jacobi
    with dense diagonal blocks of 1 to 8 rows (cgx_many_set_block_precond);
    the two replace each other, and ``rz`` then holds each system's final r.z.
    ``set_form`` chooses between a workgroup and, for n <= 256, a wave per
    system (cgx_many_set_form); ``form`` is (requested, in effect)."""

    MAX_N = 4096
    FORM_AUTO, FORM_WORKGROUP, FORM_WAVE = (N.MANY_FORM_AUTO, N.MANY_FORM_WORKGROUP,
                                            N.MANY_FORM_WAVE)

    def __init__(self, queue: Queue, rows, cols, vals, max_workgroups: int = 0):
        vals = np.asarray(vals)
        if vals.dtype == np.float32:
            raise TypeError("ManyCG solves float64 systems; vals is float32")
        if vals.ndim != 2:
            raise ValueError(f"vals must be a 2-D (nsys, nnz) array, got {vals.ndim} dimension(s)")
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        nsys, nnz = vals.shape
        n = len(rows) - 1
        if nsys < 1:
            raise ValueError("vals holds no system (nsys must be at least 1)")
        if not 1 <= n <= self.MAX_N:
            raise ValueError(f"a system has 1 to {self.MAX_N} rows, got {n}; solve larger "
                             "systems one at a time with CG.solve")
        if len(cols) != nnz:
            raise ValueError(f"cols has {len(cols)} entries, vals {nnz} per system")
        if rows[0] != 0 or rows[-1] != nnz:
            raise ValueError(f"rows must run from 0 to nnz = {nnz}, got {rows[0]} .. {rows[-1]}")
        if int(max_workgroups) < 0:
            raise ValueError(f"max_workgroups {max_workgroups!r} must not be negative")
        self._queue = queue
        self.nsys, self.n, self.nnz = nsys, n, nnz
        self.bodies = self.rxr = self.stopped = self.rz = None
        self._h = None
        self._precond, self._diag = Preconditioner.None_, None
        self._block, self._blocks = BlockPreconditioner.None_, None
        self._rows = DeviceArray(queue, n + 1, np.int32).upload(rows)
        self._cols = DeviceArray(queue, nnz, np.int32).upload(cols)
        self._vals = DeviceArray(queue, nsys * nnz, np.float64).upload(
            np.asarray(vals, dtype=np.float64).ravel())
        h = _vp()
        check(lib().cgx_many_create(queue.handle, N.F64, nsys, n, nnz, self._rows.ptr,
                                    self._cols.ptr, self._vals.ptr, nnz, C.byref(h)))
        self._h = h
        if max_workgroups:
            self.config(max_workgroups)

    def config(self, max_workgroups: int = 0) -> None:
        """Cap the grid (0: the resident workgroups); a tuning knob."""
        check(lib().cgx_many_config(self._h, int(max_workgroups)))

    def info(self):
        """(workgroups of the next solve, rows per thread, LDS bytes per workgroup)"""
        wg, r, lds = C.c_int(0), C.c_int(0), C.c_int64(0)
        check(lib().cgx_many_info(self._h, C.byref(wg), C.byref(r), C.byref(lds)))
        return wg.value, r.value, lds.value

    def set_form(self, form) -> None:
        """The next solves' kernel form: ``FORM_AUTO`` (the default),
        ``FORM_WORKGROUP`` (a workgroup per system) or ``FORM_WAVE`` (a wave per
        system, n <= 256; CgxError above). The results do not depend on it
        wherever the dots are clear, and not at all for n <= 64. ValueError,
        before any device call, for an unknown form."""
        if form not in (self.FORM_AUTO, self.FORM_WORKGROUP, self.FORM_WAVE) or \
                isinstance(form, (bool, float)):
            raise ValueError(f"unknown form {form!r}")
        check(lib().cgx_many_set_form(self._h, int(form)))

    @property
    def form(self):
        """(the form as requested, the form the next solve launches: 1 or 2)"""
        req, eff = C.c_int(0), C.c_int(0)
        check(lib().cgx_many_get_form(self._h, C.byref(req), C.byref(eff)))
        return req.value, eff.value

    def set_values(self, vals) -> None:
        """Overwrite every system's values in place; the next solve reads them."""
        vals = np.asarray(vals, dtype=np.float64)
        if vals.shape != (self.nsys, self.nnz):
            raise ValueError(f"vals has shape {vals.shape}, expected {(self.nsys, self.nnz)}")
        self._vals.upload(vals.ravel())

    def set_preconditioner(self, kind, diag=None) -> None:
        """The next solves' preconditioner: ``Preconditioner.None_``, ``Jacobi``
        (1 / a_ii, formed in the kernel from the values each solve reads) or
        ``Diagonal`` with ``diag`` (nsys, n), system s's m in row s. A system
        whose diagonal (Jacobi) or m (Diagonal) is not positive and finite
        stops alone with code 3 and its x untouched. ValueError, before any
        device call, for an unknown kind, a missing ``diag`` or a wrong shape."""
        try:
            kind = Preconditioner(kind)
        except ValueError:
            raise ValueError(f"unknown preconditioner kind {kind!r}") from None
        d_diag = None
        if kind == Preconditioner.Diagonal:
            if diag is None:
                raise ValueError("Preconditioner.Diagonal needs diag, an (nsys, n) array")
            diag = np.asarray(diag, dtype=np.float64)
            if diag.shape != (self.nsys, self.n):
                raise ValueError(f"diag has shape {diag.shape}, expected {(self.nsys, self.n)}")
            d_diag = DeviceArray(self._queue, self.nsys * self.n, np.float64).upload(diag.ravel())
        check(lib().cgx_many_set_precond(self._h, int(kind), d_diag.ptr if d_diag else None,
                                         self.n))
        self._precond, self._diag = kind, d_diag  # (the old diag lives until the call above)
        self._block, self._blocks = BlockPreconditioner.None_, None  # replaced
        self.rz = None

    def set_block_preconditioner(self, kind, block_size: int = 0, blocks=None) -> None:
        """The next solves' block preconditioner (cgx_many_set_block_precond):
        ``BlockPreconditioner.None_``, ``Jacobi`` (the inverses of every
        system's diagonal blocks of ``block_size`` rows, 1..8, formed on the
        device at each solve from the values that solve reads) or ``Given``
        with ``blocks``, an (nsys, n, block_size) or (nsys, n * block_size)
        array, row i of system s holding row i of its block's matrix; it is
        uploaded and kept alive by the object. Each block symmetric positive
        definite is the caller's duty. A system with a bad block stops alone
        with code 3 and its x untouched. It replaces a preconditioner set by
        ``set_preconditioner`` and is replaced by it. ValueError, before any
        device call, for an unknown kind, a block size outside 1..8, missing
        ``blocks`` or a wrong shape."""
        try:
            kind = BlockPreconditioner(kind)
        except (ValueError, TypeError):
            raise ValueError(f"unknown block preconditioner kind {kind!r}") from None
        bs, d_w = 0, None
        if kind != BlockPreconditioner.None_:
            bs = int(block_size)
            if not 1 <= bs <= MAX_BLOCK_SIZE:
                raise ValueError(f"block_size {block_size!r} must be 1..{MAX_BLOCK_SIZE}")
        if kind == BlockPreconditioner.Given:
            if blocks is None:
                raise ValueError("BlockPreconditioner.Given needs blocks, an (nsys, n, "
                                 "block_size) array")
            arr = np.asarray(blocks, dtype=np.float64)
            if arr.shape not in ((self.nsys, self.n, bs), (self.nsys, self.n * bs)):
                raise ValueError(f"blocks has shape {arr.shape}, expected "
                                 f"{(self.nsys, self.n, bs)} or {(self.nsys, self.n * bs)}")
            d_w = DeviceArray(self._queue, self.nsys * self.n * bs, np.float64).upload(arr.ravel())
        check(lib().cgx_many_set_block_precond(self._h, int(kind), bs,
                                               d_w.ptr if d_w else None, self.n * bs))
        self._block, self._blocks = kind, d_w  # (the old blocks live until the call above)
        self._precond, self._diag = Preconditioner.None_, None  # replaced
        self.rz = None

    def block_inv(self, block_size: int):
        """(W, bad_systems): W (nsys, n, block_size), the inverses of every
        system's diagonal blocks as ``set_block_preconditioner(Jacobi)`` forms
        them from the current values (cgx_many_block_inv; the columns past a
        partial last block are 0), and the indices of the systems with a block
        whose pivot is not positive and finite. ValueError, before any device
        call, for a block size outside 1..8."""
        bs = int(block_size)
        if not 1 <= bs <= MAX_BLOCK_SIZE:
            raise ValueError(f"block_size {block_size!r} must be 1..{MAX_BLOCK_SIZE}")
        ns, n = self.nsys, self.n
        out = DeviceArray(self._queue, ns * n * bs, np.float64)
        nbad, first = C.c_int64(0), C.c_int64(-1)
        check(lib().cgx_many_block_inv(self._h, bs, out.ptr, n * bs, C.byref(nbad),
                                       C.byref(first)))
        verdicts = (C.c_int * ns)()
        check(lib().cgx_many_block_bad(self._h, verdicts))
        bad = np.nonzero(np.array(verdicts[:]))[0]  # (nbad of them, the first one `first`)
        return out.download()[:ns * n * bs].reshape(ns, n, bs), bad

    def solve(self, B, X0=None, improvement: float = 0.0, max_iter: int = -1) -> np.ndarray:
        """Solve A_s x_s = b_s for every s: ``B`` (nsys, n), ``X0`` the initial
        guesses (same shape; default 0). ``improvement`` is the absolute
        tolerance on sqrt(r.r) and ``max_iter`` caps the bodies (-1: n + 1), as
        CG.solve's. Returns X (nsys, n) and sets ``bodies``, ``rxr`` (the r.r
        after each system's last body), ``stopped`` (1 stop rule or NaN,
        2 cap, 3 a bad diagonal under a preconditioner) and, under a
        preconditioner, ``rz`` (else None). ValueError, before any device
        call, for a wrong shape."""
        B = np.asarray(B)
        if B.shape != (self.nsys, self.n):
            raise ValueError(f"B has shape {B.shape}, expected {(self.nsys, self.n)}")
        if X0 is not None:
            X0 = np.asarray(X0)
            if X0.shape != B.shape:
                raise ValueError(f"X0 has shape {X0.shape}, B {B.shape}")
        ns, n = self.nsys, self.n
        dB = DeviceArray(self._queue, ns * n, np.float64).upload(
            np.asarray(B, dtype=np.float64).ravel())
        dX = DeviceArray(self._queue, ns * n, np.float64)
        if X0 is None:
            dX.fill(0.0)
        else:
            dX.upload(np.asarray(X0, dtype=np.float64).ravel())
        bodies, rxr, stopped = (C.c_int64 * ns)(), (C.c_double * ns)(), (C.c_int * ns)()
        check(lib().cgx_many_solve(self._h, dB.ptr, n, dX.ptr, n, float(improvement),
                                   int(max_iter), bodies, rxr, stopped))
        self.bodies = np.array(bodies[:], dtype=np.int64)
        self.rxr = np.array(rxr[:], dtype=np.float64)
        self.stopped = np.array(stopped[:], dtype=np.int32)
        self.rz = None
        if getattr(self, "_precond", Preconditioner.None_) != Preconditioner.None_ or \
                getattr(self, "_block", BlockPreconditioner.None_) != BlockPreconditioner.None_:
            rz = (C.c_double * ns)()
            check(lib().cgx_many_rz(self._h, rz))
            self.rz = np.array(rz[:], dtype=np.float64)
        return dX.download().reshape(ns, n)

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().cgx_many_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass
