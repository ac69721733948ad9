#ifndef CG_HPP
#define CG_HPP
/**
 * @file CG.hpp
 * Drop-in for the reference's src/CG.hpp: class CGSolver::CG<DT, Debuglevel>
 * with the same members (cited per member), running on libcgx's gfx950
 * kernels (include/cgx.h). test/Tester.cpp compiles against it unmodified.
 *
 * solve() keeps the reference's iteration semantics: the body
 * runs, then stops if r.r at the START of the body is NaN or its square root
 * is <= improvement; at most N + 1 bodies; improvement 0 runs until r.r
 * underflows (then x is NaN, as in the reference). Instead of 12 submissions
 * and a host drain per iteration (CG.hpp:359-436) it runs three fused kernels
 * per iteration with device-resident scalars and polls the stop flag every
 * few iterations.
 */
#include <AdaptiveCpp/sycl/sycl.hpp>
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <exception>
#include <iostream>
#include <limits>
#include <memory>
#include <ostream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "LinearAlgebraTypes.hpp"
#include "VectorOperations.hpp"

namespace CGSolver {

namespace asycl = acpp::sycl;

namespace detail {
struct CgDeleter {
  void operator()(cgx_cg *c) const {
    if (c) cgx_cg_destroy(c);
  }
};
struct MixedDeleter {
  void operator()(cgx_mixed *m) const {
    if (m) cgx_mixed_destroy(m);
  }
};
}  // namespace detail

/**
 * Extension (not in the reference): diagonal preconditioning of solve(),
 * cgx.h's CGX_PRECOND_* kinds. Jacobi: 1 / diag(A), built on the device from
 * the matrix; Diagonal: a vector the caller supplies.
 */
enum class Preconditioner { None = CGX_PRECOND_NONE, Jacobi = CGX_PRECOND_JACOBI,
                            Diagonal = CGX_PRECOND_DIAGONAL };

/**
 * Extension (not in the reference): block-Jacobi preconditioning of solve(),
 * cgx.h's CGX_BLOCK_* kinds, with dense diagonal blocks of 1 to 8 rows.
 * Jacobi: the inverses of A's diagonal blocks, built on the device; Given:
 * N x block_size row-major values the caller supplies.
 */
enum class BlockPreconditioner { None = CGX_BLOCK_NONE, Jacobi = CGX_BLOCK_JACOBI,
                                 Given = CGX_BLOCK_GIVEN };

/**
 * @class CG (CG.hpp:53-601)
 * Set matrix, right-hand side and optional initial guess, solve, extract.
 */
template <typename DT, Debuglevel debug = Debuglevel::None> class CG {
 public:
  using Scalar = ::CGSolver::Scalar<DT>;
  using Matrix = ::CGSolver::Matrix<DT>;
  using Vector = ::CGSolver::Vector<DT>;

  /** :61 — no device memory is allocated yet */
  CG(asycl::queue &queue) : _queue(queue), A(queue), x(_queue), b(_queue) {
    if constexpr (debug == Debuglevel::Verbose) std::clog << "Constructing CG Object\n";
  }

  /** :70-77 — a CG on a default queue */
  static std::unique_ptr<CG> createCG() {
    asycl::queue q;
    std::unique_ptr<CG> cg(new CG(q));
    return cg;
  }

  /** :87-93 — CSR triple from the host */
  void setMatrix(std::vector<DT> &data, std::vector<int> &columns, std::vector<int> &rows) {
    if constexpr (debug == Debuglevel::Verbose) std::clog << "Setting Matrix\n";
    A.init(data, columns, rows);
    _solver.reset();
    _mixed.reset();
  }

  /** :102 — a device matrix, moved */
  void setMatrix(Matrix &&M) {
    A = std::forward<Matrix>(M);
    _solver.reset();
    _mixed.reset();
  }

  /** :156 */
  int getDimension() const { return this->A.N(); }

  /** :164-170 */
  void setTarget(std::vector<DT> &_data) {
    b.init(_data);
    executeQueue();
  }

  /** :206 */
  void setTarget(Vector &&V) { b = std::forward<Vector>(V); }

  /** :215-219 (sic) — initial guess from the host */
  void setInital(std::vector<DT> &_data) {
    x.init(_data);
    executeQueue();
  }

  /** :235 (empty in the reference) */
  void calculateExpectedStepCount(DT accuracy) {}

  /** :244 — initial guess on the device, moved */
  void setInitial(Vector &&V) { x = std::forward<Vector>(V); }

  /**
   * :255-454 — Solve A x = b.
   * @throw std::runtime_error if b or A is missing (:266-272)
   */
  void solve(DT improvement = static_cast<DT>(0)) {
    if constexpr (debug == Debuglevel::Verbose) std::clog << "Solving System\n";
    // :260-261 (its constructor prints the work-group line under Verbose)
    VectorOperations<DT, debug> vecops(this->_queue);
    vecops.setVectorSize(A.N());
    if (this->b.data() == nullptr) throw std::runtime_error("No right hand side to solve for");
    if (this->A.columns().get() == nullptr) throw std::runtime_error("No Matrix given");
    const auto N = A.N();
    if (x.ptr() == nullptr) {
      if constexpr (debug == Debuglevel::Verbose) std::clog << "x init empty" << std::endl;
      x.init_empty(N);
    }
    cgx_cg *s = solver();  // the solver's vectors and scalars (:276-302)
    if constexpr (debug == Debuglevel::Verbose) std::clog << "Prepared Memory" << std::endl;
    // :314-341: r = b - A x, p = r, rxr = r.r
    check(cgx_cg_begin(s, b.ptr(), x.ptr(), (double)improvement, _max_iterations), "solve");
    if constexpr (debug == Debuglevel::Verbose) {
      check(cgx_sync(_queue.native()), "solve");
      std::clog << "Init done" << std::endl;
      std::clog << "Entering Loop" << std::endl;
    }
    // :359-436: at most N + 1 bodies (or the extension's cap)
    int64_t cap = static_cast<int64_t>(N) + 1;
    if (_max_iterations >= 0) cap = std::min<int64_t>(cap, std::max<int64_t>(_max_iterations, 1));
    int64_t bodies = 0;
    int stopped = 0;
    check(cgx_cg_run(s, cap, &bodies, &stopped), "solve");
    double rxr = 0;
    check(cgx_cg_rxr(s, &rxr), "solve");  // :437-440
    _iterations = bodies;
    _final_rxr = rxr;
    this->is_solved = true;
    if constexpr (debug == Debuglevel::Verbose) {
      // :428-434: the progress line the reference writes after every body
      // whose counter is a multiple of 100, in the same order and format
      // (written here once the device loop has finished: the loop does not
      // return to the host per body)
      for (int64_t counter = 0; counter < bodies; counter += 100) {
        std::clog << "\r\033[2K";
        std::clog << ((static_cast<double>(counter) / N) * 100) << "%";
        std::flush(std::clog);
      }
      std::clog << std::endl;  // :450-453
      std::clog << "Finished solving" << std::endl;
    }
  }

  /** :463-515 — |sum (b - A x)^2 / sum x^2| (squared norms) */
  DT accuracy() {
    if constexpr (debug == Debuglevel::Verbose) std::clog << "Calculating accuracy" << std::endl;
    double out = 0;
    check(cgx_accuracy(_queue.native(), A.schedule(), b.ptr(), x.ptr(), &out), "accuracy");
    return static_cast<DT>(out);
  }

  /** :517-523 */
  std::vector<DT> extract() {
    std::vector<DT> ret(A.N());
    check(cgx_d2h(_queue.native(), ret.data(), x.ptr(), A.N() * sizeof(DT)), "extract");
    return ret;
  }

  /** :529-532 — resizes `result` to N */
  void extractTo(std::vector<DT> &result) {
    result.resize(A.N());
    check(cgx_d2h(_queue.native(), result.data(), x.ptr(), A.N() * sizeof(DT)), "extractTo");
  }

  /** :555-558 */
  std::size_t memoryFootprint() const {
    return (2 * this->A.NNZ() + (4 * this->A.N())) * sizeof(DT) +
           (2 * this->A.N() * sizeof(int));
  }

  // ---- extensions (not in the reference) -------------------------------
  /** loop bodies executed by the last solve() */
  long long iterations() const { return _iterations; }
  /** r.r after the last body (the value the reference reads back, :437-438) */
  double finalResidualSquared() const { return _final_rxr; }
  /** cap the loop bodies (< 0: the reference cap N + 1) */
  void setMaxIterations(long long m) { _max_iterations = m; }
  /**
   * None or Jacobi for the following solves (modes 1 and 3 of cgx.h; the
   * stop rule still tests the true r.r). Diagonal needs its vector: the
   * overload below.
   * @throw std::invalid_argument for Diagonal
   */
  void setPreconditioner(Preconditioner kind) {
    if (kind == Preconditioner::Diagonal)
      throw std::invalid_argument("Preconditioner::Diagonal needs its vector: "
                                  "setPreconditioner(Vector &&)");
    _precond = kind;
    _minv = Vector(_queue);
    drop_block();
    if (_solver) apply_precond(_solver.get());
  }
  /** Diagonal: minv (N positive, finite values on the device) is moved in */
  void setPreconditioner(Vector &&minv) {
    _minv = std::forward<Vector>(minv);
    _precond = Preconditioner::Diagonal;
    drop_block();
    if (_solver) apply_precond(_solver.get());
  }
  Preconditioner preconditioner() const { return _precond; }
  /**
   * Block-Jacobi preconditioning of the following solves (cgx.h
   * cgx_cg_set_block_precond: f64, modes 1 and 3): None, or Jacobi with
   * block_size rows per block (1..8). It replaces a preconditioner set by
   * setPreconditioner and is replaced by it. Given needs its values: the
   * overload below.
   * @throw std::invalid_argument for Given, or a block size outside 1..8
   */
  void setBlockPreconditioner(BlockPreconditioner kind, int block_size = 0) {
    if (kind == BlockPreconditioner::Given)
      throw std::invalid_argument("BlockPreconditioner::Given needs its values: "
                                  "setBlockPreconditioner(int, Vector &&)");
    if (kind != BlockPreconditioner::None && (block_size < 1 || block_size > 8))
      throw std::invalid_argument("setBlockPreconditioner: block_size must be 1..8");
    _blk = kind;
    _blk_bs = kind == BlockPreconditioner::None ? 0 : block_size;
    _blk_w = Vector(_queue);
    _precond = Preconditioner::None;
    _minv = Vector(_queue);
    if (_solver) apply_precond(_solver.get());
  }
  /**
   * Given: blocks (N * block_size values on the device, row i's block_size
   * values its row of its block's matrix) is moved in. Each block must be
   * symmetric positive definite: the caller's duty, only finite entries and a
   * positive diagonal are checked.
   */
  void setBlockPreconditioner(int block_size, Vector &&blocks) {
    if (block_size < 1 || block_size > 8)
      throw std::invalid_argument("setBlockPreconditioner: block_size must be 1..8");
    _blk_w = std::forward<Vector>(blocks);
    _blk = BlockPreconditioner::Given;
    _blk_bs = block_size;
    _precond = Preconditioner::None;
    _minv = Vector(_queue);
    if (_solver) apply_precond(_solver.get());
  }
  BlockPreconditioner blockPreconditioner() const { return _blk; }
  int blockSize() const { return _blk_bs; }
  /**
   * Batched solve (cgx_cg_solve_batch of cgx.h): B.size() = k independent
   * right-hand sides, 1 <= k <= 8, on the matrix in place. X[c] holds column
   * c's initial guess on entry (an unallocated Vector: zero) and its solution
   * on return. The vectors are copied to and from column-major device
   * storage. Every column is the single solve's in mode 1, bit for bit, where
   * the fused form runs (setBatchForm: 0 auto, 1 fused, 2 sequential).
   * @throw std::invalid_argument for k outside 1..8, X.size() != k or a
   *        vector whose length is not N
   */
  void solveBatch(const std::vector<Vector> &B, std::vector<Vector> &X,
                  DT improvement = static_cast<DT>(0)) {
    const std::size_t k = B.size(), n = static_cast<std::size_t>(A.N());
    if (k < 1 || k > 8) throw std::invalid_argument("solveBatch: 1 to 8 right-hand sides");
    if (X.size() != k) throw std::invalid_argument("solveBatch: X.size() != B.size()");
    if (this->A.columns().get() == nullptr) throw std::runtime_error("No Matrix given");
    for (std::size_t c = 0; c < k; ++c) {
      Vector &bc = const_cast<Vector &>(B[c]);  // the accessors are not const
      if (X[c].ptr() == nullptr) X[c].init_empty(n);
      if (bc.ptr() == nullptr || static_cast<std::size_t>(bc.N()) != n ||
          static_cast<std::size_t>(X[c].N()) != n)
        throw std::invalid_argument("solveBatch: a vector's length is not N");
    }
    Vector Bd(_queue, n * k), Xd(_queue, n * k);
    for (std::size_t c = 0; c < k; ++c) {
      Vector &bc = const_cast<Vector &>(B[c]);
      check(cgx_d2d(_queue.native(), Bd.ptr() + c * n, bc.ptr(), n * sizeof(DT)), "solveBatch");
      check(cgx_d2d(_queue.native(), Xd.ptr() + c * n, X[c].ptr(), n * sizeof(DT)), "solveBatch");
    }
    cgx_cg *s = solver();
    check(cgx_cg_set_batch_form(s, _batch_form), "setBatchForm");
    std::vector<int64_t> bodies(k);
    std::vector<double> rxr(k);
    std::vector<int> stopped(k);
    check(cgx_cg_solve_batch(s, static_cast<int>(k), Bd.ptr(), static_cast<int64_t>(n), Xd.ptr(),
                             static_cast<int64_t>(n), (double)improvement, _max_iterations,
                             bodies.data(), rxr.data(), stopped.data()),
          "solveBatch");
    for (std::size_t c = 0; c < k; ++c)
      check(cgx_d2d(_queue.native(), X[c].ptr(), Xd.ptr() + c * n, n * sizeof(DT)), "solveBatch");
    check(cgx_sync(_queue.native()), "solveBatch");
    _batch_iterations.assign(bodies.begin(), bodies.end());
    _batch_rxr = rxr;
    _batch_stopped = stopped;
  }
  /** 0 auto, 1 fused, 2 sequential (cgx_cg_set_batch_form) */
  void setBatchForm(int form) { _batch_form = form; }
  /** per column of the last solveBatch: loop bodies, r.r after the last body, stop code */
  const std::vector<long long> &batchIterations() const { return _batch_iterations; }
  const std::vector<double> &batchFinalResidualSquared() const { return _batch_rxr; }
  const std::vector<int> &batchStopped() const { return _batch_stopped; }

  /**
   * Multi-shift solve (cgx_cg_solve_shifted of cgx.h): (A + sigma[s] I) x_s = b
   * for 1 to 8 shifts sigma[s] >= 0 on the matrix and the right-hand side
   * (setTarget) in place, every x_s from zero, all from one Krylov space. X is
   * resized to sigma.size() vectors of N and receives the solutions (copied
   * from column-major device storage). A sigma = 0 column is the single solve
   * in mode 1 from a zero initial guess, bit for bit. f64 without a
   * preconditioner (else the cgx error is thrown).
   * @throw std::invalid_argument for a shift count outside 1..8 or a shift
   *        that is negative or not finite
   */
  void solveShifted(const std::vector<DT> &sigma, std::vector<Vector> &X,
                    DT improvement = static_cast<DT>(0)) {
    const std::size_t k = sigma.size(), n = static_cast<std::size_t>(A.N());
    if (k < 1 || k > 8) throw std::invalid_argument("solveShifted: 1 to 8 shifts");
    std::vector<double> sg(k);
    for (std::size_t c = 0; c < k; ++c) {
      sg[c] = static_cast<double>(sigma[c]);
      if (!(sg[c] >= 0.0) || sg[c] > std::numeric_limits<double>::max())
        throw std::invalid_argument("solveShifted: a shift is finite and not negative");
    }
    if (this->b.data() == nullptr) throw std::runtime_error("No right hand side to solve for");
    if (this->A.columns().get() == nullptr) throw std::runtime_error("No Matrix given");
    Vector Xd(_queue, n * k);
    cgx_cg *s = solver();
    std::vector<int64_t> bodies(k);
    std::vector<double> res(k);
    std::vector<int> stopped(k);
    check(cgx_cg_solve_shifted(s, static_cast<int>(k), sg.data(), b.ptr(), Xd.ptr(),
                               static_cast<int64_t>(n), (double)improvement, _max_iterations,
                               bodies.data(), res.data(), stopped.data()),
          "solveShifted");
    X.clear();
    for (std::size_t c = 0; c < k; ++c) {
      X.emplace_back(_queue);
      X[c].init_empty(n);
      check(cgx_d2d(_queue.native(), X[c].ptr(), Xd.ptr() + c * n, n * sizeof(DT)), "solveShifted");
    }
    check(cgx_sync(_queue.native()), "solveShifted");
    _shifted_iterations.assign(bodies.begin(), bodies.end());
    _shifted_res = res;
    _shifted_stopped = stopped;
  }
  /** per shift of the last solveShifted: loop bodies, |zeta_s| ||r|| after the
   * shift's last body, stop code (1 frozen by the rule, 2 cap reached) */
  const std::vector<long long> &shiftedIterations() const { return _shifted_iterations; }
  const std::vector<double> &shiftedResidual() const { return _shifted_res; }
  const std::vector<int> &shiftedStopped() const { return _shifted_stopped; }

  /** one residual evaluation of solveMixed (cgx_mixed_history) */
  struct MixedRecord {
    double rr;               ///< the f64 true r.r
    long long inner_bodies;  ///< bodies of the inner solve before it (0 for the first)
    double inner_rxr;        ///< that solve's final f32 r.r (of the scaled system)
  };
  /**
   * Mixed-precision solve (cgx_mixed_solve of cgx.h; CG<double> only): A x = b
   * to `improvement` on the true f64 residual, the loop bodies run by the f32
   * solver on a cast copy of the matrix (iterative refinement). The
   * preconditioner set here applies inside (a Diagonal vector is cast to
   * f32), setMixedInnerMode picks the inner solver's mode, setMaxIterations
   * caps the inner bodies of the whole call. inner_reduction, max_outer and
   * inner_cap: 0 keeps the default (1e-5, 8, N + 1). Sets iterations() (inner
   * bodies), outerSteps(), finalResidualSquared() (the last true r.r),
   * mixedStatus() (1 tolerance reached, 2 cap, 3 stagnated, 4 NaN) and
   * mixedHistory(). With `fallback` a status 3 or 4 continues with the
   * ordinary solve() from the current x; its bodies are added to iterations()
   * and mixedStatus() keeps the 3 or 4.
   * @throw std::invalid_argument for a negative or non-finite knob
   * @throw std::runtime_error if b or A is missing
   */
  void solveMixed(DT improvement = static_cast<DT>(0), double inner_reduction = 0,
                  int max_outer = 0, long long inner_cap = 0, bool fallback = true) {
    static_assert(std::is_same<DT, double>::value, "solveMixed refines a double system");
    if (!(inner_reduction >= 0) || inner_reduction > std::numeric_limits<double>::max())
      throw std::invalid_argument("solveMixed: inner_reduction must be finite and not negative");
    if (max_outer < 0) throw std::invalid_argument("solveMixed: max_outer must not be negative");
    if (inner_cap < 0) throw std::invalid_argument("solveMixed: inner_cap must not be negative");
    if (this->b.data() == nullptr) throw std::runtime_error("No right hand side to solve for");
    if (this->A.columns().get() == nullptr) throw std::runtime_error("No Matrix given");
    if (x.ptr() == nullptr) x.init_empty(A.N());
    cgx_csr *sched = A.schedule();
    if (!_mixed || _mixed_for != sched) {
      cgx_mixed *m = nullptr;
      check(cgx_mixed_create(_queue.native(), sched, &m), "cgx_mixed_create");
      _mixed = std::shared_ptr<cgx_mixed>(m, detail::MixedDeleter());
      _mixed_for = sched;
      _mixed_set = false;
    }
    cgx_mixed *m = _mixed.get();
    if (_blk != BlockPreconditioner::None) {
      // refused, whatever the kind: the inner solver is f32 (CGX_EUNSUPPORTED)
      cgx_cg *inner = nullptr;
      check(cgx_mixed_inner(m, nullptr, &inner), "solveMixed");
      check(cgx_cg_set_block_precond(inner, CGX_BLOCK_JACOBI, _blk_bs, nullptr),
            "setBlockPreconditioner");
    }
    if (!_mixed_set || _mixed_mode_set != _mixed_mode || _mixed_precond_set != _precond ||
        _mixed_minv_set != _minv.ptr()) {
      // mode before the preconditioner, and None first: whichever of the two
      // comes second refuses a mode that runs no preconditioner
      _mixed_set = false;
      check(cgx_mixed_set_precond(m, CGX_PRECOND_NONE, nullptr), "solveMixed");
      check(cgx_mixed_set_mode(m, _mixed_mode), "setMixedInnerMode");
      if (_precond != Preconditioner::None) {
        if (_precond == Preconditioner::Diagonal &&
            static_cast<std::size_t>(_minv.N()) != static_cast<std::size_t>(A.N()))
          throw std::invalid_argument("setPreconditioner: the diagonal's length is not N");
        check(cgx_mixed_set_precond(m, static_cast<int>(_precond),
                                    _precond == Preconditioner::Diagonal ? _minv.ptr() : nullptr),
              "setPreconditioner");
      }
      _mixed_set = true;
      _mixed_mode_set = _mixed_mode;
      _mixed_precond_set = _precond;
      _mixed_minv_set = _minv.ptr();
    }
    check(cgx_mixed_config(m, inner_reduction, max_outer, inner_cap), "solveMixed");
    int outer = 0, status = 0;
    int64_t bodies = 0;
    double rxr = 0;
    check(cgx_mixed_solve(m, b.ptr(), x.ptr(), (double)improvement, _max_iterations, &outer,
                          &bodies, &rxr, &status),
          "solveMixed");
    int count = 0;
    check(cgx_mixed_history(m, nullptr, nullptr, nullptr, 0, &count), "solveMixed");
    std::vector<double> rr(count), irxr(count);
    std::vector<int64_t> ib(count);
    check(cgx_mixed_history(m, rr.data(), ib.data(), irxr.data(), count, &count), "solveMixed");
    _mixed_history.clear();
    for (int i = 0; i < count; ++i) _mixed_history.push_back({rr[i], (long long)ib[i], irxr[i]});
    _iterations = bodies;
    _final_rxr = rxr;
    _outer_steps = outer;
    _mixed_status = status;
    this->is_solved = true;
    if (fallback && (status == 3 || status == 4)) {
      solve(improvement);
      _iterations += bodies;
    }
  }
  /** the inner f32 solver's mode (cgx_cg_set_mode; 0 auto) for the following solveMixed */
  void setMixedInnerMode(int mode) { _mixed_mode = mode; }
  int outerSteps() const { return _outer_steps; }
  int mixedStatus() const { return _mixed_status; }
  const std::vector<MixedRecord> &mixedHistory() const { return _mixed_history; }
  /** the cgx_mixed handle of the last solveMixed (null before one): cgx_mixed_inner, cgx_mixed_bytes */
  cgx_mixed *mixedHandle() const { return _mixed.get(); }

 private:
  void executeQueue() {
    try {
      this->_queue.wait_and_throw();
    } catch (asycl::exception &e) {
      std::cerr << "Caught Sycl Exception " << e.what() << std::endl;
      throw e;
    } catch (std::exception &e) {
      std::cerr << "Caught Exception " << e.what() << std::endl;
      throw e;
    }
  }

  static void check(int rc, const char *what) { asycl::detail::check(rc, what); }

  cgx_cg *solver() {
    cgx_csr *sched = A.schedule();
    if (!_solver || _solver_for != sched) {
      cgx_cg *c = nullptr;
      check(cgx_cg_create(_queue.native(), sched, &c), "cgx_cg_create");
      _solver = std::shared_ptr<cgx_cg>(c, detail::CgDeleter());
      _solver_for = sched;
      // the choice survives a setMatrix (Jacobi is rebuilt from the new matrix)
      if (_precond != Preconditioner::None || _blk != BlockPreconditioner::None)
        apply_precond(c);
    }
    return _solver.get();
  }

  void drop_block() {  // a diagonal preconditioner replaces a block one
    _blk = BlockPreconditioner::None;
    _blk_bs = 0;
    _blk_w = Vector(_queue);
  }

  void apply_precond(cgx_cg *c) {
    if (_blk != BlockPreconditioner::None) {
      const bool given = _blk == BlockPreconditioner::Given;
      if (given && static_cast<std::size_t>(_blk_w.N()) !=
                       static_cast<std::size_t>(A.N()) * static_cast<std::size_t>(_blk_bs))
        throw std::invalid_argument("setBlockPreconditioner: the blocks' length is not "
                                    "N * block_size");
      check(cgx_cg_set_block_precond(c, static_cast<int>(_blk), _blk_bs,
                                     given ? _blk_w.ptr() : nullptr),
            "setBlockPreconditioner");
      return;
    }
    if (_precond == Preconditioner::Diagonal &&
        static_cast<std::size_t>(_minv.N()) != static_cast<std::size_t>(A.N()))
      throw std::invalid_argument("setPreconditioner: the diagonal's length is not N");
    check(cgx_cg_set_precond(c, static_cast<int>(_precond),
                             _precond == Preconditioner::Diagonal ? _minv.ptr() : nullptr),
          "setPreconditioner");
  }

  asycl::queue _queue;
  bool is_solved = false;
  Matrix A;
  Vector x;
  Vector b;
  std::shared_ptr<cgx_cg> _solver;
  cgx_csr *_solver_for = nullptr;
  long long _iterations = 0;
  double _final_rxr = 0;
  long long _max_iterations = -1;
  Preconditioner _precond = Preconditioner::None;
  Vector _minv{_queue};
  BlockPreconditioner _blk = BlockPreconditioner::None;
  int _blk_bs = 0;
  Vector _blk_w{_queue};
  int _batch_form = 0;
  std::vector<long long> _batch_iterations;
  std::vector<double> _batch_rxr;
  std::vector<int> _batch_stopped;
  std::vector<long long> _shifted_iterations;
  std::vector<double> _shifted_res;
  std::vector<int> _shifted_stopped;
  std::shared_ptr<cgx_mixed> _mixed;
  cgx_csr *_mixed_for = nullptr;
  // what the inner solver was last given (setting either drops its captured graphs)
  bool _mixed_set = false;
  int _mixed_mode = 0, _mixed_mode_set = 0;
  Preconditioner _mixed_precond_set = Preconditioner::None;
  const void *_mixed_minv_set = nullptr;
  int _outer_steps = 0, _mixed_status = 0;
  std::vector<MixedRecord> _mixed_history;
};

};  // namespace CGSolver

#endif /*CG_HPP */
