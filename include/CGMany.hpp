/*
 * CGMany.hpp — many small SPD systems on one sparsity pattern, each solved by
 * one workgroup that runs the whole CG loop (cgx.h "cgx_many").
 *
 * An extension: the reference solves one system. A thin C++ layer over the C
 * ABI in the style of the drop-in CG.hpp; double only (CGMany<float> does not
 * compile). Every system's result is the single solve's in mode 1, bit for
 * bit (cgx.h), plain, under setPreconditioner's Jacobi / diagonal or under
 * setBlockPreconditioner's dense diagonal blocks.
 */
#ifndef CGSOLVER_CGMANY_HPP
#define CGSOLVER_CGMANY_HPP

#include <cstdint>
#include <memory>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "LinearAlgebraTypes.hpp"

namespace CGSolver {

namespace detail {
struct ManyDeleter {
  void operator()(cgx_many *m) const {
    if (m) cgx_many_destroy(m);
  }
};
}  // namespace detail

template <typename DT> class CGMany {
  static_assert(std::is_same<DT, double>::value, "CGMany solves double systems");

 public:
  /**
   * rows (n + 1) and columns (nnz): the shared CSR pattern; values: nsys * nnz,
   * system s at values[s * nnz ...]. 1 <= n <= 4096.
   * @throw std::invalid_argument for sizes that do not fit
   */
  CGMany(acpp::sycl::queue &queue, const std::vector<int> &rows, const std::vector<int> &columns,
         const std::vector<DT> &values)
      : _queue(queue) {
    if (rows.size() < 2) throw std::invalid_argument("CGMany: rows needs n + 1 >= 2 entries");
    _n = (int64_t)rows.size() - 1;
    _nnz = (int64_t)columns.size();
    if (_nnz == 0 || values.size() % columns.size() != 0 || values.empty())
      throw std::invalid_argument("CGMany: values must hold nsys * nnz entries");
    _nsys = (int64_t)(values.size() / columns.size());
    _rows = alloc(rows.size() * sizeof(int));
    _cols = alloc(columns.size() * sizeof(int));
    _vals = alloc(values.size() * sizeof(DT));
    check(cgx_h2d(_queue.native(), _rows.get(), rows.data(), rows.size() * sizeof(int)), "CGMany");
    check(cgx_h2d(_queue.native(), _cols.get(), columns.data(), columns.size() * sizeof(int)),
          "CGMany");
    check(cgx_h2d(_queue.native(), _vals.get(), values.data(), values.size() * sizeof(DT)),
          "CGMany");
    cgx_many *m = nullptr;
    check(cgx_many_create(_queue.native(), CGX_F64, _nsys, _n, _nnz, (const int32_t *)_rows.get(),
                          (const int32_t *)_cols.get(), _vals.get(), _nnz, &m),
          "cgx_many_create");
    _many = std::shared_ptr<cgx_many>(m, detail::ManyDeleter());
  }

  int64_t systems() const { return _nsys; }
  int64_t dimension() const { return _n; }

  /** cap the grid (0: the resident workgroups); a tuning knob */
  void setMaxWorkgroups(int g) { check(cgx_many_config(_many.get(), g), "cgx_many_config"); }
  /** cap the bodies of each solve (-1: n + 1) */
  void setMaxIterations(long long m) { _max_iterations = m; }

  /** overwrite every system's values in place; the next solve reads them */
  void setValues(const std::vector<DT> &values) {
    if ((int64_t)values.size() != _nsys * _nnz)
      throw std::invalid_argument("CGMany::setValues: values must hold nsys * nnz entries");
    check(cgx_h2d(_queue.native(), _vals.get(), values.data(), values.size() * sizeof(DT)),
          "setValues");
  }

  /**
   * The next solves' preconditioner (cgx_many_set_precond): kind is
   * CGX_PRECOND_NONE, CGX_PRECOND_JACOBI (1 / a_ii, formed in the kernel from
   * the values each solve reads) or CGX_PRECOND_DIAGONAL with *diag, nsys * n
   * host values, system s's m at diag[s * n ...]. A system whose diagonal or m
   * is not positive and finite stops alone with code 3, its X untouched.
   * @throw std::invalid_argument for an unknown kind, a missing diag or a wrong length
   */
  void setPreconditioner(int kind, const std::vector<DT> *diag = nullptr) {
    if (kind != CGX_PRECOND_NONE && kind != CGX_PRECOND_JACOBI && kind != CGX_PRECOND_DIAGONAL)
      throw std::invalid_argument("CGMany::setPreconditioner: unknown kind");
    std::shared_ptr<void> d;
    if (kind == CGX_PRECOND_DIAGONAL) {
      if (!diag || (int64_t)diag->size() != _nsys * _n)
        throw std::invalid_argument("CGMany::setPreconditioner: diag must hold nsys * n entries");
      d = alloc(diag->size() * sizeof(DT));
      check(cgx_h2d(_queue.native(), d.get(), diag->data(), diag->size() * sizeof(DT)),
            "setPreconditioner");
    }
    check(cgx_many_set_precond(_many.get(), kind, d.get(), _n), "cgx_many_set_precond");
    _diag = d;
    _precond = kind;
    _blocks.reset();  // (replaced)
    _block = CGX_BLOCK_NONE;
    _final_rz.clear();
  }
  int preconditioner() const { return _precond; }

  /**
   * The next solves' block preconditioner (cgx_many_set_block_precond): kind
   * is CGX_BLOCK_NONE, CGX_BLOCK_JACOBI (the inverses of every system's
   * diagonal blocks of bs rows, 1..8, formed on the device at every solve from
   * the values that solve reads) or CGX_BLOCK_GIVEN with *blocks, nsys * n * bs
   * host values: system s's W, n x bs row-major, at blocks[s * n * bs ...], each
   * block symmetric positive definite (the caller's duty). A system with a bad
   * block stops alone with code 3, its X untouched. It replaces
   * setPreconditioner's and is replaced by it.
   * @throw std::invalid_argument for an unknown kind, bs outside 1..8, missing
   *        blocks or a wrong length
   */
  void setBlockPreconditioner(int kind, int bs, const std::vector<DT> *blocks = nullptr) {
    if (kind != CGX_BLOCK_NONE && kind != CGX_BLOCK_JACOBI && kind != CGX_BLOCK_GIVEN)
      throw std::invalid_argument("CGMany::setBlockPreconditioner: unknown kind");
    if (kind != CGX_BLOCK_NONE && (bs < 1 || bs > 8))
      throw std::invalid_argument("CGMany::setBlockPreconditioner: bs must be 1..8");
    std::shared_ptr<void> w;
    if (kind == CGX_BLOCK_GIVEN) {
      if (!blocks || (int64_t)blocks->size() != _nsys * _n * bs)
        throw std::invalid_argument(
            "CGMany::setBlockPreconditioner: blocks must hold nsys * n * bs entries");
      w = alloc(blocks->size() * sizeof(DT));
      check(cgx_h2d(_queue.native(), w.get(), blocks->data(), blocks->size() * sizeof(DT)),
            "setBlockPreconditioner");
    }
    check(cgx_many_set_block_precond(_many.get(), kind, bs, w.get(), _n * bs),
          "cgx_many_set_block_precond");
    _blocks = w;
    _block = kind;
    _diag.reset();  // (replaced)
    _precond = CGX_PRECOND_NONE;
    _final_rz.clear();
  }
  int blockPreconditioner() const { return _block; }

  /**
   * The inverses of every system's diagonal blocks of bs rows as
   * CGX_BLOCK_JACOBI forms them from the current values (cgx_many_block_inv):
   * nsys * n * bs values, system s's W at [s * n * bs ...]. *badSystems, when
   * given, receives the number of systems with a pivot that is not positive
   * and finite.
   * @throw std::invalid_argument for bs outside 1..8
   */
  std::vector<DT> blockInverse(int bs, int64_t *badSystems = nullptr) {
    if (bs < 1 || bs > 8) throw std::invalid_argument("CGMany::blockInverse: bs must be 1..8");
    const size_t len = (size_t)(_nsys * _n * bs);
    auto w = alloc(len * sizeof(DT));
    int64_t nbad = 0;
    check(cgx_many_block_inv(_many.get(), bs, w.get(), _n * bs, &nbad, nullptr),
          "cgx_many_block_inv");
    std::vector<DT> out(len);
    check(cgx_d2h(_queue.native(), out.data(), w.get(), len * sizeof(DT)), "blockInverse");
    if (badSystems) *badSystems = nbad;
    return out;
  }

  /**
   * The next solves' kernel form (cgx_many_set_form): CGX_MANY_FORM_AUTO (the
   * default), CGX_MANY_FORM_WORKGROUP or CGX_MANY_FORM_WAVE, a wave per system
   * for n <= 256.
   * @throw std::invalid_argument for an unknown form; std::runtime_error from
   *        the library for the wave form above 256 rows
   */
  void setForm(int form) {
    if (form != CGX_MANY_FORM_AUTO && form != CGX_MANY_FORM_WORKGROUP &&
        form != CGX_MANY_FORM_WAVE)
      throw std::invalid_argument("CGMany::setForm: unknown form");
    check(cgx_many_set_form(_many.get(), form), "cgx_many_set_form");
  }
  /** the form the next solve launches: CGX_MANY_FORM_WORKGROUP or CGX_MANY_FORM_WAVE */
  int form() const {
    int in_effect = 0;
    check(cgx_many_get_form(_many.get(), nullptr, &in_effect), "cgx_many_get_form");
    return in_effect;
  }

  /**
   * B and X: nsys * n host values, system-major; X holds the initial guesses
   * and receives the results. improvement: the absolute tolerance on sqrt(r.r).
   * @throw std::invalid_argument for a wrong length
   */
  void solve(const std::vector<DT> &B, std::vector<DT> &X, DT improvement = static_cast<DT>(0)) {
    const size_t len = (size_t)(_nsys * _n);
    if (B.size() != len || X.size() != len)
      throw std::invalid_argument("CGMany::solve: B and X must hold nsys * n entries");
    auto dB = alloc(len * sizeof(DT)), dX = alloc(len * sizeof(DT));
    check(cgx_h2d(_queue.native(), dB.get(), B.data(), len * sizeof(DT)), "solve");
    check(cgx_h2d(_queue.native(), dX.get(), X.data(), len * sizeof(DT)), "solve");
    _iterations.assign((size_t)_nsys, 0);
    _final_rxr.assign((size_t)_nsys, 0.0);
    _stopped.assign((size_t)_nsys, 0);
    check(cgx_many_solve(_many.get(), dB.get(), _n, dX.get(), _n, (double)improvement,
                         _max_iterations, _iterations.data(), _final_rxr.data(), _stopped.data()),
          "cgx_many_solve");
    _final_rz.clear();
    if (_precond != CGX_PRECOND_NONE || _block != CGX_BLOCK_NONE) {
      _final_rz.assign((size_t)_nsys, 0.0);
      check(cgx_many_rz(_many.get(), _final_rz.data()), "cgx_many_rz");
    }
    check(cgx_d2h(_queue.native(), X.data(), dX.get(), len * sizeof(DT)), "solve");
  }

  /** per system: loop bodies, r.r after the last body, stop code (1 rule or NaN, 2 cap,
   *  3 a bad diagonal under a preconditioner); finalRz: r.z after the last body (empty
   *  without a preconditioner) */
  const std::vector<int64_t> &iterations() const { return _iterations; }
  const std::vector<double> &finalResidualSquared() const { return _final_rxr; }
  const std::vector<double> &finalRz() const { return _final_rz; }
  const std::vector<int> &stopped() const { return _stopped; }
  cgx_many *handle() const { return _many.get(); }

 private:
  static void check(int rc, const char *what) { acpp::sycl::detail::check(rc, what); }
  std::shared_ptr<void> alloc(size_t bytes) {
    void *p = nullptr;
    check(cgx_alloc(_queue.native(), bytes, &p), "cgx_alloc");
    cgx_ctx *ctx = _queue.native();
    return std::shared_ptr<void>(p, [ctx](void *q) { cgx_free(ctx, q); });
  }

  acpp::sycl::queue _queue;
  int64_t _nsys = 0, _n = 0, _nnz = 0;
  long long _max_iterations = -1;
  std::shared_ptr<void> _rows, _cols, _vals, _diag, _blocks;
  int _precond = CGX_PRECOND_NONE, _block = CGX_BLOCK_NONE;
  std::shared_ptr<cgx_many> _many;
  std::vector<int64_t> _iterations;
  std::vector<double> _final_rxr, _final_rz;
  std::vector<int> _stopped;
};

}  // namespace CGSolver
#endif /* CGSOLVER_CGMANY_HPP */
