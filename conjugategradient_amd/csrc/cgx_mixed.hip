// cgx_mixed.hip — mixed-precision solve (cgx.h "cgx_mixed"):
// an f64 system solved to an f64 tolerance on the true residual, the bodies
// run by the f32 solver on a cast copy of the matrix. Iterative refinement:
// per outer step one f64 SpMV (cgx_spmv on A) and three streaming kernels
// here (residual with r.r, down-scale, up-add), then an f32 cgx_cg_solve on
// the scaled residual. The kernels follow the update kernels' idiom
// (cgx_kernels.hip): 16-byte lanes, a scalar tail, no scratch, the dot a
// double-length sum (cgx_dd.h) whose per-workgroup partials a following
// launch adds in a fixed order.
#include <cmath>
#include <cstring>
#include <limits>

#include "cgx_dd.h"
#include "cgx_objects.h"

using namespace cgx;

namespace {

struct DeviceGuard {
  explicit DeviceGuard(int dev) { (void)hipSetDevice(dev); }
};

// ---- kernels ----------------------------------------------------------------
// Workgroup sum of one pair per thread in a fixed order (waves, then wave 0
// to 3); valid in thread 0. lds: 8 doubles.
__device__ __forceinline__ Dd<double> mx_block_sum(Dd<double> v, double *lds) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  v = wave_sum_dd(v);
  if (lane == 0) {
    lds[2 * w] = v.hi;
    lds[2 * w + 1] = v.lo;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    v = Dd<double>(lds[0], lds[1]);
#pragma unroll
    for (int k = 1; k < kBlock / 64; ++k) v += Dd<double>(lds[2 * k], lds[2 * k + 1]);
  }
  __syncthreads();
  return v;
}

// out[k] = (float)in[k], round to nearest even. CHECK: bad[0] counts the
// values that cast to +-inf and the non-zero values that cast to 0, bad[1] is
// the lowest such index (the caller presets {0, ~0}). Two double2 loads per
// float4 store; the last n & 3 elements one by one.
template <bool CHECK>
__global__ __launch_bounds__(kBlock) void k_mixed_cast(int64_t n, const double *__restrict__ in,
                                                       float *__restrict__ out,
                                                       unsigned long long *bad) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const double2 *in2 = reinterpret_cast<const double2 *>(in);
  float4 *o4 = reinterpret_cast<float4 *>(out);
  unsigned long long cnt = 0, first = ~0ull;
  auto chk = [&](double d, float f, int64_t k) {
    if (CHECK && (isinf(f) || (f == 0.0f && d != 0.0))) {
      ++cnt;
      if ((unsigned long long)k < first) first = (unsigned long long)k;
    }
  };
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += stride) {
    const double2 a = in2[2 * i], b = in2[2 * i + 1];
    float4 f;
    f.x = (float)a.x;
    f.y = (float)a.y;
    f.z = (float)b.x;
    f.w = (float)b.y;
    o4[i] = f;
    chk(a.x, f.x, 4 * i);
    chk(a.y, f.y, 4 * i + 1);
    chk(b.x, f.z, 4 * i + 2);
    chk(b.y, f.w, 4 * i + 3);
  }
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < (n & 3)) {
    const int64_t k = 4 * n4 + threadIdx.x;
    const double d = in[k];
    const float f = (float)d;
    out[k] = f;
    chk(d, f, k);
  }
  if (CHECK && cnt) {
    atomicAdd(&bad[0], cnt);
    atomicMin(&bad[1], first);
  }
}

// r = b - Ax and this workgroup's share of r.r (each product rounded, then a
// double-length sum) at part[2 blockIdx.x ..]; k_mixed_rr adds the shares.
__global__ __launch_bounds__(kBlock) void k_mixed_resid(int64_t n, const double *__restrict__ b,
                                                        const double *__restrict__ Ax,
                                                        double *__restrict__ r,
                                                        double *__restrict__ part) {
  __shared__ double red[8];
  const int64_t n2 = n >> 1;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const double2 *b2 = reinterpret_cast<const double2 *>(b);
  const double2 *a2 = reinterpret_cast<const double2 *>(Ax);
  double2 *r2 = reinterpret_cast<double2 *>(r);
  Dd<double> acc(0.0);
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n2; i += stride) {
    const double2 bv = b2[i], av = a2[i];
    double2 rv;
    rv.x = bv.x - av.x;
    rv.y = bv.y - av.y;
    r2[i] = rv;
    acc += rv.x * rv.x;
    acc += rv.y * rv.y;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double v = b[n - 1] - Ax[n - 1];
    r[n - 1] = v;
    acc += v * v;
  }
  const Dd<double> v = mx_block_sum(acc, red);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = v.hi;
    part[2 * blockIdx.x + 1] = v.lo;
  }
}

// *out = the sum of the np shares (thread t: t, t + 256, ...; then the
// workgroup), rounded once. One workgroup.
__global__ __launch_bounds__(kBlock) void k_mixed_rr(const double *__restrict__ part, int np,
                                                     double *__restrict__ out) {
  __shared__ double red[8];
  Dd<double> v(0.0);
  for (int i = threadIdx.x; i < np; i += kBlock) v += Dd<double>(part[2 * i], part[2 * i + 1]);
  v = mx_block_sum(v, red);
  if (threadIdx.x == 0) out[0] = v.value();
}

// r32 = (float)(r s), s a power of two (the product is exact, the cast the
// one rounding), and d32 = 0: the inner solve's right-hand side and its
// initial guess. Two double2 loads per float4 store.
__global__ __launch_bounds__(kBlock) void k_mixed_down(int64_t n, const double *__restrict__ r,
                                                       double s, float *__restrict__ r32,
                                                       float *__restrict__ d32) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const double2 *r2 = reinterpret_cast<const double2 *>(r);
  float4 *o4 = reinterpret_cast<float4 *>(r32);
  float4 *d4 = reinterpret_cast<float4 *>(d32);
  const float4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += stride) {
    const double2 a = r2[2 * i], b = r2[2 * i + 1];
    float4 f;
    f.x = (float)(a.x * s);
    f.y = (float)(a.y * s);
    f.z = (float)(b.x * s);
    f.w = (float)(b.y * s);
    o4[i] = f;
    d4[i] = zero;
  }
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < (n & 3)) {
    const int64_t k = 4 * n4 + threadIdx.x;
    r32[k] = (float)(r[k] * s);
    d32[k] = 0.0f;
  }
}

// x += (double)d32 sinv, sinv a power of two (product exact, one add).
__global__ __launch_bounds__(kBlock) void k_mixed_up(int64_t n, double *__restrict__ x,
                                                     const float *__restrict__ d32, double sinv) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  double2 *x2 = reinterpret_cast<double2 *>(x);
  const float4 *d4 = reinterpret_cast<const float4 *>(d32);
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += stride) {
    const float4 d = d4[i];
    double2 a = x2[2 * i], b = x2[2 * i + 1];
    a.x = a.x + (double)d.x * sinv;
    a.y = a.y + (double)d.y * sinv;
    b.x = b.x + (double)d.z * sinv;
    b.y = b.y + (double)d.w * sinv;
    x2[2 * i] = a;
    x2[2 * i + 1] = b;
  }
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < (n & 3)) {
    const int64_t k = 4 * n4 + threadIdx.x;
    x[k] = x[k] + (double)d32[k] * sinv;
  }
}

// workgroups of a launch whose threads take `lanes` 16- or 32-byte lanes
int mx_grid(int64_t lanes) {
  const int64_t g = (lanes + kBlock - 1) / kBlock;
  return (int)std::min<int64_t>(std::max<int64_t>(g, 1), kMaxGrid);
}

struct Record {
  double rr;
  int64_t inner_bodies;
  double inner_rxr;
};

size_t alloc_bytes(const void *p) {
  size_t b = 0;
  if (!p || hipMemPtrGetInfo(const_cast<void *>(p), &b) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return b;
}

}  // namespace

struct cgx_mixed {
  cgx_ctx *ctx = nullptr;
  cgx_csr *A = nullptr;     // the caller's f64 matrix (retained)
  cgx_csr *A32 = nullptr;   // its f32 copy: val32 on A's rowptr and col
  cgx_cg *cg32 = nullptr;   // the inner solver
  int64_t n = 0, nnz = 0;
  float *val32 = nullptr;
  double *r = nullptr, *Ax = nullptr;  // n + 2 (slack: 16-byte lanes)
  float *r32 = nullptr, *d32 = nullptr;  // n + 4
  float *m32 = nullptr;                // the f32 copy of a caller's diagonal
  double *part = nullptr;              // 2 kMaxGrid shares of r.r, then its value
  double *h_rr = nullptr;              // pinned
  unsigned long long *bad = nullptr;   // the cast's count and first index
  double inner_reduction = 1e-5;
  int max_outer = 8;
  int64_t inner_cap = -1;
  std::vector<Record> history;
};

namespace {

void mixed_free(cgx_mixed *m) {
  if (!m) return;
  if (m->cg32) (void)cgx_cg_destroy(m->cg32);
  if (m->A32) (void)cgx_csr_destroy(m->A32);
  void *dev[] = {m->val32, m->r, m->Ax, m->r32, m->d32, m->m32, m->part, m->bad};
  for (void *p : dev)
    if (p) (void)hipFree(p);
  if (m->h_rr) (void)hipHostFree(m->h_rr);
  if (m->A) csr_release(m->A);
  if (m->ctx) ctx_release(m->ctx);
  delete m;
}

}  // namespace

extern "C" int cgx_mixed_create(cgx_ctx *ctx, cgx_csr *A, cgx_mixed **out) {
  CGX_REQUIRE(ctx && A && out, CGX_EINVAL, "NULL argument");
  *out = nullptr;
  CGX_REQUIRE(A->ctx == ctx, CGX_EINVAL, "matrix belongs to another context");
  CGX_REQUIRE(!A->dist, CGX_EUNSUPPORTED,
              "cgx_mixed_create: the matrix is partitioned (cgx_csr_create_dist); the mixed "
              "solve runs on one device");
  CGX_REQUIRE(A->dtype == CGX_F64, CGX_EINVAL,
              "cgx_mixed_create: the matrix is f32; the mixed solve refines an f64 system");
  CGX_REQUIRE(((uintptr_t)A->dev.val & 15) == 0, CGX_EINVAL,
              "cgx_mixed_create: the matrix values must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  auto *m = new cgx_mixed();
  m->ctx = ctx;
  m->A = A;
  ctx_retain(ctx);
  csr_retain(A);
  const int64_t n = m->n = A->dev.n, nnz = m->nnz = A->dev.nnz;
  hipError_t e = hipMalloc((void **)&m->val32, ((size_t)nnz + 4) * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void **)&m->r, ((size_t)n + 2) * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void **)&m->Ax, ((size_t)n + 2) * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void **)&m->r32, ((size_t)n + 4) * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void **)&m->d32, ((size_t)n + 4) * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void **)&m->part, (2 * (size_t)kMaxGrid + 2) * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void **)&m->bad, 2 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipHostMalloc((void **)&m->h_rr, 64, hipHostMallocDefault);
  // the slack elements are read by nobody's arithmetic, but never uninitialised
  if (e == hipSuccess) e = hipMemsetAsync(m->val32, 0, ((size_t)nnz + 4) * sizeof(float), s);
  if (e == hipSuccess) e = hipMemsetAsync(m->r, 0, ((size_t)n + 2) * sizeof(double), s);
  if (e == hipSuccess) e = hipMemsetAsync(m->Ax, 0, ((size_t)n + 2) * sizeof(double), s);
  if (e == hipSuccess) e = hipMemsetAsync(m->r32, 0, ((size_t)n + 4) * sizeof(float), s);
  if (e == hipSuccess) e = hipMemsetAsync(m->d32, 0, ((size_t)n + 4) * sizeof(float), s);
  unsigned long long h[2] = {0, ~0ull};
  if (e == hipSuccess) e = hipMemcpyAsync(m->bad, h, sizeof(h), hipMemcpyHostToDevice, s);
  if (e == hipSuccess && nnz > 0) {
    hipLaunchKernelGGL(k_mixed_cast<true>, dim3(mx_grid(nnz >> 2)), dim3(kBlock), 0, s, nnz,
                       (const double *)A->dev.val, m->val32, m->bad);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h, m->bad, sizeof(h), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    mixed_free(m);
    if (e == hipErrorOutOfMemory) {
      set_error("cgx_mixed_create: out of device memory (n=%lld, nnz=%lld)", (long long)n,
                (long long)nnz);
      return CGX_ENOMEM;
    }
    return hip_fail(e, "cgx_mixed_create");
  }
  if (h[0] != 0) {
    mixed_free(m);
    set_error("cgx_mixed_create: %llu value%s of A overflow to inf or underflow to 0 in f32; the "
              "first is entry %llu", h[0], h[0] == 1 ? "" : "s", h[1]);
    return CGX_EINVAL;
  }
  int rc = cgx_csr_create(ctx, n, nnz, A->dev.rowptr, A->dev.col, m->val32, CGX_F32, nullptr,
                          &m->A32);
  if (!rc) rc = cgx_cg_create(ctx, m->A32, &m->cg32);
  if (rc) {
    mixed_free(m);
    return rc;
  }
  *out = m;
  return CGX_OK;
}

extern "C" int cgx_mixed_destroy(cgx_mixed *m) {
  if (!m) return CGX_OK;
  DeviceGuard g(m->ctx->device);
  (void)hipStreamSynchronize(m->ctx->stream);
  mixed_free(m);
  return CGX_OK;
}

extern "C" int cgx_mixed_config(cgx_mixed *m, double inner_reduction, int max_outer,
                                int64_t inner_cap) {
  CGX_REQUIRE(m, CGX_EINVAL, "NULL argument");
  CGX_REQUIRE(std::isfinite(inner_reduction) && inner_reduction >= 0, CGX_EINVAL,
              "cgx_mixed_config: inner_reduction %g must be finite and not negative (0: the "
              "default 1e-5)", inner_reduction);
  CGX_REQUIRE(max_outer >= 0, CGX_EINVAL,
              "cgx_mixed_config: max_outer %d must not be negative (0: the default 8)", max_outer);
  CGX_REQUIRE(inner_cap >= 0, CGX_EINVAL,
              "cgx_mixed_config: inner_cap %lld must not be negative (0: the default n + 1)",
              (long long)inner_cap);
  m->inner_reduction = inner_reduction > 0 ? inner_reduction : 1e-5;
  m->max_outer = max_outer > 0 ? max_outer : 8;
  m->inner_cap = inner_cap > 0 ? inner_cap : -1;
  return CGX_OK;
}

extern "C" int cgx_mixed_set_mode(cgx_mixed *m, int mode) {
  CGX_REQUIRE(m, CGX_EINVAL, "NULL argument");
  return cgx_cg_set_mode(m->cg32, mode);
}

extern "C" int cgx_mixed_set_precond(cgx_mixed *m, int kind, const void *d_minv) {
  CGX_REQUIRE(m, CGX_EINVAL, "NULL argument");
  if (kind != CGX_PRECOND_DIAGONAL) {
    const int rc = cgx_cg_set_precond(m->cg32, kind, nullptr);
    if (!rc && m->m32) {  // (set_precond drained the stream: nothing reads m32 any more)
      (void)hipFree(m->m32);
      m->m32 = nullptr;
    }
    return rc;
  }
  CGX_REQUIRE(d_minv, CGX_EINVAL, "CGX_PRECOND_DIAGONAL needs d_minv");
  CGX_REQUIRE(((uintptr_t)d_minv & 15) == 0, CGX_EINVAL,
              "d_minv must be 16-byte aligned (the kernels read it in 16-byte lanes)");
  DeviceGuard g(m->ctx->device);
  hipStream_t s = m->ctx->stream;
  float *m32 = nullptr;
  CGX_HIP(hipMalloc((void **)&m32, ((size_t)m->n + 4) * sizeof(float)));
  hipError_t e = hipMemsetAsync(m32, 0, ((size_t)m->n + 4) * sizeof(float), s);
  if (e == hipSuccess && m->n > 0) {
    hipLaunchKernelGGL(k_mixed_cast<false>, dim3(mx_grid(m->n >> 2)), dim3(kBlock), 0, s, m->n,
                       (const double *)d_minv, m32, (unsigned long long *)nullptr);
    e = hipGetLastError();
  }
  if (e != hipSuccess) {
    (void)hipFree(m32);
    return hip_fail(e, "cgx_mixed_set_precond (the f32 copy of d_minv)");
  }
  // the inner solver checks the copy: positive and finite AFTER the cast, the
  // first bad entry named in its message; on an error it keeps what it had
  const int rc = cgx_cg_set_precond(m->cg32, CGX_PRECOND_DIAGONAL, m32);
  if (rc) {
    (void)hipStreamSynchronize(s);
    (void)hipFree(m32);
    return rc;
  }
  if (m->m32) (void)hipFree(m->m32);
  m->m32 = m32;
  return CGX_OK;
}

extern "C" int cgx_mixed_solve(cgx_mixed *m, const void *d_b, void *d_x, double tol,
                               int64_t max_bodies, int *outer, int64_t *inner_bodies,
                               double *rxr, int *status) {
  CGX_REQUIRE(m, CGX_EINVAL, "NULL argument");
  CGX_REQUIRE(d_b, CGX_ESTATE, "No right hand side to solve for");
  CGX_REQUIRE(d_x, CGX_EINVAL, "x is NULL");
  CGX_REQUIRE((((uintptr_t)d_b | (uintptr_t)d_x) & 15) == 0, CGX_EINVAL,
              "cgx_mixed_solve: b and x must be 16-byte aligned (cgx_alloc's are)");
  DeviceGuard g(m->ctx->device);
  hipStream_t s = m->ctx->stream;
  const int64_t n = m->n;
  const int64_t cap = max_bodies < 0 ? n + 1 : std::min<int64_t>(n + 1, std::max<int64_t>(max_bodies, 1));
  const int64_t icap = m->inner_cap < 0 ? n + 1 : std::min<int64_t>(n + 1, m->inner_cap);
  const double *b = (const double *)d_b;
  double *x = (double *)d_x;
  m->history.clear();
  int64_t tot = 0, last_bodies = 0;
  double prev = std::numeric_limits<double>::infinity(), last_rxr = 0.0, rr = 0.0;
  int st = 0, o = 0;
  for (;; ++o) {
    int rc = cgx_spmv(m->ctx, m->A, x, m->Ax, n);
    if (rc) return rc;
    const int gr = mx_grid(n >> 1);
    hipLaunchKernelGGL(k_mixed_resid, dim3(gr), dim3(kBlock), 0, s, n, b, (const double *)m->Ax,
                       m->r, m->part);
    hipLaunchKernelGGL(k_mixed_rr, dim3(1), dim3(kBlock), 0, s, (const double *)m->part, gr,
                       m->part + 2 * kMaxGrid);
    CGX_HIP(hipGetLastError());
    CGX_HIP(hipMemcpyAsync(m->h_rr, m->part + 2 * kMaxGrid, sizeof(double),
                           hipMemcpyDeviceToHost, s));
    CGX_HIP(hipStreamSynchronize(s));
    rr = m->h_rr[0];
    m->history.push_back({rr, last_bodies, last_rxr});
    const double nr = std::sqrt(rr);
    if (!std::isfinite(rr)) { st = 4; break; }
    if (nr <= tol) { st = 1; break; }
    if (nr > 0.5 * prev) { st = 3; break; }
    if (o == m->max_outer || tot >= cap) { st = 2; break; }
    prev = nr;
    int e2 = 0;
    (void)std::frexp(nr, &e2);  // nr = f 2^e2, f in [0.5, 1)
    const double sc = std::ldexp(1.0, -e2), sinv = std::ldexp(1.0, e2);
    const double tol_in = std::max(m->inner_reduction, 0.5 * tol * sc);
    hipLaunchKernelGGL(k_mixed_down, dim3(mx_grid(n >> 2)), dim3(kBlock), 0, s, n,
                       (const double *)m->r, sc, m->r32, m->d32);
    CGX_HIP(hipGetLastError());
    int64_t ib = 0;
    double irxr = 0.0;
    rc = cgx_cg_solve(m->cg32, m->r32, m->d32, tol_in, std::min(icap, cap - tot), &ib, &irxr);
    if (rc) return rc;
    if (std::isnan(irxr)) {  // the correction is not applied: x stays the last finite iterate
      st = 4;
      break;
    }
    hipLaunchKernelGGL(k_mixed_up, dim3(mx_grid(n >> 2)), dim3(kBlock), 0, s, n, x,
                       (const float *)m->d32, sinv);
    CGX_HIP(hipGetLastError());
    tot += ib;
    last_bodies = ib;
    last_rxr = irxr;
  }
  CGX_HIP(hipStreamSynchronize(s));
  if (outer) *outer = o;
  if (inner_bodies) *inner_bodies = tot;
  if (rxr) *rxr = rr;
  if (status) *status = st;
  return CGX_OK;
}

extern "C" int cgx_mixed_history(cgx_mixed *m, double *rr, int64_t *inner_bodies,
                                 double *inner_rxr, int cap, int *count) {
  CGX_REQUIRE(m && count, CGX_EINVAL, "NULL argument");
  *count = (int)m->history.size();
  for (int i = 0; i < *count && i < cap; ++i) {
    if (rr) rr[i] = m->history[i].rr;
    if (inner_bodies) inner_bodies[i] = m->history[i].inner_bodies;
    if (inner_rxr) inner_rxr[i] = m->history[i].inner_rxr;
  }
  return CGX_OK;
}

extern "C" int cgx_mixed_inner(cgx_mixed *m, cgx_csr **A32, cgx_cg **cg32) {
  CGX_REQUIRE(m, CGX_EINVAL, "NULL argument");
  if (A32) *A32 = m->A32;
  if (cg32) *cg32 = m->cg32;
  return CGX_OK;
}

extern "C" int cgx_mixed_bytes(cgx_mixed *m, int64_t *bytes) {
  CGX_REQUIRE(m && bytes, CGX_EINVAL, "NULL argument");
  DeviceGuard g(m->ctx->device);
  const cgx_csr *a = m->A32;
  const cgx_cg *c = m->cg32;
  // every device allocation of this object, of the f32 matrix's schedule and
  // formats and of the inner solver, at its allocated size
  const void *ptrs[] = {
      m->val32, m->r, m->Ax, m->r32, m->d32, m->m32, m->part, m->bad,
      a->d_rb, a->d_ext, a->d_sell_sl, a->d_sell_dict, a->d_sell_idx, a->d_sell_val,
      a->d_sell_order, a->d_sell_mask, a->d_sell_vc, a->d_sell_vdict, a->d_sell_vc4,
      a->d_sell_sl_t, a->d_vct, a->d_col16, a->d_il, a->d_rbo, a->d_vl_cls, a->d_vl_tab,
      a->d_split, a->d_bnd_blk,
      c->r, c->p, c->Ap, c->p2, c->pk[0], c->pk[1], c->pk[2], c->minv_own, c->st, c->ws,
      c->coop_ws, c->coop_trace, c->bt.r, c->bt.p, c->bt.Ap, c->bt.st, c->bt.ws, c->bt.seq_b,
      c->bt.seq_x};
  int64_t sum = 0;
  for (const void *p : ptrs) sum += (int64_t)alloc_bytes(p);
  *bytes = sum;
  return CGX_OK;
}
