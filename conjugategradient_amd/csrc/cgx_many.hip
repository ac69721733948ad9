// cgx_many.hip — many small SPD systems on one sparsity pattern (cgx.h
// "cgx_many"): one workgroup of kBlock threads runs a whole CG
// solve, init and every body, then takes the next system. Thread t owns rows
// t, t + 256, ...: their x and r stay in registers, p (the gather source)
// lives in LDS, a dot is a workgroup reduction. There is no kernel boundary,
// no graph replay and no traffic between workgroups; the body loop is bounded
// by the cap (at most n + 1 <= 4,097 bodies), so a workgroup always ends.
//
// Arithmetic (normative; cgx.h): system s's x, body count, stop code and final
// r.r are those of cgx_cg_solve in mode 1 on (rowptr, col, val_s), bit for
// bit: the single kernels' per-element expressions with products rounded
// before adds (-ffp-contract=off), a row summed by one thread from 0 in
// ascending entry order, the dots double-length sums (cgx_dd.h) rounded once,
// stop rule Q5 as k_update_xp applies it. With cgx_many_set_precond the same
// kernel runs PCG with a diagonal M^-1 (k_many_cg's PC), pinned the same way
// to mode 1 under cgx_cg_set_precond. For n <= 256 k_many_cg_wave gives each
// system a wave instead (cgx_many_set_form): the same arithmetic, four
// independent solves per workgroup and no workgroup barrier.
#include <cmath>
#include <climits>
#include <limits>
#include <map>
#include <mutex>

#include "cgx_dd.h"
#include "cgx_objects.h"

using namespace cgx;

namespace {

struct DeviceGuard {
  explicit DeviceGuard(int dev) { (void)hipSetDevice(dev); }
};

constexpr int kManyMaxN = 16 * kBlock;  // rows of one system: the widest instantiation's

struct ManyArgs {
  const int *rowptr, *col;
  const double *val, *B;
  double *X;
  int64_t ldv, ldb, ldx;
  long long *bodies;  // per system: the outputs
  double *rxr;
  int *stopped;
  double tol;
  int nsys, n, cap;
  // the preconditioned form's (last: the plain form's arguments stay where they were)
  const double *M;  // DIAGONAL: the caller's m, system s at M + s ldm; JACOBI: NULL
  int64_t ldm;
  double *rz;       // per system: r.z after the last body
};

// k_diag_inv's verdict on a diagonal (or on a caller's m): positive and finite
__device__ __forceinline__ bool many_pc_ok(double d) {
  return d > 0.0 && d <= std::numeric_limits<double>::max();  // false for NaN
}

// The workgroup sum of one pair per thread, rounded once, in every thread:
// waves first (wave_sum_dd), then wave 0 to 3 in that order, as
// mx_block_sum (cgx_mixed.hip). red: 8 doubles that no thread writes again
// before the workgroup's next barrier but one (the callers alternate two).
__device__ __forceinline__ double many_sum(Dd<double> v, double *red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  v = wave_sum_dd(v);
  if (lane == 0) {
    red[2 * w] = v.hi;
    red[2 * w + 1] = v.lo;
  }
  __syncthreads();
  Dd<double> s(red[0], red[1]);
#pragma unroll
  for (int k = 1; k < kBlock / 64; ++k) s += Dd<double>(red[2 * k], red[2 * k + 1]);
  return s.value();
}

// Two workgroup sums behind one barrier: many_sum's value for each pair (the
// same wave sums, the same wave order). red: 16 doubles, as many_sum's 8.
__device__ __forceinline__ void many_sum2(Dd<double> u, Dd<double> v, double *red, double *su,
                                          double *sv) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  u = wave_sum_dd(u);
  v = wave_sum_dd(v);
  if (lane == 0) {
    red[2 * w] = u.hi;
    red[2 * w + 1] = u.lo;
    red[8 + 2 * w] = v.hi;
    red[8 + 2 * w + 1] = v.lo;
  }
  __syncthreads();
  Dd<double> s(red[0], red[1]), z(red[8], red[9]);
#pragma unroll
  for (int k = 1; k < kBlock / 64; ++k) {
    s += Dd<double>(red[2 * k], red[2 * k + 1]);
    z += Dd<double>(red[8 + 2 * k], red[8 + 2 * k + 1]);
  }
  *su = s.value();
  *sv = z.value();
}

// R rows per thread: n <= R kBlock. LDS: p (R kBlock doubles) and two
// reduction stagings.
//
// PC: diagonal preconditioning (cgx_many_set_precond), statement for statement
// as k_pc_init, update_r_pc_body, k_update_xp_pc and pc_stop_rule
// (cgx_kernels.hip): z_i = m_i * r_i, rounded, never stored beyond the body
// that forms it (it takes Ap's register once r is updated); alpha = rz / p.Ap,
// beta = rz' / rz, r.r and r.z summed behind one barrier, so a body keeps its
// three barriers; the stop rule tests the true r.r. m is a second R kBlock
// doubles of LDS that a thread reads and writes only at its own rows (stride
// 1, no barrier of its own): a.M's entries (DIAGONAL), or 1 / a_ii formed by
// the row's thread from the values this solve reads (JACOBI, a.M == NULL; the
// entries with col == row summed from 0 in entry order, as k_diag_inv), so a
// caller who overwrites the values in place never meets a stale diagonal.
// A row without a diagonal entry (JACOBI), or a d (JACOBI) or m_i (DIAGONAL)
// that is not positive and finite, ends that system before anything of it is
// written: X as given, 0 bodies, NaN r.r and r.z, stop code 3. `refused`
// carries the verdict across the init's first barrier; the extra barrier of
// that path keeps a thread that is already at the next system from writing
// the word while another still reads it. The plain form (PC = false) is the
// code it was: every addition is behind `if constexpr (PC)`.
template <int R, bool PC>
__global__ __launch_bounds__(kBlock) void k_many_cg(ManyArgs a) {
  __shared__ double p[R * kBlock];
  __shared__ double red[2][PC ? 16 : 8];
  __shared__ double mm[PC ? R * kBlock : 1];  // (unused, and dropped, without PC)
  __shared__ int refused;                     // (the same)
  const int t = threadIdx.x, n = a.n;
  if constexpr (PC) {
    if (t == 0) refused = 0;
    __syncthreads();
  }
  // the pattern is every system's: a thread's row bounds stay in registers
  int e0[R], e1[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int i = t + k * kBlock;
    e0[k] = i < n ? a.rowptr[i] : 0;
    e1[k] = i < n ? a.rowptr[i + 1] : 0;
  }
  for (int s = blockIdx.x; s < a.nsys; s += gridDim.x) {
    const double *__restrict__ val = a.val + (int64_t)s * a.ldv;
    const double *__restrict__ b = a.B + (int64_t)s * a.ldb;
    double *__restrict__ xs = a.X + (int64_t)s * a.ldx;
    double x[R], r[R];
    // ---- init: r = b - A x, p = r, rxr = r.r (k_cg_init) ----
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int i = t + k * kBlock;
      x[k] = i < n ? xs[i] : 0.0;
      if (i < n) p[i] = x[k];  // x through LDS: the init's gather source
    }
    if constexpr (PC) {  // m of the own rows, and the verdict on it
      bool bad = false;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int i = t + k * kBlock;
        if (i < n) {
          double mv;
          if (a.M) {
            mv = a.M[(int64_t)s * a.ldm + i];
            bad = bad || !many_pc_ok(mv);
          } else {
            double d = 0.0;
            bool found = false;
            for (int e = e0[k]; e < e1[k]; ++e)
              if (a.col[e] == i) {
                d = d + val[e];
                found = true;
              }
            mv = 1.0 / d;
            bad = bad || !found || !many_pc_ok(d);
          }
          mm[i] = mv;
        }
      }
      if (bad) refused = s + 1;  // (s + 1 > 0 marks this system alone: no reset)
    }
    __syncthreads();
    if constexpr (PC) {
      if (refused == s + 1) {  // uniform: every thread reads it behind the barrier
        if (t == 0) {
          a.bodies[s] = 0;
          a.rxr[s] = __builtin_nan("");
          a.rz[s] = __builtin_nan("");
          a.stopped[s] = 3;
        }
        __syncthreads();  // every read of `refused`, before the next system may write it
        continue;
      }
    }
    Dd<double> acc(0.0);
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int i = t + k * kBlock;
      double sum = 0.0;
      for (int e = e0[k]; e < e1[k]; ++e) sum = sum + val[e] * p[a.col[e]];
      r[k] = 0.0;
      if (i < n) {
        r[k] = b[i] - sum;
        acc += r[k] * r[k];
      }
    }
    __syncthreads();  // every gather of x is done: p may be overwritten
    double rxr, rz = 0.0;
    if constexpr (PC) {  // p = m o r, rz = r.(m o r) (k_pc_init)
      Dd<double> accz(0.0);
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int i = t + k * kBlock;
        if (i < n) {
          const double z = mm[i] * r[k];
          p[i] = z;
          accz += r[k] * z;
        }
      }
      many_sum2(acc, accz, red[1], &rxr, &rz);  // (its barrier publishes p too)
    } else {
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int i = t + k * kBlock;
        if (i < n) p[i] = r[k];
      }
      rxr = many_sum(acc, red[1]);  // (its barrier publishes p too)
    }
    long long bodies = 0;
    int stopped = 0;
    // ---- the bodies ----
    for (;;) {
      // Ap = A p and p.Ap (k_spmv_dot)
      double Ap[R];
      acc = Dd<double>(0.0);
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int i = t + k * kBlock;
        double sum = 0.0;
        for (int e = e0[k]; e < e1[k]; ++e) sum = sum + val[e] * p[a.col[e]];
        Ap[k] = sum;
        if (i < n) acc += sum * p[i];
      }
      const double pAp = many_sum(acc, red[0]);
      const double alpha = (PC ? rz : rxr) / pAp;
      // r -= alpha Ap and r.r (k_update_r); PC: r.z in the same sweep, z
      // kept where Ap was (update_r_pc_body)
      acc = Dd<double>(0.0);
      double rr, rzn = 0.0;
      if constexpr (PC) {
        Dd<double> accz(0.0);
#pragma unroll
        for (int k = 0; k < R; ++k) {
          const int i = t + k * kBlock;
          if (i < n) {
            r[k] = r[k] - alpha * Ap[k];
            acc += r[k] * r[k];
            const double z = mm[i] * r[k];
            accz += r[k] * z;
            Ap[k] = z;
          }
        }
        many_sum2(acc, accz, red[1], &rr, &rzn);
      } else {
#pragma unroll
        for (int k = 0; k < R; ++k) {
          const int i = t + k * kBlock;
          if (i < n) {
            r[k] = r[k] - alpha * Ap[k];
            acc += r[k] * r[k];
          }
        }
        rr = many_sum(acc, red[1]);
      }
      const double beta = PC ? rzn / rz : rr / rxr;
      // x += alpha p; p = r + beta p (PC: m o r + beta p); the stop rule
      // (k_update_xp, k_update_xp_pc). Every gather of this body's p lies
      // before the two barriers above.
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int i = t + k * kBlock;
        if (i < n) {
          const double pv = p[i];
          x[k] = x[k] + alpha * pv;
          p[i] = (PC ? Ap[k] : r[k]) + beta * pv;
        }
      }
      ++bodies;
      const bool cond = isnan(rxr) || sqrt(rxr) <= a.tol;  // Q5: the r.r the body began with
      const bool cont = !cond && bodies < a.cap;
      stopped = cond ? 1 : (cont ? 0 : 2);
      rxr = rr;
      if constexpr (PC) rz = rzn;
      __syncthreads();  // the new p, before the next gather (or the next system's x)
      if (!cont) break;
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int i = t + k * kBlock;
      if (i < n) xs[i] = x[k];
    }
    if (t == 0) {
      a.bodies[s] = bodies;
      a.rxr[s] = rxr;
      a.stopped[s] = stopped;
      if constexpr (PC) a.rz[s] = rz;
    }
  }
}

// ---- a wave per system (n <= 256; cgx_many_set_form) --------
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;  // systems a workgroup runs side by side
constexpr int kManyWaveMaxN = 4 * kWave;  // rows of one system in the wave form

// Orders a wave's LDS accesses around it: what the lanes wrote before is what
// they read after, and nothing read before is overwritten early. A wave issues
// its LDS instructions in order, so all this has to stop is the compiler: a
// wavefront-scope fence and a wave barrier, neither of which is an s_barrier.
__device__ __forceinline__ void wave_order() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// lane 0's value in every lane, as scalars: the compiler sees it wave-uniform
__device__ __forceinline__ double wave_first(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// The wave's sum of one pair per lane, rounded once, the same bits in every
// lane. At R = 1 it is many_sum's value: the workgroup form's waves 1 to 3
// then add Dd(0, 0), which changes neither hi nor the rounded value.
__device__ __forceinline__ double wave_dot(Dd<double> v) {
  return wave_first(wave_sum_dd(v).value());
}

// R rows per lane: n <= R kWave. Wave w of workgroup b runs systems 4 b + w,
// 4 b + w + 4 grid, ...; lane l owns rows l, l + 64, ...: their x and r in
// registers, p (and m under PC) in the wave's own R kWave doubles of LDS. The
// four waves of a workgroup never meet: there is no workgroup barrier below
// (they run different body counts, so one would hang), only wave_order()
// where k_many_cg has a barrier. The arithmetic is k_many_cg's, statement for
// statement; a bad diagonal's verdict is a wave vote.
template <int R, bool PC>
__global__ __launch_bounds__(kBlock) void k_many_cg_wave(ManyArgs a) {
  __shared__ double p_all[kWaves * R * kWave];
  __shared__ double m_all[PC ? kWaves * R * kWave : 1];  // (unused, and dropped, without PC)
  const int lane = threadIdx.x & (kWave - 1), n = a.n;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  double *const p = p_all + w * (R * kWave);
  [[maybe_unused]] double *const mm = m_all + (PC ? w * (R * kWave) : 0);
  // the pattern is every system's: a lane's row bounds stay in registers
  int e0[R], e1[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int i = lane + k * kWave;
    e0[k] = i < n ? a.rowptr[i] : 0;
    e1[k] = i < n ? a.rowptr[i + 1] : 0;
  }
  for (int s = blockIdx.x * kWaves + w; s < a.nsys; s += gridDim.x * kWaves) {
    const double *__restrict__ val = a.val + (int64_t)s * a.ldv;
    const double *__restrict__ b = a.B + (int64_t)s * a.ldb;
    double *__restrict__ xs = a.X + (int64_t)s * a.ldx;
    double x[R], r[R];
    // ---- init: r = b - A x, p = r, rxr = r.r (k_cg_init) ----
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int i = lane + k * kWave;
      x[k] = i < n ? xs[i] : 0.0;
      if (i < n) p[i] = x[k];  // x through LDS: the init's gather source
    }
    if constexpr (PC) {  // m of the own rows, and the verdict on it
      bool bad = false;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int i = lane + k * kWave;
        if (i < n) {
          double mv;
          if (a.M) {
            mv = a.M[(int64_t)s * a.ldm + i];
            bad = bad || !many_pc_ok(mv);
          } else {
            double d = 0.0;
            bool found = false;
            for (int e = e0[k]; e < e1[k]; ++e)
              if (a.col[e] == i) {
                d = d + val[e];
                found = true;
              }
            mv = 1.0 / d;
            bad = bad || !found || !many_pc_ok(d);
          }
          mm[i] = mv;
        }
      }
      if (__any(bad)) {  // uniform: the wave's vote
        if (lane == 0) {
          a.bodies[s] = 0;
          a.rxr[s] = __builtin_nan("");
          a.rz[s] = __builtin_nan("");
          a.stopped[s] = 3;
        }
        continue;  // (p holds x, which nobody gathered: the next system overwrites it)
      }
    }
    wave_order();  // x is in p
    Dd<double> acc(0.0);
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int i = lane + k * kWave;
      double sum = 0.0;
      for (int e = e0[k]; e < e1[k]; ++e) sum = sum + val[e] * p[a.col[e]];
      r[k] = 0.0;
      if (i < n) {
        r[k] = b[i] - sum;
        acc += r[k] * r[k];
      }
    }
    wave_order();  // every gather of x is done: p may be overwritten
    double rxr, rz = 0.0;
    if constexpr (PC) {  // p = m o r, rz = r.(m o r) (k_pc_init)
      Dd<double> accz(0.0);
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int i = lane + k * kWave;
        if (i < n) {
          const double z = mm[i] * r[k];
          p[i] = z;
          accz += r[k] * z;
        }
      }
      rxr = wave_dot(acc);
      rz = wave_dot(accz);
    } else {
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int i = lane + k * kWave;
        if (i < n) p[i] = r[k];
      }
      rxr = wave_dot(acc);
    }
    wave_order();  // p is written
    long long bodies = 0;
    int stopped = 0;
    // ---- the bodies ----
    for (;;) {
      // Ap = A p and p.Ap (k_spmv_dot)
      double Ap[R];
      acc = Dd<double>(0.0);
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int i = lane + k * kWave;
        double sum = 0.0;
        for (int e = e0[k]; e < e1[k]; ++e) sum = sum + val[e] * p[a.col[e]];
        Ap[k] = sum;
        if (i < n) acc += sum * p[i];
      }
      const double pAp = wave_dot(acc);
      const double alpha = (PC ? rz : rxr) / pAp;
      // r -= alpha Ap and r.r (k_update_r); PC: r.z in the same sweep, z
      // kept where Ap was (update_r_pc_body)
      acc = Dd<double>(0.0);
      double rr, rzn = 0.0;
      if constexpr (PC) {
        Dd<double> accz(0.0);
#pragma unroll
        for (int k = 0; k < R; ++k) {
          const int i = lane + k * kWave;
          if (i < n) {
            r[k] = r[k] - alpha * Ap[k];
            acc += r[k] * r[k];
            const double z = mm[i] * r[k];
            accz += r[k] * z;
            Ap[k] = z;
          }
        }
        rr = wave_dot(acc);
        rzn = wave_dot(accz);
      } else {
#pragma unroll
        for (int k = 0; k < R; ++k) {
          const int i = lane + k * kWave;
          if (i < n) {
            r[k] = r[k] - alpha * Ap[k];
            acc += r[k] * r[k];
          }
        }
        rr = wave_dot(acc);
      }
      const double beta = PC ? rzn / rz : rr / rxr;
      wave_order();  // every gather of this body's p is done
      // x += alpha p; p = r + beta p (PC: m o r + beta p); the stop rule
      // (k_update_xp, k_update_xp_pc)
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int i = lane + k * kWave;
        if (i < n) {
          const double pv = p[i];
          x[k] = x[k] + alpha * pv;
          p[i] = (PC ? Ap[k] : r[k]) + beta * pv;
        }
      }
      ++bodies;
      const bool cond = isnan(rxr) || sqrt(rxr) <= a.tol;  // Q5: the r.r the body began with
      const bool cont = !cond && bodies < a.cap;
      stopped = cond ? 1 : (cont ? 0 : 2);
      rxr = rr;
      if constexpr (PC) rz = rzn;
      wave_order();  // the new p, before the next gather (or the next system's x)
      if (!cont) break;
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int i = lane + k * kWave;
      if (i < n) xs[i] = x[k];
    }
    if (lane == 0) {
      a.bodies[s] = bodies;
      a.rxr[s] = rxr;
      a.stopped[s] = stopped;
      if constexpr (PC) a.rz[s] = rz;
    }
  }
}

// The pattern's check, once at create: bad[0] counts the entries of rowptr
// that are outside [0, nnz], descend, or miss rowptr[0] = 0 / rowptr[n] = nnz,
// bad[1] the columns outside [0, n).
__global__ __launch_bounds__(kBlock) void k_many_check(int n, int nnz,
                                                       const int *__restrict__ rowptr,
                                                       const int *__restrict__ col,
                                                       unsigned long long *bad) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  unsigned long long br = 0, bc = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += stride) {
    const int v = rowptr[i];
    if (v < 0 || v > nnz) ++br;
    else if (i == 0 && v != 0) ++br;
    else if (i == n && v != nnz) ++br;
    else if (i > 0 && rowptr[i - 1] > v) ++br;
  }
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz; e += stride) {
    const int c = col[e];
    if (c < 0 || c >= n) ++bc;
  }
  if (br) atomicAdd(&bad[0], br);
  if (bc) atomicAdd(&bad[1], bc);
}

int many_rows_per_thread(int64_t n) {
  int r = 1;
  while ((int64_t)r * kBlock < n) r *= 2;
  return r;
}

template <bool PC> const void *many_kernel_of(int r) {
  switch (r) {
    case 1: return reinterpret_cast<const void *>(&k_many_cg<1, PC>);
    case 2: return reinterpret_cast<const void *>(&k_many_cg<2, PC>);
    case 4: return reinterpret_cast<const void *>(&k_many_cg<4, PC>);
    case 8: return reinterpret_cast<const void *>(&k_many_cg<8, PC>);
    case 16: return reinterpret_cast<const void *>(&k_many_cg<16, PC>);
    default: return nullptr;
  }
}

int many_rows_per_lane(int64_t n) {  // the wave form's R (n <= kManyWaveMaxN)
  int r = 1;
  while ((int64_t)r * kWave < n) r *= 2;
  return r;
}

template <bool PC> const void *many_wave_kernel_of(int r) {
  switch (r) {
    case 1: return reinterpret_cast<const void *>(&k_many_cg_wave<1, PC>);
    case 2: return reinterpret_cast<const void *>(&k_many_cg_wave<2, PC>);
    case 4: return reinterpret_cast<const void *>(&k_many_cg_wave<4, PC>);
    default: return nullptr;
  }
}

const void *many_kernel(int r, bool pc, bool wave) {
  if (wave) return pc ? many_wave_kernel_of<true>(r) : many_wave_kernel_of<false>(r);
  return pc ? many_kernel_of<true>(r) : many_kernel_of<false>(r);
}

// workgroups of k_many_cg<r, pc> (wave: k_many_cg_wave<r, pc>) resident on the
// device at once (occupancy x CUs; 0: unknown), as spmv_dot_resident
int many_resident(int r, bool pc, bool wave) {
  static std::mutex mu;
  // (device, 4 r + 2 with the wave form + 1 with pc) -> workgroups
  static std::map<std::pair<int, int>, int> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  std::lock_guard<std::mutex> lk(mu);
  const std::pair<int, int> key{dev, 4 * r + (wave ? 2 : 0) + (pc ? 1 : 0)};
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int res = 0, nb = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, many_kernel(r, pc, wave), kBlock, 0) ==
          hipSuccess &&
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
    res = nb * cus;
  cache[key] = res;
  return res;
}

}  // namespace

struct cgx_many {
  cgx_ctx *ctx = nullptr;
  int64_t nsys = 0, n = 0, nnz = 0, ldv = 0;
  const int *rowptr = nullptr, *col = nullptr;  // the caller's
  const double *val = nullptr;
  int r = 1;               // rows per thread (the workgroup form's)
  int form = CGX_MANY_FORM_AUTO;  // cgx_many_set_form: as requested
  int max_workgroups = 0;  // cgx_many_config (0: the resident workgroups)
  int precond = CGX_PRECOND_NONE;  // cgx_many_set_precond: the next solve's
  const double *d_M = nullptr;     // DIAGONAL: the caller's
  int64_t ldm = 0;
  bool rz_valid = false;  // the last solve was preconditioned, with this preconditioner
  long long *d_bodies = nullptr;
  double *d_rxr = nullptr, *d_rz = nullptr;
  int *d_stopped = nullptr;
  long long *h_bodies = nullptr;  // pinned, nsys each
  double *h_rxr = nullptr, *h_rz = nullptr;
  int *h_stopped = nullptr;
};

namespace {

void many_free(cgx_many *m) {
  if (!m) return;
  void *dev[] = {m->d_bodies, m->d_rxr, m->d_rz, m->d_stopped};
  for (void *p : dev)
    if (p) (void)hipFree(p);
  void *host[] = {m->h_bodies, m->h_rxr, m->h_rz, m->h_stopped};
  for (void *p : host)
    if (p) (void)hipHostFree(p);
  if (m->ctx) ctx_release(m->ctx);
  delete m;
}

template <bool PC>
void many_launch(int r, dim3 grid, dim3 block, hipStream_t s, const ManyArgs &a) {
  switch (r) {
    case 1: hipLaunchKernelGGL((k_many_cg<1, PC>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_many_cg<2, PC>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((k_many_cg<4, PC>), grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL((k_many_cg<8, PC>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((k_many_cg<16, PC>), grid, block, 0, s, a); break;
  }
}

template <bool PC>
void many_launch_wave(int r, dim3 grid, dim3 block, hipStream_t s, const ManyArgs &a) {
  switch (r) {
    case 1: hipLaunchKernelGGL((k_many_cg_wave<1, PC>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_many_cg_wave<2, PC>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((k_many_cg_wave<4, PC>), grid, block, 0, s, a); break;
  }
}

// Auto takes the wave form up to this many rows (0: never). See DESIGN.md §5e,
// "A wave per system", for the measurement behind the value.
constexpr int kManyAutoWaveMaxN = 64;

// the form the next solve launches: CGX_MANY_FORM_WORKGROUP or CGX_MANY_FORM_WAVE
int many_form(const cgx_many *m) {
  if (m->form != CGX_MANY_FORM_AUTO) return m->form;
  return m->n <= kManyAutoWaveMaxN ? CGX_MANY_FORM_WAVE : CGX_MANY_FORM_WORKGROUP;
}

// rows per thread (per lane in the wave form) of the next solve's instantiation
int many_rows(const cgx_many *m) {
  return many_form(m) == CGX_MANY_FORM_WAVE ? many_rows_per_lane(m->n) : m->r;
}

int many_grid(const cgx_many *m) {
  const bool wave = many_form(m) == CGX_MANY_FORM_WAVE;
  int64_t g = wave ? (m->nsys + kWaves - 1) / kWaves : m->nsys;
  const int res = many_resident(many_rows(m), m->precond != CGX_PRECOND_NONE, wave);
  if (res > 0) g = std::min<int64_t>(g, res);
  if (m->max_workgroups > 0) g = std::min<int64_t>(g, m->max_workgroups);
  return (int)std::min<int64_t>(std::max<int64_t>(g, 1), INT_MAX);
}

}  // namespace

extern "C" int cgx_many_create(cgx_ctx *ctx, int dtype, int64_t nsys, int64_t n, int64_t nnz,
                               const int32_t *d_rowptr, const int32_t *d_col, const void *d_val,
                               int64_t ldv, cgx_many **out) {
  CGX_REQUIRE(out, CGX_EINVAL, "cgx_many_create: out is NULL");
  *out = nullptr;
  CGX_REQUIRE(dtype == CGX_F64 || dtype == CGX_F32, CGX_EINVAL,
              "cgx_many_create: unknown dtype %d", dtype);
  CGX_REQUIRE(dtype == CGX_F64, CGX_EUNSUPPORTED,
              "cgx_many_create: f32 systems are not supported (the many-systems solve is f64)");
  CGX_REQUIRE(nsys >= 1, CGX_EINVAL, "cgx_many_create: nsys %lld must be at least 1",
              (long long)nsys);
  CGX_REQUIRE(nsys <= INT_MAX, CGX_EINVAL, "cgx_many_create: nsys %lld exceeds %d",
              (long long)nsys, INT_MAX);
  CGX_REQUIRE(n >= 1, CGX_EINVAL, "cgx_many_create: n %lld must be at least 1", (long long)n);
  CGX_REQUIRE(n <= kManyMaxN, CGX_EUNSUPPORTED,
              "cgx_many_create: n %lld exceeds %d rows, the most one workgroup holds; solve "
              "larger systems one at a time with cgx_cg_solve",
              (long long)n, kManyMaxN);
  CGX_REQUIRE(nnz >= 0 && nnz <= INT_MAX, CGX_EINVAL,
              "cgx_many_create: nnz %lld is outside [0, %d]", (long long)nnz, INT_MAX);
  CGX_REQUIRE(ldv >= nnz, CGX_EINVAL, "cgx_many_create: ldv %lld is below nnz %lld",
              (long long)ldv, (long long)nnz);
  CGX_REQUIRE((((uintptr_t)d_rowptr | (uintptr_t)d_col) & 3) == 0, CGX_EINVAL,
              "cgx_many_create: rowptr and col must be 4-byte aligned");
  CGX_REQUIRE(((uintptr_t)d_val & 7) == 0, CGX_EINVAL,
              "cgx_many_create: the values must be 8-byte aligned");
  // (last, so that the refusals above need no device)
  CGX_REQUIRE(ctx && d_rowptr && d_col && d_val, CGX_EINVAL, "cgx_many_create: NULL argument");
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  auto *m = new cgx_many();
  m->ctx = ctx;
  ctx_retain(ctx);
  m->nsys = nsys;
  m->n = n;
  m->nnz = nnz;
  m->ldv = ldv;
  m->rowptr = d_rowptr;
  m->col = d_col;
  m->val = (const double *)d_val;
  m->r = many_rows_per_thread(n);
  unsigned long long *bad = nullptr, h[2] = {0, 0};
  hipError_t e = hipMalloc((void **)&m->d_bodies, (size_t)nsys * sizeof(long long));
  if (e == hipSuccess) e = hipMalloc((void **)&m->d_rxr, (size_t)nsys * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void **)&m->d_rz, (size_t)nsys * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void **)&m->d_stopped, (size_t)nsys * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void **)&bad, sizeof(h));
  if (e == hipSuccess)
    e = hipHostMalloc((void **)&m->h_bodies, (size_t)nsys * sizeof(long long), hipHostMallocDefault);
  if (e == hipSuccess)
    e = hipHostMalloc((void **)&m->h_rxr, (size_t)nsys * sizeof(double), hipHostMallocDefault);
  if (e == hipSuccess)
    e = hipHostMalloc((void **)&m->h_rz, (size_t)nsys * sizeof(double), hipHostMallocDefault);
  if (e == hipSuccess)
    e = hipHostMalloc((void **)&m->h_stopped, (size_t)nsys * sizeof(int), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMemsetAsync(bad, 0, sizeof(h), s);
  if (e == hipSuccess) {
    const int64_t items = std::max<int64_t>(n + 1, nnz);
    const int grid = (int)std::min<int64_t>((items + kBlock - 1) / kBlock, kMaxGrid);
    hipLaunchKernelGGL(k_many_check, dim3(grid), dim3(kBlock), 0, s, (int)n, (int)nnz, d_rowptr,
                       d_col, bad);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h, bad, sizeof(h), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (bad) (void)hipFree(bad);
  if (e != hipSuccess) {
    many_free(m);
    if (e == hipErrorOutOfMemory) {
      set_error("cgx_many_create: out of memory (nsys=%lld)", (long long)nsys);
      return CGX_ENOMEM;
    }
    return hip_fail(e, "cgx_many_create");
  }
  if (h[0] || h[1]) {
    many_free(m);
    if (h[0])
      set_error("cgx_many_create: %llu entr%s of rowptr outside a CSR row pointer's (rowptr[0] = "
                "0, ascending, rowptr[n] = nnz = %lld)", h[0], h[0] == 1 ? "y" : "ies",
                (long long)nnz);
    else
      set_error("cgx_many_create: %llu column ind%s outside [0, %lld)", h[1],
                h[1] == 1 ? "ex" : "ices", (long long)n);
    return CGX_EINVAL;
  }
  *out = m;
  return CGX_OK;
}

extern "C" int cgx_many_destroy(cgx_many *m) {
  if (!m) return CGX_OK;
  DeviceGuard g(m->ctx->device);
  (void)hipStreamSynchronize(m->ctx->stream);
  many_free(m);
  return CGX_OK;
}

extern "C" int cgx_many_config(cgx_many *m, int max_workgroups) {
  CGX_REQUIRE(m, CGX_EINVAL, "NULL argument");
  CGX_REQUIRE(max_workgroups >= 0, CGX_EINVAL,
              "cgx_many_config: max_workgroups %d must not be negative (0: the default, the "
              "resident workgroups)", max_workgroups);
  m->max_workgroups = max_workgroups;
  return CGX_OK;
}

extern "C" int cgx_many_solve(cgx_many *m, const void *d_B, int64_t ldb, void *d_X, int64_t ldx,
                              double tol, int64_t max_bodies, int64_t *bodies_out,
                              double *rxr_out, int *stopped_out) {
  CGX_REQUIRE(m, CGX_EINVAL, "NULL argument");
  CGX_REQUIRE(d_B, CGX_EINVAL, "cgx_many_solve: B is NULL");
  CGX_REQUIRE(d_X, CGX_EINVAL, "cgx_many_solve: X is NULL");
  CGX_REQUIRE(bodies_out && rxr_out, CGX_EINVAL, "cgx_many_solve: bodies_out or rxr_out is NULL");
  CGX_REQUIRE(ldb >= m->n && ldx >= m->n, CGX_EINVAL,
              "cgx_many_solve: ldb %lld or ldx %lld is below n %lld", (long long)ldb,
              (long long)ldx, (long long)m->n);
  CGX_REQUIRE((((uintptr_t)d_B | (uintptr_t)d_X) & 7) == 0, CGX_EINVAL,
              "cgx_many_solve: B and X must be 8-byte aligned");
  DeviceGuard g(m->ctx->device);
  hipStream_t s = m->ctx->stream;
  const int64_t n = m->n;
  const int64_t cap = max_bodies < 0 ? n + 1 : std::min<int64_t>(n + 1, std::max<int64_t>(max_bodies, 1));
  ManyArgs a;
  a.rowptr = m->rowptr;
  a.col = m->col;
  a.val = m->val;
  a.B = (const double *)d_B;
  a.X = (double *)d_X;
  a.ldv = m->ldv;
  a.ldb = ldb;
  a.ldx = ldx;
  a.bodies = m->d_bodies;
  a.rxr = m->d_rxr;
  a.stopped = m->d_stopped;
  a.tol = tol;
  a.nsys = (int)m->nsys;
  a.n = (int)n;
  a.cap = (int)cap;
  const bool pc = m->precond != CGX_PRECOND_NONE;
  a.M = m->precond == CGX_PRECOND_DIAGONAL ? m->d_M : nullptr;
  a.ldm = m->ldm;
  a.rz = m->d_rz;
  m->rz_valid = false;
  const dim3 grid(many_grid(m)), block(kBlock);
  if (many_form(m) == CGX_MANY_FORM_WAVE) {
    if (pc) many_launch_wave<true>(many_rows(m), grid, block, s, a);
    else many_launch_wave<false>(many_rows(m), grid, block, s, a);
  } else {
    if (pc) many_launch<true>(m->r, grid, block, s, a);
    else many_launch<false>(m->r, grid, block, s, a);
  }
  CGX_HIP(hipGetLastError());
  const size_t ns = (size_t)m->nsys;
  if (pc) CGX_HIP(hipMemcpyAsync(m->h_rz, m->d_rz, ns * sizeof(double), hipMemcpyDeviceToHost, s));
  CGX_HIP(hipMemcpyAsync(m->h_bodies, m->d_bodies, ns * sizeof(long long), hipMemcpyDeviceToHost, s));
  CGX_HIP(hipMemcpyAsync(m->h_rxr, m->d_rxr, ns * sizeof(double), hipMemcpyDeviceToHost, s));
  CGX_HIP(hipMemcpyAsync(m->h_stopped, m->d_stopped, ns * sizeof(int), hipMemcpyDeviceToHost, s));
  CGX_HIP(hipStreamSynchronize(s));
  for (size_t i = 0; i < ns; ++i) {
    bodies_out[i] = (int64_t)m->h_bodies[i];
    rxr_out[i] = m->h_rxr[i];
    if (stopped_out) stopped_out[i] = m->h_stopped[i];
  }
  m->rz_valid = pc;
  return CGX_OK;
}

extern "C" int cgx_many_set_precond(cgx_many *m, int kind, const void *d_M, int64_t ldm) {
  CGX_REQUIRE(kind == CGX_PRECOND_NONE || kind == CGX_PRECOND_JACOBI ||
                  kind == CGX_PRECOND_DIAGONAL,
              CGX_EINVAL, "cgx_many_set_precond: unknown kind %d", kind);
  if (kind == CGX_PRECOND_DIAGONAL) {
    CGX_REQUIRE(d_M, CGX_EINVAL, "cgx_many_set_precond: DIAGONAL needs d_M, which is NULL");
    CGX_REQUIRE(((uintptr_t)d_M & 7) == 0, CGX_EINVAL,
                "cgx_many_set_precond: d_M must be 8-byte aligned");
  }
  CGX_REQUIRE(m, CGX_EINVAL, "cgx_many_set_precond: NULL handle");
  if (kind == CGX_PRECOND_DIAGONAL)
    CGX_REQUIRE(ldm >= m->n, CGX_EINVAL, "cgx_many_set_precond: ldm %lld is below n %lld",
                (long long)ldm, (long long)m->n);
  m->precond = kind;
  m->d_M = kind == CGX_PRECOND_DIAGONAL ? (const double *)d_M : nullptr;
  m->ldm = kind == CGX_PRECOND_DIAGONAL ? ldm : 0;
  m->rz_valid = false;
  return CGX_OK;
}

extern "C" int cgx_many_get_precond(cgx_many *m, int *kind) {
  CGX_REQUIRE(m && kind, CGX_EINVAL, "cgx_many_get_precond: NULL argument");
  *kind = m->precond;
  return CGX_OK;
}

extern "C" int cgx_many_rz(cgx_many *m, double *rz_out) {
  CGX_REQUIRE(m && rz_out, CGX_EINVAL, "cgx_many_rz: NULL argument");
  CGX_REQUIRE(m->precond != CGX_PRECOND_NONE, CGX_ESTATE,
              "cgx_many_rz: no preconditioner is set");
  CGX_REQUIRE(m->rz_valid, CGX_ESTATE,
              "cgx_many_rz: no solve has run under this preconditioner");
  for (int64_t i = 0; i < m->nsys; ++i) rz_out[i] = m->h_rz[i];
  return CGX_OK;
}

extern "C" int cgx_many_info(cgx_many *m, int *workgroups, int *rows_per_thread,
                             int64_t *lds_bytes) {
  CGX_REQUIRE(m, CGX_EINVAL, "NULL argument");
  DeviceGuard g(m->ctx->device);
  if (workgroups) *workgroups = many_grid(m);
  if (rows_per_thread) *rows_per_thread = many_rows(m);
  if (lds_bytes) {
    if (many_form(m) == CGX_MANY_FORM_WAVE)  // four waves' p; preconditioned: their m too
      *lds_bytes = (int64_t)(m->precond == CGX_PRECOND_NONE ? 1 : 2) * kWaves * many_rows(m) *
                   kWave * (int64_t)sizeof(double);
    else  // p and the stagings; preconditioned: m, wider stagings and the verdict word
      *lds_bytes = m->precond == CGX_PRECOND_NONE
                       ? ((int64_t)m->r * kBlock + 16) * (int64_t)sizeof(double)
                       : ((int64_t)2 * m->r * kBlock + 32) * (int64_t)sizeof(double) + 8;
  }
  return CGX_OK;
}

extern "C" int cgx_many_set_form(cgx_many *m, int form) {
  CGX_REQUIRE(form == CGX_MANY_FORM_AUTO || form == CGX_MANY_FORM_WORKGROUP ||
                  form == CGX_MANY_FORM_WAVE,
              CGX_EINVAL, "cgx_many_set_form: unknown form %d", form);
  CGX_REQUIRE(m, CGX_EINVAL, "cgx_many_set_form: NULL handle");
  CGX_REQUIRE(form != CGX_MANY_FORM_WAVE || m->n <= kManyWaveMaxN, CGX_EUNSUPPORTED,
              "cgx_many_set_form: n %lld exceeds %d rows, the most one wave holds; larger "
              "systems run in the workgroup form",
              (long long)m->n, kManyWaveMaxN);
  m->form = form;
  return CGX_OK;
}

extern "C" int cgx_many_get_form(cgx_many *m, int *requested, int *in_effect) {
  CGX_REQUIRE(m, CGX_EINVAL, "cgx_many_get_form: NULL handle");
  if (requested) *requested = m->form;
  if (in_effect) *in_effect = many_form(m);
  return CGX_OK;
}
