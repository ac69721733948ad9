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
// kernel runs PCG with a diagonal M^-1 (kManyDiag), pinned the same way
// to mode 1 under cgx_cg_set_precond. For n <= 256 k_many_cg_wave gives each
// system a wave instead (cgx_many_set_form): the same function
// (many_cg_body) run by another team, four independent solves per workgroup
// and no workgroup barrier. With
// cgx_many_set_block_precond both forms run PCG with dense diagonal blocks of
// 1 to 8 rows (kManyBlock), pinned to mode 1 under cgx_cg_set_block_precond;
// the blocks' inverses come from a launch of their own (k_many_block_inv).
#include <cmath>
#include <climits>
#include <limits>
#include <map>
#include <mutex>
#include <type_traits>

#include "cgx_block_inv.h"
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
  int bs;  // the block form's block size (in what was padding: every other argument stays
           // where it was, and so does the size)
  // the preconditioned form's (last: the plain form's arguments stay where they were)
  const double *M;  // DIAGONAL: the caller's m, system s at M + s ldm; JACOBI: NULL; the
                    // block form: W, system s's n x bs inverse blocks at M + s ldm
  int64_t ldm;
  double *rz;       // per system: r.z after the last body
};
// The block form's verdict on a system is its word of `stopped`: zeroed before
// the launches of a solve, set to not 0 by the fill or the check where a block
// is bad, read by the CG kernel when it takes the system.

// what a CG kernel does with the residual before it enters p
enum ManyPc {
  kManyPlain = 0,  // nothing: CG
  kManyDiag = 1,   // z = m o r (cgx_many_set_precond)
  kManyBlock = 2   // z = blockdiag(W_b) r (cgx_many_set_block_precond)
};

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

// z_i = sum_j w[j] rs[b0 + j] over the block's real columns: from +0.0 in
// ascending j, each product rounded before its add (k_pc_init_blk,
// update_r_blk_body). w: the row's BS values of W; rs: the system's r in LDS;
// b0 the block's first row. All BS loads of w are issued before the first
// add, with no branch between them. In a partial last block rs is read up to
// BS - 1 doubles past row n - 1, at most kManyStagePad past the staged rows
// (LDS of the kernel's own), and w's +0.0 padding columns: neither is added.
constexpr int kManyStagePad = 8;
template <int BS>
__device__ __forceinline__ double many_block_z(const double *__restrict__ w, int b0, int n,
                                               const double *rs) {
  const int nc = min(BS, n - b0);  // the block's real columns (BS but in a partial last block)
  double wv[BS];
#pragma unroll
  for (int j = 0; j < BS; ++j) wv[j] = w[j];
  const double *rb = rs + b0;
  double z = 0.0;
#pragma unroll
  for (int j = 0; j < BS; ++j) {
    const double t = z + wv[j] * rb[j];
    z = j < nc ? t : z;
  }
  return z;
}

// z = M^-1 r at a thread's own rows t, t + S, ... (S: kBlock, or kWave in the
// wave form) from the staged r: z into zk, and into pz where that is not NULL
// (the init's p); r.z's share into accz. bs is uniform, and so is the switch:
// each block size has its own unrolled sweep, whose loads sit at constant
// offsets from the row's one address. That address is formed anew at every
// use (the empty asm hides that it never changes): kept across the body loop
// the rows' addresses would push x, r and z out of the registers.
// A row's block starts at floor(i / bs) bs: for i < 4,096 and bs <= 8
// (i + 0.5) / bs lies at least 1 / 16 from an integer, far beyond a float's
// rounding of it, so the truncated float quotient is the integer one.
template <int R, int S>
__device__ __forceinline__ void many_block_sweep(const double *__restrict__ Ws, int bs, int t,
                                                 int n, const double *rs, const double *r,
                                                 double *zk, Dd<double> &accz, double *pz) {
  const float inv = 1.0f / (float)bs;
  auto sweep = [&](auto BS) {
    constexpr int bsc = decltype(BS)::value;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      int i = t + k * S;
      if (i < n) {
        asm volatile("" : "+v"(i));
        const int b0 = (int)(((float)i + 0.5f) * inv) * bsc;
        const double z = many_block_z<bsc>(Ws + i * bsc, b0, n, rs);
        accz += r[k] * z;
        zk[k] = z;
        if (pz) pz[i] = z;
      }
    }
  };
  switch (bs) {
    case 1: sweep(std::integral_constant<int, 1>()); break;
    case 2: sweep(std::integral_constant<int, 2>()); break;
    case 3: sweep(std::integral_constant<int, 3>()); break;
    case 4: sweep(std::integral_constant<int, 4>()); break;
    case 5: sweep(std::integral_constant<int, 5>()); break;
    case 6: sweep(std::integral_constant<int, 6>()); break;
    case 7: sweep(std::integral_constant<int, 7>()); break;
    default: sweep(std::integral_constant<int, 8>()); break;
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

// ---- the team that runs one system -----------------------------------------
// What many_cg_body asks of the threads that share a system: who I am (me; my
// rows are me, me + S, ...), which systems the team takes (first, step), what
// separates an LDS write from its read by another thread (sync where both forms
// need a point, order where a workgroup sum's barrier already serves), how a
// dot is summed (sum, sum2; red + at: the staging, which only the workgroup
// uses) and how a bad diagonal's verdict reaches every thread (vote).

// A workgroup per system: kBlock threads, R kBlock rows, workgroup barriers.
struct TeamWg {
  static constexpr int S = kBlock;
  static __device__ __forceinline__ int me() { return threadIdx.x; }
  static __device__ __forceinline__ int first() { return blockIdx.x; }
  static __device__ __forceinline__ int step() { return gridDim.x; }
  static __device__ __forceinline__ void sync() { __syncthreads(); }
  static __device__ __forceinline__ void order() {}
  static __device__ __forceinline__ double sum(Dd<double> v, double *red, int at) {
    return many_sum(v, red + at);
  }
  static __device__ __forceinline__ void sum2(Dd<double> u, Dd<double> v, double *red, int at,
                                              double *su, double *sv) {
    many_sum2(u, v, red + at, su, sv);
  }
  // `refused` carries the verdict across the barrier (s + 1 > 0 marks this
  // system alone: no reset). A refused system's path has a sync() of its own,
  // which keeps a thread that is already at the next system from writing the
  // word while another still reads it.
  static __device__ __forceinline__ bool vote(bool bad, int s, int *refused) {
    if (bad) *refused = s + 1;
    __syncthreads();
    return *refused == s + 1;  // uniform: every thread reads it behind the barrier
  }
};

// A wave per system: wave w of workgroup b runs systems 4 b + w, 4 b + w +
// 4 grid, ...; 64 lanes, R kWave rows, p (and m, or the block form's staged r)
// in the wave's own part of the LDS. The four waves of a workgroup never meet:
// there is no workgroup barrier (they run different body counts, so one would
// hang), only wave_order().
struct TeamWave {
  static constexpr int S = kWave;
  static __device__ __forceinline__ int wave() {  // (a scalar: the compiler sees it uniform)
    return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  }
  static __device__ __forceinline__ int me() { return threadIdx.x & (kWave - 1); }
  static __device__ __forceinline__ int first() { return blockIdx.x * kWaves + wave(); }
  static __device__ __forceinline__ int step() { return gridDim.x * kWaves; }
  static __device__ __forceinline__ void sync() { wave_order(); }
  static __device__ __forceinline__ void order() { wave_order(); }
  static __device__ __forceinline__ double sum(Dd<double> v, double *, int) { return wave_dot(v); }
  static __device__ __forceinline__ void sum2(Dd<double> u, Dd<double> v, double *, int,
                                              double *su, double *sv) {
    *su = wave_dot(u);
    *sv = wave_dot(v);
  }
  static __device__ __forceinline__ bool vote(bool bad, int, int *) {
    const bool any = __any(bad);  // uniform: the wave's vote
    wave_order();
    return any;
  }
};

// a system that is not solved: X as given, 0 bodies, NaN r.r and r.z, stop code 3
__device__ __forceinline__ void many_refuse(const ManyArgs &a, int s) {
  a.bodies[s] = 0;
  a.rxr[s] = __builtin_nan("");
  a.rz[s] = __builtin_nan("");
  a.stopped[s] = 3;
}

// The solve, once for both forms: the team's systems one after another, each
// from init to its last body. R rows per thread: n <= R Team::S. p: R Team::S
// doubles of LDS, the gather source. red: the workgroup's reduction stagings.
//
// kManyDiag: diagonal preconditioning (cgx_many_set_precond), statement for statement
// as k_pc_init, update_r_body with ZDiag, k_update_xp_pc and stop_rule
// (cgx_kernels.hip): z_i = m_i * r_i, rounded, never stored beyond the body
// that forms it (it takes Ap's register once r is updated); alpha = rz / p.Ap,
// beta = rz' / rz, r.r and r.z summed behind one barrier, so a body keeps its
// three barriers; the stop rule tests the true r.r. m (mm) is a second R
// Team::S doubles of LDS that a thread reads and writes only at its own rows
// (stride 1, no barrier of its own): a.M's entries (DIAGONAL), or 1 / a_ii
// formed by the row's thread from the values this solve reads (JACOBI, a.M ==
// NULL; the entries with col == row summed from 0 in entry order, as
// k_diag_inv), so a caller who overwrites the values in place never meets a
// stale diagonal. A row without a diagonal entry (JACOBI), or a d (JACOBI) or
// m_i (DIAGONAL) that is not positive and finite, ends that system before
// anything of it is written (many_refuse); the verdict is the team's vote.
// The plain form (kManyPlain) has none of this: every addition is behind
// `if constexpr`.
//
// kManyBlock: block-Jacobi preconditioning (cgx_many_set_block_precond),
// statement for statement as k_pc_init_blk and update_r_blk_body. A block's
// rows belong to different threads (a block across a multiple of Team::S wraps
// from the last thread to thread 0), so the updated r goes through LDS: mm is
// the r staging here (there is no m), published by the barrier of the r.r sum
// (the wave form: by order()); each thread then forms z for its own rows from
// its row of W_s (bs contiguous doubles, read from memory every body) and the
// block's r, keeps it where Ap was, and r.z is a third sum: four barriers a
// body. The sums use three stagings, red[0..8) for p.Ap, red[16..24) for r.r
// and red[24..32) for r.z, each written once a body, so many_sum's rule holds.
// A bad system's verdict comes from the launch before this one (stopped[s]): its
// address is uniform, so is the `continue`, and nothing of that system is
// touched but its four outputs.
template <int R, ManyPc PC, class Team>
__device__ __forceinline__ void many_cg_body(const ManyArgs &a, double *p, double *mm,
                                             double *red, int *refused) {
  constexpr bool DG = PC == kManyDiag, BK = PC == kManyBlock, PCD = PC != kManyPlain;
  constexpr int S = Team::S;
  constexpr int kRed1 = PCD ? 16 : 8;  // the second staging's place in red
  const int t = Team::me(), n = a.n;
  // the pattern is every system's: a thread's row bounds stay in registers
  int e0[R], e1[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int i = t + k * S;
    e0[k] = i < n ? a.rowptr[i] : 0;
    e1[k] = i < n ? a.rowptr[i + 1] : 0;
  }
  for (int s = Team::first(); s < a.nsys; s += Team::step()) {
    const double *__restrict__ val = a.val + (int64_t)s * a.ldv;
    const double *__restrict__ b = a.B + (int64_t)s * a.ldb;
    double *__restrict__ xs = a.X + (int64_t)s * a.ldx;
    if constexpr (BK) {
      if (a.stopped[s] != 0) {  // the verdict; uniform: one address for the team
        if (t == 0) many_refuse(a, s);
        continue;
      }
    }
    double x[R], r[R];
    // ---- init: r = b - A x, p = r, rxr = r.r (k_cg_init) ----
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int i = t + k * S;
      x[k] = i < n ? xs[i] : 0.0;
      if (i < n) p[i] = x[k];  // x through LDS: the init's gather source
    }
    if constexpr (DG) {  // m of the own rows, and the verdict on it
      bool bad = false;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int i = t + k * S;
        if (i < n) {
          double mv;
          if (a.M) {
            mv = a.M[(int64_t)s * a.ldm + i];
            bad = bad || !pc_ok(mv);
          } else {
            double d = 0.0;
            bool found = false;
            for (int e = e0[k]; e < e1[k]; ++e)
              if (a.col[e] == i) {
                d = d + val[e];
                found = true;
              }
            mv = 1.0 / d;
            bad = bad || !found || !pc_ok(d);
          }
          mm[i] = mv;
        }
      }
      if (Team::vote(bad, s, refused)) {  // (its point is the one below: x is in p)
        if (t == 0) many_refuse(a, s);
        Team::sync();  // every read of the verdict, before the next system's
        continue;      // (p holds x, which nobody gathered: the next system overwrites it)
      }
    } else {
      Team::sync();  // x is in p
    }
    Dd<double> acc(0.0);
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int i = t + k * S;
      double sum = 0.0;
      for (int e = e0[k]; e < e1[k]; ++e) sum = sum + val[e] * p[a.col[e]];
      r[k] = 0.0;
      if (i < n) {
        r[k] = b[i] - sum;
        acc += r[k] * r[k];
        if constexpr (BK) mm[i] = r[k];  // staged for the blocks' other rows
      }
    }
    Team::sync();  // every gather of x is done: p may be overwritten
    double rxr, rz = 0.0;
    if constexpr (BK) {  // p = z = M^-1 r, rz = r.z (k_pc_init_blk)
      Dd<double> accz(0.0);
      double z0[R];
      many_block_sweep<R, S>(a.M + (int64_t)s * a.ldm, a.bs, t, n, mm, r, z0, accz, p);
      Team::sum2(acc, accz, red, kRed1, &rxr, &rz);
    } else if constexpr (DG) {  // p = m o r, rz = r.(m o r) (k_pc_init)
      Dd<double> accz(0.0);
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int i = t + k * S;
        if (i < n) {
          const double z = mm[i] * r[k];
          p[i] = z;
          accz += r[k] * z;
        }
      }
      Team::sum2(acc, accz, red, kRed1, &rxr, &rz);
    } else {
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int i = t + k * S;
        if (i < n) p[i] = r[k];
      }
      rxr = Team::sum(acc, red, kRed1);
    }
    Team::order();  // p is written (a workgroup sum's barrier publishes it too)
    long long bodies = 0;
    int stopped = 0;
    // ---- the bodies ----
    for (;;) {
      // Ap = A p and p.Ap (k_spmv_dot)
      double Ap[R];
      acc = Dd<double>(0.0);
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int i = t + k * S;
        double sum = 0.0;
        for (int e = e0[k]; e < e1[k]; ++e) sum = sum + val[e] * p[a.col[e]];
        Ap[k] = sum;
        if (i < n) acc += sum * p[i];
      }
      const double pAp = Team::sum(acc, red, 0);
      const double alpha = (PCD ? rz : rxr) / pAp;
      // r -= alpha Ap and r.r (k_update_r); PC: r.z in the same sweep, z
      // kept where Ap was (update_r_body, ZDiag)
      acc = Dd<double>(0.0);
      double rr, rzn = 0.0;
      if constexpr (BK) {  // (update_r_blk_body)
#pragma unroll
        for (int k = 0; k < R; ++k) {
          const int i = t + k * S;
          if (i < n) {
            r[k] = r[k] - alpha * Ap[k];
            acc += r[k] * r[k];
            mm[i] = r[k];
          }
        }
        rr = Team::sum(acc, red, kRed1);
        Team::order();  // the staged r is written (a workgroup sum's barrier publishes it too)
        Dd<double> accz(0.0);
        many_block_sweep<R, S>(a.M + (int64_t)s * a.ldm, a.bs, t, n, mm, r, Ap, accz, nullptr);
        rzn = Team::sum(accz, red, kRed1 + 8);
      } else if constexpr (DG) {
        Dd<double> accz(0.0);
#pragma unroll
        for (int k = 0; k < R; ++k) {
          const int i = t + k * S;
          if (i < n) {
            r[k] = r[k] - alpha * Ap[k];
            acc += r[k] * r[k];
            const double z = mm[i] * r[k];
            accz += r[k] * z;
            Ap[k] = z;
          }
        }
        Team::sum2(acc, accz, red, kRed1, &rr, &rzn);
      } else {
#pragma unroll
        for (int k = 0; k < R; ++k) {
          const int i = t + k * S;
          if (i < n) {
            r[k] = r[k] - alpha * Ap[k];
            acc += r[k] * r[k];
          }
        }
        rr = Team::sum(acc, red, kRed1);
      }
      const double beta = PCD ? rzn / rz : rr / rxr;
      // x += alpha p; p = r + beta p (PC: m o r + beta p); the stop rule
      // (k_update_xp, k_update_xp_pc). Every gather of this body's p is done:
      // in a workgroup it lies before the sums' barriers above.
      Team::order();
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int i = t + k * S;
        if (i < n) {
          const double pv = p[i];
          x[k] = x[k] + alpha * pv;
          p[i] = (PCD ? Ap[k] : r[k]) + beta * pv;
        }
      }
      ++bodies;
      const bool cond = isnan(rxr) || sqrt(rxr) <= a.tol;  // Q5: the r.r the body began with
      const bool cont = !cond && bodies < a.cap;
      stopped = cond ? 1 : (cont ? 0 : 2);
      rxr = rr;
      if constexpr (PCD) rz = rzn;
      Team::sync();  // the new p, before the next gather (or the next system's x)
      if (!cont) break;
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int i = t + k * S;
      if (i < n) xs[i] = x[k];
    }
    if (t == 0) {
      a.bodies[s] = bodies;
      a.rxr[s] = rxr;
      a.stopped[s] = stopped;
      if constexpr (PCD) a.rz[s] = rz;
    }
  }
}

// A workgroup per system. LDS: p (R kBlock doubles) and two reduction
// stagings; preconditioned: m, or the block form's staged r, and wider
// stagings; the diagonal form: the verdict word.
template <int R, ManyPc PC>
__global__ __launch_bounds__(kBlock) void k_many_cg(ManyArgs a) {
  constexpr bool DG = PC == kManyDiag, BK = PC == kManyBlock, PCD = PC != kManyPlain;
  __shared__ double p[R * kBlock];
  __shared__ double red[2][PCD ? 16 : 8];
  // (unused, and dropped, in the plain form; the block form's staged r, read past its end)
  __shared__ double mm[PCD ? R * kBlock + (BK ? kManyStagePad : 0) : 1];
  __shared__ int refused;                      // (the same; the diagonal form's alone)
  if constexpr (DG) {
    if (threadIdx.x == 0) refused = 0;
    __syncthreads();
  }
  many_cg_body<R, PC, TeamWg>(a, p, mm, &red[0][0], &refused);
}

// A wave per system (n <= R kWave): the same function, four independent
// solves per workgroup, each in its own part of the LDS.
template <int R, ManyPc PC>
__global__ __launch_bounds__(kBlock) void k_many_cg_wave(ManyArgs a) {
  constexpr bool BK = PC == kManyBlock, PCD = PC != kManyPlain;
  __shared__ double p_all[kWaves * R * kWave];
  // (unused, and dropped, in the plain form; the block form's staged r, read past its end)
  __shared__ double m_all[PCD ? kWaves * R * kWave + (BK ? kManyStagePad : 0) : 1];
  const int w = TeamWave::wave();
  many_cg_body<R, PC, TeamWave>(a, p_all + w * (R * kWave), m_all + (PCD ? w * (R * kWave) : 0),
                                nullptr, nullptr);
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

// ---- block-Jacobi: the blocks' inverses (cgx_many_set_block_precond) -------
// W_b = (diagonal block b of A_s)^-1 for every system s and block b, one thread
// per (system, block): block_inv_one (cgx_block_inv.h), the function k_block_inv
// (cgx_kernels.hip) calls, here with int indices. System s's W is n x BS
// row-major at out + s ldw; [n BS, ldw) is not written. A pivot that is not
// positive and finite (pc_ok) marks the system: bad[s] = 1, atomically, and the
// block's W holds whatever the statements give.
template <int BS>
__global__ __launch_bounds__(kBlock) void k_many_block_inv(int nsys, int n,
                                                           const int *__restrict__ rowptr,
                                                           const int *__restrict__ col,
                                                           const double *__restrict__ vals,
                                                           int64_t ldv, double *__restrict__ outs,
                                                           int64_t ldw, int *bad) {
  const int nb = (n + BS - 1) / BS;
  const int64_t items = (int64_t)nsys * nb, stride = (int64_t)gridDim.x * kBlock;
  for (int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x; it < items; it += stride) {
    const int s = (int)(it / nb);
    const int b0 = (int)(it - (int64_t)s * nb) * BS;
    const double *__restrict__ val = vals + (int64_t)s * ldv;
    double *__restrict__ out = outs + (int64_t)s * ldw;
    const int m = min(BS, n - b0);  // rows of this block
    if (!block_inv_one<BS, int>(rowptr, col, val, out, b0, m)) atomicOr(&bad[s], 1);
  }
}

// A caller's W (CGX_BLOCK_GIVEN), one thread per (system, row), k_block_check's
// verdict (block_row_ok, cgx_block_inv.h): every entry of a real column finite,
// W_b[i, i] positive and finite; a row that fails marks its system, bad[s] = 1,
// atomically.
__global__ __launch_bounds__(kBlock) void k_many_block_check(int nsys, int n, int bs,
                                                             const double *__restrict__ Ws,
                                                             int64_t ldw, int *bad) {
  const int64_t items = (int64_t)nsys * n, stride = (int64_t)gridDim.x * kBlock;
  for (int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x; it < items; it += stride) {
    const int s = (int)(it / n);
    const int i = (int)(it - (int64_t)s * n);
    const double *__restrict__ w = Ws + (int64_t)s * ldw + (int64_t)i * bs;
    const int b0 = (i / bs) * bs;
    const int nc = min(bs, n - b0);
    if (!block_row_ok(w, i - b0, nc)) atomicOr(&bad[s], 1);
  }
}

int many_rows_per_thread(int64_t n) {
  int r = 1;
  while ((int64_t)r * kBlock < n) r *= 2;
  return r;
}

template <ManyPc PC> const void *many_kernel_of(int r) {
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

template <ManyPc PC> const void *many_wave_kernel_of(int r) {
  switch (r) {
    case 1: return reinterpret_cast<const void *>(&k_many_cg_wave<1, PC>);
    case 2: return reinterpret_cast<const void *>(&k_many_cg_wave<2, PC>);
    case 4: return reinterpret_cast<const void *>(&k_many_cg_wave<4, PC>);
    default: return nullptr;
  }
}

const void *many_kernel(int r, ManyPc pc, bool wave) {
  if (wave)
    return pc == kManyBlock  ? many_wave_kernel_of<kManyBlock>(r)
           : pc == kManyDiag ? many_wave_kernel_of<kManyDiag>(r)
                             : many_wave_kernel_of<kManyPlain>(r);
  return pc == kManyBlock  ? many_kernel_of<kManyBlock>(r)
         : pc == kManyDiag ? many_kernel_of<kManyDiag>(r)
                           : many_kernel_of<kManyPlain>(r);
}

// workgroups of k_many_cg<r, pc> (wave: k_many_cg_wave<r, pc>) resident on the
// device at once (occupancy x CUs; 0: unknown), as spmv_dot_resident
int many_resident(int r, ManyPc pc, bool wave) {
  static std::mutex mu;
  // (device, 8 r + 4 with the wave form + pc) -> workgroups
  static std::map<std::pair<int, int>, int> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  std::lock_guard<std::mutex> lk(mu);
  const std::pair<int, int> key{dev, 8 * r + (wave ? 4 : 0) + (int)pc};
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
  // cgx_many_set_block_precond (excludes the diagonal one: at most one is set)
  int blk_kind = CGX_BLOCK_NONE, blk_bs = 0;
  const double *d_W = nullptr;  // GIVEN: the caller's
  int64_t ldw = 0;
  double *d_Wown = nullptr;     // JACOBI: nsys x n blk_bs, refilled by every solve
  bool bad_valid = false;       // h_stopped holds the last cgx_many_block_inv's verdicts
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
  void *dev[] = {m->d_bodies, m->d_rxr, m->d_rz, m->d_stopped, m->d_Wown};
  for (void *p : dev)
    if (p) (void)hipFree(p);
  void *host[] = {m->h_bodies, m->h_rxr, m->h_rz, m->h_stopped};
  for (void *p : host)
    if (p) (void)hipHostFree(p);
  if (m->ctx) ctx_release(m->ctx);
  delete m;
}

// what the next solve's kernel does with r
ManyPc many_pc(const cgx_many *m) {
  if (m->blk_kind != CGX_BLOCK_NONE) return kManyBlock;
  return m->precond != CGX_PRECOND_NONE ? kManyDiag : kManyPlain;
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

// back to no block preconditioner; its workspace goes
void many_drop_block(cgx_many *m) {
  if (m->d_Wown) {
    (void)hipStreamSynchronize(m->ctx->stream);
    (void)hipFree(m->d_Wown);
    m->d_Wown = nullptr;
  }
  m->blk_kind = CGX_BLOCK_NONE;
  m->blk_bs = 0;
  m->d_W = nullptr;
  m->ldw = 0;
}

int many_elem_grid(int64_t items) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((items + kBlock - 1) / kBlock, kMaxGrid));
}

// every system's W into out (system s at out + s ldw), bad[s] set where a block is bad
hipError_t many_block_fill(const cgx_many *m, int bs, double *out, int64_t ldw, int *bad,
                           hipStream_t s) {
  const int n = (int)m->n, nsys = (int)m->nsys;
  const dim3 grid(many_elem_grid((int64_t)nsys * ((n + bs - 1) / bs))), block(kBlock);
#define CGX_MANY_BINV(BS)                                                                    \
  case BS:                                                                                   \
    hipLaunchKernelGGL(k_many_block_inv<BS>, grid, block, 0, s, nsys, n, m->rowptr, m->col,  \
                       m->val, m->ldv, out, ldw, bad);                                       \
    break
  switch (bs) {
    CGX_MANY_BINV(1);
    CGX_MANY_BINV(2);
    CGX_MANY_BINV(3);
    CGX_MANY_BINV(4);
    CGX_MANY_BINV(5);
    CGX_MANY_BINV(6);
    CGX_MANY_BINV(7);
    CGX_MANY_BINV(8);
    default: return hipErrorInvalidValue;
  }
#undef CGX_MANY_BINV
  return hipGetLastError();
}

int many_grid(const cgx_many *m) {
  const bool wave = many_form(m) == CGX_MANY_FORM_WAVE;
  int64_t g = wave ? (m->nsys + kWaves - 1) / kWaves : m->nsys;
  const int res = many_resident(many_rows(m), many_pc(m), wave);
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
  const ManyPc kind = many_pc(m);
  const bool pc = kind != kManyPlain;
  const bool wave = many_form(m) == CGX_MANY_FORM_WAVE;
  const void *kernel = many_kernel(many_rows(m), kind, wave);
  CGX_REQUIRE(kernel, CGX_EUNSUPPORTED,
              "cgx_many_solve: no kernel is built for %d rows per %s (n %lld)", many_rows(m),
              wave ? "lane" : "thread", (long long)n);
  a.M = m->precond == CGX_PRECOND_DIAGONAL ? m->d_M : nullptr;
  a.ldm = m->ldm;
  a.rz = m->d_rz;
  a.bs = m->blk_bs;
  m->rz_valid = false;
  m->bad_valid = false;
  if (kind == kManyBlock) {  // the verdicts, and under JACOBI this solve's W, in launches before
    CGX_HIP(hipMemsetAsync(m->d_stopped, 0, (size_t)m->nsys * sizeof(int), s));
    if (m->blk_kind == CGX_BLOCK_JACOBI) {
      a.M = m->d_Wown;
      a.ldm = n * m->blk_bs;
      CGX_HIP(many_block_fill(m, m->blk_bs, m->d_Wown, a.ldm, m->d_stopped, s));
    } else {
      a.M = m->d_W;
      a.ldm = m->ldw;
      hipLaunchKernelGGL(k_many_block_check, dim3(many_elem_grid(m->nsys * n)), dim3(kBlock), 0,
                         s, (int)m->nsys, (int)n, m->blk_bs, m->d_W, m->ldw, m->d_stopped);
      CGX_HIP(hipGetLastError());
    }
  }
  const dim3 grid(many_grid(m)), block(kBlock);
  void *args[] = {&a};
  CGX_HIP(hipLaunchKernel(kernel, grid, block, args, 0, s));
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
  if (m->blk_kind != CGX_BLOCK_NONE) many_drop_block(m);  // either call replaces the other's
  m->precond = kind;
  m->d_M = kind == CGX_PRECOND_DIAGONAL ? (const double *)d_M : nullptr;
  m->ldm = kind == CGX_PRECOND_DIAGONAL ? ldm : 0;
  m->rz_valid = false;
  return CGX_OK;
}

extern "C" int cgx_many_set_block_precond(cgx_many *m, int kind, int bs, const void *d_W,
                                          int64_t ldw) {
  CGX_REQUIRE(kind == CGX_BLOCK_NONE || kind == CGX_BLOCK_JACOBI || kind == CGX_BLOCK_GIVEN,
              CGX_EINVAL, "cgx_many_set_block_precond: unknown kind %d", kind);
  if (kind != CGX_BLOCK_NONE)
    CGX_REQUIRE(bs >= 1 && bs <= 8, CGX_EINVAL,
                "cgx_many_set_block_precond: block size %d is outside 1..8", bs);
  if (kind == CGX_BLOCK_GIVEN) {
    CGX_REQUIRE(d_W, CGX_EINVAL, "cgx_many_set_block_precond: GIVEN needs d_W, which is NULL");
    CGX_REQUIRE(((uintptr_t)d_W & 7) == 0, CGX_EINVAL,
                "cgx_many_set_block_precond: d_W must be 8-byte aligned");
  }
  CGX_REQUIRE(m, CGX_EINVAL, "cgx_many_set_block_precond: NULL handle");
  if (kind == CGX_BLOCK_GIVEN)
    CGX_REQUIRE(ldw >= m->n * bs, CGX_EINVAL,
                "cgx_many_set_block_precond: ldw %lld is below n * bs = %lld", (long long)ldw,
                (long long)(m->n * bs));
  if (kind != CGX_BLOCK_NONE) {
    DeviceGuard g(m->ctx->device);
    double *own = nullptr;
    hipError_t e = hipSuccess;
    if (kind == CGX_BLOCK_JACOBI &&
        !(m->blk_kind == CGX_BLOCK_JACOBI && m->blk_bs == bs))  // (else: the one it has)
      e = hipMalloc((void **)&own, (size_t)m->nsys * (size_t)m->n * bs * sizeof(double));
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      set_error("cgx_many_set_block_precond: out of memory (nsys=%lld, n=%lld, bs=%d)",
                (long long)m->nsys, (long long)m->n, bs);
      return CGX_ENOMEM;
    }
    if (e != hipSuccess) return hip_fail(e, "cgx_many_set_block_precond");
    if (own || kind == CGX_BLOCK_GIVEN) {
      CGX_HIP(hipStreamSynchronize(m->ctx->stream));  // (no solve is in flight: they block)
      if (m->d_Wown) (void)hipFree(m->d_Wown);
      m->d_Wown = own;
    }
  } else {
    many_drop_block(m);
  }
  m->blk_kind = kind;
  m->blk_bs = kind == CGX_BLOCK_NONE ? 0 : bs;
  m->d_W = kind == CGX_BLOCK_GIVEN ? (const double *)d_W : nullptr;
  m->ldw = kind == CGX_BLOCK_GIVEN ? ldw : 0;
  m->precond = CGX_PRECOND_NONE;
  m->d_M = nullptr;
  m->ldm = 0;
  m->rz_valid = false;
  return CGX_OK;
}

extern "C" int cgx_many_get_block_precond(cgx_many *m, int *kind, int *bs) {
  CGX_REQUIRE(m, CGX_EINVAL, "cgx_many_get_block_precond: NULL handle");
  if (kind) *kind = m->blk_kind;
  if (bs) *bs = m->blk_bs;
  return CGX_OK;
}

extern "C" int cgx_many_block_inv(cgx_many *m, int bs, void *d_W, int64_t ldw, int64_t *n_bad,
                                  int64_t *first_bad) {
  CGX_REQUIRE(bs >= 1 && bs <= 8, CGX_EINVAL, "cgx_many_block_inv: block size %d is outside 1..8",
              bs);
  CGX_REQUIRE(d_W, CGX_EINVAL, "cgx_many_block_inv: d_W is NULL");
  CGX_REQUIRE(((uintptr_t)d_W & 7) == 0, CGX_EINVAL,
              "cgx_many_block_inv: d_W must be 8-byte aligned");
  CGX_REQUIRE(m, CGX_EINVAL, "cgx_many_block_inv: NULL handle");
  CGX_REQUIRE(ldw >= m->n * bs, CGX_EINVAL,
              "cgx_many_block_inv: ldw %lld is below n * bs = %lld", (long long)ldw,
              (long long)(m->n * bs));
  DeviceGuard g(m->ctx->device);
  hipStream_t s = m->ctx->stream;
  const size_t ns = (size_t)m->nsys;
  m->bad_valid = false;
  CGX_HIP(hipMemsetAsync(m->d_stopped, 0, ns * sizeof(int), s));  // (a solve's scratch: free here)
  CGX_HIP(many_block_fill(m, bs, (double *)d_W, ldw, m->d_stopped, s));
  CGX_HIP(hipMemcpyAsync(m->h_stopped, m->d_stopped, ns * sizeof(int), hipMemcpyDeviceToHost, s));
  CGX_HIP(hipStreamSynchronize(s));
  int64_t nbad = 0, first = -1;
  for (size_t i = 0; i < ns; ++i)
    if (m->h_stopped[i]) {
      if (first < 0) first = (int64_t)i;
      ++nbad;
    }
  if (n_bad) *n_bad = nbad;
  if (first_bad) *first_bad = first;
  m->bad_valid = true;
  return CGX_OK;
}

extern "C" int cgx_many_block_bad(cgx_many *m, int *bad_out) {
  CGX_REQUIRE(m && bad_out, CGX_EINVAL, "cgx_many_block_bad: NULL argument");
  CGX_REQUIRE(m->bad_valid, CGX_ESTATE,
              "cgx_many_block_bad: no cgx_many_block_inv has run since the last solve");
  for (int64_t i = 0; i < m->nsys; ++i) bad_out[i] = m->h_stopped[i] != 0;
  return CGX_OK;
}

extern "C" int cgx_many_get_precond(cgx_many *m, int *kind) {
  CGX_REQUIRE(m && kind, CGX_EINVAL, "cgx_many_get_precond: NULL argument");
  *kind = m->precond;
  return CGX_OK;
}

extern "C" int cgx_many_rz(cgx_many *m, double *rz_out) {
  CGX_REQUIRE(m && rz_out, CGX_EINVAL, "cgx_many_rz: NULL argument");
  CGX_REQUIRE(many_pc(m) != kManyPlain, CGX_ESTATE, "cgx_many_rz: no preconditioner is set");
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
    const ManyPc pc = many_pc(m);
    if (many_form(m) == CGX_MANY_FORM_WAVE)  // four waves' p; preconditioned: their m (block
                                             // form: their staged r) too
      *lds_bytes = ((int64_t)(pc == kManyPlain ? 1 : 2) * kWaves * many_rows(m) * kWave +
                    (pc == kManyBlock ? kManyStagePad : 0)) * (int64_t)sizeof(double);
    else  // p and the stagings; preconditioned: m (block form: the staged r), wider stagings
          // and, in the diagonal form, the verdict word
      *lds_bytes = pc == kManyPlain
                       ? ((int64_t)m->r * kBlock + 16) * (int64_t)sizeof(double)
                       : ((int64_t)2 * m->r * kBlock + 32) * (int64_t)sizeof(double) +
                             (pc == kManyDiag ? 8 : kManyStagePad * (int64_t)sizeof(double));
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
