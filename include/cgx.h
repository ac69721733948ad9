/*
 * cgx.h — C ABI of libcgx.so, the MI355X (gfx950) conjugate-gradient engine.
 *
 * The reference (XeniaHerr/ConjugateGradient) has no FFI: its boundary is the
 * header-only C++ template API in src/CG.hpp, src/VectorOperations.hpp and
 * src/LinearAlgebraTypes.hpp. Our drop-in copies of those
 * headers (include/CG.hpp, include/VectorOperations.hpp,
 * include/LinearAlgebraTypes.hpp) are thin C++ over the entry points below;
 * each entry point names the reference interface it replaces.
 *
 * Conventions
 *   - Every function returns int: 0 = CGX_OK, otherwise an error code; the
 *     message is in cgx_last_error() (thread-local).
 *   - Pointers named d_* are device pointers (hipMalloc'ed, e.g. by cgx_alloc);
 *     h_* are host pointers. Sizes are element counts unless named *_bytes.
 *   - dtype: CGX_F64 or CGX_F32 (the reference's DT template parameter).
 *   - All kernels are asynchronous on the context's stream (the SYCL queue's
 *     role, CG.hpp:590); functions documented as "blocking" drain it, as the
 *     reference's executeQueue() does (CG.hpp:561-578).
 *   - Indices are int32 (Matrix<DT> stores int columns/rows,
 *     LinearAlgebraTypes.hpp:620-622).
 */
#ifndef CGX_H
#define CGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { CGX_OK = 0, CGX_EINVAL = 1, CGX_EHIP = 2, CGX_ENOMEM = 3, CGX_ESTATE = 4,
       CGX_ENCCL = 5, CGX_EUNSUPPORTED = 6 };
enum { CGX_F64 = 0, CGX_F32 = 1 };

typedef struct cgx_ctx cgx_ctx; /* device + stream (+ optional RCCL comm)      */
typedef struct cgx_csr cgx_csr; /* CSR matrix view + SpMV row-block schedule  */
typedef struct cgx_cg cgx_cg;   /* fused CG solver state                      */

/* ---- errors / version ---------------------------------------------------- */
const char *cgx_last_error(void);
const char *cgx_version(void);
/* Number of visible HIP devices (0 when none; never fails on a CPU host). */
int cgx_device_count(int *count);

/* ---- context: replaces the sycl::queue (CG.hpp:61,70-77,590) -------------- */
int cgx_create(int device, cgx_ctx **out);          /* CG::createCG :70-77   */
int cgx_destroy(cgx_ctx *ctx);
int cgx_sync(cgx_ctx *ctx);                          /* executeQueue :561-578 */
int cgx_get_stream(cgx_ctx *ctx, void **hip_stream);
int cgx_get_device(cgx_ctx *ctx, int *device);
/* the device's max_work_group_size (VectorOperations.hpp:478-487 queries it
 * through sycl::info::device::max_work_group_size) */
int cgx_max_work_group_size(cgx_ctx *ctx, int *size);

/* ---- memory: replaces sycl::malloc_device/free/copy/fill ------------------
 * (LinearAlgebraTypes.hpp:43-49 Asycl_deleter, :109-119 Matrix::init,
 *  :160-183 Vector::init_empty/init, :217-224 Scalar::init) */
int cgx_alloc(cgx_ctx *ctx, size_t bytes, void **d_out);
int cgx_free(cgx_ctx *ctx, void *d_ptr);
int cgx_h2d(cgx_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);     /* blocking */
int cgx_d2h(cgx_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);     /* blocking */
int cgx_d2d(cgx_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);     /* async    */
int cgx_h2d_async(cgx_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int cgx_fill(cgx_ctx *ctx, int dtype, void *d_ptr, double value, size_t n);  /* async    */

/* ---- CSR matrix (Matrix<DT>, LinearAlgebraTypes.hpp:57-132) ---------------
 * The device arrays stay owned by the caller (the Matrix object's
 * shared_ptrs); cgx_csr only adds the SpMV schedule. h_rowptr may be NULL (it
 * is then read back from the device). */
int cgx_csr_create(cgx_ctx *ctx, int64_t n, int64_t nnz, const int *d_rowptr,
                   const int *d_col, const void *d_val, int dtype,
                   const int *h_rowptr, cgx_csr **out);
int cgx_csr_destroy(cgx_csr *csr);
int cgx_csr_info(cgx_csr *csr, int64_t *n, int64_t *nnz, int64_t *row_blocks,
                 int *max_row_nnz);
/* Rebuild the SpMV schedule for row blocks of `tile` entries (2048, the
 * default, or 1024 with at most 128 rows). Blocking. */
int cgx_csr_set_tile(cgx_csr *csr, int tile);
/* CSR-stream's row-block visit order. A matrix from a 3-D grid gathers p one
 * plane (D rows) away from every row; walking chunks of `chunk_rows` rows of a
 * plane through the planes of each XCD's eighth keeps those p lines in the
 * XCD's L2. chunk_rows: 0 the natural order, -1 automatic (an order only
 * where a dominant offset D makes two planes of stream overflow half an L2),
 * > 0 that chunk (CGX_EINVAL without a dominant offset). The result is the
 * same for any order; only the p.Ap partials group differently. Blocking.
 * Replaces nothing in the reference: a schedule of VectorOperations.hpp:
 * 438-466's SpMV. */
int cgx_csr_set_block_order(cgx_csr *csr, int chunk_rows);
/* The order in use: the plane offset D and the chunk rows (0 / 0: natural). */
int cgx_csr_block_order_info(cgx_csr *csr, int *D, int *chunk_rows);
/* SpMV variant the matrix's launches use: the one cgx_csr_create picked by
 * timing the candidate kernels on the device ($CGX_SPMV_VARIANT or
 * cgx_csr_set_variant override), resolved against the matrix's layout
 * (e.g. 6146 = SELL, 2 rows per lane, non-temporal loads). */
int cgx_csr_variant(cgx_csr *csr, int *variant);
/* Force the SpMV variant of this matrix (0: size heuristic). Variants with
 * bit 2048 use the SELL-64 copy cgx_csr_create builds for matrices whose
 * slices of 64 rows have at most 64 distinct (col - row) offsets; they fail
 * with CGX_EUNSUPPORTED when the matrix has none (or it was freed because
 * the autotune chose a CSR-stream variant). */
int cgx_csr_set_variant(cgx_csr *csr, int variant);
/* Rebuild the SELL copy: 1 or 2 = dictionary SELL with 1 or 2 rows per
 * lane (slices of 64 or 128 rows), 3 = SELL-P (slices of 128 rows, one
 * offset pattern per slice, one slot mask per row), 0 = drop it. A matrix
 * that does not qualify ends without one. Blocking. */
int cgx_csr_set_sell(cgx_csr *csr, int rows_per_lane);
/* The matrix's SELL layout (0 none, 1 / 2 dictionary SELL with that many
 * rows per lane, 3 SELL-P) and its padded entry count. */
int cgx_csr_sell_info(cgx_csr *csr, int *has_sell, int64_t *padded_entries);
/* The SELL walk's slice visit order: 1 when the slices are walked in
 * XCD-local chunks of z-planes (automatic where planes span >= 1,024
 * slices), 2 when a partitioned matrix's interior slice
 * list is, 0 for the natural order. */
int cgx_csr_visit_order(cgx_csr *csr, int *ordered);
/* Distinct values of the matrix's SELL-P value codes (variant bit 32768, kVc in cgx_variant.h:
 * one code byte per slot into a dictionary of at most 255 values, built by
 * cgx_csr_create when the SELL-P copy exists and the matrix has that few
 * distinct values; $CGX_VALUE_CODES=0 disables it), 0 when it has none. */
int cgx_csr_value_codes(cgx_csr *csr, int *n_values);
/* Value-code templates (variant bit 8388608, kVT): the number of distinct 4-bit
 * code chunks stored once and read from LDS, and the slices that use one
 * (0 / 0: none). */
int cgx_csr_templates(cgx_csr *csr, int *n_templates, int64_t *slices);
/* The lean stencil walk (variant bit 33554432, kVL; kept by the autotune where it
 * wins or requested with cgx_csr_set_variant): slices whose pattern is a
 * subset of one stencil's {-D, -a, -1, 0, +1, +a, +D} and whose template
 * chunk holds one value per slot, summed from per-class values with no
 * per-row stream. *classes: distinct (template, pattern) classes, *slices:
 * slices that run it, *grid: its launch's workgroups, *D / *a: the stencil's
 * offsets, *chunked: 1 when its waves walk chunks of a plane through the
 * planes (planes wider than a grid step; all 0 when the matrix has none
 * built). Replaces nothing in the reference: a format of
 * VectorOperations.hpp:438-466's SpMV. */
int cgx_csr_lean_info(cgx_csr *csr, int *classes, int64_t *slices, int *grid, int *D, int *a,
                      int *chunked);
/* Which form of the plane-per-step walk the recomputed-Ap modes take on this
 * matrix: *tile = 1 when the tile walk applies (modes 6 and 7's first kernels:
 * one wave per x-line, the planes it needs in flight ahead of its sums),
 * *ring = 1 when mode 7's first kernel runs its ring form (a workgroup shares
 * a plane's lines through LDS), which is also where auto resolves to mode 7
 * for f64. Read at the call: $CGX_LEAN_RING=0 keeps the per-wave tile form. */
int cgx_csr_lean_ring(cgx_csr *csr, int *tile, int *ring);
/* The SpMV autotune's record of this matrix (cgx_csr_create /
 * cgx_csr_create_dist): every form it timed, how it was timed and its median
 * µs per launch over the interleaved rounds; *count = the record's length
 * (0 when a variant was forced or the matrix is small enough for the size
 * rule). Up to `cap` entries are written. A form displaces the preferred
 * (more specialised) one only when at least 3% faster. Replaces nothing in
 * the reference (its SpMV has one form, VectorOperations.hpp:438-466). */
#define CGX_TUNE_DOT 0          /* k_spmv_dot over the whole matrix */
#define CGX_TUNE_DOT_INTERIOR 1 /* k_spmv_dot over a split matrix's interior slices */
#define CGX_TUNE_FD 2           /* k_spmv_fd (mode 4's SpMV; 2-D plane march) */
#define CGX_TUNE_LEAN 3         /* the lean walk over the whole matrix */
#define CGX_TUNE_LEAN_INTERIOR 4 /* the lean walk over a split matrix's interior */
#define CGX_TUNE_LEAN_TEAM 5     /* mode 4's fused walk, team form (cgx_csr_set_lean_team) */
#define CGX_TUNE_INCUMBENT 6     /* the pick before the lean walk's rounds, re-timed in them */
#define CGX_TUNE_BOUNDARY 7      /* a split matrix's boundary rows (CSR-stream launch), added
                                    to its interior forms' times before the pick */
int cgx_csr_autotune_record(cgx_csr *csr, int *variants, int *kinds, float *us, int cap,
                            int *count);
/* The setup cost of cgx_csr_create / cgx_csr_create_dist by phase, wall
 * milliseconds (*count = 6; up to `cap` written): [0] row-block schedule (and
 * the halo plan of a partitioned matrix), [1] SELL plan and pack, [2] value
 * codes and templates, [3] interior / boundary split, [4] SpMV autotune
 * (lean layouts included), [5] the rest. Replaces nothing in the reference
 * (Matrix::init only uploads, LinearAlgebraTypes.hpp:101-121). */
int cgx_csr_setup_times(cgx_csr *csr, double *ms, int cap, int *count);
/* Mode 4's fused lean walk (k_spmv_fd_lean) in its team form: 1,024-thread
 * workgroups whose 16 waves share their slices' formed p_k neighbour pairs
 * through LDS instead of gathering r and p_{k-1} for them.
 * on = 1 selects it (grid / 4 workgroups), 0 the 4-wave form; the plain
 * SpMV always runs the 4-wave walk. CGX_EUNSUPPORTED without an f64
 * whole-matrix lean layout whose grid is a multiple of 32. The autotune
 * decides it at creation. Replaces nothing in the reference
 * (VectorOperations.hpp:438-466 has one SpMV form). */
int cgx_csr_set_lean_team(cgx_csr *csr, int on);
int cgx_csr_lean_team(cgx_csr *csr, int *on);
/* The plane-march plan of the matrix's SELL-P copy (variant bit 2097152, kMarch):
 * *stride = slices (of 128 rows) between a slice and its +-D neighbour
 * (0: the dominant slice pattern is not a 7-point / 5-point stencil with D
 * a multiple of 128 rows, and the bit is ignored), *offset_a = the 3-D
 * form's +-a offset (0: 2-D form), *run_planes = planes per run (0: chosen
 * per launch to fill the grid). */
int cgx_csr_march_info(cgx_csr *csr, int *stride, int *offset_a, int *run_planes);
/* Bytes of the matrix stream one SpMV launch in the matrix's current
 * variant reads (values, indices / codes / masks, slice descriptors;
 * vectors excluded): the format's algorithmic bytes, next to CSR's
 * 12 nnz + 4 (n + 1) in fp64. */
int cgx_csr_stream_bytes(cgx_csr *csr, int64_t *bytes);

/* ---- VectorOperations<DT> (src/VectorOperations.hpp) ----------------------
 * Scalars are DEVICE pointers, as in the reference (Scalar<DT>::ptr()). */
/* y = A x over all rows; `count` must equal A.N() (spmv :438-466, assert :444) */
int cgx_spmv(cgx_ctx *ctx, cgx_csr *A, const void *d_x, void *d_y, int64_t count);
/* *d_res += x.y  (dot_product_trivial :287-309: accumulates, Q4) */
int cgx_dot_acc(cgx_ctx *ctx, int dtype, int64_t n, const void *d_x,
                const void *d_y, void *d_res);
/* *d_res += x.x  (norm :311-331; sum of squares, no sqrt) */
int cgx_norm_acc(cgx_ctx *ctx, int dtype, int64_t n, const void *d_x, void *d_res);
/* res = x + (*d_b) y (sapbx :410-428), res = x - (*d_b) y (sambx :380-397),
 * res = (*d_a) x + (*d_b) y (saxpby :349-367). res may alias x or y. */
int cgx_sapbx(cgx_ctx *ctx, int dtype, int64_t n, const void *d_x,
              const void *d_y, const void *d_b, void *d_res);
int cgx_sambx(cgx_ctx *ctx, int dtype, int64_t n, const void *d_x,
              const void *d_y, const void *d_b, void *d_res);
int cgx_saxpby(cgx_ctx *ctx, int dtype, int64_t n, const void *d_x,
               const void *d_y, const void *d_a, const void *d_b, void *d_res);
/* Device scalar helper: *d_out = *d_num / *d_den (CG.hpp:385-386, :414). */
int cgx_scalar_div(cgx_ctx *ctx, int dtype, const void *d_num, const void *d_den,
                   void *d_out);

/* ---- fused CG: CG<DT>::solve (CG.hpp:255-454) -----------------------------
 * Per iteration three kernels (SpMV+p.Ap, r-update+r.r, x/p-update), device-
 * resident scalars and stop flag; the host polls every few iterations instead
 * of draining the queue every iteration (CG.hpp:425). Iteration semantics are
 * the reference's (Q5): the stop test uses the r.r at the START of the body
 * after the body's x update, NaN stops, at most A.N()+1 bodies. */
int cgx_cg_create(cgx_ctx *ctx, cgx_csr *A, cgx_cg **out);
int cgx_cg_destroy(cgx_cg *cg);
/* Blocking. d_x holds the initial guess (zero it for the reference default)
 * and receives the result. max_bodies < 0 keeps the reference cap N+1;
 * otherwise the cap is min(N+1, max_bodies). */
int cgx_cg_solve(cgx_cg *cg, const void *d_b, void *d_x, double tol,
                 int64_t max_bodies, int64_t *bodies_out, double *rxr_out);
/* Split form used by benchmarks: init (r = b - A x, p = r, rxr = r.r) then
 * run up to `bodies` more loop bodies (stops early on the stop rule). */
int cgx_cg_begin(cgx_cg *cg, const void *d_b, void *d_x, double tol,
                 int64_t max_bodies);
int cgx_cg_run(cgx_cg *cg, int64_t bodies, int64_t *bodies_total, int *stopped);
/* Capture, ahead of time, the hipGraphs a following cgx_cg_run(cg, bodies)
 * replays (chunks of the poll interval from the current slot; a run builds
 * only full chunks itself and launches a shorter tail eagerly). Blocking
 * host work, no kernel runs. Benchmarks call it before a timed run. */
int cgx_cg_prepare(cgx_cg *cg, int64_t bodies);
/* r.r after the last body run so far (the value the reference reads back
 * after its loop, CG.hpp:437-440); blocking. */
int cgx_cg_rxr(cgx_cg *cg, double *rxr);
/* Per-kernel device time, accumulated with HIP events on the solver stream
 * while enabled: avg_ms[0..3] = init, spmv_dot, update_r, update_xp;
 * calls[0..3] = launches timed. */
int cgx_cg_set_kernel_timing(cgx_cg *cg, int enable);
int cgx_cg_kernel_times(cgx_cg *cg, double *avg_ms, int64_t *calls);
/* The same kernels' execution times: event pairs each kernel's dispatch
 * records itself (hipExtLaunchKernel), so without the dispatch latency the
 * pairs of cgx_cg_kernel_times include; the durations rocprofv3 reports.
 * calls[i] = 0 where a launch did not record them. */
int cgx_cg_kernel_exec_times(cgx_cg *cg, double *avg_ms, int64_t *calls);
/* Tuning knobs (0 = default): iterations per host poll; use hipGraph replay. */
int cgx_cg_config(cgx_cg *cg, int poll_every, int use_graph);
/* Iteration structure (before cgx_cg_begin): 0 auto (4 for the 2-D plane
 * march, cache-resident stencil matrices, lean walks of >= 32 M rows and
 * partitioned lean interiors of <= 4 M rows, else 3; the default), 1
 * three kernels
 * (SpMV+p.Ap, r-update+r.r, x/p-update), 2 fused (single device only): two
 * kernels, the x/p update folded into the next iteration's SpMV (p_j =
 * r_j + beta p_old_j computed in the gather), 8 bytes/row less traffic but
 * twice the gathers; 3 three kernels with the x update deferred: p cycles
 * through four buffers and x += a0 p0 + ... + a3 p3 (in order) runs once
 * per four bodies and at the end of each cgx_cg_run (34 N instead of 40 N
 * bytes per body for the x/p update); 4 fused with deferred x (f64,
 * production SpMV formats): two kernels per body, p_k = r +
 * beta p_{k-1} computed where the SpMV reads it and stored once into the
 * p ring, update_r with the stop rule, x from the four p buffers in slot 3
 * (72 N + matrix bytes per body against 78 N in mode 3); on a partitioned
 * matrix it needs the device peer transport and the lean interior walk
 * (three launches: interior walk with the push of the formed p_k, boundary
 * rows, update_r with both all-reduces; x bit-identical to mode 3; auto at
 * <= 4 M rows per rank); 5 persistent body
 * (single device, f64; register forms up to 1024 rows per CU, the streamed form
 * up to 8 x 1024 x min(256, CUs) rows): one launch runs a whole chunk of
 * bodies, each with two grid-wide exchanges of the dot partials instead of
 * three kernel boundaries; Ap bit-identical, the dots summed in another
 * order (x equal to rounding). $CGX_COOP_R picks its rows per thread,
 * $CGX_COOP_STREAM=1 / 0 always / never the streamed form.
 * Mode 6 (round 6; single device, the lean stencil walk): mode 3's body with
 * no Ap vector — kernel 1 walks A p keeping only p.Ap, kernel 2 walks A p
 * again and updates r in its epilogue (8 N bytes written and read less).
 * Mode 7 (single device, f64, a 3-D stencil whose lean layout takes the tile
 * walk): mode 4's body with no Ap vector — kernel 1 forms p_k into the p ring
 * and keeps p.Ap, kernel 2 walks A p_k again, updates r and runs the stop
 * rule; in slot 3 it also applies the group's x updates from the four p
 * buffers, row by row in the same walk (58 N + 2 x matrix bytes per body).
 * Auto takes 7 instead of 6 where kernel 1 runs the ring form of the tile
 * walk (cgx_csr_lean_ring; 256^3: DESIGN.md §5) and 6 for the other
 * whole-matrix lean walks between mode 4's two bounds.
 * The dots are double-length sums (round 6), so modes 1, 3, 4, 6 and 7 give
 * bit-identical x whatever their grids.
 * With a preconditioner set (cgx_cg_set_precond, cgx_cg_set_block_precond)
 * only modes 1 and 3 run:
 * auto resolves to 3 whatever the matrix, and modes 2, 4, 5, 6 and 7 return
 * CGX_EUNSUPPORTED. */
int cgx_cg_set_mode(cgx_cg *cg, int mode);
/* mode 5's launch shape: rows per thread, threads per workgroup (1024),
 * workgroups, and the form: 0 the register form (drained write-through
 * stores), 2 the streamed form (the matrix read every body, entries staged
 * through LDS; $CGX_COOP_STREAM=1 forces it, $CGX_COOP_R its rows per
 * thread) */
int cgx_cg_coop_shape(cgx_cg *cg, int *rows_per_thread, int *threads, int *workgroups,
                      int *form);
/* diagnostics: with $CGX_COOP_TRACE=1 set before mode 5 is chosen, the
 * wall-clock stamps (100 MHz) of the last launch: [workgroup][body 8..15]
 * [phase 0..7] (0 body start, 1 SpMV done, 2 p.Ap partial ready, 3 p.Ap
 * exchanged, 4 r.r partial ready, 5 next gathers done, 6 r.r exchanged) */
int cgx_cg_coop_trace(cgx_cg *cg, uint64_t *host, int64_t words);
/* the iteration structure in effect (1-5; auto resolved) */
int cgx_cg_get_mode(cgx_cg *cg, int *mode);
/* The sweep directions (0: rows low to high, 1: high to low) the body in
 * slot `slot & 3` is enqueued with in the mode in effect, in stream order:
 * *n = the body's launches that take a direction, dirs[0 .. min(*n, cap) - 1]
 * filled. The launches alternate in stream order (launch k of the body in
 * slot s of an L-launch body: (s L + k) & 1), so each starts at the end of the
 * vectors the launch before it left newest in the caches: three launches
 * (modes 1, 3, 6; preconditioned and partitioned bodies) s & 1, 1 - (s & 1),
 * s & 1; the two-kernel bodies on one device (modes 4 and 7) 0, 1 in every
 * slot. Mode 4 on a partitioned matrix keeps the three-launch rule's first
 * two (*n = 2). Modes 2 and 5 sweep forward only: *n = 0. Diagnostics: the
 * directions change no value. */
int cgx_cg_sweep_dirs(cgx_cg *cg, int slot, int *dirs, int cap, int *n);
/* mode 4's fused SpMV grid and the SpMV's: where they are equal mode 4 is
 * bit-identical to mode 1, else equal to rounding (one dot's sum order) */
int cgx_csr_fd_grid(cgx_csr *A, int *fd_grid, int *spmv_grid);

/* ---- diagonal preconditioning (replaces nothing in the reference: CG.hpp's
 * solve is unpreconditioned) ------------------------------------------------
 * PCG with M^-1 = diag(m): z = m o r (element product, rounded) is never
 * stored, it is formed where the kernels hold r. init: p = m o r, rz = r.z;
 * body: alpha = rz / p.Ap, r -= alpha Ap, rr' = r.r and rz' = r.(m o r) in
 * one sweep, x += alpha p, beta = rz' / rz, p = m o r + beta p. tol, the
 * body count, cgx_cg_rxr and cgx_cg_solve's rxr_out keep their meaning: the
 * stop rule tests the true r.r (Q5), not r.z. With m == 1 every value is the
 * plain solver's, bit for bit. The init is two launches (the plain one, then
 * p = m o r with rz), both under index 0 of cgx_cg_kernel_times.
 * Modes 1 and 3, f64 and f32, every SpMV format, on a single device and on
 * partitioned matrices (cgx_csr_create_dist) over every transport of the
 * partitioned solver; mode 0 (auto) resolves to 3 while a preconditioner is
 * set. Modes 2, 4, 5, 6 and 7 return CGX_EUNSUPPORTED, from whichever of
 * cgx_cg_set_mode and cgx_cg_set_precond comes second.
 * Partitioned: m covers the rank's own rows (n_local values); r.z is
 * all-reduced with r.r as one collective of two values, so a body has the
 * plain partitioned body's launches and round trips (tags: p.Ap at base + 1,
 * {r.r, r.z} at base + 2), ranks may mix modes 1 and 3, and cgx_cg_rz,
 * cgx_cg_rxr and cgx_cg_solve's outputs are the world values, identical on
 * every rank. cgx_csr_diag_inv and cgx_cg_set_precond (kinds JACOBI and
 * DIAGONAL) are then COLLECTIVE: every rank makes the same call with the same
 * kind. The verdict on a bad diagonal is agreed over the setup transport, so
 * every rank returns the same code and message, with the GLOBAL index; an
 * argument error or a failed allocation on one rank fails the call on all. */
enum { CGX_PRECOND_NONE = 0, CGX_PRECOND_JACOBI = 1, CGX_PRECOND_DIAGONAL = 2 };
/* d_out[i] = 1 / a_ii (entries with col == row summed). Blocking. CGX_EINVAL when a row has no
 * diagonal entry or a_ii is not positive and finite (the message gives the count and the first row).
 * Partitioned A: n_local values, 1 / a_ii of the rank's own rows; collective (above): the count
 * is the world's and the row the lowest global one, on every rank. */
int cgx_csr_diag_inv(cgx_csr *A, void *d_out);
/* kind NONE: d_minv ignored. JACOBI: the solver builds and owns 1/diag(A) (d_minv ignored).
 * DIAGONAL: d_minv = n (partitioned: n_local, the own rows') caller-owned device values,
 * positive and finite (checked, blocking; partitioned: collectively, the global entry reported),
 * 16-byte aligned (cgx_alloc's are), alive until replaced or the solver is destroyed.
 * Allowed between solves: it ends the current one (cgx_cg_run and cgx_cg_rxr need a new
 * cgx_cg_begin, where it takes effect) and drops the captured graphs. On an error the
 * solver keeps the preconditioner it had. */
int cgx_cg_set_precond(cgx_cg *cg, int kind, const void *d_minv);
int cgx_cg_get_precond(cgx_cg *cg, int *kind);
/* r.z after the last body (blocking); CGX_ESTATE without a preconditioner */
int cgx_cg_rz(cgx_cg *cg, double *rz);

/* ---- block-Jacobi preconditioning (replaces nothing in the reference;
 * DESIGN.md §5f) --------------------------------------------------------------
 * PCG with M^-1 = blockdiag(W_0, W_1, ...): block b covers rows [b bs,
 * min((b + 1) bs, n)) with one block size 1 <= bs <= 8 (the last block is
 * partial when n % bs != 0). W is an n x bs row-major device array, W[i bs + j]
 * = W_b[i - b bs, j]; the columns past a partial block's size hold +0.0 and
 * are never multiplied. z_i = sum_j W[i bs + j] r_{b bs + j}, from +0.0 in
 * ascending j over the block's real columns, each product rounded before its
 * add. The loop is the diagonal one's with z = M^-1 r in place of m o r; the
 * stop rule tests the true r.r, and cgx_cg_rxr, the body count and cgx_cg_rz
 * keep their meanings. update_r stores z over the Ap vector (no new vector);
 * the p update reads it there: per body (86 + 8 bs) N bytes of vector traffic
 * against the diagonal form's 94 N.
 * f64, one device, modes 1 and 3 (auto resolves to 3); modes 2, 4, 5, 6 and 7
 * return CGX_EUNSUPPORTED from whichever of cgx_cg_set_mode and
 * cgx_cg_set_block_precond comes second. CGX_EUNSUPPORTED too for an f32
 * solver (cgx_mixed's inner solver is one), a partitioned matrix and the fused
 * batch form (the sequential form runs it). The diagonal and the block
 * preconditioner exclude each other: setting one replaces the other, and
 * cgx_cg_get_precond reports CGX_PRECOND_NONE while a block one is set.
 * Out of scope: block sizes that vary, bs > 8, f32, partitioned matrices, the
 * fused batch form, modes 4, 6 and 7. (The many-systems solver has its own:
 * cgx_many_set_block_precond.) */
enum { CGX_BLOCK_NONE = 0, CGX_BLOCK_JACOBI = 1, CGX_BLOCK_GIVEN = 2 };
/* d_out (n * bs values) = W for W_b the inverse of A's diagonal block b.
 * Row i of a block takes the entries of CSR row i whose column lies in the
 * block and is <= i: the lower triangle decides, the upper is ignored;
 * duplicates are summed from 0 in entry order; rows may be unsorted. LDL^T
 * without pivoting, W = L^-T D^-1 L^-1 with the lower triangle computed and
 * mirrored (W is exactly symmetric; bs = 1 gives cgx_csr_diag_inv's values).
 * Blocking. CGX_EINVAL for bs outside 1..8 and when a block has a pivot that
 * is not positive and finite, a missing diagonal entry included (the message
 * gives the count of such blocks and the first one's index and first row);
 * CGX_EUNSUPPORTED for an f32 or a partitioned matrix.
 * Replaces nothing in the reference. */
int cgx_csr_block_inv(cgx_csr *A, int bs, void *d_out);
/* kind NONE: bs and d_w ignored. JACOBI: the solver builds and owns
 * cgx_csr_block_inv(A, bs) (d_w ignored). GIVEN: d_w = n * bs caller-owned
 * device values, 16-byte aligned; the solver makes and owns a copy. Checked on
 * the device (blocking): every entry of a real column finite, every W_b[i, i]
 * positive and finite (CGX_EINVAL names the first row). That each W_b is
 * SYMMETRIC and POSITIVE DEFINITE is the caller's duty: CG with another M is
 * not CG, and nothing here tests it. CGX_EINVAL before any device call for a
 * NULL handle, an unknown kind, bs outside 1..8, GIVEN with a NULL or
 * misaligned d_w. Allowed between solves as cgx_cg_set_precond is: it ends the
 * current solve, drops the captured graphs, and on any error the solver keeps
 * what it had. Replaces nothing in the reference. */
int cgx_cg_set_block_precond(cgx_cg *cg, int kind, int bs, const void *d_w);
/* the block preconditioner in effect (*bs = 0 with CGX_BLOCK_NONE); either
 * output may be NULL. Replaces nothing in the reference. */
int cgx_cg_get_block_precond(cgx_cg *cg, int *kind, int *bs);

/* ---- batched CG: several right-hand sides on one matrix (replaces nothing in
 * the reference, whose solve takes one b) ----------------------
 * A batch is nrhs (1..8) INDEPENDENT solves A x_c = b_c: column c has its own
 * scalar ring, stop rule (Q5), cap min(N + 1, max_bodies) and stop code, and
 * stops on its own; the batch ends when every column has. Column c's x, body
 * count, stop code and final r.r are, bit for bit, those of cgx_cg_solve in
 * mode 1 on the same matrix, b_c, initial x_c, tol and cap (the double-length
 * dots make the sums independent of how rows are dealt to threads). A NaN or
 * Inf in one column stops that column by the NaN rule and reaches no other.
 * d_B and d_X are column-major: column c starts at element c * ld, ld >= n;
 * elements [n, ld) of a column are neither read nor written. d_X holds the
 * initial guesses and receives the results.
 * Two forms (cgx_cg_set_batch_form):
 *   fused (1): one pass over the CSR arrays per body serves every column
 *     (three launches per body for the whole batch: the batched SpMV with each
 *     column's p.Ap, then the r and the x / p updates with each column's own
 *     alpha and beta). p, r and Ap are kept interleaved (a row's columns
 *     adjacent), so a gathered row is one 16 / 32-byte access per 2 / 4
 *     columns. Widths 2, 4 and 8 are built; another nrhs runs the next width
 *     with padding columns that never become active. Any single-device f64
 *     matrix (it walks the CSR arrays, whatever the matrix's SpMV format);
 *     CGX_EUNSUPPORTED with a preconditioner set, on an f32 solver and on a
 *     partitioned matrix (the message names the reason).
 *   sequential (2): cgx_cg_solve's steps once per column, in whatever mode
 *     the solver has, a preconditioner and f32 included (a column that is not
 *     16-byte aligned, i.e. an odd ld, is solved through an aligned copy).
 *   auto (0, the default): fused for nrhs >= 2 where the matrix's production
 *     SpMV variant is a CSR-stream form and the fused form supports the
 *     solver, else sequential. Measured with tools/batch_bench.py on an
 *     MI355X (400 bodies, graph replay, three interleaved rounds, medians;
 *     profiles/batch_bench.log), µs per body per column, fused against the
 *     auto-mode single solve: G3 stand-in (4.8 entries per row) 38.4 / 35.9 /
 *     38.3 against 40.8 at 2 / 4 / 8 columns, every fused round below every
 *     single round; irregular_spd(400,000, mean_deg 26) 29.9 / 24.4 / 23.4
 *     against 33.5 in mode 1 (its auto mode, 5, ran 277). One column alone
 *     runs width 2 with a padding column and loses, 72.2 against 40.8 and
 *     56.3 against 33.5, so auto keeps nrhs = 1 sequential.
 * Partitioned matrices return CGX_EUNSUPPORTED in both forms.
 * A batch call ends a single solve in progress (cgx_cg_run then needs a new
 * cgx_cg_begin) and cgx_cg_begin ends a batch in progress. The batch's
 * buffers are allocated on first use and freed by cgx_cg_destroy.
 * cgx_cg_solve_batch: blocking. bodies_out[nrhs], rxr_out[nrhs] (the r.r
 * after each column's last body), stopped_out[nrhs] (may be NULL; 1 stop rule
 * or NaN, 2 cap reached). CGX_EINVAL for nrhs outside 1..8, ld < n or a NULL
 * pointer. */
int cgx_cg_solve_batch(cgx_cg *cg, int nrhs, const void *d_B, int64_t ldb, void *d_X, int64_t ldx,
                       double tol, int64_t max_bodies, int64_t *bodies_out, double *rxr_out,
                       int *stopped_out);
/* The split form of the FUSED batch (CGX_EUNSUPPORTED while the sequential
 * form is in effect), as cgx_cg_begin / cgx_cg_run: init of every column,
 * then up to `bodies` more bodies, captured as hipGraphs in chunks of the
 * poll interval (cgx_cg_config); the host's poll copies the nrhs scalar
 * rings. bodies_total[nrhs]: each column's bodies so far; *all_stopped: 1
 * when no column is active any more. A stopped column's x, r and p are not
 * touched by later bodies. */
int cgx_cg_begin_batch(cgx_cg *cg, int nrhs, const void *d_B, int64_t ldb, void *d_X, int64_t ldx,
                       double tol, int64_t max_bodies);
int cgx_cg_run_batch(cgx_cg *cg, int64_t bodies, int64_t *bodies_total, int *all_stopped);
/* form: 0 auto, 1 fused, 2 sequential (above); takes effect at the next batch call. */
int cgx_cg_set_batch_form(cgx_cg *cg, int form);
/* *form_in_effect: 1 or 2: the form the last batch call took or, before any
 * since the form was set, auto resolved for nrhs >= 2 against the matrix and
 * the solver as they are now; *width: the instantiated width of the fused
 * form's buffers (2, 4 or 8; 0 before its first batch and while sequential is
 * in effect). */
int cgx_cg_batch_info(cgx_cg *cg, int *form_in_effect, int *width);

/* ---- multi-shift CG: one matrix under several diagonal shifts (replaces
 * nothing in the reference, whose solve takes one matrix) -------
 * cgx_cg_solve_shifted solves (A + sigma_s I) x_s = b for nshift (1..8) shifts
 * sigma_s >= 0 from x_s = 0 in one Krylov space: the shifted residuals stay
 * collinear with the base residual of A, r_s = zeta_s r, so one SpMV and one
 * pair of dots per body serve every shift and a shift costs its own x_s and
 * p_s update (32 N bytes per body). The body is three launches (the mode-1
 * shape, whatever the solver's mode; graph-replayed in chunks of the poll
 * interval, cgx_cg_config): the SpMV with p.Ap and the r update of the single
 * solver, unchanged, in every SpMV format, then one launch with the base p
 * update and every active shift's updates. Scalars stay on the device.
 * The base recurrence is the mode-1 loop on A from x = 0 (it keeps no x): in
 * body n, a = alpha_n = rxr / pAp and bt = beta_n = rr / rxr as cgx_cg_solve
 * forms them; ap = alpha_{n-1}, bp = beta_{n-1} (1 and 0 in body 0). A shift
 * keeps zc = zeta_n and zp = zeta_{n-1} (1 and 1 in body 0), p_s = b, x_s = 0.
 * After r is updated an active shift runs, in f64, every operation rounded
 * and none contracted, the parentheses being the order:
 *   t1 = (a * bp) * (zp - zc)
 *   t2 = (zp * ap) * (1 + sigma * a)
 *   zn = ((zc * zp) * ap) / (t1 + t2)
 *   q  = zn / zc ;  as = a * q ;  bs = (bt * q) * q
 *   x_s[i] = x_s[i] + as * p_s[i]
 *   p_s[i] = zn * r[i] + bs * p_s[i]              (r is r_{n+1})
 *   zp = zc ; zc = zn
 * and the base does p = r + bt * p. With sigma = 0 and finite scalars zn = 1,
 * as = a and bs = bt exactly: that column is cgx_cg_solve in mode 1 from
 * x0 = 0, bit for bit (x, bodies, stop code).
 * Freeze rule (Q5 on the shift's own residual norm |zeta_s| ||r|| at the start
 * of the body): in body n, with m = bodies + 1, an active shift has
 *   stop = isnan(rxr_n) || fabs(zc) * sqrt(rxr_n) <= tol || !(fabs(zn) >= DBL_MIN)
 * bodies_s = m; stop -> code 1 and the shift is frozen from the next body on;
 * else m >= cap -> code 2. (The third term freezes a shift whose zeta left the
 * normal range: its residual is below DBL_MIN ||r||.) Later bodies neither
 * read nor write a frozen shift's x_s and p_s. The solve goes on while any
 * shift is active and m < cap = min(N + 1, max_bodies) (N + 1 when
 * max_bodies < 0). With a base scalar that is not finite the body counts and
 * codes are the single solve's (the NaN rule ends every shift) and the values
 * of x_s are unspecified.
 * Blocking. d_X (output only, column-major, ldx >= n; elements [n, ldx) of a
 * column are not touched; a column that is not 16-byte aligned, from an odd
 * ldx, takes 8-byte accesses). bodies_out[nshift]; res_out[nshift] =
 * fabs(zeta_s) * sqrt(r.r) after the shift's last body; stopped_out[nshift]
 * (may be NULL; 1 frozen by the rule, 2 cap reached). Duplicate shifts are
 * allowed. CGX_EINVAL for nshift outside 1..8, a NULL pointer, ldx < n, and a
 * shift that is negative or not finite (A + sigma I must stay SPD, and for
 * sigma >= 0 every shift's residual is bounded by the base's).
 * CGX_EUNSUPPORTED, the reason named, on an f32 solver, on a partitioned
 * matrix and with a diagonal or block preconditioner set (M (A + sigma I) is
 * not a shift of M A). The call ends a single solve or a batch in progress;
 * cgx_cg_begin and the batch calls end it. The auto choices never pick it.
 * The shifts' buffers (one p_s of n + 2 doubles per shift, the state) are
 * allocated on first use and freed by cgx_cg_destroy.
 * One shift alone carries a second direction vector on top of the single
 * solve's body and loses to cgx_cg_solve on the shifted matrix: 1.08 to 1.17
 * of a mode-1 body on an MI355X; from two shifts on it wins, 0.57 to 0.73 at
 * two and 0.20 to 0.44 at eight of as many mode-1 bodies
 * (tools/shift_bench.py, profiles/shift_bench.log).
 * cgx_cg_shifted_zeta: zeta_s after each shift's last body of the last
 * shifted solve (CGX_ESTATE before any). */
enum { CGX_SHIFT_MAX = 8 };
int cgx_cg_solve_shifted(cgx_cg *cg, int nshift, const double *h_sigma, const void *d_b,
                         void *d_X, int64_t ldx, double tol, int64_t max_bodies,
                         int64_t *bodies_out, double *res_out, int *stopped_out);
int cgx_cg_shifted_zeta(cgx_cg *cg, double *zeta_out /* [nshift] */);

/* ---- cgx_mixed: an f64 system solved with f32 bodies (replaces nothing in
 * the reference, whose solve runs in one precision) -----------
 * Iterative refinement: A x = b in f64 is solved to `tol` on the TRUE f64
 * residual, the loop bodies run by the f32 solver (cgx_cg, any mode, format,
 * graph replay, preconditioner) on A32, A's values cast once to f32. Per outer
 * step the f64 work is one SpMV (cgx_spmv's launch on A) and three streaming
 * kernels. The loop, with tot = 0 and prev = +inf:
 *   r = b - A x; rr = r.r (double-length sum, rounded once); nr = sqrt(rr)
 *   record (rr, bodies and final f32 r.r of the previous inner solve; 0, 0 first)
 *   rr NaN or Inf -> status 4; nr <= tol -> 1; nr > 0.5 prev -> 3 (stagnated:
 *   less than one bit gained); o == max_outer or tot >= cap -> 2
 *   prev = nr; nr = f 2^e, f in [0.5, 1); s = 2^-e
 *   r32 = (float)(r s) (one rounding to nearest even, subnormals kept), d32 = 0
 *   f32 CG on A32 d = r32, absolute tolerance max(inner_reduction, 0.5 tol s),
 *   at most min(n + 1, inner_cap, cap - tot) bodies
 *   its final r.r NaN -> status 4, the correction NOT applied (this includes an
 *   inner system solved exactly, n = 1 or a diagonal A: stop rule Q5 runs one
 *   more body on r.r = 0), its bodies not counted
 *   x += (double)d32 2^e (product exact, one add); tot += its bodies
 * tol is absolute on sqrt(r.r) and cap is max_bodies, both as cgx_cg_solve's
 * (max_bodies < 0: n + 1); cap counts inner bodies over the whole call. */
typedef struct cgx_mixed cgx_mixed;
/* A: f64, single device (an f32 matrix: CGX_EINVAL, a partitioned one:
 * CGX_EUNSUPPORTED), values 16-byte aligned, alive (with its arrays) until
 * cgx_mixed_destroy. Builds the f32 values (A's rowptr and col are shared, not
 * rewritten), an f32 cgx_csr through cgx_csr_create (autotune included), an
 * f32 cgx_cg and the vectors r, Ax, r32, d32. CGX_EINVAL when a value of A
 * casts to +-inf or a non-zero value casts to 0 (the message gives the count
 * and the first entry). Blocking. Replaces nothing in the reference. */
int cgx_mixed_create(cgx_ctx *ctx, cgx_csr *A, cgx_mixed **out);
/* Replaces nothing in the reference. */
int cgx_mixed_destroy(cgx_mixed *m);
/* inner_reduction (default 1e-5: about what f32 CG delivers before its
 * recursive residual leaves the true one), max_outer (8), inner_cap (n + 1);
 * 0 keeps a default, CGX_EINVAL for a negative or non-finite value.
 * Replaces nothing in the reference. */
int cgx_mixed_config(cgx_mixed *m, double inner_reduction, int max_outer, int64_t inner_cap);
/* cgx_cg_set_mode on the inner solver. Replaces nothing in the reference. */
int cgx_mixed_set_mode(cgx_mixed *m, int mode);
/* cgx_cg_set_precond on the inner solver. JACOBI: 1 / a_ii formed in f32 from
 * A32. DIAGONAL: d_minv = n f64 device values (16-byte aligned), of which an
 * f32 copy is made and owned here (the caller's need not outlive the call);
 * CGX_EINVAL when a value is not positive and finite after the cast (the
 * message names the first entry). A mode that refuses a preconditioner fails
 * as cgx_cg_set_precond does. Blocking. Replaces nothing in the reference. */
int cgx_mixed_set_precond(cgx_mixed *m, int kind, const void *d_minv);
/* Blocking. d_b, d_x: n f64 device values, 16-byte aligned; d_x holds the
 * initial guess and receives the result. Outputs (each may be NULL): *outer
 * corrections applied, *inner_bodies f32 bodies counted against the cap, *rxr
 * the last f64 true r.r (the one that decided the status), *status 1 tol
 * reached, 2 max_outer or the body cap, 3 stagnated, 4 NaN (x is the last
 * finite iterate). The outer steps launch eagerly; the inner solves replay
 * their graphs. Replaces nothing in the reference. */
int cgx_mixed_solve(cgx_mixed *m, const void *d_b, void *d_x, double tol, int64_t max_bodies,
                    int *outer, int64_t *inner_bodies, double *rxr, int *status);
/* One record per residual evaluation of the last solve: rr[i] the f64 r.r,
 * inner_bodies[i] / inner_rxr[i] the bodies and final f32 r.r (of the scaled
 * system) of the inner solve before it (0 / 0 for the first). *count = the
 * records; up to `cap` are written. Replaces nothing in the reference. */
int cgx_mixed_history(cgx_mixed *m, double *rr, int64_t *inner_bodies, double *inner_rxr, int cap,
                      int *count);
/* Borrowed handles of the f32 matrix and the inner solver: the info, timing
 * and configuration calls work on them; do not destroy them.
 * Replaces nothing in the reference. */
int cgx_mixed_inner(cgx_mixed *m, cgx_csr **A32, cgx_cg **cg32);
/* Device bytes the object holds on top of A: the f32 values, its vectors, the
 * f32 matrix's schedule and formats and the inner solver's buffers, each at
 * its allocated size, as of the call. Replaces nothing in the reference. */
int cgx_mixed_bytes(cgx_mixed *m, int64_t *bytes);

/* ---- cgx_many: many small systems, one workgroup (or, up to 256 rows, one
 * wave: cgx_many_set_form) per system (replaces nothing in the reference,
 * which solves one system) ----------
 * nsys SPD systems of n <= 4,096 rows share one sparsity pattern (d_rowptr:
 * n + 1 entries, d_col: nnz entries, entries in CSR order as given); system s
 * has its own values at d_val + s * ldv, its right-hand side at d_B + s * ldb
 * and its initial guess / result at d_X + s * ldx. One workgroup of 256
 * threads runs a whole solve (init and every body; p in LDS, the own rows' x
 * and r in registers, a dot a workgroup reduction), then takes the next
 * system: no kernel boundary, no graph replay, no exchange between workgroups.
 * Arithmetic (normative): system s's x, body count, stop code and final r.r
 * equal, bit for bit, those of cgx_cg_solve in mode 1 on a cgx_csr made from
 * (rowptr, col, val_s) with the same b_s, x0_s, tol and cap, wherever both
 * dots of that run are clear of a rounding boundary (cgx_dd.h): the single
 * kernels' per-element expressions, products rounded before adds, a row summed
 * by one thread from 0 in ascending entry order whatever its length (the
 * single solve tree-sums a row longer than a tile), double-length dots rounded
 * once, alpha = rr / pAp, beta = rr' / rr, stop rule Q5 (the r.r a body began
 * with, tested after that body's x update; NaN stops). A NaN or Inf in one
 * system's values, b or x0 stops that system and reaches no other.
 * Measured with tools/many_bench.py on an MI355X (4,096 systems to 1e-8 ||b||,
 * three interleaved rounds, medians; profiles/many_bench.log), µs per system:
 * scaled 32 x 32 Poisson 3.85 against 1,998 for a cgx_cg_solve per system
 * (auto mode 5, create not counted) and 19.2 for one solve on the block-diagonal
 * assembly; irregular_spd(1000) 6.36 against 2,974 and 37.9.
 * Diagonal preconditioning (cgx_many_set_precond) and block-Jacobi
 * preconditioning (cgx_many_set_block_precond) run in the same kernels: see
 * there.
 * Out of scope: f32 systems, a preconditioner other than a diagonal or dense
 * diagonal blocks of one size up to 8, systems with differing patterns,
 * partitioned or multi-GPU use, and any auto route from cgx_cg_solve into
 * this path; in the wave form (cgx_many_set_form) also
 * several systems per wave for n <= 32 and values cached in registers. */
typedef struct cgx_many cgx_many;
/* dtype: CGX_F64 (CGX_F32: CGX_EUNSUPPORTED). 1 <= n <= 4,096 (above:
 * CGX_EUNSUPPORTED; use cgx_cg_solve), nsys >= 1, ldv >= nnz, rows of any
 * length, an empty row included. The arrays are the caller's and stay alive
 * until cgx_many_destroy. The VALUES are read at every solve: a caller may
 * overwrite them in place between solves, which is how a time-stepping caller
 * refreshes its matrices without a new create; values in [nnz, ldv) are never
 * read. The pattern is checked once, here, on the device: CGX_EINVAL for
 * rowptr[0] != 0, rowptr[n] != nnz, a descending rowptr or a column outside
 * [0, n); also for nsys < 1, ldv < nnz, a NULL pointer, values that are not
 * 8-byte aligned. Blocking. Replaces nothing in the reference. */
int cgx_many_create(cgx_ctx *ctx, int dtype, int64_t nsys, int64_t n, int64_t nnz,
                    const int32_t *d_rowptr, const int32_t *d_col, const void *d_val,
                    int64_t ldv, cgx_many **out);
/* Replaces nothing in the reference. */
int cgx_many_destroy(cgx_many *m);
/* max_workgroups caps the grid, min(nsys, resident workgroups,
 * max_workgroups) (in the wave form ceil(nsys / 4) takes the place of nsys:
 * cgx_many_set_form); 0: no cap (the default), negative: CGX_EINVAL. A tuning
 * knob, as cgx_cg_config: a workgroup takes systems blockIdx, blockIdx + grid,
 * ... and the results do not depend on it. Replaces nothing in the reference. */
int cgx_many_config(cgx_many *m, int max_workgroups);
/* Blocking. d_B, d_X: system-major f64 device arrays, 8-byte aligned, ldb and
 * ldx >= n (CGX_EINVAL otherwise); elements in [n, ld) are neither read nor
 * written. tol is absolute on sqrt(r.r); the cap is min(n + 1, max_bodies), or
 * n + 1 when max_bodies < 0: both as cgx_cg_solve's. Host outputs of nsys
 * entries: bodies_out, rxr_out (the r.r after each system's last body),
 * stopped_out (may be NULL; cgx_cg_solve_batch's codes: 1 stop rule or NaN,
 * 2 cap reached). Replaces nothing in the reference. */
int cgx_many_solve(cgx_many *m, const void *d_B, int64_t ldb, void *d_X, int64_t ldx, double tol,
                   int64_t max_bodies, int64_t *bodies_out, double *rxr_out, int *stopped_out);
/* *workgroups: the grid the next solve launches; *rows_per_thread: the
 * instantiation (1, 2, 4, 8 or 16: the least with n <= 256 rows_per_thread;
 * in the wave form 1, 2 or 4 rows per lane: the least with n <= 64
 * rows_per_thread); *lds_bytes: its LDS per workgroup (wave form: four waves'
 * p, 4 * 64 rows_per_thread doubles, twice that under a preconditioner). Each
 * may be NULL. Replaces nothing in the reference. */
int cgx_many_info(cgx_many *m, int *workgroups, int *rows_per_thread, int64_t *lds_bytes);
/* Diagonal preconditioning inside the many-systems kernel. kind: CGX_PRECOND_NONE
 * (the default), CGX_PRECOND_JACOBI or CGX_PRECOND_DIAGONAL; it may be set
 * between solves and takes effect at the next one (cgx_many_info then reports
 * the preconditioned instantiation's grid and LDS). NONE and JACOBI ignore d_M
 * and ldm. JACOBI: m_i = 1 / a_ii, a_ii the row's entries with col == row
 * summed from 0 in entry order, formed in the kernel at EVERY solve from the
 * values that solve reads, so values overwritten in place never meet a stale
 * diagonal. DIAGONAL: system s's m is the n f64 values at d_M + s * ldm,
 * ldm >= n; the array is the caller's, 8-byte aligned, alive until replaced or
 * cgx_many_destroy, read at every solve; [n, ldm) is never read.
 * Arithmetic (normative): system s's x, body count, stop code, final r.r and
 * final r.z equal, bit for bit, those of cgx_cg_solve in mode 1 with
 * cgx_cg_set_precond(kind) on that system alone, wherever the run's dots are
 * clear of a rounding boundary: z = m o r rounded and never stored,
 * alpha = rz / p.Ap, r.r and r.z in one sweep, beta = rz' / rz,
 * p = m o r + beta p, stop rule Q5 on the true r.r. With m == 1 every value
 * is the plain kernel's.
 * A bad diagonal stops its own system and no other: where a row has no
 * diagonal entry or a_ii is not positive and finite (JACOBI), or an m_i is
 * not positive and finite (DIAGONAL), that system's X is left exactly as
 * given and it reports 0 bodies, NaN r.r, NaN r.z and stop code 3; the call
 * still returns CGX_OK. Code 3 does not occur without a preconditioner.
 * Measured with tools/many_pcg_bench.py on an MI355X (many_bench's systems,
 * medians; profiles/many_pcg_bench.log), µs per system plain -> JACOBI: scaled
 * 32 x 32 Poisson 3.89 -> 0.98 (418 -> 104 bodies), irregular_spd(1000) 6.44 ->
 * 1.31 (381 -> 73); a preconditioned body costs 1.5 to 6.5 % more.
 * CGX_EINVAL, before any device call, for a NULL handle, an unknown kind,
 * DIAGONAL with a NULL or misaligned d_M or ldm < n; on an error the object
 * keeps the preconditioner it had. Replaces nothing in the reference. */
int cgx_many_set_precond(cgx_many *m, int kind, const void *d_M, int64_t ldm);
/* Replaces nothing in the reference. */
int cgx_many_get_precond(cgx_many *m, int *kind);
/* nsys host values: r.z after each system's last body in the last solve.
 * CGX_ESTATE without a preconditioner, or before a solve under the one that
 * is set. Replaces nothing in the reference. */
int cgx_many_rz(cgx_many *m, double *rz_out);

/* The form of the many-systems kernel. WORKGROUP: one workgroup of 256 threads
 * per system, any n <= 4,096 (above). WAVE: one wave per system for n <= 256:
 * wave w of workgroup g runs systems 4 g + w, 4 g + w + 4 grid, ...; lane l
 * owns rows l, l + 64, ... (1, 2 or 4 rows per lane), their x and r in
 * registers, p (and m under a preconditioner) in LDS of the wave's own; a dot
 * is a wave reduction broadcast from lane 0, a bad diagonal's verdict a wave
 * vote. The four waves of a workgroup run four independent solves and never
 * wait for each other: the kernel has no workgroup barrier. The grid is
 * min(ceil(nsys / 4), resident workgroups, max_workgroups); results do not
 * depend on it. AUTO (the default) takes the wave form for n <= 64 and the
 * workgroup form above; for 65 <= n <= 256 the wave form is by request only.
 * Arithmetic (normative): the workgroup form's, statement for statement, with
 * the same pin to cgx_cg_solve in mode 1 (with cgx_cg_set_precond under a
 * preconditioner) wherever the dots are clear, and the same outputs for a bad
 * diagonal (X untouched, 0 bodies, NaN r.r and r.z, stop code 3). For n <= 64
 * the two forms give the same bits, clear or not, NaN and Inf included: the
 * workgroup form's other three waves add (0, 0) to the double-length sum.
 * Measured with tools/many_wave_bench.py on an MI355X (65,536 systems to 1e-8
 * ||b||, medians; profiles/many_wave_bench.log), µs per system workgroup ->
 * wave: scaled 8 x 8 Poisson 0.105 -> 0.026 (JACOBI 0.119 -> 0.027),
 * irregular_spd(60) 0.212 -> 0.080 (0.168 -> 0.047); by request at n = 121
 * 0.145 -> 0.049 and at n = 256 0.225 -> 0.156. Every wave round lay below
 * every workgroup round, which is why AUTO takes the wave form up to 64 rows.
 * cgx_many_set_form: CGX_EINVAL, before any device call, for an unknown form
 * or a NULL handle; CGX_EUNSUPPORTED for WAVE on an object with n > 256 (use
 * the workgroup form). It may be called between solves and takes effect at
 * the next one (cgx_many_info then reports that form's instantiation); on an
 * error the object keeps the form it had.
 * cgx_many_get_form: *requested as set, *in_effect CGX_MANY_FORM_WORKGROUP or
 * CGX_MANY_FORM_WAVE: what the next solve launches. Each may be NULL.
 * Replace nothing in the reference. */
enum { CGX_MANY_FORM_AUTO = 0, CGX_MANY_FORM_WORKGROUP = 1, CGX_MANY_FORM_WAVE = 2 };
int cgx_many_set_form(cgx_many *m, int form);
int cgx_many_get_form(cgx_many *m, int *requested, int *in_effect);

/* Block-Jacobi preconditioning inside the many-systems kernels, both forms:
 * M^-1 = blockdiag(W_0, W_1, ...) per system, block b over rows [b bs,
 * min((b + 1) bs, n)) with one bs in 1..8, as cgx_cg_set_block_precond's.
 * System s's W is n x bs row-major at d_W + s * ldw, ldw >= n * bs, 8-byte
 * aligned: W[i bs + j] = W_b[i - b bs, j]; the columns past a partial last
 * block hold +0.0 and are never multiplied; [n bs, ldw) is never read, and
 * cgx_many_block_inv never writes it. kind is CGX_BLOCK_NONE, CGX_BLOCK_JACOBI
 * or CGX_BLOCK_GIVEN; it may be set between solves and takes effect at the
 * next one (cgx_many_info then reports the block instantiation's grid, rows
 * per thread and LDS: p, the staged r and the reduction words, the diagonal
 * form's footprint). NONE ignores bs, d_W and ldw.
 * JACOBI: d_W and ldw are ignored; the object owns an nsys x n bs workspace,
 * allocated by this call (CGX_ENOMEM keeps what was set), and EVERY
 * cgx_many_solve refills it from the values that solve reads, in a launch of
 * its own before the CG kernel on the same stream: one thread per (system,
 * block), cgx_csr_block_inv's statements (the lower triangle decides,
 * duplicates summed from 0 in entry order, rows may be unsorted, LDL^T without
 * pivoting, W mirrored). Values overwritten in place never meet a stale W.
 * GIVEN: the caller's array, alive until replaced or cgx_many_destroy and read
 * at every solve, as DIAGONAL's d_M; no copy is made. That each W_b is
 * SYMMETRIC and POSITIVE DEFINITE is the caller's duty: CG with another M is
 * not CG, and nothing here tests it.
 * Arithmetic (normative): system s's x, body count, stop code, final r.r and
 * final r.z equal, bit for bit, those of cgx_cg_solve in mode 1 with
 * cgx_cg_set_block_precond(JACOBI, bs) (under GIVEN: (GIVEN, bs, W_s)) on that
 * system alone, wherever the run's dots are clear of a rounding boundary:
 * z_i = sum_j W[i bs + j] r_{b bs + j} from +0.0 in ascending j over the
 * block's real columns, each product rounded before its add; p = z and
 * rz = r.z at the start; per body alpha = rz / p.Ap, r -= alpha Ap, r.r and r.z
 * double-length sums rounded once, beta = rz' / rz, x += alpha p,
 * p = z + beta p; stop rule Q5 on the true r.r. With bs = 1 and JACOBI every
 * value is the in-kernel Jacobi's on finite systems; with W the identity every
 * value is the plain kernel's. A body has four barriers in the workgroup form
 * (the staged r is published by the r.r sum's, r.z is a third sum) and none in
 * the wave form; for n <= 64 the two forms give the same bits.
 * A bad system stops alone: under JACOBI one with a pivot that is not positive
 * and finite, a missing diagonal entry included; under GIVEN one with an entry
 * of a real column that is not finite or a W_b[i, i] that is not positive and
 * finite (checked at every solve in a launch before the CG kernel). Its X is
 * left exactly as given and it reports 0 bodies, NaN r.r, NaN r.z and stop
 * code 3; the call returns CGX_OK and no other system is touched.
 * The diagonal and the block preconditioner exclude each other on a cgx_many:
 * setting either replaces the other, NONE included; cgx_many_get_precond
 * reports CGX_PRECOND_NONE while a block one is set; cgx_many_rz works under
 * either. AUTO never chooses a block preconditioner.
 * Measured with tools/many_block_pcg_bench.py on an MI355X (node_mixed
 * principal systems scaled per system, to 1e-8 ||b||, three interleaved rounds
 * after an untimed pass, medians; profiles/many_block_pcg_bench.log), µs per
 * system in-kernel Jacobi -> block-Jacobi with the fill launch inside: 65,536
 * systems of 60 rows, bs = 3 (wave form) 0.159 -> 0.058 (61 bodies, Jacobi's
 * cap, -> 17); 4,096 of 396 rows, bs = 3, 9.04 -> 1.34 (313 -> 48); 4,096 of
 * 392 rows, bs = 8, 40.5 -> 2.82 (375 -> 25); 4,096 of 3,000 rows, bs = 3,
 * 186.4 -> 30.5 (814 -> 124). Every block round lay below every Jacobi and
 * every plain round at each size. A block body costs 0.96 to 1.31 of a Jacobi
 * body (1.31 in the wave form at 60 rows); the fill alone, timed as a
 * blocking cgx_many_block_inv, is 1.5 to 10 % of the block solve.
 * CGX_EINVAL, before any device call, for a NULL handle, an unknown kind, bs
 * outside 1..8 (kind != NONE), GIVEN with a NULL or misaligned d_W or
 * ldw < n * bs; on any error the object keeps what it had.
 * cgx_many_get_block_precond: the block preconditioner in effect (*bs = 0
 * with CGX_BLOCK_NONE); either output may be NULL.
 * cgx_many_block_inv: the same fill into a caller's array (how a caller makes
 * a GIVEN array); blocking. CGX_OK whether or not blocks are bad: *n_bad is
 * the number of systems with a bad block, *first_bad the lowest such system
 * or -1 (either may be NULL); a bad block's W holds whatever the statements
 * give. CGX_EINVAL for a NULL handle, bs outside 1..8, a NULL or misaligned
 * d_W, ldw < n * bs.
 * cgx_many_block_bad: nsys host ints, 1 for each system the last
 * cgx_many_block_inv found a bad block in (*n_bad of them, *first_bad the
 * first); CGX_ESTATE before one has run, and after a solve since.
 * Out of scope: block sizes that vary, bs > 8, f32, an auto route into block
 * preconditioning, several systems per wave.
 * Each of the four: Replaces nothing in the reference. */
int cgx_many_set_block_precond(cgx_many *m, int kind, int bs, const void *d_W, int64_t ldw);
/* Replaces nothing in the reference. */
int cgx_many_get_block_precond(cgx_many *m, int *kind, int *bs);
/* Replaces nothing in the reference. */
int cgx_many_block_inv(cgx_many *m, int bs, void *d_W, int64_t ldw, int64_t *n_bad,
                       int64_t *first_bad);
/* Replaces nothing in the reference. */
int cgx_many_block_bad(cgx_many *m, int *bad_out);

/* CG::accuracy (CG.hpp:463-515): blocking; |sum (b-Ax)^2 / sum x^2|. */
int cgx_accuracy(cgx_ctx *ctx, cgx_csr *A, const void *d_b, const void *d_x,
                 double *out);

/* ---- synthetic inputs ---------------------------------------
 * Dirichlet Poisson CSR generated on the device (dim 2: 5-point, dim 3:
 * 7-point; lexicographic, x fastest; columns ascending; diag 2*dim, off -1).
 * Rows [row_begin, row_end) of the global matrix; column indices global. */
int64_t cgx_poisson_nnz(int dim, int nx, int ny, int nz, int64_t row_begin,
                        int64_t row_end);
int cgx_poisson_fill(cgx_ctx *ctx, int dtype, int dim, int nx, int ny, int nz,
                     int64_t row_begin, int64_t row_end, int *d_rowptr,
                     int *d_col, void *d_val);
/* b_i = i + 1 + offset (Tester.cpp:29-30) */
int cgx_iota(cgx_ctx *ctx, int dtype, void *d_b, int64_t n, double offset);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI --------
 * Rows are partitioned in contiguous blocks; p's ghost entries are exchanged
 * each iteration with ncclSend/ncclRecv and the two dots are all-reduced. */
int cgx_nccl_unique_id(char *id_out, size_t len);            /* len >= 128 */
int cgx_dist_init(cgx_ctx *ctx, int rank, int world, const char *id, size_t len);
int cgx_dist_rank(cgx_ctx *ctx, int *rank, int *world);
/* Host-staged transport: the same partitioned solver with every collective
 * done by caller callbacks on HOST buffers (return 0 on success). Used to run
 * several ranks on one GPU (RCCL refuses that) in tests; slow by design.
 *   allgather: recv[world * bytes] <- every rank's `bytes` from send
 *   allreduce: vals[count] <- element-wise sum over ranks (in place)
 *   exchange : for i < n, send[i] (send_bytes[i]) to peers[i] and receive
 *              recv_bytes[i] from peers[i] into recv[i] */
typedef int (*cgx_allgather_fn)(void *user, const void *send, size_t bytes, void *recv);
typedef int (*cgx_allreduce_fn)(void *user, double *vals, int count);
typedef int (*cgx_exchange_fn)(void *user, int n, const int *peers, const void *const *send,
                               const size_t *send_bytes, void *const *recv,
                               const size_t *recv_bytes);
int cgx_dist_init_host(cgx_ctx *ctx, int rank, int world, cgx_allgather_fn allgather,
                       cgx_allreduce_fn allreduce, cgx_exchange_fn exchange, void *user);
/* Host transport, asynchronous halo: the per-iteration exchange runs on the
 * context's comm stream (D2H, `exchange` as a host function, H2D, an event the
 * solver stream waits on), so a split SpMV's interior slices overlap it — the
 * stream/event ordering of the RCCL exchange. The callback then runs on the
 * HIP runtime's callback thread. Call before cgx_csr_create_dist. */
int cgx_dist_host_async(cgx_ctx *ctx, int on);
/* exchanges a partitioned matrix has posted on the comm stream (host transport) */
int cgx_csr_halo_async_calls(cgx_csr *A, int64_t *calls);
/* Local block of a globally row-partitioned matrix: rows
 * [row_begin, row_begin + n_local) with GLOBAL column indices (device arrays,
 * caller-owned, d_col is rewritten in place to local/ghost numbering).
 * n_global is the global dimension. Collective over the communicator. */
int cgx_csr_create_dist(cgx_ctx *ctx, int64_t n_global, int64_t row_begin,
                        int64_t n_local, int64_t nnz_local, const int *d_rowptr,
                        int *d_col, const void *d_val, int dtype, cgx_csr **out);
/* ghost entries this rank receives per iteration */
int cgx_csr_halo_info(cgx_csr *csr, int64_t *ghosts, int *neighbours);
/* Reduce a host double over ranks (sum); utility for tests. */
/* Slices of a partitioned SELL matrix without / with ghost columns: the
 * SpMV runs the interior ones while the halo exchange is in flight. Both 0
 * when the matrix is not split (no SELL copy, or no ghosts). */
int cgx_csr_split_info(cgx_csr *csr, int *interior_slices, int *boundary_slices);
int cgx_dist_allreduce_sum(cgx_ctx *ctx, double *value);
/* Device peer transport over xGMI for a partitioned matrix (collective):
 * every rank maps the other ranks' mailboxes and its neighbours' halo
 * landing buffers (hipIpc, uncached device memory), and the solver's halo
 * exchange and dot all-reduces then run as kernels that store straight into
 * peer memory — no host-enqueued collective per iteration, so the
 * partitioned iteration is graph-captured like the single-GPU one. The
 * transport is checked against the setup transport (RCCL or host) before it
 * is used: *enabled = 1 when every rank passed, 0 when the solver keeps the
 * setup transport (not an error; cgx_last_error() says why). Call before
 * cgx_cg_create. $CGX_PEER=0 declines; $CGX_PEER_TIMEOUT_S bounds every
 * device-side wait (default 10 s; a timeout stops the solve with an error). */
int cgx_dist_peer_enable(cgx_csr *csr, int *enabled);
int cgx_dist_peer_info(cgx_csr *csr, int *enabled);
/* The peer transport's iteration form: *colocated = ranks whose device is
 * this rank's (0 when the transport is off), *one_waiter = 1 when at most one
 * workgroup per rank waits on another rank at any time (a one-workgroup wait
 * launch before the boundary rows, one-workgroup all-reduces before the
 * kernels that consume the dots). Taken on every rank when any two ranks
 * share a GPU, where whole waiting grids could hold the CUs a peer needs;
 * otherwise the fused form (the waits inside the consuming kernels, fewer
 * launches). Same values either way. $CGX_PEER_ONE_WAITER=0/1 forces it. */
int cgx_dist_peer_form(cgx_csr *csr, int *colocated, int *one_waiter);

/* ---- host-only helpers (no device needed; the CPU test-suite drives them) --
 * Halo plan of rows [row_begin, row_begin + n_local) whose global column
 * indices are `col`: sorted distinct off-block columns (*ghosts, malloc'ed,
 * release with cgx_free_host) and per-rank receive counts (recv_cnt[world]);
 * begins/counts give every rank's row range (contiguous, ordered by rank). */
int cgx_plan_ghosts(int64_t n_local, int64_t row_begin, int64_t nnz, const int *col,
                    int world, const int64_t *begins, const int64_t *counts,
                    int64_t *n_ghost, int64_t **ghosts, int64_t *recv_cnt);
/* Global -> local column numbering (own rows, then ghosts in list order). */
int cgx_plan_remap(int64_t n_local, int64_t row_begin, int64_t nnz, int *col,
                   int64_t n_ghost, const int64_t *ghosts);
/* The SpMV row-block schedule cgx_csr_create builds (for tests). */
int cgx_row_blocks(const int *h_rowptr, int64_t n, int64_t *nrb, int **rb,
                   int *max_row_nnz);
void cgx_free_host(void *p);
/* Host-only: the SELL layout (rows_per_lane 1 or 2) cgx_csr_create would
 * build for a host CSR (DESIGN.md §SpMV formats). *nsl = 0 when the matrix
 * does not qualify.
 * slices[4 q .. 4 q + 3] = {first value slot, first index word, first
 * dictionary entry, width} of slice q; dict[ndict] = the offset pool (col -
 * row), idx[nidx] = 8 one-byte dictionary indices per word (0xff: padding);
 * value_slots = length of the value array. Release with cgx_free_host. */
/* ---- Matrix-Market ingest / emit (test/mm_reader.cpp read_file) ---------
 * cgx_mm_read: the reference loader's semantics (banner of 5 words, line 2
 * always discarded, '%' lines skipped, a size line, "i j v" triplets until
 * the first token that does not parse, off-diagonals always mirrored,
 * entries sorted by (row, col), empty rows dropped from rowptr), parsed with
 * `threads` threads (0: $OMP_NUM_THREADS or min(cores, 16)). Arrays are
 * host memory; release with cgx_free_host. Replaces read_file
 * (mm_reader.cpp:154-171).
 * cgx_mm_write_lower: the lower triangle as a `symmetric` file with one
 * comment line, values "%.17g" (reads back bit-identically). */
int cgx_mm_read(const char *path, int threads, int64_t *n, int64_t *nnz, int **rowptr,
                int **col, double **val);
int cgx_mm_write_lower(const char *path, int64_t n, const int *rowptr, const int *col,
                       const double *val, int threads);

/* Host-only: the SELL-P layout (2 rows per lane, slices of 128 rows): per
 * slice {first value slot, first 16-byte value-code chunk, first pattern
 * entry, pattern width}; pat[npat]
 * the sorted (col - row) patterns. *nsl = 0 when the matrix does not
 * qualify (a pattern wider than 32, unsorted rows, too much padding). */
int cgx_sellp_plan(const int *h_rowptr, const int *h_col, int64_t n, int64_t *nsl,
                   int64_t **slices, int64_t *npat, int **pat, int64_t *value_slots,
                   int *max_width);
/* The same plan formed on the device (cgx_csr_create's own path since round
 * 6): k_sellp_plan builds each slice's pattern with one wave, so the column
 * array never crosses to the host; the pattern pool, offsets and padding
 * bound follow on the host as above. Outputs as cgx_sellp_plan (free with
 * cgx_free_host). Needs a device. */
int cgx_sellp_plan_device(cgx_ctx *ctx, const int *d_rowptr, const int *d_col, int64_t n,
                          int64_t nnz, int64_t *nsl, int64_t **slices, int64_t *npat, int **pat,
                          int64_t *value_slots, int *max_width);
int cgx_sell_plan(const int *h_rowptr, const int *h_col, int64_t n, int rows_per_lane,
                  int64_t *nsl,
                  int64_t **slices, int64_t *ndict, int **dict, int64_t *nidx,
                  unsigned long long **idx, int64_t *value_slots);

/* ---- diagnostics ------------------------------------------------------------
 * Average device time (ms) of `iters` launches of the SpMV + p.Ap kernel in
 * variant `variant` (bit 1: XCD-contiguous split, 2: non-temporal val/col
 * loads, 4: paired 16-B/8-B loads), y = A x. For A/B tuning on one device. */
int cgx_tune_spmv(cgx_ctx *ctx, cgx_csr *A, int variant, const void *d_x, void *d_y,
                  int iters, double *avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* CGX_H */
