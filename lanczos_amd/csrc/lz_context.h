// Shared host-side state of the C ABI (lz_api.hip, lz_loops.hip, lz_matrix.hip, lz_ritz.hip, lz_twosided_api.hip, lz_orth.hip and the
// three solvers on it, lz_trl_api.hip, lz_gk_api.hip and lz_ztrl_api.hip, lz_zspmv.hip, lz_expm.hip, lz_minres.hip, lz_lsmr.hip): the handle, the error macros, the per-launch profiling scope and the helpers those files call across each other.  Internal: nothing
// here is part of include/lanczos_hip.h.
#pragma once

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <system_error>
#include <thread>

#include "lz_internal.h"

using lz::CsrDev;
using lz::QtwPlan;
using lz::Xfer;

struct EventRec {
  int cls;
  hipEvent_t a, b;
};

struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

// The polynomial p of A that the thick-restart solver multiplies by: with kind != kNone lz_trl_extend forms p(A) V[j] instead of A V[j].
// One at a time: lz_trl_set_filter and lz_trl_set_series both go through trl_set_poly (lz_trl_api.hip), which clears before it sets.
struct TrlPoly {
  enum Kind { kNone, kFilter, kSeries } kind = kNone;
  int degree = 0, coef_cap = 0;  // coef_cap: the doubles behind d_coef
  double c = 0.0, inv_e = 0.0;   // the centre of the damped interval (filter) or of the map to [-1, 1] (series); 1 / e of that map
  double* d_coef = nullptr;      // filter: a[0 .. degree), b[0 .. degree) of z = a_i (A y - c y) - b_i x; series: mu[0 .. degree]
  double* d_rot = nullptr;       // two work vectors of ld doubles each, rotated with trl.w (allocated when the first polynomial is set)
  double* d_acc = nullptr;       // the series' running sum, ld doubles (allocated when the first series is set)
  int64_t ld = 0;                // the row length d_rot and d_acc were allocated for
  void clear() { kind = kNone, degree = 0; }
};

// The Gram-Schmidt basis layer under the restart solvers (lz_orth.hip).  OrthBasis: one orthonormal row basis and the work vector that is
// orthogonalised against it and stored as its next row.  planes == 1: real.  planes == 2: planar complex - row j is the real rows 2 j
// (real part) and 2 j + 1 (imaginary part) of B, w is two rows ld apart; only the C ABI speaks interleaved complex128.  nrows counts
// rows of the basis' kind (complex rows of a complex basis: B holds planes * nrows real rows), and so does every row index the layer takes.
// h->trl follows the square matrix set last: trl_state (lz_trl_api.hip), which
// every lz_trl_* entry point behind lz_trl_begin calls first, sets its len and pad from h->rows / h->rows_pad on every call; code that
// uses h->trl without going through trl_state or trl_alloc reads the lengths of the last call that did.
struct OrthBasis {
  double* B = nullptr;  // planes * nrows real rows, ld doubles apart
  double* w = nullptr;  // planes * ld doubles; [len, ld) of each is zero whenever a walk reads it: the walks stream pad doubles, the products write len
  int64_t len = 0, pad = 0, ld = 0;  // the vectors' length, padded to kPadDoubles, and the (skewed) row stride
  int nrows = 0;        // sizes the walks' plan (orth_plan) and the head of the small arrays (orth_small_head)
  int planes = 1;       // 1: real, 2: planar complex
};
// What the bases of one solver share: the small arrays (head: OrthSmallHead, the rest the solver's own), the gate and the partials.
struct OrthWork {
  double* sm = nullptr;
  int* gate = nullptr;     // [0] gate of the second CGS pass
  double* part = nullptr;  // partials of the passes, the products and the residual norms
  size_t part_cap = 0;
};
// c of pass 1 and of pass 2 (planes doubles per row, interleaved; row nrows is the self slot), nrm2 + a scratch slot; the solver's own
// arrays start at end
struct OrthSmallHead {
  int64_t c1, c2, nrm2, end;
};
inline OrthSmallHead orth_small_head(int nrows, int planes = 1) {
  const int64_t cl = lz::qtw_ldp(planes * (nrows + 1)) + 16;
  return {0, cl, 2 * cl, 2 * cl + 8};
}

// Golub-Kahan-Lanczos bidiagonalisation (lz_gk_api.hip, lanczos_amd.svds): a rectangular operator and two bases of their own, separate
// from the handle's square operator, its fixed-n run and its thick-restart basis.  A is p x q (p >= q), AT its transpose - or, after
// lz_gk_set_dense, D.S is the one dense copy of either of them and A, AT are empty: gk_product (lz_gk_api.hip) is the only place that asks.
struct GkState {
  bool set = false;
  CsrDev A, AT;
  lz::DenseDev D;    // D.S != nullptr: the operator is dense
  int m = 0;         // 0: no basis (lz_gk_begin)
  int u_ready = -1;  // k: U[k] was made by lz_gk_probe, so lz_gk_extend(k, ..) starts step k at its second half
  OrthBasis U;       // the long side (len p): m + 1 rows (row m stays zero: launch_trl_restart copies it to row kk); w = A V[j]
  OrthBasis V;       // the short side (len q): m + 1 rows; w = z = A^T U[j]
  OrthWork wk;       // small arrays: see gk_small_layout in lz_gk_api.hip
};

// Complex Hermitian operator and its thick-restart basis (lz_zspmv.hip, lz_ztrl_api.hip; lanczos_amd.eigsh on complex input).  While a
// complex matrix is set h->kind stays 0, so every real entry point answers "no matrix set"; h->rows / h->rows_pad are the complex
// matrix' n and its padding.  The basis is a two-plane OrthBasis of its own, separate from h->trl: a real and a complex basis coexist
// on a handle across matrix swaps.
struct ZState {
  int kind = 0;  // 0 none, 1 CSR, 2 dense
  int64_t n = 0, nnz = 0;
  int32_t* rowptr = nullptr;
  int32_t* colidx = nullptr;
  double* vals = nullptr;   // CSR: 2 nnz doubles (re, im interleaved); dense: 2 n n, row-major
  int group = 1;            // lanes per row of the CSR product (a power of two <= 64, from the mean row length)
  double* xtmp = nullptr;   // lz_zspmv_host: x and y in planar form (4 padded vectors)
  int64_t xtmp_pad = 0;
  OrthBasis B;              // planes == 2, m + 1 complex rows
  OrthWork wk;              // small arrays: see ztrl_small_layout in lz_ztrl_api.hip
  int m = 0;
};

// Matrix exponential action (lz_expm.hip; lanczos_amd.expm_multiply): the propagator's basis, real (planes == 1) or planar complex, of
// its own beside h->trl and h->z.B, so eigsh's bases survive a propagation on the same handle and the other way round.  The matrix is
// whichever is set: the real one (h->kind != 0; with a planar basis the product is the mixed one) or the complex one (h->z.kind != 0).
struct ExpmState {
  OrthBasis B;              // m + 1 rows
  OrthWork wk;              // small arrays: see expm_small_layout in lz_expm.hip; part also takes the real product's partials
  int m = 0;
  int form = 0;             // lz_expm_set_product: 0 auto, 1 two launches of the real product, 2 the two-plane kernel
  int product = 0;          // the form the last mixed product took: 0 none yet, 1 two launches of the real product, 2 the two-plane kernel
  double* xtmp = nullptr;   // lz_zspmv_real_host: x and y in planar form (4 padded vectors)
  int64_t xtmp_pad = 0;
};

// MINRES (lz_minres.hip; lanczos_amd.minres): (A - shift I) x = b on the real matrix set.  No basis: seven padded vectors of ld doubles
// each behind vec, in this order - V[0], V[1] (v_j lives in V[j & 1]), Y (the product), R (the un-normalised residual: v_{k} = R / nu),
// W[0], W[1] (w_j lives in W[j & 1]), X - and the small device state of minres_layout (lz_minres.hip).  Between two calls of the ABI
// the pending update of the lagged step is applied (the flush), so steps / done below mirror the device.
struct MinresState {
  double* vec = nullptr;   // 7 * ld doubles; [rows, ld) of each is zero
  double* ds = nullptr;    // scalars (kMinresDoubles)
  int* di = nullptr;       // done, step counter (kMinresInts)
  double* part = nullptr;  // the product's alpha partials, then the step kernel's |r|^2 partials
  size_t part_cap = 0;
  double* hist = nullptr;  // phibar after every step
  int hist_cap = 0;
  int64_t ld = 0;
  bool live = false;       // lz_minres_begin / lz_minres_set_state ran on the matrix now set
  int steps = 0;           // steps done (the device's counter, as of the last synchronisation)
  int done = 0;
};

// LSMR (lz_lsmr.hip; lanczos_amd.lsmr): min |A x - b|^2 + damp^2 |x|^2 on the rectangular matrix h->gk holds (A is that matrix or, with
// transposed, its transpose).  No basis: two padded vectors of b's length behind bvec - UH (the un-normalised u: u_k = UH / nu_u), Y (the
// product A v) - and five of x's length behind xvec - VH (the un-normalised v: v_k = VH / nu_v), Z (the product A^T u), H, HBAR, X - and
// the small device state of lz_lsmr.hip.  Between two calls of the ABI the pending update of the lagged step is applied (the flush),
// so steps / done below mirror the device.
struct LsmrState {
  double* bvec = nullptr;  // 2 * bpad doubles; [blen, bpad) of each is zero
  double* xvec = nullptr;  // 5 * xpad doubles; [xlen, xpad) of each is zero
  double* ds = nullptr;    // scalars (kLsmrDoubles)
  int* di = nullptr;       // done, step counter, istop, fresh (kLsmrInts)
  double* part = nullptr;  // the partials of |u|^2, |v|^2, |x|^2 (kLsmrMaxBlocks each) and a spare set for lz_lsmr_begin
  double* hist = nullptr;  // normr, normar after every step
  int hist_cap = 0;
  int64_t blen = 0, bpad = 0, xlen = 0, xpad = 0;
  int transposed = 0;
  bool live = false;       // lz_lsmr_begin / lz_lsmr_set_state ran on the gk matrix now set
  bool pending = false;    // the update of the last step has not been applied (behind begin / set_state: the flush of a run applies it)
  int steps = 0;           // steps done (the device's counter, as of the last synchronisation)
  int done = 0;
};

// BiCGSTAB (lz_bicgstab.hip; lanczos_amd.bicgstab): A x = b on the real square matrix set, symmetric or not.  No basis: six padded
// vectors of ld doubles each behind vec, in this order - X, R (the residual; s = r - alpha v between the two products of an
// iteration, in place), RT (the shadow residual r~), P, V (= A p), T (= A s) - and the small device state of lz_bicgstab.hip.
struct BicgstabState {
  double* vec = nullptr;   // 6 * ld doubles; [rows, ld) of each is zero
  double* ds = nullptr;    // scalars (kBicgstabDoubles)
  int* di = nullptr;       // done, iteration counter, code, exit kind ... (kBicgstabInts)
  double* part = nullptr;  // the products' x_own . y partials, then four sets of the passes' own
  size_t part_cap = 0;
  double* hist = nullptr;  // |s|, |r| of every iteration
  int hist_cap = 0;        // in iterations (two doubles each)
  int64_t ld = 0;
  bool live = false;       // lz_bicgstab_begin / lz_bicgstab_set_state ran on the matrix now set
  bool fresh = false;      // the head tests of the coming iteration have not been applied yet (the next lz_bicgstab_run does, with its atol)
  int steps = 0;           // iterations done (the device's counter, as of the last synchronisation)
  int done = 0;
};

// Conjugate gradients (lz_cg.hip; lanczos_amd.cg): A x = b on the real square matrix set, taken as symmetric positive definite, with an
// optional diagonal preconditioner.  No basis: five padded vectors of ld doubles each behind vec, in this order - X, R, P, Q (= A p),
// D (the preconditioner's diagonal; zero and unread without one) - and the small device state of lz_cg.hip.
struct CgState {
  double* vec = nullptr;   // 5 * ld doubles; [rows, ld) of each is zero
  double* ds = nullptr;    // scalars (kCgDoubles)
  int* di = nullptr;       // done, iteration counter, code, exit kind ... (kCgInts)
  double* part = nullptr;  // the product's x_own . y partials, then two sets of the passes' own
  size_t part_cap = 0;
  double* hist = nullptr;  // |r| at every head test
  int hist_cap = 0;
  int64_t ld = 0;
  bool live = false;       // lz_cg_begin / lz_cg_set_state ran on the matrix now set
  bool fresh = false;      // the head test of the coming iteration has not been applied yet (the next lz_cg_run does, with its atol)
  bool given = false;      // rho of the fresh state was uploaded (lz_cg_set_state), not formed on the device
  bool pre = false;        // D holds a preconditioner
  int steps = 0;           // iterations done (the device's counter, as of the last synchronisation)
  int done = 0;
};

// Restarted GMRES (lz_gmres.hip; lanczos_amd.gmres): A x = b on the real square matrix set.  A basis of its own, max(m, 2) + 1 rows
// (m: the restart length), beside h->trl, h->z.B and h->ex.B, so eigsh's and eigs' thick-restart basis survives a solve on the same
// handle; B.w is the work vector of the steps and the residual b - A x of the cycle ends.  x and b: two padded vectors behind vec.
struct GmresState {
  OrthBasis B;
  OrthWork wk;              // small arrays: see gmres_small_layout in lz_gmres.hip; part also takes the products' partials
  int m = 0;                // the restart length the basis was allocated for
  double* vec = nullptr;    // 2 * B.ld doubles: x, b; [rows, ld) of each is zero
  int* di = nullptr;        // done, inner exit, breakdown, converged, cols, steps, cycles (kGmresInts)
  double* rpart = nullptr;  // the partials of |b - A x|^2
  double* hist = nullptr;   // presid of every inner step
  int hist_cap = 0;
  double* chist = nullptr;  // rnorm, cols, ptol of every cycle
  int chist_cap = 0;        // in cycles (three doubles each)
  bool live = false;        // lz_gmres_begin / lz_gmres_set_state ran on the matrix now set
  bool fresh = false;       // the first test has not been applied yet (the next lz_gmres_run does, with its atol)
  bool pending = false;     // the last synchronisation showed an inner exit inside a cycle: the next call begins with that cycle's end
  int hcol = 0;             // the column the next step of the host's loop makes (the device's cols wherever no flag is set)
  int iters = 0, cycles = 0, done = 0;  // the device's counters, as of the last synchronisation
};

constexpr int kTuneKnobs = 24;  // lz_set_tuning's indices 0 .. 23

struct lz_context {
  int dev = 0;
  hipStream_t stream = nullptr;
  std::string err;
  std::string name;
  int flags = 0;
  int tune[kTuneKnobs] = {0};  // A/B knobs, see lz_set_tuning

  // partition
  int64_t Mg = 0, row0 = 0, rows = 0, ncols_ext = 0;
  int64_t rows_pad = 0;  // owned rows padded to 32 doubles
  int64_t ldv = 0;       // stride between basis rows (>= rows_pad, + ghost tail in halo mode)

  // matrix
  int kind = 0;  // 0 none, 1 csr, 2 dense
  CsrDev csr;
  double* d_dense = nullptr;
  int64_t dense_lda = 0;  // row stride of the device copy (even: 16-byte aligned rows)

  // basis and work vectors
  int n = 0;
  double* d_V = nullptr;
  double* d_r = nullptr;
  double* d_r2 = nullptr;     // fused small-problem path: r of the three-term recurrence (d_r then holds the SpMV output)
  double* d_alpha = nullptr;  // n
  double* d_beta = nullptr;   // n
  double* d_c = nullptr;      // n + 1
  double* d_nrm2 = nullptr;   // 2 : [0] = ||r||^2
  double* d_part = nullptr;   // partials
  size_t part_cap = 0;
  double* d_xtmp = nullptr;   // lz_spmv_host scratch
  QtwPlan qplan;

  // two-sided Lanczos (IrrLanczos.py:77-187): H^T, the three extra bases P / Qb / Pb (Q is d_V), s, gamma, scalars
  CsrDev csrT;
  bool has_T = false;      // false: H declared symmetric, H^T x runs on csr
  bool T_declared = false; // lz_set_csr_transpose was called for the current matrix
  double* d_B3 = nullptr;  // 3 * n * ldv
  int bi_n = 0;
  double* d_s = nullptr;
  double* d_gamma = nullptr;  // n + 1
  double* d_bi = nullptr;     // [0..3] raw sums S, [4..6] factors f

  // Ritz vectors: Y = V^T-layout x S.  Resident (d_Y holds all y_rows rows) when it fits beside the basis; otherwise
  // CHUNKED: d_Y is a y_chunk-row buffer, the padded S stays on the device (d_S) and every consumer (Gram matrix, row
  // fetch, quality sums) re-forms the rows it needs - a 16-row tile of Y depends only on the same 16 columns of V.
  double* d_Y = nullptr;
  int64_t y_rows = 0;
  int y_n = 0;
  double* d_S = nullptr;
  int s_npad = 0;
  uint64_t* d_rclk = nullptr;  // in-kernel clock record of the last S-stationary back-transform (lz_ritz_info)
  double* d_gram = nullptr;    // scratch of lz_ritz_gram (K-slice partials + per-chunk slices + G), kept between calls
  size_t gram_cap = 0;
  uint64_t* d_gclk = nullptr;  // in-kernel clock record of the last symmetric Gram kernel (lz_gram_info)
  bool gram_sym_last = false;
  bool y_chunked = false;
  int64_t y_chunk = 0;     // rows per chunk (multiple of 16)
  int64_t y_cap = 0;       // doubles allocated behind d_Y

  // communication
  int world = 1, rank = 0;
  int comm_kind = 0;  // 0 none, 1 rccl, 2 host callbacks
  ncclComm_t comm = nullptr;
  lz_host_allreduce_fn h_ar = nullptr;
  lz_host_exchange_fn h_ex = nullptr;
  lz_host_allgather_fn h_ag = nullptr;
  void* h_user = nullptr;
  std::vector<double> hbuf_a, hbuf_b;
  int xmode = 0;  // 0 none, 1 halo, 2 allgather
  std::vector<int32_t> peers;
  std::vector<int64_t> scount, rcount, soff, roff;
  std::vector<int64_t> sstart;  // >= 0: the peer's send list is the contiguous run x[sstart .. sstart+scount) (stencil faces)
  bool all_contig = false;
  // LZ_FLAG_OVERLAP_HALO: the boundary positions of V[j] are updated first, their halo exchange runs on `cstream`
  // while the compute stream updates the interior; the SpMV waits for `e_halo`.
  hipStream_t cstream = nullptr;
  hipEvent_t e_bnd = nullptr, e_halo = nullptr;
  int halo_inflight_j = -1;
  std::vector<std::pair<int64_t, int64_t>> bnd_ranges, int_ranges;  // double2 position ranges of a basis row
  int64_t total_send = 0, total_recv = 0;
  int64_t n_allreduce = 0, n_exchange = 0;            // collectives issued since the last lz_get_timings ...
  int64_t n_allreduce_last = 0, n_exchange_last = 0;  // ... and in the interval that call closed (lz_comm_counts)
  int32_t* d_send_idx = nullptr;
  double* d_sendbuf = nullptr;
  int64_t ag_chunk = 0;
  double* d_xfull = nullptr;

  // timing
  std::vector<EventRec> events;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> free_events;
  hipEvent_t run_a = nullptr, run_b = nullptr;
  bool run_timed = false;
  // the per-run record - last_engine, last_sweeps, last_misses, last_gate_trips, last_os_fused, last_os_pairs, last_pair_abandoned, last_os_quads, last_quad_abandoned, sweep_log,
  // host_syncs, r_state: reset in one place, RunFrame::begin (lz_loops.hip), by lz_run and by both resumes
  int last_sweeps = 0;
  std::vector<int> sweep_log;  // per step of the last lz_run: 1 = the re-orthogonalisation sweep ran (lz_last_sweep_log; device-decided loops only, else all 1)
  int last_misses = 0;  // one-reduce partial loop: vectors whose exact omega exceeded sqrt(eps) although the look-ahead gate had not swept them
  int last_engine = 0;  // which loop ran last (enum Loop)
  int r_state = 0;      // what d_r holds after the last run: 0 nothing usable, 1 the residual entering step n, 2 y = A v_{n-1} (three-term pending)
  Xfer* xfer = nullptr;        // staging ring of the large device -> host copies (lz_xfer.hip), created at the first one
  double* h_pinned = nullptr;  // 8 pinned doubles for the per-step scalar read-back of the host-decided partial-reorth loop (tune[18] == 1)
  double* d_os = nullptr;      // one-sweep loop: G (n x n), H (n x n), c_hat (n + 1), correction g (2n), max |e| per step (n), the group form's predictions (4 (n + 4)), the group chain's ||z||^2 partials (2048) and b_3 (8); os_n = its n
  int* d_osi = nullptr;        //   ... [0] gate of the correcting sweep, [1] gate trips of the run, [3] / [4] a pair's / a group's leftover exceeded tau
  int os_n = 0;
  int os_step_n = 0;           //   ... the n of the state lz_os_state_set left in d_os (0: none; a run lays d_os out for its own n)
  // The group form's side stream (one_sweep_quad_iter; knob 15 = 13 keeps it on the main stream): behind a group walk the second-stage sums, post and the chat prediction
  // run on os_stream beside the closing product and the next chain.  os_side_pending: such work is in flight and e_os_ready not yet
  // waited for - whatever reads G, H, chat, the flags, elog or d_c next joins first (one_sweep_join).  d_ospart: the alpha partials of
  // the chain's and the closing products (d_part still holds the walk's while the side stream adds them up).
  hipStream_t os_stream = nullptr;
  hipEvent_t e_os_walk = nullptr, e_os_alpha = nullptr, e_os_ready = nullptr;
  bool os_side_pending = false;
  double* d_ospart = nullptr;
  size_t ospart_cap = 0;
  // lz_os_step's tap: check_launch copies the first tap_count doubles of d_part to d_tap behind the launch named tap_what (the walk of
  // the step: later launches of the same step reuse the head of d_part).  nullptr outside lz_os_step.
  const char* tap_what = nullptr;
  double* d_tap = nullptr;
  size_t tap_cap = 0, tap_count = 0;
  int last_gate_trips = 0;     // one-sweep loop: steps of the last lz_run whose prediction missed by more than kOneSweepTau
  int last_os_fused = 0;       // one-sweep loop: 1 = the last lz_run took the fused form (no three-term pass)
  int last_os_pairs = 0;       // one-sweep loop: pair walks (one walk per two steps) behind the last lz_run's result; 0 after a repeat
  int last_pair_abandoned = 0; // 1 = the last run (lz_run or a resume) tried the pair form, a leftover exceeded kOneSweepTau and the run was repeated on the single form
  bool pair_tripped = false;   // remembered until the matrix is set again: the pair form is not tried a second time
  int last_os_quads = 0;       // one-sweep loop: group walks (one walk per four steps) behind the last lz_run's result; 0 after a repeat
  int last_quad_abandoned = 0; // 1 = the last run tried the group form, a leftover exceeded kOneSweepTau and the run was repeated on the pair form
  bool quad_tripped = false;   // remembered until the matrix is set again: the group form is not tried a second time
  double* d_om = nullptr;      // device-resident partial re-orthogonalisation: omega-recurrence state (omega_state_doubles)
  int* d_omi = nullptr;        //   ... gate of the coming step, sweep count, per-step sweep log (omega_state_ints)
  int om_n = 0;
  int om_run_n = 0;            // n of the last device-decided partial run: the layout of d_om (lz_get_omega_state)
  int64_t host_syncs = 0;      // host <-> device synchronisations between the first and the last launch of the last run (lz_run or a resume)
  // lz_reserve (may be called from a second host thread while this one prepares the matrix): device buffers for the basis and
  // the Ritz vectors of the coming run, adopted by basis_alloc / lz_ritz_vectors.  Only these fields are touched by it.
  std::mutex res_mu;
  double* res_V = nullptr;
  size_t res_V_count = 0;
  double* res_Y = nullptr;
  size_t res_Y_count = 0;
  // thick-restart Lanczos (lz_trl_api.hip): a basis of its own (trl_m + trl_b rows), never the fixed-n run's d_V / d_Y
  OrthBasis trl;               // w = A V[j], then the residual
  int trl_m = 0;
  int trl_b = 1;               // residual rows behind the m basis rows: 1 (lz_trl_begin) or the band width (lz_trl_begin_band)
  double* d_tW = nullptr;      // band Lanczos: the trl_b work vectors of a batch (trl.ld apart)
  OrthWork trl_wk;             // small arrays: see trl_small_layout in lz_trl_api.hip
  TrlPoly poly;  // none, the Chebyshev filter or the Chebyshev series
  GkState gk;    // Golub-Kahan-Lanczos (lz_gk_*): freed by gk_free
  ZState z;      // complex Hermitian matrix and its thick-restart basis (lz_set_*_cplx, lz_ztrl_*): freed by z_free
  ExpmState ex;  // the propagator's basis (lz_expm_*): freed by expm_free
  MinresState mr;  // the linear solver's vectors (lz_minres_*): freed by minres_free, dropped by every matrix setter (z_drop_matrix)
  LsmrState ls;    // the least-squares solver's vectors (lz_lsmr_*): freed by lsmr_free, dropped by lz_gk_set_csr / lz_gk_set_dense
  BicgstabState bc;  // the non-symmetric solver's vectors (lz_bicgstab_*): freed by bicgstab_free, dropped by every matrix setter (z_drop_matrix)
  GmresState gm;     // the restarted solver's basis and vectors (lz_gmres_*): freed by gmres_free, dropped by every matrix setter (z_drop_matrix)
  CgState cg;        // the conjugate-gradient solver's vectors (lz_cg_*): freed by cg_free, dropped by every matrix setter (z_drop_matrix)
  bool prof_iter = true;  // false while lz_run skips an iteration under profile sampling (tune[7])
  lz_timings acc;
};

namespace lz {
namespace api {

extern std::string g_create_error;
extern RcclApi g_rccl;
extern std::string g_rccl_path;
const char* load_rccl();  // nullptr, or why RCCL could not be loaded

int fail(lz_handle h, int code, const std::string& msg);

#define LZ_HIP(h, call)                                                                                   \
  do {                                                                                                    \
    hipError_t e_ = (call);                                                                               \
    if (e_ != hipSuccess)                                                                                 \
      return fail(h, e_ == hipErrorOutOfMemory ? LZ_ERR_NOMEM : LZ_ERR_HIP,                               \
                  std::string(#call) + ": " + hipGetErrorString(e_));                                     \
  } while (0)

#define LZ_NCCL(h, call)                                                                                  \
  do {                                                                                                    \
    ncclResult_t r_ = (call);                                                                             \
    if (r_ != ncclSuccess) return fail(h, LZ_ERR_COMM, std::string(#call) + ": " + g_rccl.GetErrorString(r_)); \
  } while (0)

#define LZ_TRY(expr)          \
  do {                        \
    int rc_ = (expr);         \
    if (rc_ != LZ_OK) return rc_; \
  } while (0)

int64_t skew_stride(lz_handle h, int64_t ld);
int check_launch(lz_handle h, const char* what);

// large buffers (>= kBigMinBytes: the basis, the Ritz vectors, a dense matrix): a reserved virtual range backed by physical chunks
// instead of hipMalloc, whose 16 GB calls stall for seconds now and then on this pool (lz_api.hip); big_free releases either kind
constexpr size_t kBigMinBytes = (size_t)256 << 20;
hipError_t big_alloc(int dev, void** out, size_t bytes);
hipError_t big_free(void* p);
void big_vmm_disable();  // from now on big_alloc uses hipMalloc (process-wide)

template <class T>
inline int dev_free(lz_handle h, T*& p) {
  if (p) {
    LZ_HIP(h, big_free(p));
    p = nullptr;
  }
  return LZ_OK;
}

template <class T>
inline int dev_alloc(lz_handle h, T*& p, size_t count) {
  LZ_TRY(dev_free(h, p));
  void* q = nullptr;
  LZ_HIP(h, big_alloc(h->dev, &q, std::max<size_t>(count, 1) * sizeof(T)));
  p = static_cast<T*>(q);
  return LZ_OK;
}

int upload(lz_handle h, void* dst, const void* src, size_t bytes);
int upload2d(lz_handle h, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height);

// per-launch accounting (algorithmic bytes / flops per kernel class), optional hipEvent bracket and roctx range
struct Scope {
  lz_handle h;
  int cls;
  hipEvent_t a = nullptr, b = nullptr;
  bool on;
  bool marked = false;
  hipStream_t st;  // the stream the bracket is recorded on
  Scope(lz_handle h_, int cls_, double bytes, double flops, hipStream_t stream = nullptr);  // nullptr: h->stream
  ~Scope();
};
int drain_events(lz_handle h);

// collectives (RCCL or host-staged)
int comm_allreduce(lz_handle h, double* dbuf, int64_t count);
int comm_exchange_x(lz_handle h, int j, const double** x_out);

// the individual steps of the recurrence (lz_loops.hip)
int ensure_part(lz_handle h, size_t need);
double spmv_bytes(lz_handle h, bool ell = false);  // ell: the launch takes the ELL copy whatever the plain SpMV does (the partial loop's fused SpMV)
double spmv_flops(lz_handle h);
int step_spmv(lz_handle h, int j, double* alpha_dst = nullptr, bool reduce = true, int* np_out = nullptr);
int step_reorth(lz_handle h, int j, int nrows, bool scale, int beta_idx, bool in_run_loop = false);
int step_three_term(lz_handle h, int j, int jm1, const double* d_alpha, const double* d_beta, bool need_norm = true, int* np_out = nullptr,
                    double* r = nullptr, const char* what = "three_term");  // r: the residual buffer, nullptr = h->d_r; what: check_launch's name
size_t fused_coff(lz_handle h);
size_t onered_part_off(lz_handle h);
int breakdown_status(lz_handle h, int n, const double* alpha_out, const double* beta_out);

// basis (lz_api.hip)
int basis_alloc(lz_handle h, int n, int zero_rows);
int require_basis(lz_handle h, int j);
inline size_t y_doubles(int64_t rows, int n) { return (size_t)(round_up(rows, 16) + 16) * (size_t)n + 64; }

// matrix setup (lz_matrix.hip)
int fill_csr_meta(lz_handle h, CsrDev& A, const int32_t* rowptr_host, int64_t rows_local, int64_t ncols_ext, int64_t nnz, int fixed_k,
                  int max_nnz);
int upload_csr(lz_handle h, CsrDev& A, const char* who, int64_t rows, int64_t ncols, int64_t nnz, const int32_t* rowptr,
               const int32_t* colidx, const double* vals, int* fixed_k_out, int* max_nnz_out);

// Golub-Kahan-Lanczos state (lz_gk_api.hip): releases everything h->gk owns (lz_destroy)
void gk_free(lz_handle h);
// y = Aop x (transpose == 0) or Aop^T x with whichever rectangular operator h->gk holds (CSR or the one dense copy); y[len .. pad) = 0
hipError_t gk_product(lz_handle h, int transpose, const double* x, double* y, int64_t pad);

// complex Hermitian state (lz_zspmv.hip).  z_drop_matrix: what every real matrix setter calls - the complex matrix is gone (its basis
// stays allocated for the next one); z_free: everything h->z owns (lz_destroy)
int z_drop_matrix(lz_handle h);
void z_free(lz_handle h);
// w = A x on the complex matrix, planar vectors (real part at x / y, imaginary part at x + ld / y + ld); writes n entries of each part
void z_matvec(lz_handle h, const double* x, double* y, int64_t ld);

// matrix exponential action (lz_expm.hip): releases everything h->ex owns (lz_destroy)
void expm_free(lz_handle h);

// MINRES (lz_minres.hip): releases everything h->mr owns (lz_destroy)
void minres_free(lz_handle h);

// LSMR (lz_lsmr.hip): releases everything h->ls owns (lz_destroy)
void lsmr_free(lz_handle h);

// BiCGSTAB (lz_bicgstab.hip): releases everything h->bc owns (lz_destroy)
void bicgstab_free(lz_handle h);

// GMRES (lz_gmres.hip): releases everything h->gm owns (lz_destroy)
void gmres_free(lz_handle h);

// CG (lz_cg.hip): releases everything h->cg owns (lz_destroy)
void cg_free(lz_handle h);

// Gram-Schmidt basis layer (lz_orth.hip): what lz_trl_*, lz_gk_* and lz_ztrl_* all do with an OrthBasis, real or planar complex, and
// its OrthWork.  Row counts and indices are in rows of the basis' kind; coefficients of a complex basis are interleaved complex.
QtwPlan orth_plan(lz_handle h, const OrthBasis& b);  // (a complex basis' walks plan themselves: an empty plan)
// c[0 .. n) = <B[0 .. n), w>, c[n] = <w, w> (the self slot); gate: the launches return at once where gate[0] == 0
int orth_dots(lz_handle h, const OrthBasis& b, const OrthWork& wk, const QtwPlan& plan, int n, double* c, const int* gate = nullptr);
// row k = w made orthogonal to rows [0, k) by two CGS passes, normalised; synchronises.  what: the name check_launch reports
int orth_store(lz_handle h, const OrthBasis& b, const OrthWork& wk, const QtwPlan& plan, int k, const char* what);
// one extension step: w against rows [0, nb) - CGS and a second pass -, its norm to norm_slot, w / norm to row nb.  proj: where the nb
// measured coefficients go (both passes' sums).  nb == 0: the norm only (real bases).  No check_launch, no synchronisation: the caller's.
enum class OrthPass2 {
  kGated,    // the DGKS gate: pass 2's launches return at once unless pass 1 cancelled more than half of |w|^2
  kForced,   // the same gated launches, the gate always set (LZ_FLAG_TRL_PASS2_ALWAYS)
  kUngated,  // pass 2's launches take no gate at all (the tail of a band batch, on a view of the rows the batch has made; real bases)
};
int orth_cgs_step(lz_handle h, const OrthBasis& b, const OrthWork& wk, const QtwPlan& plan, int nb, double* proj, double* norm_slot,
                  OrthPass2 pass2);
// Across the ABI a real basis moves raw doubles, a complex one interleaved complex128 without padding:
int orth_upload_x(lz_handle h, const OrthBasis& b, const double* x);         // w = x (len elements), zero beyond len
int orth_get_vectors(lz_handle h, const OrthBasis& b, int k, double* out);  // out (len x k elements, row-major) = rows [0, k) transposed
// rows j0 .. j0 + count - 1, ld elements apart on the host.  Real: raw rows with their padding, ld >= pad.  Complex: ld >= len, the
// padding is written as zero on set.  who, top: the caller and its name for the last row, for the argument error's text
int orth_set_rows(lz_handle h, const OrthBasis& b, const char* who, const char* top, int j0, int count, const double* rows, int64_t ld);
int orth_get_rows(lz_handle h, const OrthBasis& b, const char* who, const char* top, int j0, int count, double* rows, int64_t ld);
// n interleaved complex z <-> the planes re and im
void to_planar(const double* z, int64_t n, double* re, double* im);
void to_interleaved(const double* re, const double* im, int64_t n, double* z);
// out[i] (device) = |y_i - theta_i B_i|, i < k, where product(i) leaves y_i in b.w; theta on the device.  No check_launch, no synchronisation.
int orth_resid_norms(lz_handle h, const OrthBasis& b, const OrthWork& wk, int k, const double* theta, double* out,
                     const std::function<hipError_t(int)>& product);
// partials that the sequences above and m residual norms need; the solver adds its own terms and reserves the largest
size_t orth_part_need(const OrthBasis& b, const QtwPlan& plan, int m);
int orth_part_reserve(lz_handle h, OrthWork& wk, size_t need);
void orth_free(OrthBasis& b);
void orth_free(OrthWork& wk);

}  // namespace api
}  // namespace lz
