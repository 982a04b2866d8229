// Internal declarations shared by the kernel translation units and the C ABI.
// gfx950 (MI355X / CDNA4) only: wave = 64 lanes, 256 CUs in 8 XCDs.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "lanczos_hip.h"

namespace lz {

constexpr int kWave = 64;
constexpr int kTPB = 256;          // threads per block for all streaming kernels
constexpr int kPadDoubles = 32;    // vectors are padded to 256-byte multiples
constexpr int kNumCU = 256;
constexpr int kNumXCD = 8;

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

int xfer_threads();
// run fn(t, lo, hi) over [0, count) on a few host threads (the validation sweeps over all nnz of lz_set_csr)
template <class F>
inline void parallel_ranges(int64_t count, int64_t min_per_thread, F fn) {
  const unsigned hc = std::thread::hardware_concurrency();
  int T = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(16, hc ? hc / 2 : 1), count / std::max<int64_t>(min_per_thread, 1)));
  if (xfer_threads() == 0) T = 1;  // LZ_XFER_THREADS=0: no helper threads anywhere
  std::vector<std::thread> pool;
  const int64_t per = (count + T - 1) / T;
  int started = 0;
  try {
    for (int t = 1; t < T; ++t) {
      pool.emplace_back(fn, t, std::min(count, t * per), std::min(count, (t + 1) * per));
      ++started;
    }
  } catch (const std::system_error&) {
  }
  fn(0, (int64_t)0, std::min(count, per));
  for (int t = started + 1; t < T; ++t) fn(t, std::min(count, t * per), std::min(count, (t + 1) * per));  // threads that could not be had
  for (auto& th : pool) th.join();
}
constexpr int kMaxHostThreads = 16;

// ---- CSR SpMV ----------------------------------------------------------
struct CsrDev {
  int64_t rows = 0, ncols = 0, nnz = 0;
  int32_t* rowptr = nullptr;
  int32_t* colidx = nullptr;
  double* vals = nullptr;
  int fixed_k = 0;            // > 0: every row has exactly fixed_k entries
  int32_t* rowblk = nullptr;  // CSR-stream row blocks: rows [rowblk[b], rowblk[b+1])
  int n_rowblk = 0;
  int fixed_rb = 512;         // rows per block of the fixed-K kernel
  int blk_nnz_cap = 4096;     // products per row block (LDS tile of the CSR-stream kernel)
  int max_row_nnz = 0;
  double avg_row_nnz = 0;
  double far_frac = 0;        // share of entries whose column is > 2^18 away from their row: no L2 reuse of x to speak of
  struct PbDev* pb = nullptr; // column-blocked two-phase layout (lz_spmv_pb.hip), built when the matrix has no column locality
  // ELL-ordered copy of a fixed-K matrix (lz_spmv.hip, k_spmv_ell): blocks of ell_rb rows, entry k of every row of a block
  // contiguous - a lane owns whole rows, its loads and the stencil's gathers are coalesced, no LDS transposition.
  int32_t* ell_c = nullptr;
  double* ell_v = nullptr;
  int ell_rb = 0;             // rows per block of the ELL copy (0: none)
  int ell_variant = 0;        // 0: one row per lane and trip (rows t, t + 256, ...); 1: two adjacent rows per lane (16-byte loads)
  bool ell_default = false;   // true: every SpMV takes the ELL copy (knob 17 >= 2, or a row-class coded one); false: only the partial loop's fused SpMV does
  // row-class coding of the ELL copy (round 5; k_spmv_ell, CODED): one byte per row names its class; a class is the row's K offsets
  // col - row (ell_coded >= 1: ell_c is not kept) and, for constant coefficients, its K values (ell_coded == 2: ell_v is not kept either)
  uint8_t* ell_cls = nullptr;
  int32_t* cls_off = nullptr; // [256][K]
  double* cls_val = nullptr;  // [256][K]
  double* cls_diag = nullptr; // ell_coded == 3: the diagonal's values, one per row (the class holds the offsets and the OTHER values)
  int ell_coded = 0;
  int ell_ncls = 0;
  int cls_group = 0;          // knob 23: 0 k_spmv_cls2 (two adjacent rows per lane); 1 / 3: k_spmv_cls with one / two units per workgroup (A/B)
  const int32_t* host_colidx = nullptr;  // the caller's arrays, valid ONLY inside lz_set_csr / lz_set_csr_transpose (pb_build reads them)
  const double* host_vals = nullptr;
  // rectangular product (lz_gk.hip; only the matrices of lz_gk_set_csr have these, and they have none of the layouts above): work items
  // of four int32 each - a block of whole rows or one segment of a long row -, the long rows and their segment partials
  int32_t* rect_items = nullptr;
  int n_rect = 0;
  int32_t* rect_long = nullptr;
  int n_rect_long = 0;
  double* rect_seg = nullptr;
};

// ---- rectangular product (lz_gk.hip): y = A x for rows != ncols in either direction, no x_own . y epilogue, y[rows .. rows_pad) = 0.
// rect_plan (host): the work items for tiles of nnz_cap products; split == false keeps a long row in one workgroup (A/B arm).
void rect_plan(const int32_t* rowptr, int64_t rows, int nnz_cap, bool split, std::vector<int32_t>& items, std::vector<int32_t>& lrows,
               int* nslots);
hipError_t launch_spmv_rect(const CsrDev& A, const double* x, double* y, int64_t rows_pad, hipStream_t s);

// ---- dense rectangular product (lz_gk.hip; lz_gk_set_dense): ONE row-major copy S (R x C, stride ld: even, >= C, a padding column is
// zero) of the caller's array, which is the tall operator Aop (stored_t == false) or its transpose.  rowdot: out[r] = sum_c S[r, c] x[c];
// colsum: out[c] = sum_r S[r, c] u[r].  Stored tall, Aop x is rowdot and Aop^T u colsum; stored wide the other way round.  Both follow
// launch_spmv_rect's contract: out[len .. pad) = 0, the input read at valid positions only, no atomics, one summation order per plan.
// The form codes are lz_gk_plan's (include/lanczos_hip.h).
enum DenseForm {
  kRdShort = 1,  // rowdot: a lane group of rd_group lanes per row, several rows per wave (rows of up to kDenseShortMax)
  kRdWave = 2,   // rowdot: one wave per row (gemv_row_wave)
  kRdSeg = 3,    // rowdot: a row cut into rd_nseg segments of rd_seg doubles, a wave per segment of four rows, partials folded in segment order
  kCsSlab = 11,  // colsum: 128-column tiles x slabs of cs_slab rows, partials folded in slab order
  kCsOne = 12,   // colsum: the same tiles, one slab holds every row: written directly, no fold
  kCsNarrow = 13 // colsum: cs_group lanes cover a row, 256 / cs_group rows per trip, combined through LDS; slabs folded in order
};
struct DenseDev {
  double* S = nullptr;
  int64_t R = 0, C = 0, ld = 0;
  bool stored_t = false;
  int rd_form = 0, rd_group = 0, rd_nseg = 0;
  int64_t rd_seg = 0;
  int cs_form = 0, cs_group = 0, cs_nslab = 0;
  int64_t cs_slab = 0;
  double* rd_part = nullptr;  // rd_nseg x round_up(R, 32)
  double* cs_part = nullptr;  // cs_nslab x round_up(C, 32)
};
constexpr int kDenseTileCols = 128;  // colsum: at most this many columns per workgroup tile (a wave's 16-byte loads)
constexpr int kDenseShortMax = 128;  // rowdot: the longest row of the lane-group form
constexpr int kDenseShortRows = 4;   // ... and the rows a lane group has in flight
constexpr int kDenseMediumMax = 1024;// rowdot: up to this length a wave takes four whole rows (the segment form with one segment)
constexpr int kDenseSegRows = 4;     // rowdot segments: adjacent rows per wave (they share the loads of x)
constexpr int kDenseSegMaxRows = 768;// ... and the row count from which one wave per row fills the device
constexpr int kDenseFoldSub = 16;    // fold: lanes that share one output, each adding every 16th partial
// dense_plan (host): the forms and their sizes from R, C and the CU count; force_* / seg_knob / slab_knob: tuning knobs 14, 4 and 2 (0 auto)
void dense_plan(DenseDev& D, int force_rd, int force_cs, int seg_knob, int slab_knob);
hipError_t launch_dense_rowdot(const DenseDev& D, const double* x, double* out, int64_t pad, hipStream_t s);
hipError_t launch_dense_colsum(const DenseDev& D, const double* u, double* out, int64_t pad, hipStream_t s);

// ---- column-blocked two-phase SpMV (lz_spmv_pb.hip): gathers out of LDS only; y bit-identical to the CSR-stream kernel
hipError_t pb_build(const CsrDev& A, const int32_t* rowptr_host, PbDev** out, hipStream_t s, int cap_knob = 0, int groups = 0);  // *out == nullptr: not applicable; groups > 1: the A/B arm of knob 22
void pb_free(PbDev*& pb);
int pb_num_partials(const PbDev* pb);
void pb_layout_info(const PbDev* pb, int64_t* np, int* in_bytes_x2, int* diag);
int launch_spmv_pb(const CsrDev& A, const PbDev* pb, const double* x, double* y, const double* x_own, double* part, hipStream_t s);

// launch wrappers (all asynchronous on `s`)
// y = A x (rows), part[b] = sum_{rows of block b} x_own[i] * y[i]; returns number of partials written
int launch_spmv_csr(const CsrDev& A, const double* x, double* y, const double* x_own, double* part, int flags,
                    hipStream_t s);
// ELL copy of a fixed-K matrix (K in {5, 7, 27}); variant as CsrDev::ell_variant.  ell_free releases it.
hipError_t ell_build(CsrDev& A, int variant, hipStream_t s, int coding = 0, bool plain_fallback = true);
void ell_free(CsrDev& A);
bool ell_usable(const CsrDev& A, int flags);
// The device-resident partial re-orthogonalisation loop's SpMV: when gate[0] == 0 (no sweep ran on this vector) the kernel
// forms v_j = r / sqrt(nrm2[0]) ITSELF wherever it reads an entry of x (IEEE division: the same bits wherever it is formed),
// stores the rows it owns to vj and beta to beta_slot; when gate[0] != 0 the sweep kernels have written vj and it is a plain
// y = A vj.  y must not alias r.  Returns the number of alpha partials.
struct EllCode {
  const double* diag = nullptr;  // coded 3: the value of the entry at offset 0 comes from here
  const uint8_t* cls = nullptr;
  const int32_t* off = nullptr;
  const double* val = nullptr;
  int ncls = 0;
};
struct SpmvScale {
  const double* r = nullptr;
  const double* nrm2 = nullptr;
  double* vj = nullptr;
  double* beta_slot = nullptr;
  const int* gate = nullptr;
};
// The Chebyshev filter step as the SpMV's epilogue (thick-restart Lanczos, lz_trl_api.hip): the lane that owns row r forms
// z[r] = a (sum - c x_own[r]) - b xprev[r] from its row sum (cheb_combine, lz_device.h: k_cheb_step's expression) and stores that instead
// of y[r]; a = coef[i], b = coef[degree + i] are read on the device.  y is not written, no alpha partials are formed.  z must alias
// neither x nor xprev.
// With acc set it is a step of the Chebyshev SERIES sum_i mu_i T_i(A^) x instead (series_combine, lz_device.h: k_cheb_series_step's
// expression): coef = mu[0 .. degree], i = 1 .. degree the term formed, z[r] = that term (nullptr on the last step: nothing reads it),
// acc[r] = acc_in[r] + mu_i z[r] (i = 1: mu_0 x_own[r] + mu_1 z[r]; acc_in and xprev are not read).  acc may be acc_in.
struct SpmvCheb {
  const double* xprev = nullptr;
  double* z = nullptr;
  const double* coef = nullptr;
  int i = 0, degree = 0;
  double c = 0.0;
  const double* acc_in = nullptr;
  double* acc = nullptr;
  double inv_e = 0.0;
};
int launch_spmv_ell(const CsrDev& A, const double* x, double* y, const double* x_own, double* part, hipStream_t s,
                    const SpmvScale* sc = nullptr, const SpmvCheb* ch = nullptr);
struct StencilArgs {  // by-value kernel argument of the stencil assembly
  int Nx, Ny, Nz, negate, pot_kind, renumber, nranges;
  int64_t row0, rows_local;
  double tf, w[4], par[8];
  int64_t gstart[16], glen[16], gext[16];  // ghost ranges: global start, length, first extended-local index
};
void launch_build_stencil3d(const StencilArgs& a, int points, const double* pot, int32_t* rowptr, int32_t* colidx, double* vals,
                            hipStream_t s);
int launch_gemv_dense(const double* A, int64_t M, int64_t cols, int64_t lda, const double* x, const double* x_own, double* y,
                      double* part, hipStream_t s);

// out[0] = sum(part[0..n)) (fixed order)
void launch_final_sum(const double* part, int n, double* out, hipStream_t s);
// c[i] = sum_b part[i*G + b]; transposed (4x4x4 MFMA kernel): c[i] = sum_b part[b*qtw_ldp(nrows) + i]
inline int qtw_ldp(int nrows) { return (nrows + 15) & ~15; }
void launch_final_rows(const double* part, int nrows, int G, double* c, hipStream_t s, bool transposed = false, const int* gate = nullptr);
void launch_final_rows_t(const double* part, int G, int ldp, int nout, double* c, hipStream_t s, const int* gate = nullptr);
// up to four independent k_final_sum's in one launch: out[q][0] = sum(part[q][0 .. n[q])) in k_final_sum's grouping
struct FinalMulti {
  const double* part[4];
  int n[4];
  double* out[4];
};
void launch_final_sum_multi(const FinalMulti& fm, int count, hipStream_t s);

struct QtwPlan {
  int64_t L = 0;    // elements of w owned by one block (multiple of 512)
  int G = 0;        // number of blocks
  int P = 0;        // partials per basis row (G for the VALU kernel, 4G for the MFMA kernel)
  bool mfma = false;
  int family = 2;   // 2 = 4x4x4 MFMA (default), 1 = 16x16x4 MFMA, 0 = VALU
  int variant = 0;  // A/B knob (unroll / rows per tile)
};
QtwPlan plan_qtw(int64_t len, int flags, const int* tune, int nrows_max);
// pass 1 of the re-orthogonalisation (+ optional v_j = r / sqrt(nrm2)):
//   part[i*G + b] = sum_{m in block b} V[i][m] * V[j][m],  i in [0, nrows)
// Fused small-problem mode of pass 1 (mode 4): the kernel's prologue finishes the previous step itself - alpha from the
// SpMV's block partials (k_final_sum's grouping), r = (y - alpha v_prev) - beta v_prev2 on its own slice - before it
// stages and dots r.  Three launches per Lanczos step instead of six, same bits.
struct QtwFuse {
  const double* apart = nullptr;  // alpha partials of the SpMV that produced y
  int np = 0;
  int jprev = 0, jprev2 = -1;     // basis rows of v_prev (the vector just multiplied) and v_prev2 (-1: none)
  const double* beta_prev = nullptr;
  double* alpha_out = nullptr;
  double* r_out = nullptr;        // where r goes (NOT y itself: with the row split several blocks read the same slice of y)
  const int* gate = nullptr;      // any mode: the kernel returns at once when gate[0] == 0 (device-resident partial re-orthogonalisation)
  unsigned* ticket = nullptr;     // mode 1: the last block to finish also adds up all blocks' runs into c_out (k_final_rows_t's order)
  double* c_out = nullptr;
};
// returns the error of the per-kernel LDS-limit raise (hipFuncSetAttribute), if that was needed and failed
hipError_t launch_qtw(double* V, int64_t ldv, int64_t len, int nrows, int j, const double* r, const double* nrm2,
                      double* beta_slot, const QtwPlan& plan, double* part, int mode, hipStream_t s, const QtwFuse* fuse = nullptr);
// pass 2: V[j] = 2 V[j] - sum_{i<nrows} c[i] V[i] (sequential, unfused: bitwise NumPy order)
// raw_c (fused mode only): c holds the reduced sums, beta = sqrt(c[j]) is formed and stored by the kernel itself
// raw_c == 2 (fused small-problem mode): c points at pass 1's block partials, cG runs of cldp doubles; the kernel adds
// them in k_final_rows_t's order itself
void launch_update(double* V, int64_t ldv, int64_t len, int nrows, int j, const double* c, const double* r_fused,
                   double* beta, int variant, hipStream_t s, int64_t pos_lo = 0, int64_t pos_hi = -1, int raw_c = 0,
                   int64_t pos_lo_b = 0, int64_t pos_hi_b = 0,  // second range: only with the small-range (face) kernel
                   int cG = 0, int cldp = 0, const int* gate = nullptr,
                   // one-reduce partial loop (r_fused, raw_c == 1, gate): w = (r_fused - asub[0] usub) / beta formed in the kernel; gate[0] == 0:
                   // V[j] = w (no sweep) instead of returning
                   const double* usub = nullptr, const double* asub = nullptr);
// gate != nullptr: runs only when gate[0] == 0 (the step without a sweep)
void launch_scale_store(double* vj, const double* r, const double* nrm2, double* beta_slot, int64_t len, hipStream_t s, const int* gate = nullptr);

// ---- one-sweep full re-orthogonalisation (run_loop_one_sweep, lz_loops.hip) ----
// G = V^T V and H (A V_i = sum_l H[l, i] V_l to rounding) are n x n, column-major (column i at [i * n]).  Per step j, in the
// units of u_j = w_j / beta_j: the sweep applies the predicted c_hat and measures d_i = V_i . u_j from the same loads; post
// forms e_i = d_i - c_hat_i and G[:, j]; predict forms the next step's c_hat from G, H, alpha and beta.  The per-entry
// arithmetic below is shared by the kernels and the host check (lz_one_sweep_host, tools/one_sweep_prototype.py).
constexpr double kOneSweepTau = 1e-14;  // gate: max |e| above this runs one correcting sweep (profiles/one_sweep_prototype.md)
constexpr int kOneSweepMaxN = 1536;     // the sweep parks 4 x qtw_ldp(n) per-wave dots in LDS (48 KiB)
constexpr int kOneSweepFusedMaxN = kOneSweepMaxN - 16;  // the fused form parks one slot more per wave (qtw_ldp(n + 1))
// c_hat_i of step j + 1 (i <= j): ((A V_i) . v_j - alpha_j G[i, j] - beta_j G[i, j-1]) / sqrt(nrm2)
__host__ __device__ inline double os_predict_one(int i, int j, int n, const double* H, const double* G, double a, double bj, double bn) {
  double s;
  if (i < j) {
    s = 0.0;
    for (int l = 0; l <= i + 1; ++l) s += H[(int64_t)i * n + l] * G[(int64_t)j * n + l];
  } else {
    s = a;  // V_j . A v_j: the SpMV's own dot
  }
  s = s - a * G[(int64_t)j * n + i];
  if (j > 0) s = s - bj * G[(int64_t)(j - 1) * n + i];
  return s / bn;
}
// G[i, j] (i < j) of v_j = (2 - cs) u_j - sum_{l<j} c_hat_l V_l: (2 - cs) d_i - sum_l c_hat_l G[i, l]
__host__ __device__ inline double os_post_one(int i, int j, int n, const double* G, const double* d, const double* chat, double cs) {
  double s = (2.0 - cs) * d[i];
  for (int l = 0; l < j; ++l) s -= chat[l] * G[(int64_t)l * n + i];
  return s;
}
// sweep (mode 0): V[j] = 2 u - (sum_{i<j} coef_i V_i + cs u), u = r / sqrt(nrm2) (beta stored to beta_slot); part[b * ldp + i] =
// block b's share of V_i . u (i < j) and, at i = j, of V[j] . V[j] (ldp = qtw_ldp(j + 1)).  Mode 1 (correction, runs only when
// gate[0] != 0): dst -= sum_{i<j} coef_i V_i, no dots.  Mode 2 (the fused form, j >= 1; r = y = A v_{j-1}): the sweep forms
// w = (y - alpha_prev V[j-1]) - beta_prev V[j-2] itself (k_three_term's expression; no beta term at j = 1) and works in the units of w:
// dst = u~ = 2 w - (sum_{i<j} coef_i V_i + w), coef the un-normalised predictions; part[b * ldp + i] = V_i . w (i < j), u~ . u~ (i = j),
// ||w||^2 (i = j + 1), ldp = qtw_ldp(j + 2).  dst == nullptr: V[j].  Returns the number of blocks (the partial runs).
int os_sweep_blocks(int64_t len);
int launch_os_sweep(int mode, double* V, int64_t ldv, int64_t len, int j, const double* coef, const double* r, const double* nrm2,
                    double* beta_slot, double* part, const int* gate, hipStream_t s, double* dst = nullptr, const double* alpha_prev = nullptr,
                    const double* beta_prev = nullptr);
// post (one block): d = [V_i . u_j (i < j), v_j . v_j] (the second-stage sums); writes G[:, j] / G[j, :], H[:, j-1]'s update
// part, and when max |e| > tau the correction g (= G[:j, j]) with the corrected column; ist[0] = gate, ist[1] += trips,
// elog[j] = max |e|.  fused: d = [V_i . w (i < j), u~ . u~, ||w||^2] and chat in the units of w; post normalises both by
// b = sqrt(||w||^2), takes cs = 1, leaves ||w||^2 in nrm2[0] and the correction's coefficients for u~ (b g_i) in g[n ..].
void launch_os_post(const double* d, const double* chat, double* G, double* H, int n, int j, double* nrm2, double tau, double* g, int* ist,
                    double* elog, bool fused, hipStream_t s);
// one block: sum_out[0] = sum(part[0 .. np)) in k_final_sum's grouping - ||w_{j+1}||^2 behind the three-term kernel, or (fused) alpha_j
// behind the SpMV - and then, when `predict`, chat[0..j] of step j + 1 (fused: not divided by sqrt(nrm2)) and H[:, j]'s alpha / beta entries.
// fused with part == nullptr: the predictions alone, alpha_j read from its slot (nothing is summed, sum_out is not written)
void launch_os_sum_predict(const double* part, int np, double* sum_out, const double* G, double* H, int n, int j, const double* alpha_j,
                           const double* beta_j, double* chat, bool fused, bool predict, hipStream_t s);
// Pair form (run_loop_one_sweep_pair): one walk per two steps, j >= 2 the first step of the pair; the arithmetic is one_sweep_pair_lanczos's
// (tools/one_sweep_prototype.py).  The walk parks 4 x 2 x os_pair_ldp(j) per-wave dots in LDS: n + 1 <= kOneSweepPairMaxLdp keeps that
// within 64 KiB.  predict: alpha_out[0] = a0 = sum(part[0 .. np)) (the speculative SpMV's dot), H[:, j-1] gets step j's applied
// coefficients, kap[0..j] / p[0..j] as the prototype names them.  sweep: V[j] = v_j, y (in: y° = A w / b; out: u~_{j+1}, in place),
// part[b * 2 ldp + ..] = [V_i . w (i < j), u~ . u~ | V_i . z (i < j), v_j . z, ||u~_{j+1}||^2]; wide16: 16 positions per lane instead
// of 8 on long vectors (A/B).  post: d = the runs' sums (launch_final_rows_t over 2 ldp columns); G[:, j], G[:, j+1], H[:, j], elog[j],
// elog[j+1], nrm2[0] = ||u~_{j+1}||^2, and ist[3] = 1 when a leftover exceeds tau (sticky).
constexpr int kOneSweepPairMaxLdp = 1024;
int os_pair_ldp(int j);
int os_pair_sweep_blocks(int64_t len, bool wide16);
void launch_os_pair_predict(const double* part, int np, double* alpha_out, const double* nrm2, const double* chat, const double* G, double* H,
                            int n, int j, double* kap, double* p, hipStream_t s);
int launch_os_pair_sweep(double* V, int64_t ldv, int64_t len, int j, const double* chat, const double* kap, const double* w, double* y,
                         const double* nrm2, const double* alpha0, double* part, bool wide16, hipStream_t s);
void launch_os_pair_post(const double* d, int ldp, const double* chat, const double* kap, const double* p, double* G, double* H, int n, int j,
                         double* nrm2, const double* alpha_j, double tau, int* ist, double* elog, hipStream_t s);
// Group form (run_loop_one_sweep_quad): one walk per four steps, j >= 2 the first step of the group; the arithmetic is one_sweep_group_lanczos's
// at m = 4 (tools/one_sweep_group_prototype.py).  The walk parks 4 waves x 4 x os_quad_ldp(j) per-wave dots in LDS; the limit on the run
// length follows from the LDS a launch may ask for without a raise (os_quad_max_ldp), and longer runs belong to the pair form.
// predict: nrm2[0] = sum(part[0 .. np)) = ||z||^2 (b_3 = its root); alpha[0..2] = a_t, beta[0..2] = b_t as the chain left them;
// gout[t * ldg ..] = g_t: [0, j) the predicted dots of x_t against the basis rows, [j, j + t) against x_0 .. x_{t-1}.  sweep: rows j .. j+3
// of V (in: x_0 .. x_2 and, from z / b_3, x_3; out: v_j .. v_{j+3}), part[b * 4 ldp + t ldp + ..] = [V_i . x_t (i < j), v_{j+s} . x_t (s < t),
// v_{j+t} . v_{j+t}]; wide8: 8 positions per lane instead of 4 on long vectors (A/B).  post: d = the runs' sums (launch_final_rows_t over
// 4 ldp columns); G[:, j .. j+3], H[:, j-1 .. j+2], beta[3] = b_3, elog[j .. j+3], and ist[4] = 1 when a leftover exceeds tau (sticky).
constexpr int kOneSweepQuadLds = 65536;
inline size_t os_quad_lds_bytes(int ldp) { return (size_t)(kTPB / 64) * 4 * ldp * sizeof(double); }
inline int os_quad_max_ldp() { return (int)(kOneSweepQuadLds / os_quad_lds_bytes(1)); }
int os_quad_ldp(int j);
int os_quad_sweep_blocks(int64_t len, bool wide8);
void launch_os_quad_predict(const double* part, int np, double* nrm2, const double* chat, const double* G, const double* H, int n, int j,
                            const double* alpha, const double* beta, double* gout, int ldg, hipStream_t s);
// bz == nullptr: rows j .. j+2 hold x_0 .. x_2 and z holds z_3; else (the chain in the units of z) rows j .. j+3 hold the unscaled
// z_0 .. z_3, bz[t] = b_t (t < 3) and z is not read
int launch_os_quad_sweep(double* V, int64_t ldv, int64_t len, int j, const double* g, int ldg, const double* z, const double* bz, const double* nrm2,
                         double* part, bool wide8, hipStream_t s);
// returns the error of the per-kernel LDS-limit raise (hipFuncSetAttribute), if that was needed and failed
hipError_t launch_os_quad_post(const double* d, int ldp, const double* g, int ldg, double* G, double* H, int n, int j, const double* nrm2,
                               const double* alpha, double* beta, double tau, int* ist, double* elog, hipStream_t s);
// ---- device-resident partial re-orthogonalisation (Simon's omega-recurrence in a one-block kernel) ----
// State: st[0] = ||A|| estimate, st[1] = force_next, st[2 .. 2 + n + 2) = hb (hb[k] = the norm that formed V[k]), then three
// rows of n + 1 doubles (omega_{j,:} lives in row j % 3); ist[0] = the gate of the coming step (1: sweep), ist[1] = number of
// sweeps so far, ist[2 + j] = whether step j swept.
inline size_t omega_state_doubles(int n) { return (size_t)2 + (n + 2) + 3 * (size_t)(n + 1); }
inline size_t omega_state_ints(int n) { return (size_t)2 + n + 1; }
// Prepares the decision for step jn (called after step jn - 1 has left alpha[jn-1] and ||r||^2; jn == 0: after the warm-up).
// part != nullptr: first nrm2[0] = sum(part[0..np)) in k_final_sum's order (single rank: one launch for both).
void launch_omega(const double* part, int np, double* nrm2, const double* alpha, int jn, int n, double* st, int* ist, hipStream_t s,
                  double* c_clear = nullptr);  // c_clear: jn + 1 coefficients zeroed when step jn does not sweep (partitioned runs)
// The post-reduce kernel of the one-reduce partial loop (k_partial_onered_post, lz_reorth.hip): finishes the all-reduced buffer,
// advances the omega-recurrence, takes the look-ahead sweep decision of step j + 1, clears the next step's buffer.  j < 0: initialises
// the gates (ist: omega_onered_ints(n) ints).
inline size_t omega_onered_ints(int n) { return (size_t)4 + n + 2; }
void launch_partial_onered_post(double* buf, double* bufn, int nzero_next, int m, int ldp, double* alpha_slot, double* nrm2, const double* alpha,
                                int j, int n, double* st, int* ist, double kappa, double* beta_prev, double* uu_keep, hipStream_t s);
// r = r - beta vm (vm may be nullptr: r unchanged) + block partials of [r.r, u.r, u.u] at part[b], part[G + b], part[2 G + b]; returns G
int launch_three_term_self(double* r, const double* u, const double* vm, const double* beta, int64_t len, double* part, hipStream_t s);
void launch_fused_prepare(double* c, int j, double* beta_slot, hipStream_t s);
void launch_onereduce_prepare(double* buf, int m, int ldp, double* alpha_slot, double* bad, double* beta_prev, double* uu_keep, hipStream_t s);
void launch_onereduce_finish(const double* buf, int ldp, double* alpha_last, double* beta_last, const double* uu_keep, hipStream_t s);
// r = (r - alpha v_j) - beta v_jm1 ; part[b] = partial ||r||^2 ; returns number of partials
int launch_three_term(double* r, const double* vj, const double* vjm1, const double* alpha, const double* beta,
                      int64_t len, double* part, hipStream_t s);
// the group chain in the units of z: out = (y - alpha zt) - bt xm (mode 0, k_three_term's expression, out of place), or
// out = (y / bt - alpha (zt / bt)) - bt xm' with xm' = xm (mode 1) or xm / bm (mode 2); part[b] = partial ||out||^2; returns the partials
int launch_three_term_z(int mode, double* out, const double* y, const double* zt, const double* xm, const double* alpha, const double* bt,
                        const double* bm, int64_t len, double* part, hipStream_t s);
// one block: beta_slot[0] = sqrt(sum(zpart[0 .. nz))), alpha_slot[0] = sum(apart[0 .. na)) / sum(zpart[0 .. nz)) (k_final_sum's grouping)
void launch_final_sum_chain(const double* zpart, int nz, const double* apart, int na, double* beta_slot, double* alpha_slot, hipStream_t s);
// one block: out[0] = sum(part[0 .. np)) (k_final_sum), root_out[0] = sqrt(nrm2[0])
void launch_final_sum_root(const double* part, int np, double* out, const double* nrm2, double* root_out, hipStream_t s);
// gather x[idx[k]] -> buf[k]
void launch_gather(const double* x, const int32_t* idx, int64_t n, double* buf, hipStream_t s);

// ---- two-sided Lanczos (lz_twosided.hip) ----
// One link of the bi-orthogonalisation chain for both sides: optional (x, y) = (xs / f[0], ys / f[1] * f[2]) [first],
// optional x -= Sp[0]/Sp[1] * ap, y -= Sp[2]/Sp[3] * bp [pend], store, then dots: 0 -> S = [x.a, a.a, y.b, b.b] (epi 0);
// 1 -> x.y (epi 1: fo = {sqrt|.|, sqrt|.|, sign}); 2 -> [x.x, y.y] (epi 2: fo = {sqrt, sqrt, 1}); 3 -> none.
void launch_bi(int first, int pend, int dots, double* x, double* y, const double* xs, const double* ys, const double* f,
               const double* ap, const double* bp, const double* Sp, const double* a, const double* b, int64_t len, double* part,
               int epi, double* S, double* fo, double* o0, double* o1, unsigned* ticket, hipStream_t s, const double* pend_part = nullptr,
               bool defer_fold = false);
// r -= c0 u, s -= c1 v (sub); dots 0: o0 = (da.r + db.s)/2; 1: o0 = sqrt|r.s|, o1 = r.s/o0, fo = {o0, o1, 1}; 2: o0 = da.r
void launch_bi_two_term(int sub, int dots, double* r, double* sv, const double* u, const double* v, const double* c0, const double* c1,
                        const double* da, const double* db, int64_t len, double* part, double* fo, double* o0, double* o1,
                        unsigned* ticket, hipStream_t s);  // ticket != nullptr: the last block folds the partials (one launch)
// ---- result publication (lz_xfer.hip): large device -> host copies through a ring of pinned staging buffers + host copy threads
struct Xfer;
void xfer_free(Xfer*& x);
hipError_t xfer_d2h(int dev, hipStream_t stream, Xfer*& state, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width,
                    size_t height);  // returns with the destination complete (stream synchronised)
int xfer_threads();

void launch_bi_mem_safe(double* xrow, const double* B, int64_t ldv, int n, int j, int64_t len, double* coef, hipStream_t s);
int bi_partials_needed();  // per partial buffer; the handle keeps two (deferred folds ping-pong between them)

// Y(rows x n, row-major, ldy) = sum_k V[k][m] * S[k][i]   (FP64 MFMA)
// variant 0: the S-stationary kernel (S in registers, V tiles through LDS) for 49 <= n <= 200 when there are enough row
// tiles for a persistent grid, else one workgroup per 128 rows, one wave per SIMD owning 32 rows x all columns; 1: the
// latter always.  (The retired arms - persistent waves, S staged through LDS - live in the kernel-bench build.)
// clk (optional, 8 words): in-kernel clock record of the S-stationary kernel, see lz_ritz_info.
// Returns the error of the per-kernel LDS-limit raise (hipFuncSetAttribute) if that was needed and failed.
hipError_t launch_ritz_gemm(const double* V, int64_t ldv, int64_t rows, int n, const double* Spad, int npad, double* Y,
                            int64_t ldy, hipStream_t s, int variant = 0, unsigned long long* clk = nullptr);
void launch_ritz_gemm_cols(const double* V, int64_t ldv, int64_t rows, int kcount, const double* B, int ldb, int ncols, double* Y,
                           int64_t ldy, hipStream_t s);
// G = Y^T Y as K-chunk partials (n x n each); returns the number of chunks (<= nz_max)
int launch_gram(const double* Y, int64_t ldy, int64_t rows, int n, double* part, int nz_max, hipStream_t s);
void launch_sum_slices(const double* part, int nz, int64_t count, double* out, hipStream_t s);
// accumulator-stationary symmetric Gram kernel (n >= 33, >= 4096 rows; more than 208 columns: in groups of 11 column tiles):
// out = Y^T Y complete; false: not covered
constexpr int kGramMaxSlices = 768;
size_t gram_scratch_doubles(int n);
bool launch_gram_sym(const double* Y, int64_t ldy, int64_t rows, int n, double* part, double* out, hipStream_t s,
                     unsigned long long* clk = nullptr, int nz_override = 0,  // nz_override > 0: that many K slices (A/B knob 21)
                     int variant = 0);  // 0: operands staged through LDS (even n), 2: the register-ring kernels (knob 19 = 2)
// per-block [s1 (n), s2 (n)] partials of the Ritz-vector quality sums; returns the number of blocks
int launch_ritz_quality(const CsrDev& A, const double* Y, int64_t ldy, int n, double* part, hipStream_t s);
// x[r] = Y[r * ldy + col] for r < rows, 0 for rows <= r < rows_pad
void launch_extract_column(const double* Y, int64_t ldy, int col, int64_t rows, int64_t rows_pad, double* x, hipStream_t s);

// ---- thick-restart Lanczos (lz_trl.hip; C ABI in lz_trl_api.hip) ----
// V[0..kk) = S^T V[0..m) in place (S: m x kk row-major, m <= 128, kk < m), then V[kk] = V[m]; positions >= rows are not written
hipError_t launch_trl_restart(double* V, int64_t ldv, int64_t rows, int m, int kk, const double* S, hipStream_t s);
// r = r - sum_{i < nrows} c_i V_i and part[b] = block b's share of |r|^2; runs only when gate == nullptr or gate[0] != 0.  Returns the
// number of partials (trl_cgs_blocks(len)).
int launch_trl_cgs(const double* V, int64_t ldv, int64_t len, int nrows, const double* c, double* r, double* part, const int* gate, hipStream_t s);
int trl_cgs_blocks(int64_t len);
// one block between the passes of an extension step (mode 0: after pass 1, sets the gate of pass 2; 1: after the gated pass 2; 2: norm only)
void launch_trl_post(int mode, const double* part, int np, const double* c, int j, double* nrm2, double* proj, int* gate, int force, hipStream_t s);
// band Lanczos (lz_trl_extend_band): the block Gram-Schmidt of b (2 .. 8) work vectors W[c] (c-th at W + c * ldw) against V[0..r0).
// dots: part[g * run + i * b + c] = block g's share of V_i . W_c (run = trl_band_run(r0, b), g < trl_band_dots_blocks(len, b));
// launch_final_rows_t(part, blocks, run, r0 * b, C) then gives C[i * b + c].  len: a multiple of 32.
inline int trl_band_run(int r0, int b) { return (r0 * b + 15) & ~15; }
int trl_band_dots_blocks(int64_t len, int b);
hipError_t launch_trl_band_dots(const double* V, int64_t ldv, int64_t len, int r0, const double* W, int64_t ldw, int b, double* part, hipStream_t s);
// update: W_c -= sum_{i < r0} C[i * b + c] V_i for every c from one walk over the rows, part[c * G + g] = block g's share of |W_c|^2;
// returns G (= trl_band_update_blocks(len))
int trl_band_update_blocks(int64_t len);
int launch_trl_band_update(const double* V, int64_t ldv, int64_t len, int r0, const double* C, double* W, int64_t ldw, int b, double* part,
                           hipStream_t s);
// proj[c * ldf + i] = C1[i * b + c] + C2[i * b + c] (i < r0, c < nb): the two passes' coefficients summed into nb rows of the projected matrix
void launch_trl_band_proj(const double* C1, const double* C2, int r0, int b, int nb, double* proj, int ldf, hipStream_t s);
// squares of A y_i - theta_i y_i, block partials at part[i * G + b]; return G
int launch_trl_resid_csr(const CsrDev& A, const double* Y, int64_t ldy, int k, const double* theta, double* part, hipStream_t s);
int launch_trl_resid_diff(const double* y, const double* x, int64_t rows, const double* theta, int i, double* part, hipStream_t s);
// the same for complex eigenvalues re + i im of a real matrix, eigenvectors in real form (im[i] == 0: row i; im[i] > 0: rows i, i + 1
// are the real and imaginary part, (re, im)[i + 1] the conjugate - the caller checks that): squares of |A x - lambda x|, the pair's at
// part[i * G + b] and zeros at part[(i + 1) * G + b]; return G.  diff: one pair of a dense matrix, yr = A x_r, yi = A x_i.
int launch_trl_resid_cplx_csr(const CsrDev& A, const double* Y, int64_t ldy, int k, const double* re, const double* im, double* part,
                              hipStream_t s);
int launch_trl_resid_cplx_diff(const double* yr, const double* yi, const double* xr, const double* xi, int64_t rows, const double* re,
                               const double* im, int i, double* part, hipStream_t s);
void launch_trl_rownorm(const double* part, int G, int k, double* out, hipStream_t s);
// one step of the scaled Chebyshev recurrence, in place on wz (which holds w = A y): wz[r] = a (w[r] - c y[r]) - b x[r] for r < rows and
// 0 for rows <= r < len; a = coef[i], b = coef[degree + i] are read on the device.  x may alias y (degree 1: b = 0).
void launch_cheb_step(double* wz, const double* y, const double* x, const double* coef, int i, int degree, double c, int64_t rows,
                      int64_t len, hipStream_t s);
// one step of the Chebyshev series, wz holding w = A y: term i (1 .. degree) of the recurrence and acc + mu[i] term (series_combine).
// last == 0: wz = the term, acc_out = the sum; last != 0: wz = the sum, the term is dropped.  i == 1 reads neither x nor acc_in.
// Rows rows <= r < len are written as zero.  acc_out may be acc_in.
void launch_cheb_series_step(double* wz, const double* y, const double* x, const double* acc_in, double* acc_out, const double* mu, int i,
                             int last, double inv_e, double c, int64_t rows, int64_t len, hipStream_t s);

// ---- complex Hermitian operator (lz_zspmv.hip) and its Gram-Schmidt kernels (lz_ztrl.hip); C ABI in lz_ztrl_api.hip ----
// Vectors are planar: the real part at p, the imaginary part at p + ld.  Matrix values are interleaved complex128 (16 bytes an entry).
// y = A x, CSR: a group of `group` lanes (a power of two <= 64) owns a row and walks it in strides of the group; empty rows give 0
void launch_zspmv_csr(const int32_t* rowptr, const int32_t* colidx, const double* vals, int64_t rows, int group, const double* xr,
                      const double* xi, double* yr, double* yi, hipStream_t s);
// y = A x, dense row-major n x n: one wave per row, A read once
void launch_zgemv(const double* A, int64_t n, const double* xr, const double* xi, double* yr, double* yi, hipStream_t s);
constexpr int kZMaxRows = 65;  // complex rows of a basis (m + 1, m <= 64): the restart's real form holds 2 m x 2 kk doubles in LDS
// part[(2 i + 0 / 1) * G + b] = block b's share of Re / Im <V_i, w> = sum conj(V_i) w for i < nb, and of w^H w / 0 at i = nb (the self
// slot); launch_final_rows(part, 2 (nb + 1), G, c) then gives c interleaved.  V: complex row i = real rows 2 i, 2 i + 1 (ldv apart);
// w: real part, imaginary part at w + ldv.  len: the padded length.  Returns G = zdots_blocks(len).  gate as launch_trl_cgs.
int zdots_blocks(int64_t len);
int launch_zdots(const double* V, int64_t ldv, int64_t len, int nb, const double* w, double* part, const int* gate, hipStream_t s);
// w -= sum_{i < nb} c_i V_i (c interleaved complex), part[b] = block b's share of |w|^2; returns the number of partials (zcgs_blocks(len))
int zcgs_blocks(int64_t len);
int launch_zcgs(const double* V, int64_t ldv, int64_t len, int nb, const double* c, double* w, double* part, const int* gate, hipStream_t s);
// squares of |y - theta[i] x| over n complex entries (planar, parts ld apart), block partials at part[i * G + b]; returns G
int launch_zresid_diff(const double* y, const double* x, int64_t ld, int64_t n, const double* theta, int i, double* part, hipStream_t s);

// ---- small-problem engine (lz_small.hip): the whole run as one cooperative kernel
struct SmallArgs {
  int kind;  // 1 CSR, 2 dense
  const int32_t* rowptr;
  const int32_t* colidx;
  const double* vals;
  const int32_t* rowblk;  // CSR-stream row blocks (nparts + 1); nullptr: fixed blocks of 512 rows (fixed-K kernel)
  int nparts;             // alpha partials of the multi-kernel path: row blocks (CSR) or ceil(rows / 4) (dense)
  const double* dense;
  int64_t lda;
  int rows, rows_pad, n;
  int64_t ldv;
  double* V;
  const double* x0;  // scratch copy of the start vector (rows_pad doubles)
  double* y;     // SpMV output (the handle's r vector)
  double* drow;  // rows: V[j]_i * (A V[j])_i
  double* pc;    // n + 1: raw re-orthogonalisation sums [V_i . r (i < j), r . r]
  double* alpha;
  double* beta;
  unsigned* bar;  // 4 zeroed words: [0] device-scope barrier, [1] XCD-local barrier, [2] status (0 ok, 2 placement, 3 barrier timeout)
  unsigned* xcc;  // one word per participating block: the XCD it found itself on (+ 1)
  unsigned long long zero;  // 0 (a run-time value: the addend of the L2-atomic "loads", see ld_sh)
};

constexpr int kSmallMaxPadRows = 1280;
int small_grid(int rows_pad);
hipError_t launch_small_run(const SmallArgs& a, int nb, bool local, hipStream_t s);
hipError_t launch_small_step(const SmallArgs& a, int mode, int j, int nb, hipStream_t s);

}  // namespace lz
