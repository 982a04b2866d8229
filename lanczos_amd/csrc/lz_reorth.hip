// Hand-written gfx950 vector kernels of the Lanczos hot path: full re-orthogonalisation (Q^T w, update),
// three-term recurrence, second-stage reductions, halo pack.
//
// All kernels here are HBM-bandwidth bound (<= 0.25 flop/byte), so the design
// rules are: 16-byte coalesced accesses, many independent loads in flight per
// lane, non-temporal loads for data that is streamed once, deterministic
// two-stage reductions (wave shuffle -> LDS -> per-block partial -> tiny
// second-stage kernel), and no atomics.
//
// Arithmetic contract (DESIGN.md "numerics"): element-wise results follow the
// reference CPU branch's NumPy expression order with NO fused multiply-add
// (compiled with -ffp-contract=off), so SpMV row sums, the re-orthogonalisation
// update and the three-term recurrence are bit-identical to NumPy/SciPy given
// the same scalar inputs; only the inner products differ (summation order).
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "lz_device.h"

namespace lz {

// ------------------------------------------------------------------ second-stage reductions
constexpr int kFinalThreads = 1024;
// sum(part[0..n)) by one block of 1024 threads: four strided accumulators per thread (a full group of four while
// i + 3 * 1024 < n, the remainder into the first), wave shuffle tree, 16 wave sums added in order.  The grouping is part of
// the contract (final_sum_emulated in lz_device.h replays it).  The result is valid in thread 0.
// (Round 4 tried issuing all of a thread's loads - up to 24 - before its first add, on the theory that the ~4.7 us this
// one-block kernel takes are eight dependent round trips to the memory side: measured 4.85 us instead of 4.69, k_omega 6.0
// instead of 5.0 (profiles/r04/partial_loop_kernel_stats*.csv) - a one-block kernel this short pays for its instruction
// fetch, not for its loads; the plain loop is the smaller code and stays.)
__device__ __forceinline__ double final_sum_1024(const double* __restrict__ part, int n, double* sm) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int i = threadIdx.x;
  for (; i + 3 * kFinalThreads < n; i += 4 * kFinalThreads) {
    a0 += part[i];
    a1 += part[i + kFinalThreads];
    a2 += part[i + 2 * kFinalThreads];
    a3 += part[i + 3 * kFinalThreads];
  }
  for (; i < n; i += kFinalThreads) a0 += part[i];
  const double acc = wave_sum((a0 + a1) + (a2 + a3));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) sm[w] = acc;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kFinalThreads / 64; ++k) t += sm[k];
  }
  return t;
}

__global__ __launch_bounds__(kFinalThreads) void k_final_sum(const double* __restrict__ part, int n, double* __restrict__ out) {
  __shared__ double sm[kFinalThreads / 64];
  const double t = final_sum_1024(part, n, sm);
  if (threadIdx.x == 0) out[0] = t;
}

// ------------------------------------------------------------------ partial re-orthogonalisation: the decision, on the device
// Simon's omega-recurrence (H. D. Simon 1984): omega_{j,k} estimates v_j . v_k from alpha and beta alone; a sweep is due when
// max_k |omega_{j,k}| exceeds sqrt(eps), on that vector and the next.  One block; called once per step, AFTER the three-term
// kernel of step jn - 1 (optionally folding that kernel's ||r||^2 partials first, with k_final_sum's exact grouping), it leaves
// the gate of step jn in ist[0].  The sweep kernels and the SpMV of step jn read the gate: lz_run never waits for the device.
// Arithmetic: expression for expression the host loop this replaces (run_loop_six, lz_loops.hip; both compiled with
// -ffp-contract=off, IEEE sqrt and division), every k is independent and the maximum does not depend on the order, so the
// decisions - and with them every coefficient - are bit-identical to the host-decided run (tests/test_gpu_lanczos.py).
// State layout: see omega_state_doubles (lz_internal.h).
// c_clear (row-block partition): the coefficient buffer the host all-reduces EVERY step (it cannot skip a collective the device may
// need) is zeroed when the coming step does not sweep - stale coefficients would otherwise be summed over the ranks again and again
// (x world per step: inf after a few hundred steps; never read, but a trap for any later consumer - ADVICE r4).
__global__ __launch_bounds__(kFinalThreads) void k_omega(const double* __restrict__ part, int np, double* __restrict__ nrm2,
                                                        const double* __restrict__ alpha, int jn, int n, double* __restrict__ st,
                                                        int* __restrict__ ist, double* __restrict__ c_clear) {
  __shared__ double sm[kFinalThreads / 64];
  __shared__ double s_nrm2;
  __shared__ int s_sweep;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (part) {  // k_final_sum's own code
    const double t = final_sum_1024(part, np, sm);
    if (threadIdx.x == 0) {
      nrm2[0] = t;
      s_nrm2 = t;
    }
  } else if (threadIdx.x == 0) {
    s_nrm2 = nrm2[0];
  }
  __syncthreads();
  const double eps = 2.220446049250313e-16, thresh = 1.4901161193847656e-08;
  double* hb = st + 2;
  double* W = hb + (n + 2);
  const int ldw = n + 1;
  const double hbj = sqrt(s_nrm2);
  if (jn == 0) {  // after the warm-up: clear the state; step 0 always sweeps (a one-row sweep)
    for (int i = threadIdx.x; i < 3 * ldw; i += kFinalThreads) W[i] = i == 0 ? 1.0 : 0.0;  // omega_{0,0} = v_0 . v_0
    for (int i = threadIdx.x; i < n + 2; i += kFinalThreads) hb[i] = i == 0 ? hbj : 0.0;
    if (threadIdx.x == 0) {
      st[0] = 0.0;
      st[1] = 0.0;
      ist[0] = 1;
      ist[1] = 1;
      ist[2] = 1;
    }
    return;
  }
  // beta_j omega_{j,k} = beta_{k+1} omega_{j-1,k+1} + (alpha_k - alpha_{j-1}) omega_{j-1,k} + beta_k omega_{j-1,k-1}
  //                      - beta_{j-1} omega_{j-2,k}  (+ rounding of size eps ||A||),   k <= j-2
  const double a_last = alpha[jn - 1];
  const double hb_prev = hb[jn - 1];
  double normA = st[0];
  {
    const double cand = fabs(a_last) + hb_prev + hbj;
    if (cand > normA) normA = cand;
  }
  const double* cur = W + (size_t)((jn + 2) % 3) * ldw;   // omega_{jn-1,:}
  const double* prev = W + (size_t)((jn + 1) % 3) * ldw;  // omega_{jn-2,:}
  double* nw = W + (size_t)(jn % 3) * ldw;
  double worst = 0.0;
  for (int k = threadIdx.x; k <= n; k += kFinalThreads) {
    double v = 0.0;
    if (k == jn) {
      v = 1.0;
    } else if (k == jn - 1) {
      v = eps;
    } else if (k + 2 <= jn) {
      double t = hb[k + 1] * cur[k + 1] + (alpha[k] - a_last) * cur[k] - hb_prev * prev[k];
      if (k > 0) t += hb[k] * cur[k - 1];
      t += (t < 0 ? -1.0 : 1.0) * 2.0 * eps * normA;
      v = t / hbj;
      const double av = fabs(v);
      if (av > worst) worst = av;
    }
    nw[k] = v;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_down(worst, off, 64);
    if (o > worst) worst = o;
  }
  __syncthreads();  // (sm is reused)
  if (lane == 0) sm[w] = worst;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = 0.0;
#pragma unroll
    for (int k = 0; k < kFinalThreads / 64; ++k)
      if (sm[k] > m) m = sm[k];
    const bool due = m > thresh;
    const int sweep = (due || st[1] != 0.0) ? 1 : 0;  // a due sweep also covers the next vector (both feed the recurrence)
    st[1] = due ? 1.0 : 0.0;
    st[0] = normA;
    hb[jn] = hbj;
    ist[0] = sweep;
    ist[1] += sweep;
    ist[2 + jn] = sweep;
    s_sweep = sweep;
  }
  __syncthreads();
  if (s_sweep)
    for (int k = threadIdx.x; k < jn; k += kFinalThreads) nw[k] = eps;
  else if (c_clear)
    for (int k = threadIdx.x; k <= jn; k += kFinalThreads) c_clear[k] = 0.0;
}
void launch_omega(const double* part, int np, double* nrm2, const double* alpha, int jn, int n, double* st, int* ist, hipStream_t s, double* c_clear) {
  hipLaunchKernelGGL(k_omega, dim3(1), dim3(kFinalThreads), 0, s, part, np, nrm2, alpha, jn, n, st, ist, c_clear);
}

// ---- the same decision for the loop with ONE all-reduce per step (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE) --------------
// On a row-block partition the sums a step needs - alpha of the newest vector u = v_{j-1}, the three self terms that give
// ||r||^2, and (when a sweep runs) the basis dots against r'' and u - travel in ONE buffer and one all-reduce (run_loop_partial_
// onereduce, lz_loops.hip).  The sweep's dots must be in that buffer BEFORE alpha_{j-1} and beta_j - the inputs of omega_{j,:} -
// exist on any rank, so the gate of step j cannot be Simon's exact test of omega_{j,:}; it is a ONE-STEP LOOK-AHEAD, taken by this
// kernel right after the all-reduce of step j - 1:
//   * omega_{j,:} is advanced exactly (k_omega's recurrence, expression for expression) once alpha_{j-1}, beta_j are known;
//   * omega_{j+1,:} is PREDICTED with the same recurrence, the two coefficients that do not exist yet replaced by the newest
//     ones (alpha_j ~ alpha_{j-1}, beta_{j+1} ~ beta_j); a sweep of v_{j+1} (and of v_{j+2}: Simon's pair) is due when
//     kappa * max_k |pred| > sqrt(eps) (kappa = 4 by default: a sweep comes a step early rather than late - an early sweep costs
//     nothing but its place in the schedule);
//   * the exact row is the check on the prediction: a vector that was not swept although its exact omega exceeds sqrt(eps) is a
//     MISS - counted (lz_last_sweep_misses), and the next two vectors are swept.
// Every input is an all-reduced sum or derived from one: every rank takes the same decisions.  One block; it also finishes the
// all-reduced buffer like k_onereduce_prepare (alpha, c_i = p_i - alpha q_i, ||r||^2 by the three-sum form + its cancellation
// guard) and clears the buffer of the next step (coefficient slots of a step without a sweep must be zero, not stale: they are
// summed over the ranks every step).
// State: st / W as k_omega; ist[0], ist[1] = gate of the even / odd steps, ist[2] = sweeps, ist[3] = misses, ist[4 + j] = log.
__global__ __launch_bounds__(kFinalThreads) void k_partial_onered_post(double* __restrict__ buf, double* __restrict__ bufn, int nzero_next, int m,
                                                                       int ldp, double* __restrict__ alpha_slot, double* __restrict__ nrm2,
                                                                       const double* __restrict__ alpha, int j, int n, double* __restrict__ st,
                                                                       int* __restrict__ ist, double kappa, double* __restrict__ beta_prev,
                                                                       double* __restrict__ uu_keep) {
  __shared__ double sm[kFinalThreads / 64];
  __shared__ double s_v;
  __shared__ int s_flag;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (j < 0) {  // before the warm-up: step 0 always sweeps (the reference's one-row sweep)
    for (int i = threadIdx.x; i < n + 5; i += kFinalThreads) ist[i] = (i == 0 || i == 2 || i == 4) ? 1 : 0;
    return;
  }
  const int g = ist[j & 1];
  // alpha relative to u.u, and the beta of the step before put on u's measured length: as k_onereduce_prepare, and for its reason.
  // (The recurrence below keeps the norms as they were when they formed their vectors: hb is not touched.)
  const double uu = buf[ldp + m];
  const double a = buf[ldp + m + 2] / uu;
  if (bufn)
    for (int i = threadIdx.x; i < nzero_next; i += kFinalThreads) bufn[i] = 0.0;
  if (g)
    for (int i = threadIdx.x; i < m; i += kFinalThreads) buf[i] = buf[i] - a * buf[ldp + i];
  if (threadIdx.x == 0) {
    const double rr = buf[m], ur = buf[ldp + m + 1];
    const double v = (rr - 2.0 * a * ur) + a * a * uu;
    if (!(v > 1e-4 * rr)) nrm2[1] = 1.0;  // cancellation guard, as k_onereduce_prepare
    buf[m] = v;
    nrm2[0] = v;
    alpha_slot[0] = a;
    if (beta_prev) beta_prev[0] = beta_prev[0] * sqrt(uu / uu_keep[0]);
    uu_keep[0] = uu;
    s_v = v;
  }
  __syncthreads();
  const double eps = 2.220446049250313e-16, thresh = 1.4901161193847656e-08;
  double* hb = st + 2;
  double* W = hb + (n + 2);
  const int ldw = n + 1;
  const double hbj = sqrt(s_v);
  if (j == 0) {
    for (int i = threadIdx.x; i < 3 * ldw; i += kFinalThreads) W[i] = i == 0 ? 1.0 : 0.0;  // omega_{0,0} = v_0 . v_0
    for (int i = threadIdx.x; i < n + 2; i += kFinalThreads) hb[i] = i == 0 ? hbj : 0.0;
    if (threadIdx.x == 0) {
      st[0] = 0.0;
      st[1] = 0.0;
      ist[1] = 0;  // step 1: nothing to be orthogonal to but v_0, which the recurrence itself takes care of
      if (n > 1) ist[4 + 1] = 0;
    }
    return;
  }
  // exact row j (k_omega's code): alpha_{j-1} = a, beta_j = hbj
  const double hb_prev = hb[j - 1];
  double normA = st[0];
  {
    const double cand = fabs(a) + hb_prev + hbj;
    if (cand > normA) normA = cand;
  }
  const double* cur = W + (size_t)((j + 2) % 3) * ldw;   // omega_{j-1,:}
  const double* prev = W + (size_t)((j + 1) % 3) * ldw;  // omega_{j-2,:}
  double* nw = W + (size_t)(j % 3) * ldw;
  double worst = 0.0;
  for (int k = threadIdx.x; k <= n; k += kFinalThreads) {
    double v = 0.0;
    if (k == j) {
      v = 1.0;
    } else if (k == j - 1) {
      v = eps;
    } else if (k + 2 <= j) {
      const double ak = k == j - 1 ? a : alpha[k];
      double t = hb[k + 1] * cur[k + 1] + (ak - a) * cur[k] - hb_prev * prev[k];
      if (k > 0) t += hb[k] * cur[k - 1];
      t += (t < 0 ? -1.0 : 1.0) * 2.0 * eps * normA;
      v = t / hbj;
      const double av = fabs(v);
      if (av > worst) worst = av;
    }
    if (g && k < j) v = eps;  // this vector is being swept
    nw[k] = v;
  }
  auto block_max = [&](double x) -> double {  // valid in thread 0
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_down(x, off, 64);
      if (o > x) x = o;
    }
    __syncthreads();
    if (lane == 0) sm[w] = x;
    __syncthreads();
    double mx = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < kFinalThreads / 64; ++k)
        if (sm[k] > mx) mx = sm[k];
    }
    return mx;
  };
  const double worst_exact = block_max(worst);
  if (threadIdx.x == 0) s_flag = (!g && worst_exact > thresh) ? 1 : 0;
  __syncthreads();  // (also: row j complete before the prediction reads it)
  const int miss = s_flag;
  // predicted row j + 1: k <= j - 1; unknown alpha_j ~ a, beta_{j+1} ~ hbj; beta_j = hbj exact; hb[j] is not stored yet
  double worst_p = 0.0;
  if (j + 1 < n) {
    for (int k = threadIdx.x; k + 2 <= j + 1; k += kFinalThreads) {
      const double ak = k == j - 1 ? a : alpha[k];
      const double hk1 = k + 1 == j ? hbj : hb[k + 1];
      double t = hk1 * nw[k + 1] + (ak - a) * nw[k] - hbj * cur[k];
      if (k > 0) t += hb[k] * nw[k - 1];
      t += (t < 0 ? -1.0 : 1.0) * 2.0 * eps * normA;
      const double av = fabs(t / hbj);
      if (av > worst_p) worst_p = av;
    }
  }
  const double wp = block_max(worst_p);
  if (threadIdx.x == 0) {
    const bool due = kappa * wp > thresh || miss;
    const int gn = (due || st[1] != 0.0) ? 1 : 0;
    st[1] = (due && !g) ? 1.0 : 0.0;  // Simon's pair: the vector after a newly due one is swept too
    st[0] = normA;
    hb[j] = hbj;
    ist[3] += miss;
    if (j + 1 < n) {
      ist[(j + 1) & 1] = gn;
      ist[2] += gn;
      ist[4 + j + 1] = gn;
    }
  }
}
void launch_partial_onered_post(double* buf, double* bufn, int nzero_next, int m, int ldp, double* alpha_slot, double* nrm2, const double* alpha,
                                int j, int n, double* st, int* ist, double kappa, double* beta_prev, double* uu_keep, hipStream_t s) {
  hipLaunchKernelGGL(k_partial_onered_post, dim3(1), dim3(kFinalThreads), 0, s, buf, bufn, nzero_next, m, ldp, alpha_slot, nrm2, alpha, j, n, st, ist,
                     kappa, beta_prev, uu_keep);
}

// up to four independent k_final_sum's in one launch (block q adds its own run into its own slot)
__global__ __launch_bounds__(kFinalThreads) void k_final_sum_multi(FinalMulti fm) {
  __shared__ double sm[kFinalThreads / 64];
  const double t = final_sum_1024(fm.part[blockIdx.x], fm.n[blockIdx.x], sm);
  if (threadIdx.x == 0) fm.out[blockIdx.x][0] = t;
}
void launch_final_sum_multi(const FinalMulti& fm, int count, hipStream_t s) {
  hipLaunchKernelGGL(k_final_sum_multi, dim3(count), dim3(kFinalThreads), 0, s, fm);
}

__global__ __launch_bounds__(kTPB) void k_final_rows(const double* __restrict__ part, int G, double* __restrict__ c) {
  __shared__ double sm[kTPB / 64];
  const double* p = part + (int64_t)blockIdx.x * G;
  double acc = 0.0;
  for (int i = threadIdx.x; i < G; i += kTPB) acc += p[i];
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) c[blockIdx.x] = acc;
}

// Transposed partial layout of the 4x4x4 MFMA kernel: part[pid * ldp + row].  One block owns 8 rows (one 64-byte
// sector of every pid's run): 128 pid lanes x 8 row lanes, fixed summation order.
__global__ __launch_bounds__(kFinalThreads) void k_final_rows_t(const double* __restrict__ part, int P, int ldp, int nrows,
                                                              double* __restrict__ c, const int* __restrict__ gate) {
  if (gate && gate[0] == 0) return;  // device-resident partial re-orthogonalisation: no sweep on this vector
  __shared__ double sm[kFinalThreads / 8][8];
  const int rl = threadIdx.x & 7, pl = threadIdx.x >> 3;
  const int row = blockIdx.x * 8 + rl;  // < ldp (a multiple of 8); rows >= nrows hold stale values and are never stored
  const double* p = part + row;
  constexpr int S = kFinalThreads / 8;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int pid = pl;
  for (; pid + 3 * S < P; pid += 4 * S) {
    a0 += p[(int64_t)pid * ldp];
    a1 += p[(int64_t)(pid + S) * ldp];
    a2 += p[(int64_t)(pid + 2 * S) * ldp];
    a3 += p[(int64_t)(pid + 3 * S) * ldp];
  }
  for (; pid < P; pid += S) a0 += p[(int64_t)pid * ldp];
  sm[pl][rl] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (threadIdx.x < 8 && row < nrows) {
    double t = 0.0;
    for (int k = 0; k < S; ++k) t += sm[k][threadIdx.x];
    c[row] = t;
  }
}

void launch_final_sum(const double* part, int n, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_final_sum, dim3(1), dim3(kFinalThreads), 0, s, part, n, out);
}
// explicit run length: c[i] = sum_b part[b * ldp + i], i < nout (one-reduce mode: two coefficient runs per block)
void launch_final_rows_t(const double* part, int G, int ldp, int nout, double* c, hipStream_t s, const int* gate) {
  if (nout <= 0) return;
  hipLaunchKernelGGL(k_final_rows_t, dim3((nout + 7) / 8), dim3(kFinalThreads), 0, s, part, G, ldp, nout, c, gate);
}
void launch_final_rows(const double* part, int nrows, int G, double* c, hipStream_t s, bool transposed, const int* gate) {
  if (nrows <= 0) return;
  if (transposed)
    hipLaunchKernelGGL(k_final_rows_t, dim3((nrows + 7) / 8), dim3(kFinalThreads), 0, s, part, G, qtw_ldp(nrows), nrows, c, gate);
  else
    hipLaunchKernelGGL(k_final_rows, dim3(nrows), dim3(kTPB), 0, s, part, G, c);
}

// ------------------------------------------------------------------ re-orthogonalisation pass 1: c = Q^T w
// Block b owns the contiguous slice [b*L, b*L+cnt) of every basis row.  The
// slice of w (= V[j], optionally formed here as r / beta and stored) is kept in
// LDS for the whole launch; the block then streams the same slice of rows
// 0..nrows-1.
//
//  * VALU variant: R rows at a time, each lane accumulating R partial dots over
//    U*R independent 16-byte loads, one shuffle + LDS reduction per R rows.
//  * MFMA variant: each wave owns a quarter of the slice and walks 16-row tiles
//    with v_mfma_f64_16x16x4_f64: A = 16 basis rows x 4 consecutive elements,
//    B = the matching 4 entries of w broadcast over the 16 columns.  The
//    contraction over the long dimension happens inside the matrix core, so the
//    main loop has no cross-lane reduction and no barrier at all; 15/16 of the
//    MFMA columns are redundant, which is affordable because the step is HBM
//    bound (the matrix pipe is ~30 % busy at full HBM rate).
constexpr int kQtwMaxL = 5120;  // 40 KiB of LDS -> 4 blocks per CU

// SCALE: 0 = w is V[j] as stored; 1 = w = r / sqrt(nrm2), stored to V[j] (beta to beta_slot);
//        2 = w = r as is, nothing stored (fused-norm mode: the caller divides by beta afterwards).
template <int SCALE>
__device__ __forceinline__ double qtw_stage_w(double* __restrict__ V, int64_t ldv, int j, const double* __restrict__ r,
                                              const double* __restrict__ nrm2, double* __restrict__ beta_slot, int64_t base,
                                              int cnt2, double2* sw) {
  double2* vj = reinterpret_cast<double2*>(V + (int64_t)j * ldv + base);
  double self = 0.0;
  if (SCALE == 1) {
    const double beta = sqrt(nrm2[0]);
    if (blockIdx.x == 0 && threadIdx.x == 0) beta_slot[0] = beta;
    const double2* rr = reinterpret_cast<const double2*>(r + base);
    for (int t = threadIdx.x; t < cnt2; t += kTPB) {
      double2 v = rr[t];
      v.x = v.x / beta;
      v.y = v.y / beta;
      st_stream<1>(vj + t, v);  // next read of V[j] is a whole pass away: keep it out of L2
      sw[t] = v;
      self = fma(v.x, v.x, self);
      self = fma(v.y, v.y, self);
    }
  } else {
    const double2* src = SCALE == 2 ? reinterpret_cast<const double2*>(r + base) : vj;
    // five positions per trip (a full 5120-slice is two trips): all loads of a trip are issued before the first use -
    // at launch every resident block stages at once and nothing else hides the latency
    for (int t0 = threadIdx.x; t0 < cnt2; t0 += 5 * kTPB) {
      double2 v[5];
#pragma unroll
      for (int u = 0; u < 5; ++u) v[u] = (t0 + u * kTPB < cnt2) ? src[t0 + u * kTPB] : make_double2(0.0, 0.0);
#pragma unroll
      for (int u = 0; u < 5; ++u)
        if (t0 + u * kTPB < cnt2) {
          sw[t0 + u * kTPB] = v[u];
          self = fma(v[u].x, v[u].x, self);
          self = fma(v[u].y, v[u].y, self);
        }
    }
  }
  return self;
}

// One-reduce mode (SCALE == 3): two columns are staged - the two-term residual r'' = A u - beta v_{j-2} (sw) and the newest
// basis vector u = v_{j-1} (su) - and their three mutual dots come back: self[0] = r''.r'', self[1] = u.r'', self[2] = u.u.
__device__ __forceinline__ void qtw_stage_two(const double* __restrict__ r, const double* __restrict__ u, int64_t base, int cnt2,
                                              double2* sw, double2* su, double (&self)[3]) {
  const double2* rr = reinterpret_cast<const double2*>(r + base);
  const double2* uu = reinterpret_cast<const double2*>(u + base);
  self[0] = self[1] = self[2] = 0.0;
  for (int t0 = threadIdx.x; t0 < cnt2; t0 += 4 * kTPB) {
    double2 a[4], b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool ok = t0 + q * kTPB < cnt2;
      a[q] = ok ? rr[t0 + q * kTPB] : make_double2(0.0, 0.0);
      b[q] = ok ? uu[t0 + q * kTPB] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (t0 + q * kTPB < cnt2) {
        sw[t0 + q * kTPB] = a[q];
        su[t0 + q * kTPB] = b[q];
        self[0] = fma(a[q].x, a[q].x, self[0]);
        self[0] = fma(a[q].y, a[q].y, self[0]);
        self[1] = fma(a[q].x, b[q].x, self[1]);
        self[1] = fma(a[q].y, b[q].y, self[1]);
        self[2] = fma(b[q].x, b[q].x, self[2]);
        self[2] = fma(b[q].y, b[q].y, self[2]);
      }
  }
}

template <int SCALE, int R, int U, int NT = 1>
__global__ __launch_bounds__(kTPB) void k_qtw_valu(double* __restrict__ V, int64_t ldv, int64_t len, int nrows, int j,
                                                  const double* __restrict__ r, const double* __restrict__ nrm2,
                                                  double* __restrict__ beta_slot, int64_t L, int G,
                                                  double* __restrict__ part) {
  extern __shared__ double2 sw[];
  __shared__ double red[R][kTPB / 64];
  const int64_t base = (int64_t)blockIdx.x * L;
  const int cnt2 = (int)((len - base < L ? len - base : L) >> 1);  // double2 count of this slice
  const double self = qtw_stage_w<SCALE>(V, ldv, j, r, nrm2, beta_slot, base, cnt2, sw);
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // Tiles are walked from the newest rows down to row 0: pass 2 (k_update) must add rows in ascending
  // order, so the last ~256 MB this pass reads (rows 0, 1, ...) are the first pass 2 needs - they are still in
  // the Infinity Cache.
  const int i_top = ((nrows - 1) / R) * R;
  for (int i0 = i_top; i0 >= 0; i0 -= R) {
    const double2* row[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      int i = i0 + q;
      if (i >= nrows) i = nrows - 1;                    // clamped duplicate, result discarded
      if (i == j) i = i > 0 ? i - 1 : (nrows > 1 ? 1 : 0);  // self term comes from LDS: do not stream row j
      row[q] = reinterpret_cast<const double2*>(V + (int64_t)i * ldv + base);
    }
    double acc[R];
#pragma unroll
    for (int q = 0; q < R; ++q) acc[q] = 0.0;
#pragma unroll U
    for (int t = threadIdx.x; t < cnt2; t += kTPB) {
      const double2 wv = sw[t];
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const double2 v = ld_stream<NT>(row[q] + t);
        acc[q] = fma(v.x, wv.x, acc[q]);
        acc[q] = fma(v.y, wv.y, acc[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
      if (i0 + q == j) acc[q] = self;  // c_j = w.w from the LDS-resident values
      const double s = wave_sum(acc[q]);
      if (lane == 0) red[q][w] = s;
    }
    __syncthreads();
    if (threadIdx.x < R && i0 + threadIdx.x < nrows) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < kTPB / 64; ++k) s += red[threadIdx.x][k];
      part[(int64_t)(i0 + threadIdx.x) * G + blockIdx.x] = s;
    }
    __syncthreads();
  }
}

#ifdef LZ_KBENCH  // retired A/B arm (LZ_FLAG_QTW_MFMA, the 16x16x4 tiling: 20 % slower): its kernel lives in a kernel-bench-only file
#include "lz_reorth_kbench.h"
#endif

// MFMA variant 2: v_mfma_f64_4x4x4_4b_f64 (four independent 4x4x4 blocks per instruction).  Lane layout measured on
// gfx950 (tools/probes/mfma_f64_4x4x4_layout.hip): A[blk][i][k] lives in lane 16k + 4blk + i, B[blk][k][j] in lane
// 16k + 4blk + j, D[blk][i][j] in lane 16i + 4blk + j.  Here the 4 blocks are four adjacent 64-byte chunks of the SAME
// four basis rows, so one wave-load covers 4 rows x 256 contiguous bytes (whole 128-byte lines, like the VALU kernel)
// instead of the 16 rows x 64 bytes the 16x16x4 shape forces.  B = the matching w entries broadcast over j; the four
// block results of a row are added with two cross-lane steps once per tile.  No barrier in the main loop.
template <int SCALE, int U, int T>
__global__ __launch_bounds__(kTPB) void k_qtw_mfma4(double* __restrict__ V, int64_t ldv, int64_t len, int nrows, int j,
                                                   const double* __restrict__ r, const double* __restrict__ nrm2,
                                                   double* __restrict__ beta_slot, int64_t L, int ldp,
                                                   double* __restrict__ part, QtwFuse fz) {
  if (fz.gate && fz.gate[0] == 0) return;  // device-resident partial re-orthogonalisation: no sweep on this vector
  extern __shared__ double2 sw[];
  // Per-wave coefficients are parked in LDS (after the slice of w) and written when the wave is done, as one contiguous
  // run part[pid][0..nrows): 8-byte partial stores trickling into the read stream cost 6 % of the pass
  // (profiles/r01/ab_qtw_tile_epilogue.json: 1258 -> 1186 us without them), full lines at the end of a block's life do not.
  // SCALE == 3 (one-reduce mode): two LDS slices - r'' (argument `r`) and u = basis row `j` - and coefficient runs twice
  // as long: [0, ldp) the dots with r'', [ldp, 2 ldp) the dots with u.  Rows [0, nrows) are ALL streamed (u's own row
  // included, nothing is skipped); nrows may be 0 (first step: only the three self terms come back).
  constexpr int NCOL = SCALE == 3 ? 2 : 1;
  double* keep = reinterpret_cast<double*>(sw) + NCOL * L + (threadIdx.x >> 6) * (NCOL * ldp);
  const int64_t base = (int64_t)blockIdx.x * L;
  const int cnt = (int)(len - base < L ? len - base : L);
  double self = 0.0, self3[3] = {0.0, 0.0, 0.0};
  if constexpr (SCALE == 3) {
    qtw_stage_two(r, V + (int64_t)j * ldv, base, cnt >> 1, sw, sw + (L >> 1), self3);
#pragma unroll
    for (int q = 0; q < 3; ++q) self3[q] = wave_sum(self3[q]);
  } else if constexpr (SCALE == 4) {
    // fused small-problem mode: finish the previous step here (see QtwFuse), then stage and dot r like SCALE == 2
    // np > 0 (small problems): alpha is added up here from the SpMV's block partials; np == 0 (any size): alpha has been
    // reduced (and all-reduced) already and is read back from its slot
    __shared__ double sm16[16];
    double al;
    if (fz.np > 0) {
      al = final_sum_emulated(fz.apart, fz.np, sm16);
      if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) fz.alpha_out[0] = al;
    } else {
      al = fz.alpha_out[0];
    }
    const double be = fz.jprev2 >= 0 ? fz.beta_prev[0] : 0.0;
    const double2* y2 = reinterpret_cast<const double2*>(r + base);
    double2* ro2 = reinterpret_cast<double2*>(fz.r_out + base);
    const double2* v2 = reinterpret_cast<const double2*>(V + (int64_t)fz.jprev * ldv + base);
    const double2* m2 = fz.jprev2 >= 0 ? reinterpret_cast<const double2*>(V + (int64_t)fz.jprev2 * ldv + base) : nullptr;
    const int cnt2 = cnt >> 1;
    for (int t0 = threadIdx.x; t0 < cnt2; t0 += 5 * kTPB) {
      double2 x[5];
#pragma unroll
      for (int u = 0; u < 5; ++u) {
        const int t = t0 + u * kTPB;
        x[u] = make_double2(0.0, 0.0);
        if (t < cnt2) {
          x[u] = y2[t];
          const double2 v = v2[t];
          x[u].x = x[u].x - v.x * al;  // k_three_term's expression, element for element
          x[u].y = x[u].y - v.y * al;
          if (m2) {
            const double2 m = m2[t];
            x[u].x = x[u].x - m.x * be;
            x[u].y = x[u].y - m.y * be;
          }
          if (blockIdx.y == 0) ro2[t] = x[u];  // (row split: every block of the slice computes it, one stores it)
        }
      }
#pragma unroll
      for (int u = 0; u < 5; ++u)
        if (t0 + u * kTPB < cnt2) {
          sw[t0 + u * kTPB] = x[u];
          self = fma(x[u].x, x[u].x, self);
          self = fma(x[u].y, x[u].y, self);
        }
    }
    self = wave_sum(self);
  } else {
    self = qtw_stage_w<SCALE>(V, ldv, j, r, nrm2, beta_slot, base, cnt >> 1, sw);
    self = wave_sum(self);  // this wave's share of w.w (lane 0); replaces the streamed row-j result below
  }
  const int jskip = SCALE == 3 ? -1 : j;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int li = lane & 3, blk = (lane >> 2) & 3, lk = lane >> 4;
  const int sub = (int)(L >> 2);  // elements per wave (multiple of 128)
  const int m_lo = w * sub;
  int m_hi = m_lo + sub;
  if (m_hi > cnt) m_hi = cnt;
  const int nsteps = m_hi > m_lo ? (m_hi - m_lo) >> 5 : 0;  // 32 elements (256 B per row) per step
  const int eoff = 8 * blk + 2 * lk;                          // this lane's double2 within a step
  // B operand: column jj = lane & 3 of each 4x4 block; one-reduce mode gives the odd columns the second vector
  const double2* swl = sw + ((m_lo + eoff) >> 1) + ((SCALE == 3 && (lane & 1)) ? (L >> 1) : 0);  // + 16 per step
  const int i_top = nrows > 0 ? ((nrows - 1) / (4 * T)) * (4 * T) : 0;
  // Row pointers of tile k (tiles run from the newest rows down).
  auto tile_rows = [&](int i0, const double2* (&a)[T]) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      int i = i0 + 4 * t + li;
      if (i >= nrows) i = nrows - 1;  // clamped duplicate, discarded at the store
      if (i == jskip) i = j > 0 ? j - 1 : (nrows > 1 ? 1 : 0);  // row j is w itself: its coefficient comes from `self`
      a[t] = reinterpret_cast<const double2*>(V + (int64_t)i * ldv + base + m_lo + eoff);
    }
  };
  auto load_batch = [&](const double2* const (&a)[T], int s0, double2 (&av)[T][U]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < T; ++t) av[t][u] = (s0 + u < nsteps) ? ld_stream<1>(a[t] + 16 * (s0 + u)) : make_double2(0.0, 0.0);
  };
  auto mma_batch = [&](int s0, const double2 (&av)[T][U], double (&acc)[T]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const double2 bv = (s0 + u < nsteps) ? swl[16 * (s0 + u)] : make_double2(0.0, 0.0);
#pragma unroll
      for (int t = 0; t < T; ++t) {
        acc[t] = __builtin_amdgcn_mfma_f64_4x4x4f64(av[t][u].x, bv.x, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f64_4x4x4f64(av[t][u].y, bv.y, acc[t], 0, 0, 0);
      }
    }
  };
  // The first batch of loads of the NEXT tile is issued before the current tile's results are reduced and stored: the
  // end of a tile otherwise drains the wave's whole load queue (s_waitcnt 0 before the cross-lane adds), a bubble that
  // cost 6 % of the pass (profiles/r01/ab_qtw_tile_epilogue.json).
  const int ntiles = nrows > 0 ? i_top / (4 * T) + 1 : 0;  // one-reduce mode at j = 0: no rows yet, only the self terms
  // Row split (gridDim.y > 1, short vectors with many basis rows - 1Ddeuteron.py: M = n = 1001): the blocks
  // (blockIdx.x, 0..Y-1) share slice blockIdx.x and deal its row tiles round-robin; every (row, slice, quarter) dot is
  // still one wave's same MFMA sequence and every block writes exactly its own rows of the slice's run: same bits, Y
  // times the parallelism.
  const int ky = blockIdx.y, kstep = gridDim.y;
  const double2* a[T];
  double2 av0[T][U];
  if (ky < ntiles) {
    tile_rows(i_top - ky * 4 * T, a);
    load_batch(a, 0, av0);
  }
  for (int k = ky; k < ntiles; k += kstep) {
    const int i0 = i_top - k * 4 * T;
    double acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = 0.0;
    mma_batch(0, av0, acc);
    for (int s0 = U; s0 < nsteps; s0 += U) {
      double2 av[T][U];
      load_batch(a, s0, av);
      mma_batch(s0, av, acc);
    }
    if (k + kstep < ntiles) {
      tile_rows(i_top - (k + kstep) * 4 * T, a);
      load_batch(a, 0, av0);
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      double v = acc[t];                 // D[blk][i][jj] in lane 16 i + 4 blk + jj
      v += __shfl_xor(v, 4, 64);         // add the four blocks (adjacent 64-byte chunks)
      v += __shfl_xor(v, 8, 64);
      const int row = i0 + 4 * t + lk;   // lane 16 i (+0) holds row i
      if ((lane & 15) == 0 && row < nrows) keep[row] = v;
      if (SCALE == 3 && (lane & 15) == 1 && row < nrows) keep[ldp + row] = v;  // column 1: dots with u
    }
  }
  if (SCALE == 3) {
    if (lane == 0) {  // slots behind the streamed rows: [nrows] = r''.r'', [ldp + nrows] = u.u, [ldp + nrows + 1] = u.r''
      keep[nrows] = self3[0];
      keep[ldp + nrows] = self3[2];
      keep[ldp + nrows + 1] = self3[1];
    }
  } else if (lane == 0 && j < nrows) {
    keep[j] = self;  // c_j = w.w from the LDS-resident values (row j itself is not streamed)
  }
  __syncthreads();  // the only barrier after staging: the four waves' runs are added (fixed order) and leave as one
  const int run = NCOL * ldp;
  const int nout = SCALE == 3 ? ldp + nrows + 2 : nrows;
  const double* k0 = reinterpret_cast<const double*>(sw) + NCOL * L;
  double* mine = part + (int64_t)blockIdx.x * run;
  const int t_top = i_top / (4 * T);
  for (int i = threadIdx.x; i < nout; i += kTPB) {
    if (kstep > 1) {  // row split: this block owns the tiles k == ky (mod Y) counted from the top, and block 0 row j's self term
      const bool mine_row = i == j ? ky == 0 : (t_top - i / (4 * T)) % kstep == ky;
      if (!mine_row) continue;
    }
    __builtin_nontemporal_store(((k0[i] + k0[run + i]) + k0[2 * run + i]) + k0[3 * run + i], mine + i);
  }
  // Device-resident partial re-orthogonalisation (fz.ticket != nullptr; SCALE == 1 or 3, no row split): the block that finishes LAST
  // adds up every block's run itself - k_final_rows_t's additions in k_final_rows_t's order, so c has the same bits - which
  // saves that kernel's launch in the 99 % of steps where this kernel returns at its first line.  The release / acquire
  // pair around the ticket costs more than the launch it replaces (the two-sided links measured 2-4x), but only a step that
  // really sweeps pays it.
  if constexpr (SCALE == 1 || SCALE == 3) {
    if (fz.ticket != nullptr) {
      __shared__ unsigned s_last;
      __threadfence();  // this block's run is visible device-wide before its ticket is
      __syncthreads();  // (and every wave is done with the LDS image)
      if (threadIdx.x == 0) s_last = atomicAdd(fz.ticket, 1u) == gridDim.x * gridDim.y - 1 ? 1u : 0u;
      __syncthreads();
      if (s_last) {
        __threadfence();  // the other blocks' runs
        double* smf = reinterpret_cast<double*>(sw);  // [128][8] doubles of the (now free) slice image
        constexpr int S = kFinalThreads / 8;
        const int P = (int)gridDim.x;
        const int ldrun = NCOL * ldp;  // (one-reduce mode: runs of 2 ldp doubles, ldp + nrows + 2 of them meaningful)
        for (int g8 = 0; g8 < (nout + 7) / 8; ++g8) {
#pragma unroll
          for (int q = 0; q < kFinalThreads / kTPB; ++q) {  // a 256-thread block plays k_final_rows_t's 1024 threads
            const int vt = threadIdx.x + q * kTPB;
            const int rl = vt & 7, pl = vt >> 3;
            const double* p = part + (g8 * 8 + rl);
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            int pid = pl;
            for (; pid + 3 * S < P; pid += 4 * S) {
              a0 += p[(int64_t)pid * ldrun];
              a1 += p[(int64_t)(pid + S) * ldrun];
              a2 += p[(int64_t)(pid + 2 * S) * ldrun];
              a3 += p[(int64_t)(pid + 3 * S) * ldrun];
            }
            for (; pid < P; pid += S) a0 += p[(int64_t)pid * ldrun];
            smf[pl * 8 + rl] = (a0 + a1) + (a2 + a3);
          }
          __syncthreads();
          if (threadIdx.x < 8 && g8 * 8 + (int)threadIdx.x < nout) {
            double t = 0.0;
            for (int k = 0; k < S; ++k) t += smf[k * 8 + threadIdx.x];
            fz.c_out[g8 * 8 + threadIdx.x] = t;
          }
          __syncthreads();
        }
        if (threadIdx.x == 0) fz.ticket[0] = 0u;  // ready for the next sweep
      }
    }
  }
}

// LDS bytes left for ONE slice of w in the default (4x4x4 MFMA) kernel: a block stages ncol slices and parks ncol sets of four
// coefficient runs of qtw_ldp(rows) doubles (one-reduce mode: two columns, and two more "rows" for the self terms)
static int64_t qtw_room(int flags, int nrows_max) {
  const int ncol = (flags & LZ_FLAG_ONE_REDUCE) ? 2 : 1;
  return (int64_t)155 * 1024 / ncol - (int64_t)(kTPB / 64) * qtw_ldp(nrows_max + (ncol == 2 ? 2 : 0)) * 8;
}

QtwPlan plan_qtw(int64_t len, int flags, const int* tune, int nrows_max) {
  QtwPlan p;
  int64_t target = (tune && tune[0] > 0) ? tune[0] : 0;
  // Two effects set the slice length (profiles/r01/ab_qtw_slice_balance.json): (a) a CU streams at a fixed share of the
  // HBM rate, so the pass finishes when the CU with the most blocks does - G blocks on 256 CUs run at
  // (G/256) / ceil(G/256) of the balanced rate (G = 612 or 815: 80 %, G = 489, 977, 1223: 95 %); (b) every tile ends in a
  // small reduction + partial stores, which favours long slices (L = 512: -9 %, 1024: -3 %, >= 2560: < 1 %).
  int64_t L = 512;
  if (target > 0) {
    L = round_up(target, 512);
  } else {
    // the longest slice that still gives every CU about two blocks and an even share; else the best-balanced one
    double best = -1.0;
    bool found = false;
    // the default kernel also parks four coefficient runs of qtw_ldp(n) doubles in LDS: with thousands of basis rows the
    // slice has to shrink to stay inside the 160 KiB of a CU (n = 4000 -> L <= 3072)
    int64_t lmax = (flags & LZ_FLAG_ONE_REDUCE) ? kQtwMaxL / 2 : kQtwMaxL;  // one-reduce mode stages two slices per block
    const int64_t room = qtw_room(flags, nrows_max);
    if (room / 8 < lmax) lmax = std::max<int64_t>(512, room / 8 / 512 * 512);
    for (int64_t cand = lmax; cand >= 1024 && !found; cand -= 512) {
      const int64_t G = (len + cand - 1) / cand;
      if (G < 480) continue;
      const double g = (double)G / kNumCU, bal = g / std::ceil(g);
      if (bal >= 0.93) {
        L = cand;
        found = true;
      } else if (bal * (double)cand / (double)(cand + 48) > best) {
        best = bal * (double)cand / (double)(cand + 48);
        L = cand;
      }
    }
  }
  if (L > kQtwMaxL) L = kQtwMaxL;
  p.L = L;
  p.G = (int)((len + L - 1) / L);
  // kernel family: 2 = 4x4x4 MFMA (default: matrix cores, line-coalesced loads), 1 = 16x16x4 MFMA (A/B arm),
  // 0 = VALU + shuffle reductions (LZ_FLAG_QTW_VALU)
  p.family = (flags & LZ_FLAG_QTW_VALU) ? 0 : ((flags & LZ_FLAG_QTW_MFMA) ? 1 : 2);
  if (p.family == 2 && qtw_room(flags, nrows_max) < L * 8)
    p.family = 0;  // ~5000 basis rows and more: the coefficient runs no longer fit next to any slice - VALU kernel, partials in HBM
  p.mfma = p.family != 0;
  p.variant = tune ? tune[1] : 0;
  p.P = p.family == 1 ? p.G * (kTPB / 64) : p.G;  // 16x16x4 kernel: per-wave partials; the others: one run per block
  return p;
}

template <int SCALE>
static hipError_t launch_qtw_t(double* V, int64_t ldv, int64_t len, int nrows, int j, const double* r, const double* nrm2,
                         double* beta_slot, const QtwPlan& plan, double* part, hipStream_t s, const QtwFuse& fz) {
  const size_t lds = (size_t)plan.L * sizeof(double);
  const dim3 grid(plan.G), block(kTPB);
#define LZ_QTW_ARGS V, ldv, len, nrows, j, r, nrm2, beta_slot, plan.L, plan.P, part
  if (plan.family == 2) {
    const int ncol = SCALE == 3 ? 2 : 1;
    const int ldp = qtw_ldp(SCALE == 3 ? nrows + 2 : nrows);
    size_t lds4 = ncol * (lds + (size_t)(kTPB / 64) * ldp * sizeof(double));  // slice(s) of w + the four waves' coefficient runs
    if (fz.ticket) lds4 = std::max<size_t>(lds4, (size_t)kFinalThreads * sizeof(double));  // the folded second stage's [128][8] image
    // row split for short vectors (see the kernel): only where the slices alone leave most of the chip idle, and only in
    // the modes whose staging stores nothing that other blocks of the same slice would race on
    dim3 grid2 = grid;
    if ((SCALE == 2 || SCALE == 4) && plan.G <= 64 && nrows > 8) {
      const int ntiles = (nrows + 7) / 8;
      int Y = 256 / plan.G;
      if (Y > ntiles) Y = ntiles;
      if (Y > 1) grid2 = dim3(plan.G, Y);
    }
    hipError_t err = hipSuccess;
    auto go = [&](auto kern) {
      // more than 64 KiB of dynamic LDS (long slices with many hundred basis rows) has to be allowed per kernel
      if (lds4 > 65536)
        err = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds4);
      if (err == hipSuccess)
        hipLaunchKernelGGL(kern, grid2, block, lds4, s, V, ldv, len, nrows, j, r, nrm2, beta_slot, plan.L, ldp, part, fz);
    };
    switch (plan.variant) {
      case 10: go(k_qtw_mfma4<SCALE, 4, 4>); break;
      case 11: go(k_qtw_mfma4<SCALE, 2, 8>); break;
      case 13: go(k_qtw_mfma4<SCALE, 8, 2>); break;
      default: go(k_qtw_mfma4<SCALE, 4, 2>); break;     // measured best: 2 tiles of 4 rows x 4 steps = 8 loads in flight per lane
    }
    return err;
  }
  if constexpr (SCALE == 3 || SCALE == 4) return hipErrorInvalidValue;  // these modes exist for the default (4x4x4 MFMA) family only
#ifdef LZ_KBENCH
  if constexpr (SCALE != 2 && SCALE != 3 && SCALE != 4) {
    if (plan.family == 1) return kb_launch_qtw_mfma<SCALE>(V, ldv, len, nrows, j, r, nrm2, beta_slot, plan, part, s);
  }
#else
  if (plan.family == 1) return hipErrorInvalidValue;  // (lz_set_options refuses LZ_FLAG_QTW_MFMA in the product library)
#endif
  switch (plan.variant) {
    case 1: hipLaunchKernelGGL((k_qtw_valu<SCALE, 4, 2>), grid, block, lds, s, LZ_QTW_ARGS); break;
    case 7: hipLaunchKernelGGL((k_qtw_valu<SCALE, 8, 2, 0>), grid, block, lds, s, LZ_QTW_ARGS); break;  // plain (cached) loads
    default:  // measured best on MI355X (profiles/r01): 8 rows x 2 positions = 16 loads in flight per lane
      if (nrows > 4)
        hipLaunchKernelGGL((k_qtw_valu<SCALE, 8, 2>), grid, block, lds, s, LZ_QTW_ARGS);
      else
        hipLaunchKernelGGL((k_qtw_valu<SCALE, 4, 2>), grid, block, lds, s, LZ_QTW_ARGS);
      break;
  }
#undef LZ_QTW_ARGS
  return hipSuccess;
}

hipError_t launch_qtw(double* V, int64_t ldv, int64_t len, int nrows, int j, const double* r, const double* nrm2,
                      double* beta_slot, const QtwPlan& plan, double* part, int mode, hipStream_t s, const QtwFuse* fuse) {
  const QtwFuse fz = fuse ? *fuse : QtwFuse();
  if (mode == 4) return launch_qtw_t<4>(V, ldv, len, nrows, j, r, nrm2, beta_slot, plan, part, s, fz);
  if (mode == 3) return launch_qtw_t<3>(V, ldv, len, nrows, j, r, nrm2, beta_slot, plan, part, s, fz);
  if (mode == 2) return launch_qtw_t<2>(V, ldv, len, nrows, j, r, nrm2, beta_slot, plan, part, s, fz);
  if (mode == 1) return launch_qtw_t<1>(V, ldv, len, nrows, j, r, nrm2, beta_slot, plan, part, s, fz);
  return launch_qtw_t<0>(V, ldv, len, nrows, j, r, nrm2, beta_slot, plan, part, s, fz);
}

// ------------------------------------------------------------------ re-orthogonalisation pass 2
// V[j] = 2 V[j] - (((c0 V0 + c1 V1) + c2 V2) + ...): NumPy's axis-0 reduction
// order of np.sum(c[:, None] * V, axis=0) (Lanczos.py:249), products and sums
// rounded separately.  One double2 column position per lane; the row loop is
// unrolled so 8 independent 16-byte loads are in flight per lane.
template <bool FUSED, int VAR = 0, int UN = 8>
__global__ __launch_bounds__(kTPB) void k_update(double* __restrict__ V, int64_t ldv, int64_t p0, int64_t n2, int nrows, int j,
                                                const double* __restrict__ c, const double* __restrict__ r,
                                                const double* __restrict__ beta) {
  const int64_t i = p0 + (int64_t)blockIdx.x * kTPB + threadIdx.x;  // double2 positions [p0, n2)
  if (i >= n2) return;
  const double2* col = reinterpret_cast<const double2*>(V) + i;
  const int64_t ld2 = ldv >> 1;
  double2* out = reinterpret_cast<double2*>(V) + (int64_t)j * ld2 + i;
  double2 w;
  if (FUSED) {  // fused-norm mode: V[j] has not been formed yet, w = r / beta
    const double b = beta[0];
    w = reinterpret_cast<const double2*>(r)[i];
    w.x = w.x / b;
    w.y = w.y / b;
  }
  double tx = 0.0, ty = 0.0;
  int k = 0;
  for (; k + UN <= nrows; k += UN) {
    double2 q[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) q[u] = (FUSED && k + u == j) ? w : ld_stream<VAR>(col + (int64_t)(k + u) * ld2);
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const double ck = c[k + u];
      tx = tx + ck * q[u].x;
      ty = ty + ck * q[u].y;
    }
  }
  if (k < nrows) {  // tail (< UN rows): still one batch of independent loads, not one round trip per row
    const int rem = nrows - k;  // block-uniform
    double2 q[UN];
#pragma unroll
    for (int u = 0; u < UN - 1; ++u)
      if (u < rem) q[u] = (FUSED && k + u == j) ? w : ld_stream<VAR>(col + (int64_t)(k + u) * ld2);
#pragma unroll
    for (int u = 0; u < UN - 1; ++u)
      if (u < rem) {
        const double ck = c[k + u];
        tx = tx + ck * q[u].x;
        ty = ty + ck * q[u].y;
      }
  }
  const double2 v = FUSED ? w : ld_stream<VAR>(out);
  st_stream<VAR>(out, make_double2(2.0 * v.x - tx, 2.0 * v.y - ty));
}

// Default pass-2 kernel: "slice owner".  A block owns 256*P consecutive double2 positions of the row and keeps their
// running sums in registers while it walks ALL basis rows, RU rows x P positions = RU*P independent 16-byte loads in
// flight per lane.  Same per-element arithmetic and order as k_update; the difference is WHEN V[j] is written: every
// block of a residency round finishes at about the same time, so the 8M bytes of stores arrive as a few bursts at the
// end instead of trickling in between the reads for the whole launch.  A 1 % trickle of writes costs ~15 % of HBM read
// throughput on MI355X (tools/probes/hbm_read_peak.hip: 6.8 -> 5.8 TB/s), presumably read<->write bus turnarounds.
// MODE 1 (one-reduce partial loop; FUSED, raw_c == 1): w = (r'' - alpha u) / beta is formed here from the two-term residual r'' (`r`),
// the newest basis vector u (`usub`) and alpha (`asub`) - k_three_term's expression, then the division - and the gate selects
// between the sweep (V[j] = 2 w - sum c_i V_i) and the plain V[j] = w: one launch per step does either.
template <bool FUSED, int P, int RU, int MODE = 0>
__global__ __launch_bounds__(kTPB) void k_update_slice(double* __restrict__ V, int64_t ldv, int64_t p0, int64_t n2, int nrows,
                                                      int j, const double* __restrict__ c, const double* __restrict__ r,
                                                      double* __restrict__ beta, int raw_c, int nblk_a, int64_t p0b,
                                                      int64_t n2b, int cG, int cldp, const int* __restrict__ gate,
                                                      const double* __restrict__ usub, const double* __restrict__ asub) {
  bool sweep = true;
  if (MODE == 1) {
    sweep = gate[0] != 0;
  } else if (gate && gate[0] == 0) {
    return;  // device-resident partial re-orthogonalisation: no sweep on this vector
  }
  // blocks [0, nblk_a) cover positions [p0, n2); any further blocks cover a second range [p0b, n2b) (the two faces of a
  // slab in overlap mode leave in one launch)
  int bx = blockIdx.x;
  if (bx >= nblk_a) {
    bx -= nblk_a;
    p0 = p0b;
    n2 = n2b;
  }
  const int64_t base = p0 + (int64_t)bx * (kTPB * P) + threadIdx.x;
  const int64_t ld2 = ldv >> 1;
  const double2* V2 = reinterpret_cast<const double2*>(V);
  int64_t pos[P];
  bool ok[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    pos[p] = base + (int64_t)p * kTPB;
    ok[p] = pos[p] < n2;
    if (!ok[p]) pos[p] = n2 - 1;  // valid address, result discarded
  }
  double2 w[P];
#pragma unroll
  for (int p = 0; p < P; ++p) w[p] = make_double2(0.0, 0.0);
  // raw_c (fused-norm mode inside lz_run): c still holds the reduced sums [V_0.r, ..., V_{j-1}.r, r.r]; beta and the
  // coefficients of w = r / beta are formed here with k_fused_prepare's arithmetic (one tiny launch less per step).
  // raw_c == 2 (fused small-problem mode): c is pass 1's block partials (cG runs of cldp doubles); a coefficient is their
  // sum in k_final_rows_t's order (from 0.0, block by block) - the second-stage launch is folded in here: the block adds
  // them up once, into LDS (nrows doubles of dynamic shared memory).
  extern __shared__ double cs[];
  if (FUSED && raw_c == 2) {
    for (int k = threadIdx.x; k < nrows; k += kTPB) {
      double t = 0.0;
      for (int b = 0; b < cG; ++b) t += c[(int64_t)b * cldp + k];
      cs[k] = t;
    }
    __syncthreads();
  }
  double bnorm = 1.0;
  if (FUSED && raw_c) {
    bnorm = sqrt(raw_c == 2 ? cs[j] : c[j]);
    if (blockIdx.x == 0 && threadIdx.x == 0) beta[0] = bnorm;
  }
  if (FUSED) {
    const double b = raw_c ? bnorm : beta[0];
    const double a = MODE == 1 ? asub[0] : 0.0;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      w[p] = reinterpret_cast<const double2*>(r)[pos[p]];
      if (MODE == 1) {
        const double2 uu = reinterpret_cast<const double2*>(usub)[pos[p]];
        w[p].x = w[p].x - uu.x * a;
        w[p].y = w[p].y - uu.y * a;
      }
      w[p].x = w[p].x / b;
      w[p].y = w[p].y / b;
    }
  }
  if (MODE == 1 && !sweep) nrows = 0;  // no sweep on this vector: V[j] = w
  double tx[P], ty[P];
#pragma unroll
  for (int p = 0; p < P; ++p) tx[p] = ty[p] = 0.0;
  for (int k = 0; k < nrows; k += RU) {
    double2 q[RU][P];
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (k + u < nrows) {  // block-uniform
        const double2* row = V2 + (int64_t)(k + u) * ld2;
#pragma unroll
        for (int p = 0; p < P; ++p) q[u][p] = (FUSED && k + u == j) ? w[p] : ld_stream<1>(row + pos[p]);
      }
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (k + u < nrows) {
        double ck = (FUSED && raw_c == 2) ? cs[k + u] : c[k + u];
        if (FUSED && raw_c) ck = (k + u == j) ? ck / (bnorm * bnorm) : ck / bnorm;
        if (!FUSED && k + u == j) {  // row j is V[j] itself (j < nrows): keep it for the final 2 v - t instead of re-reading it
#pragma unroll
          for (int p = 0; p < P; ++p) w[p] = q[u][p];
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
          tx[p] = tx[p] + ck * q[u][p].x;
          ty[p] = ty[p] + ck * q[u][p].y;
        }
      }
  }
  double2* out = reinterpret_cast<double2*>(V) + (int64_t)j * ld2;
#pragma unroll
  for (int p = 0; p < P; ++p)
    if (ok[p]) st_stream<1>(out + pos[p], (MODE == 1 && !sweep) ? w[p] : make_double2(2.0 * w[p].x - tx[p], 2.0 * w[p].y - ty[p]));
}

// Pass 2 for SHORT vectors with many basis rows (1Ddeuteron.py: M = n = 1001): the walk over the rows is a latency chain
// per element and there are only len elements to overlap chains with, so one ELEMENT (not a double2) per lane, 32 rows per
// trip, and the next trip's loads in flight while the current one is added up (two register buffers): four times the
// loads in flight of k_update_slice<.., 1, 32>.  Same per-element arithmetic and order (NumPy's), fused-norm mode only.
__global__ __launch_bounds__(kTPB) void k_update_elem(double* __restrict__ V, int64_t ldv, int64_t len, int nrows, int j,
                                                     const double* __restrict__ c, const double* __restrict__ r,
                                                     double* __restrict__ beta, int raw_c, int cG, int cldp) {
  extern __shared__ double cs[];
  if (raw_c == 2) {  // fused small-problem mode: add pass 1's block partials in k_final_rows_t's order, once per block
    for (int k = threadIdx.x; k < nrows; k += kTPB) {
      double t = 0.0;
      for (int b = 0; b < cG; ++b) t += c[(int64_t)b * cldp + k];
      cs[k] = t;
    }
    __syncthreads();
  }
  const double* cc = raw_c == 2 ? cs : c;
  double bnorm = 1.0;
  if (raw_c) {
    bnorm = sqrt(cc[j]);
    if (blockIdx.x == 0 && threadIdx.x == 0) beta[0] = bnorm;
  }
  const int64_t e0 = (int64_t)blockIdx.x * kTPB + threadIdx.x;
  const bool ok = e0 < len;
  const int64_t e = ok ? e0 : len - 1;  // valid address, result discarded
  const double b = raw_c ? bnorm : beta[0];
  const double w = r[e] / b;
  constexpr int RU = 32;
  double q[2][RU];
  auto load = [&](int k, double (&dst)[RU]) {
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (k + u < nrows) dst[u] = (k + u == j) ? w : __builtin_nontemporal_load(V + (int64_t)(k + u) * ldv + e);
  };
  double tx = 0.0;
  auto add = [&](int k, const double (&src)[RU]) {
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (k + u < nrows) {
        double ck = cc[k + u];
        if (raw_c) ck = (k + u == j) ? ck / (bnorm * bnorm) : ck / bnorm;
        tx = tx + ck * src[u];
      }
  };
  load(0, q[0]);
  for (int k = 0; k < nrows; k += 2 * RU) {
    if (k + RU < nrows) load(k + RU, q[1]);
    add(k, q[0]);
    if (k + 2 * RU < nrows) load(k + 2 * RU, q[0]);
    if (k + RU < nrows) add(k + RU, q[1]);
  }
  if (ok) V[(int64_t)j * ldv + e] = 2.0 * w - tx;
}

template <bool FUSED, int P, int RU>
static void launch_update_slice(double* V, int64_t ldv, int64_t p0, int64_t n2, int nrows, int j, const double* c, const double* r,
                                double* beta, int raw_c, hipStream_t s, int64_t p0b = 0, int64_t n2b = 0, int cG = 0, int cldp = 0,
                                const int* gate = nullptr, const double* usub = nullptr, const double* asub = nullptr) {
  const int grid = (int)((n2 - p0 + kTPB * P - 1) / (kTPB * P));
  const int grid_b = n2b > p0b ? (int)((n2b - p0b + kTPB * P - 1) / (kTPB * P)) : 0;
  if constexpr (FUSED) {
    if (usub) {  // one-reduce partial loop: the three-term subtraction and the sweep / no-sweep choice live in the kernel
      hipLaunchKernelGGL((k_update_slice<true, P, RU, 1>), dim3(grid + grid_b), dim3(kTPB), 0, s, V, ldv, p0, n2, nrows, j, c, r, beta, raw_c, grid, p0b, n2b,
                         cG, cldp, gate, usub, asub);
      return;
    }
  }
  hipLaunchKernelGGL((k_update_slice<FUSED, P, RU>), dim3(grid + grid_b), dim3(kTPB), raw_c == 2 ? (size_t)nrows * sizeof(double) : 0, s, V, ldv, p0,
                     n2, nrows, j, c, r, beta, raw_c, grid, p0b, n2b, cG, cldp, gate, (const double*)nullptr, (const double*)nullptr);
}

void launch_update(double* V, int64_t ldv, int64_t len, int nrows, int j, const double* c, const double* r_fused,
                   double* beta, int variant, hipStream_t s, int64_t pos_lo, int64_t pos_hi, int raw_c, int64_t pos_lo_b,
                   int64_t pos_hi_b, int cG, int cldp, const int* gate, const double* usub, const double* asub) {
  // gate (device-resident partial re-orthogonalisation): the default slice-owner kernels only
  // double2 positions [pos_lo, pos_hi) of the row (default: the whole row)
  const int64_t n2 = pos_hi >= 0 ? pos_hi : (len >> 1);
  const int64_t p0 = pos_lo > 0 ? pos_lo : 0;
  if (n2 <= p0) return;
  const int grid = (int)((n2 - p0 + kTPB - 1) / kTPB);
  if (!r_fused && variant == 1) {  // A/B arm: plain (cached) loads
    hipLaunchKernelGGL((k_update<false, 0, 8>), dim3(grid), dim3(kTPB), 0, s, V, ldv, p0, n2, nrows, j, c, r_fused, beta);
    return;
  }
  if (variant == 2) {  // A/B arm: one position per lane, non-temporal loads (stores trickle through the whole launch)
    if (r_fused)
      hipLaunchKernelGGL((k_update<true, 1, 8>), dim3(grid), dim3(kTPB), 0, s, V, ldv, p0, n2, nrows, j, c, r_fused, beta);
    else
      hipLaunchKernelGGL((k_update<false, 1, 8>), dim3(grid), dim3(kTPB), 0, s, V, ldv, p0, n2, nrows, j, c, r_fused, beta);
    return;
  }
  // default: slice-owner kernel.  Positions per lane P in {16, 8, 4, 2} (always 16 loads in flight): like the Q.w pass this
  // one finishes with the most loaded CU, so take the P whose block count spreads most evenly over the 256 CUs
  // (M = 1.25e6: 306 blocks of P = 8 run at 60 %, 1223 blocks of P = 2 at 95 %); ties go to the larger P.
  const int64_t span = n2 - p0;
  int P = variant == 3 ? 8 : (variant == 4 ? 4 : 0);
  if (!P) {
    double best = -1.0;
    P = 2;
    for (int cand : {16, 8, 4, 2}) {
      const int64_t G = (span + (int64_t)kTPB * cand - 1) / ((int64_t)kTPB * cand);
      const double g = (double)G / kNumCU, bal = g / std::ceil(g);
      if (bal >= 0.93) {  // 16 loads in flight per lane: one block per CU already keeps the CU's share of HBM busy
        P = cand;
        break;
      }
      if (bal > best) {
        best = bal;
        P = cand;
      }
    }
  }
  if (variant == 6 || (variant == 0 && P == 16 && span > 16384)) {
    // 16 positions per lane, one row per trip (still 16 loads in flight): half as many, longer-lived blocks - fewer
    // residency rounds, so V[j] leaves in fewer, larger write bursts (1250 -> 1218 us at the headline)
    if (r_fused) launch_update_slice<true, 16, 1>(V, ldv, p0, n2, nrows, j, c, r_fused, beta, raw_c, s, 0, 0, cG, cldp, gate, usub, asub);
    else launch_update_slice<false, 16, 1>(V, ldv, p0, n2, nrows, j, c, r_fused, beta, 0, s, 0, 0, 0, 0, gate);
    return;
  }
  if (variant == 0 && span <= 4096 && r_fused && nrows > 64 && pos_hi < 0 && pos_lo <= 0 && !gate) {
    // a short vector against many rows: the element-per-lane, double-buffered kernel (see k_update_elem)
    const int grid_e = (int)((len + kTPB - 1) / kTPB);
    hipLaunchKernelGGL(k_update_elem, dim3(grid_e), dim3(kTPB), raw_c == 2 ? (size_t)nrows * sizeof(double) : 0, s, V, ldv, len, nrows, j, c, r_fused,
                       beta, raw_c, cG, cldp);
    return;
  }
  if ((variant == 0 && span <= 16384) || variant == 5) {
    // a face of the slab (overlap mode) or a tiny vector: a handful of blocks walk all rows, which is a latency chain,
    // not a bandwidth problem - one position per lane (most blocks) and 32 rows in flight per lane
    if (r_fused) launch_update_slice<true, 1, 32>(V, ldv, p0, n2, nrows, j, c, r_fused, beta, raw_c, s, pos_lo_b, pos_hi_b, cG, cldp, gate, usub, asub);
    else launch_update_slice<false, 1, 32>(V, ldv, p0, n2, nrows, j, c, r_fused, beta, 0, s, pos_lo_b, pos_hi_b, 0, 0, gate);
  } else if (P == 8) {
    if (r_fused) launch_update_slice<true, 8, 2>(V, ldv, p0, n2, nrows, j, c, r_fused, beta, raw_c, s, 0, 0, cG, cldp, gate, usub, asub);
    else launch_update_slice<false, 8, 2>(V, ldv, p0, n2, nrows, j, c, r_fused, beta, 0, s, 0, 0, 0, 0, gate);
  } else if (P == 4) {
    if (r_fused) launch_update_slice<true, 4, 4>(V, ldv, p0, n2, nrows, j, c, r_fused, beta, raw_c, s, 0, 0, cG, cldp, gate, usub, asub);
    else launch_update_slice<false, 4, 4>(V, ldv, p0, n2, nrows, j, c, r_fused, beta, 0, s, 0, 0, 0, 0, gate);
  } else {
    if (r_fused) launch_update_slice<true, 2, 8>(V, ldv, p0, n2, nrows, j, c, r_fused, beta, raw_c, s, 0, 0, cG, cldp, gate, usub, asub);
    else launch_update_slice<false, 2, 8>(V, ldv, p0, n2, nrows, j, c, r_fused, beta, 0, s, 0, 0, 0, 0, gate);
  }
}

// partial re-orthogonalisation mode, steps without a sweep: V[j] = r / sqrt(nrm2) and nothing else
__global__ __launch_bounds__(kTPB) void k_scale_store(double* __restrict__ vj, const double* __restrict__ r,
                                                     const double* __restrict__ nrm2, double* __restrict__ beta_slot, int64_t n2,
                                                     const int* __restrict__ gate) {
  if (gate && gate[0] != 0) return;  // device-resident partial re-orthogonalisation: the sweep kernels wrote V[j] and beta
  const double beta = sqrt(nrm2[0]);
  if (blockIdx.x == 0 && threadIdx.x == 0) beta_slot[0] = beta;
  const double2* r2 = reinterpret_cast<const double2*>(r);
  double2* v2 = reinterpret_cast<double2*>(vj);
  for (int64_t i = (int64_t)blockIdx.x * kTPB + threadIdx.x; i < n2; i += (int64_t)gridDim.x * kTPB) {
    double2 x = r2[i];
    x.x = x.x / beta;
    x.y = x.y / beta;
    v2[i] = x;
  }
}
void launch_scale_store(double* vj, const double* r, const double* nrm2, double* beta_slot, int64_t len, hipStream_t s, const int* gate) {
  const int64_t n2 = len >> 1;
  int64_t g = (n2 + kTPB - 1) / kTPB;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  hipLaunchKernelGGL(k_scale_store, dim3((int)g), dim3(kTPB), 0, s, vj, r, nrm2, beta_slot, n2, gate);
}

// fused-norm mode: c holds the all-reduced [V_0.r, ..., V_{j-1}.r, r.r]; turn it into the coefficients of
// w = r / beta:  beta = sqrt(r.r), c_i /= beta, c_j = (r.r) / beta^2
__global__ void k_fused_prepare(double* __restrict__ c, int j, double* __restrict__ beta_slot) {
  const double rr = c[j];
  const double b = sqrt(rr);
  for (int i = threadIdx.x; i < j; i += blockDim.x) c[i] = c[i] / b;
  __syncthreads();
  if (threadIdx.x == 0) {
    c[j] = rr / (b * b);
    beta_slot[0] = b;
  }
}
// One-reduce mode, after the single all-reduce of buf = [p_0..p_{m-1}, r''.r'', gap.., q_0..q_{m-1}, u.u, u.r'', alpha]
// (p_i = V_i.r'', q_i = V_i.u, m rows, second half at offset ldp, alpha = u.(A u) at ldp + m + 2):
//   c_i = V_i . (r'' - alpha u) = p_i - alpha q_i,   c_m = |r'' - alpha u|^2 = r''.r'' - 2 alpha u.r'' + alpha^2 u.u
// left in buf[0..m] exactly where the update kernel's raw-sums path expects [V_i.r ..., r.r]; alpha to alpha_slot.
// The three-sum form of |r|^2 cancels: its relative error is about eps (alpha^2 + beta^2) / beta^2.  Where that would
// break the 1e-10 bar (|r|^2 below 1e-4 of r''.r'', or not positive at all: shifted spectra, a nearly converged Krylov
// space) the kernel raises the sticky flag `bad`; lz_run then repeats the solve on the default two-reduce loop.
//
// The same cancellation leaves u itself off unit length: u was scaled by 1 / sqrt(v) of the step before, so |u| - 1 carries that
// v's relative error, alpha = u.(A u) twice that and beta all of it (on a shifted Laplacian, |alpha| = 3.5 beta, 13 to 21 times
// the rounding of the two-reduce loop).  u.u arrives in this very buffer without cancellation, so the coefficients are taken
// relative to it: alpha = u.(A u) / u.u here and in c_i, |r|^2 (the Rayleigh quotient of u as it is), and - now that the length
// of the u it formed is known - the previous step's beta, sqrt(v) when it was stored, becomes |r| / |u_before| =
// sqrt(v) sqrt(u.u / uu_keep[0]) (beta_prev; nullptr: no previous step of this run).  uu_keep[0] keeps u.u for the next call.
__global__ void k_onereduce_prepare(double* __restrict__ buf, int m, int ldp, double* __restrict__ alpha_slot, double* __restrict__ bad,
                                    double* __restrict__ beta_prev, double* __restrict__ uu_keep) {
  const double uu = buf[ldp + m];
  const double a = buf[ldp + m + 2] / uu;
  for (int i = threadIdx.x; i < m; i += blockDim.x) buf[i] = buf[i] - a * buf[ldp + i];
  __syncthreads();
  if (threadIdx.x == 0) {
    const double rr = buf[m], ur = buf[ldp + m + 1];
    const double v = (rr - 2.0 * a * ur) + a * a * uu;
    if (!(v > 1e-4 * rr)) bad[0] = 1.0;
    buf[m] = v;
    alpha_slot[0] = a;
    if (beta_prev) beta_prev[0] = beta_prev[0] * sqrt(uu / uu_keep[0]);
    uu_keep[0] = uu;
  }
}
void launch_onereduce_prepare(double* buf, int m, int ldp, double* alpha_slot, double* bad, double* beta_prev, double* uu_keep, hipStream_t s) {
  hipLaunchKernelGGL(k_onereduce_prepare, dim3(1), dim3(kTPB), 0, s, buf, m, ldp, alpha_slot, bad, beta_prev, uu_keep);
}
// After the last step of the one-reduce loop: buf holds the all-reduced self terms of a pass over no rows with u = the last basis row
// (u.u at buf[ldp], u.(A u) at buf[ldp + 2]).  The last alpha and the last beta get what k_onereduce_prepare gives every earlier one.
__global__ void k_onereduce_finish(const double* __restrict__ buf, int ldp, double* __restrict__ alpha_last, double* __restrict__ beta_last,
                                   const double* __restrict__ uu_keep) {
  if (threadIdx.x == 0) {
    const double uu = buf[ldp];
    alpha_last[0] = buf[ldp + 2] / uu;
    if (beta_last) beta_last[0] = beta_last[0] * sqrt(uu / uu_keep[0]);
  }
}
void launch_onereduce_finish(const double* buf, int ldp, double* alpha_last, double* beta_last, const double* uu_keep, hipStream_t s) {
  hipLaunchKernelGGL(k_onereduce_finish, dim3(1), dim3(64), 0, s, buf, ldp, alpha_last, beta_last, uu_keep);
}

void launch_fused_prepare(double* c, int j, double* beta_slot, hipStream_t s) {
  hipLaunchKernelGGL(k_fused_prepare, dim3(1), dim3(kTPB), 0, s, c, j, beta_slot);
}

// ------------------------------------------------------------------ three-term recurrence + ||r||^2
// r = (r - v_j * alpha) - v_{j-1} * beta   (Lanczos.py:119, NumPy evaluation order)
__global__ __launch_bounds__(kTPB) void k_three_term(double* __restrict__ r, const double* __restrict__ vj,
                                                    const double* __restrict__ vjm1, const double* __restrict__ alpha,
                                                    const double* __restrict__ beta, int64_t n2, double* __restrict__ part) {
  __shared__ double sm[kTPB / 64];
  const double a = alpha[0];
  const double b = vjm1 ? beta[0] : 0.0;
  double2* r2 = reinterpret_cast<double2*>(r);
  const double2* v2 = reinterpret_cast<const double2*>(vj);
  const double2* m2 = reinterpret_cast<const double2*>(vjm1);
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kTPB + threadIdx.x; i < n2; i += (int64_t)gridDim.x * kTPB) {
    double2 x = r2[i];
    const double2 v = ld_stream<1>(v2 + i);
    x.x = x.x - v.x * a;
    x.y = x.y - v.y * a;
    if (vjm1) {
      const double2 m = ld_stream<1>(m2 + i);
      x.x = x.x - m.x * b;
      x.y = x.y - m.y * b;
    }
    r2[i] = x;  // plain store: r is re-read by the very next kernel (an nt store measured no different)
    acc = fma(x.x, x.x, acc);
    acc = fma(x.y, x.y, acc);
  }
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

int launch_three_term(double* r, const double* vj, const double* vjm1, const double* alpha, const double* beta,
                      int64_t len, double* part, hipStream_t s) {
  const int64_t n2 = len >> 1;
  int64_t g = (n2 + kTPB - 1) / kTPB;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  hipLaunchKernelGGL(k_three_term, dim3((int)g), dim3(kTPB), 0, s, r, vj, vjm1, alpha, beta, n2, part);
  return (int)g;
}

// The group chain in the units of z (one_sweep_quad_iter, lz_loops.hip): the chain vectors stay unscaled in their basis rows, and
// x = z / b is formed by IEEE division wherever a pass reads one - the same bits the scaling SpMV used to store.  Out of place:
// `out` is the next basis row, none of the inputs.  MODE 0, the opening: out = (y - alpha zt) - beta xm, k_three_term's expression
// (zt = V[j-1], xm = V[j-2], beta in `bt`).  MODE 1 / 2, chain step t: out = (y / b_t - alpha (zt / b_t)) - b_t xm' with zt = z_t,
// b_t in `bt`, and xm' = xm = V[j-1] (MODE 1, t = 0: a finished row) or xm / b_{t-1} (MODE 2: xm = z_{t-1}, b_{t-1} in `bm`).
// part[b] = block b's share of ||out||^2.  Padding positions are 0 in every input and leave as 0.
template <int MODE>
__global__ __launch_bounds__(kTPB) void k_three_term_z(double* __restrict__ out, const double* __restrict__ y, const double* __restrict__ zt,
                                                      const double* __restrict__ xm, const double* __restrict__ alpha,
                                                      const double* __restrict__ bt, const double* __restrict__ bm, int64_t n2,
                                                      double* __restrict__ part) {
  __shared__ double sm[kTPB / 64];
  const double a = alpha[0];
  const double b = bt[0];
  const double bp = MODE == 2 ? bm[0] : 1.0;
  double2* o2 = reinterpret_cast<double2*>(out);
  const double2* y2 = reinterpret_cast<const double2*>(y);
  const double2* v2 = reinterpret_cast<const double2*>(zt);
  const double2* m2 = reinterpret_cast<const double2*>(xm);
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kTPB + threadIdx.x; i < n2; i += (int64_t)gridDim.x * kTPB) {
    double2 x = y2[i];
    double2 v, m;
    if (MODE == 0) {  // finished rows, read here for the last time before the walk: streamed
      v = ld_stream<1>(v2 + i);
      m = ld_stream<1>(m2 + i);
    } else {  // rows of this chain, just written
      v = v2[i];
      m = m2[i];
      x.x = x.x / b;
      x.y = x.y / b;
      v.x = v.x / b;
      v.y = v.y / b;
    }
    if (MODE == 2) {
      m.x = m.x / bp;
      m.y = m.y / bp;
    }
    x.x = x.x - v.x * a;
    x.y = x.y - v.y * a;
    x.x = x.x - m.x * b;
    x.y = x.y - m.y * b;
    o2[i] = x;  // plain store: the row is re-read by the very next kernel
    acc = fma(x.x, x.x, acc);
    acc = fma(x.y, x.y, acc);
  }
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

int launch_three_term_z(int mode, double* out, const double* y, const double* zt, const double* xm, const double* alpha, const double* bt,
                        const double* bm, int64_t len, double* part, hipStream_t s) {
  const int64_t n2 = len >> 1;
  int64_t g = (n2 + kTPB - 1) / kTPB;  // (k_three_term's grid)
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
#define LZ_TTZ_GO(MM) hipLaunchKernelGGL(k_three_term_z<MM>, dim3((int)g), dim3(kTPB), 0, s, out, y, zt, xm, alpha, bt, bm, n2, part)
  switch (mode) {
    case 0: LZ_TTZ_GO(0); break;
    case 1: LZ_TTZ_GO(1); break;
    default: LZ_TTZ_GO(2); break;
  }
#undef LZ_TTZ_GO
  return (int)g;
}

// One block behind a chain product on the unscaled z_t: both sums are wanted at the same moment, so one launch adds both partial runs,
// each in k_final_sum's grouping: b_t = sqrt(||z_t||^2) (zpart) -> beta_slot, a_t = (z_t . A z_t) / ||z_t||^2 (apart) -> alpha_slot.
// (nrm2[0] is left alone: the post kernel of the group before may still be reading it on the side stream.)
__global__ __launch_bounds__(kFinalThreads) void k_final_sum_chain(const double* __restrict__ zpart, int nz, const double* __restrict__ apart,
                                                                  int na, double* __restrict__ beta_slot, double* __restrict__ alpha_slot) {
  __shared__ double sm[2][kFinalThreads / 64];
  const double zz = final_sum_1024(zpart, nz, sm[0]);
  const double za = final_sum_1024(apart, na, sm[1]);
  if (threadIdx.x == 0) {
    beta_slot[0] = sqrt(zz);
    alpha_slot[0] = za / zz;
  }
}
void launch_final_sum_chain(const double* zpart, int nz, const double* apart, int na, double* beta_slot, double* alpha_slot, hipStream_t s) {
  hipLaunchKernelGGL(k_final_sum_chain, dim3(1), dim3(kFinalThreads), 0, s, zpart, nz, apart, na, beta_slot, alpha_slot);
}

// One block behind a group's closing product when post runs on the side stream: out[0] = sum(part[0 .. np)) (k_final_sum) and
// root_out[0] = sqrt(nrm2[0]) - b_3, the bits k_os_quad_post stores into its beta slot, for the next group's opening pass, which must
// not wait for post.
__global__ __launch_bounds__(kFinalThreads) void k_final_sum_root(const double* __restrict__ part, int np, double* __restrict__ out,
                                                                 const double* __restrict__ nrm2, double* __restrict__ root_out) {
  __shared__ double sm[kFinalThreads / 64];
  const double t = final_sum_1024(part, np, sm);
  if (threadIdx.x == 0) {
    out[0] = t;
    root_out[0] = sqrt(nrm2[0]);
  }
}
void launch_final_sum_root(const double* part, int np, double* out, const double* nrm2, double* root_out, hipStream_t s) {
  hipLaunchKernelGGL(k_final_sum_root, dim3(1), dim3(kFinalThreads), 0, s, part, np, out, nrm2, root_out);
}

// One-reduce partial loop, behind the SpMV of step j: r'' = y - beta v_{j-1} (k_three_term's expression) and, in the same pass,
// the block partials of the three self terms the next step's ||r||^2 is made of - r''.r'' -> part[b], u.r'' -> part[G + b],
// u.u -> part[2 G + b] with u = v_j - so that a step without a sweep needs no pass 1 at all.
__global__ __launch_bounds__(kTPB) void k_three_term_self(double* __restrict__ r, const double* __restrict__ u, const double* __restrict__ vm,
                                                         const double* __restrict__ beta, int64_t n2, double* __restrict__ part) {
  __shared__ double sm[kTPB / 64];
  const double b = vm ? beta[0] : 0.0;
  double2* r2 = reinterpret_cast<double2*>(r);
  const double2* u2 = reinterpret_cast<const double2*>(u);
  const double2* m2 = reinterpret_cast<const double2*>(vm);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kTPB + threadIdx.x; i < n2; i += (int64_t)gridDim.x * kTPB) {
    double2 x = r2[i];
    const double2 uu = u2[i];  // (v_j was just written and read by the SpMV: plain load)
    if (vm) {
      const double2 m = ld_stream<1>(m2 + i);
      x.x = x.x - m.x * b;
      x.y = x.y - m.y * b;
      r2[i] = x;
    }
    s0 = fma(x.x, x.x, s0);
    s0 = fma(x.y, x.y, s0);
    s1 = fma(uu.x, x.x, s1);
    s1 = fma(uu.y, x.y, s1);
    s2 = fma(uu.x, uu.x, s2);
    s2 = fma(uu.y, uu.y, s2);
  }
  s0 = block_sum(s0, sm);
  s1 = block_sum(s1, sm);
  s2 = block_sum(s2, sm);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = s0;
    part[gridDim.x + blockIdx.x] = s1;
    part[2 * gridDim.x + blockIdx.x] = s2;
  }
}
int launch_three_term_self(double* r, const double* u, const double* vm, const double* beta, int64_t len, double* part, hipStream_t s) {
  const int64_t n2 = len >> 1;
  int64_t g = (n2 + kTPB - 1) / kTPB;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  hipLaunchKernelGGL(k_three_term_self, dim3((int)g), dim3(kTPB), 0, s, r, u, vm, beta, n2, part);
  return (int)g;
}

// ------------------------------------------------------------------ halo pack
__global__ __launch_bounds__(kTPB) void k_gather(const double* __restrict__ x, const int32_t* __restrict__ idx, int64_t n,
                                                double* __restrict__ buf) {
  const int64_t i = (int64_t)blockIdx.x * kTPB + threadIdx.x;
  if (i < n) buf[i] = x[idx[i]];
}
void launch_gather(const double* x, const int32_t* idx, int64_t n, double* buf, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_gather, dim3((int)((n + kTPB - 1) / kTPB)), dim3(kTPB), 0, s, x, idx, n, buf);
}

// ------------------------------------------------------------------ one-sweep full re-orthogonalisation
// One walk over the basis per step instead of two (run_loop_one_sweep, lz_loops.hip): the coefficients are predicted from
// G = V^T V and H (k_os_predict) and applied here, and the dots V_i . u that pass 1 would form are measured from the SAME
// loads, so k_os_post can check the prediction (e = d - c_hat) and correct in the rare step that needs it.  The walk is
// k_update_slice's: a block owns kTPB * P consecutive double2 positions, RU rows x P positions of non-temporal loads in flight
// per lane, running sums in registers, the new row written in bursts at the end.  Per row each wave adds up its share of the
// dot with one shuffle tree and parks it in LDS; the four waves' runs leave as one contiguous run per block (k_final_rows_t
// adds them up).  Per row and lane: P 16-byte loads against 4P FMAs + a 6-step shuffle tree - still far below the VALU
// rate at the HBM rate.
template <int P, int RU, int MODE>
__global__ __launch_bounds__(kTPB) void k_os_sweep(double* __restrict__ V, int64_t ldv, int64_t n2, int j, const double* __restrict__ coef,
                                                  const double* __restrict__ r, const double* __restrict__ nrm2,
                                                  double* __restrict__ beta_slot, int ldp, double* __restrict__ part,
                                                  const int* __restrict__ gate, double* __restrict__ dst,
                                                  const double* __restrict__ alpha_prev, const double* __restrict__ beta_prev) {
  if (MODE == 1 && gate[0] == 0) return;  // no correction due on this step
  extern __shared__ double keep[];        // [kTPB / 64][ldp]: this block's per-wave dots
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * (kTPB * P) + threadIdx.x;
  const int64_t ld2 = ldv >> 1;
  const double2* V2 = reinterpret_cast<const double2*>(V);
  double2* out = reinterpret_cast<double2*>(dst);  // V[j], or the residual buffer (fused form and its correction)
  // (the fused form keeps 32-bit positions - n2 < 2^30, the SpMV's row index is an int - which is what lets its prologue fit the walk's registers)
  using pos_t = std::conditional_t<MODE == 2, int, int64_t>;
  pos_t pos[P];
  bool ok[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    pos[p] = (pos_t)(base + (int64_t)p * kTPB);
    ok[p] = base + (int64_t)p * kTPB < n2;
    if (!ok[p]) pos[p] = (pos_t)(n2 - 1);  // valid address, result discarded
  }
  double2 w[P];
  double b = 1.0, cs = MODE == 2 ? 1.0 : 0.0;  // fused form: units of w, self term 1
  if (MODE == 0) {
    const double s2 = nrm2[0];
    b = sqrt(s2);
    cs = s2 / (b * b);  // the self term c_j = ||w||^2 / beta^2 (k_update_slice's raw_c arithmetic)
    if (blockIdx.x == 0 && threadIdx.x == 0) beta_slot[0] = b;
  }
  double tx[P], ty[P];
#pragma unroll
  for (int p = 0; p < P; ++p) tx[p] = ty[p] = 0.0;
  if (MODE == 2) {
    // fused form (j >= 1): w = (y - alpha V[j-1]) - beta V[j-2] in k_three_term's expression, formed position by position so that
    // the two newest rows are consumed here - their dots against w, ||w||^2 and their share of the sum - and only w and the
    // running sums stay live for the walk over rows 0 .. j-3
    const double a = alpha_prev[0];
    const bool two = j >= 2;  // j == 1: no beta term (the reference's V[-1] is the zero row)
    const double bp = two ? beta_prev[0] : 0.0;
    const double c1 = coef[j - 1], c2 = two ? coef[j - 2] : 0.0;
    const double2* y2 = reinterpret_cast<const double2*>(r);
    const double2* v1 = V2 + (int64_t)(j - 1) * ld2;
    const double2* v2 = V2 + (int64_t)(two ? j - 2 : 0) * ld2;
    double d1 = 0.0, d2 = 0.0, ww = 0.0;
    constexpr int PB = P < 8 ? P : 8;  // positions per batch: 3 PB loads in flight, so that the prologue needs no more registers than the walk
    auto batches = [&](auto two_c) {  // (one straight-line body per case: the batches stay in order)
      constexpr bool TWO = decltype(two_c)::value;
#pragma unroll
      for (int p0 = 0; p0 < P; p0 += PB) {
        double2 x[PB], v[PB], m[PB];
#pragma unroll
        for (int q = 0; q < PB; ++q) {
          x[q] = y2[pos[p0 + q]];
          v[q] = ld_stream<1>(v1 + pos[p0 + q]);
          m[q] = TWO ? ld_stream<1>(v2 + pos[p0 + q]) : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int q = 0; q < PB; ++q) {
          const int p = p0 + q;
          x[q].x = x[q].x - v[q].x * a;
          x[q].y = x[q].y - v[q].y * a;
          if (TWO) {
            x[q].x = x[q].x - m[q].x * bp;
            x[q].y = x[q].y - m[q].y * bp;
          }
          if (!ok[p]) x[q] = make_double2(0.0, 0.0);  // so the clamped duplicates add nothing to the dots
          w[p] = x[q];
          ww = fma(x[q].x, x[q].x, ww);
          ww = fma(x[q].y, x[q].y, ww);
          d1 = fma(v[q].x, x[q].x, d1);
          d1 = fma(v[q].y, x[q].y, d1);
          tx[p] = tx[p] + c1 * v[q].x;
          ty[p] = ty[p] + c1 * v[q].y;
          if (TWO) {
            d2 = fma(m[q].x, x[q].x, d2);
            d2 = fma(m[q].y, x[q].y, d2);
            tx[p] = tx[p] + c2 * m[q].x;
            ty[p] = ty[p] + c2 * m[q].y;
          }
        }
        __builtin_amdgcn_sched_barrier(0);  // (keeps the next batch's loads behind this batch's arithmetic)
      }
    };
    if (two)  // block-uniform
      batches(std::true_type());
    else
      batches(std::false_type());
    ww = wave_sum(ww);
    d1 = wave_sum(d1);
    d2 = wave_sum(d2);
    if (lane == 0) {
      keep[wv * ldp + j + 1] = ww;
      keep[wv * ldp + j - 1] = d1;
      if (two) keep[wv * ldp + j - 2] = d2;
    }
  } else {
#pragma unroll
    for (int p = 0; p < P; ++p) {
      if (MODE == 0) {
        w[p] = reinterpret_cast<const double2*>(r)[pos[p]];
        w[p].x = w[p].x / b;
        w[p].y = w[p].y / b;
      } else {
        w[p] = out[pos[p]];
      }
      if (!ok[p]) w[p] = make_double2(0.0, 0.0);  // so the clamped duplicates add nothing to the dots
    }
  }
  const int jw = MODE == 2 ? (j >= 2 ? j - 2 : 0) : j;  // rows the walk covers
  for (int k = 0; k < jw; k += RU) {
    double2 q[RU][P];
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (k + u < jw) {  // block-uniform
        const double2* row = V2 + (int64_t)(k + u) * ld2;
#pragma unroll
        for (int p = 0; p < P; ++p) q[u][p] = ld_stream<1>(row + pos[p]);
      }
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (k + u < jw) {
        const double ck = coef[k + u];
        double d = 0.0;
#pragma unroll
        for (int p = 0; p < P; ++p) {
          tx[p] = tx[p] + ck * q[u][p].x;
          ty[p] = ty[p] + ck * q[u][p].y;
          if (MODE != 1) {
            d = fma(q[u][p].x, w[p].x, d);
            d = fma(q[u][p].y, w[p].y, d);
          }
        }
        if (MODE != 1) {
          d = wave_sum(d);
          if (lane == 0) keep[wv * ldp + k + u] = d;
        }
      }
  }
  double vv = 0.0;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    double2 o;
    if (MODE != 1) {
      tx[p] = tx[p] + cs * w[p].x;  // row j (u itself) is the last term of the sum, as in k_update_slice
      ty[p] = ty[p] + cs * w[p].y;
      o = make_double2(2.0 * w[p].x - tx[p], 2.0 * w[p].y - ty[p]);
    } else {
      o = make_double2(w[p].x - tx[p], w[p].y - ty[p]);
    }
    if (ok[p]) {
      st_stream<1>(out + pos[p], o);
      vv = fma(o.x, o.x, vv);
      vv = fma(o.y, o.y, vv);
    }
  }
  if (MODE == 1) return;
  vv = wave_sum(vv);
  if (lane == 0) keep[wv * ldp + j] = vv;
  __syncthreads();
  double* mine = part + (int64_t)blockIdx.x * ldp;
  const int nout = MODE == 2 ? j + 2 : j + 1;  // fused form: one more slot, ||w||^2
  for (int i = threadIdx.x; i < nout; i += kTPB)
    __builtin_nontemporal_store(((keep[i] + keep[ldp + i]) + keep[2 * ldp + i]) + keep[3 * ldp + i], mine + i);
}

// positions per lane: k_update_slice's choice (the P whose block count spreads most evenly over the CUs, ties to the larger
// P; 16 loads in flight per lane), and one position per lane for short vectors
static int os_sweep_p(int64_t n2) {
  if (n2 <= 16384) return 1;
  for (int cand : {16, 8, 4, 2}) {
    const int64_t G = (n2 + (int64_t)kTPB * cand - 1) / ((int64_t)kTPB * cand);
    const double g = (double)G / kNumCU;
    if (g / std::ceil(g) >= 0.93) return cand;
  }
  double best = -1.0;
  int P = 2;
  for (int cand : {16, 8, 4, 2}) {
    const int64_t G = (n2 + (int64_t)kTPB * cand - 1) / ((int64_t)kTPB * cand);
    const double g = (double)G / kNumCU, bal = g / std::ceil(g);
    if (bal > best) {
      best = bal;
      P = cand;
    }
  }
  return P;
}

int os_sweep_blocks(int64_t len) {
  const int64_t n2 = len >> 1;
  const int P = os_sweep_p(n2);
  return (int)((n2 + (int64_t)kTPB * P - 1) / ((int64_t)kTPB * P));
}

int launch_os_sweep(int mode, double* V, int64_t ldv, int64_t len, int j, const double* coef, const double* r, const double* nrm2,
                    double* beta_slot, double* part, const int* gate, hipStream_t s, double* dst, const double* alpha_prev,
                    const double* beta_prev) {
  const int64_t n2 = len >> 1;
  const int P = os_sweep_p(n2);
  const int grid = (int)((n2 + (int64_t)kTPB * P - 1) / ((int64_t)kTPB * P));
  const int ldp = qtw_ldp(mode == 2 ? j + 2 : j + 1);
  const size_t lds = mode != 1 ? (size_t)(kTPB / 64) * ldp * sizeof(double) : 0;
  if (!dst) dst = V + (int64_t)j * ldv;
#define LZ_OS_ARGS V, ldv, n2, j, coef, r, nrm2, beta_slot, ldp, part, gate, dst, alpha_prev, beta_prev
#define LZ_OS_GO(PP, RR)                                                                                       \
  do {                                                                                                         \
    if (mode == 0)                                                                                             \
      hipLaunchKernelGGL((k_os_sweep<PP, RR, 0>), dim3(grid), dim3(kTPB), lds, s, LZ_OS_ARGS);                 \
    else if (mode == 2)                                                                                        \
      hipLaunchKernelGGL((k_os_sweep<PP, RR, 2>), dim3(grid), dim3(kTPB), lds, s, LZ_OS_ARGS);                 \
    else                                                                                                       \
      hipLaunchKernelGGL((k_os_sweep<PP, RR, 1>), dim3(grid), dim3(kTPB), lds, s, LZ_OS_ARGS);                 \
  } while (0)
  switch (P) {
    case 16: LZ_OS_GO(16, 1); break;
    case 8: LZ_OS_GO(8, 2); break;
    case 4: LZ_OS_GO(4, 4); break;
    case 2: LZ_OS_GO(2, 8); break;
    default: LZ_OS_GO(1, 16); break;
  }
#undef LZ_OS_GO
#undef LZ_OS_ARGS
  return grid;
}

// The one-block kernels' O(j^2) sums, spread over the lanes of a wave: wave `wv` of `nw` takes coefficients wv * CB + q (q < CB), then
// nw * CB further on; lane t adds the terms l = t, t + 64, ... of each in that order, a fixed shuffle tree adds the lanes (reruns are
// bit-identical).  Both operands of a coefficient are contiguous in l (G is symmetric and stored both ways, a column of H is
// contiguous): coalesced loads, the CB coefficients' loads of a trip independent of each other.  f(i, sum) runs in lane 0.
constexpr int kOsCB = 4;
template <class RowA, class VecB, class Len, class F>
__device__ __forceinline__ void os_wave_dots(int count, RowA rowa, VecB vecb, Len len, F f) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int i0 = wv * kOsCB; i0 < count; i0 += nw * kOsCB) {
    double acc[kOsCB];
    const double* ra[kOsCB];
    int m = 0;
#pragma unroll
    for (int q = 0; q < kOsCB; ++q) {
      const int i = i0 + q < count ? i0 + q : count - 1;  // (a clamped duplicate: computed, not stored)
      acc[q] = 0.0;
      ra[q] = rowa(i);
      m = max(m, len(i));
    }
#pragma unroll 4
    for (int l = lane; l < m; l += 64) {
      const double b = vecb(l);
#pragma unroll
      for (int q = 0; q < kOsCB; ++q) {
        const int i = i0 + q < count ? i0 + q : count - 1;
        acc[q] = fma(l < len(i) ? ra[q][l] : 0.0, b, acc[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < kOsCB; ++q) {
      const double t = wave_sum(acc[q]);
      if (lane == 0 && i0 + q < count) f(i0 + q, t);
    }
  }
}

// k_os_post: one block.  max |e| is a max (order-free); every other sum is a fixed tree (os_wave_dots).  FUSED: the sweep worked in the
// units of w - d holds [V_i . w (i < j), u~ . u~, ||w||^2], chat the un-normalised predictions; both are divided by b = sqrt(||w||^2)
// here, the self term is cs = 1, nrm2[0] = ||w||^2 is left for the SpMV that scales u~, and the correction's coefficients for u~
// (b g_i) go to g[n ..].
template <bool FUSED>
__global__ __launch_bounds__(kFinalThreads) void k_os_post(const double* __restrict__ d, const double* __restrict__ chat, double* __restrict__ G,
                                                          double* __restrict__ H, int n, int j, double* __restrict__ nrm2, double tau,
                                                          double* __restrict__ g, int* __restrict__ ist, double* __restrict__ elog) {
  extern __shared__ double smem[];  // col [j + 1], the applied coefficients [j], the measured dots [j]
  double* col = smem;
  double* sc = col + (j + 1);
  double* sd = sc + (j + 1);
  __shared__ double smax[kFinalThreads / 64];
  __shared__ int s_trip;
  const double s2 = FUSED ? d[j + 1] : nrm2[0];
  const double b = sqrt(s2), cs = FUSED ? 1.0 : s2 / (b * b);
  double em = 0.0;
  for (int i = threadIdx.x; i < j; i += blockDim.x) {
    const double di = FUSED ? d[i] / b : d[i], ci = FUSED ? chat[i] / b : chat[i];
    const double e = fabs(di - ci);
    em = e == e ? fmax(em, e) : __builtin_inf();  // (a NaN leftover must trip the gate: fmax would drop it)
    sd[i] = di;
    sc[i] = ci;
  }
  if (threadIdx.x == 0) {
    col[j] = FUSED ? d[j] / s2 : d[j];
    if (FUSED) nrm2[0] = s2;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) em = fmax(em, __shfl_down(em, off, 64));
  if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = em;
  __syncthreads();
  // G[i, j] (i < j) of v_j = (2 - cs) u_j - sum_{l<j} c_l V_l: (2 - cs) d_i - sum_l c_l G[i, l]
  os_wave_dots(
      j, [&](int i) { return G + (int64_t)i * n; }, [&](int l) { return sc[l]; }, [&](int) { return j; },
      [&](int i, double t) { col[i] = (2.0 - cs) * sd[i] - t; });
  if (threadIdx.x == 0) {
    double m = 0.0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) m = fmax(m, smax[k]);
    const int trip = (j > 0 && !(m <= tau)) ? 1 : 0;
    s_trip = trip;
    elog[j] = m;
    ist[0] = trip;
    ist[1] += trip;
  }
  __syncthreads();
  const int trip = s_trip;
  if (trip) {
    // correction v_j -= sum_i g_i V_i with g = G[:j, j]: new G[i, j] = G[i, j] - sum_l G[i, l] g_l, new v.v from the old column
    for (int i = threadIdx.x; i < j; i += blockDim.x) g[i] = col[i];
    __syncthreads();
    os_wave_dots(
        j, [&](int i) { return G + (int64_t)i * n; }, [&](int l) { return g[l]; }, [&](int) { return j; },
        [&](int i, double t) {
          col[i] = g[i] - t;
          sd[i] = g[i] * (t - 2.0 * g[i]);  // this row's share of the change of v.v
        });
    __syncthreads();
    if (threadIdx.x == 0) {
      double vv = col[j];
      for (int i = 0; i < j; ++i) vv += sd[i];
      col[j] = vv;
    }
    if (FUSED)
      for (int i = threadIdx.x; i < j; i += blockDim.x) g[n + i] = b * g[i];  // the correction acts on u~ = b v_j
    __syncthreads();
  }
  for (int i = threadIdx.x; i <= j; i += blockDim.x) {
    G[(int64_t)j * n + i] = col[i];
    G[(int64_t)i * n + j] = col[i];
  }
  if (j > 0) {  // w_j = b / (2 - cs) (v_j + sum_{l<j} c_l V_l), c the applied coefficients: column j - 1 of H
    const double f = b / (2.0 - cs);
    double* hc = H + (int64_t)(j - 1) * n;
    for (int l = threadIdx.x; l < j; l += blockDim.x) {
      const double c = trip ? sc[l] + g[l] : sc[l];
      hc[l] = hc[l] + f * c;
    }
    if (threadIdx.x == 0) hc[j] = f;
  }
}

void launch_os_post(const double* d, const double* chat, double* G, double* H, int n, int j, double* nrm2, double tau, double* g, int* ist,
                    double* elog, bool fused, hipStream_t s) {
  const size_t lds = (size_t)3 * (j + 1) * sizeof(double);
  if (fused)
    hipLaunchKernelGGL(k_os_post<true>, dim3(1), dim3(kFinalThreads), lds, s, d, chat, G, H, n, j, nrm2, tau, g, ist, elog);
  else
    hipLaunchKernelGGL(k_os_post<false>, dim3(1), dim3(kFinalThreads), lds, s, d, chat, G, H, n, j, nrm2, tau, g, ist, elog);
}

// One block behind the SpMV (fused form: sum_out = alpha_j from the SpMV's partials) or behind the three-term kernel (sum_out =
// ||w_{j+1}||^2 from its partials), k_final_sum's grouping; then, when `predict`, the next step's predictions
//   c_hat_i = ((A V_i) . v_j - alpha_j G[i, j] - beta_j G[i, j-1]) / bn,  (A V_i) . v_j = sum_{l <= i+1} H[l, i] G[l, j]  (i < j),  alpha_j  (i = j)
// with bn = sqrt(||w_{j+1}||^2), or 1 in the fused form (whose sweep works in the units of w), and column j of H.
// predict == 2 (fused form only): the predictions alone - alpha_j is read from its slot, where a launch before this one has summed it
// (the group form's side stream), and part / sum_out are not touched.
template <bool FUSED>
__global__ __launch_bounds__(kFinalThreads) void k_os_sum_predict(const double* __restrict__ part, int np, double* __restrict__ sum_out,
                                                                 const double* __restrict__ G, double* __restrict__ H, int n, int j,
                                                                 const double* __restrict__ alpha_j, const double* __restrict__ beta_j,
                                                                 double* __restrict__ chat, int predict) {
  __shared__ double sm[kFinalThreads / 64];
  __shared__ double s_sum;
  if (predict == 2) {
    if (threadIdx.x == 0) s_sum = alpha_j[0];
  } else {
    const double t = final_sum_1024(part, np, sm);
    if (threadIdx.x == 0) {
      sum_out[0] = t;
      s_sum = t;
    }
  }
  if (!predict) return;
  __syncthreads();
  const double a = FUSED ? s_sum : alpha_j[0], bj = j > 0 ? beta_j[0] : 0.0, bn = FUSED ? 1.0 : sqrt(s_sum);
  const double* gj = G + (int64_t)j * n;
  const double* gm = G + (int64_t)(j > 0 ? j - 1 : 0) * n;
  auto finish = [&](int i, double s) {
    s = s - a * gj[i];
    if (j > 0) s = s - bj * gm[i];
    chat[i] = s / bn;
  };
  os_wave_dots(
      j, [&](int i) { return H + (int64_t)i * n; }, [&](int l) { return gj[l]; }, [&](int i) { return i + 2; }, finish);
  if (threadIdx.x == 0) finish(j, a);  // V_j . A v_j: the SpMV's own dot
  // column j of H: alpha_j on the diagonal, beta_j above it; k_os_post of step j + 1 adds the w_{j+1} terms
  double* hc = H + (int64_t)j * n;
  for (int l = threadIdx.x; l < n; l += blockDim.x) hc[l] = l == j ? a : (l == j - 1 ? bj : 0.0);
}

void launch_os_sum_predict(const double* part, int np, double* sum_out, const double* G, double* H, int n, int j, const double* alpha_j,
                           const double* beta_j, double* chat, bool fused, bool predict, hipStream_t s) {
  if (fused && !part)  // (the predictions alone)
    hipLaunchKernelGGL(k_os_sum_predict<true>, dim3(1), dim3(kFinalThreads), 0, s, part, 0, sum_out, G, H, n, j, alpha_j, beta_j, chat, 2);
  else if (fused)
    hipLaunchKernelGGL(k_os_sum_predict<true>, dim3(1), dim3(kFinalThreads), 0, s, part, np, sum_out, G, H, n, j, alpha_j, beta_j, chat, predict ? 1 : 0);
  else
    hipLaunchKernelGGL(k_os_sum_predict<false>, dim3(1), dim3(kFinalThreads), 0, s, part, np, sum_out, G, H, n, j, alpha_j, beta_j, chat, predict ? 1 : 0);
}

// ------------------------------------------------------------------ one-sweep loop, pair form: one walk per two steps
// (run_loop_one_sweep_pair, lz_loops.hip; the arithmetic is tools/one_sweep_prototype.py's one_sweep_pair_lanczos, name for name.)
// The speculative SpMV has left y° = A (w_j / b) and its alpha° partials.  The walk of step j applies only cn = c_hat / b = O(eps), so
// what it owes to w_{j+1} is a combination of basis rows: A (sum cn_i V_i) = sum_i cn_i sum_l H[l, i] V_l.
//
// k_os_pair_predict, one block: a0 = alpha° (stored as alpha_j); column j - 1 of H gets step j's applied coefficients (H[:j, j-1] += b cn,
// H[j, j-1] = b - known before the walk, because a pair applies the predictions and nothing else); then
//   mu = H[:j+1, :j] cn,   gp = [cn - G[:j, :j] cn, 1],   q = H[:j, :j]^T cn + H[j, :j],   vAv = a0 - 2 cn . q
//   p_i = sum_l H[l, i] gp_l - a0 gp_i - b G[i, j-1]  (i < j),   p_j = vAv - a0 gp_j - b gp_{j-1}      (the predictions V_i . w_{j+1})
//   kap = mu - a0 [cn, 0] + p                                     (what the walk subtracts from z to leave u~_{j+1})
// mu is a sum along ROWS of the column-major H: thread l of a chunk adds every nchunk-th column (coalesced in l), the chunks' sums are
// added in order.  Every other sum is os_wave_dots' fixed tree.
__global__ __launch_bounds__(kFinalThreads) void k_os_pair_predict(const double* __restrict__ part, int np, double* __restrict__ alpha_out,
                                                                  const double* __restrict__ nrm2, const double* __restrict__ chat,
                                                                  const double* __restrict__ G, double* __restrict__ H, int n, int j,
                                                                  double* __restrict__ kap, double* __restrict__ pout) {
  extern __shared__ double smem[];  // cn, gp, q, mu: j + 1 each; then the chunk sums of mu (kFinalThreads)
  double* cn = smem;
  double* gp = cn + (j + 1);
  double* q = gp + (j + 1);
  double* mu = q + (j + 1);
  double* red = mu + (j + 1);
  __shared__ double sm[kFinalThreads / 64];
  __shared__ double s_a0, s_cq;
  const double t0 = final_sum_1024(part, np, sm);
  if (threadIdx.x == 0) {
    alpha_out[0] = t0;
    s_a0 = t0;
  }
  const double b = sqrt(nrm2[0]);
  double* hc = H + (int64_t)(j - 1) * n;
  for (int i = threadIdx.x; i < j; i += blockDim.x) {
    const double ci = chat[i] / b;
    cn[i] = ci;
    hc[i] = hc[i] + b * ci;
  }
  if (threadIdx.x == 0) {
    hc[j] = b;
    cn[j] = 0.0;
    gp[j] = 1.0;
  }
  __syncthreads();
  const double a0 = s_a0;
  os_wave_dots(
      j, [&](int i) { return G + (int64_t)i * n; }, [&](int l) { return cn[l]; }, [&](int) { return j; },
      [&](int i, double t) { gp[i] = cn[i] - t; });
  os_wave_dots(
      j, [&](int i) { return (const double*)(H + (int64_t)i * n); }, [&](int l) { return cn[l]; }, [&](int i) { return min(i + 2, j); },
      [&](int i, double t) { q[i] = i == j - 1 ? t + b : t; });  // (H[j, i] is b at i = j - 1 and 0 before it)
  {
    const int Lp = (j + 1 + 63) & ~63, nchunk = kFinalThreads / Lp;  // j + 1 <= 1024 (os_pair_applies)
    const int l = threadIdx.x % Lp, ch = threadIdx.x / Lp;
    if (ch < nchunk) {
      double acc = 0.0;
      if (l <= j) {
        int i = ch;  // H[l, i] is 0 for i < l - 1: start at the first column of this chunk that is not
        if (i < l - 1) i += (l - 1 - i + nchunk - 1) / nchunk * nchunk;
        for (; i < j; i += nchunk) acc = fma(H[(int64_t)i * n + l], cn[i], acc);
      }
      red[ch * Lp + l] = acc;
    }
    __syncthreads();
    if (threadIdx.x <= j) {
      double m = 0.0;
      for (int c = 0; c < nchunk; ++c) m += red[c * Lp + threadIdx.x];
      mu[threadIdx.x] = m;
    }
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < j; i += 64) acc = fma(cn[i], q[i], acc);
    acc = wave_sum(acc);
    if (threadIdx.x == 0) s_cq = acc;
  }
  __syncthreads();
  const double* gm = G + (int64_t)(j - 1) * n;
  os_wave_dots(
      j, [&](int i) { return (const double*)(H + (int64_t)i * n); }, [&](int l) { return gp[l]; }, [&](int i) { return i + 2; },
      [&](int i, double t) {
        const double pi = (t - a0 * gp[i]) - b * gm[i];
        pout[i] = pi;
        kap[i] = (mu[i] - a0 * cn[i]) + pi;
      });
  if (threadIdx.x == 0) {
    const double vAv = a0 - 2.0 * s_cq;
    const double pj = (vAv - a0 * gp[j]) - b * gp[j - 1];
    pout[j] = pj;
    kap[j] = mu[j] + pj;
  }
}

void launch_os_pair_predict(const double* part, int np, double* alpha_out, const double* nrm2, const double* chat, const double* G, double* H,
                            int n, int j, double* kap, double* p, hipStream_t s) {
  const size_t lds = ((size_t)4 * (j + 1) + kFinalThreads) * sizeof(double);
  hipLaunchKernelGGL(k_os_pair_predict, dim3(1), dim3(kFinalThreads), lds, s, part, np, alpha_out, nrm2, chat, G, H, n, j, kap, p);
}

// The one walk of a pair (j >= 2), k_os_sweep's slice-owner shape with two vectors: w = w_j (wbuf, the three-term kernel's) and
//   z = (y° - a0 w / b) - b V[j-1]                        (the speculative three-term step; y° in ybuf, formed in the prologue)
// Row j - 1 is consumed in the prologue that loads it anyway, the walk covers rows 0 .. j-2: per row two running sums (c_hat against w,
// kap against z) and two dots from the same loads.  Epilogue: u~ = w - sum c_hat_i V_i, v_j = u~ / b -> V[j];
// u~_{j+1} = (z - sum kap_i V_i) - kap_j v_j -> ybuf, in place (each position is read and written by the same lane).
// Per wave in LDS, one run of 2 ldp doubles per block in part: [V_i . w (i < j), u~ . u~ | V_i . z (i < j), v_j . z, u~_{j+1} . u~_{j+1}].
// Positions are 32-bit (n2 < 2^30); out-of-range positions are clamped to a valid address and zeroed, so they add nothing.
template <int P, int RU>
__global__ __launch_bounds__(kTPB) void k_os_pair_sweep(const double* __restrict__ V, double* __restrict__ vj, int64_t ldv, int n2, int j,
                                                       const double* __restrict__ chat, const double* __restrict__ kap,
                                                       const double* __restrict__ wbuf, double* __restrict__ ybuf,
                                                       const double* __restrict__ nrm2, const double* __restrict__ alpha0, int ldp,
                                                       double* __restrict__ part) {
  extern __shared__ double keep[];  // [kTPB / 64][2 ldp]: this block's per-wave dots
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * (kTPB * P) + threadIdx.x;
  const int64_t ld2 = ldv >> 1;
  const double2* V2 = reinterpret_cast<const double2*>(V);
  double2* y2 = reinterpret_cast<double2*>(ybuf);
  double* kw = keep + wv * 2 * ldp;
  int pos[P];
  bool ok[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    ok[p] = base + (int64_t)p * kTPB < n2;
    pos[p] = ok[p] ? (int)(base + (int64_t)p * kTPB) : n2 - 1;  // valid address, result discarded
  }
  const double b = sqrt(nrm2[0]), a0 = alpha0[0];
  double2 w[P], z[P];
  double tx[P], ty[P], sx[P], sy[P];  // running sums: c_hat against w, kap against z
  {
    const double c1 = chat[j - 1], k1 = kap[j - 1];
    const double2* w2 = reinterpret_cast<const double2*>(wbuf);
    const double2* v1 = V2 + (int64_t)(j - 1) * ld2;
    double d1 = 0.0, d2 = 0.0;
    constexpr int PB = P < 8 ? P : 8;  // positions per batch: 3 PB loads in flight
#pragma unroll
    for (int p0 = 0; p0 < P; p0 += PB) {
      double2 x[PB], y[PB], m[PB];
#pragma unroll
      for (int q = 0; q < PB; ++q) {
        x[q] = w2[pos[p0 + q]];
        y[q] = y2[pos[p0 + q]];
        m[q] = ld_stream<1>(v1 + pos[p0 + q]);
      }
#pragma unroll
      for (int q = 0; q < PB; ++q) {
        const int p = p0 + q;
        double2 zz;
        zz.x = (y[q].x - a0 * (x[q].x / b)) - b * m[q].x;
        zz.y = (y[q].y - a0 * (x[q].y / b)) - b * m[q].y;
        if (!ok[p]) {  // so the clamped duplicates add nothing to the dots
          x[q] = make_double2(0.0, 0.0);
          zz = make_double2(0.0, 0.0);
        }
        w[p] = x[q];
        z[p] = zz;
        d1 = fma(m[q].x, x[q].x, d1);
        d1 = fma(m[q].y, x[q].y, d1);
        d2 = fma(m[q].x, zz.x, d2);
        d2 = fma(m[q].y, zz.y, d2);
        tx[p] = c1 * m[q].x;
        ty[p] = c1 * m[q].y;
        sx[p] = k1 * m[q].x;
        sy[p] = k1 * m[q].y;
      }
      __builtin_amdgcn_sched_barrier(0);  // (keeps the next batch's loads behind this batch's arithmetic)
    }
    d1 = wave_sum(d1);
    d2 = wave_sum(d2);
    if (lane == 0) {
      kw[j - 1] = d1;
      kw[ldp + j - 1] = d2;
    }
  }
  const int jw = j - 1;  // rows the walk covers
  for (int k = 0; k < jw; k += RU) {
    double2 q[RU][P];
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (k + u < jw) {  // block-uniform
        const double2* row = V2 + (int64_t)(k + u) * ld2;
#pragma unroll
        for (int p = 0; p < P; ++p) q[u][p] = ld_stream<1>(row + pos[p]);
      }
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (k + u < jw) {
        const double ck = chat[k + u], kk = kap[k + u];
        double d1 = 0.0, d2 = 0.0;
#pragma unroll
        for (int p = 0; p < P; ++p) {
          tx[p] = tx[p] + ck * q[u][p].x;
          ty[p] = ty[p] + ck * q[u][p].y;
          sx[p] = sx[p] + kk * q[u][p].x;
          sy[p] = sy[p] + kk * q[u][p].y;
          d1 = fma(q[u][p].x, w[p].x, d1);
          d1 = fma(q[u][p].y, w[p].y, d1);
          d2 = fma(q[u][p].x, z[p].x, d2);
          d2 = fma(q[u][p].y, z[p].y, d2);
        }
        d1 = wave_sum(d1);
        d2 = wave_sum(d2);
        if (lane == 0) {
          kw[k + u] = d1;
          kw[ldp + k + u] = d2;
        }
      }
  }
  const double kj = kap[j];
  double2* vo = reinterpret_cast<double2*>(vj);
  double uu = 0.0, vz = 0.0, uu2 = 0.0;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const double2 ut = make_double2(w[p].x - tx[p], w[p].y - ty[p]);
    const double2 v = make_double2(ut.x / b, ut.y / b);
    const double2 u2 = make_double2((z[p].x - sx[p]) - kj * v.x, (z[p].y - sy[p]) - kj * v.y);
    if (ok[p]) {
      st_stream<1>(vo + pos[p], v);
      y2[pos[p]] = u2;
      uu = fma(ut.x, ut.x, uu);
      uu = fma(ut.y, ut.y, uu);
      vz = fma(v.x, z[p].x, vz);
      vz = fma(v.y, z[p].y, vz);
      uu2 = fma(u2.x, u2.x, uu2);
      uu2 = fma(u2.y, u2.y, uu2);
    }
  }
  uu = wave_sum(uu);
  vz = wave_sum(vz);
  uu2 = wave_sum(uu2);
  if (lane == 0) {
    kw[j] = uu;
    kw[ldp + j] = vz;
    kw[ldp + j + 1] = uu2;
  }
  __syncthreads();
  double* mine = part + (int64_t)blockIdx.x * (2 * ldp);
  for (int i = threadIdx.x; i < 2 * ldp; i += kTPB) {
    const bool used = i < ldp ? i <= j : i - ldp <= j + 1;  // (the unused slots leave as zeros, not as whatever the LDS held)
    const double t = used ? ((keep[i] + keep[2 * ldp + i]) + keep[4 * ldp + i]) + keep[6 * ldp + i] : 0.0;
    __builtin_nontemporal_store(t, mine + i);
  }
}

// positions per lane of the pair walk: 8 (two waves per SIMD) or 16 (one wave) for long vectors - wide16 chooses -, else os_sweep_p's choice
static int os_pair_sweep_p(int64_t n2, bool wide16) {
  const int P = os_sweep_p(n2);
  return P >= 8 ? (wide16 ? 16 : 8) : P;
}
int os_pair_sweep_blocks(int64_t len, bool wide16) {
  const int64_t n2 = len >> 1;
  const int P = os_pair_sweep_p(n2, wide16);
  return (int)((n2 + (int64_t)kTPB * P - 1) / ((int64_t)kTPB * P));
}
int os_pair_ldp(int j) { return qtw_ldp(j + 2); }

int launch_os_pair_sweep(double* V, int64_t ldv, int64_t len, int j, const double* chat, const double* kap, const double* w, double* y,
                         const double* nrm2, const double* alpha0, double* part, bool wide16, hipStream_t s) {
  const int64_t n2 = len >> 1;
  const int P = os_pair_sweep_p(n2, wide16);
  const int grid = (int)((n2 + (int64_t)kTPB * P - 1) / ((int64_t)kTPB * P));
  const int ldp = os_pair_ldp(j);
  const size_t lds = (size_t)(kTPB / 64) * 2 * ldp * sizeof(double);
#define LZ_OSP_GO(PP, RR)                                                                                                                  \
  hipLaunchKernelGGL((k_os_pair_sweep<PP, RR>), dim3(grid), dim3(kTPB), lds, s, V, V + (int64_t)j * ldv, ldv, (int)n2, j, chat, kap, w, y, nrm2, \
                     alpha0, ldp, part)
  switch (P) {
    case 16: LZ_OSP_GO(16, 1); break;
    case 8: LZ_OSP_GO(8, 1); break;
    case 4: LZ_OSP_GO(4, 2); break;
    case 2: LZ_OSP_GO(2, 4); break;
    default: LZ_OSP_GO(1, 8); break;
  }
#undef LZ_OSP_GO
  return grid;
}

// k_os_pair_post, one block: d = the second-stage sums of the walk's two runs (run length ldp).  First step: dn = d1 / b against cn = c_hat / b
// (e1), G[:, j] = [dn - G[:j, :j] cn, u~ . u~ / ||w||^2].  Second step: b2 = sqrt(u~_{j+1} . u~_{j+1}) = beta_{j+1}, G[:j, j+1] =
// (d2 - G[:j, :j+1] kap) / b2, G[j, j+1] = (v_j . z - G[j, :j+1] kap) / b2, G[j+1, j+1] = 1, e2 = max |G[:j+1, j+1]|; column j of H =
// p + alpha_j e_j + b e_{j-1} + b2 e_{j+1}.  ||u~_{j+1}||^2 is left in nrm2[0] for the SpMV that scales it.  A pair has no correcting sweep: a
// leftover above tau (or a NaN) sets the sticky flag ist[3], and lz_run repeats the run on the single form.
__global__ __launch_bounds__(kFinalThreads) void k_os_pair_post(const double* __restrict__ d, int ldp, const double* __restrict__ chat,
                                                               const double* __restrict__ kap, const double* __restrict__ pin,
                                                               double* __restrict__ G, double* __restrict__ H, int n, int j,
                                                               double* __restrict__ nrm2, const double* __restrict__ alpha_j, double tau,
                                                               int* __restrict__ ist, double* __restrict__ elog) {
  extern __shared__ double smem[];  // cn, dn [j]; kp, colj, col2 [j + 1]
  double* cn = smem;
  double* dn = cn + j;
  double* kp = dn + j;
  double* colj = kp + (j + 1);
  double* col2 = colj + (j + 1);
  __shared__ double smax[2][kFinalThreads / 64];
  const double s2 = nrm2[0], b = sqrt(s2);
  const double uu = d[j], vz = d[ldp + j], uu2 = d[ldp + j + 1], b2 = sqrt(uu2), a0 = alpha_j[0];
  auto wave_max = [&](double em, double* dst) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) em = fmax(em, __shfl_down(em, off, 64));
    if ((threadIdx.x & 63) == 0) dst[threadIdx.x >> 6] = em;
  };
  double em = 0.0;
  for (int i = threadIdx.x; i < j; i += blockDim.x) {
    const double di = d[i] / b, ci = chat[i] / b;
    const double e = fabs(di - ci);
    em = e == e ? fmax(em, e) : __builtin_inf();  // (a NaN leftover must trip: fmax would drop it)
    dn[i] = di;
    cn[i] = ci;
    kp[i] = kap[i];
  }
  if (threadIdx.x == 0) {
    kp[j] = kap[j];
    colj[j] = uu / s2;
  }
  wave_max(em, smax[0]);
  __syncthreads();
  os_wave_dots(
      j, [&](int i) { return (const double*)(G + (int64_t)i * n); }, [&](int l) { return cn[l]; }, [&](int) { return j; },
      [&](int i, double t) { colj[i] = dn[i] - t; });
  __syncthreads();
  os_wave_dots(
      j, [&](int i) { return (const double*)(G + (int64_t)i * n); }, [&](int l) { return kp[l]; }, [&](int) { return j; },
      [&](int i, double t) { col2[i] = (d[ldp + i] - (t + colj[i] * kp[j])) / b2; });
  if (threadIdx.x < 64) {
    double acc = 0.0;
    for (int l = threadIdx.x; l < j; l += 64) acc = fma(colj[l], kp[l], acc);
    acc = wave_sum(acc);
    if (threadIdx.x == 0) col2[j] = (vz - (acc + colj[j] * kp[j])) / b2;
  }
  __syncthreads();
  em = 0.0;
  for (int i = threadIdx.x; i <= j; i += blockDim.x) {
    const double e = fabs(col2[i]);
    em = e == e ? fmax(em, e) : __builtin_inf();
  }
  wave_max(em, smax[1]);
  for (int i = threadIdx.x; i <= j; i += blockDim.x) {
    G[(int64_t)j * n + i] = colj[i];
    G[(int64_t)i * n + j] = colj[i];
    G[(int64_t)(j + 1) * n + i] = col2[i];
    G[(int64_t)i * n + j + 1] = col2[i];
  }
  double* hc = H + (int64_t)j * n;
  for (int l = threadIdx.x; l < n; l += blockDim.x) {
    double v = l <= j ? pin[l] : 0.0;
    if (l == j - 1) v = b + v;
    if (l == j) v = a0 + v;
    if (l == j + 1) v = b2;
    hc[l] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double m1 = 0.0, m2 = 0.0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) {
      m1 = fmax(m1, smax[0][k]);
      m2 = fmax(m2, smax[1][k]);
    }
    G[(int64_t)(j + 1) * n + j + 1] = 1.0;
    nrm2[0] = uu2;
    elog[j] = m1;
    elog[j + 1] = m2;
    if (!(m1 <= tau) || !(m2 <= tau) || !(b2 == b2)) ist[3] = 1;
  }
}

void launch_os_pair_post(const double* d, int ldp, const double* chat, const double* kap, const double* p, double* G, double* H, int n, int j,
                         double* nrm2, const double* alpha_j, double tau, int* ist, double* elog, hipStream_t s) {
  const size_t lds = ((size_t)2 * j + (size_t)3 * (j + 1)) * sizeof(double);
  hipLaunchKernelGGL(k_os_pair_post, dim3(1), dim3(kFinalThreads), lds, s, d, ldp, chat, kap, p, G, H, n, j, nrm2, alpha_j, tau, ist, elog);
}

// ------------------------------------------------------------------ one-sweep loop, group form: one walk per FOUR steps
// (run_loop_one_sweep_quad, lz_loops.hip; the arithmetic is tools/one_sweep_group_prototype.py's one_sweep_group_lanczos at m = 4, name for
// name.)  The chain has left x_0 .. x_2 in rows j .. j+2 of the basis, z = b_3 x_3 in a residual buffer, a_t in alpha[j + t], b_0 .. b_2 in
// their beta slots and the partials of ||z||^2 in part.
//
// k_os_quad_predict, one block: nrm2[0] = ||z||^2 (b_3 = its root), then the omega-recurrence over the extended set
// [V_0 .. V_{j-1}, x_0 .. x_3] with the full H: g_0[:j] = chat / b_0 and for t = 0, 1, 2
//   g_{t+1}[i] = ((sum_{l<j} H[l, i] g_t[l] (+ b_0 g_t[x_0] at i = j - 1) - a_t g_t[i]) - b_t g_{t-1}[i]) / b_{t+1}     (i < j; g_{-1} = G[:, j-1])
//   g_{t+1}[x_s] = (((b_{s+1} g_t[x_{s+1}] + a_s g_t[x_s]) + b_s g_t[x_{s-1}]) - a_t g_t[x_s]) - b_t g_{t-1}[x_s]) / b_{t+1}   (s < t)
//   g_{t+1}[x_t] = -b_t g_t[x_{t-1}] / b_{t+1}
// (the diagonal is 1, x_{-1} = V_{j-1}).  g_t goes to gout[t * ldg ..]: [0, j) the rows of the basis, j + s the in-group row x_s.
__global__ __launch_bounds__(kFinalThreads) void k_os_quad_predict(const double* __restrict__ part, int np, double* __restrict__ nrm2,
                                                                  const double* __restrict__ chat, const double* __restrict__ G,
                                                                  const double* __restrict__ H, int n, int j, const double* __restrict__ alpha,
                                                                  const double* __restrict__ beta, double* __restrict__ gout, int ldg) {
  extern __shared__ double smem[];  // g_0 .. g_3, j + 4 each
  const int L = j + 4;
  __shared__ double sm[kFinalThreads / 64];
  __shared__ double s_n;
  const double t0 = final_sum_1024(part, np, sm);
  if (threadIdx.x == 0) {
    nrm2[0] = t0;
    s_n = t0;
  }
  __syncthreads();
  const double b[4] = {beta[0], beta[1], beta[2], sqrt(s_n)};
  const double a[3] = {alpha[0], alpha[1], alpha[2]};
  for (int i = threadIdx.x; i < 4 * L; i += blockDim.x) smem[i] = i < j ? chat[i] / b[0] : 0.0;
  __syncthreads();
  const double* gm = G + (int64_t)(j - 1) * n;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const double* gt = smem + t * L;
    const double* gp = t ? smem + (t - 1) * L : gm;
    double* gn = smem + (t + 1) * L;
    os_wave_dots(
        j, [&](int i) { return H + (int64_t)i * n; }, [&](int l) { return gt[l]; }, [&](int i) { return min(i + 2, j); },
        [&](int i, double s) {
          if (i == j - 1) s = s + b[0] * (t ? gt[j] : 1.0);  // column j - 1 of the extended H has b_0 in row x_0
          gn[i] = ((s - a[t] * gt[i]) - b[t] * gp[i]) / b[t + 1];
        });
    if (threadIdx.x == 0) {
      for (int s = 0; s < t; ++s) {
        const double up = s + 1 == t ? 1.0 : gt[j + s + 1];
        const double lo = s ? gt[j + s - 1] : gt[j - 1];
        const double pv = s == t - 1 ? 1.0 : gp[j + s];
        gn[j + s] = ((((b[s + 1] * up + a[s] * gt[j + s]) + b[s] * lo) - a[t] * gt[j + s]) - b[t] * pv) / b[t + 1];
      }
      const double lo = t ? gt[j + t - 1] : gt[j - 1];
      gn[j + t] = -(b[t] * lo) / b[t + 1];
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < 4 * L; i += blockDim.x) gout[(i / L) * ldg + i % L] = smem[i];
}

void launch_os_quad_predict(const double* part, int np, double* nrm2, const double* chat, const double* G, const double* H, int n, int j,
                            const double* alpha, const double* beta, double* gout, int ldg, hipStream_t s) {
  const size_t lds = (size_t)4 * (j + 4) * sizeof(double);
  hipLaunchKernelGGL(k_os_quad_predict, dim3(1), dim3(kFinalThreads), lds, s, part, np, nrm2, chat, G, H, n, j, alpha, beta, gout, ldg);
}

// The NV (a power of two, <= 32) lane partials of a trip, added over the wave JOINTLY: a halving butterfly - at every stage a lane keeps
// one half of its values and hands the other half to the lane `off` away - until one value per lane is left, then a plain butterfly over
// the lanes that hold the same value.  NV - 1 + log2(64 / NV) shuffle-adds where NV trees take 6 NV; the tree is fixed (reruns are
// bit-identical).  Returns the sum of value quad_slot(lane), valid in the lanes with quad_writer(lane).
template <int NV>
__device__ __forceinline__ double quad_joint_sum(double (&v)[NV], int lane) {
  int off = 32;
#pragma unroll
  for (int cnt = NV; cnt > 1; cnt >>= 1, off >>= 1) {
    const bool hi = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < cnt / 2; ++i) {
      const double send = hi ? v[i] : v[i + cnt / 2];
      const double mine = hi ? v[i + cnt / 2] : v[i];
      v[i] = mine + __shfl_xor(send, off, 64);
    }
  }
#pragma unroll
  for (; off > 0; off >>= 1) v[0] = v[0] + __shfl_xor(v[0], off, 64);
  return v[0];
}
template <int NV>
__device__ __forceinline__ int quad_slot(int lane) {  // which of the NV values this lane ends up with
  int idx = 0, off = 32;
#pragma unroll
  for (int cnt = NV; cnt > 1; cnt >>= 1, off >>= 1)
    if (lane & off) idx += cnt / 2;
  return idx;
}
template <int NV>
__device__ __forceinline__ bool quad_writer(int lane) { return (lane & (64 / NV - 1)) == 0; }

// The one walk of a group (j >= 2): k_os_pair_sweep's slice-owner shape with FOUR vectors, x_0 .. x_2 = rows j .. j+2 as the chain left
// them and x_3 = z / b_3 (zbuf; b_3 = sqrt(nrm2[0])).  Every row 0 .. j-1 is loaded once: four running sums (g_t against the row) and four
// dots (the row against x_t) per position.  The 4 RU lane partials of a trip are added jointly (quad_joint_sum).  Epilogue:
// r_t = x_t - sum_i g_t[i] V_i, v_{j+t} = r_t - sum_{s<t} g_t[x_s] v_{j+s} -> rows j .. j+3 (each position is read and written by the same
// lane), and the dots v_{j+s} . x_t (s < t) and v_{j+t} . v_{j+t}.  Per wave in LDS, one run of 4 ldp doubles per block in part; run t:
// [V_i . x_t (i < j), v_{j+s} . x_t (s < t), v_{j+t} . v_{j+t}].  Positions are 32-bit (n2 < 2^30); out-of-range positions are clamped to a
// valid address and zeroed, so they add nothing (what they read may be mid-update: it is discarded).
template <int P, int RU>
__global__ __launch_bounds__(kTPB) void k_os_quad_sweep(double* __restrict__ V, int64_t ldv, int n2, int j, const double* __restrict__ g, int ldg,
                                                       const double* __restrict__ zbuf, const double* __restrict__ bz,
                                                       const double* __restrict__ nrm2, int ldp, double* __restrict__ part) {
  extern __shared__ double keep[];  // [kTPB / 64][4 ldp]: this block's per-wave dots
  constexpr int NV = 4 * RU;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * (kTPB * P) + threadIdx.x;
  const int64_t ld2 = ldv >> 1;
  double2* V2 = reinterpret_cast<double2*>(V);
  double* kw = keep + wv * 4 * ldp;
  int pos[P];
  bool ok[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    ok[p] = base + (int64_t)p * kTPB < n2;
    pos[p] = ok[p] ? (int)(base + (int64_t)p * kTPB) : n2 - 1;  // valid address, result discarded
  }
  const double b3 = sqrt(nrm2[0]);
  double2 x[4][P];
  double sx[4][P], sy[4][P];
  {
    // bz (the chain in the units of z): rows j .. j+3 hold the unscaled z_0 .. z_3 and bz[t] = b_t - x_t = z_t / b_t is formed here, by
    // the division the scaling SpMV did when it stored x_t; else rows j .. j+2 hold x_0 .. x_2 and zbuf holds z_3
    const double2* z2 = bz ? V2 + (int64_t)(j + 3) * ld2 : reinterpret_cast<const double2*>(zbuf);
    double bt[3] = {1.0, 1.0, 1.0};
    if (bz) {
#pragma unroll
      for (int t = 0; t < 3; ++t) bt[t] = bz[t];
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        x[t][p] = V2[(int64_t)(j + t) * ld2 + pos[p]];
        if (bz) x[t][p] = make_double2(x[t][p].x / bt[t], x[t][p].y / bt[t]);  // block-uniform
      }
      const double2 zz = z2[pos[p]];
      x[3][p] = make_double2(zz.x / b3, zz.y / b3);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (!ok[p]) x[t][p] = make_double2(0.0, 0.0);  // so the clamped duplicates add nothing to the dots
        sx[t][p] = 0.0;
        sy[t][p] = 0.0;
      }
    }
  }
  const int slot = quad_slot<NV>(lane), su = slot >> 2, st = slot & 3;
  const bool writer = quad_writer<NV>(lane);
  for (int k = 0; k < j; k += RU) {
    double2 q[RU][P];
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (k + u < j) {  // block-uniform
        const double2* row = V2 + (int64_t)(k + u) * ld2;
#pragma unroll
        for (int p = 0; p < P; ++p) q[u][p] = ld_stream<1>(row + pos[p]);
      }
    double d[NV];
#pragma unroll
    for (int u = 0; u < RU; ++u) {
#pragma unroll
      for (int t = 0; t < 4; ++t) d[u * 4 + t] = 0.0;
      if (k + u < j) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const double c = g[t * ldg + k + u];
          double dd = 0.0;
#pragma unroll
          for (int p = 0; p < P; ++p) {
            sx[t][p] = fma(c, q[u][p].x, sx[t][p]);  // (fused: the walk's arithmetic is a third shorter, the sums a rounding closer)
            sy[t][p] = fma(c, q[u][p].y, sy[t][p]);
            dd = fma(q[u][p].x, x[t][p].x, dd);
            dd = fma(q[u][p].y, x[t][p].y, dd);
          }
          d[u * 4 + t] = dd;
        }
      }
    }
    const double tot = quad_joint_sum<NV>(d, lane);
    if (writer && k + su < j) kw[st * ldp + k + su] = tot;
  }
  double gi[4][4];  // gi[t][s] = g_t[x_s], s < t
#pragma unroll
  for (int t = 1; t < 4; ++t)
#pragma unroll
    for (int s = 0; s < t; ++s) gi[t][s] = g[t * ldg + j + s];
  double mm[4][4], vv[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    vv[t] = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) mm[t][s] = 0.0;
  }
#pragma unroll
  for (int p = 0; p < P; ++p) {
    double2 v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      v[t] = make_double2(x[t][p].x - sx[t][p], x[t][p].y - sy[t][p]);
#pragma unroll
      for (int s = 0; s < t; ++s) {
        v[t].x = v[t].x - gi[t][s] * v[s].x;
        v[t].y = v[t].y - gi[t][s] * v[s].y;
      }
    }
    if (ok[p]) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        st_stream<1>(V2 + (int64_t)(j + t) * ld2 + pos[p], v[t]);
        vv[t] = fma(v[t].x, v[t].x, vv[t]);
        vv[t] = fma(v[t].y, v[t].y, vv[t]);
#pragma unroll
        for (int s = 0; s < t; ++s) {
          mm[t][s] = fma(v[s].x, x[t][p].x, mm[t][s]);
          mm[t][s] = fma(v[s].y, x[t][p].y, mm[t][s]);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const double a = wave_sum(vv[t]);
    if (lane == 0) kw[t * ldp + j + t] = a;
#pragma unroll
    for (int s = 0; s < t; ++s) {
      const double m = wave_sum(mm[t][s]);
      if (lane == 0) kw[t * ldp + j + s] = m;
    }
  }
  __syncthreads();
  double* mine = part + (int64_t)blockIdx.x * (4 * ldp);
  for (int i = threadIdx.x; i < 4 * ldp; i += kTPB) {
    const bool used = i % ldp <= j + i / ldp;  // (the unused slots leave as zeros, not as whatever the LDS held)
    const double t = used ? ((keep[i] + keep[4 * ldp + i]) + keep[8 * ldp + i]) + keep[12 * ldp + i] : 0.0;
    __builtin_nontemporal_store(t, mine + i);
  }
}

// positions per lane of the group walk: 4 (two waves per SIMD) or 8 (one wave) for long vectors - wide8 chooses -, else os_sweep_p's choice
static int os_quad_sweep_p(int64_t n2, bool wide8) {
  const int P = os_sweep_p(n2);
  return P >= 8 ? (wide8 ? 8 : 4) : P;
}
int os_quad_sweep_blocks(int64_t len, bool wide8) {
  const int64_t n2 = len >> 1;
  const int P = os_quad_sweep_p(n2, wide8);
  return (int)((n2 + (int64_t)kTPB * P - 1) / ((int64_t)kTPB * P));
}
int os_quad_ldp(int j) { return qtw_ldp(j + 4); }

int launch_os_quad_sweep(double* V, int64_t ldv, int64_t len, int j, const double* g, int ldg, const double* z, const double* bz, const double* nrm2,
                         double* part, bool wide8, hipStream_t s) {
  const int64_t n2 = len >> 1;
  const int P = os_quad_sweep_p(n2, wide8);
  const int grid = (int)((n2 + (int64_t)kTPB * P - 1) / ((int64_t)kTPB * P));
  const int ldp = os_quad_ldp(j);
  const size_t lds = os_quad_lds_bytes(ldp);  // <= kOneSweepQuadLds (os_quad_max_ldp): within what a kernel may ask for by default
#define LZ_OSQ_GO(PP, RR) \
  hipLaunchKernelGGL((k_os_quad_sweep<PP, RR>), dim3(grid), dim3(kTPB), lds, s, V, ldv, (int)n2, j, g, ldg, z, bz, nrm2, ldp, part)
  switch (P) {
    case 8: LZ_OSQ_GO(8, 1); break;
    case 4: LZ_OSQ_GO(4, 2); break;
    case 2: LZ_OSQ_GO(2, 4); break;
    default: LZ_OSQ_GO(1, 4); break;  // (eight rows a trip are 32 partials to add jointly: that instantiation spills)
  }
#undef LZ_OSQ_GO
  return grid;
}

// k_os_quad_post, one block: d = the second-stage sums of the walk's four runs (run length ldp), gin the predictions.  Leftovers:
// e_old = max |d_t[i] - g_t[i]| (i < j), e_in = max |v_{j+s} . x_t - g_t[x_s]|.  With C_t = [g_t, 1] the coefficients of x_t in the
// finished basis, the new columns of G: G[i, j+t] = d_t[i] - sum_{r<j+t} G[i, r] C_t[r] - the sums over the old columns by os_wave_dots, the
// in-group columns (kept in LDS until all four are done) added one t after the other -, G[j+t, j+t] = v_{j+t} . v_{j+t}; and of H:
// H[:, j-1] += b_0 C_0, H[:, j+t] = ((b_{t+1} C_{t+1} + a_t C_t) + b_t C_{t-1}) - sum_{r<j+t} C_t[r] H[:, r] for t < 3 (b_0 e_{j-1} in place
// of b_0 C_{-1}); the sums along the rows of the old columns of H are k_os_pair_predict's mu (chunks added in order).  beta[3] = b_3.
// A group has no correcting sweep: a leftover above tau (or a NaN) sets the sticky flag ist[4], and lz_run repeats the run on the pair form.
__global__ __launch_bounds__(kFinalThreads) void k_os_quad_post(const double* __restrict__ d, int ldp, const double* __restrict__ gin, int ldg,
                                                               double* __restrict__ G, double* __restrict__ H, int n, int j,
                                                               const double* __restrict__ nrm2, const double* __restrict__ alpha,
                                                               double* __restrict__ beta, double tau, int* __restrict__ ist,
                                                               double* __restrict__ elog) {
  extern __shared__ double smem[];  // C_0 .. C_3, the new columns of G, the new columns of H: 4 x L each; the chunk sums (kFinalThreads)
  const int L = j + 6;
  double* C = smem;
  double* col = C + 4 * L;
  double* hn = col + 4 * L;  // hn[0]: column j - 1, hn[1 + t]: column j + t (t < 3)
  double* red = hn + 4 * L;
  __shared__ double smax[2][kFinalThreads / 64];
  __shared__ double s_in[6];
  const double b[4] = {beta[0], beta[1], beta[2], sqrt(nrm2[0])};
  const double a[3] = {alpha[0], alpha[1], alpha[2]};
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  auto wave_max = [&](double em, double* dst) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) em = fmax(em, __shfl_down(em, off, 64));
    if (lane == 0) dst[wv] = em;
  };
  double e_old = 0.0, e_in = 0.0;
  for (int i = threadIdx.x; i < 4 * L; i += blockDim.x) {
    const int t = i / L, r = i % L;
    double c = 0.0;
    if (r < j + t) {
      c = gin[t * ldg + r];
      const double e = fabs(d[t * ldp + r] - c);
      if (r < j)
        e_old = e == e ? fmax(e_old, e) : __builtin_inf();  // (a NaN leftover must trip: fmax would drop it)
      else
        e_in = e == e ? fmax(e_in, e) : __builtin_inf();
    } else if (r == j + t) {
      c = 1.0;
    }
    C[i] = c;
    col[i] = 0.0;
    hn[i] = 0.0;
  }
  wave_max(e_old, smax[0]);
  wave_max(e_in, smax[1]);
  __syncthreads();
  // ---- G: the sums over the old columns, then the in-group terms
#pragma unroll 1
  for (int t = 0; t < 4; ++t) {
    const double* Ct = C + t * L;
    double* ct = col + t * L;
    os_wave_dots(
        j, [&](int i) { return (const double*)(G + (int64_t)i * n); }, [&](int l) { return Ct[l]; }, [&](int) { return j; },
        [&](int i, double s) { ct[i] = d[t * ldp + i] - s; });
  }
  __syncthreads();
#pragma unroll 1
  for (int t = 0; t < 4; ++t) {
    const double* Ct = C + t * L;
    double* ct = col + t * L;
    for (int i = threadIdx.x; i < j; i += blockDim.x) {
      double v = ct[i];
      for (int s = 0; s < t; ++s) v = v - col[s * L + i] * Ct[j + s];
      ct[i] = v;
    }
    if (wv < t) {  // row j + s of the old columns is column s of this group: sum_{r<j} G[j+s, r] C_t[r], one wave per s
      const double* cs = col + wv * L;
      double acc = 0.0;
      for (int l = lane; l < j; l += 64) acc = fma(cs[l], Ct[l], acc);
      acc = wave_sum(acc);
      if (lane == 0) s_in[wv] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int s = 0; s < t; ++s) {
        double v = d[t * ldp + j + s] - s_in[s];
        for (int q = 0; q < t; ++q) v = v - col[max(s, q) * L + j + min(s, q)] * Ct[j + q];  // G[j+s, j+q] of the columns already done
        ct[j + s] = v;
      }
      ct[j + t] = d[t * ldp + j + t];
    }
    __syncthreads();
  }
  // ---- H: hn[1 + t][l] starts as sum_{r<j-1} H[l, r] C_t[r] (l < j)
  {
    const int Lp = (j + 63) & ~63, nchunk = kFinalThreads / Lp;  // j <= 512 (os_quad_max_ldp)
    const int l = threadIdx.x % Lp, ch = threadIdx.x / Lp;
#pragma unroll 1
    for (int t = 0; t < 3; ++t) {
      const double* Ct = C + t * L;
      if (ch < nchunk) {
        double acc = 0.0;
        if (l < j) {
          int i = ch;  // H[l, i] is 0 for i < l - 1: start at the first column of this chunk that is not
          if (i < l - 1) i += (l - 1 - i + nchunk - 1) / nchunk * nchunk;
          for (; i < j - 1; i += nchunk) acc = fma(H[(int64_t)i * n + l], Ct[i], acc);
        }
        red[ch * Lp + l] = acc;
      }
      __syncthreads();
      if (threadIdx.x < j) {
        double m = 0.0;
        for (int c = 0; c < nchunk; ++c) m += red[c * Lp + threadIdx.x];
        hn[(1 + t) * L + threadIdx.x] = m;
      }
      __syncthreads();
    }
  }
  {
    const double* hc = H + (int64_t)(j - 1) * n;
    for (int l = threadIdx.x; l <= j; l += blockDim.x) hn[l] = l < j ? hc[l] + b[0] * C[l] : b[0];
  }
  __syncthreads();
#pragma unroll 1
  for (int t = 0; t < 3; ++t) {
    const double* Ct = C + t * L;
    const double* Cn = C + (t + 1) * L;
    double* ht = hn + (1 + t) * L;
    for (int l = threadIdx.x; l <= j + t + 1; l += blockDim.x) {
      double sub = ht[l] + Ct[j - 1] * hn[l];  // (hn[0][l] is 0 behind row j, ht[l] behind row j - 1)
      for (int s = 0; s < t; ++s) sub = sub + Ct[j + s] * hn[(1 + s) * L + l];
      const double last = t ? b[t] * C[(t - 1) * L + l] : (l == j - 1 ? b[0] : 0.0);
      ht[l] = ((b[t + 1] * Cn[l] + a[t] * Ct[l]) + last) - sub;
    }
    __syncthreads();
  }
  // ---- out
  for (int i = threadIdx.x; i < 4 * L; i += blockDim.x) {
    const int t = i / L, r = i % L;
    if (r <= j + t) {
      G[(int64_t)(j + t) * n + r] = col[i];
      G[(int64_t)r * n + j + t] = col[i];
    }
  }
  for (int l = threadIdx.x; l <= j; l += blockDim.x) H[(int64_t)(j - 1) * n + l] = hn[l];
  for (int i = threadIdx.x; i < 3 * n; i += blockDim.x) {
    const int t = i / n, l = i % n;
    H[(int64_t)(j + t) * n + l] = l <= j + t + 1 ? hn[(1 + t) * L + l] : 0.0;
  }
  if (threadIdx.x == 0) {
    double m1 = 0.0, m2 = 0.0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) {
      m1 = fmax(m1, smax[0][k]);
      m2 = fmax(m2, smax[1][k]);
    }
    beta[3] = b[3];
    const double m = fmax(m1, m2);
    for (int t = 0; t < 4; ++t) elog[j + t] = m;
    if (!(m1 <= tau) || !(m2 <= tau) || !(b[3] == b[3])) ist[4] = 1;
  }
}

hipError_t launch_os_quad_post(const double* d, int ldp, const double* g, int ldg, double* G, double* H, int n, int j, const double* nrm2,
                               const double* alpha, double* beta, double tau, int* ist, double* elog, hipStream_t s) {
  const size_t lds = ((size_t)12 * (j + 6) + kFinalThreads) * sizeof(double);
  // the kernel's static LDS counts against the same 64 KiB: past it the per-kernel limit has to be raised, as launch_spmv_rect does
  if (lds + 1024 > 65536) {
    const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_os_quad_post), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
  }
  hipLaunchKernelGGL(k_os_quad_post, dim3(1), dim3(kFinalThreads), lds, s, d, ldp, g, ldg, G, H, n, j, nrm2, alpha, beta, tau, ist, elog);
  return hipSuccess;
}

}  // namespace lz
