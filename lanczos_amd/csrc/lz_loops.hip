// The Krylov loops of lz_run: the individual steps, the six- / five- / three-launch loops, the one-reduce loop, the partial
// re-orthogonalisation loops (host-decided and device-resident), loop selection, the run frame (RunFrame) that lz_run, lz_run_resume and
// lz_run_resume_partial share, lz_get_residual / lz_reserve.
#include "lz_context.h"

using namespace lz;
using namespace lz::api;

namespace lz {
namespace api {

// ---- the loops' common idioms --------------------------------------------------------------------------------------------
inline double* basis_row(lz_handle h, int j) { return h->d_V + (int64_t)j * h->ldv; }
// where step j of an n-step run parks the norm that forms V[j]: beta[j-1], with Python's negative index at j = 0
inline int beta_index(int n, int j) { return (j + n - 2) % (n - 1); }
inline double* beta_slot(lz_handle h, int n, int j) { return h->d_beta + beta_index(n, j); }
// profile sampling (tune[7]): the centred sample of every stride - same mean j as the full run
inline bool iter_sampled(lz_handle h, int j) {
  const int pstride = h->tune[7] > 1 ? h->tune[7] : 1;
  return (j % pstride) == pstride / 2;
}
inline void begin_iter(lz_handle h, int j) { h->prof_iter = iter_sampled(h, j); }

// ---- the individual steps (device-resident scalars, no host sync) --------
int ensure_part(lz_handle h, size_t need) {
  if (need <= h->part_cap) return LZ_OK;
  LZ_TRY(dev_alloc(h, h->d_part, need));
  h->part_cap = need;
  return LZ_OK;
}

double spmv_bytes(lz_handle h, bool ell) {
  // (a row-class coded ELL copy: one class byte per row, the values only when they are not part of the class, x once, y)
  if (h->kind == 1 && h->csr.ell_coded && (ell || (h->csr.ell_default && ell_usable(h->csr, h->flags))))
    return 17.0 * h->rows + (h->csr.ell_coded == 1 ? 8.0 * h->csr.nnz : 0.0) + (h->csr.ell_coded == 3 ? 8.0 * h->rows : 0.0);  // (3: + the diagonal)
  if (h->kind == 1) return 12.0 * h->csr.nnz + 4.0 * (h->rows + 1) + 16.0 * h->rows;
  return 8.0 * (double)h->rows * (double)h->Mg + 8.0 * (double)h->Mg + 8.0 * h->rows;  // A block, x once, y
}
double spmv_flops(lz_handle h) { return h->kind == 1 ? 2.0 * h->csr.nnz : 2.0 * (double)h->rows * (double)h->Mg; }

// dst[0] = the sum of the np block partials a kernel left in d_part (this rank's share of a dot product)
static int step_final_sum(lz_handle h, int np, double* dst, const char* what) {
  Scope sc(h, LZ_K_FINAL, 0, 0);
  launch_final_sum(h->d_part, np, dst, h->stream);
  return check_launch(h, what);
}

// r = A V[j]; alpha_dst[0] = V[j] . r, summed over ranks unless reduce == false (one-reduce mode: the partial sum rides
// in the next all-reduce)
int step_spmv(lz_handle h, int j, double* alpha_dst, bool reduce, int* np_out) {
  if (!alpha_dst) alpha_dst = h->d_alpha + j;
  const double* x = nullptr;
  if (h->halo_inflight_j == j) {  // exchange already issued on the comm stream behind the boundary update
    LZ_HIP(h, hipStreamWaitEvent(h->stream, h->e_halo, 0));
    x = basis_row(h, j);
    h->halo_inflight_j = -1;
  } else {
    LZ_TRY(comm_exchange_x(h, j, &x));
  }
  const double* xown = basis_row(h, j);
  int np = 0;
  {
    Scope sc(h, LZ_K_SPMV, spmv_bytes(h), spmv_flops(h));
    if (h->kind == 1)
      np = launch_spmv_csr(h->csr, x, h->d_r, xown, h->d_part, h->flags, h->stream);
    else
      np = launch_gemv_dense(h->d_dense, h->rows, h->ncols_ext, h->dense_lda, x, xown, h->d_r, h->d_part, h->stream);
    LZ_TRY(check_launch(h, "spmv"));
  }
  if (np_out) {  // fused small-problem mode: the consumer kernel adds the block partials itself
    *np_out = np;
    return LZ_OK;
  }
  LZ_TRY(step_final_sum(h, np, alpha_dst, "final_sum(alpha)"));
  return reduce ? comm_allreduce(h, alpha_dst, 1) : LZ_OK;
}

// V[j] = r / sqrt(nrm2) (if scale), then c = V[0:nrows] . V[j]; V[j] = 2 V[j] - c^T V[0:nrows]
int step_reorth(lz_handle h, int j, int nrows, bool scale, int beta_idx, bool in_run_loop) {
  const double M = (double)h->rows;
  // fused-norm mode (the Python layers default to it): the reduced sums are [V_i . r (i < j), r . r] - one all-reduce at N > 1 -; beta and the scaling by
  // 1/beta are applied afterwards.  Only valid for the in-loop call shape (row j is the newest row).
  const bool fused = scale && (h->flags & LZ_FLAG_FUSED_NORM) && !(h->flags & LZ_FLAG_REORTH_PARTIAL) && nrows == j + 1;
  h->qplan.variant = h->tune[1];  // A/B knob may change between launches on one handle (same allocation for every arm)
  {
    Scope sc(h, LZ_K_QTW, 8.0 * (nrows - 1) * M + (scale && !fused ? 16.0 : 8.0) * M, 2.0 * nrows * M);
    LZ_HIP(h, launch_qtw(h->d_V, h->ldv, h->rows_pad, nrows, j, scale ? h->d_r : nullptr, h->d_nrm2, h->d_beta + beta_idx, h->qplan,
                         h->d_part, fused ? 2 : (scale ? 1 : 0), h->stream));
    LZ_TRY(check_launch(h, "qtw"));
  }
  {
    Scope sc(h, LZ_K_FINAL, 0, 0);
    launch_final_rows(h->d_part, nrows, h->qplan.P, h->d_c, h->stream, h->qplan.family == 2);
    LZ_TRY(check_launch(h, "final_rows"));
  }
  LZ_TRY(comm_allreduce(h, h->d_c, nrows));
  const bool overlap = in_run_loop && (h->flags & LZ_FLAG_OVERLAP_HALO) && h->xmode == 1 && h->all_contig && h->comm_kind == 1 &&
                       !h->peers.empty() && (h->world > 1 || h->tune[6]);
  // inside lz_run the default (slice-owner) update kernel turns the reduced sums into beta and the coefficients itself
  const bool raw_c = fused && in_run_loop && (h->tune[8] == 0 || h->tune[8] >= 3);
  if (fused && !raw_c) {
    Scope sc(h, LZ_K_FINAL, 0, 0);
    launch_fused_prepare(h->d_c, j, h->d_beta + beta_idx, h->stream);
    LZ_TRY(check_launch(h, "fused_prepare"));
  }
  if (!overlap) {
    Scope sc(h, LZ_K_UPDATE, 8.0 * (nrows - 1) * M + 16.0 * M, 2.0 * nrows * M);
    launch_update(h->d_V, h->ldv, h->rows_pad, nrows, j, h->d_c, fused ? h->d_r : nullptr, h->d_beta + beta_idx, h->tune[8], h->stream, 0, -1,
                  raw_c ? 1 : 0);
    LZ_TRY(check_launch(h, "update"));
    return LZ_OK;
  }
  // 1. boundary positions (the faces the neighbours need), 2. their exchange on the comm stream, 3. interior
  double* vj = basis_row(h, j);
  {
    Scope sc(h, LZ_K_UPDATE, 8.0 * (nrows - 1) * M + 16.0 * M, 2.0 * nrows * M);
    // both faces leave in ONE launch of the small-range kernel (the face kernel is a latency chain over the rows)
    const bool small = h->tune[8] == 0;
    for (size_t q = 0; q < h->bnd_ranges.size(); q += 2) {
      const auto& ra = h->bnd_ranges[q];
      const bool pair = small && q + 1 < h->bnd_ranges.size() && ra.second - ra.first <= 16384 &&
                        h->bnd_ranges[q + 1].second - h->bnd_ranges[q + 1].first <= 16384;
      launch_update(h->d_V, h->ldv, h->rows_pad, nrows, j, h->d_c, fused ? h->d_r : nullptr, h->d_beta + beta_idx, h->tune[8], h->stream,
                    ra.first, ra.second, raw_c ? 1 : 0, pair ? h->bnd_ranges[q + 1].first : 0, pair ? h->bnd_ranges[q + 1].second : 0);
      if (!pair && q + 1 < h->bnd_ranges.size())
        launch_update(h->d_V, h->ldv, h->rows_pad, nrows, j, h->d_c, fused ? h->d_r : nullptr, h->d_beta + beta_idx, h->tune[8], h->stream,
                      h->bnd_ranges[q + 1].first, h->bnd_ranges[q + 1].second, raw_c ? 1 : 0);
    }
    LZ_TRY(check_launch(h, "update(boundary)"));
    LZ_HIP(h, hipEventRecord(h->e_bnd, h->stream));
    for (auto& rg : h->int_ranges)
      launch_update(h->d_V, h->ldv, h->rows_pad, nrows, j, h->d_c, fused ? h->d_r : nullptr, h->d_beta + beta_idx, h->tune[8], h->stream,
                    rg.first, rg.second, raw_c ? 1 : 0);
    LZ_TRY(check_launch(h, "update(interior)"));
  }
  LZ_HIP(h, hipStreamWaitEvent(h->cstream, h->e_bnd, 0));
  h->acc.bytes[LZ_K_COMM] += 8.0 * (h->total_send + h->total_recv);
  h->acc.launches[LZ_K_COMM] += 1;
  h->n_exchange += 1;
  LZ_NCCL(h, g_rccl.GroupStart());
  for (size_t p = 0; p < h->peers.size(); ++p) {
    if (h->scount[p] > 0)
      LZ_NCCL(h, g_rccl.Send(vj + h->sstart[p], (size_t)h->scount[p], ncclDouble, h->peers[p], h->comm, h->cstream));
    if (h->rcount[p] > 0)
      LZ_NCCL(h, g_rccl.Recv(vj + h->rows_pad + h->roff[p], (size_t)h->rcount[p], ncclDouble, h->peers[p], h->comm, h->cstream));
  }
  LZ_NCCL(h, g_rccl.GroupEnd());
  LZ_HIP(h, hipEventRecord(h->e_halo, h->cstream));
  h->halo_inflight_j = j;
  return LZ_OK;
}

// r = r - alpha V[j] - beta V[jm1]; d_nrm2[0] = sum over ranks of ||r||^2.  r: the residual buffer (nullptr: h->d_r); what: the launch's
// name in an error's text
int step_three_term(lz_handle h, int j, int jm1, const double* d_alpha, const double* d_beta, bool need_norm, int* np_out, double* r,
                    const char* what) {
  const double M = (double)h->rows;
  int np = 0;
  {
    Scope sc(h, LZ_K_THREE, (jm1 >= 0 ? 32.0 : 24.0) * M, (jm1 >= 0 ? 6.0 : 4.0) * M);
    np = launch_three_term(r ? r : h->d_r, basis_row(h, j), jm1 >= 0 ? basis_row(h, jm1) : nullptr, d_alpha, d_beta, h->rows_pad, h->d_part,
                           h->stream);
    LZ_TRY(check_launch(h, what));
  }
  if (np_out) *np_out = np;  // (the caller's own kernel adds the partials)
  if (!need_norm) return LZ_OK;  // fused-norm mode: ||r||^2 travels with the next Q^T r all-reduce
  LZ_TRY(step_final_sum(h, np, h->d_nrm2, "final_sum(nrm2)"));
  return comm_allreduce(h, h->d_nrm2, 1);
}

// warm-up (Lanczos.py:108-110): r = A v0; alpha0 = r.v0; r = r - alpha0 v0, ||r||^2 if need_norm
static int warm_up(lz_handle h, bool need_norm) {
  LZ_TRY(step_spmv(h, 0));
  return step_three_term(h, 0, -1, h->d_alpha, nullptr, need_norm);
}

// r = r - coef[0] v: the one-reduce loops' halves of the recurrence
static int step_two_term(lz_handle h, const double* v, const double* coef, const char* what) {
  Scope sc(h, LZ_K_THREE, 24.0 * (double)h->rows, 2.0 * (double)h->rows);
  launch_three_term(h->d_r, v, nullptr, coef, nullptr, h->rows_pad, h->d_part, h->stream);
  return check_launch(h, what);
}

// The scale-on-read SpMV (ELL copy): V[j] = src / sqrt(nrm2[0]) wherever it reads x, beta -> its slot, dst = A V[j]; the alpha partials
// stay in d_part, *np of them.  src and dst are the two residual buffers, never the same one (it reads src through its gathers).
// gate: the kernel scales where gate[0] == 0 - the partial loop's sweep gate (a swept step's V[j] is in place), or a word that stays 0.
static int step_scaling_spmv(lz_handle h, int n, int j, const double* src, double* dst, const int* gate, int* np) {
  const double M = (double)h->rows;
  double* vj = basis_row(h, j);
  SpmvScale ss;
  ss.r = src;
  ss.nrm2 = h->d_nrm2;
  ss.vj = vj;
  ss.beta_slot = beta_slot(h, n, j);
  ss.gate = gate;
  // (the scale pass's 16M bytes ride here: BASELINE.md's accounting of the step is unchanged.  With a row-class coded matrix the
  // launch moves 25 bytes per row - r once, y, V[j], the class byte - so only V[j]'s 8 are added: counting r twice would be a
  // third of the total there)
  Scope sc(h, LZ_K_SPMV, spmv_bytes(h, true) + (h->csr.ell_coded ? 8.0 : 16.0) * M, spmv_flops(h) + M);
  *np = launch_spmv_ell(h->csr, vj, dst, vj, h->d_part, h->stream, &ss);
  return check_launch(h, "spmv(ell, scale fused)");
}

// The three-term recurrence in the prologue of step j's pass 1 (engines 2 and 3): r = (y - alpha v_{j-1}) - beta v_{j-2} -> d_r2.
// apart / np: the SpMV's alpha partials the prologue adds itself, or nullptr / 0: alpha is read from its slot.
static QtwFuse qtw_prologue_fuse(lz_handle h, int j, const double* apart, int np) {
  QtwFuse fz;
  fz.apart = apart;
  fz.np = np;
  fz.jprev = j > 0 ? j - 1 : 0;     // j == 0: the warm-up's alpha0 and r = A v0 - alpha0 v0 (Lanczos.py:109-110)
  fz.jprev2 = j >= 2 ? j - 2 : -1;  // the reference's V[-1] term at its step 0 is the zero row
  fz.beta_prev = h->d_beta + (j >= 2 ? j - 2 : 0);
  fz.alpha_out = h->d_alpha + fz.jprev;
  fz.r_out = h->d_r2;
  return fz;
}

// ---- one-reduce mode (LZ_FLAG_ONE_REDUCE): the whole Krylov loop with ONE all-reduce per iteration ---------------------
// State entering step j: r holds the two-term residual r'' = A u - beta v_{j-2} of the newest vector u = v_{j-1} (at j = 0:
// r'' = A v0, u = v0 in basis row 0), and the local partial of alpha = u.(A u) sits in the reduce buffer.  Step j:
//   pass 1 dots rows 0..j-1 against BOTH columns (r'', u) + the three self terms   -> one all-reduce with alpha
//   prepare: alpha = u.(A u) / u.u, c_i = V_i.r'' - alpha V_i.u, |r|^2 = r''.r'' - 2 alpha u.r'' + alpha^2 u.u; the beta of the
//            step before *= sqrt(u.u / the u.u before): the three-sum norm left u that far off unit length
//   r = r'' - alpha u;  update: beta = |r|, V[j] = 2 r/beta - sum c_i/beta V_i - ...   (unchanged kernels from here)
//   exchange V[j]; r = A V[j] (alpha partial into the buffer); r'' = r - beta V[j-1]
inline int onered_ldp(int m) { return qtw_ldp(m + 2); }
inline int onered_slot(int m) { return onered_ldp(m) + m + 2; }  // where alpha lives in the reduce buffer at a step with m rows

// The head of step j in both one-reduce loops (engines 6 and 8): pass 1 dots rows 0..j-1 against both columns (r'', u = row urow), the
// second stage adds the blocks' runs into buf - unless pass 1's last block does that itself (ticket: the folded form) -, and buf travels
// in THE all-reduce of the iteration.  part: where pass 1 leaves its partials.  gate == nullptr: the ungated form, its bytes counted
// here; with a gate the launches return at once where gate[0] == 0 and what really ran is accounted after the run (account_partial_device).
static int step_onereduce_head(lz_handle h, int j, int urow, double* part, double* buf, const int* gate, unsigned* ticket) {
  const double M = (double)h->rows;
  const int ldp = onered_ldp(j);
  QtwFuse fz;
  fz.gate = gate;
  if (ticket) {
    fz.ticket = ticket;
    fz.c_out = buf;
  }
  h->qplan.variant = 0;
  {
    Scope sc(h, LZ_K_QTW, gate ? 0.0 : 8.0 * j * M + 16.0 * M, gate ? 0.0 : 4.0 * (j + 1) * M);
    LZ_HIP(h, launch_qtw(h->d_V, h->ldv, h->rows_pad, j, urow, h->d_r, nullptr, nullptr, h->qplan, part, 3, h->stream, gate ? &fz : nullptr));
    LZ_TRY(check_launch(h, gate ? "qtw(two columns, gated)" : "qtw(two columns)"));
  }
  if (!ticket) {
    Scope sc(h, LZ_K_FINAL, 0, 0);
    launch_final_rows_t(part, h->qplan.G, 2 * ldp, ldp + j + 2, buf, h->stream, gate);
    LZ_TRY(check_launch(h, gate ? "final_rows(gated)" : "final_rows"));
  }
  return comm_allreduce(h, buf, onered_slot(j) + 1);
}

int run_loop_onereduce(lz_handle h, int n) {
  const double M = (double)h->rows;
  double* const uu_keep = h->d_beta + n;  // (d_beta has n + 1 doubles, the coefficients use n - 1) u.u of the step before
  LZ_TRY(step_spmv(h, 0, h->d_c + onered_slot(0), false));  // warm-up: r'' = A v0 (Lanczos.py:108), alpha0 partial
  for (int j = 0; j < n; ++j) {
    begin_iter(h, j);
    const int urow = j > 0 ? j - 1 : 0;
    LZ_TRY(step_onereduce_head(h, j, urow, h->d_part, h->d_c, nullptr, nullptr));
    {
      Scope sc(h, LZ_K_FINAL, 0, 0);
      // (j = 0: alpha[0] of the warm-up, rewritten below.  Step 0's beta has Python's index -1, the slot the last step rewrites:
      // the first beta that the next u.u corrects is step 1's)
      launch_onereduce_prepare(h->d_c, j, onered_ldp(j), h->d_alpha + urow, h->d_nrm2 + 1, j >= 2 ? beta_slot(h, n, j - 1) : nullptr, uu_keep,
                               h->stream);
      LZ_TRY(check_launch(h, "onereduce_prepare"));
    }
    LZ_TRY(step_two_term(h, basis_row(h, urow), h->d_alpha + urow, "three_term(alpha)"));  // r = r'' - alpha u
    {
      Scope sc(h, LZ_K_UPDATE, 8.0 * j * M + 16.0 * M, 2.0 * (j + 1) * M);
      launch_update(h->d_V, h->ldv, h->rows_pad, j + 1, j, h->d_c, h->d_r, beta_slot(h, n, j), h->tune[8] == 0 || h->tune[8] >= 3 ? h->tune[8] : 0,
                    h->stream, 0, -1, 1);
      LZ_TRY(check_launch(h, "update"));
    }
    const bool last = j == n - 1;
    LZ_TRY(step_spmv(h, j, h->d_c + onered_slot(last ? 0 : j + 1), false));
    // r'' = A V[j] - beta V[j-1]; at j = 0 the reference's V[-1] is the zero row
    if (!last && j > 0) LZ_TRY(step_two_term(h, basis_row(h, j - 1), beta_slot(h, n, j), "three_term(beta)"));
  }
  // The last alpha has no sweep to ride on: it travels with the self terms of a pass over no rows, whose u.u puts the last alpha and
  // the last beta on the length of the last vector (k_onereduce_prepare) - one all-reduce, as the lone alpha was
  LZ_TRY(step_onereduce_head(h, 0, n - 1, h->d_part, h->d_c, nullptr, nullptr));
  {
    Scope sc(h, LZ_K_FINAL, 0, 0);
    launch_onereduce_finish(h->d_c, onered_ldp(0), h->d_alpha + (n - 1), n >= 2 ? beta_slot(h, n, n - 1) : nullptr, uu_keep, h->stream);
    LZ_TRY(check_launch(h, "onereduce_finish"));
  }
  return LZ_OK;
}

// ---- small problems: three launches per step instead of six ---------------------------------------------------------------
// When a vector is a handful of pass-1 slices, every kernel of a step does microseconds of work and the step costs what
// its six dependent launches cost.  Here the two second-stage reductions and the three-term recurrence ride in the
// prologue of their consumer: [pass 1: alpha from the SpMV's block partials, r = (y - alpha v) - beta v', stage, dots]
// [pass 2: coefficients from pass 1's block partials, update] [SpMV].  Same arithmetic, same summation trees: bit-identical
// to the six-launch path (tests/test_gpu_small.py).
// one-reduce partial loop: where the self terms' (and pass 1's) partials start in d_part - behind the alpha partials of ANY SpMV plan
size_t onered_part_off(lz_handle h) {
  size_t np = std::max<size_t>((size_t)h->rows / 4 + 2, (size_t)std::max(h->csr.n_rowblk, 1));
  if (h->csr.pb) np = std::max<size_t>(np, (size_t)pb_num_partials(h->csr.pb));
  return (np + 64 + 63) / 64 * 64;
}

size_t fused_coff(lz_handle h) {  // where pass 1's partials start in d_part (behind the SpMV's alpha partials)
  const size_t npmax = std::max<size_t>((size_t)h->rows / 4 + 2, (size_t)std::max(h->csr.n_rowblk, 1)) + 64;
  return (npmax + 63) / 64 * 64;
}

int run_loop_fused_small(lz_handle h, int n) {
  const double M = (double)h->rows;
  const size_t coff = fused_coff(h);
  int np = 0;
  LZ_TRY(step_spmv(h, 0, nullptr, false, &np));  // warm-up: y = A v0 (Lanczos.py:108)
  for (int j = 0; j < n; ++j) {
    begin_iter(h, j);
    const QtwFuse fz = qtw_prologue_fuse(h, j, h->d_part, np);
    h->qplan.variant = 0;
    {
      Scope sc(h, LZ_K_QTW, 8.0 * j * M + 40.0 * M, 2.0 * (j + 1) * M + 4.0 * M);
      LZ_HIP(h, launch_qtw(h->d_V, h->ldv, h->rows_pad, j + 1, j, h->d_r, nullptr, nullptr, h->qplan, h->d_part + coff, 4, h->stream, &fz));
      LZ_TRY(check_launch(h, "qtw(fused three-term)"));
    }
    {
      Scope sc(h, LZ_K_UPDATE, 8.0 * j * M + 16.0 * M, 2.0 * (j + 1) * M);
      launch_update(h->d_V, h->ldv, h->rows_pad, j + 1, j, h->d_part + coff, h->d_r2, beta_slot(h, n, j), 0, h->stream, 0, -1, 2, 0, 0, h->qplan.G,
                    qtw_ldp(j + 1));
      LZ_TRY(check_launch(h, "update(fused reduction)"));
    }
    LZ_TRY(step_spmv(h, j, nullptr, false, &np));
  }
  LZ_TRY(step_final_sum(h, np, h->d_alpha + (n - 1), "final_sum(alpha)"));  // the last alpha has no consumer kernel to ride in
  h->r_state = 2;  // d_r holds y = A v_{n-1}: the recurrence rode in the next step's pass 1 (lz_get_residual forms r)
  return LZ_OK;
}


// The default loop of problems that are neither small nor huge (any number of ranks, fused-norm mode, full
// re-orthogonalisation, at most kThreeTermFusedMaxRows rows per rank - measured: C2 (10^6 rows) +3.6 %, 6 400 .. 350 000 rows
// +4 .. 11 %, the headline's 10^7 rows +0.4 %: there the separate three-term kernel streams at a higher rate than the
// prologue does, and the six-launch loop stays):
// the three-term recurrence r = (A v_j - alpha_j v_j) - beta_{j-1} v_{j-1} rides in the prologue of the NEXT step's pass 1
// (k_qtw_mfma4<4>, alpha read back from its slot after the all-reduce) instead of being a pass of its own - five launches
// per step, one read-modify-write of r less, bit-identical coefficients and basis (tests/test_gpu_small.py).
// lz_set_tuning(h, 15, 1) selects the six-launch loop.
constexpr int64_t kThreeTermFusedMaxRows = 4'000'000;
int run_loop_three_term_fused(lz_handle h, int n) {
  const double M = (double)h->rows;
  LZ_TRY(step_spmv(h, 0));  // warm-up: y = A v0, alpha_0 (Lanczos.py:108-109)
  for (int j = 0; j < n; ++j) {
    begin_iter(h, j);
    const QtwFuse fz = qtw_prologue_fuse(h, j, nullptr, 0);
    h->qplan.variant = 0;
    {
      Scope sc(h, LZ_K_QTW, 8.0 * j * M + 40.0 * M, 2.0 * (j + 1) * M + 4.0 * M);
      LZ_HIP(h, launch_qtw(h->d_V, h->ldv, h->rows_pad, j + 1, j, h->d_r, nullptr, nullptr, h->qplan, h->d_part, 4, h->stream, &fz));
      LZ_TRY(check_launch(h, "qtw(three-term in the prologue)"));
    }
    {
      Scope sc(h, LZ_K_FINAL, 0, 0);
      launch_final_rows(h->d_part, j + 1, h->qplan.P, h->d_c, h->stream, h->qplan.family == 2);
      LZ_TRY(check_launch(h, "final_rows"));
    }
    LZ_TRY(comm_allreduce(h, h->d_c, j + 1));
    {
      Scope sc(h, LZ_K_UPDATE, 8.0 * j * M + 16.0 * M, 2.0 * (j + 1) * M);
      launch_update(h->d_V, h->ldv, h->rows_pad, j + 1, j, h->d_c, h->d_r2, beta_slot(h, n, j), 0, h->stream, 0, -1, 1);
      LZ_TRY(check_launch(h, "update"));
    }
    LZ_TRY(step_spmv(h, j));
  }
  h->r_state = 2;  // as after run_loop_fused_small
  return LZ_OK;
}

#ifdef LZ_KBENCH
constexpr int kSmallStepMaxN = 64;  // per-step kernels: every block redoes both passes over all n rows
// ---- kernel-bench build only: the retired small-problem engines (lz_small.hip) ------------------------------------------
// The whole run as ONE cooperative kernel (tune[15] == 2; 3 = on a plain grid), or one launch per step (tune[15] == 5,
// n <= 64).  Both are bit-identical to the multi-kernel path and both measured no faster than the three launches per step
// that are the default for small problems (a device-coherent round trip costs ~2 us on MI355X, about
// what a kernel boundary costs), so they left the product library in round 3; tests/test_gpu_small.py keeps their
// bit-identity checks against liblanczos_kbench.so.
bool small_args(lz_handle h, int n, SmallArgs& sa) {
  memset(&sa, 0, sizeof sa);
  sa.kind = h->kind;
  if (h->kind == 2) {
    sa.dense = h->d_dense;
    sa.lda = h->dense_lda;
    sa.nparts = (int)((h->rows + 3) / 4);
  } else {
    const CsrDev& A = h->csr;
    const bool fixed = !(h->flags & LZ_FLAG_SPMV_STREAM) && (A.fixed_k == 5 || A.fixed_k == 7);
    // (one lane walks one row in the engine: rows of more than 32 entries would turn into a chain of dependent loads)
    // (the engine replays the CSR kernels' alpha grouping; a row-class coded copy of 5- / 7-entry rows groups alpha per 512-row unit
    // exactly like k_spmv_fixed<K, 512>, so it may stand in for the default SpMV)
    const bool ell_other_grouping = A.ell_default && !(A.ell_coded && fixed);
    if (A.pb || ell_other_grouping || A.max_row_nnz > 32 || (fixed && A.fixed_rb != 512)) return false;
    sa.rowptr = A.rowptr;
    sa.colidx = A.colidx;
    sa.vals = A.vals;
    sa.rowblk = fixed ? nullptr : A.rowblk;
    sa.nparts = fixed ? (int)((h->rows + 511) / 512) : A.n_rowblk;
  }
  if (sa.nparts > 1024 || h->part_cap < (size_t)(2048 + h->rows_pad)) return false;
  sa.rows = (int)h->rows;
  sa.rows_pad = (int)h->rows_pad;
  sa.n = n;
  sa.ldv = h->ldv;
  sa.V = h->d_V;
  sa.y = h->d_r;
  sa.drow = h->d_part;
  sa.x0 = h->d_part + 2048;  // d_part holds >= 4096 doubles; rows_pad <= 1280
  sa.pc = h->d_c;
  sa.alpha = h->d_alpha;
  sa.beta = h->d_beta;
  sa.bar = reinterpret_cast<unsigned*>(h->d_nrm2);  // 16 bytes, zeroed by basis_alloc
  sa.xcc = reinterpret_cast<unsigned*>(h->d_part + 3400);
  return true;
}
bool small_engine_applies(lz_handle h) {
  SmallArgs sa;
  return small_args(h, 2, sa);
}

int run_small_engine(lz_handle h, int n, const double* v0_local, bool steps, bool* ran) {
  SmallArgs sa;
  *ran = small_args(h, n, sa);
  if (!*ran) return LZ_OK;
  LZ_HIP(h, hipMemcpyAsync(h->d_part + 2048, h->d_V, (size_t)h->rows_pad * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  if (steps) {
    // one launch per step: first SpMV, steps j = -1 .. n-2, the last alpha
    const int nb = h->kind == 2 ? (int)std::min<int64_t>(256, (h->rows + 3) / 4) : (int)std::max<int64_t>(1, (h->rows + kTPB - 1) / kTPB);
    const double Mr = (double)h->rows;
    LZ_HIP(h, launch_small_step(sa, 0, -1, nb, h->stream));
    for (int j = -1; j <= n - 2; ++j) {
      const int pstride = h->tune[7] > 1 ? h->tune[7] : 1;
      h->prof_iter = ((j + 1) % pstride) == pstride / 2;
      Scope sc(h, LZ_K_UPDATE, spmv_bytes(h) + 16.0 * (j + 2) * Mr + 40.0 * Mr, spmv_flops(h) + 4.0 * (j + 2) * Mr);
      LZ_HIP(h, launch_small_step(sa, 1, j, nb, h->stream));
    }
    h->prof_iter = true;
    LZ_HIP(h, launch_small_step(sa, 2, n - 1, 1, h->stream));
    return check_launch(h, "small_step");
  }
  h->acc.launches[LZ_K_FINAL] += 1;
  // tune[15] == 2: the participating blocks share one XCD (every eighth block of the grid); 3: plain grid over all XCDs
  LZ_HIP(h, launch_small_run(sa, small_grid(sa.rows_pad), h->tune[15] == 2, h->stream));
  LZ_TRY(check_launch(h, "small_run"));
  unsigned status = 0;
  LZ_HIP(h, hipMemcpyAsync(&status, sa.bar + 2, sizeof status, hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  if (status != 0) {
    // the engine refused (its blocks were not dealt to one XCD) or a barrier timed out: the caller repeats the run
    if (getenv("LZ_DEBUG_TIMING")) fprintf(stderr, "[lz_run] small-problem engine gave up (status %u): multi-kernel path\n", status);
    *ran = false;
    LZ_TRY(basis_alloc(h, n, 1));
    LZ_HIP(h, hipMemcpyAsync(h->d_V, v0_local, (size_t)h->rows * sizeof(double), hipMemcpyHostToDevice, h->stream));
    LZ_HIP(h, hipEventRecord(h->run_a, h->stream));
  }
  return LZ_OK;
}
#endif  // LZ_KBENCH

// ---- one-sweep full re-orthogonalisation: ONE walk over the basis per step ------------------------------------------------
// The six-launch loop streams V twice per step (pass 1: c = V^T w, pass 2: v_j = 2 w/beta - sum c_i V_i), 16 j M bytes.  Here
// the coefficients are PREDICTED from G = V^T V and H (A V_i = sum_l H[l, i] V_l to rounding, A symmetric):
//   V_i . w_{j+1} = (A V_i) . v_j - alpha_j G[i, j] - beta_j G[i, j-1],  (A V_i) . v_j = sum_l H[l, i] G[l, j],  V_j . A v_j = alpha_j
// (k_os_predict, one block), applied by ONE sweep that also measures the true dots V_i . u_j from the same loads (k_os_sweep),
// and checked afterwards (k_os_post, one block): e = d - c_hat is, to rounding, how far v_j is from what the two-pass step
// would have formed, and G[:, j] follows from d, c_hat and the old G.  When max |e| > kOneSweepTau a correcting sweep
// v_j -= sum_i G[i, j] V_i runs before the SpMV (always enqueued, returns at once when the gate is 0), so the basis is never
// more than tau from orthogonal and every step's orthogonality is measured, not assumed.  8 j M + 40 M bytes per step
// (sweep 8 j M + 16 M, three-term 24 M) plus the SpMV.  The coefficients equal the two-pass loop's to rounding (not bit
// for bit: the dots that decide them are summed in another order, and ||w||^2 comes from the three-term kernel).
// One rank, fused-norm mode, full re-orthogonalisation, default kernels; lz_run_resume continues on the two-pass loop.
// Where the matrix has a scale-on-read SpMV the fused form below runs instead (lz_set_tuning(h, 15, 7): this one always).
struct OneSweepState {
  double *G, *H, *chat, *g, *elog, *gq;  // gq: the group form's predictions, 4 runs of n + 4
  double* zp;                            // the ||z||^2 partials of the group chain's three-term passes (kChainParts)
  double* b3;                            // b_3 of the group before, for the next group's opening pass while post is on the side stream
  int nb;
};
constexpr size_t kChainParts = 2048;  // (launch_three_term_z's grid limit)
// The main stream waits for what the side stream of the last group left to do (second-stage sums, post, the chat prediction): called
// immediately before the first launch, copy or memset on the main stream that touches G, H, chat, the flags, elog or d_c.
static int one_sweep_join(lz_handle h) {
  if (!h->os_side_pending) return LZ_OK;
  h->os_side_pending = false;
  LZ_HIP(h, hipStreamWaitEvent(h->stream, h->e_os_ready, 0));
  return LZ_OK;
}
// where the state of an n-step run lies in d_os
static void one_sweep_view(lz_handle h, int n, OneSweepState& st) {
  st.nb = os_sweep_blocks(h->rows_pad);
  st.G = h->d_os;
  st.H = st.G + (size_t)n * n;
  st.chat = st.H + (size_t)n * n;
  st.g = st.chat + n + 1;
  st.elog = st.g + 2 * n + 2;
  st.gq = st.elog + n + 1;
  st.zp = st.gq + (size_t)4 * (n + 4);
  st.b3 = st.zp + kChainParts;
}
static int one_sweep_setup(lz_handle h, int n, OneSweepState& st, int pair_blocks = 0) {
  const size_t os_doubles = (size_t)2 * n * n + (size_t)5 * n + 8 + (size_t)4 * (n + 4) + kChainParts + 8;
  LZ_TRY(one_sweep_join(h));  // (only behind a run that ended in an error: nothing of it may still be writing the state)
  if (!h->os_stream) {
    LZ_HIP(h, hipStreamCreateWithFlags(&h->os_stream, hipStreamNonBlocking));
    LZ_HIP(h, hipEventCreateWithFlags(&h->e_os_walk, hipEventDisableTiming));
    LZ_HIP(h, hipEventCreateWithFlags(&h->e_os_alpha, hipEventDisableTiming));
    LZ_HIP(h, hipEventCreateWithFlags(&h->e_os_ready, hipEventDisableTiming));
  }
  const size_t ospart = (size_t)(h->rows / kTPB) + 64;  // (the ELL products leave one alpha partial per block of kTPB rows or more)
  if (h->ospart_cap < ospart) {
    LZ_TRY(dev_alloc(h, h->d_ospart, ospart));
    h->ospart_cap = ospart;
  }
  if (h->os_n < n) {
    LZ_TRY(dev_alloc(h, h->d_os, os_doubles));
    LZ_TRY(dev_alloc(h, h->d_osi, 8));
    h->os_n = n;
  }
  h->os_step_n = 0;
  one_sweep_view(h, n, st);
  // (the pair walk leaves two runs per block, and its block count may differ from the single walk's)
  LZ_TRY(ensure_part(h, (size_t)std::max(st.nb, 2 * pair_blocks) * qtw_ldp(n + 1) + 64));
  LZ_HIP(h, hipMemsetAsync(h->d_os, 0, os_doubles * sizeof(double), h->stream));
  // [0] gate, [1] trips, [2] stays 0 (the fused SpMV's "scale" gate), [3] a pair's leftover exceeded tau, [4] a group's
  LZ_HIP(h, hipMemsetAsync(h->d_osi, 0, 8 * sizeof(int), h->stream));
  return LZ_OK;
}
// sweep (mode 0: units of u = w / beta, reads r and ||w||^2; mode 2: the fused form, see run_loop_one_sweep_fused), second-stage sums,
// post, gated correction of step j
static int one_sweep_step(lz_handle h, int n, int j, const OneSweepState& st, bool fused) {
  const double M = (double)h->rows;
  double* dst = fused ? h->d_r2 : basis_row(h, j);
  {
    Scope sc(h, LZ_K_UPDATE, 8.0 * j * M + 16.0 * M, 4.0 * (j + 1) * M);
    if (fused)  // w_j = (y - alpha_{j-1} v_{j-1}) - beta_{j-2} v_{j-2}: the beta that formed v_{j-1} sits at step j - 1's slot
      launch_os_sweep(2, h->d_V, h->ldv, h->rows_pad, j, st.chat, h->d_r, nullptr, nullptr, h->d_part, nullptr, h->stream, dst, h->d_alpha + (j - 1),
                      beta_slot(h, n, j - 1));
    else
      launch_os_sweep(0, h->d_V, h->ldv, h->rows_pad, j, st.chat, h->d_r, h->d_nrm2, beta_slot(h, n, j), h->d_part, nullptr, h->stream);
    LZ_TRY(check_launch(h, "one-sweep"));
  }
  {
    Scope sc(h, LZ_K_FINAL, 0, 0);
    const int nout = fused ? j + 2 : j + 1;
    launch_final_rows_t(h->d_part, st.nb, qtw_ldp(nout), nout, h->d_c, h->stream);
    LZ_TRY(check_launch(h, "final_rows(one-sweep)"));
    launch_os_post(h->d_c, st.chat, st.G, st.H, n, j, h->d_nrm2, kOneSweepTau, st.g, h->d_osi, st.elog, fused, h->stream);
    LZ_TRY(check_launch(h, "one-sweep post"));
  }
  {
    Scope sc(h, LZ_K_QTW, 0, 0);  // (bytes are not counted: the correction runs in almost no step)
    launch_os_sweep(1, h->d_V, h->ldv, h->rows_pad, j, fused ? st.g + n : st.g, nullptr, nullptr, nullptr, nullptr, h->d_osi, h->stream, dst);
    LZ_TRY(check_launch(h, "one-sweep correction"));
  }
  return LZ_OK;
}

int run_loop_one_sweep(lz_handle h, int n) {
  OneSweepState st;
  LZ_TRY(one_sweep_setup(h, n, st));
  LZ_TRY(warm_up(h, true));
  for (int j = 0; j < n; ++j) {
    begin_iter(h, j);
    LZ_TRY(one_sweep_step(h, n, j, st, false));
    LZ_TRY(step_spmv(h, j));
    // at j = 0 the reference subtracts beta * V[-1], the still-zero last row: a no-op
    int np = 0;
    LZ_TRY(step_three_term(h, j, j > 0 ? j - 1 : -1, h->d_alpha + j, beta_slot(h, n, j), false, &np));
    {  // ||w_{j+1}||^2 from the three-term kernel's partials and the next step's predictions, one launch
      Scope sc(h, LZ_K_FINAL, 0, 0);
      launch_os_sum_predict(h->d_part, np, h->d_nrm2, st.G, st.H, n, j, h->d_alpha + j, beta_slot(h, n, j), st.chat, false,
                            j + 1 < n, h->stream);
      LZ_TRY(check_launch(h, "final_sum(nrm2) + one-sweep predict"));
    }
  }
  h->r_state = 1;
  return LZ_OK;
}

// The one-sweep loop without the three-term pass (one rank, a matrix with a scale-on-read SpMV form: 5 or 7 entries per row, ELL
// ordered).  w_j = (A v_{j-1} - alpha_{j-1} v_{j-1}) - beta_{j-2} v_{j-2} reads two rows the sweep of step j walks anyway, so the sweep
// forms w itself from y = A v_{j-1} (k_os_sweep, mode 2) and measures ||w||^2 from the registers that hold it.  beta_j is then not
// known before the walk, so the step works in the units of w: the predictions c' are not divided by beta, the sweep leaves
// u~ = 2 w - (sum c'_i V_i + w) in the second residual buffer (self term exactly 1; the unfused form's ||w||^2 / beta^2 is 1 to an
// ulp), post divides the measured and the predicted dots by b = sqrt(||w||^2), and the SpMV forms v_j = u~ / b wherever it reads x,
// stores V[j], beta_j and y = A v_j (the partial loop's SC form, always scaling).  Its alpha partials are summed by the one-block
// kernel that predicts step j + 1.  Six launches per step instead of nine, 8 j M + 41 M bytes instead of 8 j M + 65 M with a
// row-class coded 5-point matrix.  Step 0 and the warm-up are the unfused form's; after the last step the three-term kernel runs
// once, so d_r, ||r||^2 and V hold what lz_get_residual / lz_run_resume expect.  Coefficients and basis equal the unfused form's to
// rounding (tests/test_gpu_one_sweep_fused.py).
bool one_sweep_fused_applies(lz_handle h, int n) {
  const bool one_rank = h->world == 1 && h->comm_kind == 0;
  return one_rank && h->kind == 1 && ell_usable(h->csr, h->flags) && (h->csr.fixed_k == 5 || h->csr.fixed_k == 7) && n <= kOneSweepFusedMaxN &&
         h->tune[15] != 7;
}
// one step of the fused form: sweep / post / gated correction, SpMV, alpha sum + the next step's predictions
static int one_sweep_fused_iter(lz_handle h, int n, int j, const OneSweepState& st) {
  double* vj = basis_row(h, j);
  LZ_TRY(one_sweep_join(h));  // (behind a group: its state)
  LZ_TRY(one_sweep_step(h, n, j, st, j > 0));
  int npa = 0;
  if (j == 0) {  // step 0 is the unfused form's: V[0] is in place, a plain SpMV
    Scope sc(h, LZ_K_SPMV, spmv_bytes(h), spmv_flops(h));
    npa = launch_spmv_csr(h->csr, vj, h->d_r, vj, h->d_part, h->flags, h->stream);
    LZ_TRY(check_launch(h, "spmv"));
  } else {
    LZ_TRY(step_scaling_spmv(h, n, j, h->d_r2, h->d_r, h->d_osi + 2, &npa));  // (d_osi[2] stays 0: always scale on read)
  }
  {  // alpha_j from the SpMV's partials and the next step's predictions, one launch
    Scope sc(h, LZ_K_FINAL, 0, 0);
    launch_os_sum_predict(h->d_part, npa, h->d_alpha + j, st.G, st.H, n, j, h->d_alpha + j, beta_slot(h, n, j), st.chat, true, j + 1 < n, h->stream);
    LZ_TRY(check_launch(h, "final_sum(alpha) + one-sweep predict"));
  }
  return LZ_OK;
}
// after the last step of the fused and the pair form: r = (A v_{n-1} - alpha_{n-1} v_{n-1}) - beta_{n-2} v_{n-2}, ||r||^2 - the
// residual entering step n
static int one_sweep_fused_tail(lz_handle h, int n) {
  LZ_TRY(one_sweep_join(h));  // (a run that ends on a group: beta_{n-1} is post's, and the run's end must be behind everything)
  LZ_TRY(step_three_term(h, n - 1, n - 2, h->d_alpha + (n - 1), beta_slot(h, n, n - 1), true));
  h->r_state = 1;
  return LZ_OK;
}
int run_loop_one_sweep_fused(lz_handle h, int n) {
  OneSweepState st;
  LZ_TRY(one_sweep_setup(h, n, st));
  h->last_os_fused = 1;
  LZ_TRY(warm_up(h, true));
  for (int j = 0; j < n; ++j) {
    begin_iter(h, j);
    LZ_TRY(one_sweep_fused_iter(h, n, j, st));
  }
  return one_sweep_fused_tail(h, n);
}

// The pair form of the fused loop: ONE walk over the basis per TWO steps.  A walk applies coefficients of size O(eps) and measures dots
// already predicted to O(eps), so the correction step j owes to w_{j+1} is itself a combination of basis rows, exact to O(eps^2):
// A (sum cn_i V_i) = sum_i cn_i sum_l H[l, i] V_l.  The SpMV therefore runs on the UNCORRECTED w_j / b (speculative; its dot is alpha_j,
// O(eps) from v_j . A v_j), and one walk finishes v_j and forms u~_{j+1}, with two coefficient vectors and two dot vectors from the same
// loads (k_os_pair_predict / k_os_pair_sweep / k_os_pair_post, lz_reorth.hip; tools/one_sweep_prototype.py, one_sweep_pair_lanczos).
// beta_{j+1} = ||u~_{j+1}||, O(eps^2) from ||w_{j+1}||.  Nine launches and 8 j M + 40 M bytes of walk per pair instead of twice
// 8 j M + 16 M.  Steps 0, 1 and an odd last step are the single fused form's.  A pair has no correcting sweep: a leftover above
// kOneSweepTau sets a sticky device flag, and lz_run repeats the run on the single form (and remembers it until the matrix is set again).
bool one_sweep_pair_applies(lz_handle h, int n) {
  const int knob = h->tune[15];
  return one_sweep_fused_applies(h, n) && knob != 6 && n >= 4 && qtw_ldp(n + 1) <= kOneSweepPairMaxLdp && !h->pair_tripped;
}
// one pair at steps j, j + 1 (2 <= j, j + 1 < n): three-term, speculative SpMV, predict, the pair walk, post, the closing SpMV
static int one_sweep_pair_iter(lz_handle h, int n, int j, const OneSweepState& st, int nbp, bool wide16) {
  const double M = (double)h->rows;
  double* kap = st.g;  // (the correcting sweep's coefficient buffers are free while a pair runs)
  double* pp = st.g + n + 1;
  const int* scale = h->d_osi + 2;  // (stays 0: the SpMVs always scale on read)
  h->prof_iter = iter_sampled(h, j) || iter_sampled(h, j + 1);
  LZ_TRY(one_sweep_join(h));  // (behind a group: its state)
  // w_j = (y - alpha_{j-1} v_{j-1}) - beta_{j-1} v_{j-2} -> d_r, ||w_j||^2 -> d_nrm2
  LZ_TRY(step_three_term(h, j - 1, j - 2, h->d_alpha + (j - 1), h->d_beta + (j - 2), true));
  int npa = 0;
  LZ_TRY(step_scaling_spmv(h, n, j, h->d_r, h->d_r2, scale, &npa));  // y° = A (w_j / b); the V[j] it stores is provisional
  const int ldp = os_pair_ldp(j);
  {
    Scope sc(h, LZ_K_FINAL, 0, 0);
    launch_os_pair_predict(h->d_part, npa, h->d_alpha + j, h->d_nrm2, st.chat, st.G, st.H, n, j, kap, pp, h->stream);
    LZ_TRY(check_launch(h, "one-sweep pair predict"));
  }
  {
    Scope sc(h, LZ_K_UPDATE, 8.0 * j * M + 40.0 * M, 8.0 * (j + 1) * M);
    launch_os_pair_sweep(h->d_V, h->ldv, h->rows_pad, j, st.chat, kap, h->d_r, h->d_r2, h->d_nrm2, h->d_alpha + j, h->d_part, wide16, h->stream);
    LZ_TRY(check_launch(h, "one-sweep pair walk"));
  }
  {
    Scope sc(h, LZ_K_FINAL, 0, 0);
    launch_final_rows_t(h->d_part, nbp, 2 * ldp, ldp + j + 2, h->d_c, h->stream);
    LZ_TRY(check_launch(h, "final_rows(one-sweep pair)"));
    launch_os_pair_post(h->d_c, ldp, st.chat, kap, pp, st.G, st.H, n, j, h->d_nrm2, h->d_alpha + j, kOneSweepTau, h->d_osi, st.elog, h->stream);
    LZ_TRY(check_launch(h, "one-sweep pair post"));
  }
  LZ_TRY(step_scaling_spmv(h, n, j + 1, h->d_r2, h->d_r, scale, &npa));  // V[j+1] = u~_{j+1} / beta_{j+1}, y = A V[j+1]
  {
    Scope sc(h, LZ_K_FINAL, 0, 0);
    launch_os_sum_predict(h->d_part, npa, h->d_alpha + (j + 1), st.G, st.H, n, j + 1, h->d_alpha + (j + 1), h->d_beta + j, st.chat, true,
                          j + 2 < n, h->stream);
    LZ_TRY(check_launch(h, "final_sum(alpha) + one-sweep predict"));
  }
  h->last_os_pairs += 1;
  return LZ_OK;
}
int run_loop_one_sweep_pair(lz_handle h, int n) {
  const bool wide16 = h->tune[15] == 9;  // (A/B: 16 positions per lane on long vectors)
  OneSweepState st;
  const int nbp = os_pair_sweep_blocks(h->rows_pad, wide16);
  LZ_TRY(one_sweep_setup(h, n, st, nbp));
  h->last_os_fused = 1;
  LZ_TRY(warm_up(h, true));
  for (int j = 0; j < n;) {
    if (j < 2 || j + 1 >= n) {
      begin_iter(h, j);
      LZ_TRY(one_sweep_fused_iter(h, n, j, st));
      j += 1;
      continue;
    }
    LZ_TRY(one_sweep_pair_iter(h, n, j, st, nbp, wide16));
    j += 2;
  }
  return one_sweep_fused_tail(h, n);
}

// The group form of the fused loop: ONE walk over the basis per FOUR steps (tools/one_sweep_group_prototype.py, one_sweep_group_lanczos at
// m = 4; k_os_quad_predict / k_os_quad_sweep / k_os_quad_post, lz_reorth.hip).  A group at step j (2 <= j, j + 4 <= n):
//   chain    three plain Lanczos steps with no walk - x_0 = w_j / b_0 and, for t < 3, y_t = A x_t, a_t = x_t . y_t,
//            z = (y_t - a_t x_t) - b_t x_{t-1}, b_{t+1} = ||z||, x_{t+1} = z / b_{t+1} - by the launches of a step that does not sweep: the
//            scaling SpMV (which stores x_t into row j + t), the alpha sum, k_three_term, the ||.||^2 sum.  alpha_{j+t} = a_t, beta = b_t.
//            That is knob 15 = 12; the default keeps the chain in the units of z (see one_sweep_quad_iter): the same steps on the unscaled
//            z_t in rows j .. j+3, three launches less and 8 M bytes less per product.
//   predict  the omega-recurrence over the extended set [V_0 .. V_{j-1}, x_0 .. x_3] with the full H: every dot of x_t against the rows
//            before it, to O(eps^2), from G, H, chat and the chain's scalars (one block; it also sums the last ||z||^2)
//   walk     rows 0 .. j-1 once, four running sums and four dots per position; its epilogue finishes v_j .. v_{j+3}
//   post     the leftovers against the gate, G[:, j .. j+3], H[:, j-1 .. j+2] (one block)
//   closing  the plain SpMV on the corrected V[j+3]; its alpha sum predicts the next chat as after any step
// With the unscaled chain the second-stage sums, post and the chat prediction run on a side stream (knob 15 = 13: on the main stream):
// nothing reads G, H, chat, the flags or elog before the next group's predict kernel, a chain of streaming kernels later (one_sweep_join).
// z differs from the two-pass loop's w_{j+t} by a vector of span(V_0 .. V_{j+t-1}) plus O(eps^2), and projecting that span out of either
// gives the same v_{j+t}: coefficients and basis equal the two-pass loop's to rounding.  8 j M + 64 M bytes of walk per group where two
// pair walks move 16 j M + 80 M.  Steps 0 and 1 are the single fused form's; a tail of two steps is a pair, a tail of one or three runs
// on the single fused form.  A group has no correcting sweep: a leftover above kOneSweepTau sets a sticky device flag, and lz_run repeats
// the run on the pair form (and remembers it until the matrix is set again).
bool one_sweep_quad_applies(lz_handle h, int n) {
  const int knob = h->tune[15];
  return one_sweep_pair_applies(h, n) && knob != 8 && knob != 9 && n >= 6 && os_quad_ldp(n - 4) <= os_quad_max_ldp() && !h->quad_tripped;
}
// one group at steps j .. j + 3 (2 <= j, j + 4 <= n): the chain, predict, the group walk, post, the closing SpMV
static int one_sweep_quad_iter(lz_handle h, int n, int j, const OneSweepState& st, int nbq, bool wide8) {
  const double M = (double)h->rows;
  const int ldg = n + 4;
  h->prof_iter = iter_sampled(h, j) || iter_sampled(h, j + 1) || iter_sampled(h, j + 2) || iter_sampled(h, j + 3);
  const bool zchain = h->tune[15] != 12;  // (12: the chain of scaled vectors through the scaling SpMV, 19 launches per group - A/B)
  // Behind the walk the second-stage sums, post and the chat prediction run on the side stream: nothing before the next group's predict
  // kernel reads what they leave (knob 15 = 13: on the main stream - A/B; the scaled chain reuses d_part at once and always keeps them there)
  const bool side = zchain && h->tune[15] != 13;
  if (!zchain) LZ_TRY(one_sweep_join(h));
  const double* z = nullptr;      // where z_3 lies
  const double* zpart = nullptr;  // the partials of ||z_3||^2
  int npz = 0;
  if (zchain) {
    // The chain in the units of z: rows j .. j+3 hold the unscaled z_0 .. z_3 until the walk finishes them, and x_t = z_t / b_t is formed by
    // division wherever a pass reads it (the bits the scaling SpMV stores).  z_0 = w_j goes straight into row j; step t: the plain coded
    // product y' = A z_t -> d_r with the partials of z_t . y', ONE launch for both sums (b_t = ||z_t||, a_t = z_t . y' / ||z_t||^2), then
    // z_{t+1} = (y' / b_t - a_t (z_t / b_t)) - b_t x_{t-1} -> row j + t + 1.  Three launches less than the scaled chain and 17 M bytes per
    // product instead of 25 M.
    // The products leave their partials in d_ospart: the side stream of the group before may still be adding up the walk's in d_part.
    // For the same reason the opening takes beta_{j-1} = b_3 of that group from st.b3 (the same bits post stores into the beta slot).
    const double* b_open = h->os_side_pending ? st.b3 : h->d_beta + (j - 2);
    auto three_term_z = [&](int mode, int t) {  // t = -1: the opening
      Scope sc(h, LZ_K_THREE, 32.0 * M, (mode == 0 ? 6.0 : mode == 1 ? 8.0 : 9.0) * M);
      npz = launch_three_term_z(mode, basis_row(h, j + t + 1), h->d_r, basis_row(h, j + t), basis_row(h, j + t - 1), h->d_alpha + (j + t),
                                mode == 0 ? b_open : h->d_beta + (j + t - 1), mode == 2 ? h->d_beta + (j + t - 2) : nullptr, h->rows_pad, st.zp,
                                h->stream);
      return check_launch(h, mode == 0 ? "three_term(chain opening)" : "three_term(chain)");
    };
    LZ_TRY(three_term_z(0, -1));
    for (int t = 0; t < 3; ++t) {
      double* zt = basis_row(h, j + t);
      int npa = 0;
      {
        Scope sc(h, LZ_K_SPMV, spmv_bytes(h, true), spmv_flops(h));
        npa = launch_spmv_ell(h->csr, zt, h->d_r, zt, h->d_ospart, h->stream);
        LZ_TRY(check_launch(h, "spmv(ell, chain)"));
      }
      {
        Scope sc(h, LZ_K_FINAL, 0, 0);
        launch_final_sum_chain(st.zp, npz, h->d_ospart, npa, h->d_beta + (j + t - 1), h->d_alpha + (j + t), h->stream);
        LZ_TRY(check_launch(h, "final_sum(chain)"));
      }
      LZ_TRY(three_term_z(t == 0 ? 1 : 2, t));  // the last ||z||^2 is summed by the predict kernel
    }
    z = basis_row(h, j + 3);
    zpart = st.zp;
  } else {
    // the chain: w_j -> d_r; then x_t = src / b_t -> V[j + t], y_t -> the other residual buffer, z in place there
    LZ_TRY(step_three_term(h, j - 1, j - 2, h->d_alpha + (j - 1), h->d_beta + (j - 2), true));
    double* src = h->d_r;
    double* dst = h->d_r2;
    for (int t = 0; t < 3; ++t) {
      int npa = 0;
      LZ_TRY(step_scaling_spmv(h, n, j + t, src, dst, h->d_osi + 2, &npa));  // (d_osi[2] stays 0: always scale on read)
      LZ_TRY(step_final_sum(h, npa, h->d_alpha + (j + t), "final_sum(alpha)"));
      // z = (y_t - a_t x_t) - b_t x_{t-1}; the last ||z||^2 is summed by the predict kernel
      LZ_TRY(step_three_term(h, j + t, j + t - 1, h->d_alpha + (j + t), h->d_beta + (j + t - 1), t < 2, &npz, dst));
      std::swap(src, dst);
    }
    z = src;  // (d_r2: three steps from d_r)
    zpart = h->d_part;
  }
  const int ldp = os_quad_ldp(j);
  LZ_TRY(one_sweep_join(h));  // the state of the group before: predict reads G, H and chat, the walk overwrites d_part
  {
    Scope sc(h, LZ_K_FINAL, 0, 0);
    launch_os_quad_predict(zpart, npz, h->d_nrm2, st.chat, st.G, st.H, n, j, h->d_alpha + j, h->d_beta + (j - 1), st.gq, ldg, h->stream);
    LZ_TRY(check_launch(h, "one-sweep group predict"));
  }
  {
    Scope sc(h, LZ_K_UPDATE, 8.0 * j * M + 64.0 * M, 16.0 * (j + 1) * M);
    launch_os_quad_sweep(h->d_V, h->ldv, h->rows_pad, j, st.gq, ldg, z, zchain ? h->d_beta + (j - 1) : nullptr, h->d_nrm2, h->d_part, wide8, h->stream);
    LZ_TRY(check_launch(h, "one-sweep group walk"));
  }
  hipStream_t ps = side ? h->os_stream : h->stream;  // where the second-stage sums and post run
  if (side) {
    LZ_HIP(h, hipEventRecord(h->e_os_walk, h->stream));
    LZ_HIP(h, hipStreamWaitEvent(h->os_stream, h->e_os_walk, 0));
    h->os_side_pending = true;  // (from here on: an error below leaves it set, and the next setup or read-back joins)
  }
  {
    Scope sc(h, LZ_K_FINAL, 0, 0, ps);
    launch_final_rows_t(h->d_part, nbq, 4 * ldp, 3 * ldp + j + 4, h->d_c, ps);
    LZ_TRY(check_launch(h, "final_rows(one-sweep group)"));
    LZ_HIP(h, launch_os_quad_post(h->d_c, ldp, st.gq, ldg, st.G, st.H, n, j, h->d_nrm2, h->d_alpha + j, h->d_beta + (j - 1), kOneSweepTau, h->d_osi,
                                  st.elog, ps));
    LZ_TRY(check_launch(h, "one-sweep group post"));
  }
  {  // closing: y = A V[j+3] -> d_r (V[j+3] is in place: the plain ELL product), alpha_{j+3} and the next chat
    double* vj = basis_row(h, j + 3);
    double* apart = zchain ? h->d_ospart : h->d_part;
    int npa = 0;
    {
      Scope sc(h, LZ_K_SPMV, spmv_bytes(h, true), spmv_flops(h));
      npa = launch_spmv_ell(h->csr, vj, h->d_r, vj, apart, h->stream);
      LZ_TRY(check_launch(h, "spmv(ell)"));
    }
    if (side) {
      {  // alpha_{j+3} on the main stream (the next opening pass reads it, and b_3), the chat prediction behind post on the side stream
        Scope sc(h, LZ_K_FINAL, 0, 0);
        launch_final_sum_root(apart, npa, h->d_alpha + (j + 3), h->d_nrm2, st.b3, h->stream);
        LZ_TRY(check_launch(h, "final_sum(alpha, b3)"));
      }
      LZ_HIP(h, hipEventRecord(h->e_os_alpha, h->stream));
      LZ_HIP(h, hipStreamWaitEvent(h->os_stream, h->e_os_alpha, 0));
      if (j + 4 < n) {
        Scope sc(h, LZ_K_FINAL, 0, 0, ps);
        launch_os_sum_predict(nullptr, 0, h->d_alpha + (j + 3), st.G, st.H, n, j + 3, h->d_alpha + (j + 3), h->d_beta + (j + 2), st.chat, true, true, ps);
        LZ_TRY(check_launch(h, "one-sweep predict(side)"));
      }
      LZ_HIP(h, hipEventRecord(h->e_os_ready, h->os_stream));
    } else {
      Scope sc(h, LZ_K_FINAL, 0, 0);
      launch_os_sum_predict(apart, npa, h->d_alpha + (j + 3), st.G, st.H, n, j + 3, h->d_alpha + (j + 3), h->d_beta + (j + 2), st.chat, true,
                            j + 4 < n, h->stream);
      LZ_TRY(check_launch(h, "final_sum(alpha) + one-sweep predict"));
    }
  }
  h->last_os_quads += 1;
  return LZ_OK;
}
int run_loop_one_sweep_quad(lz_handle h, int n) {
  const bool wide8 = h->tune[15] == 11;  // (A/B: 8 positions per lane on long vectors)
  OneSweepState st;
  const int nbp = os_pair_sweep_blocks(h->rows_pad, false), nbq = os_quad_sweep_blocks(h->rows_pad, wide8);
  LZ_TRY(one_sweep_setup(h, n, st, std::max(nbp, 2 * nbq)));
  h->last_os_fused = 1;
  LZ_TRY(warm_up(h, true));
  for (int j = 0; j < n;) {
    if (j >= 2 && n - j == 2 && (n - 2) % 4 == 2) {  // (a tail of two steps; the last two of a tail of three are single steps)
      LZ_TRY(one_sweep_pair_iter(h, n, j, st, nbp, false));
      j += 2;
      continue;
    }
    if (j < 2 || j + 4 > n) {
      begin_iter(h, j);
      LZ_TRY(one_sweep_fused_iter(h, n, j, st));
      j += 1;
      continue;
    }
    LZ_TRY(one_sweep_quad_iter(h, n, j, st, nbq, wide8));
    j += 4;
  }
  return one_sweep_fused_tail(h, n);
}

// One loop body on a state set from the host (lz_os_state_set / lz_os_step / lz_os_state_get, tests/test_gpu_one_sweep_step.py): the
// same static functions the loops call, on the basis lz_basis_alloc made.  *msg: why a step of this form cannot run at (n, j), or nullptr.
static const char* one_sweep_step_refusal(lz_handle h, int n, int j, int form) {
  const bool full_fused = (h->flags & LZ_FLAG_FUSED_NORM) && !(h->flags & LZ_FLAG_REORTH_PARTIAL);
  if (h->tune[15] == 7) return "one-sweep step: tuning knob 15 is 7 (never the fused one-sweep form)";
  if (n > kOneSweepFusedMaxN) return "one-sweep step: the basis has more rows than the fused one-sweep form takes (1520)";
  if (!one_sweep_fused_applies(h, n) || !full_fused)
    return "one-sweep step: needs one rank, fused-norm full re-orthogonalisation and a matrix with 5 or 7 entries per row (the fused one-sweep form)";
  if (j < 2) return "one-sweep step: need j >= 2";
  if (form == 1) return j + 1 > n ? "one-sweep step: need j < n" : nullptr;
  if (form == 2)
    return j + 2 > n || qtw_ldp(n + 1) > kOneSweepPairMaxLdp ? "one-sweep step: a pair needs j + 2 <= n and n + 1 within the pair walk's run length"
                                                              : nullptr;
  if (form == 4)
    return j + 4 > n || os_quad_ldp(n - 4) > os_quad_max_ldp() ? "one-sweep step: a group needs j + 4 <= n and n within the group walk's run length"
                                                               : nullptr;
  return "one-sweep step: form must be 1, 2 or 4";
}
static int one_sweep_step_blocks(lz_handle h, int form, bool wide) {
  return form == 4 ? os_quad_sweep_blocks(h->rows_pad, wide) : form == 2 ? os_pair_sweep_blocks(h->rows_pad, wide) : os_sweep_blocks(h->rows_pad);
}
int one_sweep_state_set(lz_handle h, int j, const double* G, const double* H, const double* chat, double alpha_prev, double beta_prev,
                        double beta_prev2) {
  const int n = h->n;
  if (const char* why = one_sweep_step_refusal(h, n, j, 1)) return fail(h, LZ_ERR_STATE, why);
  OneSweepState st;
  int blocks = 0;  // room for every walk a step may launch: both widths of the pair's and of the group's (two group runs per pair run)
  for (int wide = 0; wide < 2; ++wide)
    blocks = std::max({blocks, os_pair_sweep_blocks(h->rows_pad, wide != 0), 2 * os_quad_sweep_blocks(h->rows_pad, wide != 0)});
  LZ_TRY(one_sweep_setup(h, n, st, blocks));
  const size_t nn = (size_t)n * n * sizeof(double);
  LZ_HIP(h, hipMemcpyAsync(st.G, G, nn, hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipMemcpyAsync(st.H, H, nn, hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipMemcpyAsync(st.chat, chat, (size_t)j * sizeof(double), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipMemcpyAsync(h->d_alpha + (j - 1), &alpha_prev, sizeof(double), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipMemcpyAsync(h->d_beta + (j - 2), &beta_prev, sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (j >= 3) LZ_HIP(h, hipMemcpyAsync(h->d_beta + (j - 3), &beta_prev2, sizeof(double), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  h->os_step_n = n;
  return LZ_OK;
}
int one_sweep_step_run(lz_handle h, int form, int j, bool wide, int* blocks) {
  const int n = h->n;
  if (const char* why = one_sweep_step_refusal(h, n, j, form)) return fail(h, LZ_ERR_STATE, why);
  if (h->os_step_n != n || !h->d_os) return fail(h, LZ_ERR_STATE, "one-sweep step: no state set for this basis (lz_os_state_set after lz_basis_alloc)");
  OneSweepState st;
  one_sweep_view(h, n, st);
  const int nb = one_sweep_step_blocks(h, form, wide);
  const int pairs = h->last_os_pairs, quads = h->last_os_quads;  // (lz_run's record stays lz_run's)
  // what the walk leaves in d_part is copied aside behind its launch: the closing SpMV's partials reuse the head of d_part
  const size_t tap = (size_t)nb * (form == 4 ? 4 * os_quad_ldp(j) : form == 2 ? 2 * os_pair_ldp(j) : qtw_ldp(j + 2));
  if (h->tap_cap < tap) {
    LZ_TRY(dev_alloc(h, h->d_tap, tap));
    h->tap_cap = tap;
  }
  h->tap_count = tap;
  h->tap_what = form == 4 ? "one-sweep group walk" : form == 2 ? "one-sweep pair walk" : "one-sweep";
  int rc;
  if (form == 4) {
    rc = one_sweep_quad_iter(h, n, j, st, nb, wide);
  } else if (form == 2) {
    rc = one_sweep_pair_iter(h, n, j, st, nb, wide);
  } else {
    begin_iter(h, j);
    rc = one_sweep_fused_iter(h, n, j, st);
  }
  h->tap_what = nullptr;
  h->last_os_pairs = pairs;
  h->last_os_quads = quads;
  LZ_TRY(rc);
  LZ_TRY(one_sweep_join(h));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  if (blocks) *blocks = nb;
  return LZ_OK;
}
int one_sweep_state_get(lz_handle h, int form, int j, double* G, double* H, double* chat, double* g, double* gq, double* d, double* elog,
                        double* alpha, double* beta, double* nrm2, double* r2, int* ist, int* ldg, int* ldp) {
  const int n = h->n;
  if (h->os_step_n != n || !h->d_os) return fail(h, LZ_ERR_STATE, "one-sweep step: no state set for this basis (lz_os_state_set after lz_basis_alloc)");
  OneSweepState st;
  one_sweep_view(h, n, st);
  LZ_TRY(one_sweep_join(h));
  auto get = [&](void* dst, const void* src, size_t bytes) {
    return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess;
  };
  const size_t nn = (size_t)n * n * sizeof(double);
  LZ_HIP(h, get(G, st.G, nn));
  LZ_HIP(h, get(H, st.H, nn));
  LZ_HIP(h, get(chat, st.chat, ((size_t)n + 1) * sizeof(double)));
  LZ_HIP(h, get(g, st.g, ((size_t)2 * n + 2) * sizeof(double)));
  LZ_HIP(h, get(gq, st.gq, (size_t)4 * (n + 4) * sizeof(double)));
  LZ_HIP(h, get(d, h->d_c, ((size_t)4 * qtw_ldp(n + 2) + 16) * sizeof(double)));
  LZ_HIP(h, get(elog, st.elog, ((size_t)n + 1) * sizeof(double)));
  LZ_HIP(h, get(alpha, h->d_alpha, ((size_t)n + 1) * sizeof(double)));
  LZ_HIP(h, get(beta, h->d_beta, ((size_t)n + 1) * sizeof(double)));
  LZ_HIP(h, get(nrm2, h->d_nrm2, sizeof(double)));
  LZ_HIP(h, get(r2, h->d_r2, (size_t)h->rows * sizeof(double)));
  LZ_HIP(h, get(ist, h->d_osi, 8 * sizeof(int)));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  if (ldg) *ldg = n + 4;
  if (ldp) *ldp = form == 4 ? os_quad_ldp(j) : form == 2 ? os_pair_ldp(j) : qtw_ldp(j + 2);
  return LZ_OK;
}

// raw rows j0 .. j0 + count - 1 with their padding (rows_pad doubles each) and the first part_count doubles the last step's walk left in
// d_part (its tap)
int one_sweep_raw_get(lz_handle h, int j0, int count, double* rows, double* part, int64_t part_count) {
  LZ_TRY(one_sweep_join(h));
  if (rows) {
    if (count < 1 || j0 < 0 || j0 + count > h->n) return fail(h, LZ_ERR_ARG, "lz_os_raw_get: rows out of range");
    LZ_HIP(h, hipMemcpy2DAsync(rows, (size_t)h->rows_pad * sizeof(double), h->d_V + (int64_t)j0 * h->ldv, (size_t)h->ldv * sizeof(double),
                               (size_t)h->rows_pad * sizeof(double), (size_t)count, hipMemcpyDeviceToHost, h->stream));
  }
  if (part) {
    if (part_count < 0 || (size_t)part_count > h->tap_count || !h->d_tap) return fail(h, LZ_ERR_STATE, "lz_os_raw_get: the last step's walk left fewer partials");
    LZ_HIP(h, hipMemcpyAsync(part, h->d_tap, (size_t)part_count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

// ---- which loop structure runs the Krylov iteration --------------------------------------------------------------------
// (the values are what lz_last_engine reports)
enum Loop {
  LOOP_SIX = 0,               // six launches per step; also the partial re-orthogonalisation mode and every A/B arm of a kernel
  LOOP_SMALL_ENGINE = 1,      // kernel-bench build only: the whole run as one cooperative kernel (lz_small.hip)
  LOOP_FUSED_SMALL = 2,       // <= 8 pass-1 slices, one rank: three launches per step (run_loop_fused_small)
  LOOP_THREE_TERM_FUSED = 3,  // up to 4e6 rows per rank: five launches per step (run_loop_three_term_fused)
  LOOP_SMALL_STEP = 4,        // kernel-bench build only: one launch per step
  LOOP_ONE_REDUCE_REPEATED = 5,  // a one-reduce run whose cancellation guard fired: repeated on the default loop
  LOOP_ONE_REDUCE = 6,        // LZ_FLAG_ONE_REDUCE: one all-reduce per iteration
  LOOP_PARTIAL_DEVICE = 7,    // LZ_FLAG_REORTH_PARTIAL, default: the omega-recurrence and the sweep decision live on the device
  LOOP_PARTIAL_ONE_REDUCE = 8, // LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE: the same with one all-reduce per iteration (look-ahead gate)
  LOOP_ONE_SWEEP = 9          // above kThreeTermFusedMaxRows rows on one rank: one walk over the basis per step (run_loop_one_sweep)
};

// plan: the Q^T w plan the run will use - the handle's, made by basis_alloc for n rows, unless the caller asks before it allocates
Loop choose_loop(lz_handle h, int n, const QtwPlan* plan = nullptr) {
  const int f = h->flags;
  const QtwPlan& qp = plan ? *plan : h->qplan;
  const bool default_kernels = qp.family == 2 && !(f & (LZ_FLAG_QTW_MFMA | LZ_FLAG_QTW_VALU)) && h->tune[1] == 0 && h->tune[8] == 0;
  const bool full_fused = (f & LZ_FLAG_FUSED_NORM) && !(f & LZ_FLAG_REORTH_PARTIAL);
  if ((f & LZ_FLAG_ONE_REDUCE) && !(f & LZ_FLAG_REORTH_PARTIAL) && qp.family == 2) return LOOP_ONE_REDUCE;
  if ((f & LZ_FLAG_ONE_REDUCE) && (f & LZ_FLAG_REORTH_PARTIAL) && default_kernels && h->tune[18] != 1 && !(f & LZ_FLAG_OVERLAP_HALO))
    return LOOP_PARTIAL_ONE_REDUCE;
  // partial re-orthogonalisation: device-resident decisions with the default kernels (tune[18] == 1: the host-decided loop,
  // two scalars read back per step - kept for the bit-identity test and as an A/B arm)
  if ((f & LZ_FLAG_REORTH_PARTIAL) && default_kernels && h->tune[18] != 1 && !(f & LZ_FLAG_OVERLAP_HALO)) return LOOP_PARTIAL_DEVICE;
  const bool one_rank = h->world == 1 && h->comm_kind == 0;
#ifdef LZ_KBENCH
  const bool want_steps = h->tune[15] == 5 && n <= kSmallStepMaxN;
  if ((h->tune[15] == 2 || h->tune[15] == 3 || want_steps) && one_rank && full_fused && default_kernels && !(f & LZ_FLAG_SPMV_SCALAR) &&
      qp.L == 512 && h->rows_pad <= kSmallMaxPadRows && n <= kSmallMaxPadRows && small_engine_applies(h))
    return want_steps ? LOOP_SMALL_STEP : LOOP_SMALL_ENGINE;
  const bool knob_auto = h->tune[15] == 0 || h->tune[15] == 5;
#else
  const bool knob_auto = h->tune[15] == 0;
#endif
  // one-sweep loop: one rank, full fused-norm re-orthogonalisation, default kernels, no overlap; tune[15] == 6 forces it at any size
  const bool one_sweep_ok = one_rank && full_fused && default_kernels && !(f & LZ_FLAG_OVERLAP_HALO) && n >= 2 && n <= kOneSweepMaxN;
  // (7: never the fused form; 6: never the pair form; 8 / 9: the pair form where it applies, 8 / 16 positions per lane in its walk - A/B;
  // 10 / 11: the group form where it applies, 4 / 8 positions per lane in its walk - A/B)
  if (h->tune[15] >= 6 && h->tune[15] <= 13 && one_sweep_ok) return LOOP_ONE_SWEEP;
  if (!knob_auto || !full_fused || !default_kernels) return LOOP_SIX;
  if (one_rank && qp.G <= 8 && n <= 4096 && h->part_cap >= fused_coff(h) + (size_t)(n + 16) * (size_t)qp.G) return LOOP_FUSED_SMALL;
  if (!(f & LZ_FLAG_OVERLAP_HALO) && h->rows_pad <= kThreeTermFusedMaxRows) return LOOP_THREE_TERM_FUSED;
  if (one_sweep_ok) return LOOP_ONE_SWEEP;
  return LOOP_SIX;
}

// ---- the plain loop: six launches per step (pass 1, second-stage sums, pass 2, SpMV, alpha sum, three-term), with the
// opt-in partial re-orthogonalisation (Simon's omega-recurrence on the host) --------------------------------------------
// Simon's omega-recurrence on the host (the host-decided arm, knob 18 = 1): omega_{j,k} estimates v_j . v_k, and a sweep is due when
// an estimate exceeds sqrt(eps).  Plain arithmetic, no device call: run_loop_six asks due(j) before step j and feeds it the step's two
// scalars, alpha_j and ||r||^2 = beta_{j+1}^2, afterwards.
struct HostOmega {
  static constexpr double eps = 2.220446049250313e-16, thresh = 1.4901161193847656e-08;
  std::vector<double> w_prev, w_cur, w_new, ha, hb;  // omega_{j-2,:}, omega_{j-1,:}, omega_{j,:}; alpha_k; beta_k (norm forming V[k])
  double normA = 0.0;
  bool force_next = false;
  void start(int n, double nrm2_0) {  // nrm2_0: ||r||^2 of the warm-up
    for (auto* v : {&w_prev, &w_cur, &w_new, &ha, &hb}) v->assign((size_t)n + 1, 0.0);
    w_cur[0] = 1.0;  // omega_{0,0} = v_0 . v_0 (until round 4 this row was all zero, which made a spurious sweep due at j = 2)
    hb[0] = std::sqrt(nrm2_0);
  }
  // does step j sweep?  Advances the recurrence to row j.
  bool due(int j) {
    bool over = false;
    if (j >= 1) {
      // beta_j omega_{j,k} = beta_{k+1} omega_{j-1,k+1} + (alpha_k - alpha_{j-1}) omega_{j-1,k} + beta_k omega_{j-1,k-1}
      //                      - beta_{j-1} omega_{j-2,k}  (+ rounding of size eps ||A||),   k <= j-2
      std::fill(w_new.begin(), w_new.end(), 0.0);
      w_new[(size_t)j] = 1.0;
      w_new[(size_t)j - 1] = eps;
      double worst = 0.0;
      for (int k = 0; k + 2 <= j; ++k) {
        double t = hb[(size_t)k + 1] * w_cur[(size_t)k + 1] + (ha[(size_t)k] - ha[(size_t)j - 1]) * w_cur[(size_t)k] -
                   hb[(size_t)j - 1] * w_prev[(size_t)k];
        if (k > 0) t += hb[(size_t)k] * w_cur[(size_t)k - 1];
        t += (t < 0 ? -1.0 : 1.0) * 2.0 * eps * normA;
        w_new[(size_t)k] = t / hb[(size_t)j];
        worst = std::max(worst, std::fabs(w_new[(size_t)k]));
      }
      over = worst > thresh;
      std::swap(w_prev, w_cur);
      std::swap(w_cur, w_new);
    }
    const bool sweep = (j == 0) || over || force_next;  // a due sweep also covers the next vector (both feed the recurrence)
    force_next = over;
    if (sweep)
      for (int k = 0; k < j; ++k) w_cur[(size_t)k] = eps;
    return sweep;
  }
  void feed(int j, double alpha, double nrm2) {
    ha[(size_t)j] = alpha;
    hb[(size_t)j + 1] = std::sqrt(nrm2);
    normA = std::max(normA, std::fabs(alpha) + hb[(size_t)j] + hb[(size_t)j + 1]);
  }
};

// the host-decided arm's read-back: alpha[j] (j >= 0) and ||r||^2 into the pinned pair, one synchronisation
static int read_back_step(lz_handle h, int j) {
  if (!h->h_pinned) LZ_HIP(h, hipHostMalloc(reinterpret_cast<void**>(&h->h_pinned), 8 * sizeof(double), hipHostMallocDefault));
  if (j >= 0) LZ_HIP(h, hipMemcpyAsync(&h->h_pinned[0], h->d_alpha + j, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipMemcpyAsync(&h->h_pinned[1], h->d_nrm2, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  h->host_syncs += 1;
  return LZ_OK;
}

int run_loop_six(lz_handle h, int n, int j0 = 0) {
  const bool partial = (h->flags & LZ_FLAG_REORTH_PARTIAL) != 0;
  const bool fused = (h->flags & LZ_FLAG_FUSED_NORM) != 0 && !partial;
  if (j0 == 0) {
    LZ_TRY(warm_up(h, !fused));
  } else if (!fused) {
    // resumed run (lz_run_resume): steps 0 .. j0-1 are in the basis, r is the residual entering step j0; the scale-then-dot order
    // wants ||r||^2 in d_nrm2: r = r - 0 * V[0] leaves r unchanged bit for bit and refreshes it
    LZ_HIP(h, hipMemsetAsync(h->d_c + n, 0, sizeof(double), h->stream));
    LZ_TRY(step_three_term(h, 0, -1, h->d_c + n, nullptr, true));
  }
  // Partial re-orthogonalisation (opt-in, never resumed): the sweep decision is the host's, two doubles are copied back per step
  HostOmega omega;
  if (partial) {
    LZ_TRY(read_back_step(h, -1));
    omega.start(n, h->h_pinned[1]);
  }
  int sweeps = 0;
  for (int j = j0; j < n; ++j) {
    begin_iter(h, j);
    const int bidx = beta_index(n, j);
    double* bslot = h->d_beta + bidx;
    if (!partial || omega.due(j)) {
      ++sweeps;
      LZ_TRY(step_reorth(h, j, j + 1, true, bidx, true));
    } else {
      Scope sc(h, LZ_K_QTW, 16.0 * (double)h->rows, (double)h->rows);
      launch_scale_store(basis_row(h, j), h->d_r, h->d_nrm2, bslot, h->rows_pad, h->stream);
      LZ_TRY(check_launch(h, "scale_store"));
    }
    LZ_TRY(step_spmv(h, j));
    // at j = 0 the reference subtracts beta * V[-1], the still-zero last row: a no-op
    LZ_TRY(step_three_term(h, j, j > 0 ? j - 1 : -1, h->d_alpha + j, bslot, !fused));
    if (partial) {
      LZ_TRY(read_back_step(h, j));
      omega.feed(j, h->h_pinned[0], h->h_pinned[1]);
    }
  }
  h->last_sweeps = sweeps;
  h->r_state = 1;
  return LZ_OK;
}

// ---- partial re-orthogonalisation, device-resident (round 4; the default of LZ_FLAG_REORTH_PARTIAL) -----------------------
// The loop above with the host taken out: Simon's omega-recurrence runs in a one-block kernel behind the three-term kernel
// (k_omega, lz_reorth.hip; on one rank it also folds the ||r||^2 partials, so it costs no launch), which leaves a gate in
// device memory; the sweep kernels of the next step (pass 1, second-stage sums, pass 2) are always enqueued and return at
// once when the gate says no sweep is due.  No read-back, no hipStreamSynchronize between the first and the last launch
// (lz_last_host_syncs == 0 on one rank / over RCCL).  Every rank takes the same decision: its inputs are all-reduced sums.
// A step without a sweep on one rank with an ELL-ordered fixed-K matrix is TWO streaming kernels: the SpMV forms
// v_j = r / beta itself wherever it reads x (k_spmv_ell<.., SC>: the separate 16M-byte scale pass is gone; r and y
// ping-pong between two buffers), and the three-term kernel.  Other matrices keep the (gated) scale kernel.
// Decisions, coefficients and basis are bit-identical to the host-decided loop (tests/test_gpu_lanczos.py).
// j0 > 0 (lz_run_resume_partial): steps 0 .. j0-1 are in the basis, r is the residual entering step j0 and `state_j0` the omega state a
// run of j0 steps left behind (lz_get_omega_state: its layout is that of a j0-step run).
int run_loop_partial_device(lz_handle h, int n, int j0 = 0, const double* state_j0 = nullptr) {
  const double M = (double)h->rows;
  if (h->om_n < n) {
    LZ_TRY(dev_alloc(h, h->d_om, omega_state_doubles(n)));
    LZ_TRY(dev_alloc(h, h->d_omi, omega_state_ints(n) + 1));  // (+ the ticket of pass 1's folded second stage)
    h->om_n = n;
  }
  h->om_run_n = n;
  if (j0 > 0) {
    // the state of the j0-step run, re-laid for n steps: [normA, force | hb[0 .. n + 2) | three rows of n + 1]; entries past j0 are zero,
    // exactly what an uninterrupted n-step run holds there at this point
    std::vector<double> st(omega_state_doubles(n), 0.0);
    st[0] = state_j0[0];
    st[1] = state_j0[1];
    const double* hb_s = state_j0 + 2;
    const double* W_s = hb_s + (j0 + 2);
    double* hb_d = st.data() + 2;
    double* W_d = hb_d + (n + 2);
    for (int k = 0; k < j0 + 2; ++k) hb_d[k] = hb_s[k];
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k <= j0; ++k) W_d[(size_t)r * (n + 1) + k] = W_s[(size_t)r * (j0 + 1) + k];
    LZ_HIP(h, hipMemcpyAsync(h->d_om, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    LZ_HIP(h, hipMemsetAsync(h->d_omi, 0, (omega_state_ints(n) + 1) * sizeof(int), h->stream));
    LZ_HIP(h, hipStreamSynchronize(h->stream));  // (`st` is a local)
  }
  LZ_HIP(h, hipMemsetAsync(h->d_omi + omega_state_ints(n), 0, sizeof(int), h->stream));
  const int* gate = h->d_omi;
  const bool one_rank = h->world <= 1 && !(h->tune[6] && h->comm_kind);
  if (one_rank && h->kind == 1 && h->tune[18] != 2 && h->tune[17] != 1 && !h->csr.ell_rb && !h->csr.pb &&
      (h->csr.fixed_k == 5 || h->csr.fixed_k == 7))
    // first partial run on this matrix: the ELL copy the fused r / beta needs.  (5 and 7 entries per row: its alpha partials
    // are grouped exactly like k_spmv_fixed's - 512-row blocks, rows t and t + 256 per lane - so the fused and the unfused loop
    // produce the same bits; 27-point rows keep the scale kernel + the CSR-stream SpMV)
    LZ_HIP(h, ell_build(h->csr, 0, h->stream));
  const bool fuse_scale = one_rank && h->kind == 1 && ell_usable(h->csr, h->flags) && h->tune[18] != 2;
  // warm-up (Lanczos.py:108-110): r = A v0; alpha0 = r.v0; r = r - alpha0 v0; ||r||^2
  if (j0 == 0) LZ_TRY(step_spmv(h, 0));
  int np = 0;
  auto three_term_and_decide = [&](int j, int jm1, const double* d_alpha, const double* d_beta, double* r, bool decide, int jn) -> int {
    LZ_TRY(step_three_term(h, j, jm1, d_alpha, d_beta, false, &np, r));
    Scope sc(h, LZ_K_FINAL, 0, 0);
    if (one_rank && decide) {
      launch_omega(h->d_part, np, h->d_nrm2, h->d_alpha, jn, n, h->d_om, h->d_omi, h->stream);
      return check_launch(h, "final_sum(nrm2) + omega");
    }
    launch_final_sum(h->d_part, np, h->d_nrm2, h->stream);
    LZ_TRY(check_launch(h, "final_sum(nrm2)"));
    LZ_TRY(comm_allreduce(h, h->d_nrm2, 1));
    if (decide) {
      launch_omega(nullptr, 0, h->d_nrm2, h->d_alpha, jn, n, h->d_om, h->d_omi, h->stream, h->d_c);  // (d_c: zero unless step jn sweeps - it is all-reduced every step)
      LZ_TRY(check_launch(h, "omega"));
    }
    return LZ_OK;
  };
  // the warm-up's r = r - alpha0 v0; resumed: r = r - 0 * V[0] leaves r unchanged bit for bit, refreshes ||r||^2 with the very kernel
  // (and summation) that produced it in the uninterrupted run, and k_omega takes the decision of step j0 from it
  if (j0 > 0) LZ_HIP(h, hipMemsetAsync(h->d_c + n, 0, sizeof(double), h->stream));
  LZ_TRY(three_term_and_decide(0, -1, j0 > 0 ? h->d_c + n : h->d_alpha, nullptr, h->d_r, true, j0));
  double* rcur = h->d_r;   // the residual entering the step
  double* rnext = h->d_r2; // where the fused SpMV writes y (it reads r through its gathers: not in place)
  for (int j = j0; j < n; ++j) {
    begin_iter(h, j);
    double* bslot = beta_slot(h, n, j);
    // the sweep (gated; bytes are accounted after the run from the device's sweep log: the host does not know which ran)
    {
      QtwFuse fz;
      fz.gate = gate;
      // pass 1's last block adds the blocks' runs itself (k_final_rows_t's order: same bits): one gated launch less per step.
      // (tune[18] == 3: the separate second-stage kernel, A/B)
      const bool fold = h->tune[18] != 3;
      if (fold) {
        fz.ticket = reinterpret_cast<unsigned*>(h->d_omi + omega_state_ints(n));
        fz.c_out = h->d_c;
      }
      h->qplan.variant = 0;
      {
        Scope sc(h, LZ_K_QTW, 0, 0);
        LZ_HIP(h, launch_qtw(h->d_V, h->ldv, h->rows_pad, j + 1, j, rcur, h->d_nrm2, bslot, h->qplan, h->d_part, 1, h->stream, &fz));
        LZ_TRY(check_launch(h, "qtw(gated)"));
      }
      if (!fold) {
        Scope sc(h, LZ_K_FINAL, 0, 0);
        launch_final_rows(h->d_part, j + 1, h->qplan.P, h->d_c, h->stream, true, gate);
        LZ_TRY(check_launch(h, "final_rows(gated)"));
      }
      LZ_TRY(comm_allreduce(h, h->d_c, j + 1));  // (N > 1: issued every step - the host cannot skip a collective the device may need)
      {
        Scope sc(h, LZ_K_UPDATE, 0, 0);
        launch_update(h->d_V, h->ldv, h->rows_pad, j + 1, j, h->d_c, nullptr, bslot, 0, h->stream, 0, -1, 0, 0, 0, 0, 0, gate);
        LZ_TRY(check_launch(h, "update(gated)"));
      }
    }
    if (fuse_scale) {
      int npa = 0;
      LZ_TRY(step_scaling_spmv(h, n, j, rcur, rnext, gate, &npa));  // V[j] = r / beta on read unless the step swept
      LZ_TRY(step_final_sum(h, npa, h->d_alpha + j, "final_sum(alpha)"));
      std::swap(rcur, rnext);
    } else {
      {
        Scope sc(h, LZ_K_QTW, 16.0 * M, M);
        launch_scale_store(basis_row(h, j), rcur, h->d_nrm2, bslot, h->rows_pad, h->stream, gate);
        LZ_TRY(check_launch(h, "scale_store(gated)"));
      }
      LZ_TRY(step_spmv(h, j));  // r = A V[j] into h->d_r (== rcur), alpha_j
    }
    // at j = 0 the reference subtracts beta * V[-1], the still-zero last row: a no-op
    LZ_TRY(three_term_and_decide(j, j > 0 ? j - 1 : -1, h->d_alpha + j, bslot, rcur, j + 1 < n, j + 1));
  }
  if (rcur != h->d_r) std::swap(h->d_r, h->d_r2);  // the residual entering step n is what lz_get_residual hands out
  h->r_state = 1;
  return LZ_OK;
}

// ---- partial re-orthogonalisation with ONE all-reduce per step (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE; round 5) --------
// The device-decided loop above issues three collectives per step on a partition (alpha, ||r||^2 and - used or not - the
// coefficient vector): at the N = 8 rank share a step without a sweep is ~26 us of kernels, so three latency-bound all-reduces
// would make the selective arm scale negatively.  Here a step costs ONE all-reduce + ONE exchange, sweep or no sweep, exactly like
// run_loop_onereduce: the single buffer [p_0..p_{m-1}, r''.r'' | q_0..q_{m-1}, u.u, u.r'', alpha] carries alpha's partial, the three
// self terms and the sweep's dots (zero in a step without a sweep); the gate is read by every kernel from device memory and is the
// same on every rank because it is derived from reduced sums only (k_partial_onered_post: a one-step look-ahead of Simon's
// recurrence, since the exact test of omega_{j,:} needs the very sums this all-reduce delivers).
// Per step:  [pass 1, two columns - gated]  [second stage - gated]  ALL-REDUCE  [post: alpha, c, ||r||^2, omega, next gate]
//            [r = r'' - alpha u]  [update - gated | scale V[j] = r / beta - gated the other way]  EXCHANGE  [SpMV + alpha partial]
//            [r'' = A v_j - beta v_{j-1} + the three self terms' partials]  [their sums + alpha's into the next buffer]
// Two buffers alternate (the update of step j still reads buffer j & 1 while the post kernel clears the other).  No host
// synchronisation inside the loop over RCCL.  The three-sum ||r||^2 cancels like the full one-reduce loop's: same guard, same
// repeat of the solve (on the three-collective device loop) when it fires; same coefficients relative to u.u, same last alpha.
int run_loop_partial_onereduce(lz_handle h, int n) {
  const double M = (double)h->rows;
  if (h->om_n < n + 4) {  // (omega_onered_ints(n) <= omega_state_ints(n + 4) + 1)
    LZ_TRY(dev_alloc(h, h->d_om, omega_state_doubles(n + 4)));
    LZ_TRY(dev_alloc(h, h->d_omi, omega_state_ints(n + 4) + 1));
    h->om_n = n + 4;
  }
  const double kappa = h->tune[20] > 0 ? (double)h->tune[20] : 4.0;
  double* const uu_keep = h->d_beta + n;  // (d_beta has n + 1 doubles, the coefficients use n - 1) u.u of the step before
  const size_t bstride = (size_t)2 * qtw_ldp(n + 2) + 8;
  {
    Scope sc(h, LZ_K_FINAL, 0, 0);
    launch_partial_onered_post(nullptr, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, -1, n, h->d_om, h->d_omi, kappa, nullptr, nullptr, h->stream);
    LZ_TRY(check_launch(h, "partial_onered_post(init)"));
  }
  unsigned* ticket = reinterpret_cast<unsigned*>(h->d_omi + omega_onered_ints(n));
  LZ_HIP(h, hipMemsetAsync(ticket, 0, sizeof(unsigned), h->stream));
  const bool lean = h->tune[18] != 3;  // (knob 18 = 3: every folded stage as a kernel of its own - the first form of this loop, kept as the A/B arm)
  LZ_TRY(step_spmv(h, 0, h->d_c + onered_slot(0), false));  // warm-up: r'' = A v0 (Lanczos.py:108), alpha0 partial
  // the self terms' partials (and the lean form's pass 1) live behind the SpMV's alpha partials in d_part
  double* spart = h->d_part + (lean ? onered_part_off(h) : 0);
  for (int j = 0; j < n; ++j) {
    begin_iter(h, j);
    double* bslot = beta_slot(h, n, j);
    const int m = j, urow = j > 0 ? j - 1 : 0, ldp = onered_ldp(m);
    const bool last = j == n - 1;
    double* buf = h->d_c + (size_t)(j & 1) * bstride;
    double* bufn = h->d_c + (size_t)((j + 1) & 1) * bstride;
    const int* gate = h->d_omi + (j & 1);
    double* u = basis_row(h, urow);
    double* vj = basis_row(h, j);
    // (lean: pass 1's last block adds the blocks' runs itself, in k_final_rows_t's order)
    LZ_TRY(step_onereduce_head(h, j, urow, spart, buf, gate, lean ? ticket : nullptr));
    {
      Scope sc(h, LZ_K_FINAL, 0, 0);
      launch_partial_onered_post(buf, last ? nullptr : bufn, last ? 0 : onered_slot(j + 1) + 1, m, ldp, h->d_alpha + urow, h->d_nrm2, h->d_alpha, j, n,
                                 h->d_om, h->d_omi, kappa, j >= 2 ? beta_slot(h, n, j - 1) : nullptr, uu_keep, h->stream);
      LZ_TRY(check_launch(h, "partial_onered_post"));
    }
    if (lean) {
      // ONE launch forms w = (r'' - alpha u) / beta and either sweeps (V[j] = 2 w - sum c_i V_i) or stores V[j] = w
      Scope sc(h, LZ_K_UPDATE, 32.0 * M, 4.0 * M);  // (a sweep's basis rows: accounted after the run)
      launch_update(h->d_V, h->ldv, h->rows_pad, j + 1, j, buf, h->d_r, bslot, 0, h->stream, 0, -1, 1, 0, 0, 0, 0, gate, u, h->d_alpha + urow);
      LZ_TRY(check_launch(h, "update | scale (gated)"));
    } else {
      LZ_TRY(step_two_term(h, u, h->d_alpha + urow, "three_term(alpha)"));  // r = r'' - alpha u
      {
        Scope sc(h, LZ_K_UPDATE, 0, 0);
        launch_update(h->d_V, h->ldv, h->rows_pad, j + 1, j, buf, h->d_r, bslot, 0, h->stream, 0, -1, 1, 0, 0, 0, 0, gate);
        LZ_TRY(check_launch(h, "update(gated)"));
      }
      {
        Scope sc(h, LZ_K_QTW, 16.0 * M, M);
        launch_scale_store(vj, h->d_r, h->d_nrm2, bslot, h->rows_pad, h->stream, gate);
        LZ_TRY(check_launch(h, "scale_store(gated)"));
      }
    }
    if (last) {  // the last alpha travels with the last vector's u.u (an ungated pass over no rows), as in run_loop_onereduce
      LZ_TRY(step_spmv(h, j, h->d_c + onered_slot(0), false));
      LZ_TRY(step_onereduce_head(h, 0, j, h->d_part, h->d_c, nullptr, nullptr));
      Scope sc(h, LZ_K_FINAL, 0, 0);
      launch_onereduce_finish(h->d_c, onered_ldp(0), h->d_alpha + j, n >= 2 ? bslot : nullptr, uu_keep, h->stream);
      LZ_TRY(check_launch(h, "onereduce_finish"));
      break;
    }
    // r'' = A V[j] - beta V[j-1] (at j = 0 the reference's V[-1] is the zero row) + the self terms of the next step's ||r||^2;
    // the four second-stage sums (alpha's partial and the three self terms) leave in one launch
    const int mn = j + 1, ldpn = onered_ldp(mn);
    int npa = 0, G3 = 0;
    if (lean)
      LZ_TRY(step_spmv(h, j, nullptr, false, &npa));
    else
      LZ_TRY(step_spmv(h, j, bufn + onered_slot(mn), false));
    {
      Scope sc(h, LZ_K_THREE, (j > 0 ? 40.0 : 16.0) * M, (j > 0 ? 8.0 : 6.0) * M);
      G3 = launch_three_term_self(h->d_r, vj, j > 0 ? basis_row(h, j - 1) : nullptr, bslot, h->rows_pad, spart, h->stream);
      LZ_TRY(check_launch(h, "three_term(beta) + self terms"));
    }
    FinalMulti fm;
    for (int q = 0; q < 3; ++q) {
      fm.part[q] = spart + (size_t)q * G3;
      fm.n[q] = G3;
    }
    fm.out[0] = bufn + mn;             // r''.r''
    fm.out[1] = bufn + ldpn + mn + 1;  // u.r''
    fm.out[2] = bufn + ldpn + mn;      // u.u
    fm.part[3] = h->d_part, fm.n[3] = npa, fm.out[3] = bufn + onered_slot(mn);  // alpha's partial (k_final_sum's grouping)
    Scope sc(h, LZ_K_FINAL, 0, 0);
    launch_final_sum_multi(fm, lean ? 4 : 3, h->stream);
    LZ_TRY(check_launch(h, "final_sum(alpha, self terms)"));
  }
  return LZ_OK;
}

// after the final synchronisation of a device-decided partial run: the device's sweep log (its per-step words start at log0) ->
// lz_last_sweeps, lz_last_sweep_log and the byte / flop accounting of the gated launches (pass 1: 8 j M + 16 M bytes, pass 2 the same;
// in a swept step the scale kernel / fused scale did no work).  A resumed run's log holds zeros for the steps of the first leg.
void account_partial_device(lz_handle h, int n, const std::vector<int>& log, size_t log0) {
  const double M = (double)h->rows;
  int sweeps = 0;
  for (int j = 0; j < n; ++j) {
    h->sweep_log[(size_t)j] = log[log0 + j] != 0;
    if (!log[log0 + j]) continue;
    ++sweeps;
    // (pass 1's read of r and write of V[j], 16 M bytes, are on the books already: the scale pass is accounted in every step)
    const double flops = 2.0 * (j + 1) * M;
    const bool timed = (h->flags & LZ_FLAG_PROFILE) != 0 && iter_sampled(h, j);
    for (int cls : {LZ_K_QTW, LZ_K_UPDATE}) {
      const double bytes = 8.0 * j * M + (cls == LZ_K_UPDATE ? 16.0 * M : 0.0);
      h->acc.bytes[cls] += bytes;
      h->acc.flops[cls] += flops;
      if (timed) h->acc.timed_bytes[cls] += bytes;
    }
  }
  h->last_sweeps = sweeps;
}

// Breakdown report.  The reference divides by beta blindly (Lanczos.py:113): an exhausted Krylov
// space gives it a residual of rounding noise (or an exact zero and then inf/NaN), and it carries on.  So does this
// run - the coefficients are delivered exactly as computed - but the status says so: a beta at or below 64 eps times
// the scale of T (max |alpha|, |beta|), or any non-finite coefficient.  beta[n-2] is also where step j = 0 parks its
// norm before step n-1 overwrites it, so every entry of beta_out has been a divisor.
int breakdown_status(lz_handle h, int n, const double* alpha_out, const double* beta_out) {
  double tscale = 0.0;
  for (int j = 0; j < n; ++j) {
    if (std::isfinite(alpha_out[j])) tscale = std::max(tscale, std::fabs(alpha_out[j]));
    if (j < n - 1 && std::isfinite(beta_out[j])) tscale = std::max(tscale, std::fabs(beta_out[j]));
  }
  const double tiny = 64.0 * 2.220446049250313e-16 * tscale;
  for (int j = 0; j < n; ++j) {
    const bool bad_a = !std::isfinite(alpha_out[j]);
    const bool bad_b = j < n - 1 && !(std::isfinite(beta_out[j]) && beta_out[j] > tiny);
    if (bad_a || bad_b) {
      char msg[200];
      if (bad_b && std::isfinite(beta_out[j]))
        snprintf(msg, sizeof msg, "lz_run: Lanczos breakdown - beta[%d] = %.3e <= 64 eps * %.3e: the Krylov space is exhausted, later vectors are rounding noise",
                 j, beta_out[j], tscale);
      else
        snprintf(msg, sizeof msg, "lz_run: Lanczos breakdown - %s[%d] is not finite (a residual norm reached zero)", bad_b ? "beta" : "alpha", j);
      h->err = msg;
      return LZ_WARN_BREAKDOWN;
    }
  }
  return LZ_OK;
}

// ---- the run frame: what lz_run, lz_run_resume and lz_run_resume_partial do around their loop: begin -> the caller's upload ->
// uploaded -> the loop -> drain -> (the caller looks at its extra words) -> finish -----------------------------------------------
struct RunExtra {  // device words an entry point wants on the host behind alpha / beta, ahead of the one synchronisation
  void* dst;
  const void* src;
  size_t bytes;
};
struct RunFrame {
  lz_handle h;
  int n;
  double t0 = 0, t1 = 0, t2 = 0, t3 = 0;  // host clock, ms: entry, basis ready, upload enqueued, loop enqueued (LZ_DEBUG_TIMING)
  static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

  // the basis for n steps, its first zero_rows rows cleared, and the handle's per-run record as a run that has not started leaves it:
  // every step swept, no residual.  The loops overwrite what they know better, each at its own end.
  int begin(int zero_rows) {
    t0 = now();
    h->run_timed = false;  // (a pass that was abandoned after its drain books no time)
    LZ_TRY(basis_alloc(h, n, zero_rows));
    h->halo_inflight_j = -1;
    h->y_n = 0;  // the Ritz vectors of an earlier run are not this run's: fetches answer LZ_ERR_STATE until lz_ritz_vectors is called again
    h->last_engine = LOOP_SIX;
    h->last_sweeps = n;
    h->last_misses = 0;
    h->last_gate_trips = 0;
    h->last_os_fused = 0;
    h->last_os_pairs = 0;
    h->last_pair_abandoned = 0;
    h->last_os_quads = 0;
    h->last_quad_abandoned = 0;
    h->sweep_log.assign((size_t)n, 1);  // which steps ran the sweep (lz_last_sweep_log): all of them unless a partial loop says otherwise
    h->host_syncs = 0;
    h->r_state = 0;
    t1 = now();
    return LZ_OK;
  }
  int uploaded() {
    t2 = now();
    LZ_HIP(h, hipEventRecord(h->run_a, h->stream));
    return LZ_OK;
  }
  // behind the loop: alpha, beta and the extras to the host, THE synchronisation of the run
  int drain(double* alpha_out, double* beta_out, const std::vector<RunExtra>& extras = {}) {
    h->prof_iter = true;
    LZ_HIP(h, hipEventRecord(h->run_b, h->stream));
    t3 = now();
    h->run_timed = true;  // (an error from here on: drain_events books the run's time)
    LZ_HIP(h, hipMemcpyAsync(alpha_out, h->d_alpha, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    LZ_HIP(h, hipMemcpyAsync(beta_out, h->d_beta, (size_t)(n - 1) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    for (const RunExtra& e : extras) LZ_HIP(h, hipMemcpyAsync(e.dst, e.src, e.bytes, hipMemcpyDeviceToHost, h->stream));
    LZ_HIP(h, hipStreamSynchronize(h->stream));
    return LZ_OK;
  }
  // the run's time on the books, the breakdown report as the status
  int finish(const double* alpha_out, const double* beta_out) {
    float ms = 0.f;
    LZ_HIP(h, hipEventElapsedTime(&ms, h->run_a, h->run_b));
    h->acc.total_ms += ms;
    h->run_timed = false;
    return breakdown_status(h, n, alpha_out, beta_out);
  }
};

// a checkpoint of j0 completed steps: the basis rows, the residual entering step j0, alpha[0 .. j0), beta[0 .. j0 - 1)
static int upload_checkpoint(lz_handle h, int j0, const double* V_rows, int64_t ldv_in, const double* r_local, const double* alpha_in,
                             const double* beta_in) {
  LZ_TRY(upload2d(h, h->d_V, (size_t)h->ldv * sizeof(double), V_rows, (size_t)ldv_in * sizeof(double), (size_t)h->rows * sizeof(double), (size_t)j0));
  LZ_TRY(upload(h, h->d_r, r_local, (size_t)h->rows * sizeof(double)));
  LZ_HIP(h, hipMemcpyAsync(h->d_alpha, alpha_in, (size_t)j0 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (j0 > 1) LZ_HIP(h, hipMemcpyAsync(h->d_beta, beta_in, (size_t)(j0 - 1) * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return LZ_OK;
}

// One pass of lz_run.  *again: the pass's own check says its coefficients do not hold; what makes the next pass take another loop is set
// (LZ_FLAG_ONE_REDUCE cleared, or h->quad_tripped / h->pair_tripped), nothing is on the books, and lz_run makes that pass.
static int run_once(lz_handle h, int n, const double* v0_local, double* alpha_out, double* beta_out, bool* again) {
  *again = false;
  RunFrame fr{h, n};
  LZ_TRY(fr.begin(1));
  LZ_TRY(upload(h, h->d_V, v0_local, (size_t)h->rows * sizeof(double)));
  LZ_TRY(fr.uploaded());
  const Loop loop = choose_loop(h, n);
  const bool one_reduce = loop == LOOP_ONE_REDUCE || loop == LOOP_PARTIAL_ONE_REDUCE;
  bool tried_pairs = false, tried_quads = false;
  h->last_engine = (int)loop;
  switch (loop) {
#ifdef LZ_KBENCH
    case LOOP_SMALL_ENGINE:
    case LOOP_SMALL_STEP: {
      bool ran = false;
      LZ_TRY(run_small_engine(h, n, v0_local, loop == LOOP_SMALL_STEP, &ran));
      if (!ran) {  // the engine refused (placement / barrier timeout): nothing is lost, the plain loop repeats the run
        h->last_engine = LOOP_SIX;
        LZ_TRY(run_loop_six(h, n));
      }
      break;
    }
#endif
    case LOOP_FUSED_SMALL: LZ_TRY(run_loop_fused_small(h, n)); break;
    case LOOP_THREE_TERM_FUSED: LZ_TRY(run_loop_three_term_fused(h, n)); break;
    case LOOP_ONE_REDUCE: LZ_TRY(run_loop_onereduce(h, n)); break;
    case LOOP_PARTIAL_DEVICE: LZ_TRY(run_loop_partial_device(h, n)); break;
    case LOOP_PARTIAL_ONE_REDUCE: LZ_TRY(run_loop_partial_onereduce(h, n)); break;
    case LOOP_ONE_SWEEP:
      tried_pairs = one_sweep_pair_applies(h, n);
      tried_quads = one_sweep_quad_applies(h, n);  // (its tail of two steps is a pair: both flags are read)
      LZ_TRY(tried_quads   ? run_loop_one_sweep_quad(h, n)
             : tried_pairs ? run_loop_one_sweep_pair(h, n)
             : one_sweep_fused_applies(h, n) ? run_loop_one_sweep_fused(h, n)
                                             : run_loop_one_sweep(h, n));
      break;
    default: LZ_TRY(run_loop_six(h, n)); break;
  }
  double onered_bad = 0.0;
  int pair_flag = 0, quad_flag = 0;
  std::vector<int> dev_log(loop == LOOP_PARTIAL_DEVICE ? omega_state_ints(n) : loop == LOOP_PARTIAL_ONE_REDUCE ? omega_onered_ints(n) : 0);
  std::vector<RunExtra> extras;
  if (one_reduce) extras.push_back({&onered_bad, h->d_nrm2 + 1, sizeof(double)});
  if (loop == LOOP_ONE_SWEEP) extras.push_back({&h->last_gate_trips, h->d_osi + 1, sizeof(int)});
  if (tried_pairs) extras.push_back({&pair_flag, h->d_osi + 3, sizeof(int)});
  if (tried_quads) extras.push_back({&quad_flag, h->d_osi + 4, sizeof(int)});
  if (!dev_log.empty()) extras.push_back({dev_log.data(), h->d_omi, dev_log.size() * sizeof(int)});
  LZ_TRY(fr.drain(alpha_out, beta_out, extras));
  if (loop == LOOP_SIX && (h->flags & LZ_FLAG_REORTH_PARTIAL)) h->sweep_log.clear();  // (the host-decided loop keeps no per-step record)
  if (!dev_log.empty()) account_partial_device(h, n, dev_log, loop == LOOP_PARTIAL_DEVICE ? 2 : 4);
  if (loop == LOOP_PARTIAL_ONE_REDUCE) h->last_misses = dev_log[3];
  if (one_reduce && onered_bad != 0.0) {
    // cancellation guard of the one-reduce loop (k_onereduce_prepare): |r|^2 = r''.r'' - 2 alpha u.r'' + alpha^2 u.u lost too
    // many digits at some step (|alpha| >> beta).  Every rank sees the same reduced sums, so every rank takes this branch:
    // the solve is repeated on the default loop (two all-reduces per iteration), whose coefficients hold the bar.
    h->flags &= ~LZ_FLAG_ONE_REDUCE;
    *again = true;
    return LZ_OK;
  }
  if (quad_flag) {
    // a group's prediction missed by more than kOneSweepTau (k_os_quad_post): a group has no correcting sweep, so the whole solve is
    // repeated on the pair form (which may itself fall back to the single form); remembered until the matrix is set again
    h->quad_tripped = true;
    *again = true;
    return LZ_OK;
  }
  if (pair_flag) {
    // a pair's prediction missed by more than kOneSweepTau (k_os_pair_post): a pair has no correcting sweep, so the whole solve is
    // repeated on the single fused form, whose gate corrects such steps; remembered until the matrix is set again
    h->pair_tripped = true;
    *again = true;
    return LZ_OK;
  }
  if (getenv("LZ_DEBUG_TIMING"))
    fprintf(stderr, "[lz_run] alloc+memset %.3f ms, v0 upload %.3f ms, enqueue loop %.3f ms, drain+D2H %.3f ms\n", fr.t1 - fr.t0, fr.t2 - fr.t1,
            fr.t3 - fr.t2, RunFrame::now() - fr.t3);
  return fr.finish(alpha_out, beta_out);
}

}  // namespace api
}  // namespace lz

extern "C" {

// ---- early allocation of the big buffers ---------------------------------------------------------------------------------
int lz_reserve(lz_handle h, int64_t rows_local, int n, int with_ritz) {
  if (!h) return LZ_ERR_ARG;
  if (rows_local <= 0 || n < 1) return fail(nullptr, LZ_ERR_ARG, "lz_reserve: bad sizes");
  if (hipSetDevice(h->dev) != hipSuccess) return LZ_ERR_HIP;  // (h->err belongs to the thread that drives the handle: not written here)
  const int64_t rows_pad = round_up(rows_local, kPadDoubles);
  const size_t vsz = (size_t)n * (size_t)skew_stride(h, rows_pad);
  const size_t ysz = y_doubles(rows_local, n);
  // One buffer at a time: decide under the lock, allocate / free OUTSIDE it (a device allocation may take seconds and a free
  // synchronises the device: lz_run's basis_alloc and lz_ritz_vectors take the same lock to adopt a buffer), publish under the lock.
  // with_ritz: 0 the basis only, 1 both, 2 the Ritz vectors only (the helper thread's second call used to re-check the
  // basis and could strand a second 8 n M bytes once basis_alloc had adopted the first).
  auto reserve_one = [&](double*& slot, size_t& slot_count, size_t want) {
    double* stale = nullptr;
    {
      std::lock_guard<std::mutex> lk(h->res_mu);
      if (slot && slot_count >= want) return;
      stale = slot;
      slot = nullptr;
      slot_count = 0;
    }
    if (stale) (void)big_free(stale);
    size_t free_b = 0, total_b = 0;
    // leave room for the matrix, its layouts and the work vectors: reserve only what leaves a quarter of the device free
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || want * sizeof(double) + total_b / 4 > free_b) return;
    void* p = nullptr;
    if (big_alloc(h->dev, &p, want * sizeof(double)) != hipSuccess) {
      (void)hipGetLastError();
      return;  // not an error: basis_alloc / lz_ritz_vectors allocate (and report) themselves
    }
    double* loser = nullptr;
    {
      std::lock_guard<std::mutex> lk(h->res_mu);
      if (slot) {
        loser = static_cast<double*>(p);  // (another reserve call got there first)
      } else {
        slot = static_cast<double*>(p);
        slot_count = want;
      }
    }
    if (loser) (void)big_free(loser);
  };
  if (with_ritz != 2) reserve_one(h->res_V, h->res_V_count, vsz);
  if (with_ritz) reserve_one(h->res_Y, h->res_Y_count, ysz);
  return LZ_OK;
}

// ---- the run -----------------------------------------------------------------------
int lz_run(lz_handle h, int n, const double* v0_local, double* alpha_out, double* beta_out) {
  if (!h) return LZ_ERR_ARG;
  if (!v0_local || !alpha_out || !beta_out) return fail(h, LZ_ERR_ARG, "lz_run: NULL buffer");
  if (n < 2) return fail(h, LZ_ERR_ARG, "lz_run: n must be >= 2 (the reference's beta array has n-1 entries)");
  if (n > h->Mg) return fail(h, LZ_ERR_ARG, "lz_run: n cannot be larger than M");
  const int keep = h->flags;
  const bool tripped = h->pair_tripped, qtripped = h->quad_tripped;
  bool again = false;
  int rc;
  do rc = run_once(h, n, v0_local, alpha_out, beta_out, &again);  // a second pass where the first one's own check asks for it
  while (again);
  if (h->pair_tripped != tripped) h->last_pair_abandoned = 1;
  if (h->quad_tripped != qtripped) h->last_quad_abandoned = 1;
  if (h->flags != keep) h->last_engine = LOOP_ONE_REDUCE_REPEATED;
  h->flags = keep;
  return rc;
}

/* ---- checkpoint / resume ("Optional: dump (alpha, beta, j, V[:j])") ---------------------------------- */
int lz_get_residual(lz_handle h, double* r_local) {
  if (!h || !r_local) return LZ_ERR_ARG;
  LZ_TRY(require_basis(h, 0));
  LZ_HIP(h, hipSetDevice(h->dev));
  const int n = h->n;
  if (h->r_state == 2) {
    // the three- / five-launch loops leave y = A v_{n-1} behind: their three-term recurrence rides in the NEXT step's pass 1.
    // Form r = (y - alpha_{n-1} v_{n-1}) - beta_{n-2} v_{n-2} now, with the same kernel and expression (Lanczos.py:119).
    LZ_TRY(step_three_term(h, n - 1, n - 2, h->d_alpha + (n - 1), h->d_beta + (n - 2), false, nullptr, nullptr, "three_term(residual)"));
    h->r_state = 1;
  }
  if (h->r_state != 1)
    return fail(h, LZ_ERR_STATE, "lz_get_residual: the last run left no residual (run lz_run first; not after the one-reduce loop or lz_run_two_sided)");
  LZ_HIP(h, hipMemcpyAsync(r_local, h->d_r, (size_t)h->rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_get_omega_state(lz_handle h, double* out, int64_t count) {
  if (!h || !out) return LZ_ERR_ARG;
  if (h->last_engine != LOOP_PARTIAL_DEVICE || !h->d_om || h->om_run_n < 2)
    return fail(h, LZ_ERR_STATE, "lz_get_omega_state: the last run was not the device-decided partial re-orthogonalisation loop (engine 7)");
  if (count != (int64_t)omega_state_doubles(h->om_run_n)) return fail(h, LZ_ERR_ARG, "lz_get_omega_state: count must be 2 + (n + 2) + 3 (n + 1) for the n of the last run");
  LZ_HIP(h, hipSetDevice(h->dev));
  LZ_HIP(h, hipMemcpyAsync(out, h->d_om, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_run_resume_partial(lz_handle h, int n, int j0, const double* V_rows, int64_t ldv_in, const double* r_local, const double* alpha_in,
                          const double* beta_in, const double* omega_state, double* alpha_out, double* beta_out) {
  if (!h) return LZ_ERR_ARG;
  if (!V_rows || !r_local || !alpha_in || !beta_in || !omega_state || !alpha_out || !beta_out) return fail(h, LZ_ERR_ARG, "lz_run_resume_partial: NULL buffer");
  if (j0 < 2 || n <= j0) return fail(h, LZ_ERR_ARG, "lz_run_resume_partial: need 2 <= j0 < n (j0 completed steps, n in total)");
  if (n > h->Mg) return fail(h, LZ_ERR_ARG, "lz_run_resume_partial: n cannot be larger than M");
  if (ldv_in < h->rows) return fail(h, LZ_ERR_ARG, "lz_run_resume_partial: ldv_in < rows_local");
  if (!(h->flags & LZ_FLAG_REORTH_PARTIAL) || (h->flags & LZ_FLAG_ONE_REDUCE))
    return fail(h, LZ_ERR_STATE, "lz_run_resume_partial: needs LZ_FLAG_REORTH_PARTIAL without LZ_FLAG_ONE_REDUCE (the device-decided loop, engine 7)");
  // (a refused call leaves the handle as the last run left it: the check comes before the frame, on the plan basis_alloc will make for
  // n rows, and that plan is not stored - h->qplan has to match the allocation the single steps launch into)
  const QtwPlan plan = plan_qtw(h->rows_pad, h->flags, h->tune, n);
  if (h->kind != 0 && choose_loop(h, n, &plan) != LOOP_PARTIAL_DEVICE)
    return fail(h, LZ_ERR_STATE, "lz_run_resume_partial: these options / knobs do not select the device-decided partial loop");
  RunFrame fr{h, n};
  LZ_TRY(fr.begin(j0));  // (all j0 uploaded rows cleared first: see lz_run_resume)
  LZ_TRY(upload_checkpoint(h, j0, V_rows, ldv_in, r_local, alpha_in, beta_in));
  LZ_TRY(fr.uploaded());
  h->last_engine = LOOP_PARTIAL_DEVICE;
  LZ_TRY(run_loop_partial_device(h, n, j0, omega_state));
  std::vector<int> dev_log(omega_state_ints(n));
  LZ_TRY(fr.drain(alpha_out, beta_out, {{dev_log.data(), h->d_omi, dev_log.size() * sizeof(int)}}));
  account_partial_device(h, n, dev_log, 2);  // (the steps of the first leg are not on this record)
  return fr.finish(alpha_out, beta_out);
}

int lz_run_resume(lz_handle h, int n, int j0, const double* V_rows, int64_t ldv_in, const double* r_local, const double* alpha_in,
                  const double* beta_in, double* alpha_out, double* beta_out) {
  if (!h) return LZ_ERR_ARG;
  if (!V_rows || !r_local || !alpha_in || !beta_in || !alpha_out || !beta_out) return fail(h, LZ_ERR_ARG, "lz_run_resume: NULL buffer");
  if (j0 < 1 || n <= j0) return fail(h, LZ_ERR_ARG, "lz_run_resume: need 1 <= j0 < n (j0 completed steps, n in total)");
  if (n > h->Mg) return fail(h, LZ_ERR_ARG, "lz_run_resume: n cannot be larger than M");
  if (ldv_in < h->rows) return fail(h, LZ_ERR_ARG, "lz_run_resume: ldv_in < rows_local");
  if (h->flags & (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE))
    return fail(h, LZ_ERR_STATE, "lz_run_resume: not with partial re-orthogonalisation (lz_run_resume_partial continues the device-decided loop from its omega state) or the one-reduce loop");
  // The j0 rows about to be uploaded are cleared whole: the upload writes `rows` columns of each, the kernels stream rows_pad of them,
  // and a recycled allocation's padding would enter ||r||^2 (a run's own kernels write the padding of every row they produce: zeros).
  RunFrame fr{h, n};
  LZ_TRY(fr.begin(j0));
  LZ_TRY(upload_checkpoint(h, j0, V_rows, ldv_in, r_local, alpha_in, beta_in));
  LZ_TRY(fr.uploaded());
  h->last_engine = LOOP_SIX;  // every loop structure gives the same bits (tests/test_gpu_small.py): the plain one takes a start step
  LZ_TRY(run_loop_six(h, n, j0));
  LZ_TRY(fr.drain(alpha_out, beta_out));
  return fr.finish(alpha_out, beta_out);
}

/* ---- one loop body of the one-sweep loop on a state set from the host (include/lanczos_hip.h) ------------------------------ */
int lz_os_state_set(lz_handle h, int j, const double* G, const double* H, const double* chat, double alpha_prev, double beta_prev,
                    double beta_prev2) {
  if (!h) return LZ_ERR_ARG;
  if (!G || !H || !chat) return fail(h, LZ_ERR_ARG, "lz_os_state_set: NULL buffer");
  LZ_TRY(require_basis(h, 0));
  LZ_HIP(h, hipSetDevice(h->dev));
  return one_sweep_state_set(h, j, G, H, chat, alpha_prev, beta_prev, beta_prev2);
}

int lz_os_step(lz_handle h, int form, int j, int wide, int* blocks_out) {
  if (!h) return LZ_ERR_ARG;
  LZ_TRY(require_basis(h, 0));
  LZ_HIP(h, hipSetDevice(h->dev));
  return one_sweep_step_run(h, form, j, wide != 0, blocks_out);
}

int lz_os_state_get(lz_handle h, int form, int j, double* G, double* H, double* chat, double* g, double* gq, double* d, double* elog,
                    double* alpha, double* beta, double* nrm2, double* r2_local, int* ist, int* ldg_out, int* ldp_out) {
  if (!h) return LZ_ERR_ARG;
  LZ_TRY(require_basis(h, 0));
  LZ_HIP(h, hipSetDevice(h->dev));
  return one_sweep_state_get(h, form, j, G, H, chat, g, gq, d, elog, alpha, beta, nrm2, r2_local, ist, ldg_out, ldp_out);
}

int lz_os_raw_get(lz_handle h, int j0, int count, double* rows, double* part, int64_t part_count) {
  if (!h) return LZ_ERR_ARG;
  LZ_TRY(require_basis(h, 0));
  LZ_HIP(h, hipSetDevice(h->dev));
  return one_sweep_raw_get(h, j0, count, rows, part, part_count);
}

}  // extern "C"
