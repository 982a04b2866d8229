// C ABI of the thick-restart Lanczos solver (include/lanczos_hip.h, "thick-restart Lanczos"): the device half of lanczos_amd.eigsh.
// The basis is a buffer of its own (h->trl: trl_m + trl_b rows); the fixed-n run's V / Y on the same handle are untouched.
// What is here is the solver's own: the operator (A or a polynomial of A), the band batch, the restart, the residuals and the Rayleigh
// quotient.  Orthogonalising a vector against the basis and storing it, the gated two-pass step of an extension and the row transfers
// are the basis layer's (lz_orth.hip), shared with the Golub-Kahan-Lanczos solver and the complex thick-restart solver.
#include "lz_context.h"

using namespace lz;
using namespace lz::api;

namespace {

// trl_wk.sm: the basis layer's head (c of both passes, nrm2), the projected rows (m x m; band: m x (m + b)), beta (m), the restart's
// S (m x m), theta, the residual norms and the imaginary parts of lz_trl_residuals_cplx (m each); band only: the block coefficients of both passes ((m + b) x b each) and the b
// squared norms of a batch
struct TrlSmall : OrthSmallHead {
  int64_t proj, beta, S, theta, res, im, C1, C2, nrmb, total;
  int ldf;  // row length of proj
};
TrlSmall trl_small_layout(int m, int b = 1) {
  TrlSmall L;
  static_cast<OrthSmallHead&>(L) = orth_small_head(m + b);
  L.ldf = b > 1 ? m + b : m;
  L.proj = L.end;
  L.beta = L.proj + (int64_t)m * L.ldf;
  L.S = L.beta + m + 8;
  L.theta = L.S + (int64_t)m * m;
  L.res = L.theta + m;
  L.im = L.res + m + 8;
  L.C1 = L.im + m + 8;
  const int64_t cb = b > 1 ? trl_band_run(m + b, b) + 16 : 0;
  L.C2 = L.C1 + cb;
  L.nrmb = L.C2 + cb;
  L.total = L.nrmb + (b > 1 ? 16 : 0);
  return L;
}
TrlSmall trl_small_layout(lz_handle h) { return trl_small_layout(h->trl_m, h->trl_b); }

int trl_state(lz_handle h, const char* who) {
  if (!h) return LZ_ERR_ARG;
  if (!h->trl.B) return fail(h, LZ_ERR_STATE, std::string(who) + ": no thick-restart basis (lz_trl_begin first)");
  if (h->kind == 0 || skew_stride(h, h->rows_pad) != h->trl.ld) return fail(h, LZ_ERR_STATE, std::string(who) + ": the matrix changed since lz_trl_begin");
  // the view follows the matrix set last (one of another row count passes the test above where it pads to the same length): every
  // entry point behind lz_trl_begin comes through here before it touches h->trl (see OrthBasis, lz_context.h)
  h->trl.len = h->rows;
  h->trl.pad = h->rows_pad;
  LZ_HIP(h, hipSetDevice(h->dev));
  return LZ_OK;
}

// out = A x or, with a polynomial set (h->poly), p(A) x (x: a device vector of trl.ld doubles with a zero-or-ignored padding, never
// written; out: trl.w, or a work vector of a band batch).  The recurrence runs through three rotating work vectors (out and the two of
// poly.d_rot) so that step d lands in out;
// every product is the plain SpMV / GEMV launch, every recurrence step one streaming kernel in place on that product.
// Filter: the scaled Chebyshev recurrence, one k_cheb_step per step.  Series: sum_i mu_i T_i, the same rotation for the terms and the
// running sum in poly.d_acc beside them (k_cheb_series_step); the last term is only added, never stored, and the sum goes to its slot, out.
void trl_matvec(lz_handle h, const double* x, double* y) {
  if (h->kind == 1)
    launch_spmv_csr(h->csr, x, y, x, h->trl_wk.part, h->flags, h->stream);
  else
    launch_gemv_dense(h->d_dense, h->rows, h->ncols_ext, h->dense_lda, x, x, y, h->trl_wk.part, h->stream);
}
void trl_apply_op(lz_handle h, const double* x, double* out) {
  const TrlPoly& P = h->poly;
  if (P.kind == TrlPoly::kNone) {
    trl_matvec(h, x, out);
    return;
  }
  const int d = P.degree;
  const bool series = P.kind == TrlPoly::kSeries;
  // fixed-K stencil matrices whose SpMV is the ELL kernel: the step is that kernel's epilogue (filter: 24 B of vectors per row beside
  // the matrix instead of 8 + 32; series: 40 instead of 16 + 48), same bits; LZ_FLAG_TRL_FILTER_UNFUSED keeps the two launches
  const bool fused = h->kind == 1 && h->csr.ell_default && ell_usable(h->csr, h->flags) && !(h->flags & LZ_FLAG_TRL_FILTER_UNFUSED);
  double* bufs[3] = {out, P.d_rot, P.d_rot + P.ld};
  const double* prev = x;  // x of the recurrence (filter of degree 1: unused, b = 0)
  const double* cur = x;   // y of the recurrence
  for (int i = 1; i <= d; ++i) {
    double* z = bufs[(i - d) % 3 == 0 ? 0 : 3 + (i - d) % 3];  // step d -> out
    const bool last = series && i == d;
    if (fused) {
      SpmvCheb ch;
      ch.xprev = prev;
      ch.z = last ? nullptr : z;
      ch.coef = P.d_coef;
      ch.i = series ? i : i - 1;  // mu[i]; a[i - 1], b[i - 1]
      ch.degree = d;
      ch.c = P.c;
      if (series) {
        ch.inv_e = P.inv_e;
        ch.acc_in = P.d_acc;
        ch.acc = last ? out : P.d_acc;
      }
      launch_spmv_ell(h->csr, cur, z, cur, h->trl_wk.part, h->stream, nullptr, &ch);
    } else {
      trl_matvec(h, cur, z);
      if (series)
        launch_cheb_series_step(z, cur, prev, P.d_acc, P.d_acc, P.d_coef, i, last, P.inv_e, P.c, h->rows, h->rows_pad, h->stream);
      else
        launch_cheb_step(z, cur, prev, P.d_coef, i - 1, d, P.c, h->rows, h->rows_pad, h->stream);
    }
    prev = cur;
    cur = z;
  }
}

// The one place that sets h->poly (degree 0: clears it): the coefficients are coef0[0 .. n0) followed by coef1[0 .. n1).
int trl_set_poly(lz_handle h, TrlPoly::Kind kind, int degree, const double* coef0, size_t n0, const double* coef1, size_t n1, double c,
                 double inv_e) {
  TrlPoly& P = h->poly;
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  P.clear();  // one polynomial at a time: setting (or clearing) either kind drops what was set
  if (degree == 0) return LZ_OK;
  if (!P.d_rot || P.ld != h->trl.ld) {
    LZ_TRY(dev_free(h, P.d_acc));  // (of the old row length)
    LZ_TRY(dev_alloc(h, P.d_rot, 2 * (size_t)h->trl.ld));
    P.ld = h->trl.ld;
  }
  if (kind == TrlPoly::kSeries && !P.d_acc) LZ_TRY(dev_alloc(h, P.d_acc, (size_t)P.ld));
  if ((size_t)P.coef_cap < n0 + n1) {
    LZ_TRY(dev_alloc(h, P.d_coef, n0 + n1));
    P.coef_cap = (int)(n0 + n1);
  }
  LZ_HIP(h, hipMemsetAsync(P.d_rot, 0, 2 * (size_t)P.ld * sizeof(double), h->stream));
  if (kind == TrlPoly::kSeries) LZ_HIP(h, hipMemsetAsync(P.d_acc, 0, (size_t)P.ld * sizeof(double), h->stream));
  LZ_TRY(upload(h, P.d_coef, coef0, n0 * sizeof(double)));
  if (n1) LZ_TRY(upload(h, P.d_coef + n0, coef1, n1 * sizeof(double)));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  P.kind = kind;
  P.degree = degree;
  P.c = c;
  P.inv_e = inv_e;
  return LZ_OK;
}

// The basis of m + b rows (b = 1: lz_trl_begin; b >= 2: the band form), its work vectors and small arrays: allocated when m, b or the
// row length changed, zeroed always.
int trl_alloc(lz_handle h, int m, int b, const char* who) {
  const std::string w(who);
  if (h->kind == 0) return fail(h, LZ_ERR_STATE, w + ": no matrix set");
  if (h->world > 1 || h->comm_kind != 0)
    return fail(h, LZ_ERR_STATE, w + ": the thick-restart solver runs on one rank (this handle has a communicator)");
  if (h->flags & (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE))
    return fail(h, LZ_ERR_STATE, w + ": not with LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE");
  if (b == 1 && (m < 2 || m > 128 || m > h->rows)) return fail(h, LZ_ERR_ARG, w + ": need 2 <= m <= min(128, rows)");
  if (b > 1 && (m < b || m > 128 || m + b > h->rows)) return fail(h, LZ_ERR_ARG, w + ": need b <= m <= min(128, rows - b)");
  LZ_HIP(h, hipSetDevice(h->dev));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  const int64_t ld = skew_stride(h, h->rows_pad);
  const size_t nrows = (size_t)(m + b);
  if (!h->trl.B || h->trl_m != m || h->trl_b != b || h->trl.ld != ld) {
    h->poly.clear();  // its work vectors belong to the old row length
    LZ_TRY(dev_alloc(h, h->trl.B, nrows * (size_t)ld));
    LZ_TRY(dev_alloc(h, h->trl.w, (size_t)ld));
    if (b > 1)
      LZ_TRY(dev_alloc(h, h->d_tW, (size_t)b * (size_t)ld));
    else
      LZ_TRY(dev_free(h, h->d_tW));
    LZ_TRY(dev_alloc(h, h->trl_wk.sm, (size_t)trl_small_layout(m, b).total));
    LZ_TRY(dev_alloc(h, h->trl_wk.gate, 4));
    h->trl_m = m;
    h->trl_b = b;
    h->trl.ld = ld;
    h->trl.nrows = m + b;
  }
  h->trl.len = h->rows;
  h->trl.pad = h->rows_pad;
  size_t need = orth_part_need(h->trl, orth_plan(h, h->trl), m);
  need = std::max<size_t>(need, (size_t)h->rows / 4 + 64);  // dense GEMV / scalar SpMV partials
  need = std::max<size_t>(need, (size_t)h->csr.n_rowblk + 64);
  if (h->csr.pb) need = std::max<size_t>(need, (size_t)pb_num_partials(h->csr.pb) + 64);
  // residual norms + a dense product's partials + the second product of a conjugate pair (lz_trl_residuals_cplx, dense)
  need = std::max<size_t>(need, (size_t)m * (size_t)((h->rows + kTPB - 1) / kTPB) + (size_t)h->rows / 4 + 64 + (size_t)h->rows_pad + 64);
  if (b > 1) {  // the block Gram-Schmidt's coefficient runs and squared-norm partials
    need = std::max<size_t>(need, (size_t)trl_band_dots_blocks(h->rows_pad, b) * (size_t)trl_band_run(m + b, b));
    need = std::max<size_t>(need, (size_t)b * (size_t)trl_band_update_blocks(h->rows_pad));
  }
  LZ_TRY(orth_part_reserve(h, h->trl_wk, need));
  LZ_HIP(h, hipMemsetAsync(h->trl.B, 0, nrows * (size_t)ld * sizeof(double), h->stream));
  if (b > 1) LZ_HIP(h, hipMemsetAsync(h->d_tW, 0, (size_t)b * (size_t)ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(h->trl_wk.sm, 0, (size_t)trl_small_layout(m, b).total * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(h->trl_wk.gate, 0, 4 * sizeof(int), h->stream));
  return LZ_OK;
}

// V[k] = x made orthogonal to V[0..k), normalised
int trl_store_x(lz_handle h, int k, const double* x) {
  LZ_TRY(orth_upload_x(h, h->trl, x));
  return orth_store(h, h->trl, h->trl_wk, orth_plan(h, h->trl), k, "trl orthogonalise");
}

}  // namespace

extern "C" {

int lz_trl_begin(lz_handle h, int m, const double* v0) {
  if (!h || !v0) return LZ_ERR_ARG;
  LZ_TRY(trl_alloc(h, m, 1, "lz_trl_begin"));
  return trl_store_x(h, 0, v0);
}

int lz_trl_begin_band(lz_handle h, int m, int b, const double* X) {
  if (!h || !X) return LZ_ERR_ARG;
  if (b < 2 || b > 8) return fail(h, LZ_ERR_ARG, "lz_trl_begin_band: need 2 <= b <= 8");
  LZ_TRY(trl_alloc(h, m, b, "lz_trl_begin_band"));
  for (int i = 0; i < b; ++i) LZ_TRY(trl_store_x(h, i, X + (int64_t)i * h->rows));
  return LZ_OK;
}

int lz_trl_extend(lz_handle h, int k, int m, double* proj_out, double* beta_out) {
  LZ_TRY(trl_state(h, "lz_trl_extend"));
  if (h->trl_b != 1) return fail(h, LZ_ERR_STATE, "lz_trl_extend: the basis was begun as a band (lz_trl_extend_band)");
  if (m != h->trl_m || k < 0 || k >= m) return fail(h, LZ_ERR_ARG, "lz_trl_extend: need m == the m of lz_trl_begin and 0 <= k < m");
  const TrlSmall L = trl_small_layout(h);
  const OrthBasis& V = h->trl;
  double* sm = h->trl_wk.sm;
  const QtwPlan plan = orth_plan(h, V);
  const OrthPass2 pass2 = (h->flags & LZ_FLAG_TRL_PASS2_ALWAYS) ? OrthPass2::kForced : OrthPass2::kGated;
  for (int j = k; j < m; ++j) {
    trl_apply_op(h, V.B + (int64_t)j * V.ld, V.w);  // w = A V[j], or p(A) V[j] with a filter set
    // w against V[0..j]: row j of the projection; beta_j = |w|, V[j + 1] = w / beta_j
    LZ_TRY(orth_cgs_step(h, V, h->trl_wk, plan, j + 1, sm + L.proj + (int64_t)j * m, sm + L.beta + j, pass2));
    LZ_TRY(check_launch(h, "trl extend"));
  }
  if (proj_out) LZ_HIP(h, hipMemcpyAsync(proj_out, sm + L.proj, (size_t)m * m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (beta_out) LZ_HIP(h, hipMemcpyAsync(beta_out, sm + L.beta, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_trl_extend_band(lz_handle h, int k, int m, double* proj_out, double* beta_out) {
  LZ_TRY(trl_state(h, "lz_trl_extend_band"));
  if (h->trl_b < 2) return fail(h, LZ_ERR_STATE, "lz_trl_extend_band: the basis was begun without a band (lz_trl_begin_band first)");
  if (m != h->trl_m || k < 0 || k >= m) return fail(h, LZ_ERR_ARG, "lz_trl_extend_band: need m == the m of lz_trl_begin_band and 0 <= k < m");
  const int b = h->trl_b;
  const TrlSmall L = trl_small_layout(h);
  double* V = h->trl.B;
  double* W = h->d_tW;
  double* sm = h->trl_wk.sm;
  const int64_t ld = h->trl.ld;
  const QtwPlan plan = orth_plan(h, h->trl);
  // the sweeps stream rows_pad, the products write rows: a breakdown in an earlier call (0 / 0 behind a vanished residual) may have left
  // NaN in a work vector's padding, which no product would clear
  if (h->rows_pad > h->rows)
    for (int i = 0; i < b; ++i)
      LZ_HIP(h, hipMemsetAsync(W + (int64_t)i * ld + h->rows, 0, (size_t)(h->rows_pad - h->rows) * sizeof(double), h->stream));
  for (int j = k; j < m; j += b) {
    const int nb = std::min(b, m - j);  // steps j .. j + nb - 1: they need rows below r0 only, which all exist
    const int r0 = j + b;
    for (int i = 0; i < nb; ++i) trl_apply_op(h, V + (int64_t)(j + i) * ld, W + (int64_t)i * ld);  // w_i = A V[j + i], or p(A) V[j + i]
    // block CGS against V[0..r0), two passes: every row is read once per sweep for all b work vectors (a short last batch sweeps the stale
    // ones too: their coefficients are never read)
    const int G = trl_band_dots_blocks(h->rows_pad, b);
    const int run = trl_band_run(r0, b);
    int nu = 0;
    for (int pass = 0; pass < 2; ++pass) {
      double* C = sm + (pass == 0 ? L.C1 : L.C2);
      LZ_HIP(h, launch_trl_band_dots(V, ld, h->rows_pad, r0, W, ld, b, h->trl_wk.part, h->stream));
      launch_final_rows_t(h->trl_wk.part, G, run, r0 * b, C, h->stream);
      nu = launch_trl_band_update(V, ld, h->rows_pad, r0, C, W, ld, b, h->trl_wk.part, h->stream);
    }
    launch_final_rows(h->trl_wk.part, b, nu, sm + L.nrmb, h->stream);  // |w_i|^2 after the second pass
    launch_trl_band_proj(sm + L.C1, sm + L.C2, r0, b, nb, sm + L.proj + (int64_t)j * L.ldf, L.ldf, h->stream);
    // in-batch tail: w_i against the rows this batch has made so far (the single-vector step on a view based at row r0, both passes
    // always), then V[r0 + i] = w_i / |w_i|
    OrthBasis tail = h->trl;  // (nrows as the basis': the plan and the small arrays are the whole basis')
    tail.B = V + (int64_t)r0 * ld;
    for (int i = 0; i < nb; ++i) {
      tail.w = W + (int64_t)i * ld;
      if (i == 0)  // nothing new to orthogonalise against: the sweep's own norm
        launch_scale_store(tail.B, tail.w, sm + L.nrmb, sm + L.beta + j, h->rows_pad, h->stream);
      else
        LZ_TRY(orth_cgs_step(h, tail, h->trl_wk, plan, i, sm + L.proj + (int64_t)(j + i) * L.ldf + r0, sm + L.beta + j + i, OrthPass2::kUngated));
    }
    LZ_TRY(check_launch(h, "trl extend band"));
  }
  if (proj_out) LZ_HIP(h, hipMemcpyAsync(proj_out, sm + L.proj, (size_t)m * L.ldf * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (beta_out) LZ_HIP(h, hipMemcpyAsync(beta_out, sm + L.beta, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_trl_restart(lz_handle h, int m, int kk, const double* S) {
  LZ_TRY(trl_state(h, "lz_trl_restart"));
  if (!S || m != h->trl_m || kk < 1 || kk >= m) return fail(h, LZ_ERR_ARG, "lz_trl_restart: need m == the m of lz_trl_begin, 1 <= kk < m, S");
  const TrlSmall L = trl_small_layout(h);
  LZ_TRY(upload(h, h->trl_wk.sm + L.S, S, (size_t)m * kk * sizeof(double)));
  LZ_HIP(h, launch_trl_restart(h->trl.B, h->trl.ld, h->rows, m, kk, h->trl_wk.sm + L.S, h->stream));
  for (int r = 1; r < h->trl_b; ++r)  // band: the other residual rows follow V[m] (ascending: a destination is never a source still to be copied)
    LZ_HIP(h, hipMemcpyAsync(h->trl.B + (int64_t)(kk + r) * h->trl.ld, h->trl.B + (int64_t)(m + r) * h->trl.ld, (size_t)h->rows * sizeof(double),
                             hipMemcpyDeviceToDevice, h->stream));
  LZ_TRY(check_launch(h, "trl restart"));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_trl_probe(lz_handle h, int k, const double* x) {
  LZ_TRY(trl_state(h, "lz_trl_probe"));
  if (!x || k < 0 || k > h->trl_m + h->trl_b - 1) return fail(h, LZ_ERR_ARG, "lz_trl_probe: need 0 <= k <= m (band: m + b - 1) and x");
  return trl_store_x(h, k, x);
}

int lz_trl_get_vectors(lz_handle h, int k, double* Y_out) {
  LZ_TRY(trl_state(h, "lz_trl_get_vectors"));
  if (!Y_out || k < 1 || k > h->trl_m) return fail(h, LZ_ERR_ARG, "lz_trl_get_vectors: need 1 <= k <= m and Y_out");
  return orth_get_vectors(h, h->trl, k, Y_out);
}

int lz_trl_residuals(lz_handle h, int k, const double* theta, double* out) {
  LZ_TRY(trl_state(h, "lz_trl_residuals"));
  if (!theta || !out || k < 1 || k > h->trl_m) return fail(h, LZ_ERR_ARG, "lz_trl_residuals: need 1 <= k <= m, theta and out");
  const TrlSmall L = trl_small_layout(h);
  double* dth = h->trl_wk.sm + L.theta;
  LZ_TRY(upload(h, dth, theta, (size_t)k * sizeof(double)));
  if (h->kind == 1) {
    const int G = launch_trl_resid_csr(h->csr, h->trl.B, h->trl.ld, k, dth, h->trl_wk.part, h->stream);
    launch_trl_rownorm(h->trl_wk.part, G, k, h->trl_wk.sm + L.res, h->stream);
  } else {
    const int Gd = (int)((h->rows + kTPB - 1) / kTPB);  // the products' own partials lie behind the k rows of the norms'
    LZ_TRY(orth_resid_norms(h, h->trl, h->trl_wk, k, dth, h->trl_wk.sm + L.res, [&](int i) {
      const double* x = h->trl.B + (int64_t)i * h->trl.ld;
      launch_gemv_dense(h->d_dense, h->rows, h->ncols_ext, h->dense_lda, x, x, h->trl.w, h->trl_wk.part + (size_t)k * Gd, h->stream);
      return hipSuccess;
    }));
  }
  LZ_TRY(check_launch(h, "trl residuals"));
  LZ_HIP(h, hipMemcpyAsync(out, h->trl_wk.sm + L.res, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_trl_residuals_cplx(lz_handle h, int k, const double* re, const double* im, double* out) {
  LZ_TRY(trl_state(h, "lz_trl_residuals_cplx"));
  if (!re || !im || !out || k < 1 || k > h->trl_m) return fail(h, LZ_ERR_ARG, "lz_trl_residuals_cplx: need 1 <= k <= m, re, im and out");
  for (int i = 0; i < k; ++i) {  // every pair is whole before anything is launched
    if (im[i] == 0.0) continue;
    if (!(im[i] > 0.0) || i + 1 >= k || re[i + 1] != re[i] || im[i + 1] != -im[i])
      return fail(h, LZ_ERR_ARG, "lz_trl_residuals_cplx: im[i] > 0 needs its conjugate at i + 1 (re[i + 1] == re[i], im[i + 1] == -im[i], i + 1 < k)");
    ++i;
  }
  const TrlSmall L = trl_small_layout(h);
  double* dre = h->trl_wk.sm + L.theta;
  double* dimg = h->trl_wk.sm + L.im;
  LZ_TRY(upload(h, dre, re, (size_t)k * sizeof(double)));
  LZ_TRY(upload(h, dimg, im, (size_t)k * sizeof(double)));
  int G = 0;
  if (h->kind == 1) {
    G = launch_trl_resid_cplx_csr(h->csr, h->trl.B, h->trl.ld, k, dre, dimg, h->trl_wk.part, h->stream);
  } else {
    const int Gd = (int)((h->rows + kTPB - 1) / kTPB);
    double* gpart = h->trl_wk.part + (size_t)k * Gd;           // the products' own partials (not used)
    double* yi = gpart + (((size_t)h->rows / 4 + 64) & ~(size_t)1);  // A x_i of a pair (trl_alloc sized the partials for it)
    for (int i = 0; i < k; ++i) {
      const double* x = h->trl.B + (int64_t)i * h->trl.ld;
      launch_gemv_dense(h->d_dense, h->rows, h->ncols_ext, h->dense_lda, x, x, h->trl.w, gpart, h->stream);
      if (im[i] == 0.0) {
        G = launch_trl_resid_diff(h->trl.w, x, h->rows, dre, i, h->trl_wk.part, h->stream);
      } else {
        const double* xi = x + h->trl.ld;
        launch_gemv_dense(h->d_dense, h->rows, h->ncols_ext, h->dense_lda, xi, xi, yi, gpart, h->stream);
        G = launch_trl_resid_cplx_diff(h->trl.w, yi, x, xi, h->rows, dre, dimg, i, h->trl_wk.part, h->stream);
        ++i;
      }
    }
  }
  launch_trl_rownorm(h->trl_wk.part, G, k, h->trl_wk.sm + L.res, h->stream);
  LZ_TRY(check_launch(h, "trl residuals cplx"));
  LZ_HIP(h, hipMemcpyAsync(out, h->trl_wk.sm + L.res, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i + 1 < k; ++i)
    if (im[i] > 0.0) out[i + 1] = out[i];  // both members of a pair carry the pair's norm
  return LZ_OK;
}

int lz_trl_set_filter(lz_handle h, int degree, const double* a, const double* b, double c) {
  LZ_TRY(trl_state(h, "lz_trl_set_filter"));
  if (degree < 0 || degree > 4096 || (degree > 0 && (!a || !b))) return fail(h, LZ_ERR_ARG, "lz_trl_set_filter: need 0 <= degree <= 4096, a and b");
  return trl_set_poly(h, TrlPoly::kFilter, degree, a, (size_t)degree, b, (size_t)degree, c, 0.0);
}

int lz_trl_set_series(lz_handle h, int degree, const double* mu, double c, double e) {
  LZ_TRY(trl_state(h, "lz_trl_set_series"));
  if (degree < 0 || degree > 4096 || (degree > 0 && (!mu || !(e > 0.0) || !std::isfinite(c) || !std::isfinite(e))))
    return fail(h, LZ_ERR_ARG, "lz_trl_set_series: need 0 <= degree <= 4096, mu, a finite c and e > 0");
  return trl_set_poly(h, TrlPoly::kSeries, degree, mu, (size_t)degree + 1, nullptr, 0, c, 1.0 / e);
}

int lz_trl_filter_apply(lz_handle h, const double* x, double* y) {
  LZ_TRY(trl_state(h, "lz_trl_filter_apply"));
  if (!x || !y) return fail(h, LZ_ERR_ARG, "lz_trl_filter_apply: need x and y");
  if (h->poly.kind == TrlPoly::kNone)
    return fail(h, LZ_ERR_STATE, "lz_trl_filter_apply: no filter set (lz_trl_set_filter or lz_trl_set_series first)");
  double* vm = h->trl.B + (int64_t)h->trl_m * h->trl.ld;  // the residual row carries x and then the result
  LZ_TRY(upload(h, vm, x, (size_t)h->rows * sizeof(double)));
  trl_apply_op(h, vm, h->trl.w);
  LZ_TRY(check_launch(h, "trl filter apply"));
  LZ_HIP(h, hipMemcpyAsync(vm, h->trl.w, (size_t)h->rows_pad * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  LZ_HIP(h, hipMemcpyAsync(y, h->trl.w, (size_t)h->rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_trl_rayleigh(lz_handle h, int k, double* G_out) {
  LZ_TRY(trl_state(h, "lz_trl_rayleigh"));
  if (!G_out || k < 1 || k >= h->trl_m) return fail(h, LZ_ERR_ARG, "lz_trl_rayleigh: need 1 <= k < m and G_out");
  const TrlSmall L = trl_small_layout(h);
  const OrthBasis& V = h->trl;
  double* G = h->trl_wk.sm + L.S;  // k x k in the restart's S area
  const QtwPlan plan = orth_plan(h, V);
  for (int i = 0; i < k; ++i) {
    trl_matvec(h, V.B + (int64_t)i * V.ld, V.w);  // A itself, filter or not
    LZ_TRY(orth_dots(h, V, h->trl_wk, plan, k, h->trl_wk.sm + L.c1));
    LZ_HIP(h, hipMemcpyAsync(G + (int64_t)i * k, h->trl_wk.sm + L.c1, (size_t)k * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    LZ_TRY(check_launch(h, "trl rayleigh"));
  }
  LZ_HIP(h, hipMemcpyAsync(G_out, G, (size_t)k * k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_trl_set_rows(lz_handle h, int j0, int count, const double* rows, int64_t ld) {
  LZ_TRY(trl_state(h, "lz_trl_set_rows"));
  return orth_set_rows(h, h->trl, "lz_trl_set_rows", "m (band: m + b - 1)", j0, count, rows, ld);
}

int lz_trl_get_rows(lz_handle h, int j0, int count, double* rows, int64_t ld) {
  LZ_TRY(trl_state(h, "lz_trl_get_rows"));
  return orth_get_rows(h, h->trl, "lz_trl_get_rows", "m (band: m + b - 1)", j0, count, rows, ld);
}

}  // extern "C"
