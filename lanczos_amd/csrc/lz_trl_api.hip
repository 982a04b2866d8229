// C ABI of the thick-restart Lanczos solver (include/lanczos_hip.h, "thick-restart Lanczos"): the device half of lanczos_amd.eigsh.
// The basis is a buffer of its own (d_trl: trl_m + 1 rows of trl_ld doubles); the fixed-n run's V / Y on the same handle are untouched.
#include "lz_context.h"

using namespace lz;
using namespace lz::api;

namespace {

// d_tsm: c of pass 1 and of pass 2 (cl doubles each), nrm2 + a scratch beta slot, the projected rows (m x m), beta (m), the restart's
// S (m x m), theta and the residual norms (m each)
struct TrlSmall {
  int64_t c1, c2, nrm2, proj, beta, S, theta, res, total;
};
TrlSmall trl_small_layout(int m) {
  TrlSmall L;
  const int64_t cl = qtw_ldp(m + 2) + 16;
  L.c1 = 0;
  L.c2 = cl;
  L.nrm2 = 2 * cl;
  L.proj = L.nrm2 + 8;
  L.beta = L.proj + (int64_t)m * m;
  L.S = L.beta + m + 8;
  L.theta = L.S + (int64_t)m * m;
  L.res = L.theta + m;
  L.total = L.res + m + 8;
  return L;
}

QtwPlan trl_plan(lz_handle h) { return plan_qtw(h->rows_pad, h->flags & ~(LZ_FLAG_QTW_MFMA | LZ_FLAG_ONE_REDUCE), h->tune, h->trl_m + 2); }

int trl_state(lz_handle h, const char* who) {
  if (!h) return LZ_ERR_ARG;
  if (!h->d_trl) return fail(h, LZ_ERR_STATE, std::string(who) + ": no thick-restart basis (lz_trl_begin first)");
  if (h->kind == 0 || skew_stride(h, h->rows_pad) != h->trl_ld) return fail(h, LZ_ERR_STATE, std::string(who) + ": the matrix changed since lz_trl_begin");
  LZ_HIP(h, hipSetDevice(h->dev));
  return LZ_OK;
}

// V[k] = x (in d_tw) made orthogonal to V[0..k) by two CGS passes, then normalised
int trl_orth_store(lz_handle h, int k) {
  const TrlSmall L = trl_small_layout(h->trl_m);
  double* V = h->d_trl;
  const QtwPlan plan = trl_plan(h);
  int np = 0;
  for (int pass = 0; pass < (k > 0 ? 2 : 0); ++pass) {
    LZ_HIP(h, launch_qtw(V, h->trl_ld, h->rows_pad, k + 1, k, h->d_tw, nullptr, nullptr, plan, h->d_tpart, 2, h->stream));
    launch_final_rows(h->d_tpart, k + 1, plan.P, h->d_tsm + L.c1, h->stream, plan.family == 2);
    np = launch_trl_cgs(V, h->trl_ld, h->rows_pad, k, h->d_tsm + L.c1, h->d_tw, h->d_tpart, nullptr, h->stream);
  }
  if (k == 0) np = launch_trl_cgs(V, h->trl_ld, h->rows_pad, 0, h->d_tsm + L.c1, h->d_tw, h->d_tpart, nullptr, h->stream);  // |x|^2 only
  launch_trl_post(2, h->d_tpart, np, nullptr, 0, h->d_tsm + L.nrm2, nullptr, h->d_tgate, 0, h->stream);
  launch_scale_store(V + (int64_t)k * h->trl_ld, h->d_tw, h->d_tsm + L.nrm2, h->d_tsm + L.nrm2 + 1, h->rows_pad, h->stream);
  LZ_TRY(check_launch(h, "trl orthogonalise"));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int trl_upload_x(lz_handle h, const double* x) {
  LZ_HIP(h, hipMemsetAsync(h->d_tw, 0, (size_t)h->trl_ld * sizeof(double), h->stream));
  LZ_TRY(upload(h, h->d_tw, x, (size_t)h->rows * sizeof(double)));
  return LZ_OK;
}

// d_tw = A x or, with a polynomial set (h->poly), p(A) x (x: a device vector of trl_ld doubles with a zero-or-ignored padding, never
// written).  The recurrence runs through three rotating work vectors (d_tw and the two of poly.d_rot) so that step d lands in d_tw;
// every product is the plain SpMV / GEMV launch, every recurrence step one streaming kernel in place on that product.
// Filter: the scaled Chebyshev recurrence, one k_cheb_step per step.  Series: sum_i mu_i T_i, the same rotation for the terms and the
// running sum in poly.d_acc beside them (k_cheb_series_step); the last term is only added, never stored, and the sum goes to its slot, d_tw.
void trl_matvec(lz_handle h, const double* x, double* y) {
  if (h->kind == 1)
    launch_spmv_csr(h->csr, x, y, x, h->d_tpart, h->flags, h->stream);
  else
    launch_gemv_dense(h->d_dense, h->rows, h->ncols_ext, h->dense_lda, x, x, y, h->d_tpart, h->stream);
}
void trl_apply_op(lz_handle h, const double* x) {
  const TrlPoly& P = h->poly;
  if (P.kind == TrlPoly::kNone) {
    trl_matvec(h, x, h->d_tw);
    return;
  }
  const int d = P.degree;
  const bool series = P.kind == TrlPoly::kSeries;
  // fixed-K stencil matrices whose SpMV is the ELL kernel: the step is that kernel's epilogue (filter: 24 B of vectors per row beside
  // the matrix instead of 8 + 32; series: 40 instead of 16 + 48), same bits; LZ_FLAG_TRL_FILTER_UNFUSED keeps the two launches
  const bool fused = h->kind == 1 && h->csr.ell_default && ell_usable(h->csr, h->flags) && !(h->flags & LZ_FLAG_TRL_FILTER_UNFUSED);
  double* bufs[3] = {h->d_tw, P.d_rot, P.d_rot + P.ld};
  const double* prev = x;  // x of the recurrence (filter of degree 1: unused, b = 0)
  const double* cur = x;   // y of the recurrence
  for (int i = 1; i <= d; ++i) {
    double* z = bufs[(i - d) % 3 == 0 ? 0 : 3 + (i - d) % 3];  // step d -> d_tw
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
        ch.acc = last ? h->d_tw : P.d_acc;
      }
      launch_spmv_ell(h->csr, cur, z, cur, h->d_tpart, h->stream, nullptr, &ch);
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
  if (!P.d_rot || P.ld != h->trl_ld) {
    LZ_TRY(dev_free(h, P.d_acc));  // (of the old row length)
    LZ_TRY(dev_alloc(h, P.d_rot, 2 * (size_t)h->trl_ld));
    P.ld = h->trl_ld;
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

}  // namespace

extern "C" {

int lz_trl_begin(lz_handle h, int m, const double* v0) {
  if (!h || !v0) return LZ_ERR_ARG;
  if (h->kind == 0) return fail(h, LZ_ERR_STATE, "lz_trl_begin: no matrix set");
  if (h->world > 1 || h->comm_kind != 0)
    return fail(h, LZ_ERR_STATE, "lz_trl_begin: the thick-restart solver runs on one rank (this handle has a communicator)");
  if (h->flags & (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE))
    return fail(h, LZ_ERR_STATE, "lz_trl_begin: not with LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE");
  if (m < 2 || m > 128 || m > h->rows) return fail(h, LZ_ERR_ARG, "lz_trl_begin: need 2 <= m <= min(128, rows)");
  LZ_HIP(h, hipSetDevice(h->dev));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  const int64_t ld = skew_stride(h, h->rows_pad);
  if (!h->d_trl || h->trl_m != m || h->trl_ld != ld) {
    h->poly.clear();  // its work vectors belong to the old row length
    LZ_TRY(dev_alloc(h, h->d_trl, (size_t)(m + 1) * (size_t)ld));
    LZ_TRY(dev_alloc(h, h->d_tw, (size_t)ld));
    LZ_TRY(dev_alloc(h, h->d_tsm, (size_t)trl_small_layout(m).total));
    LZ_TRY(dev_alloc(h, h->d_tgate, 4));
    h->trl_m = m;
    h->trl_ld = ld;
  }
  const QtwPlan plan = trl_plan(h);
  size_t need = (size_t)(m + 2 + 32) * (size_t)plan.P;
  need = std::max<size_t>(need, (size_t)trl_cgs_blocks(h->rows_pad));
  need = std::max<size_t>(need, (size_t)h->rows / 4 + 64);  // dense GEMV / scalar SpMV partials
  need = std::max<size_t>(need, (size_t)h->csr.n_rowblk + 64);
  if (h->csr.pb) need = std::max<size_t>(need, (size_t)pb_num_partials(h->csr.pb) + 64);
  need = std::max<size_t>(need, (size_t)m * (size_t)((h->rows + kTPB - 1) / kTPB) + (size_t)h->rows / 4 + 64);  // residual norms
  need += 8192;
  if (need > h->tpart_cap) {
    LZ_TRY(dev_alloc(h, h->d_tpart, need));
    h->tpart_cap = need;
  }
  LZ_HIP(h, hipMemsetAsync(h->d_trl, 0, (size_t)(m + 1) * (size_t)ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(h->d_tsm, 0, (size_t)trl_small_layout(m).total * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(h->d_tgate, 0, 4 * sizeof(int), h->stream));
  LZ_TRY(trl_upload_x(h, v0));
  return trl_orth_store(h, 0);
}

int lz_trl_extend(lz_handle h, int k, int m, double* proj_out, double* beta_out) {
  LZ_TRY(trl_state(h, "lz_trl_extend"));
  if (m != h->trl_m || k < 0 || k >= m) return fail(h, LZ_ERR_ARG, "lz_trl_extend: need m == the m of lz_trl_begin and 0 <= k < m");
  const TrlSmall L = trl_small_layout(m);
  double* V = h->d_trl;
  double* sm = h->d_tsm;
  const int64_t ld = h->trl_ld;
  const QtwPlan plan = trl_plan(h);
  const int force = (h->flags & LZ_FLAG_TRL_PASS2_ALWAYS) != 0;
  QtwFuse gated;
  gated.gate = h->d_tgate;
  for (int j = k; j < m; ++j) {
    trl_apply_op(h, V + (int64_t)j * ld);  // w = A V[j], or p(A) V[j] with a filter set
    // pass 1: c = V[0..j] . w (row j + 1 is the self slot: c[j + 1] = w.w), w -= sum c_i V_i
    LZ_HIP(h, launch_qtw(V, ld, h->rows_pad, j + 2, j + 1, h->d_tw, nullptr, nullptr, plan, h->d_tpart, 2, h->stream));
    launch_final_rows(h->d_tpart, j + 2, plan.P, sm + L.c1, h->stream, plan.family == 2);
    int np = launch_trl_cgs(V, ld, h->rows_pad, j + 1, sm + L.c1, h->d_tw, h->d_tpart, nullptr, h->stream);
    launch_trl_post(0, h->d_tpart, np, sm + L.c1, j, sm + L.nrm2, sm + L.proj + (int64_t)j * m, h->d_tgate, force, h->stream);
    // pass 2, only where pass 1 cancelled more than half of |w| (or LZ_FLAG_TRL_PASS2_ALWAYS forces it)
    LZ_HIP(h, launch_qtw(V, ld, h->rows_pad, j + 2, j + 1, h->d_tw, nullptr, nullptr, plan, h->d_tpart, 2, h->stream, &gated));
    launch_final_rows(h->d_tpart, j + 2, plan.P, sm + L.c2, h->stream, plan.family == 2, h->d_tgate);
    np = launch_trl_cgs(V, ld, h->rows_pad, j + 1, sm + L.c2, h->d_tw, h->d_tpart, h->d_tgate, h->stream);
    launch_trl_post(1, h->d_tpart, np, sm + L.c2, j, sm + L.nrm2, sm + L.proj + (int64_t)j * m, h->d_tgate, force, h->stream);
    // beta = |w|, V[j + 1] = w / beta
    launch_scale_store(V + (int64_t)(j + 1) * ld, h->d_tw, sm + L.nrm2, sm + L.beta + j, h->rows_pad, h->stream);
    LZ_TRY(check_launch(h, "trl extend"));
  }
  if (proj_out) LZ_HIP(h, hipMemcpyAsync(proj_out, sm + L.proj, (size_t)m * m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (beta_out) LZ_HIP(h, hipMemcpyAsync(beta_out, sm + L.beta, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_trl_restart(lz_handle h, int m, int kk, const double* S) {
  LZ_TRY(trl_state(h, "lz_trl_restart"));
  if (!S || m != h->trl_m || kk < 1 || kk >= m) return fail(h, LZ_ERR_ARG, "lz_trl_restart: need m == the m of lz_trl_begin, 1 <= kk < m, S");
  const TrlSmall L = trl_small_layout(m);
  LZ_TRY(upload(h, h->d_tsm + L.S, S, (size_t)m * kk * sizeof(double)));
  LZ_HIP(h, launch_trl_restart(h->d_trl, h->trl_ld, h->rows, m, kk, h->d_tsm + L.S, h->stream));
  LZ_TRY(check_launch(h, "trl restart"));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_trl_probe(lz_handle h, int k, const double* x) {
  LZ_TRY(trl_state(h, "lz_trl_probe"));
  if (!x || k < 0 || k > h->trl_m) return fail(h, LZ_ERR_ARG, "lz_trl_probe: need 0 <= k <= m and x");
  LZ_TRY(trl_upload_x(h, x));
  return trl_orth_store(h, k);
}

int lz_trl_get_vectors(lz_handle h, int k, double* Y_out) {
  LZ_TRY(trl_state(h, "lz_trl_get_vectors"));
  if (!Y_out || k < 1 || k > h->trl_m) return fail(h, LZ_ERR_ARG, "lz_trl_get_vectors: need 1 <= k <= m and Y_out");
  std::vector<double> rowsk((size_t)k * (size_t)h->rows);
  LZ_HIP(h, xfer_d2h(h->dev, h->stream, h->xfer, rowsk.data(), (size_t)h->rows * sizeof(double), h->d_trl, (size_t)h->trl_ld * sizeof(double),
                     (size_t)h->rows * sizeof(double), (size_t)k));
  const int64_t M = h->rows;
  parallel_ranges(M, 1 << 16, [&](int, int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r)
      for (int i = 0; i < k; ++i) Y_out[r * k + i] = rowsk[(size_t)i * M + r];
  });
  return LZ_OK;
}

int lz_trl_residuals(lz_handle h, int k, const double* theta, double* out) {
  LZ_TRY(trl_state(h, "lz_trl_residuals"));
  if (!theta || !out || k < 1 || k > h->trl_m) return fail(h, LZ_ERR_ARG, "lz_trl_residuals: need 1 <= k <= m, theta and out");
  const TrlSmall L = trl_small_layout(h->trl_m);
  double* dth = h->d_tsm + L.theta;
  LZ_TRY(upload(h, dth, theta, (size_t)k * sizeof(double)));
  int G = 0;
  if (h->kind == 1) {
    G = launch_trl_resid_csr(h->csr, h->d_trl, h->trl_ld, k, dth, h->d_tpart, h->stream);
  } else {
    const int Gd = (int)((h->rows + kTPB - 1) / kTPB);
    for (int i = 0; i < k; ++i) {
      const double* x = h->d_trl + (int64_t)i * h->trl_ld;
      launch_gemv_dense(h->d_dense, h->rows, h->ncols_ext, h->dense_lda, x, x, h->d_tw, h->d_tpart + (size_t)k * Gd, h->stream);
      G = launch_trl_resid_diff(h->d_tw, x, h->rows, dth, i, h->d_tpart, h->stream);
    }
  }
  launch_trl_rownorm(h->d_tpart, G, k, h->d_tsm + L.res, h->stream);
  LZ_TRY(check_launch(h, "trl residuals"));
  LZ_HIP(h, hipMemcpyAsync(out, h->d_tsm + L.res, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
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
  double* vm = h->d_trl + (int64_t)h->trl_m * h->trl_ld;  // the residual row carries x and then the result
  LZ_TRY(upload(h, vm, x, (size_t)h->rows * sizeof(double)));
  trl_apply_op(h, vm);
  LZ_TRY(check_launch(h, "trl filter apply"));
  LZ_HIP(h, hipMemcpyAsync(vm, h->d_tw, (size_t)h->rows_pad * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  LZ_HIP(h, hipMemcpyAsync(y, h->d_tw, (size_t)h->rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_trl_rayleigh(lz_handle h, int k, double* G_out) {
  LZ_TRY(trl_state(h, "lz_trl_rayleigh"));
  if (!G_out || k < 1 || k >= h->trl_m) return fail(h, LZ_ERR_ARG, "lz_trl_rayleigh: need 1 <= k < m and G_out");
  const TrlSmall L = trl_small_layout(h->trl_m);
  double* V = h->d_trl;
  double* G = h->d_tsm + L.S;  // k x k in the restart's S area
  const QtwPlan plan = trl_plan(h);
  for (int i = 0; i < k; ++i) {
    trl_matvec(h, V + (int64_t)i * h->trl_ld, h->d_tw);  // A itself, filter or not
    LZ_HIP(h, launch_qtw(V, h->trl_ld, h->rows_pad, k + 1, k, h->d_tw, nullptr, nullptr, plan, h->d_tpart, 2, h->stream));
    launch_final_rows(h->d_tpart, k + 1, plan.P, h->d_tsm + L.c1, h->stream, plan.family == 2);
    LZ_HIP(h, hipMemcpyAsync(G + (int64_t)i * k, h->d_tsm + L.c1, (size_t)k * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    LZ_TRY(check_launch(h, "trl rayleigh"));
  }
  LZ_HIP(h, hipMemcpyAsync(G_out, G, (size_t)k * k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_trl_set_rows(lz_handle h, int j0, int count, const double* rows, int64_t ld) {
  LZ_TRY(trl_state(h, "lz_trl_set_rows"));
  if (!rows || j0 < 0 || count < 1 || j0 + count > h->trl_m + 1 || ld < h->rows_pad)
    return fail(h, LZ_ERR_ARG, "lz_trl_set_rows: need rows j0 .. j0 + count - 1 <= m and ld >= the padded row length");
  LZ_TRY(upload2d(h, h->d_trl + (int64_t)j0 * h->trl_ld, (size_t)h->trl_ld * sizeof(double), rows, (size_t)ld * sizeof(double),
                  (size_t)h->rows_pad * sizeof(double), (size_t)count));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_trl_get_rows(lz_handle h, int j0, int count, double* rows, int64_t ld) {
  LZ_TRY(trl_state(h, "lz_trl_get_rows"));
  if (!rows || j0 < 0 || count < 1 || j0 + count > h->trl_m + 1 || ld < h->rows_pad)
    return fail(h, LZ_ERR_ARG, "lz_trl_get_rows: need rows j0 .. j0 + count - 1 <= m and ld >= the padded row length");
  LZ_HIP(h, hipMemcpy2DAsync(rows, (size_t)ld * sizeof(double), h->d_trl + (int64_t)j0 * h->trl_ld, (size_t)h->trl_ld * sizeof(double),
                             (size_t)h->rows_pad * sizeof(double), (size_t)count, hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

}  // extern "C"
