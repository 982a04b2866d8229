// The Gram-Schmidt basis layer under the restart solvers (lz_trl_api.hip, lz_gk_api.hip): the launch sequences that make a work vector
// orthogonal to an OrthBasis (lz_context.h) and store it as the basis' next row, the row transfers, and the partials they need.  The
// kernels are lz_reorth.hip's (launch_qtw, launch_final_rows, launch_scale_store) and lz_trl.hip's (launch_trl_cgs, launch_trl_post).
// What every sequence relies on:
//  - the walks stream pad doubles of every row and of w, the products write len and never touch w[len .. pad).  That padding is zero
//    because orth_upload_x zeroes all of w before every begin and every probe, and a Gram-Schmidt update with finite coefficients on
//    zero-padded rows keeps it zero.  A breakdown (0 / 0 behind a vanished residual) leaves NaN there, which no product would clear: the
//    probe that follows a breakdown does, through orth_upload_x (lz_trl_extend_band clears its own work vectors itself).  A NaN left
//    there would reach every coefficient;
//  - the dots take one row more than they project on: row n of B is the self slot, whose "dot" is w . w (the kernel reads w there);
//  - launch_trl_post(0) sets gate[0] for pass 2 (pass 1 cancelled more than half of |w|, or force), the gated launches of pass 2
//    return at once where it is 0, and launch_trl_post(1) takes pass 2's norm and adds its coefficients only where it ran.
#include "lz_context.h"

using namespace lz;

namespace lz {
namespace api {

QtwPlan orth_plan(lz_handle h, const OrthBasis& b) {
  return plan_qtw(b.pad, h->flags & ~(LZ_FLAG_QTW_MFMA | LZ_FLAG_ONE_REDUCE), h->tune, b.nrows + 1);
}

int orth_dots(lz_handle h, const OrthBasis& b, const OrthWork& wk, const QtwPlan& plan, int n, double* c, const int* gate) {
  QtwFuse gated;
  gated.gate = gate;
  LZ_HIP(h, launch_qtw(b.B, b.ld, b.pad, n + 1, n, b.w, nullptr, nullptr, plan, wk.part, 2, h->stream, gate ? &gated : nullptr));
  launch_final_rows(wk.part, n + 1, plan.P, c, h->stream, plan.family == 2, gate);
  return LZ_OK;
}

int orth_store(lz_handle h, const OrthBasis& b, const OrthWork& wk, const QtwPlan& plan, int k, const char* what) {
  const OrthSmallHead L = orth_small_head(b.nrows);
  double* c = wk.sm + L.c1;
  double* nrm2 = wk.sm + L.nrm2;
  int np = 0;
  for (int pass = 0; pass < (k > 0 ? 2 : 1); ++pass) {  // (k == 0: |x|^2 only)
    if (k > 0) LZ_TRY(orth_dots(h, b, wk, plan, k, c));
    np = launch_trl_cgs(b.B, b.ld, b.pad, k, c, b.w, wk.part, nullptr, h->stream);
  }
  launch_trl_post(2, wk.part, np, nullptr, 0, nrm2, nullptr, wk.gate, 0, h->stream);
  launch_scale_store(b.B + (int64_t)k * b.ld, b.w, nrm2, nrm2 + 1, b.pad, h->stream);
  LZ_TRY(check_launch(h, what));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int orth_cgs_step(lz_handle h, const OrthBasis& b, const OrthWork& wk, const QtwPlan& plan, int nb, double* proj, double* norm_slot,
                  OrthPass2 pass2) {
  const OrthSmallHead L = orth_small_head(b.nrows);
  double* nrm2 = wk.sm + L.nrm2;
  if (nb > 0) {
    const int* gate = pass2 == OrthPass2::kUngated ? nullptr : wk.gate;
    const int force = pass2 != OrthPass2::kGated;  // (launch_trl_post(1) adds pass 2's coefficients where gate[0] is set: force sets it)
    for (int pass = 0; pass < 2; ++pass) {
      // c = B[0..nb) . w, w -= sum c_i B_i; pass 2 only where pass 1 cancelled more than half of |w| (or force)
      double* c = wk.sm + (pass == 0 ? L.c1 : L.c2);
      LZ_TRY(orth_dots(h, b, wk, plan, nb, c, pass == 0 ? nullptr : gate));
      const int np = launch_trl_cgs(b.B, b.ld, b.pad, nb, c, b.w, wk.part, pass == 0 ? nullptr : gate, h->stream);
      launch_trl_post(pass, wk.part, np, c, nb - 1, nrm2, proj, wk.gate, force, h->stream);
    }
  } else {  // nothing to project on: the norm only
    const int np = launch_trl_cgs(b.B, b.ld, b.pad, 0, wk.sm + L.c1, b.w, wk.part, nullptr, h->stream);
    launch_trl_post(2, wk.part, np, nullptr, 0, nrm2, nullptr, wk.gate, 0, h->stream);
  }
  launch_scale_store(b.B + (int64_t)nb * b.ld, b.w, nrm2, norm_slot, b.pad, h->stream);
  return LZ_OK;
}

int orth_upload_x(lz_handle h, const OrthBasis& b, const double* x) {
  LZ_HIP(h, hipMemsetAsync(b.w, 0, (size_t)b.ld * sizeof(double), h->stream));
  LZ_TRY(upload(h, b.w, x, (size_t)b.len * sizeof(double)));
  return LZ_OK;
}

int orth_get_vectors(lz_handle h, const OrthBasis& b, int k, double* out) {
  const int64_t M = b.len;
  std::vector<double> rowsk((size_t)k * (size_t)M);
  LZ_HIP(h, xfer_d2h(h->dev, h->stream, h->xfer, rowsk.data(), (size_t)M * sizeof(double), b.B, (size_t)b.ld * sizeof(double),
                     (size_t)M * sizeof(double), (size_t)k));
  parallel_ranges(M, 1 << 16, [&](int, int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r)
      for (int i = 0; i < k; ++i) out[r * k + i] = rowsk[(size_t)i * M + r];
  });
  return LZ_OK;
}

static int rows_arg(lz_handle h, const OrthBasis& b, const char* who, const char* top, int j0, int count, const double* rows, int64_t ld) {
  if (!rows || j0 < 0 || count < 1 || j0 + count > b.nrows || ld < b.pad)
    return fail(h, LZ_ERR_ARG, std::string(who) + ": need rows j0 .. j0 + count - 1 <= " + top + " and ld >= the padded row length");
  return LZ_OK;
}

int orth_set_rows(lz_handle h, const OrthBasis& b, const char* who, const char* top, int j0, int count, const double* rows, int64_t ld) {
  LZ_TRY(rows_arg(h, b, who, top, j0, count, rows, ld));
  LZ_TRY(upload2d(h, b.B + (int64_t)j0 * b.ld, (size_t)b.ld * sizeof(double), rows, (size_t)ld * sizeof(double), (size_t)b.pad * sizeof(double),
                  (size_t)count));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int orth_get_rows(lz_handle h, const OrthBasis& b, const char* who, const char* top, int j0, int count, double* rows, int64_t ld) {
  LZ_TRY(rows_arg(h, b, who, top, j0, count, rows, ld));
  LZ_HIP(h, hipMemcpy2DAsync(rows, (size_t)ld * sizeof(double), b.B + (int64_t)j0 * b.ld, (size_t)b.ld * sizeof(double),
                             (size_t)b.pad * sizeof(double), (size_t)count, hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

size_t orth_part_need(const OrthBasis& b, const QtwPlan& plan, int m) {
  size_t need = (size_t)(b.nrows + 1 + 32) * (size_t)plan.P;
  need = std::max<size_t>(need, (size_t)trl_cgs_blocks(b.pad));
  return std::max<size_t>(need, (size_t)m * (size_t)((b.len + kTPB - 1) / kTPB) + 64);  // residual norms
}

int orth_part_reserve(lz_handle h, OrthWork& wk, size_t need) {
  need += 8192;
  if (need > wk.part_cap) {
    LZ_TRY(dev_alloc(h, wk.part, need));
    wk.part_cap = need;
  }
  return LZ_OK;
}

void orth_free(OrthBasis& b) {
  big_free(b.B);
  big_free(b.w);
  b = OrthBasis();
}

void orth_free(OrthWork& wk) {
  big_free(wk.sm);
  big_free(wk.gate);
  big_free(wk.part);
  wk = OrthWork();
}

}  // namespace api
}  // namespace lz
