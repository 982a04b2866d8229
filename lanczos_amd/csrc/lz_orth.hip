// The Gram-Schmidt basis layer under the three restart solvers (lz_trl_api.hip, lz_gk_api.hip, lz_ztrl_api.hip): the launch sequences
// that make a work vector orthogonal to an OrthBasis (lz_context.h), real or planar complex, and store it as the basis' next row, the
// row transfers, the residual norms and the partials they need.  The kernels are lz_reorth.hip's (launch_qtw, launch_final_rows,
// launch_scale_store), lz_trl.hip's (launch_trl_cgs, launch_trl_post) and, for the inner products and the update of a complex basis,
// lz_ztrl.hip's (launch_zdots, launch_zcgs); the final sums, the post step and the scale-and-store of a complex basis are the real ones
// on its 2 (n + 1) interleaved coefficients and its two planes.
// What every sequence relies on:
//  - the walks stream pad doubles of every row and of w, the products write len and never touch w[len .. pad).  That padding is zero
//    because orth_upload_x zeroes all of w before every begin and every probe, and a Gram-Schmidt update with finite coefficients on
//    zero-padded rows keeps it zero.  A breakdown (0 / 0 behind a vanished residual) leaves NaN there, which no product would clear: the
//    probe that follows a breakdown does, through orth_upload_x (lz_trl_extend_band clears its own work vectors itself).  A NaN left
//    there would reach every coefficient;
//  - the dots take one row more than they project on: row n of B is the self slot, whose "dot" is w . w (the kernel reads w there);
//  - launch_trl_post(0) sets gate[0] for pass 2 (pass 1 cancelled more than half of |w|, or force), the gated launches of pass 2
//    return at once where it is 0, and launch_trl_post(1) takes pass 2's norm and adds its coefficients only where it ran.  It sees
//    the interleaved c of a complex basis as 2 n doubles followed by the self slot's real part, which is where it looks for |w|^2.
#include "lz_context.h"

using namespace lz;

namespace lz {
namespace api {

QtwPlan orth_plan(lz_handle h, const OrthBasis& b) {
  if (b.planes == 2) return QtwPlan();
  return plan_qtw(b.pad, h->flags & ~(LZ_FLAG_QTW_MFMA | LZ_FLAG_ONE_REDUCE), h->tune, b.nrows + 1);
}

int orth_dots(lz_handle h, const OrthBasis& b, const OrthWork& wk, const QtwPlan& plan, int n, double* c, const int* gate) {
  if (b.planes == 2) {
    const int G = launch_zdots(b.B, b.ld, b.pad, n, b.w, wk.part, gate, h->stream);
    // (the final sums take no gate: behind a closed gate they add stale partials into pass 2's c, which nothing reads)
    launch_final_rows(wk.part, 2 * (n + 1), G, c, h->stream);
    return LZ_OK;
  }
  QtwFuse gated;
  gated.gate = gate;
  LZ_HIP(h, launch_qtw(b.B, b.ld, b.pad, n + 1, n, b.w, nullptr, nullptr, plan, wk.part, 2, h->stream, gate ? &gated : nullptr));
  launch_final_rows(wk.part, n + 1, plan.P, c, h->stream, plan.family == 2, gate);
  return LZ_OK;
}

// w -= sum_{i < n} c_i B_i; returns the number of partials of |w|^2 it left in wk.part
static int orth_update(lz_handle h, const OrthBasis& b, const OrthWork& wk, int n, const double* c, const int* gate) {
  return (b.planes == 2 ? launch_zcgs : launch_trl_cgs)(b.B, b.ld, b.pad, n, c, b.w, wk.part, gate, h->stream);
}

// w / |w| to row k, |w| to norm_slot
static void orth_scale_store(lz_handle h, const OrthBasis& b, int k, const double* nrm2, double* norm_slot) {
  for (int p = 0; p < b.planes; ++p)
    launch_scale_store(b.B + (int64_t)(b.planes * k + p) * b.ld, b.w + p * b.ld, nrm2, norm_slot, b.pad, h->stream);
}

int orth_store(lz_handle h, const OrthBasis& b, const OrthWork& wk, const QtwPlan& plan, int k, const char* what) {
  const OrthSmallHead L = orth_small_head(b.nrows, b.planes);
  double* c = wk.sm + L.c1;
  double* nrm2 = wk.sm + L.nrm2;
  int np = 0;
  for (int pass = 0; pass < (k > 0 ? 2 : 1); ++pass) {  // (k == 0: |x|^2 only)
    if (k > 0) LZ_TRY(orth_dots(h, b, wk, plan, k, c));
    np = orth_update(h, b, wk, k, c, nullptr);
  }
  launch_trl_post(2, wk.part, np, nullptr, 0, nrm2, nullptr, wk.gate, 0, h->stream);
  orth_scale_store(h, b, k, nrm2, nrm2 + 1);
  LZ_TRY(check_launch(h, what));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

// (nb == 0 and OrthPass2::kUngated are the real solvers': no complex caller has either)
int orth_cgs_step(lz_handle h, const OrthBasis& b, const OrthWork& wk, const QtwPlan& plan, int nb, double* proj, double* norm_slot,
                  OrthPass2 pass2) {
  const OrthSmallHead L = orth_small_head(b.nrows, b.planes);
  double* nrm2 = wk.sm + L.nrm2;
  if (nb > 0) {
    const int* gate = pass2 == OrthPass2::kUngated ? nullptr : wk.gate;
    const int force = pass2 != OrthPass2::kGated;  // (launch_trl_post(1) adds pass 2's coefficients where gate[0] is set: force sets it)
    for (int pass = 0; pass < 2; ++pass) {
      // c = <B[0..nb), w>, w -= sum c_i B_i; pass 2 only where pass 1 cancelled more than half of |w| (or force)
      double* c = wk.sm + (pass == 0 ? L.c1 : L.c2);
      LZ_TRY(orth_dots(h, b, wk, plan, nb, c, pass == 0 ? nullptr : gate));
      const int np = orth_update(h, b, wk, nb, c, pass == 0 ? nullptr : gate);
      launch_trl_post(pass, wk.part, np, c, b.planes * nb - 1, nrm2, proj, wk.gate, force, h->stream);
    }
  } else {  // nothing to project on: the norm only
    const int np = launch_trl_cgs(b.B, b.ld, b.pad, 0, wk.sm + L.c1, b.w, wk.part, nullptr, h->stream);
    launch_trl_post(2, wk.part, np, nullptr, 0, nrm2, nullptr, wk.gate, 0, h->stream);
  }
  orth_scale_store(h, b, nb, nrm2, norm_slot);
  return LZ_OK;
}

void to_planar(const double* z, int64_t n, double* re, double* im) {
  for (int64_t i = 0; i < n; ++i) {
    re[i] = z[2 * i];
    im[i] = z[2 * i + 1];
  }
}

void to_interleaved(const double* re, const double* im, int64_t n, double* z) {
  for (int64_t i = 0; i < n; ++i) {
    z[2 * i] = re[i];
    z[2 * i + 1] = im[i];
  }
}

int orth_upload_x(lz_handle h, const OrthBasis& b, const double* x) {
  LZ_HIP(h, hipMemsetAsync(b.w, 0, (size_t)b.planes * (size_t)b.ld * sizeof(double), h->stream));
  if (b.planes == 1) return upload(h, b.w, x, (size_t)b.len * sizeof(double));
  std::vector<double> buf(2 * (size_t)b.len);
  to_planar(x, b.len, buf.data(), buf.data() + b.len);
  LZ_TRY(upload2d(h, b.w, (size_t)b.ld * sizeof(double), buf.data(), (size_t)b.len * sizeof(double), (size_t)b.len * sizeof(double), 2));
  LZ_HIP(h, hipStreamSynchronize(h->stream));  // (buf)
  return LZ_OK;
}

int orth_get_vectors(lz_handle h, const OrthBasis& b, int k, double* out) {
  // the 2 k real rows of a complex basis transposed are len x 2 k doubles with Re, Im of out[r, i] side by side: len x k interleaved complex
  k *= b.planes;
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
  const bool z = b.planes == 2;
  if (!rows || j0 < 0 || count < 1 || j0 + count > b.nrows || ld < (z ? b.len : b.pad))
    return fail(h, LZ_ERR_ARG, std::string(who) + ": need rows j0 .. j0 + count - 1 <= " + top +
                                   (z ? " and ld >= n (in complex elements)" : " and ld >= the padded row length"));
  return LZ_OK;
}

int orth_set_rows(lz_handle h, const OrthBasis& b, const char* who, const char* top, int j0, int count, const double* rows, int64_t ld) {
  LZ_TRY(rows_arg(h, b, who, top, j0, count, rows, ld));
  std::vector<double> buf;  // complex: planar, with a zero padding
  if (b.planes == 2) {
    buf.assign(2 * (size_t)count * (size_t)b.pad, 0.0);
    for (int j = 0; j < count; ++j) to_planar(rows + 2 * (int64_t)j * ld, b.len, &buf[(size_t)(2 * j) * b.pad], &buf[(size_t)(2 * j + 1) * b.pad]);
    rows = buf.data();
    ld = b.pad;
  }
  LZ_TRY(upload2d(h, b.B + (int64_t)b.planes * j0 * b.ld, (size_t)b.ld * sizeof(double), rows, (size_t)ld * sizeof(double),
                  (size_t)b.pad * sizeof(double), (size_t)b.planes * (size_t)count));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int orth_get_rows(lz_handle h, const OrthBasis& b, const char* who, const char* top, int j0, int count, double* rows, int64_t ld) {
  LZ_TRY(rows_arg(h, b, who, top, j0, count, rows, ld));
  const bool z = b.planes == 2;
  const int64_t n = b.len;
  std::vector<double> buf(z ? 2 * (size_t)count * (size_t)n : 0);  // complex: the planes without their padding
  LZ_HIP(h, hipMemcpy2DAsync(z ? buf.data() : rows, (size_t)(z ? n : ld) * sizeof(double), b.B + (int64_t)b.planes * j0 * b.ld,
                             (size_t)b.ld * sizeof(double), (size_t)(z ? n : b.pad) * sizeof(double), (size_t)b.planes * (size_t)count,
                             hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  for (int j = 0; z && j < count; ++j) to_interleaved(&buf[(size_t)(2 * j) * n], &buf[(size_t)(2 * j + 1) * n], n, rows + 2 * (int64_t)j * ld);
  return LZ_OK;
}

int orth_resid_norms(lz_handle h, const OrthBasis& b, const OrthWork& wk, int k, const double* theta, double* out,
                     const std::function<hipError_t(int)>& product) {
  int G = 0;
  for (int i = 0; i < k; ++i) {
    const double* x = b.B + (int64_t)b.planes * i * b.ld;
    LZ_HIP(h, product(i));
    G = b.planes == 2 ? launch_zresid_diff(b.w, x, b.ld, b.len, theta, i, wk.part, h->stream)
                      : launch_trl_resid_diff(b.w, x, b.len, theta, i, wk.part, h->stream);
  }
  launch_trl_rownorm(wk.part, G, k, out, h->stream);
  return LZ_OK;
}

size_t orth_part_need(const OrthBasis& b, const QtwPlan& plan, int m) {
  size_t need = b.planes == 2 ? 2 * (size_t)(b.nrows + 1) * (size_t)zdots_blocks(b.pad) : (size_t)(b.nrows + 1 + 32) * (size_t)plan.P;
  need = std::max<size_t>(need, (size_t)(b.planes == 2 ? zcgs_blocks(b.pad) : trl_cgs_blocks(b.pad)));
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
