// C ABI of the complex thick-restart Lanczos solver (include/lanczos_hip.h, "complex Hermitian matrices"): the device half of
// lanczos_amd.eigsh on complex Hermitian input.  The twin of lz_trl_api.hip on a complex matrix (lz_zspmv.hip) and a planar basis of
// its own (h->z.B: 2 (m + 1) real rows, complex row j = rows 2 j and 2 j + 1), so the restart is launch_trl_restart on the real form of
// S, the vectors come back through orth_get_vectors and the scale-and-store and final sums are the real kernels'.  The inner products
// and the Gram-Schmidt update are complex kernels (lz_ztrl.hip).  Across the ABI everything complex is interleaved complex128.
// The padding rule is lz_orth.hip's: the walks stream the padded length, the products write n, a begin or probe zeroes all of w.
#include "lz_context.h"

using namespace lz;
using namespace lz::api;

namespace {

constexpr int kZMaxM = kZMaxRows - 1;  // 64: the restart's real form has 2 m rows, and launch_trl_restart takes up to 128

// z.wk.sm: c of both passes (interleaved complex, the self slot last), nrm2, the projected rows (m x m complex), beta (m), the
// restart's S in real form (2 m x 2 m), theta and the residual norms (m each)
struct ZSmall {
  int64_t c1, c2, nrm2, proj, beta, S, theta, res, total;
};
ZSmall ztrl_small_layout(int m) {
  ZSmall L;
  const int64_t cl = 2 * (int64_t)(m + 2) + 16;
  L.c1 = 0;
  L.c2 = cl;
  L.nrm2 = 2 * cl;
  L.proj = L.nrm2 + 8;
  L.beta = L.proj + 2 * (int64_t)m * m;
  L.S = L.beta + m + 8;
  L.theta = L.S + 4 * (int64_t)m * m;
  L.res = L.theta + m + 8;
  L.total = L.res + m + 8;
  return L;
}

int ztrl_state(lz_handle h, const char* who) {
  if (!h) return LZ_ERR_ARG;
  ZState& z = h->z;
  if (z.kind == 0) return fail(h, LZ_ERR_STATE, std::string(who) + ": no complex matrix set (lz_set_csr_cplx / lz_set_dense_cplx)");
  if (!z.B.B) return fail(h, LZ_ERR_STATE, std::string(who) + ": no complex thick-restart basis (lz_ztrl_begin first)");
  if (skew_stride(h, h->rows_pad) != z.B.ld) return fail(h, LZ_ERR_STATE, std::string(who) + ": the matrix changed since lz_ztrl_begin");
  z.B.len = h->rows;  // the view follows the matrix set last, as trl_state's does
  z.B.pad = h->rows_pad;
  LZ_HIP(h, hipSetDevice(h->dev));
  return LZ_OK;
}

int ztrl_alloc(lz_handle h, int m) {
  ZState& z = h->z;
  if (z.kind == 0) return fail(h, LZ_ERR_STATE, "lz_ztrl_begin: no complex matrix set (lz_set_csr_cplx / lz_set_dense_cplx)");
  if (h->world > 1 || h->comm_kind != 0)
    return fail(h, LZ_ERR_STATE, "lz_ztrl_begin: the thick-restart solver runs on one rank (this handle has a communicator)");
  if (h->flags & (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE))
    return fail(h, LZ_ERR_STATE, "lz_ztrl_begin: not with LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE");
  if (m < 2 || m > kZMaxM || m > h->rows) return fail(h, LZ_ERR_ARG, "lz_ztrl_begin: need 2 <= m <= min(64, n)");
  LZ_HIP(h, hipSetDevice(h->dev));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  const int64_t ld = skew_stride(h, h->rows_pad);
  const size_t nrows = 2 * (size_t)(m + 1);
  const ZSmall L = ztrl_small_layout(m);
  if (!z.B.B || z.m != m || z.B.ld != ld) {
    LZ_TRY(dev_alloc(h, z.B.B, nrows * (size_t)ld));
    LZ_TRY(dev_alloc(h, z.B.w, 2 * (size_t)ld));
    LZ_TRY(dev_alloc(h, z.wk.sm, (size_t)L.total));
    LZ_TRY(dev_alloc(h, z.wk.gate, 4));
    z.m = m;
    z.B.ld = ld;
    z.B.nrows = (int)nrows;
  }
  z.B.len = h->rows;
  z.B.pad = h->rows_pad;
  size_t need = 2 * (size_t)(m + 2) * (size_t)zdots_blocks(h->rows_pad);
  need = std::max<size_t>(need, (size_t)zcgs_blocks(h->rows_pad));
  need = std::max<size_t>(need, (size_t)m * (size_t)((h->rows + kTPB - 1) / kTPB) + 64);  // residual norms
  LZ_TRY(orth_part_reserve(h, z.wk, need));
  LZ_HIP(h, hipMemsetAsync(z.B.B, 0, nrows * (size_t)ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(z.B.w, 0, 2 * (size_t)ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(z.wk.sm, 0, (size_t)L.total * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(z.wk.gate, 0, 4 * sizeof(int), h->stream));
  return LZ_OK;
}

// c (interleaved, nb + 1 complex: the self slot last) = <V_i, w>, i < nb
void ztrl_dots(lz_handle h, int nb, double* c, const int* gate) {
  const OrthBasis& V = h->z.B;
  const int G = launch_zdots(V.B, V.ld, V.pad, nb, V.w, h->z.wk.part, gate, h->stream);
  // (the final sums take no gate: behind a closed gate they add stale partials into pass 2's c, which nothing reads)
  launch_final_rows(h->z.wk.part, 2 * (nb + 1), G, c, h->stream);
}

// w = x (n interleaved complex), planar, everything beyond n zero
int ztrl_upload_x(lz_handle h, const double* x) {
  const OrthBasis& V = h->z.B;
  const int64_t n = V.len;
  std::vector<double> buf(2 * (size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    buf[(size_t)i] = x[2 * i];
    buf[(size_t)(n + i)] = x[2 * i + 1];
  }
  LZ_HIP(h, hipMemsetAsync(V.w, 0, 2 * (size_t)V.ld * sizeof(double), h->stream));
  LZ_TRY(upload2d(h, V.w, (size_t)V.ld * sizeof(double), buf.data(), (size_t)n * sizeof(double), (size_t)n * sizeof(double), 2));
  LZ_HIP(h, hipStreamSynchronize(h->stream));  // (buf)
  return LZ_OK;
}

// w / |w| to complex row k, |w| to norm_slot
void ztrl_scale_store(lz_handle h, int k, const double* nrm2, double* norm_slot) {
  const OrthBasis& V = h->z.B;
  launch_scale_store(V.B + (int64_t)(2 * k) * V.ld, V.w, nrm2, norm_slot, V.pad, h->stream);
  launch_scale_store(V.B + (int64_t)(2 * k + 1) * V.ld, V.w + V.ld, nrm2, norm_slot, V.pad, h->stream);
}

// row k = w made orthogonal to rows [0, k) by two CGS passes, normalised; synchronises (orth_store's sequence)
int ztrl_store(lz_handle h, int k, const char* what) {
  const OrthBasis& V = h->z.B;
  const OrthWork& wk = h->z.wk;
  const ZSmall L = ztrl_small_layout(h->z.m);
  double* c = wk.sm + L.c1;
  double* nrm2 = wk.sm + L.nrm2;
  int np = 0;
  for (int pass = 0; pass < (k > 0 ? 2 : 1); ++pass) {
    if (k > 0) ztrl_dots(h, k, c, nullptr);
    np = launch_zcgs(V.B, V.ld, V.pad, k, c, V.w, wk.part, nullptr, h->stream);
  }
  launch_trl_post(2, wk.part, np, nullptr, 0, nrm2, nullptr, wk.gate, 0, h->stream);
  ztrl_scale_store(h, k, nrm2, nrm2 + 1);
  LZ_TRY(check_launch(h, what));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

// one extension step (orth_cgs_step's sequence, nb >= 1): w against rows [0, nb), a second pass behind the DGKS gate (or forced), the
// nb complex coefficients to proj, |w| to norm_slot, w / |w| to row nb.  launch_trl_post sees the interleaved c as 2 nb doubles
// followed by the self slot's real part, which is where it looks for |w|^2 before the pass.
void ztrl_cgs_step(lz_handle h, int nb, double* proj, double* norm_slot, bool forced) {
  const OrthBasis& V = h->z.B;
  const OrthWork& wk = h->z.wk;
  const ZSmall L = ztrl_small_layout(h->z.m);
  double* nrm2 = wk.sm + L.nrm2;
  for (int pass = 0; pass < 2; ++pass) {
    double* c = wk.sm + (pass == 0 ? L.c1 : L.c2);
    const int* gate = pass == 0 ? nullptr : wk.gate;
    ztrl_dots(h, nb, c, gate);
    const int np = launch_zcgs(V.B, V.ld, V.pad, nb, c, V.w, wk.part, gate, h->stream);
    launch_trl_post(pass, wk.part, np, c, 2 * nb - 1, nrm2, proj, wk.gate, forced ? 1 : 0, h->stream);
  }
  ztrl_scale_store(h, nb, nrm2, norm_slot);
}

int zrows_arg(lz_handle h, const char* who, int j0, int count, const double* rows, int64_t ld) {
  if (!rows || j0 < 0 || count < 1 || j0 + count > h->z.m + 1 || ld < h->rows)
    return fail(h, LZ_ERR_ARG, std::string(who) + ": need rows j0 .. j0 + count - 1 <= m and ld >= n (in complex elements)");
  return LZ_OK;
}

}  // namespace

extern "C" {

int lz_ztrl_begin(lz_handle h, int m, const double* v0) {
  if (!h || !v0) return LZ_ERR_ARG;
  LZ_TRY(ztrl_alloc(h, m));
  LZ_TRY(ztrl_upload_x(h, v0));
  return ztrl_store(h, 0, "ztrl begin");
}

int lz_ztrl_extend(lz_handle h, int k, int m, double* proj_out, double* beta_out) {
  LZ_TRY(ztrl_state(h, "lz_ztrl_extend"));
  ZState& z = h->z;
  if (m != z.m || k < 0 || k >= m) return fail(h, LZ_ERR_ARG, "lz_ztrl_extend: need m == the m of lz_ztrl_begin and 0 <= k < m");
  const ZSmall L = ztrl_small_layout(m);
  const OrthBasis& V = z.B;
  double* sm = z.wk.sm;
  const bool forced = (h->flags & LZ_FLAG_TRL_PASS2_ALWAYS) != 0;
  for (int j = k; j < m; ++j) {
    z_matvec(h, V.B + (int64_t)(2 * j) * V.ld, V.w, V.ld);  // w = A V[j]
    ztrl_cgs_step(h, j + 1, sm + L.proj + 2 * (int64_t)j * m, sm + L.beta + j, forced);
    LZ_TRY(check_launch(h, "ztrl extend"));
  }
  if (proj_out) LZ_HIP(h, hipMemcpyAsync(proj_out, sm + L.proj, 2 * (size_t)m * m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (beta_out) LZ_HIP(h, hipMemcpyAsync(beta_out, sm + L.beta, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_ztrl_restart(lz_handle h, int m, int kk, const double* S) {
  LZ_TRY(ztrl_state(h, "lz_ztrl_restart"));
  ZState& z = h->z;
  if (!S || m != z.m || kk < 1 || kk >= m) return fail(h, LZ_ERR_ARG, "lz_ztrl_restart: need m == the m of lz_ztrl_begin, 1 <= kk < m, S");
  const ZSmall L = ztrl_small_layout(m);
  // Y_k = sum_i S[i, k] V_i on planar rows: input rows 2 i, 2 i + 1 = Re, Im V_i, output rows 2 k, 2 k + 1 = Re, Im Y_k, so the real
  // form is [[Sr, Si], [-Si, Sr]] in rows 2 i, 2 i + 1 and columns 2 k, 2 k + 1 (Re Y = Sr Vr - Si Vi, Im Y = Si Vr + Sr Vi)
  std::vector<double> R(4 * (size_t)m * kk);
  const size_t ldr = 2 * (size_t)kk;
  for (int i = 0; i < m; ++i)
    for (int c = 0; c < kk; ++c) {
      const double sr = S[2 * ((size_t)i * kk + c)], si = S[2 * ((size_t)i * kk + c) + 1];
      R[(size_t)(2 * i) * ldr + 2 * c] = sr;
      R[(size_t)(2 * i) * ldr + 2 * c + 1] = si;
      R[(size_t)(2 * i + 1) * ldr + 2 * c] = -si;
      R[(size_t)(2 * i + 1) * ldr + 2 * c + 1] = sr;
    }
  LZ_TRY(upload(h, z.wk.sm + L.S, R.data(), R.size() * sizeof(double)));
  LZ_HIP(h, launch_trl_restart(z.B.B, z.B.ld, h->rows, 2 * m, 2 * kk, z.wk.sm + L.S, h->stream));  // ... and real row 2 kk = row 2 m
  // the imaginary half of the residual row follows (row 2 kk + 1 was an input of the kernel above, which has finished with it)
  LZ_HIP(h, hipMemcpyAsync(z.B.B + (int64_t)(2 * kk + 1) * z.B.ld, z.B.B + (int64_t)(2 * m + 1) * z.B.ld, (size_t)h->rows * sizeof(double),
                           hipMemcpyDeviceToDevice, h->stream));
  LZ_TRY(check_launch(h, "ztrl restart"));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_ztrl_probe(lz_handle h, int k, const double* x) {
  LZ_TRY(ztrl_state(h, "lz_ztrl_probe"));
  if (!x || k < 0 || k > h->z.m) return fail(h, LZ_ERR_ARG, "lz_ztrl_probe: need 0 <= k <= m and x");
  LZ_TRY(ztrl_upload_x(h, x));
  return ztrl_store(h, k, "ztrl orthogonalise");
}

int lz_ztrl_get_vectors(lz_handle h, int k, double* Y_out) {
  LZ_TRY(ztrl_state(h, "lz_ztrl_get_vectors"));
  if (!Y_out || k < 1 || k > h->z.m) return fail(h, LZ_ERR_ARG, "lz_ztrl_get_vectors: need 1 <= k <= m and Y_out");
  // the 2 k real rows transposed are n x 2 k doubles with Re, Im of Y[r, i] side by side: n x k interleaved complex
  return orth_get_vectors(h, h->z.B, 2 * k, Y_out);
}

int lz_ztrl_residuals(lz_handle h, int k, const double* theta, double* out) {
  LZ_TRY(ztrl_state(h, "lz_ztrl_residuals"));
  ZState& z = h->z;
  if (!theta || !out || k < 1 || k > z.m) return fail(h, LZ_ERR_ARG, "lz_ztrl_residuals: need 1 <= k <= m, theta and out");
  const ZSmall L = ztrl_small_layout(z.m);
  double* dth = z.wk.sm + L.theta;
  LZ_TRY(upload(h, dth, theta, (size_t)k * sizeof(double)));
  int G = 0;
  for (int i = 0; i < k; ++i) {
    const double* x = z.B.B + (int64_t)(2 * i) * z.B.ld;
    z_matvec(h, x, z.B.w, z.B.ld);
    G = launch_zresid_diff(z.B.w, x, z.B.ld, h->rows, dth, i, z.wk.part, h->stream);
  }
  launch_trl_rownorm(z.wk.part, G, k, z.wk.sm + L.res, h->stream);
  LZ_TRY(check_launch(h, "ztrl residuals"));
  LZ_HIP(h, hipMemcpyAsync(out, z.wk.sm + L.res, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_ztrl_set_rows(lz_handle h, int j0, int count, const double* rows, int64_t ld) {
  LZ_TRY(ztrl_state(h, "lz_ztrl_set_rows"));
  LZ_TRY(zrows_arg(h, "lz_ztrl_set_rows", j0, count, rows, ld));
  const OrthBasis& V = h->z.B;
  const int64_t n = V.len, pad = V.pad;
  std::vector<double> buf(2 * (size_t)count * (size_t)pad, 0.0);  // planar, with a zero padding
  for (int j = 0; j < count; ++j) {
    const double* src = rows + 2 * (int64_t)j * ld;
    double* re = buf.data() + (size_t)(2 * j) * pad;
    double* im = re + pad;
    for (int64_t i = 0; i < n; ++i) {
      re[i] = src[2 * i];
      im[i] = src[2 * i + 1];
    }
  }
  LZ_TRY(upload2d(h, V.B + (int64_t)(2 * j0) * V.ld, (size_t)V.ld * sizeof(double), buf.data(), (size_t)pad * sizeof(double),
                  (size_t)pad * sizeof(double), 2 * (size_t)count));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_ztrl_get_rows(lz_handle h, int j0, int count, double* rows, int64_t ld) {
  LZ_TRY(ztrl_state(h, "lz_ztrl_get_rows"));
  LZ_TRY(zrows_arg(h, "lz_ztrl_get_rows", j0, count, rows, ld));
  const OrthBasis& V = h->z.B;
  const int64_t n = V.len;
  std::vector<double> buf(2 * (size_t)count * (size_t)n);
  LZ_HIP(h, hipMemcpy2DAsync(buf.data(), (size_t)n * sizeof(double), V.B + (int64_t)(2 * j0) * V.ld, (size_t)V.ld * sizeof(double),
                             (size_t)n * sizeof(double), 2 * (size_t)count, hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  for (int j = 0; j < count; ++j) {
    double* dst = rows + 2 * (int64_t)j * ld;
    const double* re = buf.data() + (size_t)(2 * j) * n;
    const double* im = re + n;
    for (int64_t i = 0; i < n; ++i) {
      dst[2 * i] = re[i];
      dst[2 * i + 1] = im[i];
    }
  }
  return LZ_OK;
}

}  // extern "C"
