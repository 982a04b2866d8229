// C ABI of the complex thick-restart Lanczos solver (include/lanczos_hip.h, "complex Hermitian matrices"): the device half of
// lanczos_amd.eigsh on complex Hermitian input.  The basis is a two-plane OrthBasis of its own (h->z.B: m + 1 complex rows), and
// orthogonalising against it, the gated two-pass step, the row transfers and the residual norms are the basis layer's (lz_orth.hip),
// shared with the real solvers.  What is here is the solver's own: the state and its checks, the product with the complex matrix
// (lz_zspmv.hip) and the restart, which is launch_trl_restart on the real form of S.  Across the ABI everything complex is interleaved
// complex128.
#include "lz_context.h"

using namespace lz;
using namespace lz::api;

namespace {

constexpr int kZMaxM = kZMaxRows - 1;  // 64: the restart's real form has 2 m rows, and launch_trl_restart takes up to 128

// z.wk.sm: the basis layer's head (c of both passes, nrm2), the projected rows (m x m complex), beta (m), the restart's S in real
// form (2 m x 2 m), theta and the residual norms (m each)
struct ZSmall : OrthSmallHead {
  int64_t proj, beta, S, theta, res, total;
};
ZSmall ztrl_small_layout(int m) {
  ZSmall L;
  static_cast<OrthSmallHead&>(L) = orth_small_head(m + 1, 2);
  L.proj = L.end;
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
  const size_t nrows = 2 * (size_t)(m + 1);  // real rows
  const ZSmall L = ztrl_small_layout(m);
  if (!z.B.B || z.m != m || z.B.ld != ld) {
    LZ_TRY(dev_alloc(h, z.B.B, nrows * (size_t)ld));
    LZ_TRY(dev_alloc(h, z.B.w, 2 * (size_t)ld));
    LZ_TRY(dev_alloc(h, z.wk.sm, (size_t)L.total));
    LZ_TRY(dev_alloc(h, z.wk.gate, 4));
    z.m = m;
    z.B.ld = ld;
    z.B.nrows = m + 1;
    z.B.planes = 2;
  }
  z.B.len = h->rows;
  z.B.pad = h->rows_pad;
  LZ_TRY(orth_part_reserve(h, z.wk, orth_part_need(z.B, orth_plan(h, z.B), m)));
  LZ_HIP(h, hipMemsetAsync(z.B.B, 0, nrows * (size_t)ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(z.B.w, 0, 2 * (size_t)ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(z.wk.sm, 0, (size_t)L.total * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(z.wk.gate, 0, 4 * sizeof(int), h->stream));
  return LZ_OK;
}

// V[k] = x made orthogonal to V[0..k), normalised
int ztrl_store_x(lz_handle h, int k, const double* x, const char* what) {
  LZ_TRY(orth_upload_x(h, h->z.B, x));
  return orth_store(h, h->z.B, h->z.wk, orth_plan(h, h->z.B), k, what);
}

}  // namespace

extern "C" {

int lz_ztrl_begin(lz_handle h, int m, const double* v0) {
  if (!h || !v0) return LZ_ERR_ARG;
  LZ_TRY(ztrl_alloc(h, m));
  return ztrl_store_x(h, 0, v0, "ztrl begin");
}

int lz_ztrl_extend(lz_handle h, int k, int m, double* proj_out, double* beta_out) {
  LZ_TRY(ztrl_state(h, "lz_ztrl_extend"));
  ZState& z = h->z;
  if (m != z.m || k < 0 || k >= m) return fail(h, LZ_ERR_ARG, "lz_ztrl_extend: need m == the m of lz_ztrl_begin and 0 <= k < m");
  const ZSmall L = ztrl_small_layout(m);
  const OrthBasis& V = z.B;
  double* sm = z.wk.sm;
  const QtwPlan plan = orth_plan(h, V);
  const OrthPass2 pass2 = (h->flags & LZ_FLAG_TRL_PASS2_ALWAYS) ? OrthPass2::kForced : OrthPass2::kGated;
  for (int j = k; j < m; ++j) {
    z_matvec(h, V.B + (int64_t)(2 * j) * V.ld, V.w, V.ld);  // w = A V[j]
    LZ_TRY(orth_cgs_step(h, V, z.wk, plan, j + 1, sm + L.proj + 2 * (int64_t)j * m, sm + L.beta + j, pass2));
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
  return ztrl_store_x(h, k, x, "ztrl orthogonalise");
}

int lz_ztrl_get_vectors(lz_handle h, int k, double* Y_out) {
  LZ_TRY(ztrl_state(h, "lz_ztrl_get_vectors"));
  if (!Y_out || k < 1 || k > h->z.m) return fail(h, LZ_ERR_ARG, "lz_ztrl_get_vectors: need 1 <= k <= m and Y_out");
  return orth_get_vectors(h, h->z.B, k, Y_out);
}

int lz_ztrl_residuals(lz_handle h, int k, const double* theta, double* out) {
  LZ_TRY(ztrl_state(h, "lz_ztrl_residuals"));
  ZState& z = h->z;
  if (!theta || !out || k < 1 || k > z.m) return fail(h, LZ_ERR_ARG, "lz_ztrl_residuals: need 1 <= k <= m, theta and out");
  const ZSmall L = ztrl_small_layout(z.m);
  double* dth = z.wk.sm + L.theta;
  LZ_TRY(upload(h, dth, theta, (size_t)k * sizeof(double)));
  LZ_TRY(orth_resid_norms(h, z.B, z.wk, k, dth, z.wk.sm + L.res, [&](int i) {
    z_matvec(h, z.B.B + (int64_t)(2 * i) * z.B.ld, z.B.w, z.B.ld);
    return hipSuccess;
  }));
  LZ_TRY(check_launch(h, "ztrl residuals"));
  LZ_HIP(h, hipMemcpyAsync(out, z.wk.sm + L.res, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_ztrl_set_rows(lz_handle h, int j0, int count, const double* rows, int64_t ld) {
  LZ_TRY(ztrl_state(h, "lz_ztrl_set_rows"));
  return orth_set_rows(h, h->z.B, "lz_ztrl_set_rows", "m", j0, count, rows, ld);
}

int lz_ztrl_get_rows(lz_handle h, int j0, int count, double* rows, int64_t ld) {
  LZ_TRY(ztrl_state(h, "lz_ztrl_get_rows"));
  return orth_get_rows(h, h->z.B, "lz_ztrl_get_rows", "m", j0, count, rows, ld);
}

}  // extern "C"
