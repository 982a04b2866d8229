// C ABI of the Golub-Kahan-Lanczos solver (include/lanczos_hip.h, "Golub-Kahan-Lanczos"): the device half of lanczos_amd.svds.
// The state (h->gk: the rectangular matrix and its transpose, the bases U and V, work vectors, small arrays) is separate from the
// handle's square operator: h->kind, h->rows, a fixed-n run's V / Y and a thick-restart basis on the same handle stay as they are.
// The Gram-Schmidt walks, the restart and the normalisation are the thick-restart solver's kernels (lz_reorth.hip, lz_trl.hip), one
// QtwPlan per row length; the products are launch_spmv_rect (lz_gk.hip) - these matrices never reach launch_spmv_csr or any of the
// square layouts, whose epilogue reads x_own[row].
#include "lz_context.h"

using namespace lz;
using namespace lz::api;

namespace {

// d_sm: c of pass 1 and of pass 2 (cl doubles each), nrm2, the coefficients on U (m x m, row j: step j), the coefficients on V of the
// step under way (never read back), alpha, beta, the restart's P or Q (m x m), sigma, the 2 m residual norms
struct GkSmall {
  int64_t c1, c2, nrm2, proj, projv, alpha, beta, S, sig, res, total;
};
GkSmall gk_small_layout(int m) {
  GkSmall L;
  const int64_t cl = qtw_ldp(m + 2) + 16;
  L.c1 = 0;
  L.c2 = cl;
  L.nrm2 = 2 * cl;
  L.proj = L.nrm2 + 8;
  L.projv = L.proj + (int64_t)m * m;
  L.alpha = L.projv + m + 8;
  L.beta = L.alpha + m + 8;
  L.S = L.beta + m + 8;
  L.sig = L.S + (int64_t)m * m;
  L.res = L.sig + m + 8;
  L.total = L.res + 2 * m + 8;
  return L;
}

// one side of the bidiagonalisation: its basis, work vector and lengths
struct GkSide {
  double* B;
  double* w;
  int64_t len, pad, ld;
  QtwPlan plan;
};
GkSide gk_side(lz_handle h, int side) {  // 0: U (length p), 1: V (length q)
  GkState& g = h->gk;
  GkSide s;
  s.B = side == 0 ? g.d_U : g.d_V;
  s.w = side == 0 ? g.d_wu : g.d_wv;
  s.len = side == 0 ? g.p : g.q;
  s.pad = side == 0 ? g.p_pad : g.q_pad;
  s.ld = side == 0 ? g.ldp : g.ldq;
  s.plan = plan_qtw(s.pad, h->flags & ~(LZ_FLAG_QTW_MFMA | LZ_FLAG_ONE_REDUCE), h->tune, g.m + 2);
  return s;
}

int gk_state(lz_handle h, const char* who, bool need_basis) {
  if (!h) return LZ_ERR_ARG;
  if (!h->gk.set) return fail(h, LZ_ERR_STATE, std::string(who) + ": no rectangular matrix (lz_gk_set_csr first)");
  if (need_basis && h->gk.m == 0) return fail(h, LZ_ERR_STATE, std::string(who) + ": no basis (lz_gk_begin first)");
  LZ_HIP(h, hipSetDevice(h->dev));
  return LZ_OK;
}

int gk_side_arg(lz_handle h, const char* who, int side) {
  if (side != 0 && side != 1) return fail(h, LZ_ERR_ARG, std::string(who) + ": side is 0 (U, the long side) or 1 (V, the short side)");
  return LZ_OK;
}

// the work items of launch_spmv_rect and the bookkeeping fill_csr_meta would do, without any of the square layouts
int gk_fill_meta(lz_handle h, CsrDev& A, const int32_t* rowptr_host, int64_t rows, int64_t ncols, int64_t nnz, int max_nnz) {
  A.host_colidx = nullptr;  // (upload_csr left the caller's arrays here for pb_build: not used)
  A.host_vals = nullptr;
  int cap = h->tune[4] > 0 ? h->tune[4] : 4096;  // the LDS tile, and the segment cap of a long row
  cap = std::min(std::max(cap, 256), 8190);       // (at most 64 KiB of products)
  A.blk_nnz_cap = cap;
  A.rows = rows;
  A.ncols = ncols;
  A.nnz = nnz;
  A.fixed_k = 0;
  A.max_row_nnz = max_nnz;
  A.avg_row_nnz = (double)nnz / (double)rows;
  A.n_rowblk = 0;
  std::vector<int32_t> items, lrows;
  int nslots = 0;
  rect_plan(rowptr_host, rows, cap, !(h->flags & LZ_FLAG_SPMV_STREAM), items, lrows, &nslots);
  LZ_TRY(dev_alloc(h, A.rect_items, items.size()));
  LZ_TRY(dev_alloc(h, A.rect_long, lrows.size()));
  LZ_TRY(dev_alloc(h, A.rect_seg, (size_t)nslots));
  LZ_HIP(h, hipMemcpy(A.rect_items, items.data(), items.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  if (!lrows.empty()) LZ_HIP(h, hipMemcpy(A.rect_long, lrows.data(), lrows.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  A.n_rect = (int)(items.size() / 4);
  A.n_rect_long = (int)(lrows.size() / 4);
  return LZ_OK;
}

void gk_free_csr(CsrDev& A) {
  big_free(A.rowptr);
  big_free(A.colidx);
  big_free(A.vals);
  big_free(A.rect_items);
  big_free(A.rect_long);
  big_free(A.rect_seg);
  A = CsrDev();
}

int gk_free_basis(lz_handle h) {
  GkState& g = h->gk;
  LZ_TRY(dev_free(h, g.d_U));
  LZ_TRY(dev_free(h, g.d_V));
  g.m = 0;
  return LZ_OK;
}

// row k of the side's basis = x (in the side's work vector, zero padding) made orthogonal to rows [0, k) by two CGS passes, normalised
int gk_orth_store(lz_handle h, int side, int k) {
  GkState& g = h->gk;
  const GkSmall L = gk_small_layout(g.m);
  const GkSide s = gk_side(h, side);
  double* sm = g.d_sm;
  int np = 0;
  for (int pass = 0; pass < (k > 0 ? 2 : 0); ++pass) {
    LZ_HIP(h, launch_qtw(s.B, s.ld, s.pad, k + 1, k, s.w, nullptr, nullptr, s.plan, g.d_part, 2, h->stream));
    launch_final_rows(g.d_part, k + 1, s.plan.P, sm + L.c1, h->stream, s.plan.family == 2);
    np = launch_trl_cgs(s.B, s.ld, s.pad, k, sm + L.c1, s.w, g.d_part, nullptr, h->stream);
  }
  if (k == 0) np = launch_trl_cgs(s.B, s.ld, s.pad, 0, sm + L.c1, s.w, g.d_part, nullptr, h->stream);  // |x|^2 only
  launch_trl_post(2, g.d_part, np, nullptr, 0, sm + L.nrm2, nullptr, g.d_gate, 0, h->stream);
  launch_scale_store(s.B + (int64_t)k * s.ld, s.w, sm + L.nrm2, sm + L.nrm2 + 1, s.pad, h->stream);
  LZ_TRY(check_launch(h, "gk orthogonalise"));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int gk_upload_x(lz_handle h, int side, const double* x) {
  const GkSide s = gk_side(h, side);
  LZ_HIP(h, hipMemsetAsync(s.w, 0, (size_t)s.ld * sizeof(double), h->stream));
  LZ_TRY(upload(h, s.w, x, (size_t)s.len * sizeof(double)));
  return LZ_OK;
}

// one half step: w (the side's work vector, holding the product) against rows [0, nb) of the side's basis - CGS, a second pass behind
// the DGKS gate -, its norm to norm_slot, w / norm to row nb.  proj: where the nb measured coefficients go (both passes' sums).
int gk_half_step(lz_handle h, const GkSide& s, int nb, double* proj, double* norm_slot, int force) {
  GkState& g = h->gk;
  const GkSmall L = gk_small_layout(g.m);
  double* sm = g.d_sm;
  if (nb > 0) {
    QtwFuse gated;
    gated.gate = g.d_gate;
    // pass 1: c = B[0..nb) . w (row nb is the self slot: c[nb] = w.w), w -= sum c_i B_i
    LZ_HIP(h, launch_qtw(s.B, s.ld, s.pad, nb + 1, nb, s.w, nullptr, nullptr, s.plan, g.d_part, 2, h->stream));
    launch_final_rows(g.d_part, nb + 1, s.plan.P, sm + L.c1, h->stream, s.plan.family == 2);
    int np = launch_trl_cgs(s.B, s.ld, s.pad, nb, sm + L.c1, s.w, g.d_part, nullptr, h->stream);
    launch_trl_post(0, g.d_part, np, sm + L.c1, nb - 1, sm + L.nrm2, proj, g.d_gate, force, h->stream);
    // pass 2, only where pass 1 cancelled more than half of |w| (or LZ_FLAG_TRL_PASS2_ALWAYS forces it)
    LZ_HIP(h, launch_qtw(s.B, s.ld, s.pad, nb + 1, nb, s.w, nullptr, nullptr, s.plan, g.d_part, 2, h->stream, &gated));
    launch_final_rows(g.d_part, nb + 1, s.plan.P, sm + L.c2, h->stream, s.plan.family == 2, g.d_gate);
    np = launch_trl_cgs(s.B, s.ld, s.pad, nb, sm + L.c2, s.w, g.d_part, g.d_gate, h->stream);
    launch_trl_post(1, g.d_part, np, sm + L.c2, nb - 1, sm + L.nrm2, proj, g.d_gate, force, h->stream);
  } else {  // nothing to project on: the norm only
    const int np = launch_trl_cgs(s.B, s.ld, s.pad, 0, sm + L.c1, s.w, g.d_part, nullptr, h->stream);
    launch_trl_post(2, g.d_part, np, nullptr, 0, sm + L.nrm2, nullptr, g.d_gate, 0, h->stream);
  }
  launch_scale_store(s.B + (int64_t)nb * s.ld, s.w, sm + L.nrm2, norm_slot, s.pad, h->stream);
  return LZ_OK;
}

}  // namespace

namespace lz {
namespace api {
void gk_free(lz_handle h) {
  GkState& g = h->gk;
  gk_free_csr(g.A);
  gk_free_csr(g.AT);
  big_free(g.d_U);
  big_free(g.d_V);
  big_free(g.d_wu);
  big_free(g.d_wv);
  big_free(g.d_sm);
  big_free(g.d_gate);
  big_free(g.d_part);
  g.d_U = g.d_V = g.d_wu = g.d_wv = g.d_sm = g.d_part = nullptr;
  g.d_gate = nullptr;
  g.part_cap = 0;
  g.m = 0;
  g.u_ready = -1;
  g.set = false;
}
}  // namespace api
}  // namespace lz

extern "C" {

int lz_gk_set_csr(lz_handle h, int64_t p, int64_t q, int64_t nnz, const int32_t* rowptr, const int32_t* colidx, const double* vals,
                  const int32_t* rowptrT, const int32_t* colidxT, const double* valsT) {
  if (!h) return LZ_ERR_ARG;
  if (q < 2 || p < q || nnz < 0 || !rowptr || !rowptrT || (nnz > 0 && (!colidx || !vals || !colidxT || !valsT)))
    return fail(h, LZ_ERR_ARG, "lz_gk_set_csr: need p >= q >= 2, nnz >= 0 and both CSR arrays (A: p x q, its transpose: q x p)");
  if (p >= (int64_t)1 << 31 || nnz >= (int64_t)1 << 31) return fail(h, LZ_ERR_ARG, "lz_gk_set_csr: sizes exceed int32 CSR indexing");
  if (h->world > 1 || h->comm_kind != 0)
    return fail(h, LZ_ERR_STATE, "lz_gk_set_csr: the Golub-Kahan-Lanczos solver runs on one rank (this handle has a communicator)");
  LZ_HIP(h, hipSetDevice(h->dev));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  GkState& g = h->gk;
  g.set = false;
  LZ_TRY(gk_free_basis(h));
  int fixed_k = 0, max_nnz = 0, max_nnzT = 0;
  LZ_TRY(upload_csr(h, g.A, "lz_gk_set_csr", p, q, nnz, rowptr, colidx, vals, &fixed_k, &max_nnz));
  LZ_TRY(gk_fill_meta(h, g.A, rowptr, p, q, nnz, max_nnz));
  LZ_TRY(upload_csr(h, g.AT, "lz_gk_set_csr (transpose)", q, p, nnz, rowptrT, colidxT, valsT, &fixed_k, &max_nnzT));
  LZ_TRY(gk_fill_meta(h, g.AT, rowptrT, q, p, nnz, max_nnzT));
  g.p = p;
  g.q = q;
  g.p_pad = round_up(p, kPadDoubles);
  g.q_pad = round_up(q, kPadDoubles);
  g.ldp = skew_stride(h, g.p_pad);
  g.ldq = skew_stride(h, g.q_pad);
  LZ_TRY(dev_alloc(h, g.d_wu, (size_t)g.ldp));
  LZ_TRY(dev_alloc(h, g.d_wv, (size_t)g.ldq));
  LZ_HIP(h, hipMemsetAsync(g.d_wu, 0, (size_t)g.ldp * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(g.d_wv, 0, (size_t)g.ldq * sizeof(double), h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  g.set = true;
  return LZ_OK;
}

int lz_gk_begin(lz_handle h, int m, const double* v0) {
  LZ_TRY(gk_state(h, "lz_gk_begin", false));
  GkState& g = h->gk;
  if (!v0 || m < 2 || m > 128 || m > g.q) return fail(h, LZ_ERR_ARG, "lz_gk_begin: need 2 <= m <= min(128, q) and v0");
  if (h->flags & (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE))
    return fail(h, LZ_ERR_STATE, "lz_gk_begin: not with LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE");
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  const size_t nrows = (size_t)m + 1;
  if (!g.d_U || g.m != m) {
    g.m = 0;
    LZ_TRY(dev_alloc(h, g.d_U, nrows * (size_t)g.ldp));
    LZ_TRY(dev_alloc(h, g.d_V, nrows * (size_t)g.ldq));
    LZ_TRY(dev_alloc(h, g.d_sm, (size_t)gk_small_layout(m).total));
    LZ_TRY(dev_alloc(h, g.d_gate, 4));
    g.m = m;
  }
  size_t need = 0;
  for (int side = 0; side < 2; ++side) {
    const GkSide s = gk_side(h, side);
    need = std::max<size_t>(need, (size_t)(m + 2 + 32) * (size_t)s.plan.P);
    need = std::max<size_t>(need, (size_t)trl_cgs_blocks(s.pad));
    need = std::max<size_t>(need, (size_t)m * (size_t)((s.len + kTPB - 1) / kTPB) + 64);  // residual norms
  }
  need += 8192;
  if (need > g.part_cap) {
    LZ_TRY(dev_alloc(h, g.d_part, need));
    g.part_cap = need;
  }
  LZ_HIP(h, hipMemsetAsync(g.d_U, 0, nrows * (size_t)g.ldp * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(g.d_V, 0, nrows * (size_t)g.ldq * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(g.d_sm, 0, (size_t)gk_small_layout(m).total * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(g.d_gate, 0, 4 * sizeof(int), h->stream));
  g.u_ready = -1;
  LZ_TRY(gk_upload_x(h, 1, v0));
  return gk_orth_store(h, 1, 0);
}

int lz_gk_extend(lz_handle h, int k, int m, double* colproj_out, double* alpha_out, double* beta_out) {
  LZ_TRY(gk_state(h, "lz_gk_extend", true));
  GkState& g = h->gk;
  if (m != g.m || k < 0 || k >= m) return fail(h, LZ_ERR_ARG, "lz_gk_extend: need m == the m of lz_gk_begin and 0 <= k < m");
  const GkSmall L = gk_small_layout(m);
  double* sm = g.d_sm;
  const GkSide su = gk_side(h, 0), sv = gk_side(h, 1);
  const int force = (h->flags & LZ_FLAG_TRL_PASS2_ALWAYS) != 0;
  const int u_ready = g.u_ready == k ? k : -1;
  g.u_ready = -1;
  for (int j = k; j < m; ++j) {
    // w = A V[j] against U[0..j): column j of B above the diagonal, alpha_j = |w|, U[j] = w / alpha_j
    // (not when U[j] is the probed direction that replaces a vanished alpha_j: the step resumes at its second half)
    if (j != u_ready) {
      LZ_HIP(h, launch_spmv_rect(g.A, sv.B + (int64_t)j * sv.ld, su.w, su.pad, h->stream));
      LZ_TRY(gk_half_step(h, su, j, sm + L.proj + (int64_t)j * m, sm + L.alpha + j, force));
    }
    // z = A^T U[j] against V[0..j]: beta_j = |z|, V[j + 1] = z / beta_j (the coefficients are alpha_j on V[j] and rounding elsewhere)
    LZ_HIP(h, launch_spmv_rect(g.AT, su.B + (int64_t)j * su.ld, sv.w, sv.pad, h->stream));
    LZ_TRY(gk_half_step(h, sv, j + 1, sm + L.projv, sm + L.beta + j, force));
    LZ_TRY(check_launch(h, "gk extend"));
  }
  if (colproj_out) LZ_HIP(h, hipMemcpyAsync(colproj_out, sm + L.proj, (size_t)m * m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (alpha_out) LZ_HIP(h, hipMemcpyAsync(alpha_out, sm + L.alpha, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (beta_out) LZ_HIP(h, hipMemcpyAsync(beta_out, sm + L.beta, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_gk_restart(lz_handle h, int m, int kk, const double* P, const double* Q) {
  LZ_TRY(gk_state(h, "lz_gk_restart", true));
  GkState& g = h->gk;
  if (!P || !Q || m != g.m || kk < 1 || kk >= m) return fail(h, LZ_ERR_ARG, "lz_gk_restart: need m == the m of lz_gk_begin, 1 <= kk < m, P and Q");
  const GkSmall L = gk_small_layout(m);
  g.u_ready = -1;
  double* S = g.d_sm + L.S;
  LZ_TRY(upload(h, S, P, (size_t)m * kk * sizeof(double)));
  LZ_HIP(h, launch_trl_restart(g.d_U, g.ldp, g.p, m, kk, S, h->stream));  // (U[kk] = U[m], the zero row: the next step overwrites it)
  LZ_TRY(upload(h, S, Q, (size_t)m * kk * sizeof(double)));               // (stream order: behind the kernel that read P)
  LZ_HIP(h, launch_trl_restart(g.d_V, g.ldq, g.q, m, kk, S, h->stream));
  LZ_TRY(check_launch(h, "gk restart"));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_gk_probe(lz_handle h, int side, int k, const double* x) {
  LZ_TRY(gk_state(h, "lz_gk_probe", true));
  LZ_TRY(gk_side_arg(h, "lz_gk_probe", side));
  if (!x || k < 0 || k > h->gk.m - (side == 0 ? 1 : 0)) return fail(h, LZ_ERR_ARG, "lz_gk_probe: need x and 0 <= k <= m (V) or 0 <= k < m (U)");
  LZ_TRY(gk_upload_x(h, side, x));
  LZ_TRY(gk_orth_store(h, side, k));
  if (side == 0) h->gk.u_ready = k;
  return LZ_OK;
}

int lz_gk_get_vectors(lz_handle h, int side, int k, double* out) {
  LZ_TRY(gk_state(h, "lz_gk_get_vectors", true));
  LZ_TRY(gk_side_arg(h, "lz_gk_get_vectors", side));
  if (!out || k < 1 || k > h->gk.m) return fail(h, LZ_ERR_ARG, "lz_gk_get_vectors: need 1 <= k <= m and out");
  const GkSide s = gk_side(h, side);
  const int64_t M = s.len;
  std::vector<double> rowsk((size_t)k * (size_t)M);
  LZ_HIP(h, xfer_d2h(h->dev, h->stream, h->xfer, rowsk.data(), (size_t)M * sizeof(double), s.B, (size_t)s.ld * sizeof(double),
                     (size_t)M * sizeof(double), (size_t)k));
  parallel_ranges(M, 1 << 16, [&](int, int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r)
      for (int i = 0; i < k; ++i) out[r * k + i] = rowsk[(size_t)i * M + r];
  });
  return LZ_OK;
}

int lz_gk_set_rows(lz_handle h, int side, int j0, int count, const double* rows, int64_t ld) {
  LZ_TRY(gk_state(h, "lz_gk_set_rows", true));
  LZ_TRY(gk_side_arg(h, "lz_gk_set_rows", side));
  const GkSide s = gk_side(h, side);
  if (!rows || j0 < 0 || count < 1 || j0 + count > h->gk.m + 1 || ld < s.pad)
    return fail(h, LZ_ERR_ARG, "lz_gk_set_rows: need rows j0 .. j0 + count - 1 <= m and ld >= the padded row length");
  LZ_TRY(upload2d(h, s.B + (int64_t)j0 * s.ld, (size_t)s.ld * sizeof(double), rows, (size_t)ld * sizeof(double), (size_t)s.pad * sizeof(double),
                  (size_t)count));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_gk_get_rows(lz_handle h, int side, int j0, int count, double* rows, int64_t ld) {
  LZ_TRY(gk_state(h, "lz_gk_get_rows", true));
  LZ_TRY(gk_side_arg(h, "lz_gk_get_rows", side));
  const GkSide s = gk_side(h, side);
  if (!rows || j0 < 0 || count < 1 || j0 + count > h->gk.m + 1 || ld < s.pad)
    return fail(h, LZ_ERR_ARG, "lz_gk_get_rows: need rows j0 .. j0 + count - 1 <= m and ld >= the padded row length");
  LZ_HIP(h, hipMemcpy2DAsync(rows, (size_t)ld * sizeof(double), s.B + (int64_t)j0 * s.ld, (size_t)s.ld * sizeof(double),
                             (size_t)s.pad * sizeof(double), (size_t)count, hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_gk_residuals(lz_handle h, int k, const double* sigma, double* out) {
  LZ_TRY(gk_state(h, "lz_gk_residuals", true));
  GkState& g = h->gk;
  if (!sigma || !out || k < 1 || k > g.m) return fail(h, LZ_ERR_ARG, "lz_gk_residuals: need 1 <= k <= m, sigma and out");
  const GkSmall L = gk_small_layout(g.m);
  double* dsig = g.d_sm + L.sig;
  LZ_TRY(upload(h, dsig, sigma, (size_t)k * sizeof(double)));
  const GkSide su = gk_side(h, 0), sv = gk_side(h, 1);
  for (int side = 0; side < 2; ++side) {  // 0: |A v_i - sigma_i u_i| (length p), 1: |A^T u_i - sigma_i v_i| (length q)
    const GkSide& in = side == 0 ? sv : su;
    const GkSide& o = side == 0 ? su : sv;
    int G = 0;
    for (int i = 0; i < k; ++i) {
      LZ_HIP(h, launch_spmv_rect(side == 0 ? g.A : g.AT, in.B + (int64_t)i * in.ld, o.w, o.pad, h->stream));
      G = launch_trl_resid_diff(o.w, o.B + (int64_t)i * o.ld, o.len, dsig, i, g.d_part, h->stream);
    }
    launch_trl_rownorm(g.d_part, G, k, g.d_sm + L.res + (int64_t)side * k, h->stream);
  }
  LZ_TRY(check_launch(h, "gk residuals"));
  LZ_HIP(h, hipMemcpyAsync(out, g.d_sm + L.res, (size_t)2 * k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_gk_spmv(lz_handle h, int transpose, const double* x, double* y) {
  LZ_TRY(gk_state(h, "lz_gk_spmv", false));
  if (!x || !y) return fail(h, LZ_ERR_ARG, "lz_gk_spmv: need x and y");
  GkState& g = h->gk;
  double* dx = transpose ? g.d_wu : g.d_wv;
  double* dy = transpose ? g.d_wv : g.d_wu;
  const int64_t nx = transpose ? g.p : g.q, ny_pad = transpose ? g.q_pad : g.p_pad;
  LZ_TRY(upload(h, dx, x, (size_t)nx * sizeof(double)));
  LZ_HIP(h, hipMemsetAsync(dy, 0xff, (size_t)ny_pad * sizeof(double), h->stream));  // NaN: whatever the kernel leaves unwritten shows
  LZ_HIP(h, launch_spmv_rect(transpose ? g.AT : g.A, dx, dy, ny_pad, h->stream));
  LZ_TRY(check_launch(h, "gk spmv"));
  LZ_HIP(h, hipMemcpyAsync(y, dy, (size_t)ny_pad * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_gk_spmv_time(lz_handle h, int transpose, int reps, double* ms_out) {
  LZ_TRY(gk_state(h, "lz_gk_spmv_time", false));
  if (!ms_out || reps < 1) return fail(h, LZ_ERR_ARG, "lz_gk_spmv_time: need reps >= 1 and ms_out");
  GkState& g = h->gk;
  const double* dx = transpose ? g.d_wu : g.d_wv;
  double* dy = transpose ? g.d_wv : g.d_wu;
  const int64_t ny_pad = transpose ? g.q_pad : g.p_pad;
  hipEvent_t a, b;
  LZ_HIP(h, hipEventCreate(&a));
  LZ_HIP(h, hipEventCreate(&b));
  hipError_t e = launch_spmv_rect(transpose ? g.AT : g.A, dx, dy, ny_pad, h->stream);  // warm-up
  if (e == hipSuccess) e = hipEventRecord(a, h->stream);
  for (int r = 0; r < reps && e == hipSuccess; ++r) e = launch_spmv_rect(transpose ? g.AT : g.A, dx, dy, ny_pad, h->stream);
  if (e == hipSuccess) e = hipEventRecord(b, h->stream);
  if (e == hipSuccess) e = hipEventSynchronize(b);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
  hipEventDestroy(a);
  hipEventDestroy(b);
  LZ_HIP(h, e);
  LZ_TRY(check_launch(h, "gk spmv time"));
  *ms_out = (double)ms / reps;
  return LZ_OK;
}

}  // extern "C"
