// C ABI of the Golub-Kahan-Lanczos solver (include/lanczos_hip.h, "Golub-Kahan-Lanczos"): the device half of lanczos_amd.svds.
// The state (h->gk: the rectangular matrix and its transpose, the bases U and V, work vectors, small arrays) is separate from the
// handle's square operator: h->kind, h->rows, a fixed-n run's V / Y and a thick-restart basis on the same handle stay as they are.
// What is here is the solver's own: the rectangular matrices and their work items, the alternating step with its resumed half, the
// two-sided restart, the residuals and the product probes.  Orthogonalising against U or V - an OrthBasis each, with one OrthWork
// between them - and the row transfers are the basis layer's (lz_orth.hip), shared with the thick-restart solvers; the products go
// through gk_product: launch_spmv_rect (lz_gk.hip) for a CSR operator - these matrices never reach launch_spmv_csr or any of the square
// layouts, whose epilogue reads x_own[row] - or the rowdot / colsum kernels on the one dense copy of lz_gk_set_dense.
#include "lz_context.h"

using namespace lz;
using namespace lz::api;

namespace {

// wk.sm: the basis layer's head (c of both passes, nrm2), the coefficients on U (m x m, row j: step j), the coefficients on V of the
// step under way (never read back), alpha, beta, the restart's P or Q (m x m), sigma, the 2 m residual norms
struct GkSmall : OrthSmallHead {
  int64_t proj, projv, alpha, beta, S, sig, res, total;
};
GkSmall gk_small_layout(int m) {
  GkSmall L;
  static_cast<OrthSmallHead&>(L) = orth_small_head(m + 1);
  L.proj = L.end;
  L.projv = L.proj + (int64_t)m * m;
  L.alpha = L.projv + m + 8;
  L.beta = L.alpha + m + 8;
  L.S = L.beta + m + 8;
  L.sig = L.S + (int64_t)m * m;
  L.res = L.sig + m + 8;
  L.total = L.res + 2 * m + 8;
  return L;
}

OrthBasis& gk_basis(lz_handle h, int side) { return side == 0 ? h->gk.U : h->gk.V; }  // 0: U (length p), 1: V (length q)

int gk_state(lz_handle h, const char* who, bool need_basis) {
  if (!h) return LZ_ERR_ARG;
  if (!h->gk.set) return fail(h, LZ_ERR_STATE, std::string(who) + ": no rectangular matrix (lz_gk_set_csr or lz_gk_set_dense first)");
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

void gk_free_dense(DenseDev& D) {
  big_free(D.S);
  big_free(D.rd_part);
  big_free(D.cs_part);
  D = DenseDev();
}

// the work vectors of both sides, sized for (p, q); the basis of an earlier operator is gone by now
int gk_alloc_work(lz_handle h, int64_t p, int64_t q) {
  GkState& g = h->gk;
  g.U.len = p;
  g.V.len = q;
  for (OrthBasis* b : {&g.U, &g.V}) {
    b->pad = round_up(b->len, kPadDoubles);
    b->ld = skew_stride(h, b->pad);
    LZ_TRY(dev_alloc(h, b->w, (size_t)b->ld));
  }
  LZ_HIP(h, hipMemsetAsync(g.U.w, 0, (size_t)g.U.ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(g.V.w, 0, (size_t)g.V.ld * sizeof(double), h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int gk_free_basis(lz_handle h) {
  GkState& g = h->gk;
  LZ_TRY(dev_free(h, g.U.B));
  LZ_TRY(dev_free(h, g.V.B));
  g.m = 0;
  return LZ_OK;
}

// row k of the side's basis = x made orthogonal to rows [0, k), normalised
int gk_store_x(lz_handle h, int side, int k, const double* x) {
  const OrthBasis& b = gk_basis(h, side);
  LZ_TRY(orth_upload_x(h, b, x));
  return orth_store(h, b, h->gk.wk, orth_plan(h, b), k, "gk orthogonalise");
}

}  // namespace

namespace lz {
namespace api {
// y = Aop x (transpose == 0) or Aop^T x with whichever operator the state holds; y[len .. pad) = 0
hipError_t gk_product(lz_handle h, int transpose, const double* x, double* y, int64_t pad) {
  const GkState& g = h->gk;
  if (!g.D.S) return launch_spmv_rect(transpose ? g.AT : g.A, x, y, pad, h->stream);
  return (transpose != 0) == g.D.stored_t ? launch_dense_rowdot(g.D, x, y, pad, h->stream) : launch_dense_colsum(g.D, x, y, pad, h->stream);
}

void gk_free(lz_handle h) {
  GkState& g = h->gk;
  gk_free_csr(g.A);
  gk_free_csr(g.AT);
  gk_free_dense(g.D);
  orth_free(g.U);
  orth_free(g.V);
  orth_free(g.wk);
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
  h->ls.live = false;  // (the least-squares state was made for the matrix that goes)
  LZ_TRY(gk_free_basis(h));
  gk_free_dense(g.D);
  int fixed_k = 0, max_nnz = 0, max_nnzT = 0;
  LZ_TRY(upload_csr(h, g.A, "lz_gk_set_csr", p, q, nnz, rowptr, colidx, vals, &fixed_k, &max_nnz));
  LZ_TRY(gk_fill_meta(h, g.A, rowptr, p, q, nnz, max_nnz));
  LZ_TRY(upload_csr(h, g.AT, "lz_gk_set_csr (transpose)", q, p, nnz, rowptrT, colidxT, valsT, &fixed_k, &max_nnzT));
  LZ_TRY(gk_fill_meta(h, g.AT, rowptrT, q, p, nnz, max_nnzT));
  LZ_TRY(gk_alloc_work(h, p, q));
  g.set = true;
  return LZ_OK;
}

int lz_gk_set_dense(lz_handle h, int64_t p, int64_t q, const double* S, int64_t ld_host, int stored_transposed) {
  if (!h) return LZ_ERR_ARG;
  const int64_t R = stored_transposed ? q : p, C = stored_transposed ? p : q;
  if (q < 2 || p < q || !S || ld_host < C)
    return fail(h, LZ_ERR_ARG, "lz_gk_set_dense: need p >= q >= 2, S (row-major, p x q, or q x p when stored_transposed) and ld_host >= its row length");
  if (p >= (int64_t)1 << 31) return fail(h, LZ_ERR_ARG, "lz_gk_set_dense: sizes exceed int32 indexing");
  if (h->world > 1 || h->comm_kind != 0)
    return fail(h, LZ_ERR_STATE, "lz_gk_set_dense: the Golub-Kahan-Lanczos solver runs on one rank (this handle has a communicator)");
  LZ_HIP(h, hipSetDevice(h->dev));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  GkState& g = h->gk;
  g.set = false;
  h->ls.live = false;  // (the least-squares state was made for the matrix that goes)
  LZ_TRY(gk_free_basis(h));
  gk_free_csr(g.A);
  gk_free_csr(g.AT);
  gk_free_dense(g.D);
  DenseDev D;
  D.R = R;
  D.C = C;
  D.ld = round_up(C, 2);
  D.stored_t = stored_transposed != 0;
  // knob 14 (the SpMV plan): rowdot form + 4 * colsum form, 0 = by shape; knob 4 (entries per segment of a long row): the segment
  // length; knob 2 (rows per block): the slab height
  dense_plan(D, h->tune[14] & 3, (h->tune[14] >> 2) & 3, h->tune[4], h->tune[2]);
  g.D = D;  // (from here on gk_free_dense releases whatever has been allocated)
  LZ_TRY(dev_alloc(h, g.D.S, (size_t)R * (size_t)D.ld));
  LZ_TRY(dev_alloc(h, g.D.rd_part, (size_t)D.rd_nseg * (size_t)round_up(R, kPadDoubles)));
  LZ_TRY(dev_alloc(h, g.D.cs_part, D.cs_form == kCsOne ? 0 : (size_t)D.cs_nslab * (size_t)round_up(C, kPadDoubles)));
  if (D.ld > C) LZ_HIP(h, hipMemset2D(g.D.S + C, (size_t)D.ld * sizeof(double), 0, sizeof(double), (size_t)R));  // the padding column
  LZ_HIP(h, hipMemcpy2D(g.D.S, (size_t)D.ld * sizeof(double), S, (size_t)ld_host * sizeof(double), (size_t)C * sizeof(double), (size_t)R,
                        hipMemcpyHostToDevice));
  LZ_TRY(gk_alloc_work(h, p, q));
  g.set = true;
  return LZ_OK;
}

int lz_gk_plan(lz_handle h, int* out) {
  LZ_TRY(gk_state(h, "lz_gk_plan", false));
  if (!out) return fail(h, LZ_ERR_ARG, "lz_gk_plan: need out (4 ints)");
  const DenseDev& D = h->gk.D;
  const bool dense = D.S != nullptr;
  out[0] = dense ? 1 : 0;
  out[1] = dense && D.stored_t ? 1 : 0;
  out[2] = !dense ? 0 : D.stored_t ? D.cs_form : D.rd_form;  // Aop x
  out[3] = !dense ? 0 : D.stored_t ? D.rd_form : D.cs_form;  // Aop^T u
  return LZ_OK;
}

int lz_gk_begin(lz_handle h, int m, const double* v0) {
  LZ_TRY(gk_state(h, "lz_gk_begin", false));
  GkState& g = h->gk;
  if (!v0 || m < 2 || m > 128 || m > g.V.len) return fail(h, LZ_ERR_ARG, "lz_gk_begin: need 2 <= m <= min(128, q) and v0");
  if (h->flags & (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE))
    return fail(h, LZ_ERR_STATE, "lz_gk_begin: not with LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE");
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  const size_t nrows = (size_t)m + 1;
  if (!g.U.B || g.m != m) {
    g.m = 0;
    LZ_TRY(dev_alloc(h, g.U.B, nrows * (size_t)g.U.ld));
    LZ_TRY(dev_alloc(h, g.V.B, nrows * (size_t)g.V.ld));
    LZ_TRY(dev_alloc(h, g.wk.sm, (size_t)gk_small_layout(m).total));
    LZ_TRY(dev_alloc(h, g.wk.gate, 4));
    g.m = m;
    g.U.nrows = g.V.nrows = m + 1;
  }
  LZ_TRY(orth_part_reserve(h, g.wk, std::max(orth_part_need(g.U, orth_plan(h, g.U), m), orth_part_need(g.V, orth_plan(h, g.V), m))));
  LZ_HIP(h, hipMemsetAsync(g.U.B, 0, nrows * (size_t)g.U.ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(g.V.B, 0, nrows * (size_t)g.V.ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(g.wk.sm, 0, (size_t)gk_small_layout(m).total * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(g.wk.gate, 0, 4 * sizeof(int), h->stream));
  g.u_ready = -1;
  return gk_store_x(h, 1, 0, v0);
}

int lz_gk_extend(lz_handle h, int k, int m, double* colproj_out, double* alpha_out, double* beta_out) {
  LZ_TRY(gk_state(h, "lz_gk_extend", true));
  GkState& g = h->gk;
  if (m != g.m || k < 0 || k >= m) return fail(h, LZ_ERR_ARG, "lz_gk_extend: need m == the m of lz_gk_begin and 0 <= k < m");
  const GkSmall L = gk_small_layout(m);
  double* sm = g.wk.sm;
  const OrthBasis &U = g.U, &V = g.V;
  const QtwPlan pu = orth_plan(h, U), pv = orth_plan(h, V);
  const OrthPass2 pass2 = (h->flags & LZ_FLAG_TRL_PASS2_ALWAYS) ? OrthPass2::kForced : OrthPass2::kGated;
  const int u_ready = g.u_ready == k ? k : -1;
  g.u_ready = -1;
  for (int j = k; j < m; ++j) {
    // w = A V[j] against U[0..j): column j of B above the diagonal, alpha_j = |w|, U[j] = w / alpha_j
    // (not when U[j] is the probed direction that replaces a vanished alpha_j: the step resumes at its second half)
    if (j != u_ready) {
      LZ_HIP(h, gk_product(h, 0, V.B + (int64_t)j * V.ld, U.w, U.pad));
      LZ_TRY(orth_cgs_step(h, U, g.wk, pu, j, sm + L.proj + (int64_t)j * m, sm + L.alpha + j, pass2));
    }
    // z = A^T U[j] against V[0..j]: beta_j = |z|, V[j + 1] = z / beta_j (the coefficients are alpha_j on V[j] and rounding elsewhere)
    LZ_HIP(h, gk_product(h, 1, U.B + (int64_t)j * U.ld, V.w, V.pad));
    LZ_TRY(orth_cgs_step(h, V, g.wk, pv, j + 1, sm + L.projv, sm + L.beta + j, pass2));
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
  double* S = g.wk.sm + L.S;
  LZ_TRY(upload(h, S, P, (size_t)m * kk * sizeof(double)));
  LZ_HIP(h, launch_trl_restart(g.U.B, g.U.ld, g.U.len, m, kk, S, h->stream));  // (U[kk] = U[m], the zero row: the next step overwrites it)
  LZ_TRY(upload(h, S, Q, (size_t)m * kk * sizeof(double)));                     // (stream order: behind the kernel that read P)
  LZ_HIP(h, launch_trl_restart(g.V.B, g.V.ld, g.V.len, m, kk, S, h->stream));
  LZ_TRY(check_launch(h, "gk restart"));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_gk_probe(lz_handle h, int side, int k, const double* x) {
  LZ_TRY(gk_state(h, "lz_gk_probe", true));
  LZ_TRY(gk_side_arg(h, "lz_gk_probe", side));
  if (!x || k < 0 || k > h->gk.m - (side == 0 ? 1 : 0)) return fail(h, LZ_ERR_ARG, "lz_gk_probe: need x and 0 <= k <= m (V) or 0 <= k < m (U)");
  LZ_TRY(gk_store_x(h, side, k, x));
  if (side == 0) h->gk.u_ready = k;
  return LZ_OK;
}

int lz_gk_get_vectors(lz_handle h, int side, int k, double* out) {
  LZ_TRY(gk_state(h, "lz_gk_get_vectors", true));
  LZ_TRY(gk_side_arg(h, "lz_gk_get_vectors", side));
  if (!out || k < 1 || k > h->gk.m) return fail(h, LZ_ERR_ARG, "lz_gk_get_vectors: need 1 <= k <= m and out");
  return orth_get_vectors(h, gk_basis(h, side), k, out);
}

int lz_gk_set_rows(lz_handle h, int side, int j0, int count, const double* rows, int64_t ld) {
  LZ_TRY(gk_state(h, "lz_gk_set_rows", true));
  LZ_TRY(gk_side_arg(h, "lz_gk_set_rows", side));
  return orth_set_rows(h, gk_basis(h, side), "lz_gk_set_rows", "m", j0, count, rows, ld);
}

int lz_gk_get_rows(lz_handle h, int side, int j0, int count, double* rows, int64_t ld) {
  LZ_TRY(gk_state(h, "lz_gk_get_rows", true));
  LZ_TRY(gk_side_arg(h, "lz_gk_get_rows", side));
  return orth_get_rows(h, gk_basis(h, side), "lz_gk_get_rows", "m", j0, count, rows, ld);
}

int lz_gk_residuals(lz_handle h, int k, const double* sigma, double* out) {
  LZ_TRY(gk_state(h, "lz_gk_residuals", true));
  GkState& g = h->gk;
  if (!sigma || !out || k < 1 || k > g.m) return fail(h, LZ_ERR_ARG, "lz_gk_residuals: need 1 <= k <= m, sigma and out");
  const GkSmall L = gk_small_layout(g.m);
  double* dsig = g.wk.sm + L.sig;
  LZ_TRY(upload(h, dsig, sigma, (size_t)k * sizeof(double)));
  for (int side = 0; side < 2; ++side) {  // 0: |A v_i - sigma_i u_i| (length p), 1: |A^T u_i - sigma_i v_i| (length q)
    const OrthBasis& in = gk_basis(h, 1 - side);
    const OrthBasis& o = gk_basis(h, side);
    LZ_TRY(orth_resid_norms(h, o, g.wk, k, dsig, g.wk.sm + L.res + (int64_t)side * k,
                            [&](int i) { return gk_product(h, side, in.B + (int64_t)i * in.ld, o.w, o.pad); }));
  }
  LZ_TRY(check_launch(h, "gk residuals"));
  LZ_HIP(h, hipMemcpyAsync(out, g.wk.sm + L.res, (size_t)2 * k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_gk_spmv(lz_handle h, int transpose, const double* x, double* y) {
  LZ_TRY(gk_state(h, "lz_gk_spmv", false));
  if (!x || !y) return fail(h, LZ_ERR_ARG, "lz_gk_spmv: need x and y");
  GkState& g = h->gk;
  double* dx = transpose ? g.U.w : g.V.w;
  double* dy = transpose ? g.V.w : g.U.w;
  const int64_t nx = transpose ? g.U.len : g.V.len, ny_pad = transpose ? g.V.pad : g.U.pad;
  const int64_t nx_pad = transpose ? g.U.pad : g.V.pad;
  LZ_TRY(upload(h, dx, x, (size_t)nx * sizeof(double)));
  LZ_HIP(h, hipMemsetAsync(dy, 0xff, (size_t)ny_pad * sizeof(double), h->stream));  // NaN: whatever the kernel leaves unwritten shows
  // ... and so does a read of x behind its length: NaN in the input's padding during the product, zero again (the walks' contract) after it
  if (nx_pad > nx) LZ_HIP(h, hipMemsetAsync(dx + nx, 0xff, (size_t)(nx_pad - nx) * sizeof(double), h->stream));
  LZ_HIP(h, gk_product(h, transpose, dx, dy, ny_pad));
  if (nx_pad > nx) LZ_HIP(h, hipMemsetAsync(dx + nx, 0, (size_t)(nx_pad - nx) * sizeof(double), h->stream));
  LZ_TRY(check_launch(h, "gk spmv"));
  LZ_HIP(h, hipMemcpyAsync(y, dy, (size_t)ny_pad * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_gk_spmv_time(lz_handle h, int transpose, int reps, double* ms_out) {
  LZ_TRY(gk_state(h, "lz_gk_spmv_time", false));
  if (!ms_out || reps < 1) return fail(h, LZ_ERR_ARG, "lz_gk_spmv_time: need reps >= 1 and ms_out");
  GkState& g = h->gk;
  const double* dx = transpose ? g.U.w : g.V.w;
  double* dy = transpose ? g.V.w : g.U.w;
  const int64_t ny_pad = transpose ? g.V.pad : g.U.pad;
  hipEvent_t a, b;
  LZ_HIP(h, hipEventCreate(&a));
  LZ_HIP(h, hipEventCreate(&b));
  hipError_t e = gk_product(h, transpose, dx, dy, ny_pad);  // warm-up
  if (e == hipSuccess) e = hipEventRecord(a, h->stream);
  for (int r = 0; r < reps && e == hipSuccess; ++r) e = gk_product(h, transpose, dx, dy, ny_pad);
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
