// Matrix exponential action (include/lanczos_hip.h, "matrix exponential action"): the device half of lanczos_amd.expm_multiply, the
// short-iterative Lanczos propagator.  A basis of its own (h->ex.B: m + 1 rows, real or planar complex), so the thick-restart bases of
// eigsh on the same handle are untouched.  Orthogonalising against it, the gated two-pass step, the row transfers and the norm are the
// basis layer's (lz_orth.hip); the combination of the rows is launch_trl_restart, on the real form of C for planar rows as
// lz_ztrl_restart builds it.  What is new here is the product of a REAL matrix with a PLANAR COMPLEX vector that reads the matrix once
// (k_spmv_csr_z2, k_gemv_z2), and the rule that chooses between it and two launches of the real product.
#include "lz_context.h"
#include "lz_device.h"

using namespace lz;
using namespace lz::api;

namespace lz {

// ------------------------------------------------------------------ CSR: (yr, yi) = A (xr, xi), A real, a group of G lanes per row
// The shape of k_zspmv_csr: lane g of a group takes entries g, g + G, ... of its row, the group adds its lanes' sums by a butterfly and
// lane 0 stores both planes.  An entry is one 8-byte value and one column index and serves both planes: two gathers and two fmas.
// An empty row stores an exact 0 in both planes.
// A group has kZ2Rows rows in flight, kTPB / G rows apart (so that the lanes of a wave still read neighbouring entries): with one row
// per group a lane waits out four dependent loads - row pointer, entry, gather, and the next row's pointer - for one entry, and the
// kernel ran at the rate the resident lanes turn over, 1.7e11 entries/s whatever the row length (0.25 - 0.5 of the HBM rate).  The
// rows of a group are independent chains, and each row's sum is formed in the order a single row in flight would form it.
constexpr int kZ2Rows = 4;
template <int G>
__global__ __launch_bounds__(kTPB) void k_spmv_csr_z2(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                      const double* __restrict__ vals, int64_t rows, const double* __restrict__ xr,
                                                      const double* __restrict__ xi, double* __restrict__ yr, double* __restrict__ yi) {
  constexpr int GPB = kTPB / G;  // groups of a block
  const int g = threadIdx.x & (G - 1);
  const int64_t row0 = (int64_t)blockIdx.x * (GPB * kZ2Rows) + threadIdx.x / G;
  int e[kZ2Rows], e1[kZ2Rows];
  double sr[kZ2Rows], si[kZ2Rows];
#pragma unroll
  for (int u = 0; u < kZ2Rows; ++u) {
    const int64_t row = row0 + (int64_t)u * GPB;
    const bool in = row < rows;
    e[u] = in ? rowptr[row] + g : 0;
    e1[u] = in ? rowptr[row + 1] : 0;
    sr[u] = si[u] = 0.0;
  }
  bool more = true;
  while (more) {
    double a[kZ2Rows];
    int32_t c[kZ2Rows];
#pragma unroll
    for (int u = 0; u < kZ2Rows; ++u) {
      const bool ok = e[u] < e1[u];
      a[u] = ok ? __builtin_nontemporal_load(vals + e[u]) : 0.0;
      c[u] = ok ? colidx[e[u]] : -1;
    }
    double br[kZ2Rows], bi[kZ2Rows];
#pragma unroll
    for (int u = 0; u < kZ2Rows; ++u) {
      br[u] = c[u] >= 0 ? xr[c[u]] : 0.0;
      bi[u] = c[u] >= 0 ? xi[c[u]] : 0.0;
    }
    more = false;
#pragma unroll
    for (int u = 0; u < kZ2Rows; ++u) {
      if (c[u] >= 0) {
        sr[u] = fma(a[u], br[u], sr[u]);
        si[u] = fma(a[u], bi[u], si[u]);
      }
      e[u] += G;
      more = more || e[u] < e1[u];
    }
  }
#pragma unroll
  for (int u = 0; u < kZ2Rows; ++u) {
#pragma unroll
    for (int off = G >> 1; off > 0; off >>= 1) {
      sr[u] += __shfl_xor(sr[u], off, 64);
      si[u] += __shfl_xor(si[u], off, 64);
    }
    const int64_t row = row0 + (int64_t)u * GPB;
    if (row < rows && g == 0) {
      yr[row] = sr[u];
      yi[row] = si[u];
    }
  }
}

template <int G>
static void launch_spmv_csr_z2_t(const CsrDev& A, const double* xr, const double* xi, double* yr, double* yi, hipStream_t s) {
  const int64_t per_block = (int64_t)(kTPB / G) * kZ2Rows;
  const int64_t grid = (A.rows + per_block - 1) / per_block;
  hipLaunchKernelGGL(k_spmv_csr_z2<G>, dim3((unsigned)grid), dim3(kTPB), 0, s, A.rowptr, A.colidx, A.vals, A.rows, xr, xi, yr, yi);
}

static void launch_spmv_csr_z2(const CsrDev& A, int group, const double* xr, const double* xi, double* yr, double* yi, hipStream_t s) {
  switch (group) {
    case 1: return launch_spmv_csr_z2_t<1>(A, xr, xi, yr, yi, s);
    case 2: return launch_spmv_csr_z2_t<2>(A, xr, xi, yr, yi, s);
    case 4: return launch_spmv_csr_z2_t<4>(A, xr, xi, yr, yi, s);
    case 8: return launch_spmv_csr_z2_t<8>(A, xr, xi, yr, yi, s);
    case 16: return launch_spmv_csr_z2_t<16>(A, xr, xi, yr, yi, s);
    case 32: return launch_spmv_csr_z2_t<32>(A, xr, xi, yr, yi, s);
    default: return launch_spmv_csr_z2_t<64>(A, xr, xi, yr, yi, s);
  }
}

// ------------------------------------------------------------------ dense: (yr, yi) = A (xr, xi), A real, one wave per row, A read once
// The shape of k_zgemv: a lane takes the 16-byte positions lane, lane + 64, ... of its row (two real entries each, rows lda apart: lda
// is even, so every row starts 16-byte aligned) with four non-temporal loads in flight, and both planes of x are multiplied out of the
// same registers; x comes through L1 / L2 as 16-byte loads too.  An odd column count leaves one last column to lane 0.
__global__ __launch_bounds__(kTPB) void k_gemv_z2(const double* __restrict__ A, int64_t n, int64_t lda, const double* __restrict__ xr,
                                                  const double* __restrict__ xi, double* __restrict__ yr, double* __restrict__ yi) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kTPB / 64) + (threadIdx.x >> 6);
  if (row >= n) return;  // (wave-uniform)
  const double* a = A + row * lda;
  const double2* a2 = reinterpret_cast<const double2*>(a);
  const double2* xr2 = reinterpret_cast<const double2*>(xr);
  const double2* xi2 = reinterpret_cast<const double2*>(xi);
  const int64_t n2 = n >> 1;
  double sr0 = 0.0, si0 = 0.0, sr1 = 0.0, si1 = 0.0;
  int64_t p = lane;
  for (; p + 192 < n2; p += 256) {
    double2 u[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) u[q] = ld_stream<1>(a2 + p + 64 * q);
#pragma unroll
    for (int q = 0; q < 4; q += 2) {
      const double2 br0 = xr2[p + 64 * q], bi0 = xi2[p + 64 * q], br1 = xr2[p + 64 * q + 64], bi1 = xi2[p + 64 * q + 64];
      sr0 = fma(u[q].x, br0.x, sr0);
      sr0 = fma(u[q].y, br0.y, sr0);
      si0 = fma(u[q].x, bi0.x, si0);
      si0 = fma(u[q].y, bi0.y, si0);
      sr1 = fma(u[q + 1].x, br1.x, sr1);
      sr1 = fma(u[q + 1].y, br1.y, sr1);
      si1 = fma(u[q + 1].x, bi1.x, si1);
      si1 = fma(u[q + 1].y, bi1.y, si1);
    }
  }
  for (; p < n2; p += 64) {
    const double2 u = ld_stream<1>(a2 + p);
    const double2 br = xr2[p], bi = xi2[p];
    sr0 = fma(u.x, br.x, sr0);
    sr0 = fma(u.y, br.y, sr0);
    si0 = fma(u.x, bi.x, si0);
    si0 = fma(u.y, bi.y, si0);
  }
  if ((n & 1) && lane == 0) {  // odd column count: the last column
    sr1 = fma(a[n - 1], xr[n - 1], sr1);
    si1 = fma(a[n - 1], xi[n - 1], si1);
  }
  const double sr = wave_sum(sr0 + sr1), si = wave_sum(si0 + si1);
  if (lane == 0) {
    yr[row] = sr;
    yi[row] = si;
  }
}

static void launch_gemv_z2(const double* A, int64_t n, int64_t lda, const double* xr, const double* xi, double* yr, double* yi, hipStream_t s) {
  const int64_t grid = (n + kTPB / 64 - 1) / (kTPB / 64);
  hipLaunchKernelGGL(k_gemv_z2, dim3((unsigned)grid), dim3(kTPB), 0, s, A, n, lda, xr, xi, yr, yi);
}

namespace api {

void expm_free(lz_handle h) {
  ExpmState& e = h->ex;
  orth_free(e.B);
  orth_free(e.wk);
  big_free(e.xtmp);
  e = ExpmState();
}

}  // namespace api
}  // namespace lz

namespace {

constexpr int kExpmMaxM = kZMaxRows - 1;  // 64 on every route: the real form of a planar C has 2 mm rows, and launch_trl_restart takes up to 128

// ex.wk.sm: the basis layer's head (c of both passes, nrm2), the projected rows (m x m elements), beta (m), the real form of C
// (planes mm x planes ncols)
struct ExpmSmall : OrthSmallHead {
  int64_t proj, beta, S, total;
};
ExpmSmall expm_small_layout(int m, int planes) {
  ExpmSmall L;
  static_cast<OrthSmallHead&>(L) = orth_small_head(m + 1, planes);
  L.proj = L.end;
  L.beta = L.proj + (int64_t)planes * m * m;
  L.S = L.beta + m + 8;
  L.total = L.S + (int64_t)planes * planes * m * m + 8;
  return L;
}

// the lanes per row of k_spmv_csr_z2, as lz_set_csr_cplx chooses them: the widest power of two that the mean row still fills
int expm_group(const CsrDev& A) {
  int group = 1;
  while (group < 64 && (int64_t)group * 2 * A.rows <= A.nnz) group *= 2;
  return group;
}

// Which form the product of the real matrix with a planar complex vector takes: 2 = the two-plane kernel (the matrix is read once),
// 1 = two launches of the real product, one per plane (the matrix is read twice).  lz_expm_set_product: 0 auto, 1 two launches
// always, 2 the two-plane kernel always.  Auto, as measured (tools/expm_probe.py, profiles/r26/expm_probe.json): the two-plane kernel for every
// dense matrix (421 against 667 us at n = 16384) and for a CSR matrix with a mean row below 16 entries (groups of up to 8 lanes:
// 1.5, 1.4 and 1.2 times faster than two launches of the CSR-stream kernel at 3, 5 and 9 entries per row) unless its SpMV is
//  - the ELL / row-class coded stencil kernel: its matrix stream is a byte per row, the second read costs next to nothing and two
//    launches take 87 us where the two-plane kernel on the plain arrays takes 270 (5-point Laplacian, 1e7 rows), or
//  - the column-blocked two-phase one, whose gathers come out of LDS (by accounting only: not measured).
// From a mean row of 16 entries on k_spmv_csr_z2 loses to two launches of the CSR-stream kernel (0.94, 0.86, 0.82 of their speed at 17,
// 33 and 65 entries per row): it runs at 2e11 entries/s whatever the row length, a third of the HBM rate there, while the stream
// kernel's LDS-staged products reach 0.7 of it.  Every CSR matrix keeps its plain fp64 rowptr / colidx / vals on the device beside
// whatever second layout it has (the coded copy and the blocked layout's fp32 or constant value streams are copies), so form 2 can
// always be honoured.
constexpr int kZ2MaxAutoGroup = 8;
int expm_mixed_form(lz_handle h) {
  if (h->ex.form == 1) return 1;
  if (h->ex.form == 2 || h->kind == 2) return 2;
  const CsrDev& A = h->csr;
  const bool coded = A.ell_default && ell_usable(A, h->flags);
  const bool blocked = A.pb && !(h->flags & LZ_FLAG_SPMV_STREAM);
  return coded || blocked || expm_group(A) > kZ2MaxAutoGroup ? 1 : 2;
}

// partials that the real product kernels write (trl_alloc's terms)
size_t expm_product_part(lz_handle h) {
  if (h->kind == 0) return 0;
  size_t need = std::max<size_t>((size_t)h->rows / 4 + 64, (size_t)h->csr.n_rowblk + 64);
  if (h->kind == 1 && h->csr.pb) need = std::max<size_t>(need, (size_t)pb_num_partials(h->csr.pb) + 64);
  return need;
}

// y = A x on the real matrix, one plane (trl_matvec's launches)
void expm_real_product(lz_handle h, const double* x, double* y, double* part) {
  if (h->kind == 1)
    launch_spmv_csr(h->csr, x, y, x, part, h->flags, h->stream);
  else
    launch_gemv_dense(h->d_dense, h->rows, h->ncols_ext, h->dense_lda, x, x, y, part, h->stream);
}

// y = A x on whatever matrix is set; planes of x and y are ld apart
void expm_matvec(lz_handle h, int planes, const double* x, double* y, int64_t ld, double* part) {
  ExpmState& e = h->ex;
  if (h->z.kind != 0) return z_matvec(h, x, y, ld);
  if (planes == 1) return expm_real_product(h, x, y, part);
  e.product = expm_mixed_form(h);
  if (e.product == 1) {
    expm_real_product(h, x, y, part);
    expm_real_product(h, x + ld, y + ld, part);
  } else if (h->kind == 1) {
    launch_spmv_csr_z2(h->csr, expm_group(h->csr), x, x + ld, y, y + ld, h->stream);
  } else {
    launch_gemv_z2(h->d_dense, h->rows, h->dense_lda, x, x + ld, y, y + ld, h->stream);
  }
}

int expm_state(lz_handle h, const char* who) {
  if (!h) return LZ_ERR_ARG;
  ExpmState& e = h->ex;
  if (!e.B.B) return fail(h, LZ_ERR_STATE, std::string(who) + ": no basis (lz_expm_begin first)");
  if ((h->kind == 0 && h->z.kind == 0) || skew_stride(h, h->rows_pad) != e.B.ld || (h->z.kind != 0 && e.B.planes != 2))
    return fail(h, LZ_ERR_STATE, std::string(who) + ": the matrix changed since lz_expm_begin");
  e.B.len = h->rows;  // the view follows the matrix set last, as trl_state's does
  e.B.pad = h->rows_pad;
  LZ_HIP(h, hipSetDevice(h->dev));
  return LZ_OK;
}

int expm_alloc(lz_handle h, int m, int planes) {
  ExpmState& e = h->ex;
  if (h->kind == 0 && h->z.kind == 0) return fail(h, LZ_ERR_STATE, "lz_expm_begin: no matrix set");
  if (h->world > 1 || h->comm_kind != 0)
    return fail(h, LZ_ERR_STATE, "lz_expm_begin: the propagator runs on one rank (this handle has a communicator)");
  if (h->flags & (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE))
    return fail(h, LZ_ERR_STATE, "lz_expm_begin: not with LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE");
  if (m < 2 || m > kExpmMaxM || m > h->rows) return fail(h, LZ_ERR_ARG, "lz_expm_begin: need 2 <= m <= min(64, n)");
  if (h->z.kind != 0 && planes != 2) return fail(h, LZ_ERR_ARG, "lz_expm_begin: a complex matrix needs the planar basis (cplx = 1)");
  LZ_HIP(h, hipSetDevice(h->dev));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  const int64_t ld = skew_stride(h, h->rows_pad);
  const size_t nrows = (size_t)planes * (size_t)(m + 1);  // real rows
  const ExpmSmall L = expm_small_layout(m, planes);
  if (!e.B.B || e.m != m || e.B.ld != ld || e.B.planes != planes) {
    LZ_TRY(dev_alloc(h, e.B.B, nrows * (size_t)ld));
    LZ_TRY(dev_alloc(h, e.B.w, (size_t)planes * (size_t)ld));
    LZ_TRY(dev_alloc(h, e.wk.sm, (size_t)L.total));
    LZ_TRY(dev_alloc(h, e.wk.gate, 4));
    e.m = m;
    e.B.ld = ld;
    e.B.nrows = m + 1;
    e.B.planes = planes;
  }
  e.B.len = h->rows;
  e.B.pad = h->rows_pad;
  LZ_TRY(orth_part_reserve(h, e.wk, std::max(orth_part_need(e.B, orth_plan(h, e.B), m), expm_product_part(h))));
  LZ_HIP(h, hipMemsetAsync(e.B.B, 0, nrows * (size_t)ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(e.B.w, 0, (size_t)planes * (size_t)ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(e.wk.sm, 0, (size_t)L.total * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(e.wk.gate, 0, 4 * sizeof(int), h->stream));
  return LZ_OK;
}

}  // namespace

extern "C" {

int lz_expm_begin(lz_handle h, int m, int cplx, const double* v0) {
  if (!h || !v0) return LZ_ERR_ARG;
  LZ_TRY(expm_alloc(h, m, cplx ? 2 : 1));
  ExpmState& e = h->ex;
  LZ_TRY(orth_upload_x(h, e.B, v0));
  return orth_store(h, e.B, e.wk, orth_plan(h, e.B), 0, "expm begin");
}

int lz_expm_extend(lz_handle h, int k0, int k1, double* proj_out, double* beta_out) {
  LZ_TRY(expm_state(h, "lz_expm_extend"));
  ExpmState& e = h->ex;
  const int m = e.m;
  if (k0 < 0 || k0 >= k1 || k1 > m) return fail(h, LZ_ERR_ARG, "lz_expm_extend: need 0 <= k0 < k1 <= the m of lz_expm_begin");
  const OrthBasis& V = e.B;
  const int pl = V.planes;
  const ExpmSmall L = expm_small_layout(m, pl);
  double* sm = e.wk.sm;
  const QtwPlan plan = orth_plan(h, V);
  const OrthPass2 pass2 = (h->flags & LZ_FLAG_TRL_PASS2_ALWAYS) ? OrthPass2::kForced : OrthPass2::kGated;
  for (int j = k0; j < k1; ++j) {
    expm_matvec(h, pl, V.B + (int64_t)(pl * j) * V.ld, V.w, V.ld, e.wk.part);  // w = A V[j]
    // w against V[0..j]: row j of the projection; beta_j = |w|, V[j + 1] = w / beta_j
    LZ_TRY(orth_cgs_step(h, V, e.wk, plan, j + 1, sm + L.proj + (int64_t)pl * j * m, sm + L.beta + j, pass2));
    LZ_TRY(check_launch(h, "expm extend"));
  }
  if (proj_out) LZ_HIP(h, hipMemcpyAsync(proj_out, sm + L.proj, (size_t)pl * m * m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (beta_out) LZ_HIP(h, hipMemcpyAsync(beta_out, sm + L.beta, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_expm_combine(lz_handle h, int mm, int ncols, const double* C, double* norm_out) {
  LZ_TRY(expm_state(h, "lz_expm_combine"));
  ExpmState& e = h->ex;
  if (!C || mm < 1 || mm > e.m || ncols < 1 || (mm == 1 ? ncols != 1 : ncols >= mm))
    return fail(h, LZ_ERR_ARG, "lz_expm_combine: need 1 <= mm <= m, 1 <= ncols < mm (mm == 1: ncols == 1) and C");
  const OrthBasis& V = e.B;
  const int pl = V.planes;
  const ExpmSmall L = expm_small_layout(e.m, pl);
  // mm == 1 scales row 0: the combination of rows 0 and 1 with a zero coefficient on row 1, which is cleared first (it may hold the NaN
  // of the breakdown that left one row; the next extension writes it again)
  const int mr = mm == 1 ? 2 : mm;
  if (mm == 1) LZ_HIP(h, hipMemsetAsync(V.B + (int64_t)pl * V.ld, 0, (size_t)pl * (size_t)V.ld * sizeof(double), h->stream));
  // Y_c = sum_i C[i, c] V_i.  Planar rows: the real form [[Cr, Ci], [-Ci, Cr]] in rows 2 i, 2 i + 1 and columns 2 c, 2 c + 1
  // (Re Y = Cr Vr - Ci Vi, Im Y = Ci Vr + Cr Vi), as lz_ztrl_restart builds it
  std::vector<double> R((size_t)pl * pl * mr * ncols, 0.0);
  const size_t ldr = (size_t)pl * ncols;
  for (int i = 0; i < mm; ++i)
    for (int c = 0; c < ncols; ++c) {
      if (pl == 1) {
        R[(size_t)i * ldr + c] = C[(size_t)i * ncols + c];
        continue;
      }
      const double cr = C[2 * ((size_t)i * ncols + c)], ci = C[2 * ((size_t)i * ncols + c) + 1];
      R[(size_t)(2 * i) * ldr + 2 * c] = cr;
      R[(size_t)(2 * i) * ldr + 2 * c + 1] = ci;
      R[(size_t)(2 * i + 1) * ldr + 2 * c] = -ci;
      R[(size_t)(2 * i + 1) * ldr + 2 * c + 1] = cr;
    }
  LZ_TRY(upload(h, e.wk.sm + L.S, R.data(), R.size() * sizeof(double)));
  // (the kernel also copies real row pl mr to real row pl ncols, which is no output: rows behind the outputs hold nothing until the
  // next extension writes them)
  LZ_HIP(h, launch_trl_restart(V.B, V.ld, h->rows, pl * mr, pl * ncols, e.wk.sm + L.S, h->stream));
  LZ_TRY(check_launch(h, "expm combine"));
  // row 0 = row 0 / |row 0|: through the work vector, whose padding is cleared first (a breakdown leaves NaN there, lz_orth.hip)
  LZ_HIP(h, hipMemsetAsync(V.w, 0, (size_t)pl * (size_t)V.ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemcpy2DAsync(V.w, (size_t)V.ld * sizeof(double), V.B, (size_t)V.ld * sizeof(double), (size_t)V.len * sizeof(double), (size_t)pl,
                             hipMemcpyDeviceToDevice, h->stream));
  LZ_TRY(orth_store(h, V, e.wk, orth_plan(h, V), 0, "expm normalise"));
  if (norm_out) {
    LZ_HIP(h, hipMemcpyAsync(norm_out, e.wk.sm + L.nrm2 + 1, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    LZ_HIP(h, hipStreamSynchronize(h->stream));
  }
  return LZ_OK;
}

int lz_expm_get_rows(lz_handle h, int j0, int count, double* rows, int64_t ld) {
  LZ_TRY(expm_state(h, "lz_expm_get_rows"));
  return orth_get_rows(h, h->ex.B, "lz_expm_get_rows", "m", j0, count, rows, ld);
}

int lz_zspmv_real_host(lz_handle h, const double* x, double* y) {
  if (!h || !x || !y) return LZ_ERR_ARG;
  if (h->kind == 0) return fail(h, LZ_ERR_STATE, "lz_zspmv_real_host: no real matrix set");
  if (h->world > 1 || h->comm_kind != 0) return fail(h, LZ_ERR_STATE, "lz_zspmv_real_host: one rank only (this handle has a communicator)");
  LZ_HIP(h, hipSetDevice(h->dev));
  ExpmState& e = h->ex;
  const int64_t n = h->rows, pad = h->rows_pad;
  if (e.xtmp_pad != pad) {
    LZ_TRY(dev_alloc(h, e.xtmp, 4 * (size_t)pad));
    e.xtmp_pad = pad;
  }
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  LZ_TRY(orth_part_reserve(h, e.wk, expm_product_part(h)));
  std::vector<double> buf(2 * (size_t)pad, 0.0);  // planar x, then planar y
  to_planar(x, n, buf.data(), buf.data() + pad);
  LZ_TRY(upload(h, e.xtmp, buf.data(), 2 * (size_t)pad * sizeof(double)));
  expm_matvec(h, 2, e.xtmp, e.xtmp + 2 * pad, pad, e.wk.part);
  LZ_TRY(check_launch(h, "zspmv real"));
  LZ_HIP(h, hipStreamSynchronize(h->stream));  // (buf is the source of the upload above)
  LZ_HIP(h, hipMemcpy2DAsync(buf.data(), (size_t)pad * sizeof(double), e.xtmp + 2 * pad, (size_t)pad * sizeof(double), (size_t)n * sizeof(double), 2,
                             hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  to_interleaved(buf.data(), buf.data() + pad, n, y);
  return LZ_OK;
}

int lz_expm_product_time(lz_handle h, int reps, double* ms_out) {
  LZ_TRY(expm_state(h, "lz_expm_product_time"));
  if (!ms_out || reps < 1) return fail(h, LZ_ERR_ARG, "lz_expm_product_time: need reps >= 1 and ms_out");
  ExpmState& e = h->ex;
  const OrthBasis& V = e.B;
  hipEvent_t a, b;
  LZ_HIP(h, hipEventCreate(&a));
  LZ_HIP(h, hipEventCreate(&b));
  expm_matvec(h, V.planes, V.B, V.w, V.ld, e.wk.part);  // warm-up
  hipError_t err = hipEventRecord(a, h->stream);
  for (int r = 0; r < reps; ++r) expm_matvec(h, V.planes, V.B, V.w, V.ld, e.wk.part);
  if (err == hipSuccess) err = hipEventRecord(b, h->stream);
  if (err == hipSuccess) err = hipEventSynchronize(b);
  float ms = 0.f;
  if (err == hipSuccess) err = hipEventElapsedTime(&ms, a, b);
  hipEventDestroy(a);
  hipEventDestroy(b);
  LZ_HIP(h, err);
  LZ_TRY(check_launch(h, "expm product time"));
  *ms_out = (double)ms / reps;
  return LZ_OK;
}

int lz_expm_set_product(lz_handle h, int form) {
  if (!h) return LZ_ERR_ARG;
  if (form < 0 || form > 2) return fail(h, LZ_ERR_ARG, "lz_expm_set_product: 0 auto, 1 two launches, 2 the two-plane kernel");
  h->ex.form = form;
  return LZ_OK;
}

int lz_expm_info(lz_handle h, int* out) {
  if (!h || !out) return LZ_ERR_ARG;
  const ExpmState& e = h->ex;
  out[0] = e.B.B ? (h->z.kind != 0 ? 2 : e.B.planes == 2 ? 1 : 0) : -1;
  out[1] = e.product;
  out[2] = h->kind == 1 ? expm_group(h->csr) : 0;
  return LZ_OK;
}

}  // extern "C"
