// Complex Hermitian operator of lanczos_amd.eigsh (include/lanczos_hip.h, "complex Hermitian matrices"): the CSR and the dense product
// kernels, lz_set_csr_cplx / lz_set_dense_cplx and lz_zspmv_host.  The matrix keeps NumPy's interleaved complex128, so one 16-byte load
// brings an entry; vectors are planar (ZState, lz_context.h), so the real basis kernels' row layout, restart and transfers serve.
// While a complex matrix is set h->kind is 0: the real entry points answer "no matrix set".
#include "lz_context.h"
#include "lz_device.h"

using namespace lz;
using namespace lz::api;

namespace lz {

// ------------------------------------------------------------------ CSR: y = A x, a group of G lanes per row
// Lane g of a group takes entries g, g + G, ... of its row (one 16-byte value load, one column index and two gathers each), the group
// adds its lanes' sums by a butterfly and lane 0 stores both parts.  Real and imaginary part of the row's inner product come from the
// same read of the row.  An empty row stores 0.
template <int G>
__global__ __launch_bounds__(kTPB) void k_zspmv_csr(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                    const double2* __restrict__ vals, int64_t rows, const double* __restrict__ xr,
                                                    const double* __restrict__ xi, double* __restrict__ yr, double* __restrict__ yi) {
  const int64_t row = ((int64_t)blockIdx.x * kTPB + threadIdx.x) / G;
  const int g = threadIdx.x & (G - 1);
  double sr = 0.0, si = 0.0;
  if (row < rows) {
    const int e1 = rowptr[row + 1];
    for (int e = rowptr[row] + g; e < e1; e += G) {
      const double2 a = ld_stream<1>(vals + e);
      const int32_t c = colidx[e];
      const double br = xr[c], bi = xi[c];
      sr = fma(a.x, br, sr);
      sr = fma(-a.y, bi, sr);
      si = fma(a.x, bi, si);
      si = fma(a.y, br, si);
    }
  }
#pragma unroll
  for (int off = G >> 1; off > 0; off >>= 1) {
    sr += __shfl_xor(sr, off, 64);
    si += __shfl_xor(si, off, 64);
  }
  if (row < rows && g == 0) {
    yr[row] = sr;
    yi[row] = si;
  }
}

template <int G>
static void launch_zspmv_csr_t(const int32_t* rowptr, const int32_t* colidx, const double* vals, int64_t rows, const double* xr,
                               const double* xi, double* yr, double* yi, hipStream_t s) {
  const int64_t grid = (rows * G + kTPB - 1) / kTPB;
  hipLaunchKernelGGL(k_zspmv_csr<G>, dim3((unsigned)grid), dim3(kTPB), 0, s, rowptr, colidx, reinterpret_cast<const double2*>(vals), rows,
                     xr, xi, yr, yi);
}

void launch_zspmv_csr(const int32_t* rowptr, const int32_t* colidx, const double* vals, int64_t rows, int group, const double* xr,
                      const double* xi, double* yr, double* yi, hipStream_t s) {
  switch (group) {
    case 1: return launch_zspmv_csr_t<1>(rowptr, colidx, vals, rows, xr, xi, yr, yi, s);
    case 2: return launch_zspmv_csr_t<2>(rowptr, colidx, vals, rows, xr, xi, yr, yi, s);
    case 4: return launch_zspmv_csr_t<4>(rowptr, colidx, vals, rows, xr, xi, yr, yi, s);
    case 8: return launch_zspmv_csr_t<8>(rowptr, colidx, vals, rows, xr, xi, yr, yi, s);
    case 16: return launch_zspmv_csr_t<16>(rowptr, colidx, vals, rows, xr, xi, yr, yi, s);
    case 32: return launch_zspmv_csr_t<32>(rowptr, colidx, vals, rows, xr, xi, yr, yi, s);
    default: return launch_zspmv_csr_t<64>(rowptr, colidx, vals, rows, xr, xi, yr, yi, s);
  }
}

// ------------------------------------------------------------------ dense: y = A x, one wave per row, A read once
// A lane takes columns lane, lane + 64, ... of its row with four 16-byte non-temporal loads in flight; x comes through L1 / L2.
__global__ __launch_bounds__(kTPB) void k_zgemv(const double2* __restrict__ A, int64_t n, const double* __restrict__ xr,
                                                const double* __restrict__ xi, double* __restrict__ yr, double* __restrict__ yi) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kTPB / 64) + (threadIdx.x >> 6);
  if (row >= n) return;  // (wave-uniform)
  const double2* a = A + row * n;
  double sr0 = 0.0, si0 = 0.0, sr1 = 0.0, si1 = 0.0;
  int64_t c = lane;
  for (; c + 192 < n; c += 256) {
    double2 u[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) u[q] = ld_stream<1>(a + c + 64 * q);
#pragma unroll
    for (int q = 0; q < 4; q += 2) {
      const double br0 = xr[c + 64 * q], bi0 = xi[c + 64 * q], br1 = xr[c + 64 * q + 64], bi1 = xi[c + 64 * q + 64];
      sr0 = fma(u[q].x, br0, sr0);
      sr0 = fma(-u[q].y, bi0, sr0);
      si0 = fma(u[q].x, bi0, si0);
      si0 = fma(u[q].y, br0, si0);
      sr1 = fma(u[q + 1].x, br1, sr1);
      sr1 = fma(-u[q + 1].y, bi1, sr1);
      si1 = fma(u[q + 1].x, bi1, si1);
      si1 = fma(u[q + 1].y, br1, si1);
    }
  }
  for (; c < n; c += 64) {
    const double2 u = ld_stream<1>(a + c);
    const double br = xr[c], bi = xi[c];
    sr0 = fma(u.x, br, sr0);
    sr0 = fma(-u.y, bi, sr0);
    si0 = fma(u.x, bi, si0);
    si0 = fma(u.y, br, si0);
  }
  const double sr = wave_sum(sr0 + sr1), si = wave_sum(si0 + si1);
  if (lane == 0) {
    yr[row] = sr;
    yi[row] = si;
  }
}

void launch_zgemv(const double* A, int64_t n, const double* xr, const double* xi, double* yr, double* yi, hipStream_t s) {
  const int64_t grid = (n + kTPB / 64 - 1) / (kTPB / 64);
  hipLaunchKernelGGL(k_zgemv, dim3((unsigned)grid), dim3(kTPB), 0, s, reinterpret_cast<const double2*>(A), n, xr, xi, yr, yi);
}

namespace api {

int z_drop_matrix(lz_handle h) {
  ZState& z = h->z;
  z.kind = 0;
  h->mr.live = false;  // every matrix setter comes through here: a new matrix drops the MINRES state (lz_minres.hip)
  h->bc.live = false;  // ... and the BiCGSTAB state (lz_bicgstab.hip)
  h->gm.live = false;  // ... and the GMRES state (lz_gmres.hip)
  h->cg.live = false;  // ... and the CG state (lz_cg.hip)
  LZ_TRY(dev_free(h, z.rowptr));
  LZ_TRY(dev_free(h, z.colidx));
  LZ_TRY(dev_free(h, z.vals));
  return LZ_OK;
}

void z_free(lz_handle h) {
  ZState& z = h->z;
  big_free(z.rowptr);
  big_free(z.colidx);
  big_free(z.vals);
  big_free(z.xtmp);
  orth_free(z.B);
  orth_free(z.wk);
  z = ZState();
}

void z_matvec(lz_handle h, const double* x, double* y, int64_t ld) {
  const ZState& z = h->z;
  if (z.kind == 1)
    launch_zspmv_csr(z.rowptr, z.colidx, z.vals, z.n, z.group, x, x + ld, y, y + ld, h->stream);
  else
    launch_zgemv(z.vals, z.n, x, x + ld, y, y + ld, h->stream);
}

}  // namespace api
}  // namespace lz

namespace {

// what both complex setters do to the handle before they upload: the real matrix and what hangs on it are gone
int z_begin_set(lz_handle h, const char* who) {
  if (h->world > 1 || h->comm_kind != 0)
    return fail(h, LZ_ERR_STATE, std::string(who) + ": a complex matrix lives on one rank (this handle has a communicator)");
  LZ_HIP(h, hipSetDevice(h->dev));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  h->kind = 0;
  h->poly.clear();
  LZ_TRY(dev_free(h, h->d_dense));
  LZ_TRY(dev_free(h, h->d_V));
  h->n = 0;
  return z_drop_matrix(h);
}

// h->rows / h->rows_pad as for a real matrix of n rows
void z_finish_set(lz_handle h, int64_t n, int64_t nnz, int kind) {
  h->T_declared = false;
  h->has_T = false;
  h->bi_n = 0;
  h->Mg = n;
  h->row0 = 0;
  h->rows = n;
  h->ncols_ext = n;
  h->rows_pad = round_up(n, kPadDoubles);
  h->ldv = skew_stride(h, h->rows_pad);
  h->xmode = 0;
  h->z.n = n;
  h->z.nnz = nnz;
  h->z.kind = kind;
}

}  // namespace

extern "C" {

int lz_set_csr_cplx(lz_handle h, int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* colidx, const double* vals) {
  if (!h) return LZ_ERR_ARG;
  if (n <= 0 || nnz < 0 || !rowptr || (nnz > 0 && (!colidx || !vals))) return fail(h, LZ_ERR_ARG, "lz_set_csr_cplx: bad sizes or NULL arrays");
  if (n >= (int64_t)1 << 31 || nnz >= (int64_t)1 << 31) return fail(h, LZ_ERR_ARG, "lz_set_csr_cplx: sizes exceed int32 CSR indexing");
  if (rowptr[0] != 0 || rowptr[n] != nnz) return fail(h, LZ_ERR_ARG, "lz_set_csr_cplx: rowptr[0] != 0 or rowptr[n] != nnz");
  for (int64_t i = 0; i < n; ++i) {
    const int64_t a = rowptr[i], b = rowptr[i + 1];
    if (b < a || a < 0 || b > nnz) return fail(h, LZ_ERR_ARG, "lz_set_csr_cplx: rowptr not monotone");
    for (int64_t e = a; e < b; ++e)
      if (colidx[e] < 0 || colidx[e] >= n) return fail(h, LZ_ERR_ARG, "lz_set_csr_cplx: column index out of range");
  }
  LZ_TRY(z_begin_set(h, "lz_set_csr_cplx"));
  ZState& z = h->z;
  LZ_TRY(dev_alloc(h, z.rowptr, (size_t)n + 1));
  LZ_TRY(dev_alloc(h, z.colidx, (size_t)nnz));
  LZ_TRY(dev_alloc(h, z.vals, 2 * (size_t)nnz));
  LZ_TRY(upload(h, z.rowptr, rowptr, ((size_t)n + 1) * sizeof(int32_t)));
  if (nnz > 0) {
    LZ_TRY(upload(h, z.colidx, colidx, (size_t)nnz * sizeof(int32_t)));
    LZ_TRY(upload(h, z.vals, vals, 2 * (size_t)nnz * sizeof(double)));
  }
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  // the widest power of two that the mean row still fills: a row of the mean length takes one trip, a longer one strides
  z.group = 1;
  while (z.group < 64 && (int64_t)z.group * 2 * n <= nnz) z.group *= 2;
  z_finish_set(h, n, nnz, 1);
  return LZ_OK;
}

int lz_set_dense_cplx(lz_handle h, int64_t n, const double* A) {
  if (!h) return LZ_ERR_ARG;
  if (n <= 0 || !A) return fail(h, LZ_ERR_ARG, "lz_set_dense_cplx: bad size or NULL matrix");
  if (n >= (int64_t)1 << 31) return fail(h, LZ_ERR_ARG, "lz_set_dense_cplx: n exceeds int32 indexing");
  LZ_TRY(z_begin_set(h, "lz_set_dense_cplx"));
  ZState& z = h->z;
  LZ_TRY(dev_alloc(h, z.vals, 2 * (size_t)n * (size_t)n));
  LZ_TRY(upload(h, z.vals, A, 2 * (size_t)n * (size_t)n * sizeof(double)));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  z_finish_set(h, n, n * n, 2);
  return LZ_OK;
}

int lz_zspmv_host(lz_handle h, const double* x, double* y) {
  if (!h || !x || !y) return LZ_ERR_ARG;
  ZState& z = h->z;
  if (z.kind == 0) return fail(h, LZ_ERR_STATE, "lz_zspmv_host: no complex matrix set (lz_set_csr_cplx / lz_set_dense_cplx)");
  LZ_HIP(h, hipSetDevice(h->dev));
  const int64_t n = z.n, pad = h->rows_pad;
  if (z.xtmp_pad != pad) {
    LZ_TRY(dev_alloc(h, z.xtmp, 4 * (size_t)pad));
    z.xtmp_pad = pad;
  }
  std::vector<double> buf(2 * (size_t)pad, 0.0);  // planar x, then planar y
  to_planar(x, n, buf.data(), buf.data() + pad);
  LZ_TRY(upload(h, z.xtmp, buf.data(), 2 * (size_t)pad * sizeof(double)));
  z_matvec(h, z.xtmp, z.xtmp + 2 * pad, pad);
  LZ_TRY(check_launch(h, "zspmv"));
  LZ_HIP(h, hipStreamSynchronize(h->stream));  // (buf is the source of the upload above)
  LZ_HIP(h, hipMemcpy2DAsync(buf.data(), (size_t)pad * sizeof(double), z.xtmp + 2 * pad, (size_t)pad * sizeof(double), (size_t)n * sizeof(double), 2,
                             hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  to_interleaved(buf.data(), buf.data() + pad, n, y);
  return LZ_OK;
}

}  // extern "C"
