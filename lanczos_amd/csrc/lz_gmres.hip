// Restarted GMRES (include/lanczos_hip.h, "restarted GMRES"): the device half of lanczos_amd.gmres, A x = b for a real square A,
// scipy.sparse.linalg.gmres' rules.  An inner step is the matrix's own product w = A V[j] (trl_matvec's launches) followed by the basis
// layer's orth_cgs_step, unchanged: classical Gram-Schmidt with the DGKS-gated second pass, the Hessenberg column left on the device.
// What is new here is everything around that step, all of it on the device so that a chunk of inner steps, cycle ends and restarts
// included, is enqueued without the host seeing a scalar:
//   k_gmres_column    one block, once per inner step: row j of the projection, h1 from the norm slot, h0^2 from the self slot of pass
//                     1's dots; the breakdown test h1 <= eps h0, the stored rotations applied to the column, the new rotation (LAPACK
//                     lartg's conventions), S, presid, the history, the inner-exit flag on presid <= ptol or on breakdown
//   k_gmres_solve     one block: SciPy's pseudo-solve of the cols x cols triangle (a zero last pivot zeroes its S entry), leaves y
//   k_gmres_update    x += sum_{i < cols} y_i V[i], cols read from device memory: rows >= cols are never read (after a breakdown they
//                     may hold Inf or NaN); every row and x read once, (cols + 2) 8 bytes a row, 16-byte loads
//   k_gmres_residual  behind the product w = A x: w = b - w, the whole padding [rows, pad) of w written as zero (the basis layer
//                     relies on that: lz_orth.hip), the partials of |w|^2
//   k_gmres_cycle     one block: rnorm, the outer test, the ptol_max_factor / ptol rule, the reset of cols, S[0], the rotations and
//                     the inner-exit flag for the next cycle; the basis layer's launch_scale_store then makes V[0]
// Once the inner-exit flag is set k_gmres_column changes nothing: cols, S, the rotations and R are frozen, and the basis rows that the
// later steps of the chunk write (all of them >= cols) are scratch that nothing reads.  Behind the done flag (converged, or a
// breakdown whose cycle has ended) every kernel here returns at once.  No atomics: the same input gives the same bits.
#include "lz_context.h"
#include "lz_device.h"

using namespace lz;
using namespace lz::api;

namespace lz {

constexpr int kGmresMaxRestart = 128;  // the basis layer holds at most 128 + 1 rows
constexpr double kGmEps = 2.220446049250313e-16;

// the scalars on the device (doubles, behind the small arrays) and the flags and counters (ints)
enum GmresD { kGmPtol = 0, kGmFactor, kGmPresid, kGmRnorm, kGmBnorm, kGmresDoubles = 8 };
enum GmresI { kGmDone = 0, kGmInner, kGmBreakdown, kGmConverged, kGmCols, kGmIters, kGmCycles, kGmresInts = 8 };

// LAPACK 3.10's dlartg: c f + s g = r, -s f + c g = 0, with its signs and its scaling
__device__ __forceinline__ void gmres_lartg(double f, double g, double& c, double& s, double& r) {
  const double safmin = 0x1p-1022, safmax = 0x1p1022, rtmin = 0x1p-511;
  const double rtmax = sqrt(0x1p1021);
  const double f1 = fabs(f), g1 = fabs(g);
  if (g == 0.0) {
    c = 1.0, s = 0.0, r = f;
  } else if (f == 0.0) {
    c = 0.0, s = copysign(1.0, g), r = g1;
  } else if (f1 > rtmin && f1 < rtmax && g1 > rtmin && g1 < rtmax) {
    const double d = sqrt(f * f + g * g);
    c = f1 / d;
    r = copysign(d, f);
    s = g / r;
  } else {
    const double u = fmin(safmax, fmax(safmin, fmax(f1, g1)));
    const double fs = f / u, gs = g / u;
    const double d = sqrt(fs * fs + gs * gs);
    c = fabs(fs) / d;
    r = copysign(d, f);
    s = gs / r;
    r = r * u;
  }
}

// Column j of the Hessenberg matrix -> column j of R (R + j m, rows 0 .. j), rotation j, S[j], S[j + 1], presid.  proj: the j + 1
// coefficients of the Gram-Schmidt step, h1: |w| behind it, h0sq: w . w in front of it.
__global__ __launch_bounds__(kTPB) void k_gmres_column(int j, int m, const double* __restrict__ proj, const double* __restrict__ h1p,
                                                      const double* __restrict__ h0sq, double* __restrict__ R, double* __restrict__ gc,
                                                      double* __restrict__ gs, double* __restrict__ S, double* __restrict__ ds, int* __restrict__ di,
                                                      double* __restrict__ hist, int hist_cap) {
  __shared__ double col[kGmresMaxRestart + 2];
  if (di[kGmDone] || di[kGmInner]) return;
  for (int i = threadIdx.x; i <= j; i += kTPB) col[i] = proj[i];
  __syncthreads();  // (every thread has read the flags before thread 0 writes one)
  if (threadIdx.x == 0) {
    double h1 = h1p[0];
    const double h0 = sqrt(h0sq[0]);
    const bool brk = h1 <= kGmEps * h0;  // the exact-solution indicator
    if (brk) h1 = 0.0;
    for (int k = 0; k < j; ++k) {
      const double c = gc[k], s = gs[k], n0 = col[k], n1 = col[k + 1];
      col[k] = c * n0 + s * n1;
      col[k + 1] = -s * n0 + c * n1;
    }
    double c, s, mag;
    gmres_lartg(col[j], h1, c, s, mag);
    gc[j] = c;
    gs[j] = s;
    col[j] = mag;
    const double sj = S[j];
    const double tmp = -s * sj;
    S[j] = c * sj;
    S[j + 1] = tmp;
    const double presid = fabs(tmp);
    ds[kGmPresid] = presid;
    const int it = di[kGmIters];
    if (it < hist_cap) hist[it] = presid;
    di[kGmIters] = it + 1;
    di[kGmCols] = j + 1;
    if (brk) di[kGmBreakdown] = 1;
    if (presid <= ds[kGmPtol] || brk) di[kGmInner] = 1;
  }
  __syncthreads();
  for (int i = threadIdx.x; i <= j; i += kTPB) R[(size_t)j * m + i] = col[i];
}

// y = the pseudo-solve of R[0 .. cols) y = S[0 .. cols): SciPy's loop, statement for statement
__global__ __launch_bounds__(kTPB) void k_gmres_solve(int m, const double* __restrict__ R, double* __restrict__ S, double* __restrict__ y,
                                                     const int* __restrict__ di) {
  __shared__ double ys[kGmresMaxRestart];
  if (di[kGmDone]) return;
  const int cols = di[kGmCols];
  if (cols < 1 || cols > m) return;
  const int col = cols - 1;
  if (threadIdx.x == 0 && R[(size_t)col * m + col] == 0.0) S[col] = 0.0;
  __syncthreads();
  for (int i = threadIdx.x; i < cols; i += kTPB) ys[i] = S[i];
  __syncthreads();
  for (int k = col; k > 0; --k) {
    if (ys[k] != 0.0) {  // (uniform: read behind a barrier)
      __syncthreads();
      if (threadIdx.x == 0) ys[k] = ys[k] / R[(size_t)k * m + k];
      __syncthreads();
      const double t = ys[k];
      for (int i = threadIdx.x; i < k; i += kTPB) ys[i] = ys[i] - t * R[(size_t)k * m + i];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && ys[0] != 0.0) ys[0] = ys[0] / R[0];
  __syncthreads();
  for (int i = threadIdx.x; i < m; i += kTPB) y[i] = i < cols ? ys[i] : 0.0;
}

// x += sum_{i < cols} y_i V[i].  Grid-stride over 16-byte positions, two positions of a lane in flight one grid stride apart, the rows
// four at a time: eight 16-byte loads of the basis issued before the first use.  The sum is formed in row order, products and sums
// rounded separately (k_trl_cgs's arithmetic), and added to x once.  Positions past `rows` are written as zero.
__global__ __launch_bounds__(kTPB) void k_gmres_update(const double* __restrict__ V, int64_t ldv, int64_t n2, int64_t rows, double* __restrict__ x,
                                                      const double* __restrict__ y, const int* __restrict__ di) {
  __shared__ double ysm[kGmresMaxRestart];
  if (di[kGmDone]) return;
  const int cols = di[kGmCols];
  if (cols < 1 || cols > kGmresMaxRestart) return;
  for (int i = threadIdx.x; i < cols; i += kTPB) ysm[i] = y[i];
  __syncthreads();
  const double2* V2 = reinterpret_cast<const double2*>(V);
  double2* x2 = reinterpret_cast<double2*>(x);
  const int64_t ld2 = ldv >> 1;
  constexpr int U = 2, RU = 4;
  const int64_t stride = (int64_t)gridDim.x * kTPB;
  for (int64_t i0 = (int64_t)blockIdx.x * kTPB + threadIdx.x; i0 < n2; i0 += U * stride) {
    int64_t pos[U];
    bool in[U];
    double tx[U], ty[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      pos[u] = i0 + u * stride;
      in[u] = pos[u] < n2;
      if (!in[u]) pos[u] = i0;  // (a position that exists: loaded, never stored)
      tx[u] = ty[u] = 0.0;
    }
    for (int k = 0; k < cols; k += RU) {
      double2 q[RU][U];
#pragma unroll
      for (int r = 0; r < RU; ++r)
        if (k + r < cols)
#pragma unroll
          for (int u = 0; u < U; ++u) q[r][u] = ld_stream<1>(V2 + (int64_t)(k + r) * ld2 + pos[u]);
#pragma unroll
      for (int r = 0; r < RU; ++r)
        if (k + r < cols) {
          const double yk = ysm[k + r];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            tx[u] = tx[u] + yk * q[r][u].x;
            ty[u] = ty[u] + yk * q[r][u].y;
          }
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!in[u]) continue;
      double2 xv = x2[pos[u]];
      xv.x = 2 * pos[u] < rows ? xv.x + tx[u] : 0.0;
      xv.y = 2 * pos[u] + 1 < rows ? xv.y + ty[u] : 0.0;
      x2[pos[u]] = xv;  // plain store: the product reads it next
    }
  }
}

// w = b - w on [0, rows), zero on [rows, pad); part[blk] = block blk's share of |w|^2.  gate may be null (lz_gmres_begin).
__global__ __launch_bounds__(kTPB) void k_gmres_residual(const double* __restrict__ b, double* __restrict__ w, int64_t rows, int64_t n2,
                                                        double* __restrict__ part, const int* __restrict__ gate) {
  __shared__ double sm[kTPB / 64];
  if (gate && gate[0]) return;
  const double2* b2 = reinterpret_cast<const double2*>(b);
  double2* w2 = reinterpret_cast<double2*>(w);
  double acc = 0.0;
  constexpr int U = 2;
  const int64_t stride = (int64_t)gridDim.x * kTPB;
  for (int64_t i0 = (int64_t)blockIdx.x * kTPB + threadIdx.x; i0 < n2; i0 += U * stride) {
    double2 bv[U], wv[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      in[u] = i < n2;
      if (!in[u]) continue;
      bv[u] = b2[i];
      wv[u] = w2[i];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (!in[u]) continue;
      double2 r;
      r.x = 2 * i < rows ? bv[u].x - wv[u].x : 0.0;
      r.y = 2 * i + 1 < rows ? bv[u].y - wv[u].y : 0.0;
      w2[i] = r;  // plain store: launch_scale_store reads it
      acc = fma(r.x, r.x, acc);
      acc = fma(r.y, r.y, acc);
    }
  }
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// MODE 0: the end of a cycle.  rnorm = |b - A x| from the np partials, the cycle's record (rnorm, cols, the ptol it ran under), the outer
// test rnorm <= atol, the end behind a breakdown, else the ptol_max_factor / ptol rule and the reset for the next cycle.  MODE 1: the
// first test of a solve, |r| < atol, and the first ptol = |b| min(1, atol / |b|).  MODE 2: |b| only (lz_gmres_begin).
template <int MODE>
__global__ __launch_bounds__(kTPB) void k_gmres_cycle(const double* __restrict__ part, int np, double atol, int m, double* __restrict__ S,
                                                     double* __restrict__ gc, double* __restrict__ gs, double* __restrict__ nrm2, double* __restrict__ ds,
                                                     int* __restrict__ di, double* __restrict__ chist, int chist_cap) {
  __shared__ double sm16[16];
  if (MODE != 2 && di[kGmDone]) return;
  const double rr = final_sum_emulated(part, np, sm16);  // (every thread has read the flag: the barriers inside)
  if (threadIdx.x != 0) return;
  const double rnorm = sqrt(rr);
  if (MODE == 2) {
    ds[kGmBnorm] = rnorm;
    return;
  }
  ds[kGmRnorm] = rnorm;
  if (MODE == 1) {
    if (rnorm < atol) {
      di[kGmConverged] = 1;
      di[kGmDone] = 1;
      return;
    }
    const double bnorm = ds[kGmBnorm];
    ds[kGmFactor] = 1.0;
    ds[kGmPtol] = bnorm * fmin(1.0, atol / bnorm);
  } else {
    const int cyc = di[kGmCycles];
    if (cyc < chist_cap) {
      chist[3 * (size_t)cyc] = rnorm;
      chist[3 * (size_t)cyc + 1] = (double)di[kGmCols];
      chist[3 * (size_t)cyc + 2] = ds[kGmPtol];
    }
    di[kGmCycles] = cyc + 1;
    if (rnorm <= atol) {
      di[kGmConverged] = 1;
      di[kGmDone] = 1;
      return;
    }
    if (di[kGmBreakdown]) {  // the exact-solution indicator fired, but the outer test failed: SciPy bails out
      di[kGmDone] = 1;
      return;
    }
    const double presid = ds[kGmPresid];
    double f = ds[kGmFactor];
    f = presid <= ds[kGmPtol] ? fmax(kGmEps, 0.25 * f) : fmin(1.0, 1.5 * f);  // inner passed but outer did not: tighten
    ds[kGmFactor] = f;
    ds[kGmPtol] = presid * fmin(f, atol / rnorm);
  }
  nrm2[0] = rr;  // launch_scale_store: V[0] = w / sqrt(rr), S[0] = sqrt(rr)
  S[0] = rnorm;
  for (int i = 0; i < m; ++i) {
    gc[i] = 0.0;
    gs[i] = 0.0;
    S[i + 1] = 0.0;
  }
  di[kGmCols] = 0;
  di[kGmInner] = 0;
}

constexpr int kGmresMaxBlocks = 2048;  // k_minres_step's grid
static int gmres_blocks(int64_t pad) {
  const int64_t g = ((pad >> 1) + kTPB - 1) / kTPB;
  return (int)std::min<int64_t>(std::max<int64_t>(g, 1), kGmresMaxBlocks);
}

namespace api {

void gmres_free(lz_handle h) {
  GmresState& g = h->gm;
  orth_free(g.B);
  orth_free(g.wk);
  big_free(g.vec);
  big_free(g.di);
  big_free(g.rpart);
  big_free(g.hist);
  big_free(g.chist);
  g = GmresState();
}

}  // namespace api
}  // namespace lz

namespace {

// gm.wk.sm: the basis layer's head (c of both passes, nrm2), the step's coefficients, its norm, R (m x m, column j at R + j m), the
// rotations, S (m + 1), y (m) and the scalars
struct GmresSmall : OrthSmallHead {
  int64_t proj, h1, R, gc, gs, S, y, ds, total;
};
int gmres_nrows(int m) { return std::max(m, 2) + 1; }
GmresSmall gmres_small_layout(int m) {
  GmresSmall L;
  static_cast<OrthSmallHead&>(L) = orth_small_head(gmres_nrows(m));
  L.proj = L.end;
  L.h1 = L.proj + gmres_nrows(m) + 8;
  L.R = L.h1 + 8;
  L.gc = L.R + (int64_t)m * m;
  L.gs = L.gc + m;
  L.S = L.gs + m;
  L.y = L.S + m + 8;
  L.ds = L.y + m + 8;
  L.total = L.ds + kGmresDoubles;
  return L;
}
// partials that the products write (trl_alloc's terms)
size_t gmres_product_part(lz_handle h) {
  size_t need = std::max<size_t>((size_t)h->rows / 4 + 64, (size_t)h->csr.n_rowblk + 64);
  if (h->kind == 1 && h->csr.pb) need = std::max<size_t>(need, (size_t)pb_num_partials(h->csr.pb) + 64);
  return need;
}

// y = A x: the matrix's own product (trl_matvec's launches), never the polynomial h->poly
void gmres_product(lz_handle h, const double* x, double* y) {
  if (h->kind == 1)
    launch_spmv_csr(h->csr, x, y, x, h->gm.wk.part, h->flags, h->stream);
  else
    launch_gemv_dense(h->d_dense, h->rows, h->ncols_ext, h->dense_lda, x, x, y, h->gm.wk.part, h->stream);
}

int gmres_alloc(lz_handle h, int m, const char* who) {
  GmresState& g = h->gm;
  const std::string w(who);
  if (h->kind == 0) return fail(h, LZ_ERR_STATE, w + (h->z.kind != 0 ? ": a complex matrix is set (GMRES takes a real one)" : ": no matrix set"));
  if (h->world > 1 || h->comm_kind != 0) return fail(h, LZ_ERR_STATE, w + ": GMRES runs on one rank (this handle has a communicator)");
  if (h->flags & (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE)) return fail(h, LZ_ERR_STATE, w + ": not with LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE");
  if (h->rows < 1 || h->ncols_ext != h->rows) return fail(h, LZ_ERR_STATE, w + ": the matrix is not square on this rank");
  if (m < 1 || m > kGmresMaxRestart || m > h->rows) return fail(h, LZ_ERR_ARG, w + ": need 1 <= restart <= min(128, n)");
  LZ_HIP(h, hipSetDevice(h->dev));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  g.live = false;
  const int64_t ld = skew_stride(h, h->rows_pad);
  const size_t nrows = (size_t)gmres_nrows(m);
  const GmresSmall L = gmres_small_layout(m);
  if (!g.B.B || g.m != m || g.B.ld != ld) {
    LZ_TRY(dev_alloc(h, g.B.B, nrows * (size_t)ld));
    LZ_TRY(dev_alloc(h, g.B.w, (size_t)ld));
    LZ_TRY(dev_alloc(h, g.vec, 2 * (size_t)ld));
    LZ_TRY(dev_alloc(h, g.wk.sm, (size_t)L.total));
    LZ_TRY(dev_alloc(h, g.wk.gate, 4));
    g.m = m;
    g.B.ld = ld;
    g.B.nrows = (int)nrows;
    g.B.planes = 1;
  }
  if (!g.di) LZ_TRY(dev_alloc(h, g.di, (size_t)kGmresInts));
  if (!g.rpart) LZ_TRY(dev_alloc(h, g.rpart, (size_t)kGmresMaxBlocks));
  g.B.len = h->rows;
  g.B.pad = h->rows_pad;
  LZ_TRY(orth_part_reserve(h, g.wk, std::max(orth_part_need(g.B, orth_plan(h, g.B), m), gmres_product_part(h))));
  LZ_HIP(h, hipMemsetAsync(g.B.B, 0, nrows * (size_t)ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(g.B.w, 0, (size_t)ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(g.vec, 0, 2 * (size_t)ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(g.wk.sm, 0, (size_t)L.total * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(g.wk.gate, 0, 4 * sizeof(int), h->stream));
  LZ_HIP(h, hipMemsetAsync(g.di, 0, kGmresInts * sizeof(int), h->stream));
  if (g.hist) LZ_HIP(h, hipMemsetAsync(g.hist, 0, (size_t)g.hist_cap * sizeof(double), h->stream));
  if (g.chist) LZ_HIP(h, hipMemsetAsync(g.chist, 0, 3 * (size_t)g.chist_cap * sizeof(double), h->stream));
  g.iters = g.cycles = g.done = g.hcol = 0;
  g.fresh = g.pending = false;
  return LZ_OK;
}

// a history of `width` doubles per entry holds at least `count` entries; what it holds is kept
int gmres_reserve(lz_handle h, double*& buf, int& cap, int width, int count) {
  if (count <= cap) return LZ_OK;
  const int ncap = std::max(count, std::max(1024, 2 * cap));
  double* p = nullptr;
  LZ_TRY(dev_alloc(h, p, (size_t)width * (size_t)ncap));
  LZ_HIP(h, hipMemsetAsync(p, 0, (size_t)width * (size_t)ncap * sizeof(double), h->stream));
  if (buf && cap > 0) LZ_HIP(h, hipMemcpyAsync(p, buf, (size_t)width * (size_t)cap * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  LZ_TRY(dev_free(h, buf));
  buf = p;
  cap = ncap;
  return LZ_OK;
}

int gmres_state(lz_handle h, const char* who) {
  if (!h) return LZ_ERR_ARG;
  GmresState& g = h->gm;
  if (!g.live || !g.B.B) return fail(h, LZ_ERR_STATE, std::string(who) + ": no state (lz_gmres_begin first; a new matrix drops it)");
  if (h->kind == 0 || skew_stride(h, h->rows_pad) != g.B.ld || h->rows != g.B.len)
    return fail(h, LZ_ERR_STATE, std::string(who) + ": the matrix changed since lz_gmres_begin");
  if (h->world > 1 || h->comm_kind != 0 || (h->flags & (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE)))
    return fail(h, LZ_ERR_STATE, std::string(who) + ": GMRES runs on one rank, without LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE");
  LZ_HIP(h, hipSetDevice(h->dev));
  return LZ_OK;
}

double* gmres_x(const GmresState& g) { return g.vec; }
double* gmres_b(const GmresState& g) { return g.vec + g.B.ld; }

// w = b - w with the partials of |w|^2 in rpart
void gmres_launch_residual(lz_handle h, const int* gate) {
  const GmresState& g = h->gm;
  hipLaunchKernelGGL(k_gmres_residual, dim3(gmres_blocks(g.B.pad)), dim3(kTPB), 0, h->stream, gmres_b(g), g.B.w, g.B.len, g.B.pad >> 1, g.rpart, gate);
}

template <int MODE>
void gmres_launch_cycle(lz_handle h, double atol) {
  const GmresState& g = h->gm;
  const GmresSmall L = gmres_small_layout(g.m);
  double* sm = g.wk.sm;
  hipLaunchKernelGGL(k_gmres_cycle<MODE>, dim3(1), dim3(kTPB), 0, h->stream, g.rpart, gmres_blocks(g.B.pad), atol, g.m, sm + L.S, sm + L.gc, sm + L.gs,
                     sm + L.nrm2, sm + L.ds, g.di, g.chist, g.chist_cap);
}

// V[0] = w / |w|, S[0] = |w|; skipped behind the done flag
void gmres_launch_v0(lz_handle h) {
  const GmresState& g = h->gm;
  const GmresSmall L = gmres_small_layout(g.m);
  launch_scale_store(g.B.B, g.B.w, g.wk.sm + L.nrm2, g.wk.sm + L.S, g.B.pad, h->stream, g.di + kGmDone);
}

// the end of a cycle: solve, update, the product w = A x, the residual, the tests and the next cycle's V[0]
int gmres_end_cycle(lz_handle h, double atol) {
  GmresState& g = h->gm;
  const GmresSmall L = gmres_small_layout(g.m);
  double* sm = g.wk.sm;
  hipLaunchKernelGGL(k_gmres_solve, dim3(1), dim3(kTPB), 0, h->stream, g.m, sm + L.R, sm + L.S, sm + L.y, g.di);
  hipLaunchKernelGGL(k_gmres_update, dim3(gmres_blocks(g.B.pad)), dim3(kTPB), 0, h->stream, g.B.B, g.B.ld, g.B.pad >> 1, g.B.len, gmres_x(g), sm + L.y, g.di);
  LZ_TRY(check_launch(h, "gmres: solve and update"));
  gmres_product(h, gmres_x(g), g.B.w);
  LZ_TRY(check_launch(h, "gmres: product A x"));
  gmres_launch_residual(h, g.di + kGmDone);
  gmres_launch_cycle<0>(h, atol);
  gmres_launch_v0(h);
  LZ_TRY(check_launch(h, "gmres: cycle end"));
  g.hcol = 0;
  g.pending = false;
  return LZ_OK;
}

int gmres_read_state(lz_handle h, double* state_out) {
  GmresState& g = h->gm;
  const GmresSmall L = gmres_small_layout(g.m);
  double ds[kGmresDoubles];
  int di[kGmresInts];
  LZ_HIP(h, hipMemcpyAsync(ds, g.wk.sm + L.ds, sizeof(ds), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipMemcpyAsync(di, g.di, sizeof(di), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  g.iters = di[kGmIters];
  g.cycles = di[kGmCycles];
  g.done = di[kGmDone];
  g.pending = !g.done && di[kGmInner] != 0;
  if (state_out) {
    state_out[0] = (double)g.iters;
    state_out[1] = (double)g.done;
    state_out[2] = (double)di[kGmConverged];
    state_out[3] = (double)di[kGmBreakdown];
    state_out[4] = (double)di[kGmInner];
    state_out[5] = (double)di[kGmCols];
    state_out[6] = (double)g.cycles;
    state_out[7] = ds[kGmPresid];
    state_out[8] = ds[kGmPtol];
    state_out[9] = ds[kGmFactor];
    state_out[10] = ds[kGmRnorm];
    state_out[11] = ds[kGmBnorm];
    state_out[12] = (double)g.hcol;
    state_out[13] = state_out[14] = state_out[15] = 0.0;
  }
  return LZ_OK;
}

// the tests of a fresh state, then the end of a cycle whose inner exit the last synchronisation showed
int gmres_head(lz_handle h, double atol) {
  GmresState& g = h->gm;
  if (g.fresh) {
    gmres_launch_cycle<1>(h, atol);
    gmres_launch_v0(h);
    LZ_TRY(check_launch(h, "gmres: first test"));
    g.fresh = false;
  }
  if (g.pending) LZ_TRY(gmres_end_cycle(h, atol));
  return LZ_OK;
}

int gmres_run_args(lz_handle h, const char* who, int steps, double atol_eff) {
  const GmresState& g = h->gm;
  if (steps < 0 || !(atol_eff >= 0.0)) return fail(h, LZ_ERR_ARG, std::string(who) + ": need steps >= 0 and atol_eff >= 0");
  if ((int64_t)g.iters + steps > INT32_MAX / 4) return fail(h, LZ_ERR_ARG, std::string(who) + ": the step counter is an int");
  return LZ_OK;
}

}  // namespace

extern "C" {

int lz_gmres_begin(lz_handle h, int restart, const double* b, const double* x0) {
  if (!h || !b) return LZ_ERR_ARG;
  LZ_TRY(gmres_alloc(h, restart, "lz_gmres_begin"));
  GmresState& g = h->gm;
  const size_t bytes = (size_t)h->rows * sizeof(double);
  LZ_TRY(upload(h, gmres_b(g), b, bytes));
  gmres_launch_residual(h, nullptr);  // w = b - 0 and the partials of |b|^2
  gmres_launch_cycle<2>(h, 0.0);
  LZ_TRY(check_launch(h, "gmres begin: |b|"));
  if (x0) {
    LZ_TRY(upload(h, gmres_x(g), x0, bytes));
    gmres_product(h, gmres_x(g), g.B.w);
    LZ_TRY(check_launch(h, "gmres begin: product"));
    gmres_launch_residual(h, nullptr);
    LZ_TRY(check_launch(h, "gmres begin: r0"));
  }
  LZ_HIP(h, hipStreamSynchronize(h->stream));  // (b and x0 are the caller's)
  g.fresh = true;
  g.live = true;
  return LZ_OK;
}

int lz_gmres_run(lz_handle h, int steps, double atol_eff, double* state_out) {
  LZ_TRY(gmres_state(h, "lz_gmres_run"));
  GmresState& g = h->gm;
  LZ_TRY(gmres_run_args(h, "lz_gmres_run", steps, atol_eff));
  if (g.done && !g.fresh) return gmres_read_state(h, state_out);
  LZ_TRY(gmres_reserve(h, g.hist, g.hist_cap, 1, g.iters + steps));
  LZ_TRY(gmres_reserve(h, g.chist, g.chist_cap, 3, g.cycles + steps + 2));
  LZ_TRY(gmres_head(h, atol_eff));
  const GmresSmall L = gmres_small_layout(g.m);
  const OrthBasis& V = g.B;
  double* sm = g.wk.sm;
  const QtwPlan plan = orth_plan(h, V);
  const OrthPass2 pass2 = (h->flags & LZ_FLAG_TRL_PASS2_ALWAYS) ? OrthPass2::kForced : OrthPass2::kGated;
  for (int i = 0; i < steps; ++i) {
    const int j = g.hcol;
    gmres_product(h, V.B + (int64_t)j * V.ld, V.w);  // w = A V[j]
    // w against V[0..j]: the Hessenberg column; h1 = |w|, V[j + 1] = w / h1
    LZ_TRY(orth_cgs_step(h, V, g.wk, plan, j + 1, sm + L.proj, sm + L.h1, pass2));
    hipLaunchKernelGGL(k_gmres_column, dim3(1), dim3(kTPB), 0, h->stream, j, g.m, sm + L.proj, sm + L.h1, sm + L.c1 + j + 1, sm + L.R, sm + L.gc, sm + L.gs,
                       sm + L.S, sm + L.ds, g.di, g.hist, g.hist_cap);
    LZ_TRY(check_launch(h, "gmres: step"));
    g.hcol = j + 1;
    if (g.hcol == g.m) LZ_TRY(gmres_end_cycle(h, atol_eff));  // the cycle end the host can foresee
  }
  return gmres_read_state(h, state_out);
}

int lz_gmres_end_cycle(lz_handle h, double atol_eff, double* state_out) {
  LZ_TRY(gmres_state(h, "lz_gmres_end_cycle"));
  GmresState& g = h->gm;
  LZ_TRY(gmres_run_args(h, "lz_gmres_end_cycle", 0, atol_eff));
  if (g.done && !g.fresh) return gmres_read_state(h, state_out);
  LZ_TRY(gmres_reserve(h, g.chist, g.chist_cap, 3, g.cycles + 2));
  LZ_TRY(gmres_head(h, atol_eff));
  if (g.hcol > 0) LZ_TRY(gmres_end_cycle(h, atol_eff));
  return gmres_read_state(h, state_out);
}

int lz_gmres_history(lz_handle h, double* presid_out, int count, double* cycles_out, int ncycles) {
  LZ_TRY(gmres_state(h, "lz_gmres_history"));
  const GmresState& g = h->gm;
  if (count < 0 || count > g.hist_cap || ncycles < 0 || ncycles > g.chist_cap || (count > 0 && !presid_out) || (ncycles > 0 && !cycles_out))
    return fail(h, LZ_ERR_ARG, "lz_gmres_history: need 0 <= count <= the steps and 0 <= ncycles <= the cycles lz_gmres_run was asked for so far (at least 1024)");
  if (count > 0) LZ_HIP(h, hipMemcpyAsync(presid_out, g.hist, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (ncycles > 0) LZ_HIP(h, hipMemcpyAsync(cycles_out, g.chist, 3 * (size_t)ncycles * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_gmres_get(lz_handle h, int which, double* out) {
  LZ_TRY(gmres_state(h, "lz_gmres_get"));
  const GmresState& g = h->gm;
  const GmresSmall L = gmres_small_layout(g.m);
  const int m = g.m;
  const bool raw = (which & LZ_GMRES_RAW) != 0;
  const int w = which & ~LZ_GMRES_RAW;
  if (!out || w < 0 || w > LZ_GMRES_SMALL) return fail(h, LZ_ERR_ARG, "lz_gmres_get: which is LZ_GMRES_X .. LZ_GMRES_SMALL, the vectors with or without LZ_GMRES_RAW");
  const double* sm = g.wk.sm;
  if (w <= LZ_GMRES_B) {
    const double* src = w == LZ_GMRES_X ? gmres_x(g) : w == LZ_GMRES_W ? g.B.w : gmres_b(g);
    LZ_HIP(h, hipMemcpyAsync(out, src, (raw ? (size_t)g.B.pad : (size_t)g.B.len) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  } else if (w == LZ_GMRES_Y) {
    LZ_HIP(h, hipMemcpyAsync(out, sm + L.y, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  } else if (w == LZ_GMRES_ROWS) {
    return orth_get_rows(h, g.B, "lz_gmres_get", "restart", 0, m + 1, out, g.B.pad);
  } else {
    std::vector<double> buf((size_t)(L.total - L.R));
    double ds[kGmresDoubles];
    int di[kGmresInts];
    LZ_HIP(h, hipMemcpyAsync(buf.data(), sm + L.R, buf.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    LZ_HIP(h, hipMemcpyAsync(di, g.di, sizeof(di), hipMemcpyDeviceToHost, h->stream));
    LZ_HIP(h, hipStreamSynchronize(h->stream));
    memcpy(ds, buf.data() + (L.ds - L.R), sizeof(ds));
    memcpy(out, buf.data(), ((size_t)m * m + 3 * (size_t)m + 1) * sizeof(double));  // (R, c, s and S lie in this order)
    double* sc = out + (size_t)m * m + 3 * (size_t)m + 1;
    sc[0] = (double)di[kGmCols];
    sc[1] = ds[kGmPtol];
    sc[2] = ds[kGmFactor];
    sc[3] = ds[kGmPresid];
    sc[4] = ds[kGmRnorm];
    sc[5] = ds[kGmBnorm];
    sc[6] = (double)di[kGmInner];
    sc[7] = (double)di[kGmBreakdown];
    sc[8] = (double)di[kGmDone];
    sc[9] = (double)di[kGmConverged];
    sc[10] = (double)di[kGmIters];
    sc[11] = (double)di[kGmCycles];
    // what the last step handed to k_gmres_column: its coefficients, h1 and the self slot of pass 1's dots at every index
    LZ_HIP(h, hipMemcpyAsync(sc + 12, sm + L.proj, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    LZ_HIP(h, hipMemcpyAsync(sc + 12 + m, sm + L.h1, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    LZ_HIP(h, hipMemcpyAsync(sc + 13 + m, sm + L.c1 + 1, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    LZ_HIP(h, hipStreamSynchronize(h->stream));
    return LZ_OK;
  }
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_gmres_set_state(lz_handle h, int restart, const double* x, const double* b, const double* w, const double* rows, int nrows, const double* small) {
  if (!h || !x || !b || !w || !rows || !small) return LZ_ERR_ARG;
  LZ_TRY(gmres_alloc(h, restart, "lz_gmres_set_state"));
  GmresState& g = h->gm;
  const int m = g.m;
  const GmresSmall L = gmres_small_layout(m);
  const double* sc = small + (size_t)m * m + 3 * (size_t)m + 1;
  const int cols = (int)sc[0], iters = (int)sc[10], cycles = (int)sc[11];
  if (nrows < 1 || nrows > m + 1 || cols < 0 || cols > m || nrows < std::min(cols + 1, m) || iters < 0 || cycles < 0)
    return fail(h, LZ_ERR_ARG, "lz_gmres_set_state: need 1 <= nrows <= restart + 1, 0 <= cols <= restart with rows 0 .. min(cols, restart - 1) given, counters >= 0");
  LZ_TRY(gmres_reserve(h, g.hist, g.hist_cap, 1, iters + 1));
  LZ_TRY(gmres_reserve(h, g.chist, g.chist_cap, 3, cycles + 2));
  const size_t bytes = (size_t)h->rows * sizeof(double);
  LZ_TRY(upload(h, gmres_x(g), x, bytes));
  LZ_TRY(upload(h, gmres_b(g), b, bytes));
  LZ_TRY(upload(h, g.B.w, w, (size_t)g.B.pad * sizeof(double)));
  LZ_TRY(orth_set_rows(h, g.B, "lz_gmres_set_state", "restart", 0, nrows, rows, g.B.pad));
  LZ_TRY(upload(h, g.wk.sm + L.R, small, ((size_t)m * m + 3 * (size_t)m + 1) * sizeof(double)));
  double ds[kGmresDoubles] = {0.0};
  ds[kGmPtol] = sc[1];
  ds[kGmFactor] = sc[2];
  ds[kGmPresid] = sc[3];
  ds[kGmRnorm] = sc[4];
  ds[kGmBnorm] = sc[5];
  const int di[kGmresInts] = {sc[8] != 0.0, sc[6] != 0.0, sc[7] != 0.0, sc[9] != 0.0, cols, iters, cycles, 0};
  LZ_HIP(h, hipMemcpyAsync(g.wk.sm + L.ds, ds, sizeof(ds), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipMemcpyAsync(g.di, di, sizeof(di), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));  // (the sources are the caller's and this frame's)
  g.iters = iters;
  g.cycles = cycles;
  g.done = di[kGmDone];
  g.hcol = cols;
  g.pending = !g.done && di[kGmInner] != 0;
  g.fresh = false;
  g.live = true;
  return LZ_OK;
}

int lz_gmres_step_time(lz_handle h, int reps, double* ms_out) {
  LZ_TRY(gmres_state(h, "lz_gmres_step_time"));
  GmresState& g = h->gm;
  if (!ms_out || reps < 1) return fail(h, LZ_ERR_ARG, "lz_gmres_step_time: need reps >= 1 and ms_out");
  if (g.done || g.fresh || g.pending || g.hcol < 1)
    return fail(h, LZ_ERR_STATE, "lz_gmres_step_time: needs a state inside a cycle, behind at least one step, with no exit flag set (a flagged state's kernels return at once)");
  const GmresSmall L = gmres_small_layout(g.m);
  const OrthBasis& V = g.B;
  double* sm = g.wk.sm;
  const QtwPlan plan = orth_plan(h, V);
  const int cols = g.hcol;
  hipEvent_t a, b;
  LZ_HIP(h, hipEventCreate(&a));
  LZ_HIP(h, hipEventCreate(&b));
  hipError_t err = hipSuccess;
  int rc = LZ_OK;
  for (int what = 0; what < 5 && err == hipSuccess && rc == LZ_OK; ++what) {
    for (int r = -1; r < reps && rc == LZ_OK; ++r) {  // (r == -1: the warm-up)
      if (r == 0) err = hipEventRecord(a, h->stream);
      if (what == 0)
        gmres_product(h, V.B + (int64_t)(cols - 1) * V.ld, V.w);
      else if (what == 1)  // (scratch: row cols and the step's coefficient slots are written again)
        rc = orth_cgs_step(h, V, g.wk, plan, cols, sm + L.proj, sm + L.h1, OrthPass2::kForced);
      else if (what == 2)
        hipLaunchKernelGGL(k_gmres_update, dim3(gmres_blocks(V.pad)), dim3(kTPB), 0, h->stream, V.B, V.ld, V.pad >> 1, V.len, gmres_x(g), sm + L.y, g.di);
      else if (what == 3)
        launch_trl_cgs(V.B, V.ld, V.pad, cols, sm + L.y, V.w, g.wk.part, nullptr, h->stream);
      else
        gmres_launch_residual(h, g.di + kGmDone);
    }
    if (err == hipSuccess) err = hipEventRecord(b, h->stream);
    if (err == hipSuccess) err = hipEventSynchronize(b);
    float ms = 0.f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, a, b);
    ms_out[what] = (double)ms / reps;
  }
  hipEventDestroy(a);
  hipEventDestroy(b);
  g.live = false;  // (the repeated passes have been applied to w and x again and again)
  LZ_TRY(rc);
  LZ_HIP(h, err);
  return check_launch(h, "gmres step time");
}

int lz_gmres_info(lz_handle h, int* out) {
  if (!h || !out) return LZ_ERR_ARG;
  const GmresState& g = h->gm;
  // the product (counted as one), two passes of dots, final sums, update and post each, the scale-and-store, k_gmres_column
  out[0] = 1 + 2 * 4 + 1 + 1;
  out[1] = 6;  // the end of a cycle: solve, update, the product, residual, cycle, scale-and-store
  out[2] = g.live && h->kind != 0 && skew_stride(h, h->rows_pad) == g.B.ld && h->rows == g.B.len ? 1 : 0;
  out[3] = g.live ? g.m : 0;
  return LZ_OK;
}

}  // extern "C"
