// Conjugate gradients (include/lanczos_hip.h, "symmetric positive definite linear solves"): the device half of lanczos_amd.cg, A x = b
// for a real symmetric positive definite A with an optional diagonal preconditioner d (z = d o r), SciPy's loop scalar for scalar.
// Four vectors (x, r, p, q) and d.  The product q = A p is the handle's, untouched, called with x_own = p: its x_own . y epilogue
// yields the partials of p . q on every plan (here x_own is x, so the column-blocked two-phase plan takes it too).  What is new here
// is the vector side, two streaming passes and two one-block kernels per iteration:
//   k_cg_alpha    one block: pq = p . q from the product's partials, the breakdown test (pq == 0 or alpha not finite: -1), alpha =
//                 rho / pq, the first iteration with pq <= 0 recorded
//   k_cg_r        r -= alpha q, the partials of r . r and of r . z with z = d o r formed on the fly and never stored
//                                                                   reads r, q (and d), writes r:        24 (32) B a row
//   k_cg_scalars  one block: |r|, the history, the head test of the NEXT iteration (|r| < atol: done, converged), rho = r . z (not
//                 finite: -1), beta = rho / rho_prev, the iteration counter, the done flag
//   k_cg_p        x += alpha p, then p = d o r + beta p from the same load of p
//                                                                   reads r, p, x (and d), writes p, x:  40 (48) B a row
// 64 (80) bytes a row against 72 (88) where x and r share a pass and p has its own, which reads p twice.  The update of x belongs to
// the iteration whose end raises the done flag: k_cg_scalars stamps the flag with that iteration's number and k_cg_p, which the host
// hands the number of its own iteration, applies x += alpha p alone where the two agree; every later launch returns at once.  So a
// chunk of iterations is enqueued with no host synchronisation; the products of the rest of the chunk run on (their output goes to
// Q, which nothing reads then).  No atomics: the same input gives the same bits.
#include "lz_context.h"
#include "lz_device.h"

using namespace lz;
using namespace lz::api;

namespace lz {

// ds: the scalars on the device
enum CgD {
  kCgRho = 0,  // r . z of the coming iteration
  kCgRhoPrev,
  kCgAlpha,
  kCgBeta,   // of the last k_cg_p
  kCgRnorm,  // the recurrence's |r| at the last head test
  kCgPq,
  kCgDoubles = 8
};
// di; kCgStep counts the iterations that updated x, so it is SciPy's `iteration` of the coming one.  kCgXAt: the value of kCgStep
// behind the iteration whose k_cg_p still owes x its update although the done flag is up (0: none).
enum CgI { kCgDone = 0, kCgStep, kCgCode, kCgExit, kCgHead, kCgXAt, kCgIndef, kCgInts = 8 };
enum { kCgExitNone = 0, kCgExitConverged = 1, kCgExitBreakdown = 2 };

struct CgVecs {
  double* X;
  double* R;
  double* P;
  double* Q;
  double* D;
};

__device__ __forceinline__ bool cg_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // (false for NaN)

// pq = p . q from np partials (k_final_sum's grouping); pq == 0 or alpha not finite: the breakdown -1 with x as it is
__global__ __launch_bounds__(kTPB) void k_cg_alpha(const double* __restrict__ part, int np, double* __restrict__ ds, int* __restrict__ di) {
  __shared__ double sm16[16];
  if (di[kCgDone]) return;
  const double pq = final_sum_emulated(part, np, sm16);  // (every thread has read the flag before thread 0 writes it: the barriers inside)
  if (threadIdx.x != 0) return;
  ds[kCgPq] = pq;
  const double alpha = ds[kCgRho] / pq;
  if (pq == 0.0 || !cg_finite(alpha)) {
    di[kCgCode] = -1;
    di[kCgExit] = kCgExitBreakdown;
    di[kCgHead] = 0;
    di[kCgDone] = 1;
    return;
  }
  ds[kCgAlpha] = alpha;
  if (pq <= 0.0 && di[kCgIndef] < 0) di[kCgIndef] = di[kCgStep];
}

// r -= alpha q; part_rr[b] = block b's share of r . r; PRE: part_rz[b] = its share of r . (d o r).  Grid-stride over 16-byte
// positions, k_minres_step's shape: two positions of a lane in flight, one grid stride apart, every load of both issued before the
// first use.
template <bool PRE>
__global__ __launch_bounds__(kTPB) void k_cg_r(CgVecs cv, const double* __restrict__ ds, const int* __restrict__ di, int64_t n2,
                                              double* __restrict__ part_rr, double* __restrict__ part_rz) {
  __shared__ double sm[kTPB / 64];
  if (di[kCgDone]) return;
  const double alpha = ds[kCgAlpha];
  double2* r2 = reinterpret_cast<double2*>(cv.R);
  const double2* q2 = reinterpret_cast<const double2*>(cv.Q);
  const double2* d2 = reinterpret_cast<const double2*>(cv.D);
  double acc = 0.0, acc2 = 0.0;
  constexpr int U = 2;
  const int64_t stride = (int64_t)gridDim.x * kTPB;
  for (int64_t i0 = (int64_t)blockIdx.x * kTPB + threadIdx.x; i0 < n2; i0 += U * stride) {
    double2 r[U], q[U], d[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      in[u] = i < n2;
      if (!in[u]) continue;
      r[u] = ld_stream<1>(r2 + i);
      q[u] = ld_stream<1>(q2 + i);  // (the product overwrites it)
      if (PRE) d[u] = d2[i];        // (k_cg_p reads it next)
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (!in[u]) continue;
      r[u].x = r[u].x - alpha * q[u].x;
      r[u].y = r[u].y - alpha * q[u].y;
      r2[i] = r[u];  // plain store: k_cg_p reads it
      acc = fma(r[u].x, r[u].x, acc);
      acc = fma(r[u].y, r[u].y, acc);
      if (PRE) {
        acc2 = fma(r[u].x, d[u].x * r[u].x, acc2);
        acc2 = fma(r[u].y, d[u].y * r[u].y, acc2);
      }
    }
  }
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) part_rr[blockIdx.x] = acc;
  if (PRE) {
    acc2 = block_sum(acc2, sm);
    if (threadIdx.x == 0) part_rz[blockIdx.x] = acc2;
  }
}

// ADVANCE: the end of an iteration - the counter, rho_prev, beta - and the head test of the next one.  !ADVANCE: the head test of the
// iteration that a fresh state (lz_cg_begin, lz_cg_set_state) starts from; p is in place, so no beta.  part_rz null: rho = r . r (no
// preconditioner); given: rho is the uploaded one (lz_cg_set_state).
template <bool ADVANCE>
__global__ __launch_bounds__(kTPB) void k_cg_scalars(const double* __restrict__ part_rr, const double* __restrict__ part_rz, int np, int given,
                                                    double* __restrict__ ds, int* __restrict__ di, double* __restrict__ hist, int hist_cap, double atol) {
  __shared__ double sm16[16];
  if (di[kCgDone]) return;
  const double rr = final_sum_emulated(part_rr, np, sm16);
  const double rz = part_rz ? final_sum_emulated(part_rz, np, sm16) : rr;
  if (threadIdx.x != 0) return;
  const double rnorm = sqrt(rr);
  int k = di[kCgStep];
  double rho_prev = ds[kCgRhoPrev];
  const double rho = given ? ds[kCgRho] : rz;
  if (ADVANCE) {
    k = k + 1;
    di[kCgStep] = k;
    rho_prev = ds[kCgRho];
    ds[kCgRhoPrev] = rho_prev;
  }
  if (k < hist_cap) hist[k] = rnorm;
  ds[kCgRho] = rho;
  ds[kCgRnorm] = rnorm;
  int code = 0, ex = kCgExitNone;
  if (rnorm < atol) {
    ex = kCgExitConverged;
  } else if (!cg_finite(rho)) {
    code = -1;
    ex = kCgExitBreakdown;
  } else if (ADVANCE) {
    ds[kCgBeta] = rho / rho_prev;
  }
  if (ex != kCgExitNone) {
    di[kCgCode] = code;
    di[kCgExit] = ex;
    di[kCgHead] = 1;
    di[kCgXAt] = ADVANCE ? k : 0;  // (the iteration that just ended still owes x its update: its k_cg_p applies it)
    di[kCgDone] = 1;
  }
}

// x += alpha p, then p = d o r + beta p from the same load of p (!PRE: p = r + beta p).  `it`: the counter behind this iteration; under
// the done flag the pass returns at once unless the flag was raised at the end of this very iteration, where x alone is updated.
template <bool PRE>
__global__ __launch_bounds__(kTPB) void k_cg_p(CgVecs cv, const double* __restrict__ ds, const int* __restrict__ di, int64_t n2, int it) {
  const bool last = di[kCgDone] != 0;
  if (last && di[kCgXAt] != it) return;
  const double alpha = ds[kCgAlpha], beta = ds[kCgBeta];
  const double2* r2 = reinterpret_cast<const double2*>(cv.R);
  const double2* d2 = reinterpret_cast<const double2*>(cv.D);
  double2* p2 = reinterpret_cast<double2*>(cv.P);
  double2* x2 = reinterpret_cast<double2*>(cv.X);
  constexpr int U = 2;
  const int64_t stride = (int64_t)gridDim.x * kTPB;
  for (int64_t i0 = (int64_t)blockIdx.x * kTPB + threadIdx.x; i0 < n2; i0 += U * stride) {
    double2 r[U], p[U], x[U], d[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      in[u] = i < n2;
      if (!in[u]) continue;
      x[u] = ld_stream<1>(x2 + i);
      p[u] = ld_stream<1>(p2 + i);
      if (!last) {
        r[u] = r2[i];             // (k_cg_r reads it next)
        if (PRE) d[u] = d2[i];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (!in[u]) continue;
      x[u].x = x[u].x + alpha * p[u].x;
      x[u].y = x[u].y + alpha * p[u].y;
      st_stream<1>(x2 + i, x[u]);
      if (!last) {
        if (PRE) {
          r[u].x = d[u].x * r[u].x;
          r[u].y = d[u].y * r[u].y;
        }
        p[u].x = r[u].x + beta * p[u].x;
        p[u].y = r[u].y + beta * p[u].y;
        p2[i] = p[u];  // plain store: the product reads it
      }
    }
  }
}

// r = r - y (r holds b, y = A x0)
__global__ __launch_bounds__(kTPB) void k_cg_r0(double* __restrict__ r, const double* __restrict__ y, int64_t n2) {
  double2* r2 = reinterpret_cast<double2*>(r);
  const double2* y2 = reinterpret_cast<const double2*>(y);
  for (int64_t i = (int64_t)blockIdx.x * kTPB + threadIdx.x; i < n2; i += (int64_t)gridDim.x * kTPB) {
    double2 v = r2[i];
    const double2 yy = y2[i];
    v.x = v.x - yy.x;
    v.y = v.y - yy.y;
    r2[i] = v;
  }
}

// the state as lz_cg_begin leaves it: p = d o r (!PRE: p = r), part_rr[b] / part_rz[b] = block b's share of r . r / r . (d o r).
// SETP false: the partials only (lz_cg_set_state uploads p).
template <bool PRE, bool SETP>
__global__ __launch_bounds__(kTPB) void k_cg_first(CgVecs cv, int64_t n2, double* __restrict__ part_rr, double* __restrict__ part_rz) {
  __shared__ double sm[kTPB / 64];
  const double2* r2 = reinterpret_cast<const double2*>(cv.R);
  const double2* d2 = reinterpret_cast<const double2*>(cv.D);
  double2* p2 = reinterpret_cast<double2*>(cv.P);
  double acc = 0.0, acc2 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kTPB + threadIdx.x; i < n2; i += (int64_t)gridDim.x * kTPB) {
    const double2 r = r2[i];
    double2 z = r;
    if (PRE) {
      const double2 d = d2[i];
      z.x = d.x * r.x;
      z.y = d.y * r.y;
    }
    if (SETP) p2[i] = z;
    acc = fma(r.x, r.x, acc);
    acc = fma(r.y, r.y, acc);
    if (PRE) {
      acc2 = fma(r.x, z.x, acc2);
      acc2 = fma(r.y, z.y, acc2);
    }
  }
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) part_rr[blockIdx.x] = acc;
  if (PRE) {
    acc2 = block_sum(acc2, sm);
    if (threadIdx.x == 0) part_rz[blockIdx.x] = acc2;
  }
}

constexpr int kCgMaxBlocks = 2048;  // k_minres_step's grid
static int cg_blocks(int64_t pad) {
  const int64_t g = ((pad >> 1) + kTPB - 1) / kTPB;
  return (int)std::min<int64_t>(std::max<int64_t>(g, 1), kCgMaxBlocks);
}

namespace api {

void cg_free(lz_handle h) {
  CgState& m = h->cg;
  big_free(m.vec);
  big_free(m.ds);
  big_free(m.di);
  big_free(m.part);
  big_free(m.hist);
  m = CgState();
}

}  // namespace api
}  // namespace lz

namespace {

CgVecs cg_vecs(const CgState& m) {
  CgVecs cv;
  cv.X = m.vec;
  cv.R = m.vec + m.ld;
  cv.P = m.vec + 2 * m.ld;
  cv.Q = m.vec + 3 * m.ld;
  cv.D = m.vec + 4 * m.ld;
  return cv;
}

// partials that the product writes (trl_alloc's terms)
size_t cg_product_part(lz_handle h) {
  size_t need = std::max<size_t>((size_t)h->rows / 4 + 64, (size_t)h->csr.n_rowblk + 64);
  if (h->kind == 1 && h->csr.pb) need = std::max<size_t>(need, (size_t)pb_num_partials(h->csr.pb) + 64);
  return need;
}

// the two sets of partials of the passes' own, behind the product's
double* cg_part(lz_handle h, int set) { return h->cg.part + cg_product_part(h) + (size_t)set * kCgMaxBlocks; }

int cg_alloc(lz_handle h, const char* who) {
  CgState& m = h->cg;
  if (h->kind == 0)
    return fail(h, LZ_ERR_STATE, std::string(who) + (h->z.kind != 0 ? ": a complex matrix is set (CG takes a real one)" : ": no matrix set"));
  if (h->world > 1 || h->comm_kind != 0) return fail(h, LZ_ERR_STATE, std::string(who) + ": CG runs on one rank (this handle has a communicator)");
  if (h->flags & (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE))
    return fail(h, LZ_ERR_STATE, std::string(who) + ": not with LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE");
  if (h->rows < 1 || h->ncols_ext != h->rows) return fail(h, LZ_ERR_STATE, std::string(who) + ": the matrix is not square on this rank");
  LZ_HIP(h, hipSetDevice(h->dev));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  m.live = false;
  const int64_t ld = h->rows_pad;
  if (!m.vec || m.ld != ld) {
    LZ_TRY(dev_alloc(h, m.vec, 5 * (size_t)ld));
    m.ld = ld;
  }
  if (!m.ds) LZ_TRY(dev_alloc(h, m.ds, (size_t)kCgDoubles));
  if (!m.di) LZ_TRY(dev_alloc(h, m.di, (size_t)kCgInts));
  const size_t need = cg_product_part(h) + 2 * (size_t)kCgMaxBlocks;
  if (m.part_cap < need) {
    LZ_TRY(dev_alloc(h, m.part, need));
    m.part_cap = need;
  }
  LZ_HIP(h, hipMemsetAsync(m.vec, 0, 5 * (size_t)ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(m.ds, 0, kCgDoubles * sizeof(double), h->stream));
  if (m.hist) LZ_HIP(h, hipMemsetAsync(m.hist, 0, (size_t)m.hist_cap * sizeof(double), h->stream));
  m.steps = 0;
  m.done = 0;
  m.fresh = false;
  m.given = false;
  m.pre = false;
  return LZ_OK;
}

// the history holds at least `count` head tests; what it holds is kept
int cg_hist_reserve(lz_handle h, int count) {
  CgState& m = h->cg;
  if (count <= m.hist_cap) return LZ_OK;
  const int cap = std::max(count, std::max(1024, 2 * m.hist_cap));
  double* p = nullptr;
  LZ_TRY(dev_alloc(h, p, (size_t)cap));
  LZ_HIP(h, hipMemsetAsync(p, 0, (size_t)cap * sizeof(double), h->stream));
  if (m.hist && m.hist_cap > 0) LZ_HIP(h, hipMemcpyAsync(p, m.hist, (size_t)m.hist_cap * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  LZ_TRY(dev_free(h, m.hist));
  m.hist = p;
  m.hist_cap = cap;
  return LZ_OK;
}

int cg_state(lz_handle h, const char* who) {
  if (!h) return LZ_ERR_ARG;
  const CgState& m = h->cg;
  if (!m.live || !m.vec) return fail(h, LZ_ERR_STATE, std::string(who) + ": no state (lz_cg_begin first; a new matrix drops it)");
  if (h->kind == 0 || h->rows_pad != m.ld) return fail(h, LZ_ERR_STATE, std::string(who) + ": the matrix changed since lz_cg_begin");
  if (h->world > 1 || h->comm_kind != 0 || (h->flags & (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE)))
    return fail(h, LZ_ERR_STATE, std::string(who) + ": CG runs on one rank, without LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE");
  LZ_HIP(h, hipSetDevice(h->dev));
  return LZ_OK;
}

// y = A x with the x . y partials at part; returns their count (lz_bicgstab.hip's route)
int cg_product(lz_handle h, const double* x, double* y, double* part) {
  if (h->kind == 1) return launch_spmv_csr(h->csr, x, y, x, part, h->flags, h->stream);
  return launch_gemv_dense(h->d_dense, h->rows, h->ncols_ext, h->dense_lda, x, x, y, part, h->stream);
}

// the partials of r . r (set 0) and r . z (set 1) of the state as it stands - what the first lz_cg_run's head test reads - and, SETP,
// p = d o r
template <bool SETP>
void cg_launch_first(lz_handle h) {
  const CgState& m = h->cg;
  const CgVecs cv = cg_vecs(m);
  const int grid = cg_blocks(m.ld);
  if (m.pre)
    hipLaunchKernelGGL((k_cg_first<true, SETP>), dim3(grid), dim3(kTPB), 0, h->stream, cv, m.ld >> 1, cg_part(h, 0), cg_part(h, 1));
  else
    hipLaunchKernelGGL((k_cg_first<false, SETP>), dim3(grid), dim3(kTPB), 0, h->stream, cv, m.ld >> 1, cg_part(h, 0), cg_part(h, 1));
}

void cg_launch_r(lz_handle h, const CgVecs& cv, int grid, int64_t n2) {
  const CgState& m = h->cg;
  if (m.pre)
    hipLaunchKernelGGL(k_cg_r<true>, dim3(grid), dim3(kTPB), 0, h->stream, cv, m.ds, m.di, n2, cg_part(h, 0), cg_part(h, 1));
  else
    hipLaunchKernelGGL(k_cg_r<false>, dim3(grid), dim3(kTPB), 0, h->stream, cv, m.ds, m.di, n2, cg_part(h, 0), cg_part(h, 1));
}

void cg_launch_p(lz_handle h, const CgVecs& cv, int grid, int64_t n2, int it) {
  const CgState& m = h->cg;
  if (m.pre)
    hipLaunchKernelGGL(k_cg_p<true>, dim3(grid), dim3(kTPB), 0, h->stream, cv, m.ds, m.di, n2, it);
  else
    hipLaunchKernelGGL(k_cg_p<false>, dim3(grid), dim3(kTPB), 0, h->stream, cv, m.ds, m.di, n2, it);
}

int cg_read_state(lz_handle h, double* state_out) {
  CgState& m = h->cg;
  double ds[kCgDoubles];
  int di[kCgInts];
  LZ_HIP(h, hipMemcpyAsync(ds, m.ds, sizeof(ds), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipMemcpyAsync(di, m.di, sizeof(di), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  m.steps = di[kCgStep];
  m.done = di[kCgDone];
  if (state_out) {
    for (int i = 0; i < 16; ++i) state_out[i] = 0.0;
    state_out[0] = (double)m.steps;
    state_out[1] = (double)m.done;
    state_out[2] = (double)di[kCgCode];
    state_out[3] = (double)di[kCgExit];
    state_out[4] = (double)di[kCgHead];
    state_out[5] = ds[kCgRnorm];
    state_out[6] = ds[kCgRho];
    state_out[7] = ds[kCgRhoPrev];
    state_out[8] = ds[kCgAlpha];
    state_out[9] = ds[kCgBeta];
    state_out[10] = ds[kCgPq];
    state_out[11] = (double)di[kCgIndef];
  }
  return LZ_OK;
}

}  // namespace

extern "C" {

int lz_cg_begin(lz_handle h, const double* b, const double* x0, const double* d) {
  if (!h || !b) return LZ_ERR_ARG;
  LZ_TRY(cg_alloc(h, "lz_cg_begin"));
  CgState& m = h->cg;
  const CgVecs cv = cg_vecs(m);
  const size_t bytes = (size_t)h->rows * sizeof(double);
  LZ_TRY(upload(h, cv.R, b, bytes));
  if (d) LZ_TRY(upload(h, cv.D, d, bytes));
  m.pre = d != nullptr;
  if (x0) {
    LZ_TRY(upload(h, cv.X, x0, bytes));
    cg_product(h, cv.X, cv.Q, m.part);
    LZ_TRY(check_launch(h, "cg begin: product"));
    hipLaunchKernelGGL(k_cg_r0, dim3(cg_blocks(m.ld)), dim3(kTPB), 0, h->stream, cv.R, cv.Q, m.ld >> 1);
    LZ_TRY(check_launch(h, "cg begin: r0"));
    LZ_HIP(h, hipMemsetAsync(cv.Q, 0, (size_t)m.ld * sizeof(double), h->stream));
  }
  cg_launch_first<true>(h);
  LZ_TRY(check_launch(h, "cg begin: rho"));
  const int di[kCgInts] = {0, 0, 0, 0, 0, 0, -1, 0};
  LZ_HIP(h, hipMemcpyAsync(m.di, di, sizeof(di), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));  // (b, x0 and d are the caller's, di this frame's)
  m.fresh = true;
  m.live = true;
  return LZ_OK;
}

int lz_cg_run(lz_handle h, int iters, double atol_eff, double* state_out) {
  LZ_TRY(cg_state(h, "lz_cg_run"));
  CgState& m = h->cg;
  if (iters < 0 || !(atol_eff >= 0.0)) return fail(h, LZ_ERR_ARG, "lz_cg_run: need iters >= 0 and atol_eff >= 0");
  if ((int64_t)m.steps + iters > INT32_MAX / 2) return fail(h, LZ_ERR_ARG, "lz_cg_run: the iteration counter is an int");
  if (m.done && !m.fresh) return cg_read_state(h, state_out);
  LZ_TRY(cg_hist_reserve(h, m.steps + iters + 1));
  const CgVecs cv = cg_vecs(m);
  const int grid = cg_blocks(m.ld);
  const int64_t n2 = m.ld >> 1;
  double* p_rr = cg_part(h, 0);
  double* p_rz = m.pre ? cg_part(h, 1) : nullptr;
  if (m.fresh) {  // the head test of the iteration the state starts from
    hipLaunchKernelGGL(k_cg_scalars<false>, dim3(1), dim3(kTPB), 0, h->stream, p_rr, p_rz, grid, m.given ? 1 : 0, m.ds, m.di, m.hist, m.hist_cap, atol_eff);
    LZ_TRY(check_launch(h, "cg: head test"));
    m.fresh = false;
  }
  for (int i = 0; i < iters; ++i) {  // (the device's counter is m.steps + i wherever the done flag is down)
    const int np = cg_product(h, cv.P, cv.Q, m.part);
    LZ_TRY(check_launch(h, "cg: product"));
    hipLaunchKernelGGL(k_cg_alpha, dim3(1), dim3(kTPB), 0, h->stream, m.part, np, m.ds, m.di);
    LZ_TRY(check_launch(h, "cg: alpha"));
    cg_launch_r(h, cv, grid, n2);
    LZ_TRY(check_launch(h, "cg: r"));
    hipLaunchKernelGGL(k_cg_scalars<true>, dim3(1), dim3(kTPB), 0, h->stream, p_rr, p_rz, grid, 0, m.ds, m.di, m.hist, m.hist_cap, atol_eff);
    LZ_TRY(check_launch(h, "cg: scalars"));
    cg_launch_p(h, cv, grid, n2, m.steps + i + 1);
    LZ_TRY(check_launch(h, "cg: p"));
  }
  return cg_read_state(h, state_out);
}

int lz_cg_history(lz_handle h, double* out, int count) {
  LZ_TRY(cg_state(h, "lz_cg_history"));
  const CgState& m = h->cg;
  if (!out || count < 0 || count > m.hist_cap)
    return fail(h, LZ_ERR_ARG, "lz_cg_history: need out and 0 <= count <= the head tests lz_cg_run was asked for so far (at least 1024)");
  if (count == 0) return LZ_OK;
  LZ_HIP(h, hipMemcpyAsync(out, m.hist, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_cg_get(lz_handle h, int which, double* out) {
  LZ_TRY(cg_state(h, "lz_cg_get"));
  const CgState& m = h->cg;
  const bool raw = (which & LZ_CG_RAW) != 0;
  const int w = which & ~LZ_CG_RAW;
  if (!out || w < 0 || w > LZ_CG_D) return fail(h, LZ_ERR_ARG, "lz_cg_get: which is LZ_CG_X .. LZ_CG_D, with or without LZ_CG_RAW");
  const double* src = m.vec + (size_t)w * m.ld;  // (the enum is the order of the vectors)
  const size_t count = raw ? (size_t)m.ld : (size_t)h->rows;
  LZ_HIP(h, hipMemcpyAsync(out, src, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_cg_set_state(lz_handle h, int k, const double* x, const double* r, const double* p, const double* d, const double* scalars) {
  if (!h || !x || !r || !p || !scalars) return LZ_ERR_ARG;
  if (k < 0) return fail(h, LZ_ERR_ARG, "lz_cg_set_state: need k >= 0");
  LZ_TRY(cg_alloc(h, "lz_cg_set_state"));
  CgState& m = h->cg;
  LZ_TRY(cg_hist_reserve(h, k + 1));
  const CgVecs cv = cg_vecs(m);
  const size_t bytes = (size_t)h->rows * sizeof(double);
  LZ_TRY(upload(h, cv.X, x, bytes));
  LZ_TRY(upload(h, cv.R, r, bytes));
  LZ_TRY(upload(h, cv.P, p, bytes));
  if (d) LZ_TRY(upload(h, cv.D, d, bytes));
  m.pre = d != nullptr;
  cg_launch_first<false>(h);
  LZ_TRY(check_launch(h, "cg set_state: |r|"));
  double ds[kCgDoubles] = {0.0};
  ds[kCgRho] = scalars[0];
  const int di[kCgInts] = {0, k, 0, 0, 0, 0, -1, 0};
  LZ_HIP(h, hipMemcpyAsync(m.ds, ds, sizeof(ds), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipMemcpyAsync(m.di, di, sizeof(di), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));  // (the sources are the caller's and this frame's)
  m.steps = k;
  m.done = 0;
  m.fresh = true;
  m.given = true;
  m.live = true;
  return LZ_OK;
}

int lz_cg_step_time(lz_handle h, int reps, double* ms_out) {
  LZ_TRY(cg_state(h, "lz_cg_step_time"));
  CgState& m = h->cg;
  if (!ms_out || reps < 1) return fail(h, LZ_ERR_ARG, "lz_cg_step_time: need reps >= 1 and ms_out");
  if (m.done || m.fresh || m.steps < 1)
    return fail(h, LZ_ERR_STATE, "lz_cg_step_time: needs a state behind at least one iteration that is not done (a done state's kernels return at once)");
  const CgVecs cv = cg_vecs(m);
  const int grid = cg_blocks(m.ld);
  const int64_t n2 = m.ld >> 1;
  hipEvent_t a, b;
  LZ_HIP(h, hipEventCreate(&a));
  LZ_HIP(h, hipEventCreate(&b));
  hipError_t err = hipSuccess;
  for (int what = 0; what < 3 && err == hipSuccess; ++what) {
    for (int r = -1; r < reps; ++r) {  // (r == -1: the warm-up)
      if (r == 0) err = hipEventRecord(a, h->stream);
      if (what == 0)
        cg_product(h, cv.P, cv.Q, m.part);
      else if (what == 1)
        cg_launch_r(h, cv, grid, n2);
      else
        cg_launch_p(h, cv, grid, n2, m.steps);
    }
    if (err == hipSuccess) err = hipEventRecord(b, h->stream);
    if (err == hipSuccess) err = hipEventSynchronize(b);
    float ms = 0.f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, a, b);
    ms_out[what] = (double)ms / reps;
  }
  hipEventDestroy(a);
  hipEventDestroy(b);
  m.live = false;  // (the repeated passes have been applied to r, p and x again and again)
  LZ_HIP(h, err);
  return check_launch(h, "cg step time");
}

int lz_cg_info(lz_handle h, int* out) {
  if (!h || !out) return LZ_ERR_ARG;
  const bool live = h->cg.live && h->kind != 0 && h->rows_pad == h->cg.ld;
  out[0] = 5;  // the product, k_cg_alpha, k_cg_r, k_cg_scalars, k_cg_p
  out[1] = live && h->cg.pre ? 1 : 0;
  out[2] = live ? 1 : 0;
  return LZ_OK;
}

}  // extern "C"
