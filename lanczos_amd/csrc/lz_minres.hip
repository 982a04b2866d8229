// MINRES (include/lanczos_hip.h, "symmetric linear solves"): the device half of lanczos_amd.minres, (A - shift I) x = b for a real
// symmetric A, definite or not (Paige & Saunders 1975).  The Lanczos three-term recurrence without a basis, and the solution updated
// from the QR factorisation of the tridiagonal matrix, one Givens rotation per step.  The products and their x_own . y epilogues are the
// handle's, untouched; what is new here is the vector side:
//   k_minres_step     one streaming pass behind the product of step k: r = y - (alpha + shift) v_k - beta_k v_{k-1} with the fixed-order
//                     partials of |r|^2 and, in the same pass, the END of step k - 1: w_{k-1} and x += phi_{k-1} w_{k-1}, whose scalars
//                     were not known before beta_k was and whose operand v_{k-1} the three-term reads anyway.  The update lags one
//                     step; the same kernel with the three-term switched off (the flush) applies the pending one when a chunk ends.
//   k_minres_alpha    one block: alpha_k from the product's partials.
//   k_minres_scalars  one block: beta_{k+1} from the |r|^2 partials, the rotation, the scalars of the lagged update, phibar, the
//                     step counter, the history and the done flag.
// Every kernel here but the flush reads the done flag first and returns at once when it is set, so a chunk of iterations is enqueued
// with no host synchronisation; the products of the rest of the chunk run on (their output goes to Y, which nothing reads then).
// There is no pass that normalises v_{k+1} = r / beta.  Where the matrix has the scale-on-read SpMV (SpmvScale: the ELL copy every
// product of the matrix takes) that kernel divides wherever it reads r and stores v itself (plan S); otherwise the product runs on the
// un-normalised r, and the step kernel divides y and r by beta as it reads them and stores v from there (plan U).  Bytes per row
// outside the product: plan S 72 (reads y, v_k, v_{k-1}, w_{k-3}, w_{k-2}, x; writes r, w_{k-1}, x), plan U 80 (v_k is a write more);
// the unfused textbook form (three-term 32, scale 16, update 48) is 96.  Launches per iteration: 4 (product, alpha, step, scalars).
// No atomics: the same input gives the same bits.
#include "lz_context.h"
#include "lz_device.h"

using namespace lz;
using namespace lz::api;

namespace lz {

// ds: the scalars on the device
enum MinresD {
  kMrNrm2 = 0,  // nu^2: v_k = R / nu (|r_{k-1}|^2 in a run; 1 behind lz_minres_set_state)
  kMrBeta,      // beta_k of the coming three-term
  kMrAlpha,     // alpha of the last step
  kMrCs,
  kMrSn,
  kMrDbar,
  kMrEpsln,
  kMrPhibar,
  kMrTnorm2,
  kMrBeta1,
  kMrShift,
  kMrOldeps,  // the lagged update's scalars, written by step j's k_minres_scalars, read by the next k_minres_step
  kMrDelta,
  kMrGamma,
  kMrPhi,
  kMrSpare,  // where the scale-on-read SpMV stores its beta
  kMinresDoubles = 16
};
enum MinresI { kMrDone = 0, kMrStep, kMinresInts = 4 };

struct MinresVecs {
  double* V[2];
  double* Y;
  double* R;
  double* W[2];
  double* X;
};

// THREE: the three-term of step k = steps + 1 behind its product; UPD: the end of step j = steps; UNNORM (plan U): Y = A R and
// v_k = R / nu is formed and stored here.  Grid-stride over 16-byte positions, k_three_term's shape; part[b] = block b's share of |r|^2.
template <bool THREE, bool UPD, bool UNNORM>
__global__ __launch_bounds__(kTPB) void k_minres_step(MinresVecs mv, const double* __restrict__ ds, const int* __restrict__ di, int64_t n2,
                                                     double* __restrict__ part) {
  __shared__ double sm[kTPB / 64];
  if (THREE && di[kMrDone]) return;  // (the flush is not gated: it ends the step that set the flag)
  const int j = di[kMrStep];
  const double2* vj = reinterpret_cast<const double2*>(mv.V[j & 1]);
  double2* vk = reinterpret_cast<double2*>(mv.V[(j + 1) & 1]);
  double2* y2 = reinterpret_cast<double2*>(mv.Y);
  double2* r2 = reinterpret_cast<double2*>(mv.R);
  double2* wj = reinterpret_cast<double2*>(mv.W[j & 1]);  // holds w_{j-2}, becomes w_j
  const double2* wm = reinterpret_cast<const double2*>(mv.W[(j + 1) & 1]);
  double2* x2 = reinterpret_cast<double2*>(mv.X);
  double a = 0.0, b = 0.0, nu = 1.0, oldeps = 0.0, delta = 0.0, gamma = 1.0, phi = 0.0;
  if (THREE) {
    a = ds[kMrAlpha] + ds[kMrShift];
    b = ds[kMrBeta];
    if (UNNORM) nu = sqrt(ds[kMrNrm2]);
  }
  if (UPD) {
    oldeps = ds[kMrOldeps];
    delta = ds[kMrDelta];
    gamma = ds[kMrGamma];
    phi = ds[kMrPhi];
  }
  double acc = 0.0;
  // two positions of a lane in flight, one grid stride apart: every load of both is issued before the first use, and the partial is
  // accumulated in the order of the positions, so the sums are those of the plain loop
  constexpr int U = 2;
  const int64_t stride = (int64_t)gridDim.x * kTPB;
  for (int64_t i0 = (int64_t)blockIdx.x * kTPB + threadIdx.x; i0 < n2; i0 += U * stride) {
    double2 m[U], y[U], v[U], w2[U], w1[U], x[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      in[u] = i < n2;
      if (!in[u]) continue;
      m[u] = vj[i];
      if (THREE) {
        y[u] = ld_stream<1>(y2 + i);
        v[u] = UNNORM ? r2[i] : vk[i];
      }
      if (UPD) {
        w2[u] = ld_stream<1>(wj + i);
        w1[u] = wm[i];
        x[u] = ld_stream<1>(x2 + i);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (!in[u]) continue;
      if (THREE) {
        if (UNNORM) {
          v[u].x = v[u].x / nu;
          v[u].y = v[u].y / nu;
          y[u].x = y[u].x / nu;
          y[u].y = y[u].y / nu;
          vk[i] = v[u];
        }
        y[u].x = (y[u].x - a * v[u].x) - b * m[u].x;
        y[u].y = (y[u].y - a * v[u].y) - b * m[u].y;
        r2[i] = y[u];  // plain store: the next product reads it
        acc = fma(y[u].x, y[u].x, acc);
        acc = fma(y[u].y, y[u].y, acc);
      }
      if (UPD) {
        double2 w;
        w.x = ((m[u].x - oldeps * w2[u].x) - delta * w1[u].x) / gamma;
        w.y = ((m[u].y - oldeps * w2[u].y) - delta * w1[u].y) / gamma;
        x[u].x = x[u].x + phi * w.x;
        x[u].y = x[u].y + phi * w.y;
        st_stream<1>(wj + i, w);
        st_stream<1>(x2 + i, x[u]);
      }
    }
  }
  if (THREE) {
    acc = block_sum(acc, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
  }
}

// alpha_k = v_k . A v_k - shift from the product's np partials (k_final_sum's grouping); unnorm: the product ran on R = nu v_k
__global__ __launch_bounds__(kTPB) void k_minres_alpha(const double* __restrict__ part, int np, double* __restrict__ ds, const int* __restrict__ di,
                                                      int unnorm) {
  __shared__ double sm16[16];
  if (di[kMrDone]) return;
  double s = final_sum_emulated(part, np, sm16);
  if (threadIdx.x == 0) {
    if (unnorm) {
      const double nu = sqrt(ds[kMrNrm2]);
      s = (s / nu) / nu;
    }
    ds[kMrAlpha] = s - ds[kMrShift];
  }
}

// The end of step k = steps + 1 on the scalars: beta_{k+1}^2 = sum(part[0 .. np)) (k_final_sum's grouping), the rotation in SciPy's sign
// convention, the stopping rule phibar <= rtol beta1 (or a beta_{k+1} that is zero or not finite)
__global__ __launch_bounds__(kTPB) void k_minres_scalars(const double* __restrict__ part, int np, double* __restrict__ ds, int* __restrict__ di,
                                                        double* __restrict__ hist, int hist_cap, double rtol) {
  __shared__ double sm16[16];
  if (di[kMrDone]) return;
  const double nrm2 = final_sum_emulated(part, np, sm16);  // (every thread has read the flag before thread 0 writes it: the barriers inside)
  if (threadIdx.x != 0) return;
  const double eps = 2.220446049250313e-16;
  const double alpha = ds[kMrAlpha], betak = ds[kMrBeta], beta = sqrt(nrm2);
  const double cs0 = ds[kMrCs], sn0 = ds[kMrSn], dbar0 = ds[kMrDbar], phibar0 = ds[kMrPhibar];
  ds[kMrTnorm2] = ds[kMrTnorm2] + ((alpha * alpha + betak * betak) + beta * beta);
  const double oldeps = ds[kMrEpsln];
  const double delta = cs0 * dbar0 + sn0 * alpha;
  const double gbar = sn0 * dbar0 - cs0 * alpha;
  const double epsln = sn0 * beta;
  const double dbar = -cs0 * beta;
  double gamma = hypot(gbar, beta);
  if (!(gamma >= eps)) gamma = gamma != gamma ? gamma : eps;  // max(gamma, eps); a NaN stays one
  const double cs = gbar / gamma, sn = beta / gamma;
  const double phi = cs * phibar0, phibar = sn * phibar0;
  ds[kMrNrm2] = nrm2;
  ds[kMrBeta] = beta;
  ds[kMrCs] = cs;
  ds[kMrSn] = sn;
  ds[kMrDbar] = dbar;
  ds[kMrEpsln] = epsln;
  ds[kMrPhibar] = phibar;
  ds[kMrOldeps] = oldeps;
  ds[kMrDelta] = delta;
  ds[kMrGamma] = gamma;
  ds[kMrPhi] = phi;
  const int k = di[kMrStep] + 1;
  di[kMrStep] = k;
  if (k <= hist_cap) hist[k - 1] = phibar;
  const bool finite = beta - beta == 0.0;
  di[kMrDone] = (!(phibar > rtol * ds[kMrBeta1]) || !(beta > 0.0) || !finite) ? 1 : 0;
}

// r0 = b - (y - shift x0) (y = A x0; y == nullptr: r0 = b) and the partials of |r0|^2
__global__ __launch_bounds__(kTPB) void k_minres_r0(const double* __restrict__ b, const double* __restrict__ y, const double* __restrict__ x0,
                                                   double shift, int64_t n2, double* __restrict__ r, double* __restrict__ part) {
  __shared__ double sm[kTPB / 64];
  const double2* b2 = reinterpret_cast<const double2*>(b);
  const double2* y2 = reinterpret_cast<const double2*>(y);
  const double2* x2 = reinterpret_cast<const double2*>(x0);
  double2* r2 = reinterpret_cast<double2*>(r);
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kTPB + threadIdx.x; i < n2; i += (int64_t)gridDim.x * kTPB) {
    double2 v = b2[i];
    if (y) {
      const double2 yy = y2[i], xx = x2[i];
      v.x = v.x - (yy.x - shift * xx.x);
      v.y = v.y - (yy.y - shift * xx.y);
    }
    r2[i] = v;
    acc = fma(v.x, v.x, acc);
    acc = fma(v.y, v.y, acc);
  }
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

constexpr int kMinresMaxBlocks = 2048;  // k_three_term's grid
static int minres_blocks(int64_t pad) {
  const int64_t g = ((pad >> 1) + kTPB - 1) / kTPB;
  return (int)std::min<int64_t>(std::max<int64_t>(g, 1), kMinresMaxBlocks);
}

namespace api {

void minres_free(lz_handle h) {
  MinresState& m = h->mr;
  big_free(m.vec);
  big_free(m.ds);
  big_free(m.di);
  big_free(m.part);
  big_free(m.hist);
  m = MinresState();
}

}  // namespace api
}  // namespace lz

namespace {

MinresVecs minres_vecs(const MinresState& m) {
  MinresVecs mv;
  mv.V[0] = m.vec;
  mv.V[1] = m.vec + m.ld;
  mv.Y = m.vec + 2 * m.ld;
  mv.R = m.vec + 3 * m.ld;
  mv.W[0] = m.vec + 4 * m.ld;
  mv.W[1] = m.vec + 5 * m.ld;
  mv.X = m.vec + 6 * m.ld;
  return mv;
}

// plan S: the matrix' own SpMV is the ELL-order kernel, which has the scale-on-read form
bool minres_scales(lz_handle h) { return h->kind == 1 && h->csr.ell_default && ell_usable(h->csr, h->flags); }

// partials that the products write (trl_alloc's terms)
size_t minres_product_part(lz_handle h) {
  size_t need = std::max<size_t>((size_t)h->rows / 4 + 64, (size_t)h->csr.n_rowblk + 64);
  if (h->kind == 1 && h->csr.pb) need = std::max<size_t>(need, (size_t)pb_num_partials(h->csr.pb) + 64);
  return need;
}

int minres_alloc(lz_handle h, const char* who) {
  MinresState& m = h->mr;
  if (h->kind == 0) return fail(h, LZ_ERR_STATE, std::string(who) + (h->z.kind != 0 ? ": a complex matrix is set (MINRES takes a real one)" : ": no matrix set"));
  if (h->world > 1 || h->comm_kind != 0) return fail(h, LZ_ERR_STATE, std::string(who) + ": MINRES runs on one rank (this handle has a communicator)");
  if (h->flags & (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE))
    return fail(h, LZ_ERR_STATE, std::string(who) + ": not with LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE");
  if (h->rows < 1 || h->ncols_ext != h->rows) return fail(h, LZ_ERR_STATE, std::string(who) + ": the matrix is not square on this rank");
  LZ_HIP(h, hipSetDevice(h->dev));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  m.live = false;
  const int64_t ld = h->rows_pad;
  if (!m.vec || m.ld != ld) {
    LZ_TRY(dev_alloc(h, m.vec, 7 * (size_t)ld));
    m.ld = ld;
  }
  if (!m.ds) LZ_TRY(dev_alloc(h, m.ds, (size_t)kMinresDoubles));
  if (!m.di) LZ_TRY(dev_alloc(h, m.di, (size_t)kMinresInts));
  const size_t need = minres_product_part(h) + kMinresMaxBlocks;
  if (m.part_cap < need) {
    LZ_TRY(dev_alloc(h, m.part, need));
    m.part_cap = need;
  }
  LZ_HIP(h, hipMemsetAsync(m.vec, 0, 7 * (size_t)ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(m.ds, 0, kMinresDoubles * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(m.di, 0, kMinresInts * sizeof(int), h->stream));
  if (m.hist) LZ_HIP(h, hipMemsetAsync(m.hist, 0, (size_t)m.hist_cap * sizeof(double), h->stream));
  m.steps = 0;
  m.done = 0;
  return LZ_OK;
}

// the history holds at least `count` steps; what it holds is kept
int minres_hist_reserve(lz_handle h, int count) {
  MinresState& m = h->mr;
  if (count <= m.hist_cap) return LZ_OK;
  const int cap = std::max(count, std::max(1024, 2 * m.hist_cap));
  double* p = nullptr;
  LZ_TRY(dev_alloc(h, p, (size_t)cap));
  LZ_HIP(h, hipMemsetAsync(p, 0, (size_t)cap * sizeof(double), h->stream));
  if (m.hist && m.steps > 0) LZ_HIP(h, hipMemcpyAsync(p, m.hist, (size_t)std::min(m.steps, m.hist_cap) * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  LZ_TRY(dev_free(h, m.hist));
  m.hist = p;
  m.hist_cap = cap;
  return LZ_OK;
}

int minres_state(lz_handle h, const char* who) {
  if (!h) return LZ_ERR_ARG;
  const MinresState& m = h->mr;
  if (!m.live || !m.vec) return fail(h, LZ_ERR_STATE, std::string(who) + ": no state (lz_minres_begin first; a new matrix drops it)");
  if (h->kind == 0 || h->rows_pad != m.ld) return fail(h, LZ_ERR_STATE, std::string(who) + ": the matrix changed since lz_minres_begin");
  LZ_HIP(h, hipSetDevice(h->dev));
  return LZ_OK;
}

// y = A x with the x_own . y partials at part; returns their count
int minres_product(lz_handle h, const double* x, double* y, double* part) {
  if (h->kind == 1) return launch_spmv_csr(h->csr, x, y, x, part, h->flags, h->stream);
  return launch_gemv_dense(h->d_dense, h->rows, h->ncols_ext, h->dense_lda, x, x, y, part, h->stream);
}

template <bool THREE, bool UPD>
void launch_minres_step(lz_handle h, bool unnorm, double* part) {
  const MinresState& m = h->mr;
  const int64_t n2 = m.ld >> 1;
  const int grid = minres_blocks(m.ld);
  if (unnorm)
    hipLaunchKernelGGL((k_minres_step<THREE, UPD, true>), dim3(grid), dim3(kTPB), 0, h->stream, minres_vecs(m), m.ds, m.di, n2, part);
  else
    hipLaunchKernelGGL((k_minres_step<THREE, UPD, false>), dim3(grid), dim3(kTPB), 0, h->stream, minres_vecs(m), m.ds, m.di, n2, part);
}

int minres_read_state(lz_handle h, double* state_out) {
  MinresState& m = h->mr;
  double ds[kMinresDoubles];
  int di[kMinresInts];
  LZ_HIP(h, hipMemcpyAsync(ds, m.ds, sizeof(ds), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipMemcpyAsync(di, m.di, sizeof(di), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  m.steps = di[kMrStep];
  m.done = di[kMrDone];
  if (state_out) {
    state_out[0] = (double)m.steps;
    state_out[1] = (double)m.done;
    state_out[2] = ds[kMrPhibar];
    state_out[3] = ds[kMrBeta1];
    state_out[4] = std::sqrt(ds[kMrTnorm2]);
    state_out[5] = ds[kMrAlpha];
    state_out[6] = ds[kMrBeta];
    state_out[7] = ds[kMrPhi];
  }
  return LZ_OK;
}

}  // namespace

extern "C" {

int lz_minres_begin(lz_handle h, const double* b, const double* x0, double shift) {
  if (!h || !b) return LZ_ERR_ARG;
  LZ_TRY(minres_alloc(h, "lz_minres_begin"));
  MinresState& m = h->mr;
  const MinresVecs mv = minres_vecs(m);
  const size_t bytes = (size_t)h->rows * sizeof(double);
  LZ_TRY(upload(h, mv.W[0], b, bytes));  // (b passes through W[0], which is cleared again below)
  double* part_r = m.part + minres_product_part(h);
  const int grid = minres_blocks(m.ld);
  if (x0) {
    LZ_TRY(upload(h, mv.X, x0, bytes));
    minres_product(h, mv.X, mv.Y, m.part);
    LZ_TRY(check_launch(h, "minres begin: product"));
  }
  hipLaunchKernelGGL(k_minres_r0, dim3(grid), dim3(kTPB), 0, h->stream, mv.W[0], x0 ? mv.Y : nullptr, mv.X, shift, m.ld >> 1, mv.R, part_r);
  LZ_TRY(check_launch(h, "minres begin: r0"));
  launch_final_sum(part_r, grid, m.ds + kMrNrm2, h->stream);
  LZ_TRY(check_launch(h, "minres begin: final_sum"));
  LZ_HIP(h, hipMemsetAsync(mv.W[0], 0, (size_t)m.ld * sizeof(double), h->stream));
  double nrm2 = 0.0;
  LZ_HIP(h, hipMemcpyAsync(&nrm2, m.ds + kMrNrm2, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));  // (b and x0 are the caller's)
  const double beta1 = std::sqrt(nrm2);
  double ds[kMinresDoubles] = {0.0};
  ds[kMrNrm2] = nrm2;
  ds[kMrBeta] = beta1;
  ds[kMrCs] = -1.0;
  ds[kMrPhibar] = beta1;
  ds[kMrBeta1] = beta1;
  ds[kMrShift] = shift;
  ds[kMrGamma] = 1.0;
  LZ_HIP(h, hipMemcpyAsync(m.ds, ds, sizeof(ds), hipMemcpyHostToDevice, h->stream));
  m.done = !(beta1 > 0.0) || !std::isfinite(beta1) ? 1 : 0;  // b - (A - shift) x0 = 0: x0 is the solution; a NaN: nothing to iterate on
  const int di[kMinresInts] = {m.done, 0, 0, 0};
  LZ_HIP(h, hipMemcpyAsync(m.di, di, sizeof(di), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  m.live = true;
  return LZ_OK;
}

int lz_minres_run(lz_handle h, int iters, double rtol, double* state_out) {
  LZ_TRY(minres_state(h, "lz_minres_run"));
  MinresState& m = h->mr;
  if (iters < 0 || !(rtol >= 0.0)) return fail(h, LZ_ERR_ARG, "lz_minres_run: need iters >= 0 and rtol >= 0");
  if (m.done || iters == 0) return minres_read_state(h, state_out);
  if ((int64_t)m.steps + iters > INT32_MAX) return fail(h, LZ_ERR_ARG, "lz_minres_run: the step counter is an int");
  LZ_TRY(minres_hist_reserve(h, m.steps + iters));
  const MinresVecs mv = minres_vecs(m);
  const bool scales = minres_scales(h);
  double* part_r = m.part + minres_product_part(h);
  const int grid = minres_blocks(m.ld);
  for (int i = 0; i < iters; ++i) {
    const int k = m.steps + i + 1;  // the device's step while the flag is clear; behind it only Y is written
    int np;
    if (scales) {
      SpmvScale ss;
      ss.r = mv.R;
      ss.nrm2 = m.ds + kMrNrm2;
      ss.vj = mv.V[k & 1];
      ss.beta_slot = m.ds + kMrSpare;
      ss.gate = m.di + kMrDone;  // flag set: a plain Y = A V[k & 1], which stores no v
      np = launch_spmv_ell(h->csr, mv.V[k & 1], mv.Y, mv.V[k & 1], m.part, h->stream, &ss);
    } else {
      np = minres_product(h, mv.R, mv.Y, m.part);
    }
    LZ_TRY(check_launch(h, "minres: product"));
    hipLaunchKernelGGL(k_minres_alpha, dim3(1), dim3(kTPB), 0, h->stream, m.part, np, m.ds, m.di, scales ? 0 : 1);
    LZ_TRY(check_launch(h, "minres: alpha"));
    if (i == 0)
      launch_minres_step<true, false>(h, !scales, part_r);  // (the flush of the last chunk has ended step k - 1)
    else
      launch_minres_step<true, true>(h, !scales, part_r);
    LZ_TRY(check_launch(h, "minres: step"));
    hipLaunchKernelGGL(k_minres_scalars, dim3(1), dim3(kTPB), 0, h->stream, part_r, grid, m.ds, m.di, m.hist, m.hist_cap, rtol);
    LZ_TRY(check_launch(h, "minres: scalars"));
  }
  launch_minres_step<false, true>(h, false, part_r);  // the flush: the state is never lagged between two calls
  LZ_TRY(check_launch(h, "minres: flush"));
  return minres_read_state(h, state_out);
}

int lz_minres_history(lz_handle h, double* out, int count) {
  LZ_TRY(minres_state(h, "lz_minres_history"));
  const MinresState& m = h->mr;
  if (!out || count < 0 || count > m.hist_cap)
    return fail(h, LZ_ERR_ARG, "lz_minres_history: need out and 0 <= count <= the steps lz_minres_run was asked for so far (at least 1024)");
  if (count == 0) return LZ_OK;
  LZ_HIP(h, hipMemcpyAsync(out, m.hist, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_minres_get(lz_handle h, int which, double* out) {
  LZ_TRY(minres_state(h, "lz_minres_get"));
  const MinresState& m = h->mr;
  const bool raw = (which & LZ_MINRES_RAW) != 0;
  const int w = which & ~LZ_MINRES_RAW;
  if (!out || w < 0 || w > LZ_MINRES_R) return fail(h, LZ_ERR_ARG, "lz_minres_get: which is LZ_MINRES_X .. LZ_MINRES_R, with or without LZ_MINRES_RAW");
  const MinresVecs mv = minres_vecs(m);
  const int j = m.steps;  // v_j, w_j are the newest stored; the coming step is k = j + 1
  const double* src = w == LZ_MINRES_X ? mv.X : w == LZ_MINRES_VPREV ? mv.V[j & 1] : w == LZ_MINRES_W1 ? mv.W[j & 1] : w == LZ_MINRES_W2 ? mv.W[(j + 1) & 1] : mv.R;
  const size_t count = raw ? (size_t)m.ld : (size_t)h->rows;
  LZ_HIP(h, hipMemcpyAsync(out, src, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  double nrm2 = 1.0;
  if (w == LZ_MINRES_V) LZ_HIP(h, hipMemcpyAsync(&nrm2, m.ds + kMrNrm2, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  if (w == LZ_MINRES_V) {  // v_k is formed on read: R / nu, the division the kernels do
    const double nu = std::sqrt(nrm2);
    for (size_t i = 0; i < count; ++i) out[i] = out[i] / nu;
  }
  return LZ_OK;
}

int lz_minres_set_state(lz_handle h, int k, const double* x, const double* vk, const double* vkm1, const double* wkm1, const double* wkm2,
                        const double* scalars) {
  if (!h || !x || !vk || !vkm1 || !wkm1 || !wkm2 || !scalars) return LZ_ERR_ARG;
  if (k < 1) return fail(h, LZ_ERR_ARG, "lz_minres_set_state: need k >= 1");
  LZ_TRY(minres_alloc(h, "lz_minres_set_state"));
  MinresState& m = h->mr;
  LZ_TRY(minres_hist_reserve(h, k));
  const MinresVecs mv = minres_vecs(m);
  const size_t bytes = (size_t)h->rows * sizeof(double);
  const int j = k - 1;
  LZ_TRY(upload(h, mv.X, x, bytes));
  LZ_TRY(upload(h, mv.R, vk, bytes));
  LZ_TRY(upload(h, mv.V[j & 1], vkm1, bytes));
  LZ_TRY(upload(h, mv.W[j & 1], wkm1, bytes));
  LZ_TRY(upload(h, mv.W[(j + 1) & 1], wkm2, bytes));
  double ds[kMinresDoubles] = {0.0};
  ds[kMrNrm2] = 1.0;  // v_k is taken as it is given
  ds[kMrBeta] = scalars[0];
  ds[kMrCs] = scalars[1];
  ds[kMrSn] = scalars[2];
  ds[kMrDbar] = scalars[3];
  ds[kMrEpsln] = scalars[4];
  ds[kMrPhibar] = scalars[5];
  ds[kMrTnorm2] = scalars[6];
  ds[kMrBeta1] = scalars[7];
  ds[kMrShift] = scalars[8];
  ds[kMrGamma] = 1.0;
  const int di[kMinresInts] = {0, j, 0, 0};
  LZ_HIP(h, hipMemcpyAsync(m.ds, ds, sizeof(ds), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipMemcpyAsync(m.di, di, sizeof(di), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));  // (the sources are the caller's and this frame's)
  m.steps = j;
  m.done = 0;
  m.live = true;
  return LZ_OK;
}

int lz_minres_step_time(lz_handle h, int reps, double* ms_out) {
  LZ_TRY(minres_state(h, "lz_minres_step_time"));
  MinresState& m = h->mr;
  if (!ms_out || reps < 1) return fail(h, LZ_ERR_ARG, "lz_minres_step_time: need reps >= 1 and ms_out");
  if (m.done) return fail(h, LZ_ERR_STATE, "lz_minres_step_time: the state is done (its gated kernels would return at once)");
  const MinresVecs mv = minres_vecs(m);
  const bool scales = minres_scales(h);
  double* part_r = m.part + minres_product_part(h);
  const int k = m.steps + 1;
  SpmvScale ss;
  ss.r = mv.R;
  ss.nrm2 = m.ds + kMrNrm2;
  ss.vj = mv.V[k & 1];
  ss.beta_slot = m.ds + kMrSpare;
  ss.gate = m.di + kMrDone;
  hipEvent_t a, b;
  LZ_HIP(h, hipEventCreate(&a));
  LZ_HIP(h, hipEventCreate(&b));
  hipError_t err = hipSuccess;
  for (int what = 0; what < 2 && err == hipSuccess; ++what) {
    for (int r = -1; r < reps; ++r) {  // (r == -1: the warm-up)
      if (r == 0) err = hipEventRecord(a, h->stream);
      if (what == 0 && scales)
        launch_spmv_ell(h->csr, mv.V[k & 1], mv.Y, mv.V[k & 1], m.part, h->stream, &ss);
      else if (what == 0)
        minres_product(h, mv.R, mv.Y, m.part);
      else
        launch_minres_step<true, true>(h, !scales, part_r);
    }
    if (err == hipSuccess) err = hipEventRecord(b, h->stream);
    if (err == hipSuccess) err = hipEventSynchronize(b);
    float ms = 0.f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, a, b);
    ms_out[what] = (double)ms / reps;
  }
  hipEventDestroy(a);
  hipEventDestroy(b);
  m.live = false;  // (the repeated pass has been applied to r, w and x again and again)
  LZ_HIP(h, err);
  return check_launch(h, "minres step time");
}

int lz_minres_info(lz_handle h, int* out) {
  if (!h || !out) return LZ_ERR_ARG;
  out[0] = 4;  // product, k_minres_alpha, k_minres_step, k_minres_scalars
  out[1] = minres_scales(h) ? 1 : 0;
  out[2] = h->mr.live && h->kind != 0 && h->rows_pad == h->mr.ld ? 1 : 0;
  return LZ_OK;
}

}  // extern "C"
