// LSMR (include/lanczos_hip.h, "least-squares solves"): the device half of lanczos_amd.lsmr, min |A x - b|^2 + damp^2 |x|^2 for a
// rectangular or non-symmetric A (Fong & Saunders 2011).  Golub-Kahan bidiagonalisation without a basis, and MINRES on the normal
// equations done implicitly: SciPy's lsmr scalar for scalar.  The products are the rectangular operator's (gk_product), untouched;
// what is new here is the vector side.  u and v are never normalised by a pass: the device holds UH = beta_k u_k and VH = alpha_k v_k
// with the numbers to divide by (nu_u, nu_v), the products run on UH and VH as they are, and every kernel divides where it reads.
//   k_lsmr_u        one streaming pass over b's length behind y = A VH: UH = y / nu_v - alpha_k (UH / nu_u) with the fixed-order
//                   partials of |UH|^2.  24 B a row.
//   k_lsmr_beta     one block: beta_{k+1} from those partials.
//   k_lsmr_v        one streaming pass over x's length behind z = A^T UH: VH = z / nu_u - beta_{k+1} (VH / nu_v) with the partials of
//                   |VH|^2 and, from the same load of VH, the END of step k - 1: hbar = h - c1 hbar, x += c2 hbar, h = v_k - c3 h with
//                   the partials of |x|^2 - c1, c2, c3 depend on alpha_k, which step k - 1 knew only behind its own pass.  The update
//                   lags one step; the same kernel with the three-term switched off (the flush) applies the pending one when a call
//                   ends.  72 B a row (reads z, VH, h, hbar, x; writes VH, h, hbar, x); the unfused form moves 120.
//   k_lsmr_scalars  one block: alpha_{k+1}, |x_{k-1}|, the rotations, the estimates of |r|, |A^T r|, |A|, cond(A), the scalars of the
//                   next lagged update, the history, the step counter, istop and the done flag.
// Every kernel here but the flush reads the done flag first and returns at once when it is set, so a chunk of iterations is enqueued
// with no host synchronisation; the products of the rest of the chunk run on (their output goes to Y and Z, which nothing reads
// then).  Launches of its own per iteration: 4, beside the two products.  No atomics: the same input gives the same bits.
#include "lz_context.h"
#include "lz_device.h"

using namespace lz;
using namespace lz::api;

namespace lz {

// ds: the scalars on the device.  [0, 24) in the order of lz_lsmr_set_state's scalars
enum LsmrD {
  kLsAlpha = 0,
  kLsBeta,
  kLsAlphabar,
  kLsRho,
  kLsRhobar,
  kLsCbar,
  kLsSbar,
  kLsZeta,
  kLsZetabar,
  kLsBetadd,
  kLsBetad,
  kLsRhodold,
  kLsTautildeold,
  kLsThetatilde,
  kLsD,
  kLsNormA2,
  kLsMaxrbar,
  kLsMinrbar,
  kLsDamp,
  kLsNormb,
  kLsC1,  // the lagged update's scalars, written by step j's k_lsmr_scalars, read by the next k_lsmr_v
  kLsC2,
  kLsC3,
  kLsSpare,
  kLsNuU,  // u_k = UH / nu_u: beta_k, or 1 where beta_k is zero (UH is the zero vector then) and behind lz_lsmr_set_state
  kLsNuV,  // v_k = VH / nu_v likewise
  kLsNormr,
  kLsNormar,
  kLsNormA,
  kLsCondA,
  kLsNormxLag,  // |x_{k-1}| as the tests of step k saw it
  kLsNormx2,    // |x|^2 of the x now held (the flush's partials)
  kLsSum,       // lz_lsmr_begin's two sums
  kLsSum2,
  kLsmrDoubles = 40
};
enum LsmrI { kLsDone = 0, kLsStep, kLsIstop, kLsFresh, kLsmrInts = 4 };  // fresh: an update is pending (the flush applies it once)

struct LsmrVecs {
  double *UH, *Y;              // b's length
  double *VH, *Z, *H, *HBAR, *X;  // x's length
};

// UH = y / nu_v - alpha (UH / nu_u), part[b] = block b's share of |UH|^2.  Grid-stride over 16-byte positions, two positions of a lane
// in flight, the partial accumulated in the order of the positions (k_minres_step's shape).
__global__ __launch_bounds__(kTPB) void k_lsmr_u(double* __restrict__ uh, const double* __restrict__ yv, const double* __restrict__ ds,
                                                const int* __restrict__ di, int64_t n2, double* __restrict__ part) {
  __shared__ double sm[kTPB / 64];
  if (di[kLsDone]) return;
  double2* u2 = reinterpret_cast<double2*>(uh);
  const double2* y2 = reinterpret_cast<const double2*>(yv);
  const double alpha = ds[kLsAlpha], nu_u = ds[kLsNuU], nu_v = ds[kLsNuV];
  double acc = 0.0;
  constexpr int U = 2;
  const int64_t stride = (int64_t)gridDim.x * kTPB;
  for (int64_t i0 = (int64_t)blockIdx.x * kTPB + threadIdx.x; i0 < n2; i0 += U * stride) {
    double2 y[U], u[U];
    bool in[U];
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int64_t i = i0 + q * stride;
      in[q] = i < n2;
      if (!in[q]) continue;
      y[q] = ld_stream<1>(y2 + i);
      u[q] = u2[i];
    }
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int64_t i = i0 + q * stride;
      if (!in[q]) continue;
      u[q].x = y[q].x / nu_v - alpha * (u[q].x / nu_u);
      u[q].y = y[q].y / nu_v - alpha * (u[q].y / nu_u);
      u2[i] = u[q];  // plain store: the next product reads it
      acc = fma(u[q].x, u[q].x, acc);
      acc = fma(u[q].y, u[q].y, acc);
    }
  }
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// beta_{k+1} = sqrt(sum(part[0 .. np))) (k_final_sum's grouping).  Zero: SciPy's branch - u stays the zero vector it is, and
// k_lsmr_v leaves v and alpha alone.  Not finite: the done flag, with the state as it is.
__global__ __launch_bounds__(kTPB) void k_lsmr_beta(const double* __restrict__ part, int np, double* __restrict__ ds, int* __restrict__ di) {
  __shared__ double sm16[16];
  if (di[kLsDone]) return;
  const double s = final_sum_emulated(part, np, sm16);  // (every thread has read the flag before thread 0 writes it: the barriers inside)
  if (threadIdx.x != 0) return;
  const double beta = sqrt(s);
  if (beta - beta == 0.0) {
    ds[kLsBeta] = beta;
    ds[kLsNuU] = beta > 0.0 ? beta : 1.0;
  } else {
    di[kLsDone] = 1;
    di[kLsIstop] = -1;
  }
}

// THREE: VH = z / nu_u - beta (VH / nu_v) behind the product z = A^T UH of step k, pv[b] = block b's share of |VH|^2 (not where beta
// is zero: v stays); UPD: the end of step k - 1 from the same load of VH, px[b] = block b's share of |x|^2.  <false, true> is the flush.
template <bool THREE, bool UPD>
__global__ __launch_bounds__(kTPB) void k_lsmr_v(LsmrVecs lv, const double* __restrict__ ds, const int* __restrict__ di, int64_t n2,
                                                double* __restrict__ pv, double* __restrict__ px) {
  __shared__ double sm[kTPB / 64];
  if (THREE && di[kLsDone]) return;  // (the flush is not gated on the flag: it ends the step that set it)
  if (!THREE && !di[kLsFresh]) return;  // ... but it applies an update once only
  double2* v2 = reinterpret_cast<double2*>(lv.VH);
  const double2* z2 = reinterpret_cast<const double2*>(lv.Z);
  double2* h2 = reinterpret_cast<double2*>(lv.H);
  double2* hb2 = reinterpret_cast<double2*>(lv.HBAR);
  double2* x2 = reinterpret_cast<double2*>(lv.X);
  const double beta = ds[kLsBeta], nu_u = ds[kLsNuU], nu_v = ds[kLsNuV];
  const bool three = THREE && beta > 0.0;
  double c1 = 0.0, c2 = 0.0, c3 = 0.0;
  if (UPD) {
    c1 = ds[kLsC1];
    c2 = ds[kLsC2];
    c3 = ds[kLsC3];
  }
  double accv = 0.0, accx = 0.0;
  constexpr int U = 2;
  const int64_t stride = (int64_t)gridDim.x * kTPB;
  for (int64_t i0 = (int64_t)blockIdx.x * kTPB + threadIdx.x; i0 < n2; i0 += U * stride) {
    double2 v[U], z[U], hh[U], hb[U], x[U];
    bool in[U];
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int64_t i = i0 + q * stride;
      in[q] = i < n2;
      if (!in[q]) continue;
      v[q] = v2[i];
      if (three) z[q] = ld_stream<1>(z2 + i);
      if (UPD) {
        hh[q] = ld_stream<1>(h2 + i);
        hb[q] = ld_stream<1>(hb2 + i);
        x[q] = ld_stream<1>(x2 + i);
      }
    }
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int64_t i = i0 + q * stride;
      if (!in[q]) continue;
      double2 vk;  // v_k
      vk.x = v[q].x / nu_v;
      vk.y = v[q].y / nu_v;
      if (three) {
        double2 vn;
        vn.x = z[q].x / nu_u - beta * vk.x;
        vn.y = z[q].y / nu_u - beta * vk.y;
        v2[i] = vn;  // plain store: the next product reads it
        accv = fma(vn.x, vn.x, accv);
        accv = fma(vn.y, vn.y, accv);
      }
      if (UPD) {
        double2 b, hn;
        b.x = hh[q].x - c1 * hb[q].x;
        b.y = hh[q].y - c1 * hb[q].y;
        x[q].x = x[q].x + c2 * b.x;
        x[q].y = x[q].y + c2 * b.y;
        hn.x = vk.x - c3 * hh[q].x;
        hn.y = vk.y - c3 * hh[q].y;
        st_stream<1>(hb2 + i, b);
        st_stream<1>(x2 + i, x[q]);
        st_stream<1>(h2 + i, hn);
        accx = fma(x[q].x, x[q].x, accx);
        accx = fma(x[q].y, x[q].y, accx);
      }
    }
  }
  if (THREE) {
    accv = block_sum(accv, sm);
    if (threadIdx.x == 0) pv[blockIdx.x] = accv;
  }
  if (UPD) {
    accx = block_sum(accx, sm);
    if (threadIdx.x == 0) px[blockIdx.x] = accx;
  }
}

// SciPy's _sym_ortho: the stable Givens rotation, with numpy.sign's sign (0 for 0)
__device__ __forceinline__ double lsmr_sign(double a) { return a > 0.0 ? 1.0 : a < 0.0 ? -1.0 : a; }
__device__ __forceinline__ void lsmr_sym_ortho(double a, double b, double& c, double& s, double& r) {
  if (b == 0.0) {
    c = lsmr_sign(a), s = 0.0, r = fabs(a);
  } else if (a == 0.0) {
    c = 0.0, s = lsmr_sign(b), r = fabs(b);
  } else if (fabs(b) > fabs(a)) {
    const double tau = a / b;
    s = lsmr_sign(b) / sqrt(1.0 + tau * tau);
    c = s * tau;
    r = b / s;
  } else {
    const double tau = b / a;
    c = lsmr_sign(a) / sqrt(1.0 + tau * tau);
    s = c * tau;
    r = a / c;
  }
}

// The end of step k = steps + 1 on the scalars: alpha_{k+1}^2 = sum(pv[0 .. np)) where beta_{k+1} > 0, |x_{k-1}|^2 = sum(px[0 .. np))
// (k_final_sum's grouping), then the body of SciPy's loop behind its two products
__global__ __launch_bounds__(kTPB) void k_lsmr_scalars(const double* __restrict__ pv, const double* __restrict__ px, int np, double* __restrict__ ds,
                                                      int* __restrict__ di, double* __restrict__ hist, int hist_cap, double atol, double btol,
                                                      double ctol) {
  __shared__ double sm16[16], sm16x[16];
  if (di[kLsDone]) return;
  const double sv = final_sum_emulated(pv, np, sm16);  // (every thread has read the flag before thread 0 writes it: the barriers inside)
  const double sx = final_sum_emulated(px, np, sm16x);
  if (threadIdx.x != 0) return;
  const double beta = ds[kLsBeta], damp = ds[kLsDamp], normb = ds[kLsNormb];
  double alpha = ds[kLsAlpha];
  if (beta > 0.0) {
    alpha = sqrt(sv);
    if (!(alpha - alpha == 0.0)) {
      di[kLsDone] = 1;
      di[kLsIstop] = -1;
      return;
    }
    ds[kLsAlpha] = alpha;
    ds[kLsNuV] = alpha > 0.0 ? alpha : 1.0;
  }
  const int itn = di[kLsStep] + 1;
  double chat, shat, alphahat, c, s, rho;
  lsmr_sym_ortho(ds[kLsAlphabar], damp, chat, shat, alphahat);
  const double rhoold = ds[kLsRho];
  lsmr_sym_ortho(alphahat, beta, c, s, rho);
  const double thetanew = s * alpha;
  const double alphabar = c * alpha;
  const double rhobarold = ds[kLsRhobar], zetaold = ds[kLsZeta];
  const double cbar0 = ds[kLsCbar], sbar0 = ds[kLsSbar];
  const double thetabar = sbar0 * rho;
  const double rhotemp = cbar0 * rho;
  double cbar, sbar, rhobar;
  lsmr_sym_ortho(cbar0 * rho, thetanew, cbar, sbar, rhobar);
  const double zetabar0 = ds[kLsZetabar];
  const double zeta = cbar * zetabar0;
  const double zetabar = -sbar * zetabar0;
  // the update of h, hbar, x that the next pass applies
  ds[kLsC1] = thetabar * rho / (rhoold * rhobarold);
  ds[kLsC2] = zeta / (rho * rhobar);
  ds[kLsC3] = thetanew / rho;
  // the estimate of |r|
  const double betadd0 = ds[kLsBetadd];
  const double betaacute = chat * betadd0;
  const double betacheck = -shat * betadd0;
  const double betahat = c * betaacute;
  const double betadd = -s * betaacute;
  const double thetatildeold = ds[kLsThetatilde];
  double ctildeold, stildeold, rhotildeold;
  lsmr_sym_ortho(ds[kLsRhodold], thetabar, ctildeold, stildeold, rhotildeold);
  const double thetatilde = stildeold * rhobar;
  const double rhodold = ctildeold * rhobar;
  const double betad = -stildeold * ds[kLsBetad] + ctildeold * betahat;
  const double tautildeold = (zetaold - thetatildeold * ds[kLsTautildeold]) / rhotildeold;
  const double taud = (zeta - thetatilde * tautildeold) / rhodold;
  const double d = ds[kLsD] + betacheck * betacheck;
  const double normr = sqrt(d + (betad - taud) * (betad - taud) + betadd * betadd);
  // |A| and cond(A)
  double normA2 = ds[kLsNormA2] + beta * beta;
  const double normA = sqrt(normA2);
  normA2 = normA2 + alpha * alpha;
  const double maxrbar = fmax(ds[kLsMaxrbar], rhobarold);
  double minrbar = ds[kLsMinrbar];
  if (itn > 1) minrbar = fmin(minrbar, rhobarold);
  const double condA = fmax(maxrbar, rhotemp) / fmin(minrbar, rhotemp);
  // the tests, on |x_{k-1}|
  const double normar = fabs(zetabar);
  const double normx = sqrt(sx);
  const double test1 = normr / normb;
  const double test2 = normA * normr != 0.0 ? normar / (normA * normr) : INFINITY;
  const double test3 = 1.0 / condA;
  const double t1 = test1 / (1.0 + normA * normx / normb);
  const double rtol = btol + atol * normA * normx / normb;
  int istop = 0;
  if (1.0 + test3 <= 1.0) istop = 6;
  if (1.0 + test2 <= 1.0) istop = 5;
  if (1.0 + t1 <= 1.0) istop = 4;
  if (test3 <= ctol) istop = 3;
  if (test2 <= atol) istop = 2;
  if (test1 <= rtol) istop = 1;
  ds[kLsAlphabar] = alphabar;
  ds[kLsRho] = rho;
  ds[kLsRhobar] = rhobar;
  ds[kLsCbar] = cbar;
  ds[kLsSbar] = sbar;
  ds[kLsZeta] = zeta;
  ds[kLsZetabar] = zetabar;
  ds[kLsBetadd] = betadd;
  ds[kLsBetad] = betad;
  ds[kLsRhodold] = rhodold;
  ds[kLsTautildeold] = tautildeold;
  ds[kLsThetatilde] = thetatilde;
  ds[kLsD] = d;
  ds[kLsNormA2] = normA2;
  ds[kLsMaxrbar] = maxrbar;
  ds[kLsMinrbar] = minrbar;
  ds[kLsNormr] = normr;
  ds[kLsNormar] = normar;
  ds[kLsNormA] = normA;
  ds[kLsCondA] = condA;
  ds[kLsNormxLag] = normx;
  di[kLsStep] = itn;
  if (itn <= hist_cap) {
    hist[2 * (int64_t)(itn - 1)] = normr;
    hist[2 * (int64_t)(itn - 1) + 1] = normar;
  }
  di[kLsFresh] = 1;
  di[kLsIstop] = istop;
  di[kLsDone] = istop != 0 ? 1 : 0;
}

// u = b - y in place of b (y == nullptr: u = b) with the partials of |u|^2 at pu and of |b|^2 at pb
__global__ __launch_bounds__(kTPB) void k_lsmr_r0(double* __restrict__ u, const double* __restrict__ y, int64_t n2, double* __restrict__ pu,
                                                 double* __restrict__ pb) {
  __shared__ double sm[kTPB / 64];
  double2* u2 = reinterpret_cast<double2*>(u);
  const double2* y2 = reinterpret_cast<const double2*>(y);
  double au = 0.0, ab = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kTPB + threadIdx.x; i < n2; i += (int64_t)gridDim.x * kTPB) {
    double2 v = u2[i];
    ab = fma(v.x, v.x, ab);
    ab = fma(v.y, v.y, ab);
    if (y) {
      const double2 yy = y2[i];
      v.x = v.x - yy.x;
      v.y = v.y - yy.y;
      u2[i] = v;
    }
    au = fma(v.x, v.x, au);
    au = fma(v.y, v.y, au);
  }
  au = block_sum(au, sm);
  ab = block_sum(ab, sm);
  if (threadIdx.x == 0) {
    pu[blockIdx.x] = au;
    pb[blockIdx.x] = ab;
  }
}

constexpr int kLsmrMaxBlocks = 2048;  // k_minres_step's grid
static int lsmr_blocks(int64_t pad) {
  const int64_t g = ((pad >> 1) + kTPB - 1) / kTPB;
  return (int)std::min<int64_t>(std::max<int64_t>(g, 1), kLsmrMaxBlocks);
}

namespace api {

void lsmr_free(lz_handle h) {
  LsmrState& m = h->ls;
  big_free(m.bvec);
  big_free(m.xvec);
  big_free(m.ds);
  big_free(m.di);
  big_free(m.part);
  big_free(m.hist);
  m = LsmrState();
}

}  // namespace api
}  // namespace lz

namespace {

LsmrVecs lsmr_vecs(const LsmrState& m) {
  LsmrVecs lv;
  lv.UH = m.bvec;
  lv.Y = m.bvec + m.bpad;
  lv.VH = m.xvec;
  lv.Z = m.xvec + m.xpad;
  lv.H = m.xvec + 2 * m.xpad;
  lv.HBAR = m.xvec + 3 * m.xpad;
  lv.X = m.xvec + 4 * m.xpad;
  return lv;
}

// the partials: |u|^2, |v|^2, |x|^2 and lz_lsmr_begin's |b|^2
double* lsmr_part(const LsmrState& m, int which) { return m.part + (size_t)which * kLsmrMaxBlocks; }

int lsmr_alloc(lz_handle h, int transposed, const char* who) {
  LsmrState& m = h->ls;
  if (!h->gk.set) return fail(h, LZ_ERR_STATE, std::string(who) + ": no rectangular matrix (lz_gk_set_csr or lz_gk_set_dense first)");
  if (h->world > 1 || h->comm_kind != 0) return fail(h, LZ_ERR_STATE, std::string(who) + ": LSMR runs on one rank (this handle has a communicator)");
  if (h->flags & (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE))
    return fail(h, LZ_ERR_STATE, std::string(who) + ": not with LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE");
  if (transposed != 0 && transposed != 1) return fail(h, LZ_ERR_ARG, std::string(who) + ": transposed is 0 or 1");
  LZ_HIP(h, hipSetDevice(h->dev));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  m.live = false;
  const GkState& g = h->gk;
  const int64_t blen = transposed ? g.V.len : g.U.len, xlen = transposed ? g.U.len : g.V.len;
  const int64_t bpad = round_up(blen, kPadDoubles), xpad = round_up(xlen, kPadDoubles);
  if (!m.bvec || m.bpad != bpad) LZ_TRY(dev_alloc(h, m.bvec, 2 * (size_t)bpad));
  if (!m.xvec || m.xpad != xpad) LZ_TRY(dev_alloc(h, m.xvec, 5 * (size_t)xpad));
  m.blen = blen, m.bpad = bpad, m.xlen = xlen, m.xpad = xpad;
  m.transposed = transposed;
  if (!m.ds) LZ_TRY(dev_alloc(h, m.ds, (size_t)kLsmrDoubles));
  if (!m.di) LZ_TRY(dev_alloc(h, m.di, (size_t)kLsmrInts));
  if (!m.part) LZ_TRY(dev_alloc(h, m.part, 4 * (size_t)kLsmrMaxBlocks));
  LZ_HIP(h, hipMemsetAsync(m.bvec, 0, 2 * (size_t)bpad * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(m.xvec, 0, 5 * (size_t)xpad * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(m.ds, 0, kLsmrDoubles * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(m.di, 0, kLsmrInts * sizeof(int), h->stream));
  LZ_HIP(h, hipMemsetAsync(m.part, 0, 4 * (size_t)kLsmrMaxBlocks * sizeof(double), h->stream));
  if (m.hist) LZ_HIP(h, hipMemsetAsync(m.hist, 0, 2 * (size_t)m.hist_cap * sizeof(double), h->stream));
  m.steps = 0;
  m.done = 0;
  m.pending = false;
  return LZ_OK;
}

// the history holds at least `count` steps; what it holds is kept
int lsmr_hist_reserve(lz_handle h, int count) {
  LsmrState& m = h->ls;
  if (count <= m.hist_cap) return LZ_OK;
  const int cap = std::max(count, std::max(1024, 2 * m.hist_cap));
  double* p = nullptr;
  LZ_TRY(dev_alloc(h, p, 2 * (size_t)cap));
  LZ_HIP(h, hipMemsetAsync(p, 0, 2 * (size_t)cap * sizeof(double), h->stream));
  if (m.hist && m.steps > 0)
    LZ_HIP(h, hipMemcpyAsync(p, m.hist, 2 * (size_t)std::min(m.steps, m.hist_cap) * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  LZ_TRY(dev_free(h, m.hist));
  m.hist = p;
  m.hist_cap = cap;
  return LZ_OK;
}

int lsmr_state(lz_handle h, const char* who) {
  if (!h) return LZ_ERR_ARG;
  const LsmrState& m = h->ls;
  if (!m.live || !m.bvec || !m.xvec || !h->gk.set)
    return fail(h, LZ_ERR_STATE, std::string(who) + ": no state (lz_lsmr_begin first; lz_gk_set_csr / lz_gk_set_dense drop it)");
  LZ_HIP(h, hipSetDevice(h->dev));
  return LZ_OK;
}

// y = A v (b's length) and z = A^T u (x's length); A is the gk matrix or, with transposed, its transpose
hipError_t lsmr_product_av(lz_handle h, const double* v, double* y) { return gk_product(h, h->ls.transposed ? 1 : 0, v, y, h->ls.bpad); }
hipError_t lsmr_product_atu(lz_handle h, const double* u, double* z) { return gk_product(h, h->ls.transposed ? 0 : 1, u, z, h->ls.xpad); }

template <bool THREE, bool UPD>
void launch_lsmr_v(lz_handle h) {
  const LsmrState& m = h->ls;
  hipLaunchKernelGGL((k_lsmr_v<THREE, UPD>), dim3(lsmr_blocks(m.xpad)), dim3(kTPB), 0, h->stream, lsmr_vecs(m), m.ds, m.di, m.xpad >> 1,
                     lsmr_part(m, 1), lsmr_part(m, 2));
}

void launch_lsmr_u(lz_handle h) {
  const LsmrState& m = h->ls;
  const LsmrVecs lv = lsmr_vecs(m);
  hipLaunchKernelGGL(k_lsmr_u, dim3(lsmr_blocks(m.bpad)), dim3(kTPB), 0, h->stream, lv.UH, lv.Y, m.ds, m.di, m.bpad >> 1, lsmr_part(m, 0));
}

int lsmr_read_state(lz_handle h, double* state_out) {
  LsmrState& m = h->ls;
  double ds[kLsmrDoubles];
  int di[kLsmrInts];
  LZ_HIP(h, hipMemcpyAsync(ds, m.ds, sizeof(ds), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipMemcpyAsync(di, m.di, sizeof(di), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  m.steps = di[kLsStep];
  m.done = di[kLsDone];
  if (state_out) {
    state_out[0] = (double)m.steps;
    state_out[1] = (double)m.done;
    state_out[2] = di[kLsIstop] < 0 ? 7.0 : (double)di[kLsIstop];
    state_out[3] = ds[kLsNormr];
    state_out[4] = ds[kLsNormar];
    state_out[5] = ds[kLsNormA];
    state_out[6] = ds[kLsCondA];
    state_out[7] = std::sqrt(ds[kLsNormx2]);
    state_out[8] = ds[kLsAlpha];
    state_out[9] = ds[kLsBeta];
    state_out[10] = ds[kLsRho];
    state_out[11] = ds[kLsRhobar];
    state_out[12] = ds[kLsZeta];
    state_out[13] = ds[kLsZetabar];
    state_out[14] = ds[kLsNormxLag];
    state_out[15] = ds[kLsNormb];
  }
  return LZ_OK;
}

}  // namespace

extern "C" {

int lz_lsmr_begin(lz_handle h, int transposed, const double* b, const double* x0, double damp) {
  if (!h || !b) return LZ_ERR_ARG;
  if (!(damp >= 0.0)) return fail(h, LZ_ERR_ARG, "lz_lsmr_begin: need damp >= 0");
  LZ_TRY(lsmr_alloc(h, transposed, "lz_lsmr_begin"));
  LsmrState& m = h->ls;
  const LsmrVecs lv = lsmr_vecs(m);
  LZ_TRY(upload(h, lv.UH, b, (size_t)m.blen * sizeof(double)));
  if (x0) {
    LZ_TRY(upload(h, lv.X, x0, (size_t)m.xlen * sizeof(double)));
    LZ_HIP(h, lsmr_product_av(h, lv.X, lv.Y));
    LZ_TRY(check_launch(h, "lsmr begin: product"));
  }
  const int gb = lsmr_blocks(m.bpad), gx = lsmr_blocks(m.xpad);
  hipLaunchKernelGGL(k_lsmr_r0, dim3(gb), dim3(kTPB), 0, h->stream, lv.UH, x0 ? lv.Y : nullptr, m.bpad >> 1, lsmr_part(m, 0), lsmr_part(m, 3));
  LZ_TRY(check_launch(h, "lsmr begin: r0"));
  launch_final_sum(lsmr_part(m, 0), gb, m.ds + kLsSum, h->stream);
  launch_final_sum(lsmr_part(m, 3), gb, m.ds + kLsSum2, h->stream);
  LZ_TRY(check_launch(h, "lsmr begin: final_sum"));
  double sums[2] = {0.0, 0.0};
  LZ_HIP(h, hipMemcpyAsync(sums, m.ds + kLsSum, sizeof(sums), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));  // (b and x0 are the caller's)
  const double beta = std::sqrt(sums[0]), normb = std::sqrt(sums[1]);
  double alpha = 0.0;
  double ds[kLsmrDoubles] = {0.0};
  ds[kLsBeta] = beta;
  ds[kLsNuU] = beta > 0.0 ? beta : 1.0;
  ds[kLsNuV] = 1.0;
  if (beta > 0.0 && std::isfinite(beta)) {  // VH = A^T UH / beta_1: the three-term on VH = 0
    LZ_HIP(h, hipMemcpyAsync(m.ds, ds, sizeof(ds), hipMemcpyHostToDevice, h->stream));
    LZ_HIP(h, lsmr_product_atu(h, lv.UH, lv.Z));
    LZ_TRY(check_launch(h, "lsmr begin: transposed product"));
    launch_lsmr_v<true, false>(h);
    LZ_TRY(check_launch(h, "lsmr begin: v"));
    launch_final_sum(lsmr_part(m, 1), gx, m.ds + kLsSum, h->stream);
    LZ_TRY(check_launch(h, "lsmr begin: final_sum"));
    LZ_HIP(h, hipMemcpyAsync(sums, m.ds + kLsSum, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    LZ_HIP(h, hipStreamSynchronize(h->stream));
    alpha = std::sqrt(sums[0]);
  }
  ds[kLsAlpha] = alpha;
  ds[kLsNuV] = alpha > 0.0 ? alpha : 1.0;
  ds[kLsAlphabar] = alpha;
  ds[kLsRho] = 1.0;
  ds[kLsRhobar] = 1.0;
  ds[kLsCbar] = 1.0;
  ds[kLsZetabar] = alpha * beta;
  ds[kLsBetadd] = beta;
  ds[kLsRhodold] = 1.0;
  ds[kLsNormA2] = alpha * alpha;
  ds[kLsMinrbar] = 1e100;
  ds[kLsDamp] = damp;
  ds[kLsNormb] = normb;
  ds[kLsNormr] = beta;
  ds[kLsNormar] = alpha * beta;
  ds[kLsNormA] = std::sqrt(alpha * alpha);
  ds[kLsCondA] = 1.0;
  const double normar = alpha * beta;
  const bool finite = std::isfinite(beta) && std::isfinite(alpha) && std::isfinite(normb);
  m.done = (!finite || normar == 0.0 || normb == 0.0) ? 1 : 0;  // x0 (or 0) is the answer; a NaN: nothing to iterate on
  const int di[kLsmrInts] = {m.done, 0, finite ? 0 : -1, 1};  // the pending update is c = (0, 0, 0) on h = hbar = 0: it makes h_1 = v_1
  LZ_HIP(h, hipMemcpyAsync(m.ds, ds, sizeof(ds), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipMemcpyAsync(m.di, di, sizeof(di), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  m.pending = true;
  m.live = true;
  return LZ_OK;
}

int lz_lsmr_run(lz_handle h, int iters, double atol, double btol, double conlim, double* state_out) {
  LZ_TRY(lsmr_state(h, "lz_lsmr_run"));
  LsmrState& m = h->ls;
  if (iters < 0 || !(atol >= 0.0) || !(btol >= 0.0) || conlim != conlim)
    return fail(h, LZ_ERR_ARG, "lz_lsmr_run: need iters >= 0, atol >= 0, btol >= 0 and a conlim that is a number");
  if (m.done || iters == 0) return lsmr_read_state(h, state_out);
  if ((int64_t)m.steps + iters > INT32_MAX / 2) return fail(h, LZ_ERR_ARG, "lz_lsmr_run: the step counter is an int");
  LZ_TRY(lsmr_hist_reserve(h, m.steps + iters));
  const LsmrVecs lv = lsmr_vecs(m);
  const double ctol = conlim > 0.0 ? 1.0 / conlim : 0.0;
  const int gb = lsmr_blocks(m.bpad), gx = lsmr_blocks(m.xpad);
  for (int i = 0; i < iters; ++i) {
    LZ_HIP(h, lsmr_product_av(h, lv.VH, lv.Y));
    LZ_TRY(check_launch(h, "lsmr: product"));
    launch_lsmr_u(h);
    LZ_TRY(check_launch(h, "lsmr: u"));
    hipLaunchKernelGGL(k_lsmr_beta, dim3(1), dim3(kTPB), 0, h->stream, lsmr_part(m, 0), gb, m.ds, m.di);
    LZ_TRY(check_launch(h, "lsmr: beta"));
    LZ_HIP(h, lsmr_product_atu(h, lv.UH, lv.Z));
    LZ_TRY(check_launch(h, "lsmr: transposed product"));
    if (i == 0 && !m.pending)
      launch_lsmr_v<true, false>(h);  // (the flush of the last call has ended step k - 1 and left the partials of |x_{k-1}|^2)
    else
      launch_lsmr_v<true, true>(h);
    LZ_TRY(check_launch(h, "lsmr: v"));
    hipLaunchKernelGGL(k_lsmr_scalars, dim3(1), dim3(kTPB), 0, h->stream, lsmr_part(m, 1), lsmr_part(m, 2), gx, m.ds, m.di, m.hist, m.hist_cap,
                       atol, btol, ctol);
    LZ_TRY(check_launch(h, "lsmr: scalars"));
  }
  launch_lsmr_v<false, true>(h);  // the flush: the state is never lagged between two calls
  LZ_TRY(check_launch(h, "lsmr: flush"));
  LZ_HIP(h, hipMemsetAsync(m.di + kLsFresh, 0, sizeof(int), h->stream));
  launch_final_sum(lsmr_part(m, 2), gx, m.ds + kLsNormx2, h->stream);
  LZ_TRY(check_launch(h, "lsmr: final_sum"));
  m.pending = false;
  return lsmr_read_state(h, state_out);
}

int lz_lsmr_history(lz_handle h, double* out, int count) {
  LZ_TRY(lsmr_state(h, "lz_lsmr_history"));
  const LsmrState& m = h->ls;
  if (!out || count < 0 || count > m.hist_cap)
    return fail(h, LZ_ERR_ARG, "lz_lsmr_history: need out and 0 <= count <= the steps lz_lsmr_run was asked for so far (at least 1024)");
  if (count == 0) return LZ_OK;
  LZ_HIP(h, hipMemcpyAsync(out, m.hist, 2 * (size_t)count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_lsmr_get(lz_handle h, int which, double* out) {
  LZ_TRY(lsmr_state(h, "lz_lsmr_get"));
  const LsmrState& m = h->ls;
  const bool raw = (which & LZ_LSMR_RAW) != 0;
  const int w = which & ~LZ_LSMR_RAW;
  if (!out || w < 0 || w > LZ_LSMR_HBAR) return fail(h, LZ_ERR_ARG, "lz_lsmr_get: which is LZ_LSMR_X .. LZ_LSMR_HBAR, with or without LZ_LSMR_RAW");
  const LsmrVecs lv = lsmr_vecs(m);
  const double* src = w == LZ_LSMR_X ? lv.X : w == LZ_LSMR_U ? lv.UH : w == LZ_LSMR_V ? lv.VH : w == LZ_LSMR_H ? lv.H : lv.HBAR;
  const size_t count = w == LZ_LSMR_U ? (size_t)(raw ? m.bpad : m.blen) : (size_t)(raw ? m.xpad : m.xlen);
  LZ_HIP(h, hipMemcpyAsync(out, src, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  const bool divide = !raw && (w == LZ_LSMR_U || w == LZ_LSMR_V);
  double nu = 1.0;
  if (divide) LZ_HIP(h, hipMemcpyAsync(&nu, m.ds + (w == LZ_LSMR_U ? kLsNuU : kLsNuV), sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  if (divide)  // formed on read: the division the kernels do
    for (size_t i = 0; i < count; ++i) out[i] = out[i] / nu;
  return LZ_OK;
}

int lz_lsmr_set_state(lz_handle h, int transposed, int k, const double* x, const double* u, const double* v, const double* hvec,
                      const double* hbar, const double* scalars) {
  if (!h || !x || !u || !v || !hvec || !hbar || !scalars) return LZ_ERR_ARG;
  if (k < 1) return fail(h, LZ_ERR_ARG, "lz_lsmr_set_state: need k >= 1");
  LZ_TRY(lsmr_alloc(h, transposed, "lz_lsmr_set_state"));
  LsmrState& m = h->ls;
  LZ_TRY(lsmr_hist_reserve(h, k));
  const LsmrVecs lv = lsmr_vecs(m);
  const size_t xb = (size_t)m.xlen * sizeof(double);
  LZ_TRY(upload(h, lv.X, x, xb));
  LZ_TRY(upload(h, lv.UH, u, (size_t)m.blen * sizeof(double)));
  LZ_TRY(upload(h, lv.VH, v, xb));
  LZ_TRY(upload(h, lv.H, hvec, xb));
  LZ_TRY(upload(h, lv.HBAR, hbar, xb));
  double ds[kLsmrDoubles] = {0.0};
  for (int i = 0; i < 24; ++i) ds[i] = scalars[i];
  ds[kLsNuU] = 1.0;  // u_k and v_k are taken as they are given
  ds[kLsNuV] = 1.0;
  const int di[kLsmrInts] = {0, k - 1, 0, 1};
  LZ_HIP(h, hipMemcpyAsync(m.ds, ds, sizeof(ds), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipMemcpyAsync(m.di, di, sizeof(di), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));  // (the sources are the caller's and this frame's)
  m.steps = k - 1;
  m.done = 0;
  m.pending = true;
  m.live = true;
  return LZ_OK;
}

int lz_lsmr_step_time(lz_handle h, int reps, double* ms_out) {
  LZ_TRY(lsmr_state(h, "lz_lsmr_step_time"));
  LsmrState& m = h->ls;
  if (!ms_out || reps < 1) return fail(h, LZ_ERR_ARG, "lz_lsmr_step_time: need reps >= 1 and ms_out");
  if (m.done) return fail(h, LZ_ERR_STATE, "lz_lsmr_step_time: the state is done (its gated kernels would return at once)");
  const LsmrVecs lv = lsmr_vecs(m);
  hipEvent_t a, b;
  LZ_HIP(h, hipEventCreate(&a));
  LZ_HIP(h, hipEventCreate(&b));
  hipError_t err = hipSuccess;
  for (int what = 0; what < 4 && err == hipSuccess; ++what) {
    for (int r = -1; r < reps && err == hipSuccess; ++r) {  // (r == -1: the warm-up)
      if (r == 0) err = hipEventRecord(a, h->stream);
      if (err != hipSuccess) break;
      if (what == 0)
        err = lsmr_product_av(h, lv.VH, lv.Y);
      else if (what == 1)
        launch_lsmr_u(h);
      else if (what == 2)
        err = lsmr_product_atu(h, lv.UH, lv.Z);
      else
        launch_lsmr_v<true, true>(h);
    }
    if (err == hipSuccess) err = hipEventRecord(b, h->stream);
    if (err == hipSuccess) err = hipEventSynchronize(b);
    float ms = 0.f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, a, b);
    ms_out[what] = (double)ms / reps;
  }
  hipEventDestroy(a);
  hipEventDestroy(b);
  m.live = false;  // (the repeated passes have been applied to u, v, h, hbar and x again and again)
  LZ_HIP(h, err);
  return check_launch(h, "lsmr step time");
}

int lz_lsmr_info(lz_handle h, int* out) {
  if (!h || !out) return LZ_ERR_ARG;
  out[0] = 4;  // k_lsmr_u, k_lsmr_beta, k_lsmr_v, k_lsmr_scalars
  out[1] = h->ls.live && h->gk.set ? 1 : 0;
  out[2] = h->ls.transposed;
  return LZ_OK;
}

}  // extern "C"
