// BiCGSTAB (include/lanczos_hip.h, "non-symmetric linear solves"): the device half of lanczos_amd.bicgstab, A x = b for a real square
// A, symmetric or not (van der Vorst 1992), SciPy's loop scalar for scalar.  No basis and no transpose product.  The two products of an
// iteration and their x_own . y epilogues are the handle's, untouched: v = A p is called with x_own = r~ and t = A s with x_own = s, so
// r~ . v and t . s cost nothing.  (One plan cannot do that: the column-blocked two-phase SpMV with the diagonal split off forms the
// diagonal's product from x_own.  There the products run with x_own = x and the two dots ride k_bicgstab_tt.)  What is new here is the
// vector side, four streaming passes and three one-block kernels per iteration:
//   k_bicgstab_p        p = (p - omega v) beta + r (the first iteration: p = r)                              reads r, p, v, writes p: 32 B a row
//   k_bicgstab_alpha    one block: rv = r~ . v from the product's partials, the rv == 0 exit (-11), alpha = rho / rv
//   k_bicgstab_s        s = r - alpha v in place, the partials of |s|^2                                      reads r, v, writes r:    24 B
//   k_bicgstab_tt       the partials of t . t                                                                reads t:                  8 B
//   k_bicgstab_omega    one block: |s|, t . s, t . t, the half-step test |s| < atol, omega = (t . s) / (t . t)
//   k_bicgstab_r        x = (x + alpha p) + omega s - both updates of x, which nothing inside the loop reads -, r = s - omega t and the
//                       partials of |r|^2 and r~ . r                                           reads s, t, r~, x, p, writes r, x:     56 B
//   k_bicgstab_scalars  one block: |r|, rho, the head tests of the NEXT iteration in SciPy's order (|r| < atol: 0; |rho| < eps^2: -10;
//                       |omega| < eps^2: -11), beta, the iteration counter, the history, the done flag and the code
// 120 bytes a row against 184 where every statement of the loop is a pass of its own.  The half-step exit must leave x + alpha p and
// r = s: k_bicgstab_omega therefore sets a flag of its own, under which k_bicgstab_r applies the first update of x only and
// k_bicgstab_scalars turns it into the done flag - the gate closes behind that pass, not in front of it.  Every kernel reads the done
// flag first and returns at once when it is set, so a chunk of iterations is enqueued with no host synchronisation; the products of
// the rest of the chunk run on (their output goes to V and T, which nothing reads then).  No atomics: the same input gives the same bits.
#include "lz_context.h"
#include "lz_device.h"

using namespace lz;
using namespace lz::api;

namespace lz {

// ds: the scalars on the device
enum BicgstabD {
  kBcRho = 0,  // r~ . r of the coming iteration
  kBcRhoPrev,
  kBcAlpha,
  kBcOmega,
  kBcBeta,   // of the coming k_bicgstab_p
  kBcRnorm,  // the recurrence's |r| (|s| behind a half-step exit)
  kBcSnorm,
  kBcRv,
  kBcTs,
  kBcTt,
  kBicgstabDoubles = 16
};
// di; kBcStep counts the iterations that updated x, so it is SciPy's `iteration` of the coming one
enum BicgstabI { kBcDone = 0, kBcStep, kBcCode, kBcExit, kBcHalf, kBcHead, kBicgstabInts = 8 };
enum { kBcExitNone = 0, kBcExitHalf = 1, kBcExitFull = 2, kBcExitBreakdown = 3 };

struct BicgstabVecs {
  double* X;
  double* R;
  double* RT;
  double* P;
  double* V;
  double* T;
};

constexpr double kBcTiny = 2.220446049250313e-16 * 2.220446049250313e-16;  // rhotol = omegatol = eps^2 (SciPy's)

// p = (p - omega v) beta + r; the first iteration (counter 0): p = r.  Grid-stride over 16-byte positions, k_minres_step's shape: two
// positions of a lane in flight, one grid stride apart, every load of both issued before the first use.
__global__ __launch_bounds__(kTPB) void k_bicgstab_p(BicgstabVecs bv, const double* __restrict__ ds, const int* __restrict__ di, int64_t n2) {
  if (di[kBcDone]) return;
  const bool first = di[kBcStep] == 0;
  const double omega = ds[kBcOmega], beta = ds[kBcBeta];
  const double2* r2 = reinterpret_cast<const double2*>(bv.R);
  const double2* v2 = reinterpret_cast<const double2*>(bv.V);
  double2* p2 = reinterpret_cast<double2*>(bv.P);
  constexpr int U = 2;
  const int64_t stride = (int64_t)gridDim.x * kTPB;
  for (int64_t i0 = (int64_t)blockIdx.x * kTPB + threadIdx.x; i0 < n2; i0 += U * stride) {
    double2 r[U], p[U], v[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      in[u] = i < n2;
      if (!in[u]) continue;
      r[u] = r2[i];  // (k_bicgstab_s reads it next)
      if (!first) {
        p[u] = ld_stream<1>(p2 + i);
        v[u] = ld_stream<1>(v2 + i);  // (the product overwrites it)
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (!in[u]) continue;
      if (!first) {
        r[u].x = (p[u].x - omega * v[u].x) * beta + r[u].x;
        r[u].y = (p[u].y - omega * v[u].y) * beta + r[u].y;
      }
      p2[i] = r[u];  // plain store: the product reads it
    }
  }
}

// rv = r~ . v from np partials (k_final_sum's grouping); rv == 0: the breakdown -11 with x as it is; else alpha = rho / rv
__global__ __launch_bounds__(kTPB) void k_bicgstab_alpha(const double* __restrict__ part, int np, double* __restrict__ ds, int* __restrict__ di) {
  __shared__ double sm16[16];
  if (di[kBcDone]) return;
  const double rv = final_sum_emulated(part, np, sm16);  // (every thread has read the flag before thread 0 writes it: the barriers inside)
  if (threadIdx.x != 0) return;
  ds[kBcRv] = rv;
  if (rv == 0.0) {
    di[kBcCode] = -11;
    di[kBcExit] = kBcExitBreakdown;
    di[kBcHead] = 0;
    di[kBcDone] = 1;
    return;
  }
  ds[kBcAlpha] = ds[kBcRho] / rv;
}

// s = r - alpha v in place; part[b] = block b's share of |s|^2
__global__ __launch_bounds__(kTPB) void k_bicgstab_s(BicgstabVecs bv, const double* __restrict__ ds, const int* __restrict__ di, int64_t n2,
                                                    double* __restrict__ part) {
  __shared__ double sm[kTPB / 64];
  if (di[kBcDone]) return;
  const double alpha = ds[kBcAlpha];
  double2* r2 = reinterpret_cast<double2*>(bv.R);
  const double2* v2 = reinterpret_cast<const double2*>(bv.V);
  double acc = 0.0;
  constexpr int U = 2;
  const int64_t stride = (int64_t)gridDim.x * kTPB;
  for (int64_t i0 = (int64_t)blockIdx.x * kTPB + threadIdx.x; i0 < n2; i0 += U * stride) {
    double2 r[U], v[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      in[u] = i < n2;
      if (!in[u]) continue;
      r[u] = ld_stream<1>(r2 + i);
      v[u] = v2[i];  // (the next k_bicgstab_p reads it again)
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (!in[u]) continue;
      r[u].x = r[u].x - alpha * v[u].x;
      r[u].y = r[u].y - alpha * v[u].y;
      r2[i] = r[u];  // plain store: the product reads it
      acc = fma(r[u].x, r[u].x, acc);
      acc = fma(r[u].y, r[u].y, acc);
    }
  }
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// part_tt[b] = block b's share of t . t; TWO: part_to[b] = its share of t . o as well (the dots of the plan whose product cannot take
// them, and rho and |r|^2 of a state that lz_bicgstab_begin / lz_bicgstab_set_state put there: t = r, o = r~).  gate may be null.
template <bool TWO>
__global__ __launch_bounds__(kTPB) void k_bicgstab_tt(const double* __restrict__ t, const double* __restrict__ o, const int* __restrict__ gate, int64_t n2,
                                                     double* __restrict__ part_tt, double* __restrict__ part_to) {
  __shared__ double sm[kTPB / 64];
  if (gate && gate[0]) return;
  const double2* t2 = reinterpret_cast<const double2*>(t);
  const double2* o2 = reinterpret_cast<const double2*>(o);
  double acc = 0.0, acc2 = 0.0;
  constexpr int U = 2;
  const int64_t stride = (int64_t)gridDim.x * kTPB;
  for (int64_t i0 = (int64_t)blockIdx.x * kTPB + threadIdx.x; i0 < n2; i0 += U * stride) {
    double2 a[U], b[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      in[u] = i < n2;
      if (!in[u]) continue;
      a[u] = t2[i];  // (k_bicgstab_r reads it next)
      if (TWO) b[u] = o2[i];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!in[u]) continue;
      acc = fma(a[u].x, a[u].x, acc);
      acc = fma(a[u].y, a[u].y, acc);
      if (TWO) {
        acc2 = fma(b[u].x, a[u].x, acc2);
        acc2 = fma(b[u].y, a[u].y, acc2);
      }
    }
  }
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) part_tt[blockIdx.x] = acc;
  if (TWO) {
    acc2 = block_sum(acc2, sm);
    if (threadIdx.x == 0) part_to[blockIdx.x] = acc2;
  }
}

// |s| from the n_ss partials of k_bicgstab_s, t . s from the n_ts partials of the product (or of k_bicgstab_tt), t . t from n_tt; the
// half-step test |s| < atol sets the half flag and omega = 0, else omega = (t . s) / (t . t)
__global__ __launch_bounds__(kTPB) void k_bicgstab_omega(const double* __restrict__ part_ss, int n_ss, const double* __restrict__ part_ts, int n_ts,
                                                        const double* __restrict__ part_tt, int n_tt, double* __restrict__ ds, int* __restrict__ di,
                                                        double* __restrict__ hist, int hist_cap, double atol) {
  __shared__ double sm16[16];
  if (di[kBcDone]) return;
  const double ss = final_sum_emulated(part_ss, n_ss, sm16);
  const double ts = final_sum_emulated(part_ts, n_ts, sm16);
  const double tt = final_sum_emulated(part_tt, n_tt, sm16);
  if (threadIdx.x != 0) return;
  const double snorm = sqrt(ss);
  const int k = di[kBcStep];
  if (k < hist_cap) hist[2 * (size_t)k] = snorm;
  ds[kBcSnorm] = snorm;
  ds[kBcTs] = ts;
  ds[kBcTt] = tt;
  if (snorm < atol) {
    di[kBcHalf] = 1;
    ds[kBcOmega] = 0.0;
  } else {
    ds[kBcOmega] = ts / tt;
  }
}

// x = (x + alpha p) + omega s, r = s - omega t, part_rr[b] / part_rho[b] = block b's share of |r|^2 / r~ . r.  Under the half flag: x = x + alpha p
// only, r stays s and no partial is formed (k_bicgstab_scalars does not read them then).
__global__ __launch_bounds__(kTPB) void k_bicgstab_r(BicgstabVecs bv, const double* __restrict__ ds, const int* __restrict__ di, int64_t n2,
                                                    double* __restrict__ part_rr, double* __restrict__ part_rho) {
  __shared__ double sm[kTPB / 64];
  if (di[kBcDone]) return;
  const bool half = di[kBcHalf] != 0;
  const double alpha = ds[kBcAlpha], omega = ds[kBcOmega];
  double2* r2 = reinterpret_cast<double2*>(bv.R);
  const double2* t2 = reinterpret_cast<const double2*>(bv.T);
  const double2* q2 = reinterpret_cast<const double2*>(bv.RT);
  const double2* p2 = reinterpret_cast<const double2*>(bv.P);
  double2* x2 = reinterpret_cast<double2*>(bv.X);
  double acc = 0.0, acc2 = 0.0;
  constexpr int U = 2;
  const int64_t stride = (int64_t)gridDim.x * kTPB;
  for (int64_t i0 = (int64_t)blockIdx.x * kTPB + threadIdx.x; i0 < n2; i0 += U * stride) {
    double2 s[U], t[U], q[U], x[U], p[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      in[u] = i < n2;
      if (!in[u]) continue;
      x[u] = ld_stream<1>(x2 + i);
      p[u] = p2[i];  // (the next k_bicgstab_p reads it again)
      if (!half) {
        s[u] = ld_stream<1>(r2 + i);
        t[u] = ld_stream<1>(t2 + i);
        q[u] = q2[i];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (!in[u]) continue;
      x[u].x = x[u].x + alpha * p[u].x;
      x[u].y = x[u].y + alpha * p[u].y;
      if (!half) {
        x[u].x = x[u].x + omega * s[u].x;
        x[u].y = x[u].y + omega * s[u].y;
        s[u].x = s[u].x - omega * t[u].x;
        s[u].y = s[u].y - omega * t[u].y;
        r2[i] = s[u];  // plain store: k_bicgstab_p and k_bicgstab_s read it
        acc = fma(s[u].x, s[u].x, acc);
        acc = fma(s[u].y, s[u].y, acc);
        acc2 = fma(q[u].x, s[u].x, acc2);
        acc2 = fma(q[u].y, s[u].y, acc2);
      }
      st_stream<1>(x2 + i, x[u]);
    }
  }
  if (half) return;  // (uniform over the grid)
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) part_rr[blockIdx.x] = acc;
  acc2 = block_sum(acc2, sm);
  if (threadIdx.x == 0) part_rho[blockIdx.x] = acc2;
}

// ADVANCE: the end of an iteration - the counter, the history, rho_prev - and the head tests of the next one.  !ADVANCE: the head tests
// of the iteration that a fresh state (lz_bicgstab_begin, lz_bicgstab_set_state) starts from, rho_prev, alpha and omega as they stand.
template <bool ADVANCE>
__global__ __launch_bounds__(kTPB) void k_bicgstab_scalars(const double* __restrict__ part_rr, const double* __restrict__ part_rho, int np,
                                                          double* __restrict__ ds, int* __restrict__ di, double* __restrict__ hist, int hist_cap, double atol) {
  __shared__ double sm16[16];
  if (di[kBcDone]) return;
  if (ADVANCE && di[kBcHalf]) {  // the half-step exit: x + alpha p and r = s are in place
    __syncthreads();             // (every thread has read both flags)
    if (threadIdx.x == 0) {
      const int k = di[kBcStep];
      const double snorm = ds[kBcSnorm];
      if (k < hist_cap) hist[2 * (size_t)k + 1] = snorm;
      ds[kBcRnorm] = snorm;
      di[kBcStep] = k + 1;
      di[kBcCode] = 0;
      di[kBcExit] = kBcExitHalf;
      di[kBcHead] = 0;
      di[kBcDone] = 1;
    }
    return;
  }
  const double rr = final_sum_emulated(part_rr, np, sm16);
  const double rho = final_sum_emulated(part_rho, np, sm16);
  if (threadIdx.x != 0) return;
  const double rnorm = sqrt(rr);
  int k = di[kBcStep];
  double rho_prev = ds[kBcRhoPrev];
  if (ADVANCE) {
    if (k < hist_cap) hist[2 * (size_t)k + 1] = rnorm;
    k = k + 1;
    di[kBcStep] = k;
    rho_prev = ds[kBcRho];
    ds[kBcRhoPrev] = rho_prev;
  }
  ds[kBcRho] = rho;
  ds[kBcRnorm] = rnorm;
  const double omega = ds[kBcOmega];
  int code = 0, ex = kBcExitNone;
  if (rnorm < atol) {
    ex = kBcExitFull;
  } else if (fabs(rho) < kBcTiny) {
    code = -10;
    ex = kBcExitBreakdown;
  } else if (k > 0 && fabs(omega) < kBcTiny) {
    code = -11;
    ex = kBcExitBreakdown;
  } else if (k > 0) {
    ds[kBcBeta] = (rho / rho_prev) * (ds[kBcAlpha] / omega);
  }
  if (ex != kBcExitNone) {
    di[kBcCode] = code;
    di[kBcExit] = ex;
    di[kBcHead] = 1;
    di[kBcDone] = 1;
  }
}

// r = r - y (r holds b, y = A x0)
__global__ __launch_bounds__(kTPB) void k_bicgstab_r0(double* __restrict__ r, const double* __restrict__ y, int64_t n2) {
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

constexpr int kBicgstabMaxBlocks = 2048;  // k_minres_step's grid
static int bicgstab_blocks(int64_t pad) {
  const int64_t g = ((pad >> 1) + kTPB - 1) / kTPB;
  return (int)std::min<int64_t>(std::max<int64_t>(g, 1), kBicgstabMaxBlocks);
}

namespace api {

void bicgstab_free(lz_handle h) {
  BicgstabState& m = h->bc;
  big_free(m.vec);
  big_free(m.ds);
  big_free(m.di);
  big_free(m.part);
  big_free(m.hist);
  m = BicgstabState();
}

}  // namespace api
}  // namespace lz

namespace {

BicgstabVecs bicgstab_vecs(const BicgstabState& m) {
  BicgstabVecs bv;
  bv.X = m.vec;
  bv.R = m.vec + m.ld;
  bv.RT = m.vec + 2 * m.ld;
  bv.P = m.vec + 3 * m.ld;
  bv.V = m.vec + 4 * m.ld;
  bv.T = m.vec + 5 * m.ld;
  return bv;
}

// partials that the products write (trl_alloc's terms)
size_t bicgstab_product_part(lz_handle h) {
  size_t need = std::max<size_t>((size_t)h->rows / 4 + 64, (size_t)h->csr.n_rowblk + 64);
  if (h->kind == 1 && h->csr.pb) need = std::max<size_t>(need, (size_t)pb_num_partials(h->csr.pb) + 64);
  return need;
}

// the product's epilogue takes an x_own that is not x on every plan but one: launch_spmv_csr's order of choice, and false where it
// takes the column-blocked two-phase kernels (k_pb_rows forms the split-off diagonal's product from x_own)
bool bicgstab_dots_in_product(lz_handle h) {
  if (h->kind != 1) return true;
  const CsrDev& A = h->csr;
  if (A.ell_default && ell_usable(A, h->flags)) return true;
  if (h->flags & LZ_FLAG_SPMV_SCALAR) return true;
  return !(A.pb && !(h->flags & LZ_FLAG_SPMV_STREAM));
}

// the four sets of partials of the passes' own, behind the products'
double* bicgstab_part(lz_handle h, int set) { return h->bc.part + bicgstab_product_part(h) + (size_t)set * kBicgstabMaxBlocks; }

int bicgstab_alloc(lz_handle h, const char* who) {
  BicgstabState& m = h->bc;
  if (h->kind == 0)
    return fail(h, LZ_ERR_STATE, std::string(who) + (h->z.kind != 0 ? ": a complex matrix is set (BiCGSTAB takes a real one)" : ": no matrix set"));
  if (h->world > 1 || h->comm_kind != 0) return fail(h, LZ_ERR_STATE, std::string(who) + ": BiCGSTAB runs on one rank (this handle has a communicator)");
  if (h->flags & (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE))
    return fail(h, LZ_ERR_STATE, std::string(who) + ": not with LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE");
  if (h->rows < 1 || h->ncols_ext != h->rows) return fail(h, LZ_ERR_STATE, std::string(who) + ": the matrix is not square on this rank");
  LZ_HIP(h, hipSetDevice(h->dev));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  m.live = false;
  const int64_t ld = h->rows_pad;
  if (!m.vec || m.ld != ld) {
    LZ_TRY(dev_alloc(h, m.vec, 6 * (size_t)ld));
    m.ld = ld;
  }
  if (!m.ds) LZ_TRY(dev_alloc(h, m.ds, (size_t)kBicgstabDoubles));
  if (!m.di) LZ_TRY(dev_alloc(h, m.di, (size_t)kBicgstabInts));
  const size_t need = bicgstab_product_part(h) + 4 * (size_t)kBicgstabMaxBlocks;
  if (m.part_cap < need) {
    LZ_TRY(dev_alloc(h, m.part, need));
    m.part_cap = need;
  }
  LZ_HIP(h, hipMemsetAsync(m.vec, 0, 6 * (size_t)ld * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(m.ds, 0, kBicgstabDoubles * sizeof(double), h->stream));
  LZ_HIP(h, hipMemsetAsync(m.di, 0, kBicgstabInts * sizeof(int), h->stream));
  if (m.hist) LZ_HIP(h, hipMemsetAsync(m.hist, 0, 2 * (size_t)m.hist_cap * sizeof(double), h->stream));
  m.steps = 0;
  m.done = 0;
  m.fresh = false;
  return LZ_OK;
}

// the history holds at least `count` iterations; what it holds is kept
int bicgstab_hist_reserve(lz_handle h, int count) {
  BicgstabState& m = h->bc;
  if (count <= m.hist_cap) return LZ_OK;
  const int cap = std::max(count, std::max(1024, 2 * m.hist_cap));
  double* p = nullptr;
  LZ_TRY(dev_alloc(h, p, 2 * (size_t)cap));
  LZ_HIP(h, hipMemsetAsync(p, 0, 2 * (size_t)cap * sizeof(double), h->stream));
  if (m.hist && m.hist_cap > 0) LZ_HIP(h, hipMemcpyAsync(p, m.hist, 2 * (size_t)m.hist_cap * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  LZ_TRY(dev_free(h, m.hist));
  m.hist = p;
  m.hist_cap = cap;
  return LZ_OK;
}

int bicgstab_state(lz_handle h, const char* who) {
  if (!h) return LZ_ERR_ARG;
  const BicgstabState& m = h->bc;
  if (!m.live || !m.vec) return fail(h, LZ_ERR_STATE, std::string(who) + ": no state (lz_bicgstab_begin first; a new matrix drops it)");
  if (h->kind == 0 || h->rows_pad != m.ld) return fail(h, LZ_ERR_STATE, std::string(who) + ": the matrix changed since lz_bicgstab_begin");
  if (h->world > 1 || h->comm_kind != 0 || (h->flags & (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE)))
    return fail(h, LZ_ERR_STATE, std::string(who) + ": BiCGSTAB runs on one rank, without LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE");
  LZ_HIP(h, hipSetDevice(h->dev));
  return LZ_OK;
}

// y = A x with the x_own . y partials at part; returns their count
int bicgstab_product(lz_handle h, const double* x, double* y, const double* x_own, double* part) {
  if (h->kind == 1) return launch_spmv_csr(h->csr, x, y, x_own, part, h->flags, h->stream);
  return launch_gemv_dense(h->d_dense, h->rows, h->ncols_ext, h->dense_lda, x, x_own, y, part, h->stream);
}

// the partials of |r|^2 (set 0) and r~ . r (set 1) of the state as it stands: what the first lz_bicgstab_run's head tests read
void bicgstab_launch_rr(lz_handle h) {
  const BicgstabState& m = h->bc;
  const BicgstabVecs bv = bicgstab_vecs(m);
  hipLaunchKernelGGL(k_bicgstab_tt<true>, dim3(bicgstab_blocks(m.ld)), dim3(kTPB), 0, h->stream, bv.R, bv.RT, (const int*)nullptr, m.ld >> 1,
                     bicgstab_part(h, 0), bicgstab_part(h, 1));
}

int bicgstab_read_state(lz_handle h, double* state_out) {
  BicgstabState& m = h->bc;
  double ds[kBicgstabDoubles];
  int di[kBicgstabInts];
  LZ_HIP(h, hipMemcpyAsync(ds, m.ds, sizeof(ds), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipMemcpyAsync(di, m.di, sizeof(di), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  m.steps = di[kBcStep];
  m.done = di[kBcDone];
  if (state_out) {
    state_out[0] = (double)m.steps;
    state_out[1] = (double)m.done;
    state_out[2] = (double)di[kBcCode];
    state_out[3] = (double)di[kBcExit];
    state_out[4] = (double)di[kBcHead];
    state_out[5] = ds[kBcRnorm];
    state_out[6] = ds[kBcRho];
    state_out[7] = ds[kBcRhoPrev];
    state_out[8] = ds[kBcAlpha];
    state_out[9] = ds[kBcOmega];
    state_out[10] = ds[kBcBeta];
    state_out[11] = ds[kBcSnorm];
    state_out[12] = ds[kBcRv];
    state_out[13] = ds[kBcTs];
    state_out[14] = ds[kBcTt];
    state_out[15] = 0.0;
  }
  return LZ_OK;
}

}  // namespace

extern "C" {

int lz_bicgstab_begin(lz_handle h, const double* b, const double* x0) {
  if (!h || !b) return LZ_ERR_ARG;
  LZ_TRY(bicgstab_alloc(h, "lz_bicgstab_begin"));
  BicgstabState& m = h->bc;
  const BicgstabVecs bv = bicgstab_vecs(m);
  const size_t bytes = (size_t)h->rows * sizeof(double);
  LZ_TRY(upload(h, bv.R, b, bytes));
  if (x0) {
    LZ_TRY(upload(h, bv.X, x0, bytes));
    bicgstab_product(h, bv.X, bv.T, bv.X, m.part);
    LZ_TRY(check_launch(h, "bicgstab begin: product"));
    hipLaunchKernelGGL(k_bicgstab_r0, dim3(bicgstab_blocks(m.ld)), dim3(kTPB), 0, h->stream, bv.R, bv.T, m.ld >> 1);
    LZ_TRY(check_launch(h, "bicgstab begin: r0"));
    LZ_HIP(h, hipMemsetAsync(bv.T, 0, (size_t)m.ld * sizeof(double), h->stream));
  }
  LZ_HIP(h, hipMemcpyAsync(bv.RT, bv.R, (size_t)m.ld * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  bicgstab_launch_rr(h);
  LZ_TRY(check_launch(h, "bicgstab begin: rho"));
  double ds[kBicgstabDoubles] = {0.0};
  ds[kBcRhoPrev] = 1.0;
  ds[kBcAlpha] = 1.0;
  ds[kBcOmega] = 1.0;
  LZ_HIP(h, hipMemcpyAsync(m.ds, ds, sizeof(ds), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));  // (b and x0 are the caller's, ds this frame's)
  m.fresh = true;
  m.live = true;
  return LZ_OK;
}

int lz_bicgstab_run(lz_handle h, int iters, double atol_eff, double* state_out) {
  LZ_TRY(bicgstab_state(h, "lz_bicgstab_run"));
  BicgstabState& m = h->bc;
  if (iters < 0 || !(atol_eff >= 0.0)) return fail(h, LZ_ERR_ARG, "lz_bicgstab_run: need iters >= 0 and atol_eff >= 0");
  if ((int64_t)m.steps + iters > INT32_MAX / 2) return fail(h, LZ_ERR_ARG, "lz_bicgstab_run: the iteration counter is an int");
  if (m.done && !m.fresh) return bicgstab_read_state(h, state_out);
  LZ_TRY(bicgstab_hist_reserve(h, m.steps + iters));
  const BicgstabVecs bv = bicgstab_vecs(m);
  const int grid = bicgstab_blocks(m.ld);
  const int64_t n2 = m.ld >> 1;
  double* p_ss = bicgstab_part(h, 0);  // |s|^2, then |r|^2
  double* p_tt = bicgstab_part(h, 1);  // t . t, then r~ . r
  double* p_alt = bicgstab_part(h, 2);  // r~ . v and t . s where the product cannot form them
  double* p_spare = bicgstab_part(h, 3);
  const int* gate = m.di + kBcDone;
  if (m.fresh) {  // the head tests of the iteration the state starts from
    hipLaunchKernelGGL(k_bicgstab_scalars<false>, dim3(1), dim3(kTPB), 0, h->stream, p_ss, p_tt, grid, m.ds, m.di, m.hist, m.hist_cap, atol_eff);
    LZ_TRY(check_launch(h, "bicgstab: head tests"));
    m.fresh = false;
  }
  const bool fused = bicgstab_dots_in_product(h);
  for (int i = 0; i < iters; ++i) {
    hipLaunchKernelGGL(k_bicgstab_p, dim3(grid), dim3(kTPB), 0, h->stream, bv, m.ds, m.di, n2);
    LZ_TRY(check_launch(h, "bicgstab: p"));
    int np = bicgstab_product(h, bv.P, bv.V, fused ? bv.RT : bv.P, m.part);
    LZ_TRY(check_launch(h, "bicgstab: product v"));
    if (!fused) {
      hipLaunchKernelGGL(k_bicgstab_tt<true>, dim3(grid), dim3(kTPB), 0, h->stream, bv.V, bv.RT, gate, n2, p_spare, p_alt);
      LZ_TRY(check_launch(h, "bicgstab: rv"));
    }
    hipLaunchKernelGGL(k_bicgstab_alpha, dim3(1), dim3(kTPB), 0, h->stream, fused ? m.part : p_alt, fused ? np : grid, m.ds, m.di);
    LZ_TRY(check_launch(h, "bicgstab: alpha"));
    hipLaunchKernelGGL(k_bicgstab_s, dim3(grid), dim3(kTPB), 0, h->stream, bv, m.ds, m.di, n2, p_ss);
    LZ_TRY(check_launch(h, "bicgstab: s"));
    np = bicgstab_product(h, bv.R, bv.T, bv.R, m.part);
    LZ_TRY(check_launch(h, "bicgstab: product t"));
    if (fused)
      hipLaunchKernelGGL(k_bicgstab_tt<false>, dim3(grid), dim3(kTPB), 0, h->stream, bv.T, bv.R, gate, n2, p_tt, p_alt);
    else
      hipLaunchKernelGGL(k_bicgstab_tt<true>, dim3(grid), dim3(kTPB), 0, h->stream, bv.T, bv.R, gate, n2, p_tt, p_alt);
    LZ_TRY(check_launch(h, "bicgstab: tt"));
    hipLaunchKernelGGL(k_bicgstab_omega, dim3(1), dim3(kTPB), 0, h->stream, p_ss, grid, fused ? m.part : p_alt, fused ? np : grid, p_tt, grid, m.ds, m.di,
                       m.hist, m.hist_cap, atol_eff);
    LZ_TRY(check_launch(h, "bicgstab: omega"));
    hipLaunchKernelGGL(k_bicgstab_r, dim3(grid), dim3(kTPB), 0, h->stream, bv, m.ds, m.di, n2, p_ss, p_tt);
    LZ_TRY(check_launch(h, "bicgstab: r"));
    hipLaunchKernelGGL(k_bicgstab_scalars<true>, dim3(1), dim3(kTPB), 0, h->stream, p_ss, p_tt, grid, m.ds, m.di, m.hist, m.hist_cap, atol_eff);
    LZ_TRY(check_launch(h, "bicgstab: scalars"));
  }
  return bicgstab_read_state(h, state_out);
}

int lz_bicgstab_history(lz_handle h, double* out, int count) {
  LZ_TRY(bicgstab_state(h, "lz_bicgstab_history"));
  const BicgstabState& m = h->bc;
  if (!out || count < 0 || count > m.hist_cap)
    return fail(h, LZ_ERR_ARG, "lz_bicgstab_history: need out and 0 <= count <= the iterations lz_bicgstab_run was asked for so far (at least 1024)");
  if (count == 0) return LZ_OK;
  LZ_HIP(h, hipMemcpyAsync(out, m.hist, 2 * (size_t)count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_bicgstab_get(lz_handle h, int which, double* out) {
  LZ_TRY(bicgstab_state(h, "lz_bicgstab_get"));
  const BicgstabState& m = h->bc;
  const bool raw = (which & LZ_BICGSTAB_RAW) != 0;
  const int w = which & ~LZ_BICGSTAB_RAW;
  if (!out || w < 0 || w > LZ_BICGSTAB_T) return fail(h, LZ_ERR_ARG, "lz_bicgstab_get: which is LZ_BICGSTAB_X .. LZ_BICGSTAB_T, with or without LZ_BICGSTAB_RAW");
  const double* src = m.vec + (size_t)w * m.ld;  // (the enum is the order of the vectors)
  const size_t count = raw ? (size_t)m.ld : (size_t)h->rows;
  LZ_HIP(h, hipMemcpyAsync(out, src, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));
  return LZ_OK;
}

int lz_bicgstab_set_state(lz_handle h, int k, const double* x, const double* r, const double* rtilde, const double* p, const double* v,
                          const double* scalars) {
  if (!h || !x || !r || !rtilde || !p || !v || !scalars) return LZ_ERR_ARG;
  if (k < 0) return fail(h, LZ_ERR_ARG, "lz_bicgstab_set_state: need k >= 0");
  LZ_TRY(bicgstab_alloc(h, "lz_bicgstab_set_state"));
  BicgstabState& m = h->bc;
  LZ_TRY(bicgstab_hist_reserve(h, k + 1));
  const BicgstabVecs bv = bicgstab_vecs(m);
  const size_t bytes = (size_t)h->rows * sizeof(double);
  LZ_TRY(upload(h, bv.X, x, bytes));
  LZ_TRY(upload(h, bv.R, r, bytes));
  LZ_TRY(upload(h, bv.RT, rtilde, bytes));
  LZ_TRY(upload(h, bv.P, p, bytes));
  LZ_TRY(upload(h, bv.V, v, bytes));
  bicgstab_launch_rr(h);
  LZ_TRY(check_launch(h, "bicgstab set_state: rho"));
  double ds[kBicgstabDoubles] = {0.0};
  ds[kBcRhoPrev] = scalars[0];
  ds[kBcAlpha] = scalars[1];
  ds[kBcOmega] = scalars[2];
  const int di[kBicgstabInts] = {0, k, 0, 0, 0, 0, 0, 0};
  LZ_HIP(h, hipMemcpyAsync(m.ds, ds, sizeof(ds), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipMemcpyAsync(m.di, di, sizeof(di), hipMemcpyHostToDevice, h->stream));
  LZ_HIP(h, hipStreamSynchronize(h->stream));  // (the sources are the caller's and this frame's)
  m.steps = k;
  m.done = 0;
  m.fresh = true;
  m.live = true;
  return LZ_OK;
}

int lz_bicgstab_step_time(lz_handle h, int reps, double* ms_out) {
  LZ_TRY(bicgstab_state(h, "lz_bicgstab_step_time"));
  BicgstabState& m = h->bc;
  if (!ms_out || reps < 1) return fail(h, LZ_ERR_ARG, "lz_bicgstab_step_time: need reps >= 1 and ms_out");
  if (m.done || m.fresh || m.steps < 1)
    return fail(h, LZ_ERR_STATE, "lz_bicgstab_step_time: needs a state behind at least one iteration that is not done (a done state's kernels return at once)");
  const BicgstabVecs bv = bicgstab_vecs(m);
  const int grid = bicgstab_blocks(m.ld);
  const int64_t n2 = m.ld >> 1;
  const bool fused = bicgstab_dots_in_product(h);
  const int* gate = m.di + kBcDone;
  hipEvent_t a, b;
  LZ_HIP(h, hipEventCreate(&a));
  LZ_HIP(h, hipEventCreate(&b));
  hipError_t err = hipSuccess;
  for (int what = 0; what < 6 && err == hipSuccess; ++what) {
    for (int r = -1; r < reps; ++r) {  // (r == -1: the warm-up)
      if (r == 0) err = hipEventRecord(a, h->stream);
      if (what == 0)
        bicgstab_product(h, bv.P, bv.V, fused ? bv.RT : bv.P, m.part);
      else if (what == 1)
        bicgstab_product(h, bv.R, bv.T, bv.R, m.part);
      else if (what == 2)
        hipLaunchKernelGGL(k_bicgstab_p, dim3(grid), dim3(kTPB), 0, h->stream, bv, m.ds, m.di, n2);
      else if (what == 3)
        hipLaunchKernelGGL(k_bicgstab_s, dim3(grid), dim3(kTPB), 0, h->stream, bv, m.ds, m.di, n2, bicgstab_part(h, 0));
      else if (what == 4)
        hipLaunchKernelGGL(k_bicgstab_tt<false>, dim3(grid), dim3(kTPB), 0, h->stream, bv.T, bv.R, gate, n2, bicgstab_part(h, 1), bicgstab_part(h, 2));
      else
        hipLaunchKernelGGL(k_bicgstab_r, dim3(grid), dim3(kTPB), 0, h->stream, bv, m.ds, m.di, n2, bicgstab_part(h, 0), bicgstab_part(h, 1));
    }
    if (err == hipSuccess) err = hipEventRecord(b, h->stream);
    if (err == hipSuccess) err = hipEventSynchronize(b);
    float ms = 0.f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, a, b);
    ms_out[what] = (double)ms / reps;
  }
  hipEventDestroy(a);
  hipEventDestroy(b);
  m.live = false;  // (the repeated passes have been applied to p, r and x again and again)
  LZ_HIP(h, err);
  return check_launch(h, "bicgstab step time");
}

int lz_bicgstab_info(lz_handle h, int* out) {
  if (!h || !out) return LZ_ERR_ARG;
  const bool fused = h->kind == 0 || bicgstab_dots_in_product(h);
  out[0] = fused ? 9 : 10;  // two products, k_bicgstab_p, _alpha, _s, _tt, _omega, _r, _scalars (and one more k_bicgstab_tt for r~ . v)
  out[1] = fused ? 1 : 0;
  out[2] = h->bc.live && h->kind != 0 && h->rows_pad == h->bc.ld ? 1 : 0;
  return LZ_OK;
}

}  // extern "C"
