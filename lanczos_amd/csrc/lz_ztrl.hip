// Kernels of the complex thick-restart Lanczos solver (lz_ztrl_api.hip, lanczos_amd/eigsh.py on complex Hermitian input): the complex
// inner products of the work vector with the basis, the complex classical Gram-Schmidt update, and the residual norm.  The basis is
// planar - complex row i is the real rows 2 i (real part) and 2 i + 1 (imaginary part) - so the restart, scale-and-store and the final
// sums are the real kernels' (lz_trl.hip, lz_reorth.hip).  Both walks are memory-bound: a lane owns P 16-byte positions of every row
// and has RU rows (2 RU P loads) in flight, as k_trl_cgs does.
#include "lz_device.h"

namespace lz {

// ------------------------------------------------------------------ zdots: c_i = <V_i, w> = sum conj(V_i) w, i < nb; self slot: w^H w
// Re = sum Vr wr + Vi wi, Im = sum Vr wi - Vi wr: both from one read of the row.  The block keeps its slice of w in registers, every
// wave adds its lanes by a shuffle tree and parks the row's two sums in LDS; the four waves are added in wave order at the end:
// part[(2 i + 0 / 1) * G + b].  Positions past n2 read a valid position and multiply it by a zero w.
template <int P, int RU>
__global__ __launch_bounds__(kTPB) void k_zdots(const double* __restrict__ V, int64_t ldv, int64_t n2, int nb, const double* __restrict__ w,
                                                double* __restrict__ part, const int* __restrict__ gate) {
  if (gate && gate[0] == 0) return;
  __shared__ double sred[kTPB / 64][2 * (kZMaxRows + 1)];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * (kTPB * P) + threadIdx.x;
  const int64_t ld2 = ldv >> 1;
  const double2* V2 = reinterpret_cast<const double2*>(V);
  const double2* w2 = reinterpret_cast<const double2*>(w);
  int64_t pos[P];
  double2 wr[P], wi[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    pos[p] = base + (int64_t)p * kTPB;
    const bool ok = pos[p] < n2;
    if (!ok) pos[p] = n2 - 1;
    wr[p] = ok ? w2[pos[p]] : make_double2(0.0, 0.0);
    wi[p] = ok ? w2[ld2 + pos[p]] : make_double2(0.0, 0.0);
  }
  for (int k = 0; k < nb; k += RU) {
    double2 qr[RU][P], qi[RU][P];
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (k + u < nb)
#pragma unroll
        for (int p = 0; p < P; ++p) {
          qr[u][p] = ld_stream<1>(V2 + (int64_t)(2 * (k + u)) * ld2 + pos[p]);
          qi[u][p] = ld_stream<1>(V2 + (int64_t)(2 * (k + u) + 1) * ld2 + pos[p]);
        }
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (k + u < nb) {  // (block-uniform)
        double ar = 0.0, ai = 0.0;
#pragma unroll
        for (int p = 0; p < P; ++p) {
          ar = fma(qr[u][p].x, wr[p].x, ar);
          ar = fma(qi[u][p].x, wi[p].x, ar);
          ar = fma(qr[u][p].y, wr[p].y, ar);
          ar = fma(qi[u][p].y, wi[p].y, ar);
          ai = fma(qr[u][p].x, wi[p].x, ai);
          ai = fma(-qi[u][p].x, wr[p].x, ai);
          ai = fma(qr[u][p].y, wi[p].y, ai);
          ai = fma(-qi[u][p].y, wr[p].y, ai);
        }
        ar = wave_sum(ar);
        ai = wave_sum(ai);
        if (lane == 0) {
          sred[wv][2 * (k + u)] = ar;
          sred[wv][2 * (k + u) + 1] = ai;
        }
      }
  }
  double ss = 0.0;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    ss = fma(wr[p].x, wr[p].x, ss);
    ss = fma(wi[p].x, wi[p].x, ss);
    ss = fma(wr[p].y, wr[p].y, ss);
    ss = fma(wi[p].y, wi[p].y, ss);
  }
  ss = wave_sum(ss);
  if (lane == 0) {
    sred[wv][2 * nb] = ss;
    sred[wv][2 * nb + 1] = 0.0;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < 2 * (nb + 1); t += kTPB)
    part[(int64_t)t * gridDim.x + blockIdx.x] = ((sred[0][t] + sred[1][t]) + sred[2][t]) + sred[3][t];
}

// The launch shapes of both walks (k_trl_cgs's): rows of at least kTPB * 4 * kNumCU double2 positions - a padded length of
// 2^19 = 524288 doubles - take four positions per lane, shorter ones one position per lane and more rows in flight.
static bool z_long(int64_t n2) { return n2 >= (int64_t)kTPB * 4 * kNumCU; }
static int z_blocks(int64_t len) {
  const int64_t n2 = len >> 1;
  return z_long(n2) ? (int)((n2 + kTPB * 4 - 1) / (kTPB * 4)) : (int)((n2 + kTPB - 1) / kTPB);
}
int zdots_blocks(int64_t len) { return z_blocks(len); }
int zcgs_blocks(int64_t len) { return z_blocks(len); }

int launch_zdots(const double* V, int64_t ldv, int64_t len, int nb, const double* w, double* part, const int* gate, hipStream_t s) {
  const int64_t n2 = len >> 1;
  const int grid = z_blocks(len);
  if (z_long(n2))
    hipLaunchKernelGGL((k_zdots<4, 2>), dim3(grid), dim3(kTPB), 0, s, V, ldv, n2, nb, w, part, gate);
  else
    hipLaunchKernelGGL((k_zdots<1, 8>), dim3(grid), dim3(kTPB), 0, s, V, ldv, n2, nb, w, part, gate);
  return grid;
}

// ------------------------------------------------------------------ zcgs: w -= sum_{i < nb} c_i V_i, part[b] = block b's share of |w|^2
// c_i V_i = (cr Vr - ci Vi) + i (cr Vi + ci Vr).  The sum is formed in row order, products and sums rounded separately, and subtracted
// once, as k_trl_cgs does.  gate: runs only when gate[0] != 0.
template <int P, int RU>
__global__ __launch_bounds__(kTPB) void k_zcgs(const double* __restrict__ V, int64_t ldv, int64_t n2, int nb, const double* __restrict__ c,
                                               double* __restrict__ w, double* __restrict__ part, const int* __restrict__ gate) {
  if (gate && gate[0] == 0) return;
  __shared__ double sm[kTPB / 64];
  const int64_t base = (int64_t)blockIdx.x * (kTPB * P) + threadIdx.x;
  const int64_t ld2 = ldv >> 1;
  const double2* V2 = reinterpret_cast<const double2*>(V);
  double2* w2 = reinterpret_cast<double2*>(w);
  int64_t pos[P];
  bool ok[P];
  double2 tr[P], ti[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    pos[p] = base + (int64_t)p * kTPB;
    ok[p] = pos[p] < n2;
    if (!ok[p]) pos[p] = n2 - 1;
    tr[p] = ti[p] = make_double2(0.0, 0.0);
  }
  for (int k = 0; k < nb; k += RU) {
    double2 qr[RU][P], qi[RU][P];
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (k + u < nb)
#pragma unroll
        for (int p = 0; p < P; ++p) {
          qr[u][p] = ld_stream<1>(V2 + (int64_t)(2 * (k + u)) * ld2 + pos[p]);
          qi[u][p] = ld_stream<1>(V2 + (int64_t)(2 * (k + u) + 1) * ld2 + pos[p]);
        }
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (k + u < nb) {
        const double cr = c[2 * (k + u)], ci = c[2 * (k + u) + 1];
#pragma unroll
        for (int p = 0; p < P; ++p) {
          tr[p].x = (tr[p].x + cr * qr[u][p].x) - ci * qi[u][p].x;
          tr[p].y = (tr[p].y + cr * qr[u][p].y) - ci * qi[u][p].y;
          ti[p].x = (ti[p].x + cr * qi[u][p].x) + ci * qr[u][p].x;
          ti[p].y = (ti[p].y + cr * qi[u][p].y) + ci * qr[u][p].y;
        }
      }
  }
  double ss = 0.0;
#pragma unroll
  for (int p = 0; p < P; ++p)
    if (ok[p]) {
      double2 xr = w2[pos[p]], xi = w2[ld2 + pos[p]];
      xr.x = xr.x - tr[p].x;
      xr.y = xr.y - tr[p].y;
      xi.x = xi.x - ti[p].x;
      xi.y = xi.y - ti[p].y;
      w2[pos[p]] = xr;
      w2[ld2 + pos[p]] = xi;
      ss = fma(xr.x, xr.x, ss);
      ss = fma(xi.x, xi.x, ss);
      ss = fma(xr.y, xr.y, ss);
      ss = fma(xi.y, xi.y, ss);
    }
  ss = block_sum(ss, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = ss;
}

int launch_zcgs(const double* V, int64_t ldv, int64_t len, int nb, const double* c, double* w, double* part, const int* gate, hipStream_t s) {
  const int64_t n2 = len >> 1;
  const int grid = z_blocks(len);
  if (z_long(n2))
    hipLaunchKernelGGL((k_zcgs<4, 2>), dim3(grid), dim3(kTPB), 0, s, V, ldv, n2, nb, c, w, part, gate);
  else
    hipLaunchKernelGGL((k_zcgs<1, 8>), dim3(grid), dim3(kTPB), 0, s, V, ldv, n2, nb, c, w, part, gate);
  return grid;
}

// ------------------------------------------------------------------ residual: squares of |y - theta_i x| over n complex entries
__global__ __launch_bounds__(kTPB) void k_zresid_diff(const double* __restrict__ y, const double* __restrict__ x, int64_t ld, int64_t n,
                                                      const double* __restrict__ theta, int i, double* __restrict__ part) {
  __shared__ double sm[kTPB / 64];
  const int64_t row = (int64_t)blockIdx.x * kTPB + threadIdx.x;
  double d = 0.0;
  if (row < n) {
    const double th = theta[i];
    const double tr = y[row] - th * x[row];
    const double ti = y[ld + row] - th * x[ld + row];
    d = tr * tr + ti * ti;
  }
  d = block_sum(d, sm);
  if (threadIdx.x == 0) part[(int64_t)i * gridDim.x + blockIdx.x] = d;
}
int launch_zresid_diff(const double* y, const double* x, int64_t ld, int64_t n, const double* theta, int i, double* part, hipStream_t s) {
  const int G = (int)((n + kTPB - 1) / kTPB);
  hipLaunchKernelGGL(k_zresid_diff, dim3(G), dim3(kTPB), 0, s, y, x, ld, n, theta, i, part);
  return G;
}

}  // namespace lz
