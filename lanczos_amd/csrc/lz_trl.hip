// Kernels of the thick-restart Lanczos solver (lz_trl_api.hip, lanczos_amd/eigsh.py): the in-place restart V[0..kk) <- S^T V[0..m),
// the classical Gram-Schmidt update of r, the band form's block Gram-Schmidt (dots and update of b work vectors per walk over the
// basis), the one-block bookkeeping between the passes, and the fused residual norms (real and, for eigs, complex eigenvalues).
#include "lz_device.h"

namespace lz {

// ------------------------------------------------------------------ restart: V[k][p] = sum_{i < m} S[i][k] V[i][p] (k < kk), V[kk] = V[m]
// v_mfma_f64_16x16x4_f64 (lane layout: lz_gemm.hip): D (16 outputs k x 16 positions) += A (16 x 4: S^T, from LDS) B (4 basis rows x 16
// positions).  A wave owns a 32-position tile (one 16-byte load per lane and k-step: rows 4t..4t+3 x 256 contiguous bytes; the even
// positions feed accE, the odd ones accO) and keeps all kk outputs of the tile in its accumulators, so it has read all m input rows of
// the tile before it writes any output row of it: tiles are disjoint, so the transform is race-free in place without a second buffer.
// Positions >= rows (the padding of a row) are read - they only reach their own output columns - and never written.
template <int KT>
__global__ __launch_bounds__(kTPB) void k_trl_restart(double* __restrict__ V, int64_t ldv, int64_t rows, int64_t ntiles, int m, int kk,
                                                      const double* __restrict__ S) {
  extern __shared__ double sS[];  // [KS][KT][64]: lane l of the A fragment of k-step t, output tile q = S[4t + (l >> 4)][16q + (l & 15)]
  const int KS = (m + 3) >> 2;
  for (int f = threadIdx.x; f < KS * KT * 64; f += kTPB) {
    const int t = f / (KT * 64), q = (f / 64) % KT, l = f & 63;
    const int i = 4 * t + (l >> 4), c = 16 * q + (l & 15);
    sS[f] = (i < m && c < kk) ? S[(int64_t)i * kk + c] : 0.0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  for (int64_t tile = (int64_t)blockIdx.x * (kTPB / 64) + w; tile < ntiles; tile += (int64_t)gridDim.x * (kTPB / 64)) {
    const int64_t p = tile * 32 + 2 * lr;
    double4_t accE[KT], accO[KT];
#pragma unroll
    for (int q = 0; q < KT; ++q) accE[q] = accO[q] = (double4_t){0.0, 0.0, 0.0, 0.0};
    for (int t0 = 0; t0 < KS; t0 += 8) {
      d2v_t b[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        int i = 4 * (t0 + u) + lk;
        i = i < m ? i : m - 1;  // rows past m: any valid row, its S entries are 0
        b[u] = t0 + u < KS ? __builtin_nontemporal_load(reinterpret_cast<const d2v_t*>(V + (int64_t)i * ldv + p)) : (d2v_t){0.0, 0.0};
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (t0 + u < KS) {
#pragma unroll
          for (int q = 0; q < KT; ++q) {
            const double a = sS[((t0 + u) * KT + q) * 64 + lane];
            accE[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[u].x, accE[q], 0, 0, 0);
            accO[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[u].y, accO[q], 0, 0, 0);
          }
        }
    }
    // every load of the tile has been consumed by the MFMAs above: the rows may now be overwritten
    const bool both = p + 1 < rows, one = p < rows;
#pragma unroll
    for (int q = 0; q < KT; ++q)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k = 16 * q + lk + 4 * g;
        if (k < kk) {
          double* dst = V + (int64_t)k * ldv + p;
          if (both)
            *reinterpret_cast<double2*>(dst) = make_double2(accE[q][g], accO[q][g]);
          else if (one)
            dst[0] = accE[q][g];
        }
      }
    if (lk == 0) {
      const double2 r = *reinterpret_cast<const double2*>(V + (int64_t)m * ldv + p);
      double* dst = V + (int64_t)kk * ldv + p;
      if (both)
        *reinterpret_cast<double2*>(dst) = r;
      else if (one)
        dst[0] = r.x;
    }
  }
}

template <int KT>
static hipError_t launch_trl_restart_t(double* V, int64_t ldv, int64_t rows, int m, int kk, const double* S, hipStream_t s) {
  const int64_t ntiles = (rows + 31) / 32;
  const size_t lds = (size_t)((m + 3) / 4) * KT * 64 * sizeof(double);
  hipError_t err = hipSuccess;
  if (lds > 65536) err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_trl_restart<KT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err != hipSuccess) return err;
  const int64_t grid = std::min<int64_t>((ntiles + 3) / 4, 8 * kNumCU);
  hipLaunchKernelGGL(k_trl_restart<KT>, dim3((unsigned)grid), dim3(kTPB), lds, s, V, ldv, rows, ntiles, m, kk, S);
  return hipSuccess;
}

hipError_t launch_trl_restart(double* V, int64_t ldv, int64_t rows, int m, int kk, const double* S, hipStream_t s) {
  switch ((kk + 15) / 16) {
    case 1: return launch_trl_restart_t<1>(V, ldv, rows, m, kk, S, s);
    case 2: return launch_trl_restart_t<2>(V, ldv, rows, m, kk, S, s);
    case 3: return launch_trl_restart_t<3>(V, ldv, rows, m, kk, S, s);
    case 4: return launch_trl_restart_t<4>(V, ldv, rows, m, kk, S, s);
    case 5: return launch_trl_restart_t<5>(V, ldv, rows, m, kk, S, s);
    case 6: return launch_trl_restart_t<6>(V, ldv, rows, m, kk, S, s);
    case 7: return launch_trl_restart_t<7>(V, ldv, rows, m, kk, S, s);
    case 8: return launch_trl_restart_t<8>(V, ldv, rows, m, kk, S, s);
    default: return hipErrorInvalidValue;
  }
}

// ------------------------------------------------------------------ CGS update: r = r - sum_{i < nrows} c_i V_i, part[b] = block b's share of r.r
// A lane owns P double2 positions and walks the rows RU at a time (P * RU 16-byte loads in flight); the sum is formed in row order
// (products and sums rounded separately, as k_update_slice does) and subtracted once.  gate: runs only when gate[0] != 0.
template <int P, int RU>
__global__ __launch_bounds__(kTPB) void k_trl_cgs(const double* __restrict__ V, int64_t ldv, int64_t n2, int nrows, const double* __restrict__ c,
                                                  double* __restrict__ r, double* __restrict__ part, const int* __restrict__ gate) {
  if (gate && gate[0] == 0) return;
  __shared__ double sm[kTPB / 64];
  const int64_t base = (int64_t)blockIdx.x * (kTPB * P) + threadIdx.x;
  const int64_t ld2 = ldv >> 1;
  const double2* V2 = reinterpret_cast<const double2*>(V);
  double2* r2 = reinterpret_cast<double2*>(r);
  int64_t pos[P];
  bool ok[P];
  double tx[P], ty[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    pos[p] = base + (int64_t)p * kTPB;
    ok[p] = pos[p] < n2;
    if (!ok[p]) pos[p] = n2 - 1;
    tx[p] = ty[p] = 0.0;
  }
  for (int k = 0; k < nrows; k += RU) {
    double2 q[RU][P];
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (k + u < nrows)
#pragma unroll
        for (int p = 0; p < P; ++p) q[u][p] = ld_stream<1>(V2 + (int64_t)(k + u) * ld2 + pos[p]);
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (k + u < nrows) {
        const double ck = c[k + u];
#pragma unroll
        for (int p = 0; p < P; ++p) {
          tx[p] = tx[p] + ck * q[u][p].x;
          ty[p] = ty[p] + ck * q[u][p].y;
        }
      }
  }
  double ss = 0.0;
#pragma unroll
  for (int p = 0; p < P; ++p)
    if (ok[p]) {
      double2 x = r2[pos[p]];
      x.x = x.x - tx[p];
      x.y = x.y - ty[p];
      r2[pos[p]] = x;
      ss = fma(x.x, x.x, ss);
      ss = fma(x.y, x.y, ss);
    }
  ss = block_sum(ss, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = ss;
}

int launch_trl_cgs(const double* V, int64_t ldv, int64_t len, int nrows, const double* c, double* r, double* part, const int* gate,
                   hipStream_t s) {
  const int64_t n2 = len >> 1;
  if (n2 >= (int64_t)kTPB * 4 * kNumCU) {  // long rows: 4 positions x 4 rows in flight per lane
    const int grid = (int)((n2 + kTPB * 4 - 1) / (kTPB * 4));
    hipLaunchKernelGGL((k_trl_cgs<4, 4>), dim3(grid), dim3(kTPB), 0, s, V, ldv, n2, nrows, c, r, part, gate);
    return grid;
  }
  const int grid = (int)((n2 + kTPB - 1) / kTPB);  // short rows: one position per lane, 16 rows in flight
  hipLaunchKernelGGL((k_trl_cgs<1, 16>), dim3(grid), dim3(kTPB), 0, s, V, ldv, n2, nrows, c, r, part, gate);
  return grid;
}
int trl_cgs_blocks(int64_t len) {
  const int64_t n2 = len >> 1;
  return n2 >= (int64_t)kTPB * 4 * kNumCU ? (int)((n2 + kTPB * 4 - 1) / (kTPB * 4)) : (int)((n2 + kTPB - 1) / kTPB);
}

// ------------------------------------------------------------------ band Lanczos: C = V[0..r0) W^T, all b columns from one walk over the basis
// v_mfma_f64_4x4x4_4b_f64 in k_qtw_mfma4's arrangement (lz_reorth.hip: A[blk][i][k] in lane 16k + 4blk + i, B[blk][k][jj] in lane
// 16k + 4blk + jj, D[blk][i][jj] in lane 16i + 4blk + jj; the four blocks are four adjacent 64-byte chunks of the same four basis
// rows).  There the B operand broadcasts one vector over the four columns jj; here column jj IS work vector 4g + jj, so one MFMA
// per four basis rows forms the dots with four work vectors (NG = 2: two MFMAs for up to eight) from one load of the rows.
// A block stages a slice of L positions of all b work vectors in LDS, walks the r0 rows of that slice from the newest down (the
// update pass that follows starts at row 0), and adds the tile results to its wave's r0 x b run in LDS; the grid is persistent
// (slice = blockIdx.x, + gridDim.x, ...), so a block leaves ONE run however long the rows are.  The four waves' runs are added in
// wave order, the blocks' runs by k_final_rows_t: a fixed order, no atomics.  len is a multiple of 32, L of 128.
template <int NG>
__global__ __launch_bounds__(kTPB) void k_trl_band_dots(const double* __restrict__ V, int64_t ldv, int64_t len, int r0,
                                                       const double* __restrict__ W, int64_t ldw, int b, int L, int run,
                                                       double* __restrict__ part) {
  extern __shared__ double2 sw[];  // [b][L / 2] double2 of W, then [4][run] doubles
  constexpr int T = 2, U = 4;
  double* keep_all = reinterpret_cast<double*>(sw) + (int64_t)b * L;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double* keep = keep_all + w * run;
  for (int i = threadIdx.x; i < 4 * run; i += kTPB) keep_all[i] = 0.0;
  const int li = lane & 3, blk = (lane >> 2) & 3, lk = lane >> 4;
  const int sub = L >> 2;  // positions per wave (a multiple of 32)
  const int m_lo = w * sub;
  const int eoff = 8 * blk + 2 * lk;
  const int L2 = L >> 1;
  const int64_t nslices = (len + L - 1) / L;
  const int i_top = ((r0 - 1) / (4 * T)) * (4 * T);
  for (int64_t slice = blockIdx.x; slice < nslices; slice += gridDim.x) {
    const int64_t base = slice * L;
    const int cnt = (int)(len - base < L ? len - base : L);
    __syncthreads();  // the previous slice's image is no longer read (first trip: the runs are zero)
    for (int c = 0; c < b; ++c) {
      const double2* src = reinterpret_cast<const double2*>(W + (int64_t)c * ldw + base);
      for (int t = threadIdx.x; t < (cnt >> 1); t += kTPB) sw[c * L2 + t] = src[t];
    }
    __syncthreads();
    int m_hi = m_lo + sub;
    if (m_hi > cnt) m_hi = cnt;
    const int nsteps = m_hi > m_lo ? (m_hi - m_lo) >> 5 : 0;  // 32 positions (256 B of a row) per step
    if (nsteps == 0) continue;                                // (wave-uniform; the barriers above are reached by every wave)
    const double2* swl[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int col = 4 * g + li;
      swl[g] = sw + (col < b ? col : 0) * L2 + ((m_lo + eoff) >> 1);
    }
    for (int i0 = i_top; i0 >= 0; i0 -= 4 * T) {
      const double2* a[T];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        int i = i0 + 4 * t + li;
        if (i >= r0) i = r0 - 1;  // clamped duplicate, discarded below
        a[t] = reinterpret_cast<const double2*>(V + (int64_t)i * ldv + base + m_lo + eoff);
      }
      double acc[T][NG];
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[t][g] = 0.0;
      for (int s0 = 0; s0 < nsteps; s0 += U) {
        double2 av[T][U];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int t = 0; t < T; ++t) av[t][u] = (s0 + u < nsteps) ? ld_stream<1>(a[t] + 16 * (s0 + u)) : make_double2(0.0, 0.0);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int g = 0; g < NG; ++g) {
            const double2 bv = (s0 + u < nsteps && 4 * g + li < b) ? swl[g][16 * (s0 + u)] : make_double2(0.0, 0.0);
#pragma unroll
            for (int t = 0; t < T; ++t) {
              acc[t][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(av[t][u].x, bv.x, acc[t][g], 0, 0, 0);
              acc[t][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(av[t][u].y, bv.y, acc[t][g], 0, 0, 0);
            }
          }
      }
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          double v = acc[t][g];       // D[blk][i][jj] in lane 16 i + 4 blk + jj
          v += __shfl_xor(v, 4, 64);  // add the four blocks (adjacent 64-byte chunks)
          v += __shfl_xor(v, 8, 64);
          const int row = i0 + 4 * t + lk, col = 4 * g + li;
          if (blk == 0 && row < r0 && col < b) keep[row * b + col] += v;  // this wave's own run: no other wave touches it
        }
    }
  }
  __syncthreads();
  double* mine = part + (int64_t)blockIdx.x * run;
  for (int i = threadIdx.x; i < run; i += kTPB) mine[i] = ((keep_all[i] + keep_all[run + i]) + keep_all[2 * run + i]) + keep_all[3 * run + i];
}

// slice length of k_trl_band_dots: about 40 KiB of work vectors per block (four blocks per CU), at least 512 positions
static int band_slice(int b) { return 512 * std::max(1, 10 / b); }
int trl_band_dots_blocks(int64_t len, int b) {
  const int L = band_slice(b);
  return (int)std::min<int64_t>((len + L - 1) / L, 4 * kNumCU);
}
hipError_t launch_trl_band_dots(const double* V, int64_t ldv, int64_t len, int r0, const double* W, int64_t ldw, int b, double* part,
                                hipStream_t s) {
  const int L = band_slice(b);
  const int run = trl_band_run(r0, b);
  const int G = trl_band_dots_blocks(len, b);
  const size_t lds = ((size_t)b * L + 4 * (size_t)run) * sizeof(double);
  if (b <= 4) {
    if (lds > 65536) {
      const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_trl_band_dots<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (err != hipSuccess) return err;
    }
    hipLaunchKernelGGL(k_trl_band_dots<1>, dim3(G), dim3(kTPB), lds, s, V, ldv, len, r0, W, ldw, b, L, run, part);
  } else {
    if (lds > 65536) {
      const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_trl_band_dots<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (err != hipSuccess) return err;
    }
    hipLaunchKernelGGL(k_trl_band_dots<2>, dim3(G), dim3(kTPB), lds, s, V, ldv, len, r0, W, ldw, b, L, run, part);
  }
  return hipSuccess;
}

// ------------------------------------------------------------------ band Lanczos: W[c] -= sum_{i < r0} C[i][c] V_i for all b columns in one walk
// k_trl_cgs with B accumulators per position: a lane owns P double2 positions of every work vector and walks the rows RU at a time,
// every row loaded once for all B columns; the sums are formed in row order (products and sums rounded separately) and subtracted
// once.  part[c * gridDim.x + block] = the block's share of |w_c|^2.
template <int B, int P, int RU>
__global__ __launch_bounds__(kTPB) void k_trl_band_update(const double* __restrict__ V, int64_t ldv, int64_t n2, int r0,
                                                         const double* __restrict__ C, double* __restrict__ W, int64_t ldw,
                                                         double* __restrict__ part) {
  __shared__ double sm[kTPB / 64];
  const int64_t base = (int64_t)blockIdx.x * (kTPB * P) + threadIdx.x;
  const int64_t ld2 = ldv >> 1, lw2 = ldw >> 1;
  const double2* V2 = reinterpret_cast<const double2*>(V);
  double2* W2 = reinterpret_cast<double2*>(W);
  int64_t pos[P];
  bool ok[P];
  double tx[B][P], ty[B][P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    pos[p] = base + (int64_t)p * kTPB;
    ok[p] = pos[p] < n2;
    if (!ok[p]) pos[p] = n2 - 1;
#pragma unroll
    for (int c = 0; c < B; ++c) tx[c][p] = ty[c][p] = 0.0;
  }
  for (int k = 0; k < r0; k += RU) {
    double2 q[RU][P];
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (k + u < r0)
#pragma unroll
        for (int p = 0; p < P; ++p) q[u][p] = ld_stream<1>(V2 + (int64_t)(k + u) * ld2 + pos[p]);
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (k + u < r0) {
#pragma unroll
        for (int c = 0; c < B; ++c) {
          const double ck = C[(k + u) * B + c];
#pragma unroll
          for (int p = 0; p < P; ++p) {
            tx[c][p] = tx[c][p] + ck * q[u][p].x;
            ty[c][p] = ty[c][p] + ck * q[u][p].y;
          }
        }
      }
  }
#pragma unroll
  for (int c = 0; c < B; ++c) {
    double ss = 0.0;
#pragma unroll
    for (int p = 0; p < P; ++p)
      if (ok[p]) {
        double2 x = W2[(int64_t)c * lw2 + pos[p]];
        x.x = x.x - tx[c][p];
        x.y = x.y - ty[c][p];
        W2[(int64_t)c * lw2 + pos[p]] = x;
        ss = fma(x.x, x.x, ss);
        ss = fma(x.y, x.y, ss);
      }
    ss = block_sum(ss, sm);
    if (threadIdx.x == 0) part[(int64_t)c * gridDim.x + blockIdx.x] = ss;
  }
}

int trl_band_update_blocks(int64_t len) {
  const int64_t n2 = len >> 1;
  return n2 >= (int64_t)kTPB * 2 * kNumCU ? (int)((n2 + kTPB * 2 - 1) / (kTPB * 2)) : (int)((n2 + kTPB - 1) / kTPB);
}
template <int B>
static int launch_trl_band_update_t(const double* V, int64_t ldv, int64_t len, int r0, const double* C, double* W, int64_t ldw, double* part,
                                    hipStream_t s) {
  const int64_t n2 = len >> 1;
  const int grid = trl_band_update_blocks(len);
  if (n2 >= (int64_t)kTPB * 2 * kNumCU)  // long rows: 2 positions x 4 rows in flight per lane
    hipLaunchKernelGGL((k_trl_band_update<B, 2, 4>), dim3(grid), dim3(kTPB), 0, s, V, ldv, n2, r0, C, W, ldw, part);
  else  // short rows: one position per lane, 8 rows in flight
    hipLaunchKernelGGL((k_trl_band_update<B, 1, 8>), dim3(grid), dim3(kTPB), 0, s, V, ldv, n2, r0, C, W, ldw, part);
  return grid;
}
int launch_trl_band_update(const double* V, int64_t ldv, int64_t len, int r0, const double* C, double* W, int64_t ldw, int b, double* part,
                           hipStream_t s) {
  switch (b) {
    case 2: return launch_trl_band_update_t<2>(V, ldv, len, r0, C, W, ldw, part, s);
    case 3: return launch_trl_band_update_t<3>(V, ldv, len, r0, C, W, ldw, part, s);
    case 4: return launch_trl_band_update_t<4>(V, ldv, len, r0, C, W, ldw, part, s);
    case 5: return launch_trl_band_update_t<5>(V, ldv, len, r0, C, W, ldw, part, s);
    case 6: return launch_trl_band_update_t<6>(V, ldv, len, r0, C, W, ldw, part, s);
    case 7: return launch_trl_band_update_t<7>(V, ldv, len, r0, C, W, ldw, part, s);
    case 8: return launch_trl_band_update_t<8>(V, ldv, len, r0, C, W, ldw, part, s);
    default: return 0;
  }
}

// proj[c * ldf + i] = C1[i * b + c] + C2[i * b + c] for i < r0, c < nb: rows j .. j + nb - 1 of the projected coefficients, columns 0 .. r0 - 1
__global__ __launch_bounds__(kTPB) void k_trl_band_proj(const double* __restrict__ C1, const double* __restrict__ C2, int r0, int b, int nb,
                                                       double* __restrict__ proj, int ldf) {
  for (int f = threadIdx.x; f < r0 * nb; f += kTPB) {
    const int c = f / r0, i = f % r0;
    proj[(int64_t)c * ldf + i] = C1[i * b + c] + C2[i * b + c];
  }
}
void launch_trl_band_proj(const double* C1, const double* C2, int r0, int b, int nb, double* proj, int ldf, hipStream_t s) {
  hipLaunchKernelGGL(k_trl_band_proj, dim3(1), dim3(kTPB), 0, s, C1, C2, r0, b, nb, proj, ldf);
}

// ------------------------------------------------------------------ between the passes (one block)
// mode 0 (after pass 1): nrm2 = sum(part) in a fixed order, proj[0..j] = c[0..j], gate = force or |r|^2 < |w|^2 / 2 (c[j + 1] = w.w:
// the DGKS criterion |r| < |w| / sqrt 2).  mode 1 (after the gated pass 2): returns when gate[0] == 0, else nrm2 = sum(part),
// proj[0..j] += c[0..j].  mode 2: nrm2 = sum(part) only.
__global__ __launch_bounds__(kTPB) void k_trl_post(int mode, const double* __restrict__ part, int np, const double* __restrict__ c, int j,
                                                   double* __restrict__ nrm2, double* __restrict__ proj, int* __restrict__ gate, int force) {
  if (mode == 1 && gate[0] == 0) return;
  __shared__ double sm[kTPB / 64];
  double s = 0.0;
  for (int b = threadIdx.x; b < np; b += kTPB) s += part[b];
  s = block_sum(s, sm);
  if (threadIdx.x == 0) {
    nrm2[0] = s;
    if (mode == 0) gate[0] = (force || s < 0.5 * c[j + 1]) ? 1 : 0;
  }
  if (mode == 2) return;
  for (int i = threadIdx.x; i <= j; i += kTPB) proj[i] = mode == 0 ? c[i] : proj[i] + c[i];
}

void launch_trl_post(int mode, const double* part, int np, const double* c, int j, double* nrm2, double* proj, int* gate, int force,
                     hipStream_t s) {
  hipLaunchKernelGGL(k_trl_post, dim3(1), dim3(kTPB), 0, s, mode, part, np, c, j, nrm2, proj, gate, force);
}

// ------------------------------------------------------------------ Chebyshev filter: one step of the scaled three-term recurrence
// z = a (w - c y) - b x with w = A y already in place (the SpMV / GEMV wrote it): three 16-byte reads and one 16-byte write per two
// rows, 32 B per row, a pure stream - no LDS, no atomics, grid sized as k_three_term's.  The arithmetic is cheb_combine (lz_device.h), shared with
// the SpMV's fused epilogue (SpmvCheb, lz_spmv.hip): same bits on either path.
// Rows >= rows (the padding the sweep kernels stream) are written as zero whatever the inputs hold there.
__global__ __launch_bounds__(kTPB) void k_cheb_step(double* __restrict__ wz, const double* y, const double* x, const double* __restrict__ coef,
                                                   int i, int degree, double c, int64_t rows, int64_t n2) {
  const double a = coef[i];
  const double b = coef[degree + i];
  double2* z2 = reinterpret_cast<double2*>(wz);
  const double2* y2 = reinterpret_cast<const double2*>(y);
  const double2* x2 = reinterpret_cast<const double2*>(x);
  for (int64_t p = (int64_t)blockIdx.x * kTPB + threadIdx.x; p < n2; p += (int64_t)gridDim.x * kTPB) {
    const double2 w = z2[p];
    const double2 yv = y2[p];  // plain loads: y is the next step's x, and x of the first step is the basis row the first pass re-reads
    const double2 xv = x2[p];
    double2 z;
    z.x = 2 * p < rows ? cheb_combine(w.x, yv.x, xv.x, a, b, c) : 0.0;
    z.y = 2 * p + 1 < rows ? cheb_combine(w.y, yv.y, xv.y, a, b, c) : 0.0;
    z2[p] = z;  // plain store: the next SpMV (or the first Gram-Schmidt pass) reads it at once
  }
}
// the grid of both streaming steps (k_cheb_step, k_cheb_series_step): a thread per two rows, 2048 blocks at the most
static int cheb_grid(int64_t n2) { return (int)std::min<int64_t>(std::max<int64_t>((n2 + kTPB - 1) / kTPB, 1), 2048); }
void launch_cheb_step(double* wz, const double* y, const double* x, const double* coef, int i, int degree, double c, int64_t rows,
                      int64_t len, hipStream_t s) {
  const int64_t n2 = len >> 1;
  hipLaunchKernelGGL(k_cheb_step, dim3(cheb_grid(n2)), dim3(kTPB), 0, s, wz, y, x, coef, i, degree, c, rows, n2);
}

// ------------------------------------------------------------------ Chebyshev series: one term of the recurrence added to the running sum
// The interior mode's filter is a sum of all terms, sum_i mu_i T_i(A^) x, so beside k_cheb_step's three reads and one write the step
// reads and writes the running sum: 48 B per row (the first step 32: no x, no sum to read; the last 40: the sum goes where the term would).
// Same grid, same 16-byte accesses, arithmetic in series_combine (lz_device.h) shared with the SpMV's fused epilogue: same bits.
__global__ __launch_bounds__(kTPB) void k_cheb_series_step(double* __restrict__ wz, const double* y, const double* x, const double* acc_in,
                                                          double* acc_out, const double* __restrict__ mu, int i, int last, double inv_e,
                                                          double c, int64_t rows, int64_t n2) {
  const bool first = i == 1;
  const double mu0 = mu[0];
  const double mui = mu[i];
  double2* z2 = reinterpret_cast<double2*>(wz);
  const double2* y2 = reinterpret_cast<const double2*>(y);
  const double2* x2 = reinterpret_cast<const double2*>(x);
  const double2* a2 = reinterpret_cast<const double2*>(acc_in);
  double2* o2 = reinterpret_cast<double2*>(acc_out);
  for (int64_t p = (int64_t)blockIdx.x * kTPB + threadIdx.x; p < n2; p += (int64_t)gridDim.x * kTPB) {
    const double2 w = z2[p];
    const double2 yv = y2[p];
    const double2 xv = first ? make_double2(0.0, 0.0) : x2[p];
    const double2 av = first ? make_double2(0.0, 0.0) : a2[p];
    double2 z = make_double2(0.0, 0.0), a = make_double2(0.0, 0.0);
    if (2 * p < rows) a.x = series_combine(w.x, yv.x, xv.x, av.x, inv_e, c, mu0, mui, first, &z.x);
    if (2 * p + 1 < rows) a.y = series_combine(w.y, yv.y, xv.y, av.y, inv_e, c, mu0, mui, first, &z.y);
    if (last) {
      z2[p] = a;
    } else {
      z2[p] = z;
      o2[p] = a;
    }
  }
}
void launch_cheb_series_step(double* wz, const double* y, const double* x, const double* acc_in, double* acc_out, const double* mu, int i,
                             int last, double inv_e, double c, int64_t rows, int64_t len, hipStream_t s) {
  const int64_t n2 = len >> 1;
  hipLaunchKernelGGL(k_cheb_series_step, dim3(cheb_grid(n2)), dim3(kTPB), 0, s, wz, y, x, acc_in, acc_out, mu, i, last, inv_e, c, rows, n2);
}

// ------------------------------------------------------------------ true residuals |A y_i - theta_i y_i|
// CSR (the assembled stencil too: its CSR arrays stay beside the coded copy): one launch for all k vectors, blockIdx.y = i, a thread per
// row forms (A y_i)_row - theta_i y_i[row] and the block adds the squares: part[i * G + b].
__global__ __launch_bounds__(kTPB) void k_trl_resid_csr(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                        const double* __restrict__ vals, const double* __restrict__ Y, int64_t ldy, int64_t rows,
                                                        const double* __restrict__ theta, double* __restrict__ part) {
  __shared__ double sm[kTPB / 64];
  const int i = blockIdx.y;
  const double* x = Y + (int64_t)i * ldy;
  const int64_t row = (int64_t)blockIdx.x * kTPB + threadIdx.x;
  double d = 0.0;
  if (row < rows) {
    double sum = 0.0;
    for (int e = rowptr[row]; e < rowptr[row + 1]; ++e) sum += vals[e] * x[colidx[e]];
    const double t = sum - theta[i] * x[row];
    d = t * t;
  }
  d = block_sum(d, sm);
  if (threadIdx.x == 0) part[(int64_t)i * gridDim.x + blockIdx.x] = d;
}
int launch_trl_resid_csr(const CsrDev& A, const double* Y, int64_t ldy, int k, const double* theta, double* part, hipStream_t s) {
  const int G = (int)((A.rows + kTPB - 1) / kTPB);
  hipLaunchKernelGGL(k_trl_resid_csr, dim3(G, k), dim3(kTPB), 0, s, A.rowptr, A.colidx, A.vals, Y, ldy, A.rows, theta, part);
  return G;
}
// dense: y = A y_i comes from the GEMV; this adds the squares of y - theta_i y_i (part[i * G + b])
__global__ __launch_bounds__(kTPB) void k_trl_resid_diff(const double* __restrict__ y, const double* __restrict__ x, int64_t rows,
                                                         const double* __restrict__ theta, int i, double* __restrict__ part) {
  __shared__ double sm[kTPB / 64];
  const int64_t row = (int64_t)blockIdx.x * kTPB + threadIdx.x;
  double d = 0.0;
  if (row < rows) {
    const double t = y[row] - theta[i] * x[row];
    d = t * t;
  }
  d = block_sum(d, sm);
  if (threadIdx.x == 0) part[(int64_t)i * gridDim.x + blockIdx.x] = d;
}
int launch_trl_resid_diff(const double* y, const double* x, int64_t rows, const double* theta, int i, double* part, hipStream_t s) {
  const int G = (int)((rows + kTPB - 1) / kTPB);
  hipLaunchKernelGGL(k_trl_resid_diff, dim3(G), dim3(kTPB), 0, s, y, x, rows, theta, i, part);
  return G;
}
// ------------------------------------------------------------------ true residuals |A x - lambda x| for complex lambda (Krylov-Schur, eigs)
// Rows 0 .. k-1 of Y hold eigenvectors of a real matrix in real form.  im[i] == 0: row i is x and the value is k_trl_resid_csr's, the
// same expressions in the same order: same bits.  im[i] > 0: rows i and i + 1 are x_r and x_i of x = x_r + i x_i (the caller has
// checked that i + 1 < k and that (re, im)[i + 1] is the conjugate); the real and imaginary parts of A x - lambda x are
//   t_r = A x_r - re x_r + im x_i,   t_i = A x_i - im x_r - re x_i,
// and the block of row i adds t_r^2 + t_i^2: it walks each matrix row once and gathers x_r and x_i at every column, so one pass over
// the matrix serves both products.  The block of row i + 1 (im < 0) reads nothing and writes a zero partial.  part[i * G + b], summed
// by k_trl_rownorm in a fixed order: no atomics.
__global__ __launch_bounds__(kTPB) void k_trl_resid_cplx_csr(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                             const double* __restrict__ vals, const double* __restrict__ Y, int64_t ldy,
                                                             int64_t rows, const double* __restrict__ re, const double* __restrict__ im,
                                                             double* __restrict__ part) {
  __shared__ double sm[kTPB / 64];
  const int i = blockIdx.y;
  const double li = im[i];  // block-uniform
  const int64_t row = (int64_t)blockIdx.x * kTPB + threadIdx.x;
  double d = 0.0;
  if (row < rows && !(li < 0.0)) {
    const double* x = Y + (int64_t)i * ldy;
    if (li == 0.0) {
      double sum = 0.0;
      for (int e = rowptr[row]; e < rowptr[row + 1]; ++e) sum += vals[e] * x[colidx[e]];
      const double t = sum - re[i] * x[row];
      d = t * t;
    } else {
      const double* xi = x + ldy;
      double sr = 0.0, si = 0.0;
      for (int e = rowptr[row]; e < rowptr[row + 1]; ++e) {
        const double v = vals[e];
        const int32_t c = colidx[e];
        sr += v * x[c];
        si += v * xi[c];
      }
      const double lr = re[i], ar = x[row], ai = xi[row];
      const double tr = (sr - lr * ar) + li * ai;
      const double ti = (si - li * ar) - lr * ai;
      d = tr * tr + ti * ti;
    }
  }
  d = block_sum(d, sm);
  if (threadIdx.x == 0) part[(int64_t)i * gridDim.x + blockIdx.x] = d;
}
int launch_trl_resid_cplx_csr(const CsrDev& A, const double* Y, int64_t ldy, int k, const double* re, const double* im, double* part,
                              hipStream_t s) {
  const int G = (int)((A.rows + kTPB - 1) / kTPB);
  hipLaunchKernelGGL(k_trl_resid_cplx_csr, dim3(G, k), dim3(kTPB), 0, s, A.rowptr, A.colidx, A.vals, Y, ldy, A.rows, re, im, part);
  return G;
}
// dense, a pair in rows i and i + 1: yr = A x_r and yi = A x_i come from two GEMVs; this adds t_r^2 + t_i^2 (part[i * G + b]) and
// writes the zero partials of row i + 1 (part[(i + 1) * G + b])
__global__ __launch_bounds__(kTPB) void k_trl_resid_cplx_diff(const double* __restrict__ yr, const double* __restrict__ yi,
                                                              const double* __restrict__ xr, const double* __restrict__ xi, int64_t rows,
                                                              const double* __restrict__ re, const double* __restrict__ im, int i,
                                                              double* __restrict__ part) {
  __shared__ double sm[kTPB / 64];
  const int64_t row = (int64_t)blockIdx.x * kTPB + threadIdx.x;
  double d = 0.0;
  if (row < rows) {
    const double lr = re[i], li = im[i], ar = xr[row], ai = xi[row];
    const double tr = (yr[row] - lr * ar) + li * ai;
    const double ti = (yi[row] - li * ar) - lr * ai;
    d = tr * tr + ti * ti;
  }
  d = block_sum(d, sm);
  if (threadIdx.x == 0) {
    part[(int64_t)i * gridDim.x + blockIdx.x] = d;
    part[(int64_t)(i + 1) * gridDim.x + blockIdx.x] = 0.0;
  }
}
int launch_trl_resid_cplx_diff(const double* yr, const double* yi, const double* xr, const double* xi, int64_t rows, const double* re,
                               const double* im, int i, double* part, hipStream_t s) {
  const int G = (int)((rows + kTPB - 1) / kTPB);
  hipLaunchKernelGGL(k_trl_resid_cplx_diff, dim3(G), dim3(kTPB), 0, s, yr, yi, xr, xi, rows, re, im, i, part);
  return G;
}
// out[i] = sqrt(sum_b part[i * G + b]), one block per vector
__global__ __launch_bounds__(kTPB) void k_trl_rownorm(const double* __restrict__ part, int G, double* __restrict__ out) {
  __shared__ double sm[kTPB / 64];
  double s = 0.0;
  for (int b = threadIdx.x; b < G; b += kTPB) s += part[(int64_t)blockIdx.x * G + b];
  s = block_sum(s, sm);
  if (threadIdx.x == 0) out[blockIdx.x] = sqrt(s);
}
void launch_trl_rownorm(const double* part, int G, int k, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_trl_rownorm, dim3(k), dim3(kTPB), 0, s, part, G, out);
}

}  // namespace lz
