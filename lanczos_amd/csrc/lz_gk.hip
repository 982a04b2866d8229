// The rectangular product of the Golub-Kahan-Lanczos solver (lz_gk_api.hip, lanczos_amd/svds.py): y = A x for a CSR matrix of any
// shape, rows != ncols in either direction.  k_spmv_stream (lz_spmv.hip) without its x_own[row] * y[row] epilogue - that read runs out
// of range as soon as rows > ncols - plus a segment path for long rows: the transpose of a tall-skinny matrix has few, very long
// rows (10^6 x 40 with 2 entries per row: 40 rows of 50 000), which a row-per-workgroup kernel would run on 40 of the 256 CUs.
//
// Work items (RectItem, built on the host by rect_plan): either a block of whole rows whose entries fit the LDS tile
// (CsrDev::blk_nnz_cap products, at most 512 rows) or one segment of at most blk_nnz_cap entries of a longer row.
//  * Row blocks: k_spmv_stream's two phases - coalesced 16 / 8-byte loads of vals / colidx, products staged in LDS, then a lane per
//    row adds them in CSR order, products and sums rounded separately (-ffp-contract=off): the bits of SciPy's csr_matvec.
//  * Segments: lane t adds the entries t, t + 256, ... of its segment in that order, the lanes' sums go through block_sum's fixed
//    tree, the block leaves one partial; k_spmv_rect_fold (one lane per long row) adds a row's partials in segment order.  No
//    atomics: the same input gives the same bits, but a split row is NOT bit-identical to SciPy (another summation order).
// The block that owns item 0 also writes the padding y[rows .. rows_pad) as zeros: the basis walks stream rows_pad.  x is read at
// colidx values only (< ncols, validated at upload; the two pad entries behind the arrays hold column 0).
#include "lz_device.h"

namespace lz {

struct RectItem {
  int32_t a, b, c, seg;  // seg < 0: rows [a, b); seg >= 0: entries [b, c) of row a, partial slot seg
};
struct RectLong {
  int32_t row, slot0, nseg, pad;
};

__global__ __launch_bounds__(kTPB) void k_spmv_rect(const RectItem* __restrict__ items, const int32_t* __restrict__ rowptr,
                                                   const int32_t* __restrict__ colidx, const double* __restrict__ vals,
                                                   const double* __restrict__ x, double* __restrict__ y, int64_t rows, int64_t rows_pad,
                                                   double* __restrict__ segpart) {
  extern __shared__ double prod[];  // blk_nnz_cap + 2 products
  __shared__ double sm[kTPB / 64];
  const int blk = xcd_remap(blockIdx.x, gridDim.x);
  if (blk == 0 && rows + threadIdx.x < rows_pad) y[rows + threadIdx.x] = 0.0;  // (rows_pad - rows < 32)
  const RectItem it = items[blk];
  if (it.seg < 0) {
    const int r0 = it.a, r1 = it.b;
    const int k0 = rowptr[r0], k1 = rowptr[r1];
    // phase 1 (k_spmv_stream's): products, two entries per lane and step, aligned to even k, batches of 4 steps
    const int kk = k0 & ~1;
    const int npair = (k1 - kk + 1) >> 1;
    constexpr int NB = 4;
    for (int pb = threadIdx.x; pb < npair; pb += NB * kTPB) {
      double2 a[NB];
      int2 c[NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        int p = pb + kTPB * i;
        if (p >= npair) p = pb;  // clamped duplicate, discarded below
        const int k = kk + 2 * p;
        a[i] = ld_stream<1>(reinterpret_cast<const double2*>(vals + k));
        c[i] = ld_stream<1>(reinterpret_cast<const int2*>(colidx + k));
      }
      double2 xv[NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) xv[i] = make_double2(x[c[i].x], x[c[i].y]);
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int p = pb + kTPB * i;
        if (p < npair) {
          const int k = kk + 2 * p;
          const double p0 = (k >= k0) ? a[i].x * xv[i].x : 0.0;
          const double p1 = (k + 1 < k1) ? a[i].y * xv[i].y : 0.0;
          *reinterpret_cast<double2*>(&prod[2 * p]) = make_double2(p0, p1);
        }
      }
    }
    __syncthreads();
    // phase 2: per-row sequential sums out of LDS, CSR order
    for (int row = r0 + threadIdx.x; row < r1; row += kTPB) {
      const int a = rowptr[row] - kk, b = rowptr[row + 1] - kk;
      double sum = 0.0;
      int k = a;
      for (; k + 4 <= b; k += 4) {
        const double p0 = prod[k], p1 = prod[k + 1], p2 = prod[k + 2], p3 = prod[k + 3];
        sum += p0;
        sum += p1;
        sum += p2;
        sum += p3;
      }
      for (; k < b; ++k) sum += prod[k];
      y[row] = sum;
    }
  } else {
    // one segment of a long row: four independent (value, column) loads and gathers in flight per lane, added in entry order
    const int kb = it.b, ke = it.c;
    double acc = 0.0;
    for (int k = kb + threadIdx.x; k < ke; k += 4 * kTPB) {
      double v[4];
      int c[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int ku = k + u * kTPB;
        const bool in = ku < ke;
        v[u] = in ? __builtin_nontemporal_load(vals + ku) : 0.0;
        c[u] = in ? __builtin_nontemporal_load(colidx + ku) : 0;
      }
      double xv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) xv[u] = x[c[u]];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (k + u * kTPB < ke) acc += v[u] * xv[u];
    }
    acc = block_sum(acc, sm);
    if (threadIdx.x == 0) segpart[it.seg] = acc;
  }
}

// y[row] = the row's segment partials added in segment order
__global__ __launch_bounds__(kTPB) void k_spmv_rect_fold(const RectLong* __restrict__ lrows, int nlong, const double* __restrict__ segpart,
                                                        double* __restrict__ y) {
  const int i = blockIdx.x * kTPB + threadIdx.x;
  if (i >= nlong) return;
  const RectLong L = lrows[i];
  double s = 0.0;
  for (int q = 0; q < L.nseg; ++q) s += segpart[L.slot0 + q];
  y[L.row] = s;
}

void rect_plan(const int32_t* rowptr, int64_t rows, int nnz_cap, bool split, std::vector<int32_t>& items, std::vector<int32_t>& lrows,
               int* nslots) {
  items.clear();
  lrows.clear();
  int slots = 0;
  int64_t r = 0;
  while (r < rows) {
    int64_t e = r;
    const int64_t k0 = rowptr[r];
    while (e < rows && e - r < 512 && (int64_t)rowptr[e + 1] - k0 <= nnz_cap) ++e;
    if (e > r) {
      const int32_t it[4] = {(int32_t)r, (int32_t)e, 0, -1};
      items.insert(items.end(), it, it + 4);
      r = e;
      continue;
    }
    // a row longer than the tile: segments of nnz_cap entries (split == false: one segment, the row-per-workgroup form)
    const int64_t k1 = rowptr[r + 1];
    const int64_t step = split ? nnz_cap : k1 - k0;
    const int32_t lr[4] = {(int32_t)r, slots, (int32_t)((k1 - k0 + step - 1) / step), 0};
    lrows.insert(lrows.end(), lr, lr + 4);
    for (int64_t k = k0; k < k1; k += step) {
      const int32_t it[4] = {(int32_t)r, (int32_t)k, (int32_t)std::min(k + step, k1), slots++};
      items.insert(items.end(), it, it + 4);
    }
    ++r;
  }
  *nslots = slots;
}

hipError_t launch_spmv_rect(const CsrDev& A, const double* x, double* y, int64_t rows_pad, hipStream_t s) {
  const size_t lds = (size_t)(A.blk_nnz_cap + 2) * sizeof(double);
  // the kernel's static block_sum scratch counts against the same 64 KiB: at the upper clamp of knob 4 (8190 + 2 products = 65 536 B)
  // the two together are past it, and the per-kernel limit has to be raised as launch_trl_restart_t does for its kernel
  if (lds + (kTPB / 64) * sizeof(double) > 65536) {
    const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_spmv_rect), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
  }
  hipLaunchKernelGGL(k_spmv_rect, dim3(A.n_rect), dim3(kTPB), lds, s, reinterpret_cast<const RectItem*>(A.rect_items), A.rowptr, A.colidx,
                     A.vals, x, y, A.rows, rows_pad, A.rect_seg);
  if (A.n_rect_long > 0)
    hipLaunchKernelGGL(k_spmv_rect_fold, dim3((A.n_rect_long + kTPB - 1) / kTPB), dim3(kTPB), 0, s,
                       reinterpret_cast<const RectLong*>(A.rect_long), A.n_rect_long, A.rect_seg, y);
  return hipSuccess;
}

// ---------------------------------------------------------------------------------------------------------------- dense operator
// One row-major copy S (R x C, stride ld) serves both directions (DenseDev, lz_internal.h).  The matrix is read once per product with
// 16-byte non-temporal loads (ld_stream<1>: ld is even, every row 16-byte aligned); x and u go through the caches.  Every sum has one
// order per plan: lane-private fma chains over a fixed stride, then shuffle trees, LDS slots added in index order, partials added by
// k_dense_fold in a fixed pattern.  No atomics.  A kernel that writes `out` directly also zeroes out[len .. pad) (pad - len < 32).

// rowdot, short and medium rows: G lanes (a power of two, <= 64) per row, 256 / G rows per trip and kDenseShortRows trips per
// workgroup with their loads in flight together - a wave that took one row only would live for one load; lane g of a group adds the
// column pairs g, g + G, .. (one trip while C <= 2 G), lane 0 an odd last column, then a shuffle tree inside the group
__global__ __launch_bounds__(kTPB) void k_dense_rowdot_short(const double* __restrict__ S, int64_t ld, int64_t R, int64_t C, int G,
                                                            const double* __restrict__ x, double* __restrict__ out, int64_t pad) {
  constexpr int K = kDenseShortRows;
  if (blockIdx.x == 0 && R + threadIdx.x < pad) out[R + threadIdx.x] = 0.0;
  const int gl = threadIdx.x & (G - 1), ngrp = kTPB / G;
  const int64_t rbase = (int64_t)blockIdx.x * (K * ngrp) + threadIdx.x / G;
  const int64_t m2 = C >> 1;
  const double2* x2 = reinterpret_cast<const double2*>(x);
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  for (int64_t p = gl; p < m2; p += G) {
    double2 a[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int64_t r = rbase + (int64_t)k * ngrp;
      a[k] = r < R ? ld_stream<1>(reinterpret_cast<const double2*>(S + r * ld) + p) : make_double2(0.0, 0.0);
    }
    const double2 xv = x2[p];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = fma(a[k].y, xv.y, fma(a[k].x, xv.x, acc[k]));
  }
  if ((C & 1) && gl == 0) {
    const double xl = x[C - 1];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int64_t r = rbase + (int64_t)k * ngrp;
      if (r < R) acc[k] = fma(S[r * ld + C - 1], xl, acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    for (int off = G >> 1; off > 0; off >>= 1) acc[k] += __shfl_down(acc[k], off, 64);  // (lane 0 of a group reads its own group only)
    const int64_t r = rbase + (int64_t)k * ngrp;
    if (gl == 0 && r < R) out[r] = acc[k];
  }
}

// rowdot, one wave per row: gemv_row_wave
__global__ __launch_bounds__(kTPB) void k_dense_rowdot_wave(const double* __restrict__ S, int64_t ld, int64_t R, int64_t C,
                                                           const double* __restrict__ x, double* __restrict__ out, int64_t pad) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * (kTPB / 64) + w;
  if (blockIdx.x == 0 && R + threadIdx.x < pad) out[R + threadIdx.x] = 0.0;
  if (row >= R) return;
  const double acc = gemv_row_wave(S + row * ld, x, C, lane);
  if (lane == 0) out[row] = acc;
}

// rowdot, row groups: one wave per segment [c0, c0 + seg) of kDenseSegRows adjacent rows, which share every load of x - a long x does
// not stay in L2, and a wave on one medium row lives for a load or two -; lane t adds the column pairs t, t + 128, .. and t + 64,
// t + 192, .. of a row on two fma chains, lane 0 an odd last column.  One segment: out[row]; else part[segment * pstride + row] for
// k_dense_fold.  A group behind the last row repeats it.
__global__ __launch_bounds__(kTPB) void k_dense_rowdot_seg(const double* __restrict__ S, int64_t ld, int64_t R, int64_t C,
                                                          const double* __restrict__ x, int nseg, int64_t seg, double* __restrict__ part,
                                                          int64_t pstride, double* __restrict__ out, int64_t pad) {
  constexpr int K = kDenseSegRows;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t wid = (int64_t)blockIdx.x * (kTPB / 64) + w;
  if (nseg == 1 && blockIdx.x == 0 && R + threadIdx.x < pad) out[R + threadIdx.x] = 0.0;
  const int64_t r0 = wid / nseg * K;
  if (r0 >= R) return;
  const int64_t sg = wid % nseg, c0 = sg * seg, len = std::min(seg, C - c0);  // (seg is even: 16-byte aligned in S and in x)
  const double2* x2 = reinterpret_cast<const double2*>(x + c0);
  const double2* a2[K];
#pragma unroll
  for (int k = 0; k < K; ++k) a2[k] = reinterpret_cast<const double2*>(S + std::min(r0 + k, R - 1) * ld + c0);
  double acc0[K], acc1[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc0[k] = acc1[k] = 0.0;
  const int64_t m2 = len >> 1;
  int64_t p = lane;
  for (; p + 64 < m2; p += 128) {
    double2 u[K], v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) u[k] = ld_stream<1>(a2[k] + p), v[k] = ld_stream<1>(a2[k] + p + 64);
    const double2 xu = x2[p], xv = x2[p + 64];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      acc0[k] = fma(u[k].y, xu.y, fma(u[k].x, xu.x, acc0[k]));
      acc1[k] = fma(v[k].y, xv.y, fma(v[k].x, xv.x, acc1[k]));
    }
  }
  if (p < m2) {
    const double2 xu = x2[p];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double2 u = ld_stream<1>(a2[k] + p);
      acc0[k] = fma(u.y, xu.y, fma(u.x, xu.x, acc0[k]));
    }
  }
  if ((len & 1) && lane == 0) {
    const double xl = x[c0 + len - 1];
#pragma unroll
    for (int k = 0; k < K; ++k) acc0[k] = fma(reinterpret_cast<const double*>(a2[k])[len - 1], xl, acc0[k]);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double s = wave_sum(acc0[k] + acc1[k]);
    if (lane == 0 && r0 + k < R) (nseg == 1 ? out : part + sg * pstride)[r0 + k] = s;
  }
}

// out[i] = part[0 .. n)[i] for i < len, 0 on [len, pad): kDenseFoldSub lanes share an output, lane s adds partials s, s + 16, .. in
// that order, their sixteen sums are added in lane order out of LDS
__global__ __launch_bounds__(kTPB) void k_dense_fold(const double* __restrict__ part, int n, int64_t stride, double* __restrict__ out,
                                                    int64_t len, int64_t pad) {
  constexpr int NO = kTPB / kDenseFoldSub;  // outputs per workgroup
  __shared__ double sm[kDenseFoldSub][NO];
  const int o = threadIdx.x % NO, sub = threadIdx.x / NO;
  const int64_t i = (int64_t)blockIdx.x * NO + o;
  double acc = 0.0;
  if (i < len)
    for (int q = sub; q < n; q += kDenseFoldSub) acc += part[(int64_t)q * stride + i];
  sm[sub][o] = acc;
  __syncthreads();
  if (sub == 0 && i < pad) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < kDenseFoldSub; ++q) t += sm[q][o];
    out[i] = i < len ? t : 0.0;
  }
}

// colsum, tiles of tw <= 64 column pairs (the pairs spread evenly over ceil(C / 128) tiles: C = 257 is three tiles of 43 pairs, not
// two full ones and one of a single pair) x slabs of `slab` rows: a lane owns two adjacent columns, the four waves of a workgroup take the rows
// r0 + w, r0 + w + 4, .. of the slab, eight rows in flight per lane on two fma chains; the waves' sums are added in wave order out of
// LDS.  direct (one slab): out[c], else out[slab * ostride + c] for k_dense_fold.  The padding column of an odd C is zero in S and not written.
__global__ __launch_bounds__(kTPB) void k_dense_colsum(const double* __restrict__ S, int64_t ld, int64_t R, int64_t C,
                                                      const double* __restrict__ u, double* __restrict__ out, int64_t ostride, int64_t slab,
                                                      int ntile, int tw, int64_t pad, int direct) {
  __shared__ double2 sm[kTPB / 64][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (direct && blockIdx.x == 0 && C + threadIdx.x < pad) out[C + threadIdx.x] = 0.0;
  const int tile = blockIdx.x % ntile;
  const int64_t sl = blockIdx.x / ntile;
  const int64_t c2 = (int64_t)tile * tw + lane, ld2 = ld >> 1;
  const bool act = lane < tw && 2 * c2 < C;
  const int64_t r0 = sl * slab, r1 = std::min(R, r0 + slab);
  const double2* s2 = reinterpret_cast<const double2*>(S) + c2;
  double2 a0 = make_double2(0.0, 0.0), a1 = a0;
  constexpr int NW = kTPB / 64;
  for (int64_t r = r0 + w; r < r1; r += 8 * NW) {
    double2 v[8];
    double uu[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t rr = r + k * NW;
      const bool in = rr < r1;
      v[k] = (in && act) ? ld_stream<1>(s2 + rr * ld2) : make_double2(0.0, 0.0);
      uu[k] = in ? u[rr] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
      a0.x = fma(v[k].x, uu[k], a0.x);
      a0.y = fma(v[k].y, uu[k], a0.y);
      a1.x = fma(v[k + 1].x, uu[k + 1], a1.x);
      a1.y = fma(v[k + 1].y, uu[k + 1], a1.y);
    }
  }
  sm[w][lane] = make_double2(a0.x + a1.x, a0.y + a1.y);
  __syncthreads();
  if (w == 0 && act) {
    double2 t = sm[0][lane];
#pragma unroll
    for (int q = 1; q < NW; ++q) t.x += sm[q][lane].x, t.y += sm[q][lane].y;
    double* o = out + (direct ? 0 : sl * ostride) + 2 * c2;
    o[0] = t.x;
    if (2 * c2 + 1 < C) o[1] = t.y;
  }
}

// colsum, narrow rows: LG lanes (a power of two, <= 64) cover the column pairs of a row - tile blockIdx.y of them where C > 2 LG -, the
// workgroup takes 256 / LG rows per trip, eight trips in flight; the row lanes' sums are added in row-lane order out of LDS
__global__ __launch_bounds__(kTPB) void k_dense_colsum_narrow(const double* __restrict__ S, int64_t ld, int64_t R, int64_t C, int LG,
                                                             const double* __restrict__ u, double* __restrict__ part, int64_t ostride,
                                                             int64_t slab) {
  __shared__ double2 sm[kTPB];
  const int cl = threadIdx.x & (LG - 1), rl = threadIdx.x / LG, NR = kTPB / LG;
  const int64_t c2 = (int64_t)blockIdx.y * LG + cl, ld2 = ld >> 1;
  const bool act = 2 * c2 < C;
  const int64_t r0 = (int64_t)blockIdx.x * slab, r1 = std::min(R, r0 + slab);
  const double2* s2 = reinterpret_cast<const double2*>(S) + c2;
  double2 a0 = make_double2(0.0, 0.0), a1 = a0;
  for (int64_t r = r0 + rl; r < r1; r += 8 * NR) {
    double2 v[8];
    double uu[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t rr = r + (int64_t)k * NR;
      const bool in = rr < r1;
      v[k] = (in && act) ? ld_stream<1>(s2 + rr * ld2) : make_double2(0.0, 0.0);
      uu[k] = in ? u[rr] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
      a0.x = fma(v[k].x, uu[k], a0.x);
      a0.y = fma(v[k].y, uu[k], a0.y);
      a1.x = fma(v[k + 1].x, uu[k + 1], a1.x);
      a1.y = fma(v[k + 1].y, uu[k + 1], a1.y);
    }
  }
  sm[threadIdx.x] = make_double2(a0.x + a1.x, a0.y + a1.y);  // slot rl * LG + cl
  __syncthreads();
  if (rl == 0 && act) {
    double2 t = sm[cl];
    for (int q = 1; q < NR; ++q) t.x += sm[q * LG + cl].x, t.y += sm[q * LG + cl].y;
    double* o = part + (int64_t)blockIdx.x * ostride + 2 * c2;
    o[0] = t.x;
    if (2 * c2 + 1 < C) o[1] = t.y;
  }
}

namespace {
int pow2_at_least(int64_t v, int cap) {
  int g = 1;
  while (g < cap && g < v) g <<= 1;
  return g;
}
int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
}  // namespace

// Form selection (measured: DESIGN.md section 8b).  rowdot: C <= kDenseShortMax -> lane groups, several rows per wave; up to
// kDenseMediumMax -> four rows per wave, one segment; longer rows: fewer than kDenseSegMaxRows of them, long enough for two segments
// of >= 2048 doubles -> four rows per wave and segment, about 2048 waves; else one wave per row.  colsum: C < 128 -> narrow (at most 512 slabs); else column tiles with slabs sized for about 4 workgroups
// per CU (a slab has at least 64 rows), which is the one-slab form where the tiles alone are that many or R is small.
void dense_plan(DenseDev& D, int force_rd, int force_cs, int seg_knob, int slab_knob) {
  const int64_t R = D.R, C = D.C;
  D.rd_group = pow2_at_least(C >> 1, 64);
  int64_t seg;
  if (seg_knob > 0) {
    seg = std::min<int64_t>(std::max<int64_t>(seg_knob & ~1, 64), (int64_t)1 << 22);
  } else {
    const int64_t want = std::max<int64_t>(1, std::min(ceil_div(C, 2048), ceil_div(2048, ceil_div(R, kDenseSegRows))));
    seg = round_up(ceil_div(C, want), 512);
  }
  int64_t nseg = ceil_div(C, seg);
  int rd = C <= kDenseShortMax ? kRdShort : (C <= kDenseMediumMax || (R < kDenseSegMaxRows && nseg >= 2)) ? kRdSeg : kRdWave;
  if (force_rd >= kRdShort && force_rd <= kRdSeg) rd = force_rd;
  D.rd_form = rd;
  D.rd_seg = rd == kRdSeg ? seg : 0;
  D.rd_nseg = rd == kRdSeg ? (int)nseg : 0;

  const int64_t npair = (C + 1) >> 1, ntile = ceil_div(C, kDenseTileCols);
  D.cs_group = pow2_at_least(npair, 64);
  int cs = C < kDenseTileCols ? kCsNarrow : kCsSlab;
  if (force_cs >= 1 && force_cs <= 3) cs = kCsSlab + force_cs - 1;
  int64_t slab;
  if (cs == kCsOne) {
    slab = R;
  } else if (slab_knob > 0) {
    slab = std::min<int64_t>(std::max<int64_t>(slab_knob, 1), (int64_t)1 << 22);
  } else if (cs == kCsNarrow) {
    const int64_t trip = kTPB / D.cs_group;
    slab = ceil_div(R, std::max<int64_t>(1, std::min<int64_t>(512, R / (8 * trip))));
  } else {
    slab = ceil_div(R, std::max<int64_t>(1, std::min(ceil_div(4 * kNumCU, ntile), R / 64)));
  }
  slab = std::min(slab, R);
  int64_t nslab = ceil_div(R, slab);
  if (cs == kCsSlab && nslab == 1 && force_cs == 0) cs = kCsOne;
  D.cs_form = cs;
  D.cs_slab = slab;
  D.cs_nslab = (int)nslab;
}

hipError_t launch_dense_rowdot(const DenseDev& D, const double* x, double* out, int64_t pad, hipStream_t s) {
  constexpr int NW = kTPB / 64;
  if (D.rd_form == kRdShort) {
    const int64_t per = kDenseShortRows * (kTPB / D.rd_group);
    hipLaunchKernelGGL(k_dense_rowdot_short, dim3((unsigned)ceil_div(D.R, per)), dim3(kTPB), 0, s, D.S, D.ld, D.R, D.C, D.rd_group, x, out, pad);
  } else if (D.rd_form == kRdWave) {
    hipLaunchKernelGGL(k_dense_rowdot_wave, dim3((unsigned)ceil_div(D.R, NW)), dim3(kTPB), 0, s, D.S, D.ld, D.R, D.C, x, out, pad);
  } else {
    const int64_t pstride = round_up(D.R, kPadDoubles);
    hipLaunchKernelGGL(k_dense_rowdot_seg, dim3((unsigned)ceil_div(ceil_div(D.R, kDenseSegRows) * D.rd_nseg, NW)), dim3(kTPB), 0, s, D.S, D.ld,
                       D.R, D.C, x, D.rd_nseg, D.rd_seg, D.rd_part, pstride, out, pad);
    if (D.rd_nseg == 1) return hipSuccess;
    hipLaunchKernelGGL(k_dense_fold, dim3((unsigned)ceil_div(pad, kTPB / kDenseFoldSub)), dim3(kTPB), 0, s, D.rd_part, D.rd_nseg, pstride, out,
                       D.R, pad);
  }
  return hipSuccess;
}

hipError_t launch_dense_colsum(const DenseDev& D, const double* u, double* out, int64_t pad, hipStream_t s) {
  const int64_t ostride = round_up(D.C, kPadDoubles);
  if (D.cs_form == kCsNarrow) {
    const int64_t npair = (D.C + 1) >> 1;
    hipLaunchKernelGGL(k_dense_colsum_narrow, dim3((unsigned)D.cs_nslab, (unsigned)ceil_div(npair, D.cs_group)), dim3(kTPB), 0, s, D.S, D.ld,
                       D.R, D.C, D.cs_group, u, D.cs_part, ostride, D.cs_slab);
  } else {
    const int ntile = (int)ceil_div(D.C, kDenseTileCols), tw = (int)ceil_div((D.C + 1) >> 1, ntile);
    const int direct = D.cs_form == kCsOne;
    hipLaunchKernelGGL(k_dense_colsum, dim3((unsigned)((int64_t)ntile * D.cs_nslab)), dim3(kTPB), 0, s, D.S, D.ld, D.R, D.C, u,
                       direct ? out : D.cs_part, ostride, D.cs_slab, ntile, tw, pad, direct);
    if (direct) return hipSuccess;
  }
  hipLaunchKernelGGL(k_dense_fold, dim3((unsigned)ceil_div(pad, kTPB / kDenseFoldSub)), dim3(kTPB), 0, s, D.cs_part, D.cs_nslab, ostride, out, D.C,
                     pad);
  return hipSuccess;
}

}  // namespace lz
