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

}  // namespace lz
