/*
 * lanczos_hip.h - C ABI of liblanczos_hip.so (MI355X / gfx950 Lanczos hot path).
 *
 * The reference (jgslunde/Lanczos) has no FFI layer: its only interface is the
 * Python class surface of Python/Regular/Lanczos.py:11-337 and
 * Python/Irregular/IrrLanczos.py:12-554, whose "GPU backend" is a run of CuPy
 * library calls.  Each entry point below therefore cites the CuPy/NumPy call
 * sites of the reference that it replaces (paths relative to /root/reference).
 * The Python host mirror of the class surface lives in lanczos_amd/ and reaches
 * this library through ctypes only (no torch types cross this boundary).
 *
 * Conventions
 *   - every function returns an int status: 0 = LZ_OK, negative = error;
 *     lz_last_error(h) returns a human-readable message for the last failure.
 *   - the caller owns all host buffers (pointer + explicit sizes); the library
 *     owns all device memory behind the opaque handle.
 *   - fp64 values, int32 CSR indices, row-major everywhere.
 *   - one handle = one GPU = one rank.  A handle is not thread-safe.
 *   - distributed runs: the basis, r and the matrix are row-block partitioned;
 *     "local" sizes refer to this rank's rows.
 */
#ifndef LANCZOS_HIP_H
#define LANCZOS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lz_context* lz_handle;

enum lz_status {
  LZ_OK = 0,
  LZ_WARN_BREAKDOWN = 1, /* lz_run finished, but a residual norm beta fell to <= 64 eps * max(|alpha|, |beta|) or a
                            coefficient is not finite: the Krylov space is exhausted.  The reference divides blindly
                            (Lanczos.py:113) and carries on with rounding noise / inf / NaN; the coefficients are
                            delivered exactly as computed, this status is the only difference. */
  LZ_ERR_ARG = -1,       /* bad argument / shape */
  LZ_ERR_HIP = -2,       /* HIP runtime error */
  LZ_ERR_COMM = -3,      /* RCCL / host-collective error */
  LZ_ERR_STATE = -4,     /* call order violated (e.g. run before set_csr) */
  LZ_ERR_NOMEM = -5,     /* device allocation failed */
  LZ_ERR_NODEVICE = -6   /* no usable GPU */
};

/* flags for lz_run / lz_set_options */
enum lz_flags {
  LZ_FLAG_NONE = 0,
  LZ_FLAG_PROFILE = 1,        /* bracket every hot kernel with hipEvents (lz_get_timings) */
  LZ_FLAG_QTW_MFMA = 2,       /* kernel-bench build only (retired A/B arm, 20 % slower): the v_mfma_f64_16x16x4_f64 Q^T w
                                 kernel; the product library refuses it (default: the 4x4x4 MFMA kernel)              */
  LZ_FLAG_QTW_VALU = 4,       /* the VALU + wave-shuffle Q^T w kernel (also the automatic fallback beyond ~5000 basis rows) */
  LZ_FLAG_SPMV_SCALAR = 8,    /* force the plain one-thread-per-row CSR kernel            */
  LZ_FLAG_FUSED_NORM = 16,    /* ||r||^2 rides with the Q^T r sums: pass 1 dots the raw residual, the update kernel forms
                                 beta, c_i = (V_i.r)/beta and V[j] = r/beta (one pass over V[j] and, at N > 1, one all-reduce
                                 less).  The Python layers set it by default; 0 = scale first, then dot (reference order) */
  LZ_FLAG_SPMV_STREAM = 32,   /* force the generic CSR-stream kernel (no fixed-K fast path) */
  LZ_FLAG_OVERLAP_HALO = 128, /* multi-rank, contiguous (stencil) halos: update the faces of V[j] first, exchange them on a
                                 second stream while the interior is updated; the SpMV waits on an event (opt-in)    */
  LZ_FLAG_ONE_REDUCE = 256,   /* opt-in, multi-rank runs: ONE all-reduce per iteration.  Pass 1 dots the basis against two
                                 columns at once on the matrix cores - r'' = A v_j - beta v_{j-1} and v_j - so that alpha_j, the
                                 coefficients V_i.(r'' - alpha_j v_j) = V_i.r'' - alpha_j V_i.v_j and |r|^2 = r''.r'' - 2 alpha_j
                                 v_j.r'' + alpha_j^2 v_j.v_j all come out of one reduced buffer (implies LZ_FLAG_FUSED_NORM).
                                 Same mathematics, different rounding (the three-term update subtracts beta v_{j-1} first, |r|^2
                                 is formed from three sums whose relative error is ~eps (alpha^2 + beta^2) / beta^2): not
                                 bit-identical to the default, and within 1e-10 only while |alpha| is not >> beta.  A guard
                                 watches exactly that: when |r|^2 falls below 1e-4 of r''.r'' (or is not positive) at any
                                 step, lz_run REPEATS the solve on the default loop and lz_last_engine reports 5 - the
                                 delivered coefficients then are the default loop's, bit for bit.
                                 With LZ_FLAG_REORTH_PARTIAL (round 5, lz_last_engine 8): the device-decided partial loop with
                                 ONE all-reduce + one exchange per iteration, sweep or no sweep (instead of three + one): the
                                 one reduced buffer carries alpha's partial, the three self terms of |r|^2 and - in a step
                                 that sweeps - the basis dots; the sweep decision is a one-step look-ahead of Simon's
                                 recurrence taken from reduced sums only, so every rank agrees (lz_last_sweep_misses counts
                                 the vectors the look-ahead should have swept and did not; they are swept one step late).
                                 Same guard; a repeat runs the three-collective partial loop (engine 5).              */
  LZ_FLAG_TRL_PASS2_ALWAYS = 512, /* thick-restart Lanczos (lz_trl_extend): run the second Gram-Schmidt pass at every step instead of
                                     only where the DGKS criterion asks for it (tests) */
  LZ_FLAG_REORTH_PARTIAL = 64, /* opt-in: partial re-orthogonalisation (Simon 1984).  The reference sweeps the whole basis
                                 every step; with this flag the sweep (same kernels, same arithmetic) runs only when the
                                 omega-recurrence estimate of the loss of orthogonality exceeds sqrt(eps), on that and the
                                 next step.  The recurrence and the decision live on the device (no host synchronisation
                                 inside lz_run: lz_last_host_syncs).  The basis stays semi-orthogonal (<= sqrt(eps)), which keeps T - and so the
                                 Ritz values - within O(eps ||A||) of the full-sweep run; V itself differs at that level. */
  LZ_FLAG_TRL_FILTER_UNFUSED = 1024 /* thick-restart Lanczos with a Chebyshev filter (lz_trl_set_filter): form every filter step as the
                                        plain SpMV plus the streaming recurrence kernel also where the SpMV has the fused epilogue
                                        (fixed-K stencil matrices): same bits, 16 more bytes per row (A/B, tests) */
};

/* kernel classes reported by lz_get_timings */
enum lz_kernel_class {
  LZ_K_SPMV = 0,     /* r = A v_j with fused alpha partials             */
  LZ_K_QTW = 1,      /* v_j = r/beta; c = Q^T v_j (reorth pass 1)        */
  LZ_K_UPDATE = 2,   /* v_j = 2 v_j - Q c        (reorth pass 2)        */
  LZ_K_THREE = 3,    /* r = r - alpha v_j - beta v_{j-1}; ||r||^2        */
  LZ_K_FINAL = 4,    /* tiny second-stage reductions                    */
  LZ_K_COMM = 5,     /* all-reduce / halo exchange / all-gather         */
  LZ_K_RITZ = 6,     /* Y = V^T-layout GEMM (FP64 MFMA)                 */
  LZ_K_COUNT = 7
};

typedef struct lz_timings {
  double ms[LZ_K_COUNT];             /* summed device time of the TIMED launches per class (hipEvent)   */
  double timed_bytes[LZ_K_COUNT];    /* ALGORITHMIC bytes of the timed launches    */
  int64_t timed_launches[LZ_K_COUNT];/* launches bracketed by events (all of them, or 1 iteration in     */
                                     /* `stride` when lz_set_tuning(h, 7, stride) samples the profiling) */
  double bytes[LZ_K_COUNT];          /* algorithmic bytes of ALL launches per class                      */
  double flops[LZ_K_COUNT];          /* algorithmic flops of all launches per class                      */
  int64_t launches[LZ_K_COUNT];      /* number of launches per class                                     */
  double total_ms;                   /* device time of the whole lz_run(s) (events)                      */
} lz_timings;

/* ---- library / device ------------------------------------------------- */
int lz_version(void);
int lz_device_count(int* count);
/* Replaces: `import cupy as np` backend switch, Lanczos.py:85-88. */
int lz_create(lz_handle* out, int device_id);
int lz_destroy(lz_handle h);
const char* lz_last_error(lz_handle h); /* h may be NULL: last error of lz_create */
int lz_set_options(lz_handle h, int flags);
/* Tuning knobs; they take effect at the next lz_set_csr / lz_basis_alloc / lz_run / lz_ritz_vectors, and results never depend
 * on them beyond summation order.
 *    0  Q^T w slice length per block            1  Q^T w kernel variant (unroll / rows per tile)
 *    2 / 4  CSR-stream rows / entries per block  5  fixed-K rows per block
 *    6  issue the collectives even when world == 1 (tests of the RCCL calls with a 1-rank communicator)
 *    7  profile only every value-th iteration of lz_run
 *    8  update-kernel variant (1 cached loads, 2 one position per lane, 3/4/5 slice owner with 8/4/1 positions per lane)
 *    9  Ritz back-transform kernel: 0 auto (33..128 columns: S resident in LDS, 32-row tiles; 129..200: S-stationary, S in
 *       registers; else one workgroup per 128 rows), 1 the latter always
 *   10  irregular SpMV: entries per row block   12  1 = no row-stride skew
 *   13  1 = NaN-poison a fresh basis allocation before the required parts are cleared (test knob)
 *   14  irregular SpMV plan (0 auto: the column-blocked two-phase kernels for matrices without column locality, 1 never, 2 always)
 *   15  loop structure (0 auto: three launches per step for small problems, five up to 4e6 rows per rank, above that on one rank
 *       the one-sweep loop - one walk over the basis per step, lz_last_engine 9 -, else six; 1 six always; 6 the one-sweep loop
 *       at any size (one rank, fused-norm full re-orthogonalisation, default kernels, n <= 1536) - its fused form (no three-term
 *       pass, lz_last_one_sweep_fused) where the matrix has a scale-on-read SpMV, as the automatic choice does; 7 the one-sweep
 *       loop at any size with the separate three-term kernel always (A/B, tests).  Where the fused form applies, n >= 4 and
 *       n <= 1023, the automatic choice takes its PAIR form - one walk over the basis per two steps, lz_last_one_sweep_pairs;
 *       6 and 7 never do; 8 the one-sweep loop at any size with pairs; 9 the same with 16 instead of 8 positions per lane in
 *       the pair walk on long vectors (A/B).  Where the pair form applies, n >= 6 and n <= 512, the automatic choice takes the
 *       GROUP form instead - one walk over the basis per four steps, lz_last_one_sweep_quads; 6, 7, 8 and 9 never do; 10 the
 *       one-sweep loop at any size with groups; 11 the same with 8 instead of 4 positions per lane in the group walk on long
 *       vectors (A/B).  The chain of three steps before a group's walk works in the units of z - the chain vectors stay unscaled
 *       in their basis rows, the plain coded product runs on them, one launch adds ||z||^2 and z . A z, and x = z / b is formed by
 *       division wherever it is read (16 launches per group) - and the second-stage sums, post and the chat prediction behind the
 *       walk run on a side stream beside the closing product and the next chain (same arithmetic, same bits); 12 the group form at any
 *       size with the scaled chain through the scale-on-read SpMV (19 launches per group, everything on the main stream; A/B), 13 the
 *       group form at any size with the unscaled chain and no side stream (A/B))
 *   16  rows per chunk of the CHUNKED Ritz mode (0 auto: chunked only when Y does not fit beside the basis; > 0 forces it: tests)
 *   11  two-sided Gram-Schmidt links (0 / 1: streaming kernel + fold kernel per link)
 *   17  fixed-K (stencil) SpMV layout: 0 auto (CSR-order kernel with products staged through LDS; the ELL-ordered second copy -
 *       a lane owns whole rows - is built and used only by the partial re-orthogonalisation loop's fused SpMV; 27 entries per
 *       row, which have no CSR-order fixed-K kernel: ELL for every SpMV, 3 % faster than CSR-stream), 1 never ELL,
 *       2 ELL for every SpMV, one row per lane and trip, 3 ELL, two adjacent rows per lane (16-byte loads).
 *       Round 5: auto first looks for ROW CLASSES (lz_spmv_coding) - a coded ELL copy is every SpMV's default; 2 / 3 keep the uncoded
 *       copy (A/B), 4 codes the offsets only even where the values repeat as well (A/B)
 *   19  Gram matrix of the Ritz vectors: 0 auto (accumulator-stationary symmetric kernel, operands staged through LDS once per workgroup),
 *       1 the split-K TN GEMM always, 2 the symmetric kernel with per-wave register rings (round 4; also what an odd n runs)
 *   18  partial re-orthogonalisation loop: 0 auto (device-resident decisions, lz_last_engine 7), 1 the host-decided loop
 *       (two scalars read back per step; same bits), 2 device-resident but with the separate scale pass (no fused r / beta),
 *       3 device-resident with pass 1's second-stage sums as a kernel of their own (default: pass 1's last block adds them)
 *   23  fully row-class coded SpMV (lz_spmv_coding == 2): 0 auto (two ADJACENT rows per lane: 16-byte gathers, half the vector-memory
 *       instructions), 1 / 3 one row per lane and trip with one / two 512-row units per workgroup (A/B; same bits in every form - the
 *       alpha partials are per unit and per the one-row-per-lane lane mapping)
 *   22  irregular (two-phase) SpMV: interleave its two phases over this many groups of row blocks (A/B arm of round 5: the product
 *       stream of a group could stay in the Infinity Cache between the phases; measured 8-110 % slower - DESIGN.md section 4; kernel-bench
 *       build only; 0 / 1 = off)
 *   21  Gram matrix: number of K slices (workgroups per unit) of the symmetric kernel; 0 auto (whole residency rounds of 256)
 *   20  one-reduce partial loop (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE): safety factor kappa of the look-ahead sweep
 *       decision (a sweep is due when kappa * max |predicted omega| > sqrt(eps); 0 = the default, 4)
 * The dense operator of lz_gk_set_dense reads three of these at that call, each in the sense it already has: 14 (the SpMV plan) forces
 * its product forms, 4 (entries per segment of a long row) is its segment length, 2 (rows per block) its slab height - see there.
 * The product library returns LZ_ERR_ARG for everything that lives only in the kernel-bench build (make KBENCH=1 ->
 * liblanczos_kbench.so, loaded by tools/ and by the tests of those arms; sources: lz_small.hip, lz_*_kbench.h): the A/B arms
 * retired in round 3 because they measured slower - the one-kernel and one-launch-per-step engines
 * (15 = 2, 3, 5), the persistent / LDS-staged / 16-row-tile Ritz GEMMs (9 = 2, 3, 4, 6), the ticket / deferred-fold two-sided links
 * (11 = 2, 3), the two-phase SpMV's row-block-group interleaving (22 >= 2), and LZ_FLAG_QTW_MFMA (lz_set_options).  The timing-only ablation arms of rounds 1-4 (kernel variants that computed
 * wrong results on purpose: knob 1 >= 20, knob 3, knob 9 >= 10) were deleted from both builds in round 5. */
int lz_set_tuning(lz_handle h, int index, int value);
/* "hip=<path of the libamdhip64 this library is bound to>;rccl=<path of the librccl it dlopened, or empty>".
 * RCCL is always taken from the directory of that HIP runtime (LZ_RCCL_PATH overrides): see DESIGN.md section 6 and LAB_NOTEBOOK.md section 5. */
int lz_runtime_info(char* buf, size_t buflen);
int lz_device_synchronize(lz_handle h);
/* free / total device memory of the handle's GPU as the runtime reports it (hipMemGetInfo): the figure the resident-versus-chunked
 * decision of lz_ritz_vectors is taken on; tests use it to see that lz_destroy gives everything back */
int lz_device_memory(lz_handle h, int64_t* free_bytes, int64_t* total_bytes);
int lz_device_name(lz_handle h, char* buf, size_t buflen);
/* vectors are padded to 256-byte multiples on the device; in halo mode the ghost
 * entries of the extended local vector start at index lz_padded_rows(rows_local). */
int64_t lz_padded_rows(int64_t rows);

/* ---- distributed setup (optional; default is a single rank) ------------
 * The reference has no communication layer; the
 * partition below is this build's own design: rows are split in contiguous
 * blocks, alpha/beta/c are summed with an all-reduce, and the SpMV input is
 * exchanged either as neighbour halos (send/recv lists) or as an all-gather. */
int lz_comm_load(void);                           /* dlopen RCCL now (optional; lz_comm_* do it lazily) */
int lz_comm_unique_id(void* id, size_t id_bytes); /* >= 128 bytes; rank 0 calls, host broadcasts */
int lz_comm_init_rccl(lz_handle h, int world, int rank, const void* id, size_t id_bytes);
/* host-staged collectives (tests / fallback): the library copies device data to
 * the given host buffer, calls back, and copies the result to the device. */
typedef int (*lz_host_allreduce_fn)(void* user, double* buf, int64_t count);
/* peers/send_counts/recv_counts have npeers entries; sendbuf/recvbuf are the
 * concatenated per-peer segments in peer order. */
typedef int (*lz_host_exchange_fn)(void* user, int npeers, const int32_t* peers, const double* sendbuf,
                                   const int64_t* send_counts, double* recvbuf, const int64_t* recv_counts);
/* allgather: sendbuf (count doubles) -> recvbuf (world*count doubles) */
typedef int (*lz_host_allgather_fn)(void* user, const double* sendbuf, double* recvbuf, int64_t count);
int lz_comm_init_host(lz_handle h, int world, int rank, lz_host_allreduce_fn ar, lz_host_exchange_fn ex,
                      lz_host_allgather_fn ag, void* user);

/* ---- matrix ----------------------------------------------------------- *
 * Replaces: cupyx.scipy.sparse.csr_matrix(H, dtype=float64), Lanczos.py:88
 * (csc_matrix in IrrLanczos.py:205; a symmetric CSC is the same arrays).
 * Single rank: rows_local == M_global, ncols_ext == M_global.
 * Multi rank : this rank's row block; colidx index the EXTENDED local vector
 *   [ owned rows (rows_local) | ghost entries ... ] of length ncols_ext
 *   (halo mode, see lz_set_halo) or the padded global vector (all-gather mode,
 *   see lz_set_allgather). */
int lz_set_csr(lz_handle h, int64_t M_global, int64_t row0, int64_t rows_local, int64_t ncols_ext, int64_t nnz,
               const int32_t* rowptr, const int32_t* colidx, const double* vals);
/* Dense row-major A (M x M), single rank only.  Replaces the dense->CSR
 * conversion the reference's GPU path performs for ndarray input
 * (1Dbox.py:27 -> Lanczos.py:88) with a real dense GEMV. */
int lz_set_dense(lz_handle h, int64_t M, const double* A);
/* Row block [row0, row0 + rows_local) of a dense symmetric A split over ranks (the north star's dense multi-GPU case;
 * nothing to mirror in the single-process reference).  A is rows_local x ncols_ext row-major with the columns laid out
 * like the all-gathered vector: rank q's entries at [q * chunk, q * chunk + rows_q), zero columns in the padding
 * (ncols_ext = world * chunk; follow with lz_set_allgather(h, chunk)).  One rank: rows_local = ncols_ext = M_global. */
int lz_set_dense_block(lz_handle h, int64_t M_global, int64_t row0, int64_t rows_local, int64_t ncols_ext, const double* A);
/* Assemble the reference's regular-grid Hamiltonian directly in device CSR (replaces the
 * Python-loop COO build of Python/Regular/Hamiltonian.py:45-128 plus `H = -T + V; H.sort_indices()` of
 * 3Ddeuteron.py:80-81): periodic N^3 grid, flat index x + y N + z N^2, `points` = 7 or 27, weights4 =
 * {centre, face, edge, corner} as the host computed them (7-point uses the first two).  Entries are
 * T_factor * w (negated if negate_T), plus potential[row] (N^3 host doubles, may be NULL) on the diagonal;
 * columns sorted.  The matrix becomes the handle's operator, exactly as after lz_set_csr. */
int lz_build_stencil3d(lz_handle h, int N, int points, double T_factor, const double* weights4, const double* potential,
                       int negate_T);
/* The same assembly for a Nx x Ny x Nz grid and for ONE RANK'S ROW BLOCK [row0, row0 + rows_local) of it (the 8-GPU form of
 * BASELINE config C4 assembles its 1.25e7-row slab in place; nothing to mirror in the single-process reference).
 * Columns are renumbered into the extended local vector of halo mode: owned rows first, then the ghost entries, given
 * as nranges <= 16 contiguous GLOBAL index ranges in the order they occupy the ghost tail (what lanczos_amd.partition
 * plans for a stencil slab; follow with lz_set_halo).  rows_local == Nx Ny Nz: whole matrix, global columns.
 * potential_kind 0: none; 1: `potential` = rows_local host doubles (this rank's diagonal); 2: `potential` = 8 parameters
 * {eCore, rCore, eWell, rWell, power, Lx, Ly, Lz} of the deuteron hard core + well of 3Ddeuteron.py:51-61,
 * eCore exp(-(r/rCore)^power) - eWell exp(-(r/rWell)^power), evaluated ON THE DEVICE at np.linspace(-L/2, L/2, N)
 * coordinates (replaces the point-by-point host loop of Hamiltonian.py:38-43; device exp/pow differ from NumPy's in the
 * last bits, so the bit-exact-vs-reference builder keeps kind 1). */
int lz_build_stencil3d_block(lz_handle h, int Nx, int Ny, int Nz, int points, double T_factor, const double* weights4,
                             int potential_kind, const double* potential, int negate_T, int64_t row0, int64_t rows_local,
                             int nranges, const int64_t* ghost_start, const int64_t* ghost_len);
int lz_csr_info(lz_handle h, int64_t* rows, int64_t* nnz);
/* which SpMV kernel the current matrix + options select: 0 scalar CSR (LZ_FLAG_SPMV_SCALAR), 1 CSR-stream, 2 fixed-K
 * (stencils), 3 column-blocked two-phase (matrices without column locality, lz_spmv_pb.hip), 4 dense GEMV */
int lz_spmv_plan(lz_handle h, int* plan);
/* Row-class coding of a fixed-K (stencil) matrix (round 5): where the rows of the matrix fall into <= 256 classes up to translation -
 * the K offsets col - row, and for constant coefficients the K values too - the SpMV streams ONE BYTE per row (the class; + 8 bytes per
 * entry when only the offsets repeat) instead of 12 bytes per entry; found and verified on the device at lz_set_csr, same products in the
 * same order (same bits).  coding: 0 none, 1 offsets by class (values streamed), 2 offsets and values by class, 3 offsets and the
 * values OFF the diagonal by class with the diagonal's values streamed (8 more bytes per row: a constant-coefficient stencil plus a
 * potential - the reference's Hamiltonians); classes: how many. */
int lz_spmv_coding(lz_handle h, int* coding, int* classes);
/* download the handle's CSR matrix (sizes from lz_csr_info) */
int lz_get_csr(lz_handle h, int32_t* rowptr, int32_t* colidx, double* vals);
/* halo plan: for peer p (npeers of them) send x[send_idx[..]] (local row
 * indices, send_counts[p] of them, concatenated) and receive recv_counts[p]
 * doubles into the ghost region, in peer order. */
int lz_set_halo(lz_handle h, int npeers, const int32_t* peers, const int64_t* send_counts, const int32_t* send_idx,
                const int64_t* recv_counts);
/* all-gather plan: every rank owns `chunk` padded rows; x_full has world*chunk entries. */
int lz_set_allgather(lz_handle h, int64_t chunk);

/* Optional: allocate the device buffers of the coming run EARLY - the (n, rows_local) Krylov basis (with_ritz 0 or 1) and, where
 * it fits, the (rows_local, n) Ritz vectors (with_ritz 1; with_ritz 2: the Ritz vectors ONLY - what the helper thread asks for
 * while the solve already runs on the basis).  A hipMalloc of 16 GB costs 0.2 ms most of the time and 0.1 - 4 s now and then on
 * this platform (since round 5 buffers of this size are a reserved virtual range backed by physical chunks, which has not been
 * seen to stall: tools/probes/alloc_pattern_probe.hip); the
 * class mirror issues this call from a helper thread while it draws the start vector, hashes, validates and uploads the
 * matrix (Lanczos.py:85-104 does the same work in sequence), so lz_run / lz_ritz_vectors find their buffers ready.  It is the
 * ONE entry point that may run concurrently with another call on the same handle (lz_set_options / lz_set_tuning / lz_set_csr /
 * lz_set_dense / lz_build_stencil3d*): it touches only its own fields.  It must have returned before lz_run.  Never fails
 * for lack of memory (lz_run then allocates, and reports, itself); reserves nothing unless a quarter of the device stays free.
 * Single rank (rows_local = M). */
int lz_reserve(lz_handle h, int64_t rows_local, int n, int with_ritz);

/* ---- the Lanczos run --------------------------------------------------- *
 * Replaces Lanczos.py:104-119 (== IrrLanczos.py:222-238): basis allocation,
 * warm-up step and the Krylov loop with full re-orthogonalisation, with the
 * reference CPU branch's arithmetic (reorthogonalize, Lanczos.py:247-249).
 * v0_local: this rank's rows of the NORMALISED start vector (Lanczos.py:93-100
 * is done by the host mirror with NumPy's legacy RNG).  alpha_out[n],
 * beta_out[n-1] (n >= 2) receive the recurrence coefficients (replicated on all
 * ranks); beta follows the reference's indexing (beta[j-1] set at step j). */
int lz_run(lz_handle h, int n, const double* v0_local, double* alpha_out, double* beta_out);
/* ---- checkpoint / resume (SURVEY.md section 5 hook; nothing to mirror: the reference keeps no solver state on disk) ----
 * After lz_run(h, n1, ...) the state (V[0..n1), r, alpha[0..n1), beta[0..n1-1)) is everything the recurrence needs to go on at
 * step n1: lz_get_basis / lz_get_residual + the coefficient arrays are a checkpoint.  lz_get_residual: r = H v_{n1-1} -
 * alpha_{n1-1} v_{n1-1} - beta_{n1-2} v_{n1-2} (Lanczos.py:119 after the last step), this rank's rows.
 * lz_run_resume continues such a run to n > j0 steps in total: V_rows is (j0, rows_local) row-major with leading dimension
 * ldv_in, alpha_in has j0 and beta_in j0 - 1 entries.  Steps j0 .. n-1 run on the plain six-launch loop (every loop
 * structure produces the same bits), so alpha_out[n], beta_out[n-1] and the basis equal those of an uninterrupted
 * lz_run(h, n, ...) BIT FOR BIT (same options).  Not with LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE (LZ_ERR_STATE). */
int lz_get_residual(lz_handle h, double* r_local);
/* The same for LZ_FLAG_REORTH_PARTIAL's device-decided loop (engine 7; round 5): its checkpoint also carries the omega-recurrence
 * state - lz_get_omega_state after a run of j0 steps: 2 + (j0 + 2) + 3 (j0 + 1) doubles [||A|| estimate, "sweep the next vector too",
 * the norms hb[k] that formed V[k], three rows of omega] - and lz_run_resume_partial continues from it (j0 >= 2): the decision of step j0
 * is taken from the refreshed ||r||^2 exactly as the uninterrupted run took it, so coefficients, basis and sweep schedule of the
 * continued run equal an uninterrupted n-step run bit for bit.  lz_last_sweeps / lz_last_sweep_log then cover the steps j0 .. n-1. */
int lz_get_omega_state(lz_handle h, double* out, int64_t count);
int lz_run_resume_partial(lz_handle h, int n, int j0, const double* V_rows, int64_t ldv_in, const double* r_local, const double* alpha_in,
                          const double* beta_in, const double* omega_state, double* alpha_out, double* beta_out);
int lz_run_resume(lz_handle h, int n, int j0, const double* V_rows, int64_t ldv_in, const double* r_local, const double* alpha_in,
                  const double* beta_in, double* alpha_out, double* beta_out);
/* Krylov basis, row-major (n, rows_local): basis vector j is row j
 * (replaces cp.asnumpy(V.T), Lanczos.py:136; the mirror exposes the transposed view).
 * Result publication: device -> host copies of 192 MB and more (this call, lz_get_basis_block, lz_ritz_vectors with Y_out,
 * lz_get_ritz_vectors / lz_get_ritz_rows) go through a ring of pinned staging buffers (6 x 32 MB per handle, created at the
 * first such copy) emptied by host copy threads: 40-45 GB/s into fresh pageable NumPy memory instead of the 15-21 GB/s of a
 * plain hipMemcpy (tools/publish_probe.py).  Environment LZ_XFER_THREADS = number of copy threads (default 6; 0 = plain copy). */
int lz_get_basis(lz_handle h, double* V_out, int64_t ld);
/* the entries [row0, row0 + nrows) of every basis vector: (n, nrows) row-major with leading dimension ld >= nrows (a window
 * of V when the whole (n, rows_local) array is too large to move: BASELINE config C4, 160 GB) */
int lz_get_basis_block(lz_handle h, int64_t row0, int64_t nrows, double* V_out, int64_t ld);
/* Ritz back-transform Y = V_cols * S  (Lanczos.py:153-156: n GEMVs np.dot(V, S[:, i])):
 * S is (n, n) row-major (columns = eigenvectors of H_eff), Y_out is (rows_local, n) row-major or NULL (Y stays on the
 * device for the checks and is fetched later, whole or by rows).  Never fails for lack of room for Y: see lz_ritz_info. */
int lz_ritz_vectors(lz_handle h, const double* S, double* Y_out);
/* copy the Y of the last lz_ritz_vectors call to the host: (rows_local, n) row-major */
int lz_get_ritz_vectors(lz_handle h, double* Y_out);
/* rows [row0, row0 + nrows) of that Y: (nrows, n) row-major.  This is how H_eigvecs (Lanczos.py:60-66) is served when the
 * whole (M, n) array fits neither beside the basis on the device nor on the host. */
int lz_get_ritz_rows(lz_handle h, int64_t row0, int64_t nrows, double* Y_out);
/* How the last lz_ritz_vectors call is held.  *chunk_rows = 0: Y is resident on the device; > 0: CHUNKED mode - a second
 * rows_local x n array does not fit beside the basis (BASELINE config C4 on one GPU: 160 GB + 160 GB), so the device keeps
 * S and a buffer of that many rows, and lz_get_ritz_rows / lz_get_ritz_vectors / lz_ritz_gram / lz_ritz_quality re-form the
 * rows (or column batches) they need from the basis: a 16-row tile of Y depends only on the same 16 columns of V.
 * lz_set_tuning(h, 16, rows) forces the chunked mode (tests).
 * clock4 (may be NULL; zeros unless one of the persistent kernels ran - n <= 200 with enough rows): {shader clock in MHz while
 * the kernel ran (s_memtime cycles / s_memrealtime ticks of the constant 100 MHz counter over workgroup 0's trip), shader
 * cycles workgroup 0 needed per 16-row tile of one of its waves, the MFMA issue floor for that in cycles (MFMAs per tile
 * and SIMD x 64), 16-row tiles walked by that wave}. */
int lz_ritz_info(lz_handle h, int64_t* chunk_rows, double* clock4);
/* Device-side versions of the two checks get_H_eigs runs on Y (Lanczos.py:157-158,
 * 288-323): column norms (n) and the (n, n) Gram matrix Y^T Y, computed on the
 * device-resident Y of the last lz_ritz_vectors call (summed over ranks). */
int lz_ritz_gram(lz_handle h, double* gram_out);
/* In-kernel clock record of the last lz_ritz_gram when it ran the accumulator-stationary symmetric kernel (48 <= n <= 208, at
 * least 4096 rows; zeros otherwise): {shader clock in MHz while workgroup 0 ran, shader cycles its wave 0 needed per k-step
 * (4 rows of Y), the MFMA issue floor of that (MFMAs per k-step and SIMD x 64 cycles), k-steps walked}. */
int lz_gram_info(lz_handle h, double* info4);
/* y_i = A * Y[:, i] residual check used by print_good_eigs (Lanczos.py:166-185):
 * out[i] = (A y_i . y_i)^2 / (||A y_i||^2), for all n columns.  One rank: one fused kernel over the CSR matrix.
 * Row-block partition (world > 1): collective; every Ritz vector is exchanged and multiplied like a Lanczos vector
 * (CSR or dense), the 2 n sums travel in one all-reduce, every rank receives the same n values. */
int lz_ritz_quality(lz_handle h, double* out);
int lz_get_timings(lz_handle h, lz_timings* out);
/* The collectives behind lz_timings.launches[LZ_K_COMM] of the interval the LAST lz_get_timings closed, by kind: all-reduces
 * (alpha / ||r||^2 / coefficient sums) and SpMV-input exchanges (halo send/recv group or all-gather). */
int lz_comm_counts(lz_handle h, int64_t* allreduces, int64_t* exchanges);
/* number of steps of the last lz_run that ran the re-orthogonalisation sweep (== n without LZ_FLAG_REORTH_PARTIAL) */
int lz_last_sweeps(lz_handle h, int* sweeps);
/* log[j] = 1 if step j of the last lz_run ran the sweep, j < n <= its number of steps (all 1 for the full-sweep loops; the device's own
 * record for the device-decided partial loops, engines 7 and 8; LZ_ERR_ARG after the host-decided loop of knob 18 = 1, which keeps none).
 * tests/ replay Simon's recurrence (and the look-ahead of engine 8) on the host from alpha / beta and hold the device to it. */
int lz_last_sweep_log(lz_handle h, int* log, int n);
/* LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE only (else 0): vectors of the last lz_run whose exact omega-recurrence estimate
 * exceeded sqrt(eps) although the one-step look-ahead gate had not swept them (lz_set_tuning(h, 20, kappa) sets the look-ahead's
 * safety factor, default 4). */
int lz_last_sweep_misses(lz_handle h, int* misses);
/* How the last lz_run was executed (choose_loop, lz_loops.hip).  0: six launches per step (also: the host-decided partial
 * re-orthogonalisation loop, every kernel A/B arm, more than 4e6 rows per rank).  7: LZ_FLAG_REORTH_PARTIAL with the decision on
 * the device (round 4, the default of that flag): the sweep kernels of every step are enqueued and return at once when the
 * device-side omega-recurrence says no sweep is due; with an ELL-ordered stencil matrix the SpMV forms r / beta itself.  2: the fused-launch path of small problems (a vector of at most eight
 * pass-1 slices, one rank, fused-norm mode): the second-stage reductions and the three-term recurrence ride in the prologue
 * of their consumer kernels - three launches per step, bit-identical results.  3: up to 4e6 rows per rank in fused-norm mode
 * with the full sweep: the three-term recurrence rides in the prologue of the next step's pass 1 (five launches per step,
 * bit-identical; not with LZ_FLAG_OVERLAP_HALO).  lz_set_tuning(h, 15, 1) selects 0 in both cases.  6: LZ_FLAG_ONE_REDUCE.
 * 8: LZ_FLAG_ONE_REDUCE | LZ_FLAG_REORTH_PARTIAL (one all-reduce per step, look-ahead sweep decision on the device).
 * 5: a one-reduce run whose cancellation guard fired and that was repeated on the default loop.  1 / 4: the one-kernel and
 * one-launch-per-step engines of the kernel-bench build (retired from the product library in round 3: bit-identical, not
 * faster - LAB_NOTEBOOK.md section 4). */
int lz_last_engine(lz_handle h, int* engine);
/* One-sweep loop (lz_last_engine 9): the steps of the last lz_run whose predicted coefficients missed the measured ones by more
 * than the gate (1e-14 in units of the new vector) and that therefore ran the correcting sweep; 0 after any other loop. */
int lz_last_gate_trips(lz_handle h, int* trips);
/* One-sweep loop: 1 when the last lz_run took the fused form - one rank, 5 or 7 entries per row in the ELL-ordered copy, n <= 1520:
 * the sweep forms w_j = (A v_{j-1} - alpha v_{j-1}) - beta v_{j-2} itself and works in the units of w, the SpMV divides by beta_j on
 * read and stores V[j]; no three-term kernel runs inside the loop.  0 for the unfused form (27-point rows, two-phase or dense
 * SpMV, lz_set_tuning(h, 15, 7)) and after any other loop.  Both forms report lz_last_engine 9. */
int lz_last_one_sweep_fused(lz_handle h, int* fused);
/* One-sweep loop, pair form: the number of pair walks behind the result the last lz_run returned - from step 2 on, one walk over
 * the basis finishes v_j and forms the un-normalised v_{j+1} (the SpMV of step j runs on the uncorrected w_j / beta_j, and what the
 * correction owes to w_{j+1} is applied as a combination of basis rows): (n - 2) / 2 pairs, an odd last step runs the single form.
 * 0 after the single forms, after any other loop, and after a run that abandoned its pairs.  lz_last_one_sweep_fused stays 1. */
int lz_last_one_sweep_pairs(lz_handle h, int* pairs);
/* 1 when the last run (lz_run or a resume) tried the pair form and a pair's prediction missed by more than the gate (1e-14): a pair has no correcting
 * sweep, so the whole run was repeated on the single fused form (what was returned is that run's result, bit for bit).  The handle
 * remembers it until a matrix is set again: later runs take the single form at once and report 0 here. */
int lz_last_pair_abandoned(lz_handle h, int* abandoned);
/* One-sweep loop, group form: the number of group walks behind the result the last lz_run returned - from step 2 on, three plain
 * Lanczos steps run with no walk at all and ONE walk over the basis then finishes four vectors, with coefficients predicted by the
 * omega-recurrence over the extended set: (n - 2) / 4 groups; a tail of two steps runs as a pair (lz_last_one_sweep_pairs is then 1),
 * a tail of one or three on the single form.  0 after the pair and single forms, after any other loop, and after a run that abandoned
 * its groups.  lz_last_one_sweep_fused stays 1. */
int lz_last_one_sweep_quads(lz_handle h, int* quads);
/* 1 when the last lz_run tried the group form and a group's prediction missed by more than the gate (1e-14): a group has no correcting
 * sweep, so the whole run was repeated on the pair form (which may itself fall back to the single form: lz_last_pair_abandoned).  The
 * handle remembers it until a matrix is set again: later runs take the pair form at once and report 0 here. */
int lz_last_quad_abandoned(lz_handle h, int* abandoned);
/* Host evaluation of the one-sweep loop's per-step arithmetic (the device kernels' expressions, summed in index order; the
 * kernels add the same terms lane-strided through a fixed shuffle tree), for checks without a GPU.  G (symmetric) and H are n x n with column i at [i * n].  predict: chat[0..j] of step j + 1 from alpha_j, the
 * norm beta_j that formed v_j and nrm2 = ||w_{j+1}||^2.  post: col[0..j) = G[:j, j] of the v_j formed with chat from the
 * measured dots d[i] = V_i . u_j, nrm2 = ||w_j||^2. */
int lz_one_sweep_host_predict(int n, int j, const double* H, const double* G, double alpha_j, double beta_j, double nrm2, double* chat);
int lz_one_sweep_host_post(int n, int j, const double* G, const double* d, const double* chat, double nrm2, double* col);
/* Host <-> device synchronisations the last run (lz_run or a resume) made between its first and its last launch (the final wait for
 * alpha / beta is not counted).  0 for every loop on one rank and over RCCL - including, since round 4, the partial re-orthogonalisation mode
 * (engine 7: Simon's omega-recurrence and the sweep decision live on the device; lz_set_tuning(h, 18, 1) selects the former
 * host-decided loop, engine 0, which reads two scalars back per step).  The host-staged collective backend (tests) counts two
 * per collective. */
int lz_last_host_syncs(lz_handle h, int64_t* syncs);

/* ---- single steps (unit parity tests drive the kernels one by one) ------ */
/* allocate a zeroed basis of n rows + r (what lz_run does first, Lanczos.py:104-107) */
int lz_basis_alloc(lz_handle h, int n);
int lz_basis_set_row(lz_handle h, int j, const double* row_local); /* host -> V[j] */
/* rows j0 .. j0 + count - 1 in one strided copy; rows_local: count rows of rows_local doubles, ld doubles apart (the (n, M) array
 * the static Lanczos.reorthogonalize(V, j) is handed, Lanczos.py:233) */
int lz_basis_set_rows(lz_handle h, int j0, int count, const double* rows_local, int64_t ld);
int lz_basis_get_row(lz_handle h, int j, double* row_local);       /* V[j] -> host */
int lz_r_set(lz_handle h, const double* r_local);
int lz_r_get(lz_handle h, double* r_local);
/* r = A V[j]; *dot_out = V[j] . r   (Lanczos.py:116-118) */
int lz_step_spmv(lz_handle h, int j, double* dot_out);
/* V[j] = r / ||r|| (if scale != 0; *beta_out = ||r||) then the reference's
 * reorthogonalize(V, j) over rows [0, nrows): c = V V[j]; V[j] = 2 V[j] - c^T V
 * (Lanczos.py:112-115, 247-249).  c_out[nrows] receives the coefficients. */
int lz_step_reorth(lz_handle h, int j, int nrows, int scale, double* beta_out, double* c_out);
/* r = r - alpha V[j] - beta V[jm1] (jm1 < 0: term skipped); *norm2_out = ||r||^2 (Lanczos.py:119,112) */
int lz_step_three_term(lz_handle h, int j, int jm1, double alpha, double beta, double* norm2_out);
/* One loop body of the one-sweep loop (engine 9) on a state set from the host: the single fused step (form 1), a pair (2) or a group
 * of four (4) at step j, by the same functions lz_run's loops call.  Before: lz_basis_alloc(n), rows 0 .. j-1 through
 * lz_basis_set_rows, lz_step_spmv(h, j - 1) for y = A V[j-1].
 * lz_os_state_set allocates and zeroes the loop's state for the n of the basis (room for every walk of every form) and uploads G = V V^T
 * and the applied coefficients H (n x n, column i at [i * n]), chat[0..j) = V_i . w_j (not normalised), alpha_{j-1}, the beta that formed
 * v_{j-1} (beta_prev) and the one before it (beta_prev2; ignored at j = 2).
 * lz_os_step runs the step; wide: the 16 / 8 positions per lane of knobs 9 / 11 in the pair / group walk.  *blocks_out: the blocks of
 * the walk it launched.
 * lz_os_state_get copies back what the step left (any pointer may be NULL): G, H (n x n), chat (n + 1), g (2 n + 2: the single form's
 * correction coefficients, or kap at [0] and p at [n + 1] of a pair), gq (4 runs of *ldg_out = n + 4: a group's predictions), d (the
 * second-stage sums, 4 qtw_ldp(n + 2) + 16 doubles, runs *ldp_out apart), elog, alpha, beta (n + 1 each; beta[k] formed v_{k+1}),
 * nrm2[0], the second residual buffer (the single form's u~; rows_local doubles) and the eight state ints ([0] gate, [1] trips,
 * [3] / [4] a pair's / a group's leftover exceeded the gate).  Rows come back through lz_basis_get_row, y through lz_r_get.
 * LZ_ERR_STATE (nothing touched) unless: one rank, fused-norm full re-orthogonalisation, 5 or 7 entries per row, tuning knob 15 not 7,
 * n <= 1520 (the fused one-sweep form's limit); j >= 2; form 1: j < n; a pair: j + 2 <= n and n + 1 <= 1024; a group: j + 4 <= n and
 * n <= 512; lz_os_step also when no state was set since the last lz_basis_alloc.  lz_run's records (lz_last_*) are not changed.
 * lz_os_raw_get: rows j0 .. j0 + count - 1 as they lie on the device, lz_padded_rows(rows_local) doubles each with the padding
 * (rows == NULL: none), and the first part_count doubles of the partial sums the last lz_os_step's walk wrote (one run of 4 / 2 / 1
 * times ldp doubles per block; copied aside behind the walk, because later launches of the step reuse that buffer; part == NULL: none). */
int lz_os_state_set(lz_handle h, int j, const double* G, const double* H, const double* chat, double alpha_prev, double beta_prev,
                    double beta_prev2);
int lz_os_step(lz_handle h, int form, int j, int wide, int* blocks_out);
int lz_os_state_get(lz_handle h, int form, int j, double* G, double* H, double* chat, double* g, double* gq, double* d, double* elog,
                    double* alpha, double* beta, double* nrm2, double* r2_local, int* ist, int* ldg_out, int* ldp_out);
int lz_os_raw_get(lz_handle h, int j0, int count, double* rows, double* part, int64_t part_count);
/* y = A x on host vectors (length rows_local / ncols_ext handled internally; single rank) */
int lz_spmv_host(lz_handle h, const double* x, double* y);

/* ---- thick-restart Lanczos (lanczos_amd.eigsh; Wu & Simon 2000) ----------------------------------------------------------------
 * Replaces the host ARPACK call of find_exact_eigs (Lanczos.py:68-71: scipy.sparse.linalg.eigsh) for matrices that live on the device.
 * The host runs the outer loop (restart policy, eigh of the m x m projected matrix T, stopping test: lanczos_amd/eigsh.py); these calls
 * do every pass over the basis.  The basis is a buffer of its own - m + 1 rows of the padded row length - so a fixed-n run's V / Y on
 * the same handle are left alone.  One rank only: a handle with a communicator, LZ_FLAG_REORTH_PARTIAL or LZ_FLAG_ONE_REDUCE gets
 * LZ_ERR_STATE.  LZ_FLAG_TRL_PASS2_ALWAYS forces the second Gram-Schmidt pass of every extension step (tests). */
/* allocate the basis for m (2 <= m <= min(128, rows)) vectors plus the residual row, zero it, V[0] = v0 / |v0| */
int lz_trl_begin(lz_handle h, int m, const double* v0);
/* steps j = k .. m-1 without a host synchronisation: w = A V[j]; c = V[0..j] . w, w -= sum c_i V_i (classical Gram-Schmidt); a second
 * such pass only when |w| fell below |w_before| / sqrt 2 (DGKS; the decision is taken on the device); beta_j = |w|, V[j + 1] = w / beta_j.
 * proj_out (m x m row-major): row j receives the measured projection T[0..j, j] (both passes' sums), rows k .. m-1 only;
 * beta_out[m]: beta_j at [j] (beta_{m-1} is the norm of the residual row V[m]).  Either may be NULL. */
int lz_trl_extend(lz_handle h, int k, int m, double* proj_out, double* beta_out);
/* in place: V[0..kk) = S^T V[0..m) with S (m x kk, row-major: column i = the i-th kept Ritz vector of T), then V[kk] = V[m]
 * (1 <= kk < m).  Reads (m + kk) rows and writes kk + 1; the padding of every row is left as it is. */
int lz_trl_restart(lz_handle h, int m, int kk, const double* S);
/* V[k] = x (rows_local doubles) made orthogonal to V[0..k) by two classical Gram-Schmidt passes and normalised (0 <= k <= m): the
 * probe direction and the fresh start after a breakdown */
int lz_trl_probe(lz_handle h, int k, const double* x);
/* the first k basis rows (after the final restart: the Ritz vectors) as an (rows_local, k) row-major array, through the staging ring */
int lz_trl_get_vectors(lz_handle h, int k, double* Y_out);
/* out[i] = |A V[i] - theta[i] V[i]| for i < k: one fused SpMV-and-norm launch (CSR, the assembled stencil included); dense: the GEMV */
int lz_trl_residuals(lz_handle h, int k, const double* theta, double* out);
/* The same for complex eigenvalues re[i] + i im[i] of a real non-symmetric matrix (lanczos_amd.eigs: Krylov-Schur on the calls above -
 * on such a matrix lz_trl_extend is an Arnoldi step and lz_trl_restart takes any m x kk matrix, orthonormal or not).  Rows 0 .. k-1 hold
 * the eigenvectors in real form.  im[i] == 0: row i is x and out[i] is lz_trl_residuals' value, bit for bit.  im[i] > 0: rows i and
 * i + 1 are x_r and x_i of x = x_r + i x_i, which needs i + 1 < k, re[i + 1] == re[i] and im[i + 1] == -im[i], and
 *   out[i] = out[i + 1] = sqrt(|A x_r - re x_r + im x_i|^2 + |A x_i - im x_r - re x_i|^2) = |A x - lambda x|.
 * Anything else - a lone positive im at k - 1, mismatched re, a negative im without its partner in front, a NaN - is LZ_ERR_ARG before
 * anything is launched.  CSR (the assembled stencil included): one fused launch, the pair's block walks each matrix row once for both
 * products.  Dense: two GEMVs per pair.  Partial sums are added in a fixed order: same input, same bits.  1 <= k <= m. */
int lz_trl_residuals_cplx(lz_handle h, int k, const double* re, const double* im, double* out);
/* Chebyshev filter (lanczos_amd.eigsh(filter_degree=...); Zhou & Saad's filtered Lanczos): with degree > 0 every later lz_trl_extend
 * forms w = p(A) V[j] instead of w = A V[j], p the polynomial of the scaled three-term recurrence
 *   y_1 = a[0] (A x - c x),   y_i = a[i-1] (A y_{i-1} - c y_{i-1}) - b[i-1] y_{i-2}   (i = 2 .. degree, y_0 = x; b[0] is ignored as 0 x).
 * a, b: degree doubles each, copied to the device (the kernels read them there); degree = 0 switches the filter off.  Needs lz_trl_begin
 * first (LZ_ERR_STATE otherwise) and allocates two more work vectors of the padded row length, only when a filter is set; a later
 * lz_trl_begin with the same m keeps the filter, a new matrix (lz_set_*, lz_build_*) or another m drops it.  All degree products and
 * recurrence steps of all steps of an extension are enqueued without a host synchronisation. */
int lz_trl_set_filter(lz_handle h, int degree, const double* a, const double* b, double c);
/* Chebyshev series (lanczos_amd.eigsh(sigma=..., filter_degree=...): the eigenvalues nearest sigma): with degree > 0 every later
 * lz_trl_extend forms w = p(A) V[j] with
 *   p(A) x = sum_{i = 0 .. degree} mu[i] T_i((A - c) / e) x,   T_1 x = (A x - c x) / e,   T_{i+1} x = (2 / e)(A T_i x - c T_i x) - T_{i-1} x,
 * every term added to the running sum as it is formed.  mu: degree + 1 doubles, copied to the device; e > 0; degree = 0 clears the
 * series.  Same lifetime rules as lz_trl_set_filter; the two are exclusive - each call of either clears the other.  Allocates one
 * running-sum vector of the padded row length beside the filter's two work vectors, only when a series is set.  Fixed-K stencil
 * matrices form the step in the SpMV's epilogue unless LZ_FLAG_TRL_FILTER_UNFUSED is set (same bits).  No host synchronisation inside
 * an extension. */
int lz_trl_set_series(lz_handle h, int degree, const double* mu, double c, double e);
/* y = p(A) x for host vectors of rows_local doubles, p the filter or the series set (LZ_ERR_STATE with neither): tests of their kernels.  The residual row
 * V[m] is used as the staging row: it receives x (its padding is left as it is) and then the result with a zero padding. */
int lz_trl_filter_apply(lz_handle h, const double* x, double* y);
/* G_out (k x k row-major, 1 <= k < m) = V[0..k) A V[0..k)^T: per row one product with A itself (a filter is ignored) and one pass over
 * the k rows.  The Rayleigh-Ritz step that turns the eigenvectors of p(A) into eigenpairs of A. */
int lz_trl_rayleigh(lz_handle h, int k, double* G_out);
/* Band (block) Lanczos, Ruhe's form (lanczos_amd.eigsh(block_size=b)): b start vectors, basis row r made from A V[r - b].  The basis has
 * m + b rows: lz_trl_begin_band allocates and zeroes them (b <= m <= min(128, rows - b), 2 <= b <= 8) and makes rows 0 .. b-1 from the
 * rows of X (b x rows_local, row-major), each orthogonalised against the ones before it as lz_trl_probe does.  lz_trl_begin is the b = 1
 * case and stays the only way to a basis for lz_trl_extend; lz_trl_extend_band on such a basis (and lz_trl_extend on a band) is
 * LZ_ERR_STATE.  On a band basis lz_trl_restart moves all b residual rows (V[kk + r] = V[m + r], r < b), and lz_trl_probe,
 * lz_trl_set_rows and lz_trl_get_rows reach rows up to m + b - 1.  A filter or series set after lz_trl_begin_band applies as it does
 * to lz_trl_extend; a basis of another m or b drops it. */
int lz_trl_begin_band(lz_handle h, int m, int b, const double* X);
/* steps j = k .. m-1 in batches of up to b, without a host synchronisation.  A batch at j forms w_i = A V[j + i] (or p(A) V[j + i]) for
 * its steps, orthogonalises all of them against V[0 .. j + b) by two classical Gram-Schmidt passes of two sweeps each - one kernel forms
 * all (j + b) x b dots, one updates all b vectors, every basis row read once per sweep - and then, one by one, against the rows the batch
 * itself has made (two passes, the single-vector kernels): beta_{j+i} = |w_i|, V[j + i + b] = w_i / beta_{j+i}.  There is no DGKS gate.
 * proj_out (m x (m + b) row-major): row j receives the coefficients of A V[j] on V[0 .. j + b) (both passes' sums), rows k .. m-1 only;
 * beta_out[m]: beta_j, the coefficient on V[j + b].  Either may be NULL.  Sums are formed in a fixed order: same input, same bits. */
int lz_trl_extend_band(lz_handle h, int k, int m, double* proj_out, double* beta_out);
/* raw basis rows j0 .. j0 + count - 1 (0 <= j0, j0 + count <= m + 1; band: m + b) including their padding (lz_padded_rows(rows) doubles each), host
 * rows ld >= that apart: tests of the restart kernel */
int lz_trl_set_rows(lz_handle h, int j0, int count, const double* rows, int64_t ld);
int lz_trl_get_rows(lz_handle h, int j0, int count, double* rows, int64_t ld);

/* ---- complex Hermitian matrices (lanczos_amd.eigsh on complex input) ------------------------------------------------------------
 * The complex twin of the thick-restart section above: a complex Hermitian matrix of its own on the handle and a basis of m + 1
 * complex rows.  Across this ABI every complex vector or matrix is interleaved complex128 as NumPy stores it, passed as const double*
 * of twice the length.  On the device the matrix stays interleaved (one 16-byte load per entry) and the vectors are planar: complex
 * basis row j is two real rows of the padded, skewed stride, real part then imaginary part - so the restart is the real MFMA kernel on
 * the real form [[Sr, Si], [-Si, Sr]] of S, which holds 2 m x 2 kk doubles in LDS and sets the limit m <= 64.
 * Handle state: one matrix at a time.  A complex setter drops the real matrix (every real entry point - lz_run, lz_trl_*, lz_spmv_host,
 * ... - then answers LZ_ERR_STATE "no matrix set"); lz_set_csr, lz_set_dense(_block) and lz_build_stencil3d(_block) drop the complex
 * one.  lz_gk_* state is separate and untouched.  Hermitian-ness is assumed, never checked.  One rank only: a handle with a
 * communicator gets LZ_ERR_STATE from the setters and from lz_ztrl_begin, which also refuses LZ_FLAG_REORTH_PARTIAL /
 * LZ_FLAG_ONE_REDUCE.  A polynomial filter (lz_trl_set_filter / lz_trl_set_series) does not apply to the complex basis. */
/* square n x n CSR, vals: nnz complex128 (2 nnz doubles); n, nnz < 2^31; rowptr and colidx validated as lz_set_csr does.  The product
 * is a plain CSR kernel: a group of lanes (the widest power of two <= min(64, nnz / n), at least 1) owns a row and walks a longer row in
 * strides; an empty row gives 0. */
int lz_set_csr_cplx(lz_handle h, int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* colidx, const double* vals);
/* dense n x n row-major complex128, uploaded as it lies in memory (a caller with a column-major Hermitian array holds the conjugate:
 * it must copy).  The product is one GEMV kernel, a wave per row, that reads A once. */
int lz_set_dense_cplx(lz_handle h, int64_t n, const double* A);
/* y = A x on host vectors of n complex128 each: the complex twin of lz_spmv_host, and the tests' way to the product kernels */
int lz_zspmv_host(lz_handle h, const double* x, double* y);
/* allocate the basis for m (2 <= m <= min(64, n)) complex vectors plus the residual row, zero it, V[0] = v0 / |v0| (v0: n complex) */
int lz_ztrl_begin(lz_handle h, int m, const double* v0);
/* steps j = k .. m-1 without a host synchronisation: w = A V[j]; c_i = <V_i, w> = sum conj(V_i) w for i <= j (real and imaginary part
 * from one read of V_i), w -= sum c_i V_i; a second such pass only when |w|^2 fell below half of what it was (DGKS, decided on the
 * device; LZ_FLAG_TRL_PASS2_ALWAYS forces it); beta_j = |w|, V[j + 1] = w / beta_j.  proj_out (m x m complex, row-major): row j
 * receives c_0 .. c_j (both passes' sums) - column j of the Hermitian projected matrix, whose diagonal entry has roundoff only in its
 * imaginary part -, rows k .. m-1 only; beta_out[m] is real.  Either may be NULL.  Sums are formed in a fixed order: same input, same
 * bits. */
int lz_ztrl_extend(lz_handle h, int k, int m, double* proj_out, double* beta_out);
/* in place: V[k] = sum_i S[i, k] V[i] for k < kk (S: m x kk complex, row-major; no conjugate is taken), then V[kk] = V[m]
 * (1 <= kk < m).  The padding of every row is left as it is. */
int lz_ztrl_restart(lz_handle h, int m, int kk, const double* S);
/* V[k] = x (n complex) made orthogonal to V[0..k) by two classical Gram-Schmidt passes and normalised (0 <= k <= m).  Zeroes the whole
 * work vector first, which also clears what a breakdown (0 / 0) left in its padding. */
int lz_ztrl_probe(lz_handle h, int k, const double* x);
/* the first k basis rows as an (n, k) row-major complex array, through the staging ring */
int lz_ztrl_get_vectors(lz_handle h, int k, double* Y_out);
/* out[i] = |A V[i] - theta[i] V[i]| for i < k and real theta: the product into the work vector, then one difference-norm kernel */
int lz_ztrl_residuals(lz_handle h, int k, const double* theta, double* out);
/* basis rows j0 .. j0 + count - 1 (0 <= j0, j0 + count <= m + 1) as unpadded rows of n complex numbers, host rows ld >= n complex
 * elements apart; set_rows writes a zero padding.  Tests of the kernels. */
int lz_ztrl_set_rows(lz_handle h, int j0, int count, const double* rows, int64_t ld);
int lz_ztrl_get_rows(lz_handle h, int j0, int count, double* rows, int64_t ld);

/* ---- matrix exponential action (lanczos_amd.expm_multiply; the short-iterative Lanczos propagator) -------------------------------
 * exp(a t A) b for a real symmetric or complex Hermitian A: m Lanczos steps from the current state, the exponential of the small
 * projected matrix on the host, the combination of the rows on the device - and again from the new state, which never leaves the
 * device.  The basis (m + 1 rows) is the propagator's own: the bases of lz_trl_* and lz_ztrl_* on the same handle are untouched, and
 * no matrix setter drops more than it drops without this section.  Real rows (cplx = 0) or planar complex rows as in the section
 * above (cplx = 1); across this ABI a complex vector is interleaved complex128.  Three routes: a real matrix and a real basis run the
 * real product; a complex matrix needs the planar basis and runs lz_zspmv_host's product; a REAL matrix with a PLANAR basis (a real
 * Hamiltonian in Schroedinger time) runs the mixed product, which takes one of two forms: the two-plane kernel, which reads the
 * matrix once for both planes (CSR: a group of lanes per row, chosen from the mean row length as lz_set_csr_cplx does; dense: a wave
 * per row), or two launches of the real product, one per plane.  lz_expm_set_product chooses: 0 auto, 1 two launches, 2 the two-plane
 * kernel (a call of its own, not an lz_set_tuning index: every index up to 23 is taken and 24 is refused as out of range).  Auto takes the two-plane kernel for every dense matrix and for a CSR matrix with a mean row below 16 entries whose SpMV is
 * neither the ELL / row-class coded stencil kernel nor the column-blocked two-phase one (DESIGN.md section 8e has the measurements).
 * One rank only: LZ_ERR_STATE on a handle with a communicator and with LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE.  Every call
 * behind lz_expm_begin answers LZ_ERR_STATE before it, after the matrix changed its padded row length, with no matrix set, and for a
 * real basis once a complex matrix is set. */
/* allocate the basis for m steps (2 <= m <= min(64, n): the real form of a planar C has 2 m rows, launch_trl_restart's limit),
 * zero it, V[0] = v0 / |v0| (v0: n doubles, or n complex with cplx).  LZ_ERR_ARG for cplx = 0 while a complex matrix is set. */
int lz_expm_begin(lz_handle h, int m, int cplx, const double* v0);
/* steps j = k0 .. k1 - 1 (0 <= k0 < k1 <= m) without a host synchronisation, each as lz_trl_extend / lz_ztrl_extend run it: w = A V[j],
 * classical Gram-Schmidt against V[0..j] with the second pass behind the DGKS gate, beta_j = |w|, V[j + 1] = w / beta_j.  proj_out
 * (m x m elements, row-major) and beta_out[m] as there; rows k0 .. k1 - 1 are written on the device, the whole arrays are copied. */
int lz_expm_extend(lz_handle h, int k0, int k1, double* proj_out, double* beta_out);
/* in place: V[c] = sum_{i < mm} C[i, c] V[i] for c < ncols (C: mm x ncols row-major, complex with a planar basis; 1 <= mm <= m,
 * 1 <= ncols < mm), then V[0] = V[0] / |V[0]| with that norm in *norm_out (may be NULL).  Rows mm and above have no weight in the
 * result, whatever they hold (a breakdown leaves NaN there).  mm == 1 takes ncols == 1 and scales row 0 (row 1 is cleared).  Rows
 * ncols .. m are undefined afterwards until the next extension writes them. */
int lz_expm_combine(lz_handle h, int mm, int ncols, const double* C, double* norm_out);
/* basis rows j0 .. j0 + count - 1 (j0 + count <= m + 1).  Real basis: raw rows with their padding, as lz_trl_get_rows; planar basis:
 * unpadded rows of n complex numbers, as lz_ztrl_get_rows. */
int lz_expm_get_rows(lz_handle h, int j0, int count, double* rows, int64_t ld);
/* y = A x for the REAL matrix set and host vectors of n complex128 each, through the mixed product in the form lz_expm_set_product selects: the
 * tests' way to its kernels.  Needs no lz_expm_begin. */
int lz_zspmv_real_host(lz_handle h, const double* x, double* y);
/* out[0] = the route of the basis under the matrix now set (0 real, 1 mixed, 2 complex; -1 before lz_expm_begin), out[1] = the form
 * the last mixed product took (0 none yet, 1 two launches, 2 the two-plane kernel), out[2] = the lanes per row of the two-plane CSR
 * kernel for the CSR matrix now set (0: none set) */
int lz_expm_info(lz_handle h, int* out);
/* the form of the mixed product from now on (read at every product): 0 automatic (above), 1 two launches of the real product always,
 * 2 the two-plane kernel always (A/B, tests).  Kept on the handle until lz_destroy.  LZ_ERR_ARG for anything else. */
int lz_expm_set_product(lz_handle h, int form);
/* *ms_out = the device time (hipEvents) of one product w = A V[0] of the route, in the form lz_expm_set_product selects on the mixed route: the mean
 * of reps launches behind one warm-up launch.  The work vector is overwritten.  The measurements of tools/expm_probe.py */
int lz_expm_product_time(lz_handle h, int reps, double* ms_out);

/* ---- symmetric linear solves (lanczos_amd.minres; MINRES, Paige & Saunders 1975) ------------------------------------------------
 * (A - shift I) x = b for the REAL symmetric matrix set, definite or not: the Lanczos three-term recurrence with no basis stored and
 * the solution updated from the QR factorisation of the tridiagonal matrix, one Givens rotation per step (SciPy's sign convention:
 * cs = -1, sn = 0 at the start).  Seven padded vectors of their own: the fixed-n run's basis, the thick-restart basis and the
 * propagator's basis on the same handle are untouched; every matrix setter drops the state.  A step is four launches - the matrix'
 * product with its x_own . y epilogue, a one-block kernel for alpha, one streaming pass (the three-term, the partials of |r|^2 and the
 * END of the step before: w and x += phi w, whose scalars were not known sooner) and a one-block kernel for beta, the rotation and
 * the stopping rule.  The update therefore lags one step inside lz_minres_run and is applied before it returns: between two calls
 * the state is never lagged.  v_{k+1} = r / beta is never stored by a pass of its own: the product divides as it reads r where the
 * matrix has the scale-on-read SpMV (a row-class coded or ELL-ordered stencil), else the product runs on r and the streaming pass
 * divides.  No atomics: the same input gives the same bits.  One rank only: LZ_ERR_STATE with no real matrix, on a handle with a
 * communicator and with LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE; every call behind lz_minres_begin answers LZ_ERR_STATE before
 * it and after a matrix setter. */
/* allocate and zero, r0 = b - (A - shift I) x0 by one product (x0 NULL: r0 = b, no product), beta1 = |r0|.  b, x0: n doubles. */
int lz_minres_begin(lz_handle h, const double* b, const double* x0, double shift);
/* up to iters steps without a host synchronisation, then the pending update, then one synchronisation.  Stopping rule, on the device:
 * after the first step with phibar <= rtol beta1, or whose beta is zero or not finite, the done flag is set and every later launch of
 * this section returns at once (the products of the rest of the call still run; their output is not read).  A call on a state that
 * is done enqueues nothing.  state_out (8 doubles, may be NULL): steps done in total, done, phibar (the estimate of
 * |b - (A - shift I) x|), beta1, sqrt(tnorm2) (an estimate of |A - shift I|), the last alpha, the last beta, the last phi. */
int lz_minres_run(lz_handle h, int iters, double rtol, double* state_out);
/* out[0 .. count) = phibar after steps 1 .. count.  count may pass the steps done, up to the steps lz_minres_run was asked for so far
 * (the history holds 1024 at least): a step that did not run, or that lz_minres_set_state skipped, reads zero. */
int lz_minres_history(lz_handle h, double* out, int count);
/* a vector of the state as n host doubles; with k the step that would run next: x_{k-1}, v_k (formed on read: r / |r|), v_{k-1},
 * w_{k-1}, w_{k-2}, and r = the un-normalised v_k.  which | LZ_MINRES_RAW: the padded device vector as it is (lz_padded_rows(n)
 * doubles; for LZ_MINRES_V: r's, divided) - the tests' look at the padding. */
enum { LZ_MINRES_X = 0, LZ_MINRES_V = 1, LZ_MINRES_VPREV = 2, LZ_MINRES_W1 = 3, LZ_MINRES_W2 = 4, LZ_MINRES_R = 5, LZ_MINRES_RAW = 8 };
int lz_minres_get(lz_handle h, int which, double* out);
/* upload the state that step k >= 1 starts from (allocates as lz_minres_begin does): x_{k-1}, v_k (taken as given, not normalised),
 * v_{k-1}, w_{k-1}, w_{k-2} - n doubles each - and scalars[9] = beta_k, cs, sn, dbar, epsln, phibar, tnorm2, beta1, shift.  The
 * history of steps 1 .. k - 1 reads zero.  Tests drive one step from chosen numbers with it, as lz_os_state_set does for lz_os_step. */
int lz_minres_set_state(lz_handle h, int k, const double* x, const double* vk, const double* vkm1, const double* wkm1, const double* wkm2,
                        const double* scalars);
/* ms_out[0] = the device time (hipEvents) of one product of the plan, ms_out[1] = of one k_minres_step with the three-term and the
 * lagged update: each the mean of reps launches behind one warm-up launch.  The state is spent afterwards (LZ_ERR_STATE until the next
 * lz_minres_begin).  The measurements of tools/minres_probe.py */
int lz_minres_step_time(lz_handle h, int reps, double* ms_out);
/* out[0] = launches per iteration of the plan for the matrix set, product included; out[1] = 1 where the product scales on read;
 * out[2] = 1 while a state is live */
int lz_minres_info(lz_handle h, int* out);

/* ---- least-squares solves (lanczos_amd.lsmr; LSMR, Fong & Saunders 2011) --------------------------------------------------------
 * min |A x - b|^2 + damp^2 |x|^2 for the rectangular matrix lz_gk_set_csr / lz_gk_set_dense holds (tall orientation, p x q):
 * transposed == 0 means A is that matrix (b: p doubles, x: q doubles), transposed == 1 means A is its transpose (b: q, x: p).
 * Golub-Kahan bidiagonalisation with no basis kept and SciPy's lsmr scalar for scalar (the same rotations, the same estimates of |r|,
 * |A^T r|, |A| and cond(A)).  Seven padded vectors of its own, two of b's length and five of x's: no lz_gk_begin is needed, the bases
 * of lz_gk_*, the square matrix and every other state on the handle are untouched; lz_gk_set_csr / lz_gk_set_dense drop the state.
 * u and v are kept un-normalised together with their divisors, and every kernel divides where it reads.  A step is the two products
 * and four launches of its own: one streaming pass over b's length (u = A v - alpha u with the partials of |u|^2: 24 B a row), a
 * one-block kernel for beta, one streaming pass over x's length (v = A^T u - beta v with the partials of |v|^2 and, from the same
 * load of v, the END of the step before: hbar, x, h and the partials of |x|^2, whose scalars were not known before alpha was: 72 B a
 * row) and a one-block kernel for alpha, the rotations, the estimates and the stopping tests.  The update therefore lags one step
 * inside lz_lsmr_run and is applied before it returns: between two calls the state is never lagged.  The tests of step k use
 * |x_{k-1}|, which the lagged pass yields (SciPy uses |x_k|).  No atomics: the same input gives the same bits.  One rank only:
 * LZ_ERR_STATE with no rectangular matrix, on a handle with a communicator and with LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE;
 * every call behind lz_lsmr_begin answers LZ_ERR_STATE before it and after lz_gk_set_csr / lz_gk_set_dense. */
/* allocate and zero, u = b - A x0 by one product (x0 NULL: u = b, no product), beta_1 = |u|, v = A^T u / beta_1, alpha_1 = |v|; the
 * pending update is the empty one that makes h_1 = v_1.  The state is done at once (istop 0) when alpha_1 beta_1 = 0 or b = 0. */
int lz_lsmr_begin(lz_handle h, int transposed, const double* b, const double* x0, double damp);
/* up to iters steps without a host synchronisation, then the pending update, then one synchronisation.  The stopping tests run on
 * the device with SciPy's codes 1 .. 6 (conlim <= 0: no limit on cond(A)); the first step that meets one sets the done flag and every
 * later launch of this section in the call returns at once (the products of the rest of the call still run; their output is not
 * read).  A beta that is not finite sets the flag with the state as it is and reports 7.  A call on a state that is done enqueues
 * nothing.  state_out (16 doubles, may be NULL): steps done in total, done, istop, normr, normar, normA, condA, |x| of the x now
 * held, alpha, beta, rho, rhobar, zeta, zetabar, |x_{k-1}| as the last step's tests saw it, normb. */
int lz_lsmr_run(lz_handle h, int iters, double atol, double btol, double conlim, double* state_out);
/* a vector of the state as host doubles: x, u_k and v_k (formed on read: divided as the kernels divide), h, hbar.  which |
 * LZ_LSMR_RAW: the padded device vector as it is (lz_padded_rows of its length; U and V un-normalised: beta_k u_k and alpha_k v_k) -
 * the tests' look at the padding. */
enum { LZ_LSMR_X = 0, LZ_LSMR_U = 1, LZ_LSMR_V = 2, LZ_LSMR_H = 3, LZ_LSMR_HBAR = 4, LZ_LSMR_RAW = 8 };
int lz_lsmr_get(lz_handle h, int which, double* out);
/* upload the state that step k >= 1 starts from (allocates as lz_lsmr_begin does) with the update of step k - 1 pending: x_{k-2},
 * u_k and v_k (taken as given, their divisors set to 1), h_{k-1}, hbar_{k-2}, and scalars[24] = alpha, beta, alphabar, rho, rhobar,
 * cbar, sbar, zeta, zetabar, betadd, betad, rhodold, tautildeold, thetatilde, d, normA2, maxrbar, minrbar, damp, normb, and c1, c2,
 * c3 of the pending update (hbar = h - c1 hbar, x += c2 hbar, h = v_k - c3 h), one spare.  The history of steps 1 .. k - 1 reads
 * zero.  Tests drive one step from chosen numbers with it. */
int lz_lsmr_set_state(lz_handle h, int transposed, int k, const double* x, const double* u, const double* v, const double* hvec,
                      const double* hbar, const double* scalars);
/* out[2 i], out[2 i + 1] = normr, normar after step i + 1, i < count.  count may pass the steps done, up to the steps lz_lsmr_run was
 * asked for so far (the history holds 1024 at least): a step that did not run reads zero. */
int lz_lsmr_history(lz_handle h, double* out, int count);
/* out[0] = launches of the solver's own per iteration beside the two products (4); out[1] = 1 while a state is live; out[2] = its
 * transposed */
int lz_lsmr_info(lz_handle h, int* out);
/* ms_out[0 .. 4) = the device times (hipEvents) of the product A v, of k_lsmr_u, of the product A^T u and of k_lsmr_v with the
 * lagged update: each the mean of reps launches behind one warm-up launch.  The state is spent afterwards (LZ_ERR_STATE until the
 * next lz_lsmr_begin).  The measurements of tools/lsmr_probe.py */
int lz_lsmr_step_time(lz_handle h, int reps, double* ms_out);

/* ---- non-symmetric linear solves (lanczos_amd.bicgstab; BiCGSTAB, van der Vorst 1992) -------------------------------------------
 * A x = b for the REAL square matrix set, symmetric or not, SciPy's bicgstab scalar for scalar: no basis, no transpose product.  With
 * k = 0, 1, ... SciPy's `iteration`, r~ = r_0 and rho = r~ . r, iteration k is
 *     head tests, in this order: |r| < atol (code 0), |rho| < eps^2 (-10), from k = 1 on |omega| < eps^2 (-11)
 *     p = (p - omega v) beta + r,  beta = (rho / rho_prev)(alpha / omega)        (k = 0: p = r)
 *     v = A p,  rv = r~ . v (rv == 0: -11),  alpha = rho / rv
 *     s = r - alpha v;  |s| < atol: x += alpha p, code 0 - the half-step exit, the residual kept is s
 *     t = A s,  omega = (t . s) / (t . t),  x = (x + alpha p) + omega s,  r = s - omega t,  rho_prev = rho,  rho = r~ . r
 * Six padded vectors of its own (x, r - which holds s between the two products -, r~, p, v, t): every other state on the handle is
 * untouched; every setter of the square matrix drops the state.  The products are the handle's in whatever plan the matrix has; their
 * x_own . y epilogue yields r~ . v and t . s (the column-blocked two-phase plan cannot take an x_own that is not x: there one more
 * launch forms r~ . v and the t . t pass forms t . s).  Beside them an iteration is seven launches: four streaming passes (p: 32 B a
 * row; s and the partials of |s|^2: 24; the partials of t . t: 8; both updates of x, r and the partials of |r|^2 and r~ . r: 56) and
 * three one-block kernels (alpha; omega and the half-step test; rho, beta and the head tests of the NEXT iteration, so an iteration
 * that ends with |r| < atol reports 0 at once).  No atomics: the same input gives the same bits.  One rank only: LZ_ERR_STATE with no
 * real square matrix, on a handle with a communicator and with LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE; every call behind
 * lz_bicgstab_begin answers LZ_ERR_STATE before it and after a matrix setter. */
/* allocate and zero all six vectors, r = b - A x0 by one product (x0 NULL: r = b, no product), r~ = r, the partials of rho = r~ . r
 * and |r|^2.  The head tests of iteration 0 need atol: the first lz_bicgstab_run applies them.  b, x0: n doubles. */
int lz_bicgstab_begin(lz_handle h, const double* b, const double* x0);
/* first the head tests of a state fresh from lz_bicgstab_begin / lz_bicgstab_set_state, then up to iters iterations without a host
 * synchronisation, then one synchronisation.  Every test runs on the device against atol_eff (the caller's max(atol, rtol |b|)); the
 * first that is met sets the done flag and every later launch of this section returns at once (the products of the rest of the call
 * still run; their output is not read).  A call on a state that is done enqueues nothing.  state_out (16 doubles, may be NULL):
 * iterations that updated x in total (a half-step exit counts), done, code (0, -10, -11), exit kind (0 none yet, 1 half step,
 * 2 full step: |r| < atol at a head test, 3 breakdown), 1 where a head test set the flag (0: inside an iteration), the recurrence's
 * |r| (|s| behind a half-step exit), rho, rho_prev, alpha, omega, beta, the last |s|, rv, t . s, t . t, one spare. */
int lz_bicgstab_run(lz_handle h, int iters, double atol_eff, double* state_out);
/* out[2 i], out[2 i + 1] = |s|, |r| of iteration i, i < count (behind a half-step exit |r| repeats |s|).  count may pass the
 * iterations done, up to those lz_bicgstab_run was asked for so far (the history holds 1024 at least): an iteration that did not run,
 * or that lz_bicgstab_set_state skipped, reads zero. */
int lz_bicgstab_history(lz_handle h, double* out, int count);
/* a vector of the state as n host doubles: x, r (s behind a half-step exit), r~, p, v = A p, t = A s as the last iteration left
 * them.  which | LZ_BICGSTAB_RAW: the padded device vector as it is (lz_padded_rows(n) doubles) - the tests' look at the padding. */
enum { LZ_BICGSTAB_X = 0, LZ_BICGSTAB_R = 1, LZ_BICGSTAB_RTILDE = 2, LZ_BICGSTAB_P = 3, LZ_BICGSTAB_V = 4, LZ_BICGSTAB_T = 5, LZ_BICGSTAB_RAW = 8 };
int lz_bicgstab_get(lz_handle h, int which, double* out);
/* upload the state that iteration k >= 0 starts from (allocates and zeroes as lz_bicgstab_begin does): x, r, r~, p, v - n doubles
 * each; p and v of the iteration before, not read when k = 0 - and scalars[3] = rho_prev, alpha, omega.  rho and |r| are formed on the
 * device exactly as lz_bicgstab_begin forms them, and the first lz_bicgstab_run applies the head tests of iteration k to them.  The
 * history of iterations 0 .. k - 1 reads zero.  Tests drive one iteration, and the breakdown exits, from chosen numbers with it. */
int lz_bicgstab_set_state(lz_handle h, int k, const double* x, const double* r, const double* rtilde, const double* p, const double* v,
                          const double* scalars);
/* ms_out[0 .. 6) = the device times (hipEvents) of the product v = A p, of the product t = A s, of k_bicgstab_p, k_bicgstab_s,
 * k_bicgstab_tt and k_bicgstab_r: each the mean of reps launches behind one warm-up launch.  Needs a state that has run at least one
 * iteration and is not done; the state is spent afterwards (LZ_ERR_STATE until the next lz_bicgstab_begin).  The measurements of
 * tools/bicgstab_probe.py */
int lz_bicgstab_step_time(lz_handle h, int reps, double* ms_out);
/* out[0] = launches per iteration of the plan for the matrix set, each product counted as one (9, or 10 where the product cannot form
 * r~ . v); out[1] = 1 where the products' epilogue yields r~ . v and t . s; out[2] = 1 while a state is live */
int lz_bicgstab_info(lz_handle h, int* out);

/* ---- symmetric positive definite linear solves (lanczos_amd.cg; Hestenes & Stiefel 1952) -----------------------------------------
 * A x = b for the REAL square matrix set, taken as symmetric positive definite (neither is tested), scipy.sparse.linalg.cg scalar
 * for scalar, with an optional diagonal preconditioner d (z = d o r; d NULL: z = r).  With k = 0, 1, ... SciPy's `iteration` and
 * rho = r . z, iteration k is
 *     head test: |r| < atol (code 0)
 *     p = z + (rho / rho_prev) p                                                  (k = 0: p = z)
 *     q = A p,  pq = p . q (pq == 0 or alpha not finite: -1),  alpha = rho / pq,  x += alpha p,  r -= alpha q,  rho_prev = rho
 * Five padded vectors of its own (x, r, p, q, d): every other state on the handle is untouched; every setter of the square matrix
 * drops the state.  The product is the handle's in whatever plan the matrix has, called with x_own = p: its x_own . y epilogue
 * yields p . q on every plan.  Beside it an iteration is four launches: k_cg_alpha (one block: pq, the breakdown test, alpha, the
 * first iteration with pq <= 0), k_cg_r (r -= alpha q, the partials of r . r and r . z, z formed on the fly: 24 B a row, 32 with d),
 * k_cg_scalars (one block: |r|, the history, the head test of the NEXT iteration - so an iteration that ends with |r| < atol
 * reports 0 at once -, rho, beta, the counter, the done flag) and k_cg_p (x += alpha p, then p = z + beta p from the same load of
 * p: 40 B a row, 48 with d; the iteration that raised the done flag still updates x).  No atomics: the same input gives the same
 * bits.  One rank only: LZ_ERR_STATE with no real square matrix, on a handle with a communicator and with LZ_FLAG_REORTH_PARTIAL /
 * LZ_FLAG_ONE_REDUCE; every call behind lz_cg_begin answers LZ_ERR_STATE before it and after a matrix setter. */
/* replaces r = b - A x0, z = M r, p = z, rho = r . z ahead of SciPy's loop: allocate and zero all five vectors, r by one product
 * (x0 NULL: r = b, no product), p = d o r, the partials of r . r and r . z in one pass.  The head test of iteration 0 needs atol: the
 * first lz_cg_run applies it.  b, x0, d: n doubles; d NULL: no preconditioner; d is not validated (the caller's: finite, positive). */
int lz_cg_begin(lz_handle h, const double* b, const double* x0, const double* d);
/* replaces the body of SciPy's loop: first the head test of a state fresh from lz_cg_begin / lz_cg_set_state, then up to iters
 * iterations without a host synchronisation, then one synchronisation.  Every test runs on the device against atol_eff (the
 * caller's max(atol, rtol |b|)); the first that is met sets the done flag and every later launch of this section returns at once
 * (the products of the rest of the call still run; their output is not read).  A call on a state that is done enqueues nothing.
 * state_out (16 doubles, may be NULL): iterations that updated x in total, done, code (0, -1), exit kind (0 none yet, 1 converged,
 * 2 breakdown), 1 where a head test set the flag (0: inside an iteration - x did not move), the recurrence's |r| at the last head
 * test, rho, rho_prev, alpha, beta, pq, the first iteration with pq <= 0 (-1: none), four spares. */
int lz_cg_run(lz_handle h, int iters, double atol_eff, double* state_out);
/* replaces the norm(r) of SciPy's head test as a record: out[i] = |r| at the head test of iteration i, i < count.  count may pass
 * the tests done, up to the iterations lz_cg_run was asked for so far plus one (the history holds 1024 at least): a test that did
 * not run, or that lz_cg_set_state skipped, reads zero. */
int lz_cg_history(lz_handle h, double* out, int count);
/* replaces reading SciPy's x (and r, p, q in a debugger): a vector of the state as n host doubles.  which | LZ_CG_RAW: the padded
 * device vector as it is (lz_padded_rows(n) doubles) - the tests' look at the padding. */
enum { LZ_CG_X = 0, LZ_CG_R = 1, LZ_CG_P = 2, LZ_CG_Q = 3, LZ_CG_D = 4, LZ_CG_RAW = 8 };
int lz_cg_get(lz_handle h, int which, double* out);
/* replaces SciPy's locals at the head of iteration k >= 0 (allocates and zeroes as lz_cg_begin does): x, r, p - already p_k, the
 * direction iteration k multiplies -, n doubles each; d or NULL; scalars[1] = rho = r . z.  |r| is formed on the device, and the
 * first lz_cg_run applies the head test of iteration k.  The history of iterations 0 .. k - 1 reads zero.  Tests drive one iteration,
 * and the breakdown exit, from chosen numbers with it. */
int lz_cg_set_state(lz_handle h, int k, const double* x, const double* r, const double* p, const double* d, const double* scalars);
/* ms_out[0 .. 3) = the device times (hipEvents) of the product q = A p, of k_cg_r and of k_cg_p: each the mean of reps launches
 * behind one warm-up launch.  Needs a state that has run at least one iteration and is not done; the state is spent afterwards
 * (LZ_ERR_STATE until the next lz_cg_begin).  The measurements of tools/cg_probe.py */
int lz_cg_step_time(lz_handle h, int reps, double* ms_out);
/* out[0] = launches per iteration, the product counted as one (5); out[1] = 1 where the live state has a preconditioner; out[2] = 1
 * while a state is live */
int lz_cg_info(lz_handle h, int* out);

/* ---- restarted GMRES (lanczos_amd.gmres; Saad & Schultz 1986) -------------------------------------------------------------------
 * A x = b for the REAL square matrix set, scipy.sparse.linalg.gmres' rules: with m the restart length, a cycle is
 *     V[0] = r / |r|, S = |r| e_0;  for j = 0 .. m - 1: w = A V[j], w against V[0 .. j] (the Hessenberg column), h1 = |w|,
 *       breakdown where h1 <= eps h0 (h0 = |A V[j]|), the stored rotations on the column, the new rotation (LAPACK lartg), S,
 *       presid = |S[j + 1]|, the inner exit on presid <= ptol or on breakdown
 *     y = the pseudo-solve of the cols x cols triangle, x += y . V[:cols], r = b - A x, rnorm = |r|
 *     rnorm <= atol: converged;  behind a breakdown: the end;  else ptol_max_factor = max(eps, 0.25 f) where presid <= ptol, min(1, 1.5 f)
 *       where not, ptol = presid min(f, atol / rnorm)
 * The first test of a solve is |r| < atol and the first ptol is |b| min(1, atol / |b|).  The orthogonalisation is the basis layer's
 * (lz_trl_extend's step: classical Gram-Schmidt with the DGKS-gated second pass, no host synchronisation), not SciPy's modified
 * Gram-Schmidt: results agree to rounding, not bit for bit.  The product is the matrix's own, never the polynomial of
 * lz_trl_set_filter / lz_trl_set_series.  A basis of m + 1 rows (at least 3) and the vectors x and b of its own: the thick-restart
 * basis and every other state on the handle are untouched; every setter of the square matrix drops the state.  Everything around the
 * step runs on the device - one one-block kernel per step, and at a cycle's end the solve, the update of x (which reads cols from
 * device memory and never a row >= cols), the product, the residual pass (which writes the whole padding of w as zero) and the
 * cycle's tests - so lz_gmres_run enqueues steps, cycle ends and restarts without a synchronisation.  Behind an inner exit the
 * steps that are still enqueued change nothing: cols, S, the rotations and R are frozen and the rows they write (>= cols) are
 * scratch.  No atomics: the same input gives the same bits.  One rank only: LZ_ERR_STATE with no real square matrix, on a handle
 * with a communicator and with LZ_FLAG_REORTH_PARTIAL / LZ_FLAG_ONE_REDUCE; every call behind lz_gmres_begin answers LZ_ERR_STATE
 * before it and after a matrix setter. */
/* allocate and zero the basis (max(restart, 2) + 1 rows), x and b; |b| on the device; r = b - A x0 by one product (x0 NULL: r = b, no
 * product) and the partials of |r|^2.  The first test needs atol: the first lz_gmres_run applies it.  1 <= restart <= min(128, n),
 * else LZ_ERR_ARG.  b, x0: n doubles. */
int lz_gmres_begin(lz_handle h, int restart, const double* b, const double* x0);
/* first the first test of a state fresh from lz_gmres_begin, then - where the last synchronisation showed an inner exit inside a
 * cycle - that cycle's end, then up to `steps` inner steps with the end of a cycle enqueued wherever the host can foresee it
 * (cols == restart), then one synchronisation.  Every test runs on the device against atol_eff (the caller's max(atol, rtol |b|));
 * behind the done flag every launch of this section returns at once (the products of the rest of the call still run; their output
 * is not read).  A call on a state that is done enqueues nothing.  state_out (16 doubles, may be NULL): inner steps in total, done,
 * converged, breakdown, the inner-exit flag, cols, cycles ended, presid, ptol, ptol_max_factor, rnorm (the true |b - A x| of the last
 * cycle end), |b|, the column the host's loop makes next, three spares. */
int lz_gmres_run(lz_handle h, int steps, double atol_eff, double* state_out);
/* the first test where it is due, then the end of the cycle under way whatever its length (cols >= 1; nothing where cols == 0), then
 * one synchronisation: SciPy's legacy exit in the middle of a cycle, and the tests' way to one solve-and-update.  state_out as above. */
int lz_gmres_end_cycle(lz_handle h, double atol_eff, double* state_out);
/* presid_out[i] = presid of inner step i, i < count; cycles_out[3 c .. 3 c + 3) = rnorm, cols and the ptol cycle c ran under,
 * c < ncycles.  The counts may pass what was done, up to what lz_gmres_run was asked for so far (both histories hold 1024 at least):
 * an entry that was not made reads zero.  Either pointer may be NULL where its count is 0. */
int lz_gmres_history(lz_handle h, double* presid_out, int count, double* cycles_out, int ncycles);
/* LZ_GMRES_X, _W (the work vector: the residual b - A x behind a cycle end), _B: n host doubles, or with LZ_GMRES_RAW the padded
 * device vector as it is (lz_padded_rows(n) doubles) - the tests' look at the padding.  LZ_GMRES_Y: restart doubles, the last solve's
 * y (zero from cols on).  LZ_GMRES_ROWS: the restart + 1 basis rows with their padding, lz_padded_rows(n) doubles apart.
 * LZ_GMRES_SMALL: restart^2 + 5 restart + 14 doubles - R (column j at j restart, rows 0 .. j), the rotations' c, their s,
 * S (restart + 1), then cols, ptol, ptol_max_factor, presid, rnorm, |b|, the inner-exit flag, breakdown, done, converged, inner steps,
 * cycles (lz_gmres_set_state reads up to here: restart^2 + 3 restart + 13), then what the last step handed to k_gmres_column: its
 * coefficients (restart slots, j + 1 used), h1, and the self slots of pass 1's dots (restart; the step that made column j left
 * h0^2 at index j). */
enum { LZ_GMRES_X = 0, LZ_GMRES_W = 1, LZ_GMRES_B = 2, LZ_GMRES_Y = 3, LZ_GMRES_ROWS = 4, LZ_GMRES_SMALL = 5, LZ_GMRES_RAW = 8 };
int lz_gmres_get(lz_handle h, int which, double* out);
/* upload a whole state (allocates and zeroes as lz_gmres_begin does): x and b, n doubles each; w with its padding
 * (lz_padded_rows(n) doubles); basis rows 0 .. nrows - 1 with their padding, lz_padded_rows(n) doubles apart (rows 0 ..
 * min(cols, restart - 1) at least); small in LZ_GMRES_SMALL's layout.  No test is pending behind it: the next lz_gmres_run makes
 * column cols, or begins with the cycle's end where the inner-exit flag is set.  Tests drive one step, one solve-and-update and one
 * cycle end from chosen numbers with it. */
int lz_gmres_set_state(lz_handle h, int restart, const double* x, const double* b, const double* w, const double* rows, int nrows,
                       const double* small);
/* ms_out[0 .. 5) = the device times (hipEvents) of the product A V[cols - 1], of the Gram-Schmidt step against cols rows (both
 * passes), of k_gmres_update at cols rows, of launch_trl_cgs at cols rows (the yardstick: the same bytes) and of k_gmres_residual:
 * each the mean of reps launches behind one warm-up launch.  Needs a state inside a cycle with cols >= 1 and no flag set; the state
 * is spent afterwards (LZ_ERR_STATE until the next lz_gmres_begin).  The measurements of tools/gmres_probe.py */
int lz_gmres_step_time(lz_handle h, int reps, double* ms_out);
/* out[0] = launches per inner step, the product counted as one (11); out[1] = launches per cycle end (6); out[2] = 1 while a state
 * is live; out[3] = its restart length */
int lz_gmres_info(lz_handle h, int* out);

/* ---- Golub-Kahan-Lanczos bidiagonalisation with thick restart (lanczos_amd.svds; Baglama & Reichel 2005) ------------------------
 * Every function of this section replaces a part of scipy.sparse.linalg.svds on the host: singular triplets of a rectangular or
 * non-symmetric sparse matrix that lives on the device.  The host runs the outer loop (SVD of the m x m projected matrix B, restart
 * policy, stopping test: lanczos_amd/svds.py); these calls do every product and every pass over the two bases.  The state is separate
 * from the handle's square operator: lz_set_*'s matrix, a fixed-n run's V / Y and a thick-restart basis on the same handle stay as
 * they are.  One rank only: a handle with a communicator gets LZ_ERR_STATE.  LZ_FLAG_TRL_PASS2_ALWAYS forces the second Gram-Schmidt
 * pass of every half step (tests), as it does for lz_trl_extend.
 * A is p x q with p >= q (the caller passes the transpose of a wide matrix); U holds vectors of length p, V of length q.  `side`
 * arguments: 0 = U, 1 = V. */
/* A (p x q, p >= q >= 2) and its transpose (q x p), both CSR with sorted indices; p, q, nnz < 2^31.  Validated as lz_set_csr validates.
 * Neither matrix gets any of the square SpMV layouts: their products run through the rectangular kernel only (row blocks in SciPy's
 * csr_matvec order, bit-identical to it; a row longer than the LDS tile - 4096 entries, tuning knob 4 - is split into segments summed
 * by one workgroup each and added in segment order: deterministic, but another order than SciPy's).  LZ_FLAG_SPMV_STREAM set at this
 * call keeps every long row in one workgroup (the A/B arm of the segment path).  Drops a basis of an earlier matrix. */
int lz_gk_set_csr(lz_handle h, int64_t p, int64_t q, int64_t nnz, const int32_t* rowptr, const int32_t* colidx, const double* vals,
                  const int32_t* rowptrT, const int32_t* colidxT, const double* valsT);
/* The same operator as ONE dense row-major array: S is p x q (stored_transposed == 0) or q x p (the transpose of the tall operator:
 * a wide matrix as its caller holds it), p >= q >= 2, host rows ld_host >= the row length apart.  The device keeps one copy with an
 * even row stride (8 B per entry, nothing is transposed or indexed) and runs both directions on it: along the rows ("rowdot",
 * out[r] = sum_c S[r, c] x[c]) and down the columns ("colsum", out[c] = sum_r S[r, c] u[r]).  Stored tall, A x is rowdot and A^T u
 * colsum; stored wide the other way round.  The form of each is chosen here from the shape and the CU count (lz_gk_plan reports it):
 *   rowdot  1 short rows (row length <= 128): a group of lanes per row, several rows per wave
 *           2 one wave per row
 *           3 four adjacent rows per wave, which share the loads of x: medium rows (up to 1024) whole, and fewer than 768 longer
 *             rows cut into two or more segments of >= 2048 doubles, a wave per segment (tuning knob 4: the segment length in
 *             doubles, even, clamped to 64 .. 2^22), the partials added in segment order by a fold kernel
 *   colsum 11 tiles of 128 columns x slabs of rows (knob 2: rows per slab, clamped to 1 .. 2^22), the slabs added in order by a
 *             fold kernel
 *          12 the same tiles with one slab that holds every row: no fold kernel (the tiles alone fill the device, or few rows)
 *          13 rows shorter than 128: a group of lanes per row, many rows per workgroup and trip, slabs as in 11
 * Knob 14 = r + 4 c forces the rowdot form r (1 / 2 / 3) and the colsum form 10 + c (c = 1 / 2 / 3) at any shape, r or c = 0 leaves
 * that one to the shape (A/B, tests); the three knobs are read at this call.  No atomics: the same input gives the same bits; the sums use fma and another order than a
 * CSR copy's.  Values are not validated (lz_gk_set_csr does not validate its values either).  Errors as lz_gk_set_csr, before any
 * device work.  Frees the CSR operator of an earlier lz_gk_set_csr, as that call frees a dense one; drops a basis of an earlier matrix. */
int lz_gk_set_dense(lz_handle h, int64_t p, int64_t q, const double* S, int64_t ld_host, int stored_transposed);
/* out[0] = the operator's kind (0 CSR, 1 dense), out[1] = 1 when the dense copy is the transpose (q x p), out[2] / out[3] = the form
 * that A x / A^T u run (the codes above; 0 for CSR).  LZ_ERR_STATE before lz_gk_set_csr / lz_gk_set_dense. */
int lz_gk_plan(lz_handle h, int* out);
/* allocate and zero V (m + 1 rows of the padded q) and U (m + 1 rows of the padded p; row m stays zero), 2 <= m <= min(128, q);
 * V[0] = v0 / |v0| (v0: q doubles) */
int lz_gk_begin(lz_handle h, int m, const double* v0);
/* steps j = k .. m-1 without a host synchronisation: w = A V[j] made orthogonal to U[0..j) (classical Gram-Schmidt, a second pass
 * behind the DGKS gate, decided on the device), alpha_j = |w|, U[j] = w / alpha_j; z = A^T U[j] made orthogonal to V[0..j] likewise,
 * beta_j = |z|, V[j + 1] = z / beta_j.  colproj_out (m x m row-major): row j receives the measured coefficients of A V[j] on U[0..j)
 * (both passes' sums), rows k .. m-1 only; alpha_out[m], beta_out[m].  Any of the three may be NULL.
 * When U[k] was made by lz_gk_probe(h, 0, k, ..) since the last extension, restart or begin - the fresh direction behind a vanished
 * alpha_k - step k starts at its second half: A V[k] is not formed, row k of colproj_out and alpha_out[k] are not written. */
int lz_gk_extend(lz_handle h, int k, int m, double* colproj_out, double* alpha_out, double* beta_out);
/* in place: U[0..kk) = P^T U[0..m), V[0..kk) = Q^T V[0..m), V[kk] = V[m] (P, Q: m x kk row-major, 1 <= kk < m); U[kk] becomes the
 * zero row U[m] */
int lz_gk_restart(lz_handle h, int m, int kk, const double* P, const double* Q);
/* row k of the side's basis = x (p or q doubles) made orthogonal to the rows below it by two Gram-Schmidt passes and normalised
 * (U: 0 <= k < m, V: 0 <= k <= m): the fresh direction after a breakdown */
int lz_gk_probe(lz_handle h, int side, int k, const double* x);
/* the first k rows of the side's basis as a (p or q, k) row-major array, through the staging ring */
int lz_gk_get_vectors(lz_handle h, int side, int k, double* out);
/* raw rows j0 .. j0 + count - 1 (j0 + count <= m + 1) of the side's basis including their padding (lz_padded_rows(p or q) doubles
 * each), host rows ld >= that apart: tests */
int lz_gk_set_rows(lz_handle h, int side, int j0, int count, const double* rows, int64_t ld);
int lz_gk_get_rows(lz_handle h, int side, int j0, int count, double* rows, int64_t ld);
/* out[i] = |A V[i] - sigma[i] U[i]|, out[k + i] = |A^T U[i] - sigma[i] V[i]| for i < k (1 <= k <= m) */
int lz_gk_residuals(lz_handle h, int k, const double* sigma, double* out);
/* one product through the rectangular kernel on host vectors: y = A x (transpose == 0: x q doubles, y lz_padded_rows(p) doubles) or
 * y = A^T x (x p doubles, y lz_padded_rows(q) doubles).  y receives the padding too, which the kernel writes as zeros.  Needs
 * lz_gk_set_csr or lz_gk_set_dense only; uses the work vectors of lz_gk_extend. */
int lz_gk_spmv(lz_handle h, int transpose, const double* x, double* y);
/* *ms_out = the device time (hipEvents) of one such product, the mean of reps launches behind one warm-up launch, on whatever the work
 * vectors hold: the measurements of tools/svds_probe.py */
int lz_gk_spmv_time(lz_handle h, int transpose, int reps, double* ms_out);

/* ---- two-sided (bi-orthogonal) Lanczos: the Irregular copy's execute_Lanczos --------------------------------
 * Replaces Python/Irregular/IrrLanczos.py:77-187 (driver loop) and :408-441 (bireorthogonalize, default branch).
 * Single rank, CSR only.  Four (n, rows) bases live on the device: 0 = q (published as V: lz_get_basis /
 * lz_ritz_vectors read it), 1 = p, 2 = q_basis, 3 = p_basis (the orthonormalised copies the reference projects on). */

/* HT = csr_matrix(H.transpose()) (IrrLanczos.py:92/96) as sorted CSR of the same square shape as lz_set_csr's matrix.
 * rowptr == NULL: H is symmetric, H^T x runs on H itself. */
int lz_set_csr_transpose(lz_handle h, int64_t nnz, const int32_t* rowptr, const int32_t* colidx, const double* vals);
/* The whole run: q0, p0 are the start pair already scaled so that q0 . p0 = +-1 (IrrLanczos.py:104-106, host side).
 * alpha_out[n], beta_out[n-1], gamma_out[n-1] (IrrLanczos.py:119-121).  n >= 2. */
int lz_run_two_sided(lz_handle h, int n, const double* q0, const double* p0, double* alpha_out, double* beta_out,
                     double* gamma_out);
/* Step API for unit parity tests and for the static IrrLanczos.bireorthogonalize(V1, V2, q_basis, p_basis, j):
 * allocate the four bases (zeroed), move rows, run the default branch of bireorthogonalize on row j (j >= 0; with j = 0 there
 * is nothing to project on: the pair is rescaled to q.p = +-1 and seeds the two orthonormal bases, IrrLanczos.py:418-438). */
int lz_bi_alloc(lz_handle h, int n);
int lz_bi_set_row(lz_handle h, int which, int j, const double* row);
int lz_bi_get_row(lz_handle h, int which, int j, double* row);
int lz_step_bireorth(lz_handle h, int j);
/* The other branch of the same static method, bireorthogonalize(..., mem_safe=True) (IrrLanczos.py:398-407; no caller in the
 * reference): V1[j] -= sum_i (V1[j].V2[i] / V2[i].V2[i]) V2[i], then V2[j] against the rows of V1 likewise - one sweep over
 * ALL n rows with the reference's uu[j:] = 1, uv[j] = 0; bases 0 (V1) and 1 (V2) only, q_basis / p_basis untouched.  j >= 0. */
int lz_step_bireorth_mem_safe(lz_handle h, int j);

#ifdef __cplusplus
}
#endif
#endif /* LANCZOS_HIP_H */
