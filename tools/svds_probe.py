"""Measurements of the Golub-Kahan-Lanczos solver (lanczos_amd.svds) on one GPU, written to profiles/r14/svds_probe.json:

1. the rectangular product (launch_spmv_rect) on a square 1e6-row random CSR against k_spmv_stream (LZ_FLAG_SPMV_STREAM) on the same
   matrix, interleaved;
2. the 1e6 x 40 transpose product (40 rows of about 50 000 entries) with the segment path and with each long row in one workgroup;
3. the per-step time of lz_gk_extend at (1e6, 257), m = 40, beside the byte accounting of DESIGN.md section 8b.

    python tools/svds_probe.py [--out profiles/r14/svds_probe.json]

With --dense: the dense operator (lz_gk_set_dense) against the CSR packing of the same matrix at (1e6, 40), (2e5, 257) and
(30000, 4096), each stored tall and wide, written to profiles/r19/svds_dense_probe.json (dense_probe below).

    python tools/svds_probe.py --dense [--out profiles/r19/svds_dense_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lanczos_amd import _capi  # noqa: E402
from lanczos_amd.svds import _pack  # noqa: E402


def random_csr(M, N, per_row, seed):
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, N, (M, per_row))
    A = scipy.sparse.csr_matrix((rng.standard_normal(M * per_row), (np.repeat(np.arange(M), per_row), cols.ravel())), shape=(M, N))
    A.sum_duplicates()
    A.sort_indices()
    return A


def stream_ms(h, reps):
    """device time of one k_spmv_stream launch (hipEvents of LZ_FLAG_PROFILE), mean of reps"""
    h.timings()
    for _ in range(reps):
        h.step_spmv(0)
    t = h.timings()["spmv"]
    return t["ms"] / max(t["timed_launches"], 1)


def dense_probe(args):
    """--dense: the dense operator (lz_gk_set_dense, arm A) against the same matrix packed as CSR (lz_gk_set_csr, arm B: what svds did
    with a dense array before), per shape and storage: five interleaved rounds of gk_spmv_time on one handle pair, both directions;
    then one svds(k=6) wall time on either path and the device memory each operator holds."""
    import lanczos_amd

    out = {"device": None, "reps": args.reps, "shapes": {}}
    for p, q in ((1_000_000, 40), (200_000, 257), (30_000, 4096)):
        A = np.random.default_rng(p + q).standard_normal((p, q))
        rec = {"entries": p * q, "dense_bytes": 8.0 * p * q}
        hb = _capi.Handle(0)
        out["device"] = hb.device_name()
        free0 = hb.device_memory()[0]
        t0 = time.perf_counter()
        Aop, AopT, _ = _pack(scipy.sparse.csr_matrix(A))
        rec["csr_pack_host_s"] = time.perf_counter() - t0
        hb.gk_set_csr(Aop, AopT)
        rec["csr_device_mib"] = (free0 - hb.device_memory()[0]) / 2**20
        x, u = np.random.default_rng(1).standard_normal(q), np.random.default_rng(2).standard_normal(p)
        for storage in ("tall", "wide"):
            ha = _capi.Handle(0)
            free0 = ha.device_memory()[0]
            ha.gk_set_dense(np.ascontiguousarray(A.T) if storage == "wide" else A, stored_transposed=storage == "wide")
            srec = {"plan": list(ha.gk_plan()), "dense_device_mib": (free0 - ha.device_memory()[0]) / 2**20}
            for name, transpose, vec in (("A_x", False, x), ("AT_u", True, u)):
                ya, yb = ha.gk_spmv(vec, transpose=transpose), hb.gk_spmv(vec, transpose=transpose)  # (leaves vec in the work vectors)
                n = len(vec)
                srec[name + "_dense_vs_csr_max_rel"] = float(np.abs(ya - yb).max() / np.abs(yb).max())
                a_ms, b_ms = [], []
                for _ in range(5):
                    a_ms.append(ha.gk_spmv_time(transpose, args.reps))
                    b_ms.append(hb.gk_spmv_time(transpose, args.reps))
                ma, mb = float(np.median(a_ms)), float(np.median(b_ms))
                srec[name] = {"dense_us": [1e3 * t for t in a_ms], "csr_us": [1e3 * t for t in b_ms], "dense_us_median": 1e3 * ma,
                              "csr_us_median": 1e3 * mb, "dense_share_of_8_tb_s": 8.0 * p * q / ma / 1e9 / 8.0, "csr_over_dense": mb / ma,
                              "terms": n}
            ha.close()
            rec[storage] = srec
        hb.close()
        walls = {}
        for name, M in (("dense", A), ("csr", None)):
            info = {}
            t0 = time.perf_counter()
            s = lanczos_amd.svds(A if M is not None else scipy.sparse.csr_matrix(A), k=6, return_singular_vectors=False, info=info)
            walls[name] = {"wall_s": time.perf_counter() - t0, "plan": info["plan"], "cycles": info["cycles"], "s_max": float(s[-1])}
        rec["svds_k6"] = walls
        out["shapes"][f"{p}x{q}"] = rec
        print(json.dumps({f"{p}x{q}": rec}), flush=True)
        del A, Aop, AopT
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--dense", action="store_true", help="the dense operator against its CSR packing -> profiles/r19/svds_dense_probe.json")
    args = ap.parse_args()
    if args.dense:
        args.out = args.out or os.path.join("profiles", "r19", "svds_dense_probe.json")
        return dense_probe(args)
    args.out = args.out or os.path.join("profiles", "r14", "svds_probe.json")
    out = {"device": None, "reps": args.reps}

    # 1. square matrix: the rectangular kernel against the parent's CSR-stream kernel
    M = 1_000_000
    A = random_csr(M, M, 10, 1)
    AT = A.T.tocsr()
    AT.sort_indices()
    hs = _capi.Handle(0)
    out["device"] = hs.device_name()
    hs.set_options(_capi.FLAG_SPMV_STREAM | _capi.FLAG_PROFILE)
    hs.set_csr(M, 0, A.indptr, A.indices, A.data)
    hs.basis_alloc(2)
    x = np.random.default_rng(2).standard_normal(M)
    hs.basis_set_row(0, x)
    hr = _capi.Handle(0)
    hr.gk_set_csr(A, AT)
    hr.gk_spmv(x)  # (leaves x in the work vector the timed launches read)
    stream_ms(hs, 5)
    rect, stream = [], []
    for _ in range(5):
        rect.append(hr.gk_spmv_time(False, args.reps))
        stream.append(stream_ms(hs, args.reps))
    bytes_sq = 12.0 * A.nnz + 4.0 * (M + 1) + 16.0 * M
    out["square_1e6"] = {"nnz": int(A.nnz), "rect_ms": rect, "stream_ms": stream, "rect_over_stream": float(np.median(rect) / np.median(stream)),
                         "algorithmic_bytes": bytes_sq, "rect_tb_s": bytes_sq / np.median(rect) / 1e9}
    hs.close()
    hr.close()

    # 2. long rows: the transpose of 1e6 x 40 with 2 entries per row
    B = random_csr(M, 40, 2, 3)
    Bop, BopT, _ = _pack(B)
    arms = {}
    for name, flags in (("segments", 0), ("row_per_workgroup", _capi.FLAG_SPMV_STREAM)):
        h = _capi.Handle(0)
        if flags:
            h.set_options(flags)
        h.gk_set_csr(Bop, BopT)
        h.gk_spmv(np.random.default_rng(4).standard_normal(M), transpose=True)
        arms[name] = [h.gk_spmv_time(True, args.reps) for _ in range(5)]
        h.close()
    bytes_t = 12.0 * Bop.nnz + 8.0 * M
    out["transpose_1e6x40"] = {"nnz": int(Bop.nnz), "ms": arms, "algorithmic_bytes": bytes_t,
                               "segments_share_of_8_tb_s": bytes_t / np.median(arms["segments"]) / 1e9 / 8.0,
                               "row_per_workgroup_share_of_8_tb_s": bytes_t / np.median(arms["row_per_workgroup"]) / 1e9 / 8.0}

    # 3. step time of lz_gk_extend at (1e6, 257), m = 40
    p, q, m = 1_000_000, 257, 40
    Cm = random_csr(p, q, 4, 5)
    Cop, CopT, _ = _pack(Cm)
    h = _capi.Handle(0)
    h.gk_set_csr(Cop, CopT)
    h.gk_begin(m, np.random.default_rng(6).standard_normal(q))
    h.gk_extend(0, m)
    walls = []
    for _ in range(3):
        h.gk_begin(m, np.random.default_rng(6).standard_normal(q))
        t0 = time.perf_counter()
        h.gk_extend(0, m)
        walls.append((time.perf_counter() - t0) * 1e3 / m)
    pp, qp = h.padded_rows(p), h.padded_rows(q)
    # per step j (one Gram-Schmidt pass pair per side: dots + update each walk the rows once): two products + 2 (j p + (j + 1) q) 8 B
    model = [2 * (12.0 * Cop.nnz + 8.0 * (pp + qp)) + 2.0 * (j * pp + (j + 1) * qp) * 8 for j in range(m)]
    out["extend_1e6x257_m40"] = {"nnz": int(Cop.nnz), "ms_per_step": walls, "model_bytes_per_step_mean": float(np.mean(model)),
                                 "model_share_of_8_tb_s": float(np.mean(model)) / np.median(walls) / 1e9 / 8.0}
    h.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
