"""Thick-restart Lanczos (lanczos_amd.eigsh) on the device: the restart kernel's rate, the extension step with and without the DGKS
gate next to the fixed-n loop's step, and one eigsh run on the device-assembled deuteron Hamiltonian.

    python tools/trl_probe.py [--out FILE]      (one JSON object; the record is profiles/r07/trl_probe.json)
    python tools/trl_probe.py --filter [--out FILE]   the Chebyshev filter (eigsh(filter_degree=...)): the filter step fused into the
                                                SpMV against SpMV + k_cheb_step, and filtered against unfiltered solves
                                                (the record is profiles/r08/trl_filter_probe.json)
    python tools/trl_probe.py --series [--out FILE]   the Chebyshev series of the interior mode (eigsh(sigma=..., filter_degree=...)):
                                                the series step fused into the SpMV against SpMV + k_cheb_series_step, and the
                                                eigenvalues nearest zero filtered against the unfiltered which="SM"
                                                (the record is profiles/r09/trl_series_probe.json)
    python tools/trl_probe.py --band [--out FILE]     band Lanczos (eigsh(block_size=b)): one batch of lz_trl_extend_band against b
                                                single-vector steps of lz_trl_extend at the same basis size, and block_size
                                                None / 2 / 4 solves with and without the filter
                                                (the record is profiles/r10/trl_band_probe.json)
    python tools/trl_probe.py --eigs [--out FILE]     Krylov-Schur (lanczos_amd.eigs): eigs(k=6, "LR") on a 3-D convection-diffusion
                                                grid of --eigs-n^3 rows (default 160: 4.1e6) against scipy.sparse.linalg.eigs
                                                (host ARPACK) with the same k, which, ncv and tol
                                                (the record is profiles/r17/trl_eigs_probe.json)

Times are host wall clock around calls that end in a stream synchronisation, median of several repetitions: a call's fixed cost
(~20 us: upload of S, launch, synchronisation) is included."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from lanczos_amd import Hamiltonian, _capi, synthetic  # noqa: E402
from lanczos_amd.eigsh import ChebFilter, DeviceBackend, SeriesFilter, trl, trl_band, trl_filtered, trl_interior, upload_matrix  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s


def median_time(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def restart_rate(h, M, m, kk, reps=20):
    rng = np.random.default_rng(1)
    h.trl_begin(m, rng.standard_normal(M))
    h.trl_extend(0, m)  # a real basis (the values do not matter for the rate)
    S = np.linalg.qr(rng.standard_normal((m, m)))[0][:, :kk].copy()
    t = median_time(lambda: h.trl_restart(m, kk, S), reps)
    nbytes = (m + kk) * M * 8.0
    return {"M": M, "m": m, "kk": kk, "us": t * 1e6, "bytes": nbytes, "TBps": nbytes / t / 1e12, "frac_hbm_peak": nbytes / t / HBM_PEAK}


def extend_step(h, M, m, k0, force, reps=5):
    h.set_options(_capi.FLAG_TRL_PASS2_ALWAYS if force else 0)
    rng = np.random.default_rng(2)
    h.trl_begin(m, rng.standard_normal(M))
    h.trl_extend(0, m)
    t = median_time(lambda: h.trl_extend(k0, m), reps)  # steps k0 .. m-1 on a full basis
    h.set_options(0)
    return t / (m - k0) * 1e6


def fixed_step(h, M, n0, n1, reps=3):
    v0 = np.random.default_rng(3).standard_normal(M)
    v0 /= np.linalg.norm(v0)
    t0 = median_time(lambda: h.run(n0, v0), reps)
    t1 = median_time(lambda: h.run(n1, v0), reps)
    return (t1 - t0) / (n1 - n0) * 1e6


def filter_step_rates(A, label, matrix_bytes_per_row, reps=21, d_lo=4, d_hi=36, series=False):
    """One filter step (product + recurrence) fused into the ELL SpMV against SpMV + k_cheb_step, on two handles that hold the same
    matrix, arms interleaved.  A step's time is the difference of lz_trl_filter_apply at degrees d_hi and d_lo over d_hi - d_lo: the
    upload of x and the download of y cancel.  k_cheb_step's own time: `--filter-trace` under a kernel trace.
    series: the step of the Chebyshev series instead (lz_trl_set_series; k_cheb_series_step), which also reads and writes the running
    sum.  Vector bytes per row, fused: x, the previous term and the sum read, the term and the sum written, 40; unfused: the SpMV reads x
    and writes w, the step reads w, two terms and the sum and writes the term and the sum, 64."""
    hs = {}
    for arm, flags in (("fused", 0), ("unfused", _capi.FLAG_TRL_FILTER_UNFUSED)):
        h = _capi.Handle(0)
        h.set_options(flags)
        n = upload_matrix(h, A)
        x = np.random.default_rng(4).standard_normal(n)
        m = 12
        h.trl_begin(m, x)
        hs[arm] = h
    # the damped interval holds the whole spectrum, so |p| < 1 and nothing overflows while it is timed: bounds from m plain steps
    # (theta_max + beta, theta_min - beta), widened by the width on either side
    proj, beta = h.trl_extend(0, m)
    T = np.triu(proj.T) + np.triu(proj.T, 1).T
    T[np.arange(m - 1), np.arange(1, m)] = T[np.arange(1, m), np.arange(m - 1)] = beta[: m - 1]
    th = np.linalg.eigvalsh(T)
    w = th[-1] - th[0] + 2 * beta[m - 1]
    lo, hi = th[0] - beta[m - 1] - w, th[-1] + beta[m - 1] + w
    if series:
        filt = {d: SeriesFilter(lo, hi, float(th[0] + 0.3 * (th[-1] - th[0])), d) for d in (d_lo, d_hi)}
    else:
        filt = {d: ChebFilter(lo, hi, lo - 0.05 * w, d) for d in (d_lo, d_hi)}
    ts = {(arm, d): [] for arm in hs for d in filt}
    for rep in range(reps + 2):  # two warm-up rounds
        for arm, h in hs.items():
            for d, f in filt.items():
                if series:
                    h.trl_set_series(f.coefficients(), f.c, f.e)
                else:
                    h.trl_set_filter(f.coefficients(), f.c)
                t = time.perf_counter()
                y_last = h.trl_filter_apply(x)
                if rep >= 2:
                    ts[(arm, d)].append(time.perf_counter() - t)
    for h in hs.values():
        h.close()
    out = {"matrix": label, "rows": n, "reps": reps, "degrees": [d_lo, d_hi], "matrix_bytes_per_row": matrix_bytes_per_row,
           "filter": {"lo": lo, "hi": hi, "ritz_min": float(th[0]), "ritz_max": float(th[-1])}, "finite": bool(np.isfinite(y_last).all())}
    for arm, vec_bytes in ((("fused", 40), ("unfused", 64)) if series else (("fused", 24), ("unfused", 40))):
        step = (float(np.median(ts[(arm, d_hi)])) - float(np.median(ts[(arm, d_lo)]))) / (d_hi - d_lo)
        nbytes = (vec_bytes + matrix_bytes_per_row) * n
        out[arm] = {"us_per_step": step * 1e6, "vector_bytes_per_row": vec_bytes, "TBps": nbytes / step / 1e12, "frac_hbm_peak": nbytes / step / HBM_PEAK}
    out["unfused_over_fused"] = out["unfused"]["us_per_step"] / out["fused"]["us_per_step"]
    return out


def solve_series(A, label, k, ncv, degrees, maxiter=None):
    """eigsh(k, 'SA') unfiltered and at every degree, on one handle in this order; a run that does not converge within maxiter cycles is recorded as such"""
    from scipy.sparse.linalg import ArpackNoConvergence

    h = _capi.Handle(0)
    n = upload_matrix(h, A)
    v0 = np.random.default_rng(3).standard_normal(n)
    runs = []
    for d in [None] + list(degrees):
        be = DeviceBackend(h, n)
        t = time.perf_counter()
        try:
            if d is None:
                theta, info = trl(be, n, k, "SA", ncv=ncv, v0=v0, maxiter=maxiter)
                info = dict(info, steps=info["matvecs"])
            else:
                theta, info = trl_filtered(be, n, k, "SA", d, ncv=ncv, v0=v0, maxiter=maxiter)
        except ArpackNoConvergence as e:
            runs.append({"filter_degree": d, "converged": False, "wall_s": time.perf_counter() - t, "note": str(e)})
            print(json.dumps(runs[-1]), flush=True)
            continue
        wall = time.perf_counter() - t
        res = h.trl_residuals(k, theta)
        runs.append({"filter_degree": d, "degree_used": info.get("filter", {}).get("degree"), "converged": True, "steps": info["steps"],
                     "A_products": info["matvecs"], "cycles": info["cycles"], "probes": info["probes"], "wall_s": wall,
                     "theta": theta.tolist(), "max_residual_over_anorm": float(res.max() / info["anorm"])})
        print(json.dumps(runs[-1]), flush=True)
    h.close()
    base = runs[0]["wall_s"] if runs[0]["converged"] else None
    for r in runs[1:]:
        r["unfiltered_over_this"] = base / r["wall_s"] if base and r["converged"] else None
    return {"matrix": label, "rows": n, "k": k, "which": "SA", "ncv": ncv, "maxiter": maxiter, "runs": runs}


def filter_probe(a):
    out = {}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    Hamiltonian.verbose = False
    N = a.deuteron_n
    ham = Hamiltonian(N, 25, synthetic.DeuteronPotential(), 197.327**2 / (2 * 469.4592) / (25.0 / N) ** 2)
    ham.device_potential = True
    op = ham.operator("27")
    H = synthetic.laplacian_2d_5pt(4000, a.rows // 4000)
    # matrix bytes per row of the row-class coded copies: one class byte (5-point, constant coefficients); class byte + the diagonal (27-point)
    out["step_lap2d"] = filter_step_rates(H, f"laplacian_2d_5pt 4000x{a.rows // 4000}", 1)
    print(json.dumps(out["step_lap2d"]), flush=True)
    save()
    out["step_deuteron"] = filter_step_rates(op, f"deuteron 27-point N={N}", 9)
    print(json.dumps(out["step_deuteron"]), flush=True)
    save()
    out["solve_deuteron"] = solve_series(op, f"deuteron 27-point N={N}", 4, None, (8, 16, 32))
    save()
    out["solve_lap2d"] = solve_series(H, f"laplacian_2d_5pt 4000x{a.rows // 4000}", 10, 41, (8, 16, 32), maxiter=a.maxiter)
    save()


def solve_nearest_zero(A, label, k, degrees, maxiter):
    """eigsh(k, which="SM") unfiltered, then the interior mode (sigma = 0) at every degree, on one handle in this order; a run that
    does not converge within maxiter cycles (per attempt of the interior mode) is recorded as such"""
    from scipy.sparse.linalg import ArpackNoConvergence

    h = _capi.Handle(0)
    n = upload_matrix(h, A)
    v0 = np.random.default_rng(3).standard_normal(n)
    runs = []
    for d in [None] + list(degrees):
        be = DeviceBackend(h, n)
        t = time.perf_counter()
        try:
            if d is None:
                theta, info = trl(be, n, k, "SM", v0=v0, maxiter=maxiter)
                info = dict(info, steps=info["matvecs"])
            else:
                theta, info = trl_interior(be, n, k, 0.0, d, v0=v0, maxiter=maxiter)
        except ArpackNoConvergence as e:
            runs.append({"filter_degree": d, "converged": False, "wall_s": time.perf_counter() - t, "note": str(e),
                         "attempts": getattr(e, "info", {}).get("filter", {}).get("attempts")})
            print(json.dumps(runs[-1]), flush=True)
            continue
        wall = time.perf_counter() - t
        res = h.trl_residuals(k, theta)
        f = info.get("filter", {})
        runs.append({"filter_degree": d, "degree_used": f.get("degree"), "converged": True, "steps": info["steps"], "A_products": info["matvecs"],
                     "cycles": info["cycles"], "probes": info["probes"], "wall_s": wall, "theta": theta.tolist(),
                     "max_residual_over_anorm": float(res.max() / info["anorm"]),
                     "attempts": [{key: (bool(v) if isinstance(v, (bool, np.bool_)) else v) for key, v in at.items()} for at in f.get("attempts", [])]})
        print(json.dumps(runs[-1]), flush=True)
    h.close()
    base = runs[0]["wall_s"] if runs[0]["converged"] else None
    for r in runs[1:]:
        r["unfiltered_over_this"] = base / r["wall_s"] if base and r["converged"] else None
    return {"matrix": label, "rows": n, "k": k, "which": "SM / sigma=0", "maxiter": maxiter, "runs": runs}


def deuteron(N):
    ham = Hamiltonian(N, 25, synthetic.DeuteronPotential(), 197.327**2 / (2 * 469.4592) / (25.0 / N) ** 2)
    ham.device_potential = True
    return ham.operator("27")


def series_probe(a):
    out = {}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    Hamiltonian.verbose = False
    N = a.deuteron_n
    op = deuteron(N)
    H = synthetic.laplacian_2d_5pt(4000, a.rows // 4000)
    out["step_lap2d"] = filter_step_rates(H, f"laplacian_2d_5pt 4000x{a.rows // 4000}", 1, series=True)
    print(json.dumps(out["step_lap2d"]), flush=True)
    save()
    out["step_deuteron"] = filter_step_rates(op, f"deuteron 27-point N={N}", 9, series=True)
    print(json.dumps(out["step_deuteron"]), flush=True)
    save()
    for n_solve in sorted({a.solve_n, N}):  # the small grid first: the one where the unfiltered loop finishes
        out[f"solve_deuteron_N{n_solve}"] = solve_nearest_zero(op if n_solve == N else deuteron(n_solve), f"deuteron 27-point N={n_solve}", 20,
                                                             (16, 32, 64), a.maxiter if n_solve == N else a.solve_maxiter)
        save()


def band_batch_rates(H, r0=36, reps=9):
    """One batch of b band steps (rows r0 .. r0 + b - 1 made from b products, four block sweeps over r0 rows and the in-batch tail) against
    b steps of the single-vector lz_trl_extend whose Gram-Schmidt sees r0 - b/2 + 1 .. r0 + b/2 rows, on two handles that hold the same
    matrix, arms interleaved.  Byte model: a sweep over r rows for c vectors moves (r + c) rows_pad 8 bytes, an update writes c more;
    the band batch is four sweeps (r0 rows, b vectors), the single-vector step four sweeps (j + 1 rows, one vector), second pass included
    (the gate "trips on nearly every step")."""
    out = []
    hs, hb = _capi.Handle(0), _capi.Handle(0)
    hs.set_options(_capi.FLAG_TRL_PASS2_ALWAYS)
    for h in (hs, hb):
        M = upload_matrix(h, H)
    pad = hs.padded_rows(M)
    rng = np.random.default_rng(5)
    for b in (2, 4, 8):
        ms = r0 + b // 2
        hs.trl_begin(ms, rng.standard_normal(M))
        hs.trl_extend(0, ms)
        hb.trl_begin_band(r0, rng.standard_normal((b, M)))
        hb.trl_extend_band(0, r0)
        tb, ts = [], []
        for rep in range(reps + 2):  # two warm-up rounds
            t = time.perf_counter()
            hb.trl_extend_band(r0 - b, r0)
            t1 = time.perf_counter()
            hs.trl_extend(ms - b, ms)
            t2 = time.perf_counter()
            if rep >= 2:
                tb.append(t1 - t)
                ts.append(t2 - t1)
        tb, ts = float(np.median(tb)), float(np.median(ts))
        bytes_band = (4 * (r0 + b) + 2 * b) * pad * 8.0
        bytes_single = sum(4 * (j + 2) + 2 for j in range(ms - b, ms)) * pad * 8.0
        out.append({"b": b, "rows": M, "r0": r0, "single_rows": f"{ms - b + 1}..{ms}", "reps": reps,
                    "band_us_per_row": tb / b * 1e6, "single_us_per_row": ts / b * 1e6, "single_over_band": ts / tb,
                    "band_model_bytes": bytes_band, "single_model_bytes": bytes_single, "model_bytes_ratio": bytes_single / bytes_band,
                    "band_frac_hbm_peak": bytes_band / tb / HBM_PEAK, "single_frac_hbm_peak": bytes_single / ts / HBM_PEAK})
        print(json.dumps(out[-1]), flush=True)
    hs.close()
    hb.close()
    return out


def solve_band(A, label, k, ncv=None, maxiter=None):
    """eigsh(k, 'SA') at block_size None / 2 / 4, without and with filter_degree = 16, on one handle in this order; a run that does not
    converge within maxiter cycles is recorded as such"""
    from scipy.sparse.linalg import ArpackNoConvergence

    h = _capi.Handle(0)
    n = upload_matrix(h, A)
    v0 = np.random.default_rng(3).standard_normal(n)
    runs = []
    for d in (None, 16):
        for b in (None, 2, 4):
            be = DeviceBackend(h, n, block_size=b)
            t = time.perf_counter()
            try:
                if d is not None:
                    theta, info = trl_filtered(be, n, k, "SA", d, ncv=ncv, v0=v0, maxiter=maxiter, block_size=b)
                elif b is None:
                    theta, info = trl(be, n, k, "SA", ncv=ncv, v0=v0, maxiter=maxiter)
                else:
                    theta, info = trl_band(be, n, k, "SA", b, ncv=ncv, v0=v0, maxiter=maxiter)
            except ArpackNoConvergence as e:
                runs.append({"block_size": b, "filter_degree": d, "converged": False, "wall_s": time.perf_counter() - t, "note": str(e)})
                print(json.dumps(runs[-1]), flush=True)
                continue
            wall = time.perf_counter() - t
            res = h.trl_residuals(k, theta)
            runs.append({"block_size": b, "filter_degree": d, "converged": True, "steps": info.get("steps", info["matvecs"]),
                         "A_products": info["matvecs"], "cycles": info["cycles"], "probes": info["probes"], "breakdowns": info["breakdowns"],
                         "wall_s": wall, "theta": theta.tolist(), "max_residual_over_anorm": float(res.max() / info["anorm"])})
            print(json.dumps(runs[-1]), flush=True)
    h.close()
    return {"matrix": label, "rows": n, "k": k, "which": "SA", "ncv": ncv or "default", "maxiter": maxiter, "runs": runs}


def band_probe(a):
    out = {}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    Hamiltonian.verbose = False
    if a.no_batch and a.out and os.path.exists(a.out):  # keep the batch record of an earlier run
        with open(a.out) as f:
            out.update(json.load(f))
    if not a.no_batch:
        H = synthetic.laplacian_2d_5pt(4000, a.rows // 4000)
        out["batch_lap2d"] = band_batch_rates(H)
        save()
    N = a.deuteron_n
    op = deuteron(N)
    for ncv in (None, 40):  # the default, and room for the band (see trl_band)
        out[f"solve_deuteron_ncv{ncv or 'default'}"] = solve_band(op, f"deuteron 27-point N={N}", 4, ncv=ncv, maxiter=a.band_maxiter)
        save()


def convdiff3d(N, p=(0.3, 0.2, 0.1)):
    """7-point convection-diffusion on an N^3 grid, Dirichlet: diagonal 6, off-diagonals -1 -+ p per axis (non-symmetric, real spectrum)"""
    import scipy.sparse as sp

    def line(q):
        return sp.diags([np.full(N - 1, -1.0 - q), np.full(N, 2.0), np.full(N - 1, -1.0 + q)], [-1, 0, 1], format="csr")

    I = sp.identity(N, format="csr")
    A = sp.kron(I, sp.kron(I, line(p[0]))) + sp.kron(I, sp.kron(line(p[1]), I)) + sp.kron(line(p[2]), sp.kron(I, I))
    A = A.tocsr()
    A.sort_indices()
    return A


def eigs_probe(a):
    """lanczos_amd.eigs(k=6, which="LR") against scipy.sparse.linalg.eigs on the same matrix: wall time of the whole call (the device
    call includes the upload of the matrix), restart cycles, products, and the true residuals of both measured on the host"""
    import scipy.sparse.linalg as sla

    import lanczos_amd

    N, k, which, tol = a.eigs_n, 6, "LR", a.eigs_tol
    A = convdiff3d(N)
    n = A.shape[0]
    out = {"matrix": f"3-D convection-diffusion {N}^3, p = (0.3, 0.2, 0.1)", "rows": n, "nnz": int(A.nnz), "k": k, "which": which, "tol": tol,
           "ncv": "default (20)"}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    def residual(w, X):
        return float((np.linalg.norm(A @ X - X * w, axis=0)).max() / np.abs(w).max())

    h = _capi.Handle(0)
    for rep in range(2):  # the second call runs on a warm handle (kernels loaded, buffers allocated)
        info = {}
        t = time.perf_counter()
        try:
            w, X = lanczos_amd.eigs(A, k=k, which=which, tol=tol, maxiter=a.eigs_maxiter, handle=h, info=info)
        except sla.ArpackNoConvergence as e:
            out[f"device_run{rep}"] = {"converged": False, "wall_s": time.perf_counter() - t, "note": str(e)}
            print(json.dumps(out[f"device_run{rep}"]), flush=True)
            continue
        wall = time.perf_counter() - t
        out[f"device_run{rep}"] = {"converged": True, "wall_s": wall, "cycles": info["cycles"], "A_products": info["matvecs"],
                                   "breakdowns": info["breakdowns"], "w": [[z.real, z.imag] for z in w],
                                   "max_residual_over_max_w_host": residual(w, X),
                                   "max_residual_over_anorm_device": float(info["residuals"].max() / info["anorm"])}
        print(json.dumps(out[f"device_run{rep}"]), flush=True)
        save()
    h.close()
    if not a.no_host:
        t = time.perf_counter()
        try:
            w, X = sla.eigs(A, k=k, which=which, tol=tol, maxiter=a.eigs_maxiter)
            out["host_arpack"] = {"converged": True, "wall_s": time.perf_counter() - t, "w": [[z.real, z.imag] for z in w],
                                  "max_residual_over_max_w_host": residual(w, X), "threads": os.environ.get("OMP_NUM_THREADS")}
        except sla.ArpackNoConvergence as e:
            out["host_arpack"] = {"converged": False, "wall_s": time.perf_counter() - t, "note": str(e)}
        print(json.dumps(out["host_arpack"]), flush=True)
    save()


def filter_trace(a):
    """A short run for `rocprofv3 --kernel-trace --stats -- python tools/trl_probe.py --filter-trace`: ten degree-16 filter applications
    on each arm and matrix, so that the trace's per-kernel averages give k_cheb_step, the plain SpMV and the fused SpMV step."""
    Hamiltonian.verbose = False
    N = a.deuteron_n
    ham = Hamiltonian(N, 25, synthetic.DeuteronPotential(), 197.327**2 / (2 * 469.4592) / (25.0 / N) ** 2)
    ham.device_potential = True
    for A in (synthetic.laplacian_2d_5pt(4000, a.rows // 4000), ham.operator("27")):
        for flags in (0, _capi.FLAG_TRL_FILTER_UNFUSED):
            h = _capi.Handle(0)
            h.set_options(flags)
            n = upload_matrix(h, A)
            x = np.random.default_rng(4).standard_normal(n)
            h.trl_begin(2, x)
            f = ChebFilter(-1.0e6, 1.0e6, -1.1e6, 16)  # (degree 16 of values inside the damped interval: bounded whatever the spectrum)
            h.trl_set_filter(f.coefficients(), f.c)
            for _ in range(10):
                h.trl_filter_apply(x)
            h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--filter", action="store_true", help="probe the Chebyshev filter instead (see the module docstring)")
    ap.add_argument("--series", action="store_true", help="probe the Chebyshev series of the interior mode instead (see the module docstring)")
    ap.add_argument("--band", action="store_true", help="probe band Lanczos (eigsh(block_size=...)) instead (see the module docstring)")
    ap.add_argument("--no-batch", action="store_true", help="--band: the solves only (the batch record in --out is kept)")
    ap.add_argument("--band-maxiter", type=int, default=3000, help="--band: restart cycles allowed to each solve")
    ap.add_argument("--solve-n", type=int, default=48, help="--series: a second, smaller deuteron grid for the solves")
    ap.add_argument("--solve-maxiter", type=int, default=4000, help="--series: restart cycles allowed to each solve on the smaller grid")
    ap.add_argument("--eigs", action="store_true", help="probe Krylov-Schur (lanczos_amd.eigs) instead (see the module docstring)")
    ap.add_argument("--eigs-n", type=int, default=160, help="--eigs: the grid is eigs-n^3")
    ap.add_argument("--eigs-tol", type=float, default=1e-10, help="--eigs: tol of both solvers")
    ap.add_argument("--eigs-maxiter", type=int, default=20000, help="--eigs: restart cycles allowed to each solver")
    ap.add_argument("--no-host", action="store_true", help="--eigs: skip the host ARPACK run")
    ap.add_argument("--filter-trace", action="store_true", help="the short run meant for a kernel trace (see filter_trace)")
    ap.add_argument("--deuteron-n", type=int, default=160)
    ap.add_argument("--maxiter", type=int, default=400, help="--filter: restart cycles allowed to each solve on the 2-D Laplacian; --series: to "
                    "each solve (each attempt of the interior mode)")
    a = ap.parse_args()
    if a.filter_trace:
        return filter_trace(a)
    if a.filter:
        return filter_probe(a)
    if a.series:
        return series_probe(a)
    if a.band:
        return band_probe(a)
    if a.eigs:
        return eigs_probe(a)
    out = {}
    M = a.rows
    H = synthetic.laplacian_2d_5pt(4000, M // 4000)  # the headline's matrix family at M = 1e7
    h = _capi.Handle(0)
    h.set_csr(H.shape[0], 0, H.rowptr, H.colidx, H.vals)
    M = H.shape[0]
    out["restart"] = restart_rate(h, M, 41, 30)
    print(json.dumps(out["restart"]), flush=True)
    m, k0 = 41, 31
    gated = extend_step(h, M, m, k0, False)
    forced = extend_step(h, M, m, k0, True)
    fixed = fixed_step(h, M, k0, m)
    out["extend"] = {"M": M, "basis_rows": f"{k0 + 1}..{m}", "us_per_step_gated": gated, "us_per_step_forced": forced,
                     "us_per_step_fixed_n": fixed, "gated_over_fixed": gated / fixed}
    print(json.dumps(out["extend"]), flush=True)
    h.close()
    Hamiltonian.verbose = False
    N = 160
    ham = Hamiltonian(N, 25, synthetic.DeuteronPotential(), 197.327**2 / (2 * 469.4592) / (25.0 / N) ** 2)
    ham.device_potential = True
    op = ham.operator("27")
    h = _capi.Handle(0)
    n = upload_matrix(h, op)
    t = time.perf_counter()
    theta, info = trl(DeviceBackend(h, n), n, 4, "SA")
    wall = time.perf_counter() - t
    res = h.trl_residuals(4, theta)
    h.close()
    out["deuteron"] = {"N": N, "rows": n, "k": 4, "which": "SA", "theta": theta.tolist(), "matvecs": info["matvecs"], "cycles": info["cycles"],
                       "probes": info["probes"], "wall_s": wall, "max_residual_over_anorm": float(res.max() / info["anorm"])}
    print(json.dumps(out["deuteron"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
