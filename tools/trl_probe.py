"""Thick-restart Lanczos (lanczos_amd.eigsh) on the device: the restart kernel's rate, the extension step with and without the DGKS
gate next to the fixed-n loop's step, and one eigsh run on the device-assembled deuteron Hamiltonian.

    python tools/trl_probe.py [--out FILE]      (one JSON object; the record is profiles/r07/trl_probe.json)

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
from lanczos_amd.eigsh import DeviceBackend, trl, upload_matrix  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=10_000_000)
    a = ap.parse_args()
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
