"""The forms of the two-pass sweep that exist only inside lz_run - pass 1 on two columns (mode 3, one-reduce), the fused
small-problem engine (mode 4), pass 2 reading raw sums (raw_c = 1, 2), the gated sweep of the partial loops - driven through 20
steps of lz_run, so that nrows passes 8 and 16 and the row split engages, and compared with a longdouble Lanczos run of the same
full sweep (reorth_reference.lanczos_longdouble).

Every run asserts the engine its id names (last_engine()).  Tolerance: per matrix and per quantity (alpha, beta, basis) 8 times the
deviation of the float64 oracle (oracle/lanczos_ref.py) from the longdouble run, computed here on the CPU OVER THE SAME STEPS as the
device's - the factor covers another summation order over at most 20 steps of a recurrence that amplifies rounding.

A partial-flag run is compared up to its first skipped sweep (last_sweep_log()), and so is the oracle it is held to.  On all four
matrices that is ONE step - step 0 always sweeps, step 1 never does: nothing is yet there to lose orthogonality to - so these runs
check alpha[0] and row 0 after the one-row sweep of step 0 and the engine, and do NOT cover a gated sweep at nrows > 1; the partial
loops' later sweeps are held to the full sweep's Ritz values elsewhere (tests/test_gpu_lanczos.py, tests/test_partial_gates.py).  The
host-decided partial loop keeps no per-step record: its window is the device-decided loop's on the same matrix, and the run must
report that record's number of sweeps (last_sweeps()), or the borrowed window is wrong and the test says so.

tests/golden/reorth_loop_margins.json records, per run, the device's deviations and the oracle's over the same steps as measured on
an MI355X, and the deviations of the float64 restatement of the one-reduce loops (oracle.execute_lanczos_one_reduce).  Recorded
results only: nothing reads it as a tolerance.  To regenerate it run this module on the device with REORTH_LOOP_MARGINS_OUT set to
the file to write.

(The "mfma2x8" one-reduce runs repeat the default's bits: step_onereduce_head sets the plan's variant to 0, knob 1 does not reach mode 3.)"""
import functools
import json
import os

import numpy as np
import pytest
import reorth_reference as R
import scipy.sparse
from oracle import lanczos_ref as oracle

from lanczos_amd import synthetic

pytestmark = pytest.mark.gpu

N_STEPS = 20
FACTOR = 8.0
# name -> (knob 0, G): the slices of pass 1
MATRICES = {"lap23x29-G1": (1024, 1), "lap61x67-G8": (512, 8), "lap62x67-G9": (512, 9), "dense300-G1": (0, 1)}
FLAGS = {"plain": 0, "fused": 16, "one-reduce": 16 | 256, "partial": 64 | 16, "partial-one-reduce": 64 | 16 | 256}
KERNELS = {"default": (0, 0), "mfma2x8": (0, 11), "valu": (R.FLAG_VALU, 0)}  # (extra flag, knob 1)


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name.startswith("dense"):
        return synthetic.dense_symmetric(300, seed=7)
    nx, ny = (int(s) for s in name[3 : name.index("-")].split("x"))
    L = synthetic.laplacian_2d_5pt(nx, ny).to_scipy()
    A = (L + scipy.sparse.diags(np.random.default_rng(nx).uniform(0.0, 4.0, L.shape[0]))).tocsr()  # a random diagonal: no degenerate levels
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def references(name):
    """(v0, the longdouble run, the float64 oracle's run)"""
    A = matrix(name)
    v0 = synthetic.reference_start_vector(A.shape[0])
    v0 /= np.linalg.norm(v0)
    exact = R.lanczos_longdouble(A, N_STEPS, v0)
    return v0, exact, oracle.execute_lanczos(A, N_STEPS, v0=v0, economy=True)


@functools.lru_cache(maxsize=None)
def oracle_deviations(name, k):
    """the oracle's deviation from the longdouble run over the first k steps, per quantity"""
    _, exact, (a, b, V) = references(name)
    return deviations(exact, a, b, V, k)


def deviations(exact, a, b, V, k):
    """max |difference| over the first k steps: alpha[:k], beta[:k - 1], V[:k]"""
    ea, eb, eV = exact
    return {"alpha": float(np.abs(a[:k] - ea[:k]).max()), "beta": float(np.abs(b[: k - 1] - eb[: k - 1]).max()) if k > 1 else 0.0,
            "basis": float(np.abs(V[:k] - eV[:k]).max())}


_LOGS = {}


def device_sweep_log(hip, name):
    """last_sweep_log() of the device-resident partial loop on this matrix, default kernels"""
    if name not in _LOGS:
        A = matrix(name)
        h = hip.Handle(0)
        try:
            h.set_options(FLAGS["partial"])
            h.set_tuning(0, MATRICES[name][0])
            if scipy.sparse.issparse(A):
                h.set_csr(A.shape[0], 0, A.indptr, A.indices, A.data)
            else:
                h.set_dense(A)
            h.run(N_STEPS, references(name)[0])
            assert h.last_engine() == "partial-device"
            _LOGS[name] = h.last_sweep_log()
        finally:
            h.close()
    return _LOGS[name]


def run_variant(hip, name, flags_name, kernels_name):
    """(engine, expected engine, steps compared, the device's deviations)"""
    A = matrix(name)
    knob0, G = MATRICES[name]
    extra, knob1 = KERNELS[kernels_name]
    flags = FLAGS[flags_name] | extra
    knob15 = 1 if flags_name == "plain" else 0
    v0, exact, _ = references(name)
    h = hip.Handle(0)
    try:
        h.set_options(flags)
        h.set_tuning(0, knob0)
        h.set_tuning(1, knob1)
        h.set_tuning(15, knob15)
        if scipy.sparse.issparse(A):
            h.set_csr(A.shape[0], 0, A.indptr, A.indices, A.data)
        else:
            h.set_dense(A)
        a, b = h.run(N_STEPS, v0)
        V = h.get_basis()
        engine = h.last_engine()
        host_decided = bool(flags & R.FLAG_PARTIAL) and engine == "kernels"
        log = None if host_decided else h.last_sweep_log()
        sweeps = h.last_sweeps()
    finally:
        h.close()
    assert R.plan_qtw(R.padded(A.shape[0]), flags, {0: knob0}, N_STEPS)[1] == G
    if log is None:
        # The host-decided partial loop (other pass-1 kernels than the default) keeps no per-step record.  It runs Simon's exact
        # test, the one the device-resident loop runs on the default kernels (bit-identical decisions on equal coefficients,
        # tests/test_gpu_lanczos.py): that run's record says how far the sweeps were full.
        log = device_sweep_log(hip, name)
        assert sweeps == int(log.sum()), f"the host-decided loop swept {sweeps} times, the borrowed record {int(log.sum())} times: the window is not this run's"
    skipped = np.flatnonzero(~log)
    k = int(skipped[0]) if skipped.size else N_STEPS
    if not flags & R.FLAG_PARTIAL:
        assert k == N_STEPS, "a full re-orthogonalisation run skipped a sweep"
    return engine, R.expected_engine(flags, knob1, knob15, G), k, deviations(exact, a, b, V, k)


def variants():
    """(matrix, flags, kernels, the engine choose_loop takes for them): the engine is part of the id"""
    out = []
    for name, (_, G) in MATRICES.items():
        for flags_name, flags in FLAGS.items():
            for kernels_name, (extra, knob1) in KERNELS.items():
                out.append((name, flags_name, kernels_name, R.expected_engine(flags | extra, knob1, 1 if flags_name == "plain" else 0, G)))
    return out


def record(name, flags_name, kernels_name, engine, k, dev, ref):
    """REORTH_LOOP_MARGINS_OUT=<file>: write this run's figures into that file (how tests/golden/reorth_loop_margins.json is made)"""
    path = os.environ.get("REORTH_LOOP_MARGINS_OUT")
    if not path:
        return
    d = {"steps": N_STEPS, "factor": FACTOR, "device": {}, "one_reduce_float64": {}}
    if os.path.isfile(path):
        with open(path) as f:
            d = json.load(f)
    d["device"][f"{name}-{flags_name}-{kernels_name}"] = dict(dev, engine=engine, steps_compared=k, oracle_same_steps=ref)
    for partial in (False, True):
        key = name + ("-partial" if partial else "")
        if key not in d["one_reduce_float64"]:
            A = matrix(name)
            v0, exact, _ = references(name)
            a, b, V, gates, _ = oracle.execute_lanczos_one_reduce(A, N_STEPS, [0, A.shape[0]], v0=v0, partial=partial)
            kk = gates.index(False) if False in gates else N_STEPS
            d["one_reduce_float64"][key] = dict(deviations(exact, a, b, V, kk), steps_compared=kk, oracle_same_steps=oracle_deviations(name, kk))
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.mark.parametrize("name,flags_name,kernels_name,want", variants(), ids=lambda v: str(v))
def test_run_loop_against_longdouble(hip, name, flags_name, kernels_name, want):
    engine, expected, k, dev = run_variant(hip, name, flags_name, kernels_name)
    assert k >= 1
    ref = oracle_deviations(name, k)
    print(f"{name} {flags_name} {kernels_name}: engine {engine}, {k} steps compared, device {dev}, oracle over the same steps {ref}")
    record(name, flags_name, kernels_name, engine, k, dev, ref)
    assert engine == want == expected
    for q in ("alpha", "beta", "basis"):
        assert dev[q] <= FACTOR * ref[q], f"{q}: the device deviates by {dev[q]:.3e}, the oracle by {ref[q]:.3e} ({dev[q] / max(ref[q], 1e-300):.2f}x)"
