"""Host checks of the one-sweep loop's per-step arithmetic (no GPU): the library's host evaluation of the predict / post
expressions - the ones its kernels run - against the NumPy prototype (tools/one_sweep_prototype.py), and the prototype's
loop against the oracle."""
import ctypes as C
import os
import sys

import numpy as np

import lanczos_amd
from conftest import load_golden
from oracle import lanczos_ref as oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import one_sweep_prototype as proto  # noqa: E402


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_host_predict_and_post_match_the_prototype_bit_for_bit():
    _, H = load_golden("lap2d_32x32_n30")
    n = 30
    _, _, V, st = proto.one_sweep_lanczos(H, n, tau=1e-14, fast=False)
    G = np.ascontiguousarray(st["G"])
    rng = np.random.default_rng(3)
    lib = lanczos_amd.load_library()
    for j in (0, 1, 7, n - 2):
        Hm = np.triu(rng.standard_normal((n, n)), -1)  # upper Hessenberg, like the recurrence's
        a, bj, nrm2 = 2.5, 1.75, 3.2
        want = proto.predict(G, Hm, a, bj if j else 0.0, nrm2, j)
        got = np.zeros(j + 1)
        assert lib.lz_one_sweep_host_predict(n, j, _dp(np.ascontiguousarray(Hm.T)), _dp(G), a, bj, nrm2, _dp(got)) == 0
        assert np.array_equal(got, want), j
        if j == 0:
            continue
        du = rng.standard_normal(j + 1) * 1e-16
        chat = rng.standard_normal(j) * 1e-16
        _, col = proto.post(G, du, 1.0, chat, nrm2 / (np.sqrt(nrm2) ** 2), j)
        got = np.zeros(j)
        assert lib.lz_one_sweep_host_post(n, j, _dp(G), _dp(du), _dp(chat), nrm2, _dp(got)) == 0
        assert np.array_equal(got, col[:j]), j


def test_prototype_meets_the_bars_on_a_fixture():
    d, H = load_golden("graph_M2000_E7000_n40")
    n = int(d["n"])
    a0, b0, V0 = oracle.execute_lanczos(H, n, economy=True)
    a1, b1, V1, st = proto.one_sweep_lanczos(H, n, tau=1e-14)
    scale = np.abs(np.linalg.eigvalsh(oracle.build_h_eff(a0, b0))).max()
    assert st["trips"] == [] and st["emax"].max() < 1e-14
    assert np.abs(V1 @ V1.T - np.eye(n)).max() < 1e-13
    assert np.abs(a1 - a0).max() <= 1e-12 * scale and np.abs(b1 - b0).max() <= 1e-12 * scale
