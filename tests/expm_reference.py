"""The exact reference of ``expm_multiply`` and the matrices its tests share: ``exact(A, b, a, times)`` through ``numpy.linalg.eigh``
of the dense matrix - for a Hermitian ``A``, ``exp(a t A) b = U (exp(a t lambda) * (U^H b))``, whose error is a few ``eps`` times the
norm of the result while ``|exp(a t lambda)|`` stays moderate (the tests keep the growth below about 1e4).

A plain module: no fixtures, nothing collected from it."""
import functools

import numpy as np
import scipy.sparse as sp

from lanczos_amd import synthetic


def dense_of(A):
    if sp.issparse(A):
        return A.toarray()
    if hasattr(A, "to_scipy"):
        return A.to_scipy().toarray()
    return np.asarray(A)


def exact(A, b, a, times):
    """``(len(times), n)`` complex128: ``exp(a t A) b`` for every ``t``"""
    lam, U = np.linalg.eigh(dense_of(A))
    y = U.conj().T @ np.asarray(b).reshape(-1)
    return np.stack([U @ (np.exp(a * t * lam) * y) for t in np.atleast_1d(times)])


@functools.lru_cache(maxsize=None)
def matrix(name):
    """the three matrices of the accuracy tests: a real stencil, a complex Hermitian sparse one, a real dense one"""
    if name == "lap20":
        return synthetic.laplacian_2d_5pt(20, 20).to_scipy()
    if name == "hof24x17":
        return synthetic.hofstadter(24, 17, 1 / 8)
    assert name == "dense96"
    G = np.random.default_rng(96).standard_normal((96, 96))
    return (G + G.T) / 2  # eigenvalues within about [-14, 14]


def vector(n, cplx, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n) if cplx else rng.standard_normal(n)


def rel_errors(out, ref):
    """per time: ``|out - ref| / |ref|``"""
    out, ref = np.asarray(out).reshape(ref.shape), np.asarray(ref)
    return np.linalg.norm(out - ref, axis=1) / np.linalg.norm(ref, axis=1)
