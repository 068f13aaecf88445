"""CPU restatement of the seeded sampler of include/gcnmaxcut.h (gmc_decode_sample_seeded_f32), written from the
header's draw rule in vectorised numpy ``uint64`` arithmetic (which wraps modulo 2^64) - independently of the product's
host form (``TestingNeuralNetwork.assign_partitions_seeded``: Python integers, one node at a time).

``keys`` are the graphs' keys, ``hashes`` / ``uniforms`` the [iters, n] draws of one graph (columns 0..2 are defined
but never used: the terminals take no draw), ``assignments`` its samples; ``sample`` adds the cuts (the edge counting
of tests/refine_ref.py, float64, rounded to the float32 the kernel reports - exact for unit and small-integer weights)
and the pick (strictly best, first on ties)."""
import numpy as np

from tests import refine_ref as RR
from tests.util import mix64

U = np.uint64
GOLD = U(0x9E3779B97F4A7C15)


def keys(seed, indices):
    """mix64(seed + GOLD * (index + 1)) for every index: [len(indices)] uint64."""
    idx = np.asarray(list(indices), np.uint64)
    with np.errstate(over="ignore"):
        return mix64(U(int(seed) & (2 ** 64 - 1)) + GOLD * (idx + U(1)))


def hashes(key, iters, n, first_iter=0):
    """h of iterations first_iter .. first_iter+iters-1 (rows) and local nodes 0..n-1 (columns): [iters, n] uint64."""
    it = np.arange(first_iter, first_iter + iters, dtype=np.uint64)[:, None]
    l = np.arange(n, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        return mix64(U(key) + GOLD * (((it << U(32)) | l) + U(1)))


def uniforms(key, iters, n, first_iter=0):
    """u = (double)(h >> 11) * 2^-53 in [0, 1): [iters, n] float64 (the conversion of a 53-bit integer is exact)."""
    return (hashes(key, iters, n, first_iter) >> U(11)).astype(np.float64) * 2.0 ** -53


def assignments(P, key, iters, first_iter=0):
    """P [n, 3] float32 -> [iters, n] int8: nodes 0,1,2 fixed, node l >= 3 class 0 if u < c0, else 1 if u < c1, else 2,
    with c0 = (double)p[0] and c1 = c0 + (double)p[1]."""
    P = np.asarray(P)
    assert P.dtype == np.float32 and P.ndim == 2 and P.shape[1] == 3
    n = P.shape[0]
    u = uniforms(key, iters, n, first_iter)
    c0 = P[:, 0].astype(np.float64)
    c1 = c0 + P[:, 1].astype(np.float64)
    a = np.where(u < c0[None, :], 0, np.where(u < c1[None, :], 1, 2)).astype(np.int8)
    a[:, :min(n, 3)] = np.arange(min(n, 3), dtype=np.int8)
    return a


def sample(handle, P, key, iters):
    """What the entry point reports for one graph: assign_all [iters, n] int8, cut_all [iters] float32, best_assign
    [n] int32, best_cut (float32), best_iter."""
    a = assignments(P, key, iters)
    cuts = np.array([RR.cut(handle.rowptr, handle.col, handle.weight, row) for row in a])
    cut_all = cuts.astype(np.float32)
    assert (cut_all.astype(np.float64) == cuts).all()       # the cases the tests use have exactly representable cuts
    bi = int(np.argmax(cut_all))                            # the first of the largest
    return dict(assign_all=a, cut_all=cut_all, best_assign=a[bi].astype(np.int32), best_cut=cut_all[bi], best_iter=bi)
