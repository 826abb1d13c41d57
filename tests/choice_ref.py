"""Numpy restatement of the device draw of sam6d_hip.inputs.draw_choice (csrc/choice.hip), code of its own: uint64 arithmetic masked
to 32 bits and a stable argsort.  All arithmetic is modulo 2^32:

    fmix(x):  x ^= x >> 16;  x *= 0x85ebca6b;  x ^= x >> 13;  x *= 0xc2b2ae35;  x ^= x >> 16      (murmur3's finaliser, a bijection)
    a    = fmix(seed ^ 0x9E3779B9)
    b    = fmix(a + row)                  row = global row index of the draw
    h(r) = fmix(fmix(r ^ b) + a)          a bijection of r: a row has no ties

Row `row` with n candidates and ns wanted indices: n > ns -> the ns values r in [0, n) with the smallest h(r), in ascending order of
h; 1 <= n <= ns -> sel[j] = (h(j) * n) >> 32; n <= 0 -> zeros.  n above 2^24 counts as 2^24.
"""
import functools

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
N_MAX = 1 << 24


def fmix(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & M32
    return x ^ (x >> np.uint64(16))


def keys(seed, row, r):
    """h(r) for the rows `row` (a scalar, or an array that broadcasts against r) as uint64 values below 2^32"""
    a = fmix(np.uint64(int(seed) & 0xFFFFFFFF) ^ np.uint64(0x9E3779B9))
    b = fmix((a + (np.asarray(row, dtype=np.uint64) & M32)) & M32)
    r = np.asarray(r, dtype=np.uint64)
    return fmix((fmix(r ^ b) + a) & M32)


@functools.lru_cache(maxsize=64)
def _order(seed, row, n):
    """all n candidates of a row in ascending order of h (shared by the draws of every ns from the same row)"""
    o = np.argsort(keys(seed, row, np.arange(n)), kind="stable").astype(np.int32)
    o.setflags(write=False)
    return o


def draw_row(seed, row, n, ns):
    n = min(int(n), N_MAX)
    if n <= 0:
        return np.zeros(ns, np.int32)
    if n <= ns:
        return ((keys(seed, row, np.arange(ns)) * np.uint64(n)) >> np.uint64(32)).astype(np.int32)
    return _order(int(seed), int(row), n)[:ns].copy()


def draw(n, ns, seed, row0=0):
    """sel (N, ns) int32 for the candidate counts n (N): row i is global row row0 + i"""
    n = np.asarray(n).reshape(-1)
    return np.stack([draw_row(seed, row0 + i, v, ns) for i, v in enumerate(n)]) if n.size else np.zeros((0, ns), np.int32)


def draw_rows(seed, rows, n, ns):
    """the draws of many rows that share one n, vectorised: (len(rows), ns) int32"""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    if n <= ns:
        return ((keys(seed, rows, np.arange(ns)[None]) * np.uint64(n)) >> np.uint64(32)).astype(np.int32)
    return np.argsort(keys(seed, rows, np.arange(n)[None]), axis=1, kind="stable")[:, :ns].astype(np.int32)
