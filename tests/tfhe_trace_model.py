"""Plain model of the TGLWE automorphism key switch, the trace and the ring packing (k = 1), written from the definitions in
include/fhe_ring.h in Python integers, on top of tfhe_mul_model (negacyclic, gadget_sum, encrypt, phase):

  sigma_g   : coefficient i goes to i g mod 2n, a position >= n means position - n with the sign flipped
  key       : AK_{g,j} encrypts -h_j sigma_g(S), h_j = 2^(64 - log_b (d - j))
  autks_g   : out_a = sum_j digit_j(sigma_g(a)) AK_{g,j}.a,  out_b = sigma_g(b) + sum_j digit_j(sigma_g(a)) AK_{g,j}.b   mod 2^64
  trace     : for u = hi .. lo + 1: ct <- ct + autks_{2^u + 1}(ct)
  embed     : the inverse of sample_extract(0)
  merge_l   : (E, O) -> (E + X^(n/l) O) + autks_{l+1}(E - X^(n/l) O)
  ring_pack : P(x) = embed(x); P(x_0 .. x_{m-1}) = merge_m(P(evens), P(odds)); out = trace(P(all), lo = log2 count, hi = log2 n)

Ciphertexts are pairs of lists of Python integers in [0, 2^64); keys are dicts g -> (rows_a, rows_b) [d][n]."""
import numpy as np

from tfhe_mul_model import M64, gadget_sum


def log2(n):
    return int(n).bit_length() - 1


def galois_set(n):
    return [(1 << u) + 1 for u in range(1, log2(n) + 1)]


def sigma(p, g):
    n = len(p)
    out = [0] * n
    for i, v in enumerate(p):
        m = (i * g) % (2 * n)
        out[m % n] = int(v) % M64 if m < n else (-int(v)) % M64
    return out


def index_table(n, g):
    """[(target, negated)] for every coefficient: what csrc/tfhe_trace.hpp's auto_target returns"""
    return [((i * g) % (2 * n) % n, (i * g) % (2 * n) >= n) for i in range(n)]


def rotate(p, r):
    """X^r p, 0 <= r < 2n"""
    n = len(p)
    out = [0] * n
    for i, v in enumerate(p):
        m = (i + r) % (2 * n)
        out[m % n] = int(v) % M64 if m < n else (-int(v)) % M64
    return out


def atk_plain(log_b, d, sk, gs):
    """the plaintext rows of a key set: [len(gs)][d][n] uint64, row (q, j) = -2^(64 - log_b (d - j)) sigma_{gs[q]}(S) mod 2^64"""
    n = len(sk)
    out = np.zeros((len(gs), d, n), dtype=np.uint64)
    for q, g in enumerate(gs):
        s = sigma([int(v) for v in sk], g)
        for j in range(d):
            out[q, j] = np.array([(-(v << (64 - log_b * (d - j)))) % M64 for v in s], dtype=np.uint64)
    return out


def autks(log_b, d, key, g, ct):
    a, b = ct
    ra, rb = key[g]
    pa, pb = sigma(a, g), sigma(b, g)
    sa, sb = gadget_sum(log_b, d, pa, ra, rb)
    return [x % M64 for x in sa], [(x + y) % M64 for x, y in zip(pb, sb)]


def add(x, y):
    return [(u + v) % M64 for u, v in zip(x[0], y[0])], [(u + v) % M64 for u, v in zip(x[1], y[1])]


def sub(x, y):
    return [(u - v) % M64 for u, v in zip(x[0], y[0])], [(u - v) % M64 for u, v in zip(x[1], y[1])]


def trace(log_b, d, key, ct, lo, hi):
    ct = ([int(v) for v in ct[0]], [int(v) for v in ct[1]])
    for u in range(hi, lo, -1):
        ct = add(ct, autks(log_b, d, key, (1 << u) + 1, ct))
    return ct


def embed(a, b):
    """TLWE (a' [n], b') -> TGLWE (a, b)"""
    n = len(a)
    return [int(a[0])] + [(-int(a[n - i])) % M64 for i in range(1, n)], [int(b) % M64] + [0] * (n - 1)


def sample_extract0(ct):
    a, b = ct
    n = len(a)
    return [int(a[0])] + [(-int(a[n - j])) % M64 for j in range(1, n)], int(b[0])


def merge(log_b, d, key, l, E, O):
    n = len(E[0])
    R = (rotate(O[0], n // l), rotate(O[1], n // l))
    return add(add(E, R), autks(log_b, d, key, l + 1, sub(E, R)))


def tree(log_b, d, key, cts):
    """P(x_0 .. x_{m-1}); cts: list of TLWE (a' [n], b')"""
    m = len(cts)
    if m == 1:
        return embed(*cts[0])
    return merge(log_b, d, key, m, tree(log_b, d, key, cts[0::2]), tree(log_b, d, key, cts[1::2]))


def ring_pack(log_b, d, key, cts):
    n = len(cts[0][0])
    c = log2(len(cts))
    P = tree(log_b, d, key, cts)
    return trace(log_b, d, key, P, c, log2(n)) if c < log2(n) else P


def key_dict(gs, atk_a, atk_b, d, n):
    ka, kb = np.asarray(atk_a, dtype=np.uint64).reshape(len(gs), d, n), np.asarray(atk_b, dtype=np.uint64).reshape(len(gs), d, n)
    return {int(g): (ka[q], kb[q]) for q, g in enumerate(gs)}


def u64(ct):
    return np.array(ct[0], dtype=np.uint64), np.array(ct[1], dtype=np.uint64)


def ks_error_bound(n, log_b, d, key_noise):
    """|phase(autks_g(ct)) - sigma_g(phase(ct))| per coefficient under a binary key (the digit-rounding and key-noise
    rows of 9.9's table with |S|_1 <= n in place of |S^2|):
      digit rounding   n 2^(63 - log_b d)          (0 when log_b d = 64)
      key noise        d n 2^(log_b - 1) key_noise"""
    digit = n * (1 << (63 - log_b * d)) if log_b * d < 64 else 0
    return digit + d * n * (1 << (log_b - 1)) * key_noise


def trace_error_bound(n, log_b, d, steps, e_in, key_noise):
    """err <- 2 err + ks per step: after `steps` steps err <= 2^steps e_in + (2^steps - 1) ks; a pack of any count is log2 n steps on
    every path from an input to the result (c merge levels, log2 n - c trace steps): n e_in + (n - 1) ks"""
    return (1 << steps) * e_in + ((1 << steps) - 1) * ks_error_bound(n, log_b, d, key_noise)
