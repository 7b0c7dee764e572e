"""Plain model of the TGLWE ciphertext product (k = 1), written from the definition in include/fhe_ring.h in Python integers:

  tensor : C2 = rnd_p(s(A1) s(A2)),  C1 = rnd_p(s(A1) s(B2) + s(B1) s(A2)),  C0 = rnd_p(s(B1) s(B2))   mod 2^64
  relin  : out_a = C1 + sum_j digit_j(C2) RLK_j.a,  out_b = C0 + sum_j digit_j(C2) RLK_j.b             mod 2^64
  mul    : relin(tensor)

s(w) the signed reading of a 64-bit word, rnd_p(x) = floor((x + 2^(p - 1)) / 2^p), products in Z[X]/(X^n + 1) over the integers.
The negacyclic products go through Kronecker substitution: a polynomial becomes one big integer (one slot of SLOT bits per
coefficient), Python multiplies, and the slots come back out with their signs."""
import numpy as np

from tfhe_cbs_model import M64, digits

SLOT = 160  # bits per coefficient: |product coefficient| <= 2 n 2^126 < 2^139 at n = 2048, and a sum of 64 digit products stays below 2^159


def s64(w):
    w = int(w) % M64
    return w - M64 if w >> 63 else w


def signed(words):
    return [s64(w) for w in words]


def _pack(coeffs):
    return sum(c << (SLOT * i) for i, c in enumerate(coeffs))


def negacyclic(a, b):
    """a, b: lists of n Python integers (|a_i b_j| summed stays below 2^(SLOT - 1)) -> the n coefficients of a b mod X^n + 1"""
    n = len(a)
    assert len(b) == n
    slots = 2 * n
    half = 1 << (SLOT - 1)
    off = sum(half << (SLOT * i) for i in range(slots))  # every slot non-negative: the slots then read independently
    raw = (_pack(a) * _pack(b) + off).to_bytes(slots * SLOT // 8 + 1, "little")
    w = SLOT // 8
    full = [int.from_bytes(raw[i * w:(i + 1) * w], "little") - half for i in range(slots)]
    return [full[k] - full[k + n] for k in range(n)]


def schoolbook(a, b):
    n = len(a)
    out = [0] * n
    for i in range(n):
        for j in range(n):
            if i + j < n:
                out[i + j] += a[i] * b[j]
            else:
                out[i + j - n] -= a[i] * b[j]
    return out


def rnd(x, p):
    return (x + (1 << (p - 1))) >> p


def _u(vals):
    return np.array([v % M64 for v in vals], dtype=np.uint64)


def tensor1(a1, b1, a2, b2, p):
    """one pair, [n] words each -> (c0, c1, c2) uint64 [n]"""
    A1, B1, A2, B2 = signed(a1), signed(b1), signed(a2), signed(b2)
    t = negacyclic(A1, A2)
    r = [x + y for x, y in zip(negacyclic(A1, B2), negacyclic(B1, A2))]
    b = negacyclic(B1, B2)
    return _u(rnd(v, p) for v in b), _u(rnd(v, p) for v in r), _u(rnd(v, p) for v in t)


def _batched(f, n, *arrs):
    arrs = [np.asarray(a, dtype=np.uint64).reshape(-1, n) for a in arrs]
    outs = [f(*(a[g] for a in arrs)) for g in range(arrs[0].shape[0])]
    return tuple(np.stack([o[i] for o in outs]) for i in range(len(outs[0])))


def tensor(ct0_a, ct0_b, ct1_a, ct1_b, n, p):
    """[batch][n] halves -> (c0, c1, c2) [batch][n]"""
    return _batched(lambda a1, b1, a2, b2: tensor1(a1, b1, a2, b2, p), n, ct0_a, ct0_b, ct1_a, ct1_b)


def gadget_sum(log_b, d, poly, rows_a, rows_b):
    """sum_j digit_j(poly) rows[j] -> (a, b) lists of integers (not reduced); rows [d][n]"""
    n = len(poly)
    dg = digits(log_b, d, [int(v) for v in poly])  # [n][d]
    acc_a, acc_b = [0] * n, [0] * n
    for j in range(d):
        dj = [dg[i][j] for i in range(n)]
        pa, pb = negacyclic(dj, signed(rows_a[j])), negacyclic(dj, signed(rows_b[j]))
        acc_a = [x + y for x, y in zip(acc_a, pa)]
        acc_b = [x + y for x, y in zip(acc_b, pb)]
    return acc_a, acc_b


def relin1(log_b, d, rlk_a, rlk_b, c0, c1, c2):
    sa, sb = gadget_sum(log_b, d, c2, rlk_a, rlk_b)
    return _u(int(x) + y for x, y in zip(c1, sa)), _u(int(x) + y for x, y in zip(c0, sb))


def relin(log_b, d, rlk_a, rlk_b, c0, c1, c2, n):
    """rlk [d][n]; c0, c1, c2 [batch][n] -> (out_a, out_b) [batch][n]"""
    ra, rb = np.asarray(rlk_a, dtype=np.uint64).reshape(d, n), np.asarray(rlk_b, dtype=np.uint64).reshape(d, n)
    return _batched(lambda x0, x1, x2: relin1(log_b, d, ra, rb, x0, x1, x2), n, c0, c1, c2)


def mul(log_b, d, rlk_a, rlk_b, ct0_a, ct0_b, ct1_a, ct1_b, n, p):
    c0, c1, c2 = tensor(ct0_a, ct0_b, ct1_a, ct1_b, n, p)
    return relin(log_b, d, rlk_a, rlk_b, c0, c1, c2, n)


def external_product1(log_b, d, rows_a, rows_b, a, b):
    """tggsw.rs:100-112 for k = 1 on one ciphertext: rows [2d][n], the first d multiply the digits of a, the last d those of b"""
    xa, xb = gadget_sum(log_b, d, a, rows_a[:d], rows_b[:d])
    ya, yb = gadget_sum(log_b, d, b, rows_a[d:], rows_b[d:])
    return _u(x + y for x, y in zip(xa, ya)), _u(x + y for x, y in zip(xb, yb))


def key_square(sk):
    """S^2 over the integers (the key polynomial is binary: coefficients in [-n, n])"""
    return negacyclic([int(v) for v in sk], [int(v) for v in sk])


def rlk_plain(log_b, d, sk):
    """the plaintext rows of a relinearisation key: [d][n], row j = 2^(64 - log_b (d - j)) S^2 mod 2^64: the weight of digit j, least
    significant first (tfhe_cbs_model.gadget)"""
    s2 = key_square(sk)
    return np.stack([_u(v << (64 - log_b * (d - j)) for v in s2) for j in range(d)])


def phase(a, b, sk):
    """b - a S mod 2^64 -> list of integers in [0, 2^64)"""
    prod = negacyclic(signed(a), [int(v) for v in sk])
    return [(int(x) - y) % M64 for x, y in zip(b, prod)]


def phase3(c0, c1, c2, sk):
    """c0 - c1 S + c2 S^2 mod 2^64"""
    S = [int(v) for v in sk]
    p1, p2 = negacyclic(signed(c1), S), negacyclic(signed(c2), key_square(sk))
    return [(int(x) - y + z) % M64 for x, y, z in zip(c0, p1, p2)]


def encrypt(rng, sk, pt, noise=None):
    """tglwe.rs:91-103 with a uniform mask from rng: (a, b = a S + pt + noise) uint64 [n]; pt, noise lists of integers"""
    n = len(sk)
    a = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    prod = negacyclic(signed(a), [int(v) for v in sk])
    e = noise if noise is not None else [0] * n
    return a, _u(x + int(y) + z for x, y, z in zip(prod, pt, e))


def centred(v):
    return s64(v)


def mul_error_bound(n, log_b, d, p, m_max, e_max, key_noise=0):
    """|phase(mul) - 2^p m1 m2| per coefficient for operands with phases 2^p m_i + e_i, |m_i|_1 <= m_max (sum of |coefficients|),
    |e_i|_inf <= e_max, under a binary key:
      m1 e2 + m2 e1            <= 2 m_max e_max
      e1 e2 / 2^p              <= n e_max^2 / 2^p
      wraps u e 2^(64 - p)     u = (s(B) - s(A) S - phase) / 2^64, |u| <= (n + 1) / 2; the wrap multiples of the OTHER operand's phase
                               2^p m + e leave 2^64 u m (vanishes mod 2^64) and u e 2^(64 - p): n terms of each operand
      rounding of C0, C1, C2   1/2 + n / 2 + n^2 / 2        (|S|_1 <= n, |S^2|_1 <= n^2)
      digit rounding           n |S^2|_inf 2^(63 - log_b d) <= n n 2^(63 - log_b d)   (0 when log_b d = 64)
      key noise                d n 2^(log_b - 1) key_noise
    """
    wrap = 2 * n * ((n + 1) // 2) * e_max * (1 << (64 - p))
    digit = n * n * (1 << (63 - log_b * d)) if log_b * d < 64 else 0
    return 2 * m_max * e_max + (n * e_max * e_max >> p) + 1 + wrap + 1 + n + n * n + digit + d * n * (1 << (log_b - 1)) * key_noise
