"""The exact model of the CKKS bootstrap glue for tests/test_ckks_bootstrap_*.py in Python integers: `mod_raise`, the monomial X^(n/2),
the conjugate split and the join (include/fhe_ring.h fhe_ckks_mod_raise, fhe_ckks_conj_split, fhe_ckks_conj_join).  Polynomials are
lists of n residues of ONE modulus q; a limb-major polynomial is a list of those."""


def centred(v, q):
    """the representative of v mod q in (-q/2, q/2]"""
    v %= q
    return v - q if v > q // 2 else v


def mod_raise(limb0, q0, qs):
    """residues mod q0 -> the centred integers reduced into every modulus of qs (Python's % maps a negative v to q - (|v| mod q), 0 to 0)"""
    lifted = [centred(v, q0) for v in limb0]
    return [[v % q for v in lifted] for q in qs]


def shift_half(p, q):
    """X^(n/2) p in Z_q[X] / (X^n + 1): coefficient j is p[j - n/2] from n/2 on and -p[j + n/2] below"""
    n, h = len(p), len(p) // 2
    return [p[j - h] % q if j >= h else (-p[j + h]) % q for j in range(n)]


def monomial_schoolbook(p, k, q):
    """X^k p by the schoolbook negacyclic product with the polynomial that has a single 1 at position k"""
    n = len(p)
    mono = [1 if i == k else 0 for i in range(n)]
    out = [0] * n
    for i in range(n):
        for j in range(n):
            s = i + j
            out[s % n] += (-1 if s >= n else 1) * mono[i] * p[j]
    return [v % q for v in out]


def split(x, cx, q):
    """(R, J) = (x + cx, -X^(n/2) (x - cx))"""
    r = [(a + b) % q for a, b in zip(x, cx)]
    d = [(a - b) % q for a, b in zip(x, cx)]
    return r, [(-v) % q for v in shift_half(d, q)]


def join(r, j, q):
    """R + X^(n/2) J"""
    return [(a + b) % q for a, b in zip(r, shift_half(j, q))]


def negacyclic_int(a, s):
    """a s in Z[X] / (X^n + 1) over the integers"""
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(s):
                if y:
                    k = i + j
                    out[k % n] += -x * y if k >= n else x * y
    return out
