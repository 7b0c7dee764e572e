"""Big-integer model of fhe_ckks_lincomb and fhe_ckks_mul_eval (include/fhe_ring.h), built from oracle.pyref: `ckks_mul`
(scheme/ckks/src/ckks.rs:250-272), `rns_rescale_k(.., 1)` (util/src/ring/rns.rs:99-111) and `ckks_primes`.  Ciphertext halves are lists of
limbs, each a list of n Python integers.  trunc(c * scale) is exact rational arithmetic (fractions.Fraction)."""
import math
from fractions import Fraction

from oracle import pyref as P


def trunc_scaled(c, scale):
    """trunc(c * scale) toward zero, exactly: c is the rational number the float64 holds"""
    v = Fraction(c) * scale
    return math.floor(v) if v >= 0 else -math.floor(-v)


def scaled_constant(c, scale, q):
    return trunc_scaled(c, scale) % q


def lincomb(qs, cts, real, mults, c0, scale):
    """cts: [(b, a)] with at least len(qs) limbs each (only that prefix is read) -> (b, a) on len(qs) limbs (integer mode: sum i_j ct_j +
    trunc(c0 scale) e0) or len(qs) - 1 limbs (real mode: rescale(sum trunc(c_j scale) ct_j + trunc(c0 scale) scale e0))"""
    ell = len(qs)
    n = len(cts[0][0][0])
    ks = [trunc_scaled(m, scale) if real else int(m) for m in mults]
    k0 = trunc_scaled(c0, scale) * (scale if real else 1)
    out = []
    for half in (0, 1):
        limbs = []
        for l, q in enumerate(qs):
            row = [sum(k * ct[half][l][i] for k, ct in zip(ks, cts)) % q for i in range(n)]
            if half == 0:
                row[0] = (row[0] + k0) % q
            limbs.append(row)
        assert all(len(ct[half]) >= ell for ct in cts)
        out.append(P.rns_rescale_k(list(qs), limbs, 1) if real else limbs)
    return out[0], out[1]


def mul_eval(qs, ps, rlk_b, rlk_a, x, y, alpha=1, c=None):
    """x, y: (b, a) COEFFICIENT-domain limbs of the operands (the model has no evaluation domain: the device's operands are their
    transforms) on at least len(qs) limbs; rlk over qs ++ ps -> alpha * mul(x, y) - c on len(qs) - 1 limbs"""
    ell = len(qs)
    ob, oa = P.ckks_mul(list(qs), list(ps), rlk_b, rlk_a, x[0][:ell], x[1][:ell], y[0][:ell], y[1][:ell])
    if alpha == 1 and c is None:
        return ob, oa
    cts = [(ob, oa)] + ([c] if c is not None else [])
    return lincomb(qs[:ell - 1], cts, False, [alpha, -1][:len(cts)], 0.0, 1)
