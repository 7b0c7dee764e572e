"""The definitions of the hoisted CKKS rotations and the double-hoisted diagonal-matrix product (include/fhe_ring.h)
written from the oracle's existing functions: rns_extend_bases, rns_automorphism, rns_mul, rns_rescale_k (also over qs alone with
k = 1, which is `rescale`) and ckks_rotate.  `Ops(cref)` works on numpy arrays through the C oracle, `Ops(pyref)` on lists of Python
integers.  Everything is in the coefficient domain: sigma is the reference's automorphism, (*) its ring product."""
import math

import numpy as np


class Ops:
    def __init__(self, ref):
        self.R, self.c = ref, ref.__name__.rsplit(".", 1)[-1] == "cref"

    def ext(self, qs, ps, limbs):
        return self.R.rns_extend_bases(qs, ps, limbs) if self.c else self.R.rns_extend_bases(qs, limbs, ps)

    def rescale_k(self, qps, k, limbs):
        return self.R.rns_rescale_k(qps, k, limbs) if self.c else self.R.rns_rescale_k(qps, limbs, k)

    def auto(self, mods, limbs, t):
        return self.R.rns_automorphism(mods, limbs, t)

    def mul(self, mods, a, b):
        return self.R.rns_mul(mods, a, b)

    def add(self, mods, a, b):
        if self.c:
            qv = np.array(mods, dtype=np.uint64)[:, None]
            s = np.asarray(a, dtype=np.uint64) + np.asarray(b, dtype=np.uint64)  # moduli below 2^62: no wrap
            return np.where(s >= qv, s - qv, s)
        return [[(x + y) % q for x, y in zip(ra, rb)] for q, ra, rb in zip(mods, a, b)]

    def cat(self, a, b):
        return np.concatenate([np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)]) if self.c else [list(r) for r in a] + [list(r) for r in b]

    def const(self, vals, n):
        """the constant polynomials vals[l]"""
        rows = [[int(v)] + [0] * (n - 1) for v in vals]
        return np.array(rows, dtype=np.uint64) if self.c else rows

    def rotate(self, qs, ps, key, t, b, a):
        return self.R.ckks_rotate(qs, ps, key[0], key[1], t, b, a)


def lift(O, qs, ps, b, a):
    """-> (a~, b~) over qs ++ ps: a~ = (a || ext(a)), b~ = P b with zero p-limbs"""
    n, big_p = len(a[0]), math.prod(ps)
    a_t = O.cat(a, O.ext(qs, ps, a))
    b_t = O.cat(O.mul(qs, b, O.const([big_p % q for q in qs], n)), O.const([0] * len(ps), n))
    return a_t, b_t


def hoisted_u(O, qs, ps, j, key, a_t, b_t):
    """u_j over qs ++ ps, coefficient domain; key = (k.b, k.a) [L+K][n] or None for j = 0"""
    qps, n, big_p = list(qs) + list(ps), len(a_t[0]), math.prod(ps)
    if j == 0:
        return b_t, O.mul(qps, a_t, O.const([big_p % q for q in qs] + [0] * len(ps), n))
    t = pow(5, j, 2 * n)
    sa, sb = O.auto(qps, a_t, t), O.auto(qps, b_t, t)
    return O.add(qps, sb, O.mul(qps, key[0], sa)), O.mul(qps, key[1], sa)


def rotate_many(O, qs, ps, amounts, keys, b, a):
    """fhe_ckks_rotate_many for one ciphertext ([L][n] b, a) -> [(b, a), ...]"""
    qps = list(qs) + list(ps)
    a_t, b_t = lift(O, qs, ps, b, a)
    outs = []
    for j, key in zip(amounts, keys):
        if j == 0:  # the entry copies: u_0 = (P b, P a) has zero p-limbs, the one input on which rescale_k's base conversion sits on a tie
            outs.append((b, a))
            continue
        ub, ua = hoisted_u(O, qs, ps, j, key, a_t, b_t)
        outs.append((O.rescale_k(qps, len(ps), ub), O.rescale_k(qps, len(ps), ua)))
    return outs


def mul_mat_hoisted(O, qs, ps, split, diags, raw_baby, raw_giant, b, a):
    """fhe_ckks_mul_mat_hoisted for one ciphertext.  split {i: [j, ...]}; diags [terms][L+K][n] in the order of sorted i, sorted j;
    raw_baby {j: key over qs ++ ps}, raw_giant {i: key over qs[:-1] ++ ps} -> (b, a) [L-1][n]"""
    qps, ql, n = list(qs) + list(ps), list(qs[:-1]), len(a[0])
    a_t, b_t = lift(O, qs, ps, b, a)
    u = {j: hoisted_u(O, qs, ps, j, raw_baby.get(j), a_t, b_t) for j in sorted({j for js in split.values() for j in js})}
    total, t = None, 0
    for i in sorted(split):
        w = None
        for j in sorted(set(split[i])):
            term = [O.mul(qps, diags[t], u[j][h]) for h in (0, 1)]
            t += 1
            w = term if w is None else [O.add(qps, w[h], term[h]) for h in (0, 1)]
        v = [O.rescale_k(list(qs), 1, O.rescale_k(qps, len(ps), w[h])) for h in (0, 1)]
        if i:
            v = list(O.rotate(ql, ps, raw_giant[i], pow(5, i, 2 * n), v[0], v[1]))
        total = v if total is None else [O.add(ql, total[h], v[h]) for h in (0, 1)]
    return total[0], total[1]


def pi_table(log_n, t):
    """The permutation sigma_t is in the evaluation domain, from the order of the transform's output alone: index k holds the value at
    psi^(2 brev(k) + 1), and the output's value at psi^e is the input's at psi^(e t) -> [pi(k)]"""
    n = 1 << log_n
    brev = lambda v: int(format(v, "0%db" % log_n)[::-1], 2) if log_n else 0  # noqa: E731
    point = [2 * brev(k) + 1 for k in range(n)]
    index = {e: k for k, e in enumerate(point)}
    return [index[point[k] * t % (2 * n)] for k in range(n)]


# ---- the seeded inputs on which rotate_many is held against ckks_rotate: tests/test_ckks_hoist_cpu.py clears them with the reference
# alone (Python integers), tests/test_ckks_hoist_gpu.py then asserts device == fhe_ckks_rotate on them ----------------------------
CLEARED = dict(log_n=4, bits=50, L=3, K=2, batch=2, amounts=[1, 2, 5])


def rand_limbs(seed, mods, n, batch=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = [rng.integers(0, m, size=(n if batch is None else (batch, n)), dtype=np.uint64) for m in mods]
    return np.stack(rows, axis=0 if batch is None else 1)  # [limb][n] or [batch][limb][n]


def cleared_inputs(primes):
    """primes: the first L + K two-adic primes of CLEARED's bit length for 2n -> (qs, ps, {j: (k.b, k.a)}, ct_b, ct_a [batch][L][n])"""
    c = CLEARED
    n, qs, ps = 1 << c["log_n"], list(primes[:c["L"]]), list(primes[c["L"]:c["L"] + c["K"]])
    keys = {j: (rand_limbs(7100 + j, qs + ps, n), rand_limbs(7200 + j, qs + ps, n)) for j in c["amounts"]}
    return qs, ps, keys, rand_limbs(7301, qs, n, c["batch"]), rand_limbs(7302, qs, n, c["batch"])
