"""TGLWE automorphism key switch, trace and ring packing (k = 1) on top of the C ABI (include/fhe_ring.h has the definitions; DESIGN.md
9.10 the noise terms and the key sizes).

  galois_set          the g a full pack needs: 2^u + 1 for u = 1 .. log2 n
  atk_gen             fhe_tglwe_atk_gen: encryptions of -h_j sigma_g(S) for every g of a set -> (atk_a, atk_b) [n_g][d][n]
  AutoKey             those rows prepared once for the three entries below
  automorphism        fhe_tglwe_automorphism: autks_g, one launch
  trace               fhe_tglwe_trace: ct <- ct + autks_{2^u + 1}(ct) for u = hi .. lo + 1, one launch
  ring_pack           fhe_tlwe_ring_pack: count = 2^c TLWE ciphertexts -> one TGLWE ciphertext, n phase(x_r) at coefficient r n / count
  embed               the TGLWE ciphertext whose sample_extract(0) a TLWE ciphertext is
  trace_composed      the trace through fhe_tglwe_automorphism and an addition per step
  ring_pack_composed  the pack through embed, fhe_tglwe_rotate, fhe_tglwe_automorphism and additions mod 2^64
  matvec              an encrypted matrix times an encrypted vector: one dot-style product a row, traced, rotated to its row, summed
  matvec_plain        what matvec computes on plain values
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .ring import TorusContext, _buf, _is_torch, _like, _rng, tglwe_rotate
from .tfhe_mul import RelinKey, _zeros, mul
from .tfhe_pack import PackKey, pack


def _log2(n):
    return int(n).bit_length() - 1


def _u32(gs):
    arr = (C.c_uint32 * len(gs))(*[int(g) for g in gs])
    return arr


def galois_set(n):
    """2^u + 1 for u = 1 .. log2 n (the last is n + 1)"""
    return [(1 << u) + 1 for u in range(1, _log2(n) + 1)]


def atk_gen(t: TorusContext, log_b, d, sk, n, gs, std_dev, seed, stream_id):
    """fhe_tglwe_atk_gen: row (q, j) encrypts -2^(64 - log_b (d - j)) sigma_{gs[q]}(S) under sk [n] -> (atk_a, atk_b) [len(gs)][d][n]"""
    ps, _, mem, st = _buf(sk)
    ra, rb = _like(sk, (len(gs), d, n)), _like(sk, (len(gs), d, n))
    L.check(L.lib().fhe_tglwe_atk_gen(t.handle, log_b, d, ps, n, _u32(gs), len(gs), std_dev, _rng(seed), stream_id, _buf(ra)[0], _buf(rb)[0], mem, st),
            "fhe_tglwe_atk_gen")
    return ra, rb


class AutoKey:
    """fhe_tglwe_atk_prepare: atk_a, atk_b [len(gs)][d][n] (numpy, or torch CUDA tensors read on their current stream) in the evaluation
    domain of the two 60-bit primes; the constructor returns when the prepared rows are complete"""

    def __init__(self, t: TorusContext, log_b, d, atk_a, atk_b, n, gs):
        self.t, self.log_b, self.d, self.n, self.gs = t, log_b, d, n, [int(g) for g in gs]
        pa, cnt, mem, st = _buf(atk_a)
        assert cnt == len(gs) * d * n and _buf(atk_b)[1] == cnt, "atk_a, atk_b [n_g][d][n]"
        self._h = C.c_void_p()
        L.check(L.lib().fhe_tglwe_atk_prepare(t.handle, log_b, d, pa, _buf(atk_b)[0], n, _u32(gs), len(gs), mem, st, C.byref(self._h)),
                "fhe_tglwe_atk_prepare")

    def device_bytes(self):
        """bytes of the prepared rows on the device: two primes, a and b, len(gs) d rows of n words"""
        return 2 * 2 * len(self.gs) * self.d * self.n * 8

    def destroy(self):
        h, self._h = getattr(self, "_h", None), None
        if h and L is not None and getattr(L, "lib", None):  # (module globals are gone at interpreter shutdown)
            L.lib().fhe_tglwe_atk_destroy(h)

    __del__ = destroy


def _outs(ct_a, batch, n, out):
    return out if out is not None else (_like(ct_a, (batch, n)), _like(ct_a, (batch, n)))


def automorphism(key: AutoKey, g, ct_a, ct_b, out=None):
    """fhe_tglwe_automorphism on [batch][n] halves -> (out_a, out_b); out = (out_a, out_b) to write there (it may be the input)"""
    pa, cnt, mem, st = _buf(ct_a)
    batch = cnt // key.n
    out_a, out_b = _outs(ct_a, batch, key.n, out)
    L.check(L.lib().fhe_tglwe_automorphism(key.t.handle, key._h, int(g), pa, _buf(ct_b)[0], _buf(out_a)[0], _buf(out_b)[0], batch, mem, st),
            "fhe_tglwe_automorphism")
    return out_a, out_b


def trace(key: AutoKey, ct_a, ct_b, lo=0, hi=None, out=None):
    """fhe_tglwe_trace, steps u = hi .. lo + 1 (hi defaults to log2 n) -> (out_a, out_b); out may be the input"""
    pa, cnt, mem, st = _buf(ct_a)
    batch = cnt // key.n
    out_a, out_b = _outs(ct_a, batch, key.n, out)
    hi = _log2(key.n) if hi is None else hi
    L.check(L.lib().fhe_tglwe_trace(key.t.handle, key._h, lo, hi, pa, _buf(ct_b)[0], _buf(out_a)[0], _buf(out_b)[0], batch, mem, st), "fhe_tglwe_trace")
    return out_a, out_b


def ring_pack(key: AutoKey, ct_a, ct_b, count):
    """fhe_tlwe_ring_pack: ct_a [packs][count][n], ct_b [packs][count] -> (out_a, out_b) [packs][n]"""
    pa, cnt, mem, st = _buf(ct_a)
    packs = cnt // (count * key.n)
    assert packs * count * key.n == cnt and _buf(ct_b)[1] == packs * count
    out_a, out_b = _like(ct_a, (packs, key.n)), _like(ct_a, (packs, key.n))
    L.check(L.lib().fhe_tlwe_ring_pack(key.t.handle, key._h, pa, _buf(ct_b)[0], count, packs, _buf(out_a)[0], _buf(out_b)[0], mem, st), "fhe_tlwe_ring_pack")
    return out_a, out_b


def embed(ct_a, ct_b, n):
    """TLWE (a' [batch][n], b' [batch]) -> TGLWE (a, b) [batch][n] with sample_extract(0) = (a', b'): a[0] = a'[0], a[i] = -a'[n - i],
    b = b' at coefficient 0"""
    a = ct_a.reshape(-1, n)
    batch = a.shape[0]
    out_a, out_b = _like(ct_a, (batch, n)), _zeros(ct_a, (batch, n))
    out_a[:, 0] = a[:, 0]
    if _is_torch(a):
        out_a[:, 1:] = -a[:, 1:].flip(1)
    else:
        out_a[:, 1:] = np.negative(a[:, 1:][:, ::-1])
    out_b[:, 0] = ct_b.reshape(batch)
    return out_a, out_b


def trace_composed(key: AutoKey, ct_a, ct_b, lo=0, hi=None):
    """the trace step by step: fhe_tglwe_automorphism with g = 2^u + 1 and an addition mod 2^64"""
    hi = _log2(key.n) if hi is None else hi
    ca, cb = ct_a.reshape(-1, key.n), ct_b.reshape(-1, key.n)
    for u in range(hi, lo, -1):
        xa, xb = automorphism(key, (1 << u) + 1, ca, cb)
        ca, cb = ca + xa, cb + xb
    return ca, cb


def ring_pack_composed(key: AutoKey, ct_a, ct_b, count):
    """the pack through the public entries: embed every input, then level l = 2, 4, .., count: node o of a pack from nodes o and
    o + count / l of the level below, (E + X^(n/l) O) + autks_{l+1}(E - X^(n/l) O), then the trace over u = log2 n .. log2 count + 1"""
    n = key.n
    packs = _buf(ct_a)[1] // (count * n)
    cont = (lambda v: v.contiguous()) if _is_torch(ct_a) else np.ascontiguousarray
    ca, cb = embed(ct_a, ct_b, n)
    ca, cb = ca.reshape(packs, count, n), cb.reshape(packs, count, n)
    l = 2
    while l <= count:
        s = count // l
        ea, eb = cont(ca[:, :s]).reshape(-1, n), cont(cb[:, :s]).reshape(-1, n)
        oa, ob = tglwe_rotate(cont(ca[:, s:]).reshape(-1, n), cont(cb[:, s:]).reshape(-1, n), n, n // l)
        xa, xb = automorphism(key, l + 1, cont(ea - oa), cont(eb - ob))
        ca, cb = (ea + oa + xa).reshape(packs, s, n), (eb + ob + xb).reshape(packs, s, n)
        l *= 2
    ca, cb = cont(ca.reshape(packs, n)), cont(cb.reshape(packs, n))
    c = _log2(count)
    if c < _log2(n):
        ca, cb = trace_composed(key, ca, cb, c, _log2(n))
    return ca, cb


def matvec(pack_key: PackKey, relin_key: RelinKey, auto_key: AutoKey, rows, xs, p):
    """rows = (a [r][m][n_in], b [r][m]): the r rows of an encrypted matrix, TLWE encryptions of 2^p-scaled entries; xs = (a [m][n_in],
    b [m]) the vector, m <= n, r <= n.  -> one TGLWE ciphertext (a [1][n], b [1][n]) with n 2^p (M x)_i at coefficient i for i < r and
    zero phase elsewhere.  Per row the product of tfhe_mul.dot (xs at coefficient j, the row reversed and negated, so that the inner
    product lands at coefficient 0), all rows in one fhe_tglwe_mul; one fhe_tglwe_trace zeroes the cross terms and multiplies by n; row
    i is rotated to coefficient i and the rows are summed mod 2^64.  n 2^p (M x)_i must fit the torus."""
    n, n_in = relin_key.n, pack_key.n_in
    a_r, b_r = rows
    a_x, b_x = xs
    m = _buf(b_x)[1]
    r = _buf(b_r)[1] // m
    assert 1 <= m <= n and 1 <= r <= n
    cont = (lambda v: v.contiguous()) if _is_torch(a_x) else np.ascontiguousarray
    a_r, b_r = a_r.reshape(r, m, n_in), b_r.reshape(r, m)
    ya, yb = _zeros(a_r, (r, n, n_in)), _zeros(b_r, (r, n))
    ya[:, 0], yb[:, 0] = a_r[:, 0], b_r[:, 0]
    if m > 1:  # position n - j holds -M_ij
        if _is_torch(ya):
            ya[:, n - m + 1:], yb[:, n - m + 1:] = -a_r[:, 1:].flip(1), -b_r[:, 1:].flip(1)
        else:
            ya[:, n - m + 1:], yb[:, n - m + 1:] = np.negative(a_r[:, 1:][:, ::-1]), np.negative(b_r[:, 1:][:, ::-1])
    px = pack(pack_key, cont(a_x.reshape(1, m, n_in)), cont(b_x.reshape(1, m)), m, 1)
    py = pack(pack_key, ya, yb, n, 1)
    rep = (lambda v: v.expand(r, n).contiguous()) if _is_torch(a_x) else (lambda v: np.ascontiguousarray(np.broadcast_to(v, (r, n))))
    ma, mb = mul(relin_key, rep(px[0]), rep(px[1]), py[0], py[1], p)
    ta, tb = trace(auto_key, ma, mb)
    out_a, out_b = _zeros(ta, (1, n)), _zeros(tb, (1, n))
    for i in range(r):
        ra, rb = tglwe_rotate(cont(ta[i:i + 1]), cont(tb[i:i + 1]), n, i)
        out_a, out_b = out_a + ra, out_b + rb
    return out_a, out_b


def matvec_plain(rows, xs):
    """what matvec computes on plain integers: [sum_j M_ij x_j for every row i] (the ciphertext holds n 2^p times these)"""
    return [sum(int(a) * int(b) for a, b in zip(row, xs)) for row in rows]
