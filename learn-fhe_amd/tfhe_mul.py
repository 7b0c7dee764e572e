"""TGLWE ciphertext product (k = 1) on top of the C ABI: the tensor of two ciphertexts over the integers, an exact rounded division by
2^p, and the relinearisation of the S^2 part (include/fhe_ring.h has the definition; DESIGN.md 9.9 the noise terms).

  rlk_gen         fhe_tglwe_rlk_gen: encryptions of h_j S^2 -> (rlk_a, rlk_b) [d][n]
  RelinKey        those rows prepared once for fhe_tglwe_relin / fhe_tglwe_mul
  tensor          fhe_tglwe_tensor -> (c0, c1, c2), phase c0 - c1 S + c2 S^2
  relin           fhe_tglwe_relin  -> (out_a, out_b)
  mul             fhe_tglwe_mul: relin(tensor(...)) in one launch
  relin_composed  the same bits through fhe_tggsw_prepare + fhe_tggsw_external_product on (c2, 0) under [RLK rows; zero rows], plus (c1, c0)
  lwe_mul         TLWE x TLWE: pack each operand at coefficient 0, multiply, sample_extract(0)
  dot             inner product of two encrypted vectors: xs at r stride, ys reversed and negated, one product, sample_extract(0)
  lwe_mul_plain, dot_plain   what the two helpers compute on plain values
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .ring import TggswKey, TorusContext, _buf, _is_torch, _like, _rng, tglwe_sample_extract
from .tfhe_pack import PackKey, pack


def rlk_gen(t: TorusContext, log_b, d, sk, n, std_dev, seed, stream_id):
    """fhe_tglwe_rlk_gen: row j encrypts 2^(64 - log_b (d - j)) S^2 under sk [n] -> (rlk_a, rlk_b) [d][n]"""
    ps, _, mem, st = _buf(sk)
    ra, rb = _like(sk, (d, n)), _like(sk, (d, n))
    L.check(L.lib().fhe_tglwe_rlk_gen(t.handle, log_b, d, ps, n, std_dev, _rng(seed), stream_id, _buf(ra)[0], _buf(rb)[0], mem, st), "fhe_tglwe_rlk_gen")
    return ra, rb


class RelinKey:
    """fhe_tglwe_rlk_prepare: rlk_a, rlk_b [d][n] (numpy, or torch CUDA tensors read on their current stream) in the evaluation domain
    of the two 60-bit primes; the constructor returns when the prepared rows are complete"""

    def __init__(self, t: TorusContext, log_b, d, rlk_a, rlk_b, n):
        self.t, self.log_b, self.d, self.n = t, log_b, d, n
        pa, cnt, mem, st = _buf(rlk_a)
        assert cnt == d * n and _buf(rlk_b)[1] == cnt, "rlk_a, rlk_b [d][n]"
        self._h = C.c_void_p()
        L.check(L.lib().fhe_tglwe_rlk_prepare(t.handle, log_b, d, pa, _buf(rlk_b)[0], n, mem, st, C.byref(self._h)), "fhe_tglwe_rlk_prepare")

    def destroy(self):
        h, self._h = getattr(self, "_h", None), None
        if h and L is not None and getattr(L, "lib", None):  # (module globals are gone at interpreter shutdown)
            L.lib().fhe_tglwe_rlk_destroy(h)

    __del__ = destroy


def tensor(t: TorusContext, ct0_a, ct0_b, ct1_a, ct1_b, n, log_delta):
    """fhe_tglwe_tensor on [batch][n] halves -> (c0, c1, c2)"""
    p0a, cnt, mem, st = _buf(ct0_a)
    batch = cnt // n
    c0, c1, c2 = (_like(ct0_a, (batch, n)) for _ in range(3))
    L.check(L.lib().fhe_tglwe_tensor(t.handle, p0a, _buf(ct0_b)[0], _buf(ct1_a)[0], _buf(ct1_b)[0], n, log_delta, _buf(c0)[0], _buf(c1)[0],
                                     _buf(c2)[0], batch, mem, st), "fhe_tglwe_tensor")
    return c0, c1, c2


def relin(key: RelinKey, c0, c1, c2, out=None):
    """fhe_tglwe_relin -> (out_a, out_b); out = (out_a, out_b) to write there (it may be (c1, c0))"""
    p0, cnt, mem, st = _buf(c0)
    batch = cnt // key.n
    out_a, out_b = out if out is not None else (_like(c0, (batch, key.n)), _like(c0, (batch, key.n)))
    L.check(L.lib().fhe_tglwe_relin(key.t.handle, key._h, p0, _buf(c1)[0], _buf(c2)[0], _buf(out_a)[0], _buf(out_b)[0], batch, mem, st), "fhe_tglwe_relin")
    return out_a, out_b


def mul(key: RelinKey, ct0_a, ct0_b, ct1_a, ct1_b, log_delta, out=None):
    """fhe_tglwe_mul -> (out_a, out_b); out = (out_a, out_b) to write there (it may be either input)"""
    p0a, cnt, mem, st = _buf(ct0_a)
    batch = cnt // key.n
    out_a, out_b = out if out is not None else (_like(ct0_a, (batch, key.n)), _like(ct0_a, (batch, key.n)))
    L.check(L.lib().fhe_tglwe_mul(key.t.handle, key._h, p0a, _buf(ct0_b)[0], _buf(ct1_a)[0], _buf(ct1_b)[0], log_delta, _buf(out_a)[0],
                                  _buf(out_b)[0], batch, mem, st), "fhe_tglwe_mul")
    return out_a, out_b


def _zeros(like, shape):
    z = _like(like, shape)
    if _is_torch(z):
        z.zero_()
    else:
        z[...] = 0
    return z


def relin_composed(t: TorusContext, log_b, d, rlk_a, rlk_b, c0, c1, c2, n):
    """The relinearisation through the public TGGSW entries: a pseudo-TGGSW whose first d rows -- the rows the digits of `a` multiply
    (torus_kernels.hpp: team_torus_gadget) -- are the key and whose last d rows are zero, applied to (c2, 0); then + (c1, c0)."""
    rows_a, rows_b = _zeros(rlk_a, (1, 2 * d, n)), _zeros(rlk_a, (1, 2 * d, n))
    rows_a[0, :d] = rlk_a.reshape(d, n)
    rows_b[0, :d] = rlk_b.reshape(d, n)
    key = TggswKey(t, log_b, d, rows_a, rows_b, n)
    batch = _buf(c2)[1] // n
    xa = c2.clone() if _is_torch(c2) else c2.copy()
    xb = _zeros(c2, (batch, n))
    xa = xa.reshape(batch, n)
    key.external_product_(0, xa, xb)
    return xa + c1.reshape(batch, n), xb + c0.reshape(batch, n)


def lwe_mul(pack_key: PackKey, relin_key: RelinKey, x, y, p):
    """x = (a [batch][n_in], b [batch]), y likewise: TLWE encryptions of 2^p-scaled values under the packing key's input key ->
    (a [batch][n], b [batch]), the TLWE ciphertext of the product under the TGLWE key's coefficients.  pack (count = 1) each,
    fhe_tglwe_mul, sample_extract(0)."""
    n = relin_key.n
    xa, xb = pack(pack_key, x[0], x[1], 1, 1)
    ya, yb = pack(pack_key, y[0], y[1], 1, 1)
    ma, mb = mul(relin_key, xa, xb, ya, yb, p)
    return tglwe_sample_extract(ma, mb, n, 0)


def dot(pack_key: PackKey, relin_key: RelinKey, xs, ys, p, stride=1):
    """xs = (a [m][n_in], b [m]), ys likewise, m <= n / stride entries: the TLWE ciphertext (a [1][n], b [1]) of sum_r x_r y_r.
    xs go to coefficients r stride; ys are packed as [y_0, -y_{m'-1}, ..., -y_1] over m' = n / stride positions (all-zero ciphertexts
    where there is no entry), so that -y_r sits at n - r stride and X^(r stride) X^(n - r stride) = -1 brings x_r y_r to coefficient 0."""
    n, n_in = relin_key.n, pack_key.n_in
    full = n // stride
    a_x, b_x = xs
    a_y, b_y = ys
    m = _buf(b_x)[1]
    assert 1 <= m <= full and _buf(b_y)[1] == m
    ya, yb = _zeros(a_y, (full, n_in)), _zeros(b_y, (full,))
    ya[0], yb[0] = a_y.reshape(m, n_in)[0], b_y.reshape(m)[0]
    if m > 1:  # position full - r holds -y_r
        if _is_torch(ya):
            ya[full - m + 1:] = -a_y.reshape(m, n_in)[1:].flip(0)
            yb[full - m + 1:] = -b_y.reshape(m)[1:].flip(0)
        else:
            ya[full - m + 1:] = np.negative(a_y.reshape(m, n_in)[1:][::-1])
            yb[full - m + 1:] = np.negative(b_y.reshape(m)[1:][::-1])
    cont = (lambda v: v.contiguous()) if _is_torch(a_x) else np.ascontiguousarray
    px = pack(pack_key, cont(a_x.reshape(1, m, n_in)), cont(b_x.reshape(1, m)), m, stride)
    py = pack(pack_key, ya.reshape(1, full, n_in), yb.reshape(1, full), full, stride)
    ma, mb = mul(relin_key, px[0], px[1], py[0], py[1], p)
    return tglwe_sample_extract(ma, mb, n, 0)


def lwe_mul_plain(x, y):
    """what lwe_mul computes on plain integers (the messages, without the scale)"""
    return [int(a) * int(b) for a, b in zip(x, y)]


def dot_plain(xs, ys):
    """what dot computes on plain integers"""
    return sum(int(a) * int(b) for a, b in zip(xs, ys))
