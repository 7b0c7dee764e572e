"""Packing key switch (k = 1) on top of the C ABI: `count` TLWE ciphertexts become ONE TGLWE ciphertext whose phase carries input r at
coefficient r stride (tlwe.rs:144-153's digit x key product against TGLWE rows, tglwe.rs:91-103, each result times X^(r stride) as
tglwe.rs:61-66 rotates, summed).

  pack_funcs     the one plaintext function of a packing key: the identity, [1, 0, ..., 0]
  PackKey        a key of tfhe_cbs.pfksk_gen (n_funcs = 1, funcs = pack_funcs(n)) prepared once for fhe_tlwe_pack
  pack           fhe_tlwe_pack: ct_a [packs][count][n_in], ct_b [packs][count] -> (out_a, out_b) [packs][n]
  pack_composed  the same bits through the public entries: fhe_tlwe_pfks, fhe_tglwe_rotate per position, additions mod 2^64
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .ring import TorusContext, _buf, _is_torch, _like, tglwe_rotate
from .tfhe_cbs import pfks


def pack_funcs(n, like=None):
    """funcs [1][n] of fhe_tlwe_pfksk_gen for a packing key: F_0 = 1 -> numpy uint64, or a tensor where `like` lives"""
    f = np.zeros((1, n), dtype=np.uint64)
    f[0, 0] = 1
    if like is not None and _is_torch(like):
        import torch
        return torch.from_numpy(f.view(np.int64)).to(like.device)
    return f


class PackKey:
    """fhe_tlwe_pack_key_prepare: pfksk [d (n_in + 1)][1][2][n] (numpy, or a torch CUDA tensor read on its current stream) in the
    evaluation domain of the two 60-bit primes; the constructor returns when the prepared rows are complete"""

    def __init__(self, t: TorusContext, log_b, d, pfksk, n_in, n):
        self.t, self.log_b, self.d, self.n_in, self.n = t, log_b, d, n_in, n
        pk, cnt, mem, st = _buf(pfksk)
        assert cnt == d * (n_in + 1) * 2 * n, "a one-function key: [d (n_in + 1)][1][2][n]"
        self._h = C.c_void_p()
        L.check(L.lib().fhe_tlwe_pack_key_prepare(t.handle, log_b, d, pk, n_in, n, mem, st, C.byref(self._h)), "fhe_tlwe_pack_key_prepare")

    def destroy(self):
        h, self._h = getattr(self, "_h", None), None
        if h and L is not None and getattr(L, "lib", None):  # (module globals are gone at interpreter shutdown)
            L.lib().fhe_tlwe_pack_key_destroy(h)

    __del__ = destroy


def pack(key: PackKey, ct_a, ct_b, count, stride):
    """fhe_tlwe_pack: input (g, r) lands at coefficient r stride of TGLWE ciphertext g -> (out_a, out_b) [packs][n]"""
    pa, _, mem, st = _buf(ct_a)
    pb, total, _, _ = _buf(ct_b)
    assert count >= 1 and total % count == 0, "ct_b [packs][count]"
    packs = total // count
    out_a, out_b = _like(ct_a, (packs, key.n)), _like(ct_a, (packs, key.n))
    L.check(L.lib().fhe_tlwe_pack(key.t.handle, key._h, pa, pb, count, stride, packs, _buf(out_a)[0], _buf(out_b)[0], mem, st), "fhe_tlwe_pack")
    return out_a, out_b


def pack_composed(log_b, d, pfksk, ct_a, ct_b, n_in, n, count, stride):
    """The route through the public entries: fhe_tlwe_pfks (n_funcs = 1, group = 1) on all packs count inputs, fhe_tglwe_rotate by
    r stride of the r-th result of every pack, and the sum mod 2^64 -> (out_a, out_b) [packs][n]"""
    total = _buf(ct_b)[1]
    packs = total // count
    ka, kb = pfks(log_b, d, pfksk, 1, ct_a, ct_b, n_in, n)
    ka, kb = ka.reshape(packs, count, n), kb.reshape(packs, count, n)
    cont = (lambda x: x.contiguous()) if _is_torch(ka) else np.ascontiguousarray
    out_a, out_b = _like(ct_a, (packs, n)), _like(ct_a, (packs, n))
    if _is_torch(out_a):
        out_a.zero_()
        out_b.zero_()
    else:
        out_a[:], out_b[:] = 0, 0
    for r in range(count):
        ra, rb = tglwe_rotate(cont(ka[:, r]), cont(kb[:, r]), n, r * stride)
        out_a += ra.reshape(packs, n)
        out_b += rb.reshape(packs, n)
    return out_a, out_b
