"""Circuit bootstrap (k = 1) and CMUX-tree look-ups on top of the C ABI: a computed TLWE bit becomes the TGGSW selector of
fhe_tggsw_cmux (tggsw.rs:114-121), so that a table of 2^m plaintext entries is read with m circuit bootstraps and 2^m - 1 CMUXes.

  cbs_table          the interleaved test polynomial (fhe_tfhe_cbs_table)
  pfksk_funcs        the two plaintext functions of the circuit bootstrap's key switch: -S and 1
  pfksk_gen, pfks    the private functional key-switch key and the key switch TLWE -> TGLWE
  circuit_bootstrap  TLWE bits -> TGGSW rows in one call (fhe_tfhe_circuit_bootstrap), and circuit_bootstrap_steps: the public entries
                     chained by hand
  lut_eval           the CMUX tree over trivial TGLWE ciphertexts, one fhe_tggsw_cmux call per level; lut_eval_plain: its plain values
  lut_shape, lut_pack, lut_eval_batch
                     vertical packing: a table of n_out x 2^m words as packed polynomials, read by a whole batch in one call
                     (fhe_tfhe_lut_eval), every ciphertext under its own m selectors; lut_eval_batch_steps: the public entries chained
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .ring import TggswKey, TorusContext, _buf, _is_torch, _like, _rng, tglwe_sample_extract, tglwe_sample_extract_many

M64 = 1 << 64


def cbs_nu(cb_d):
    """ceil(log2 cb_d): the blind rotation serves 2^nu tables"""
    return max(0, (cb_d - 1).bit_length())


def cbs_table(cb_log_b, cb_d, n):
    """P[c] = T_{c mod 2^nu}[c - c mod 2^nu], T_j = g_j on n/4 <= c < 3n/4 for j < cb_d, else 0 -> [n] uint64"""
    out = np.empty(n, dtype=np.uint64)
    L.check(L.lib().fhe_tfhe_cbs_table(cb_log_b, cb_d, n, out.ctypes.data_as(L.u64p)), "fhe_tfhe_cbs_table")
    return out


def cbs_workspace(n, n_lwe, cb_d, batch):
    words = C.c_size_t()
    L.check(L.lib().fhe_tfhe_cbs_workspace(n, n_lwe, cb_d, batch, C.byref(words)), "fhe_tfhe_cbs_workspace")
    return words.value


def pfksk_funcs(s):
    """The functions of the circuit bootstrap's key for the TGLWE key s [n] (numpy or torch): F_0 = -S, F_1 = 1 -> [2][n], like s"""
    n = s.numel() if _is_torch(s) else s.size
    f = _like(s, (2, n))
    if _is_torch(s):
        f[0] = -s.reshape(n)
        f[1] = 0
        f[1, 0] = 1
    else:
        f[0] = np.uint64(0) - s.reshape(n)
        f[1] = 0
        f[1, 0] = 1
    return f


def pfksk_gen(t: TorusContext, log_b, d, sk_in, sk_out, funcs, std_dev, seed, stream_id):
    """fhe_tlwe_pfksk_gen -> pfksk [d (n_in + 1)][n_funcs][2][n]: row (j (n_in + 1) + i, u) encrypts w_i g_j F_u under sk_out"""
    pi, n_in, mem, st = _buf(sk_in)
    po, n, _, _ = _buf(sk_out)
    pf, cnt, _, _ = _buf(funcs)
    n_funcs = cnt // n
    key = _like(sk_in, (d * (n_in + 1), n_funcs, 2, n))
    L.check(L.lib().fhe_tlwe_pfksk_gen(t.handle, log_b, d, pi, n_in, po, n, pf, n_funcs, std_dev, _rng(seed), stream_id, _buf(key)[0], mem, st),
            "fhe_tlwe_pfksk_gen")
    return key


def pfks(log_b, d, pfksk, n_funcs, ct_a, ct_b, n_in, n, group=1):
    """fhe_tlwe_pfks: ct_a [batch][n_in], ct_b [batch] -> (out_a, out_b) [batch n_funcs][n]; the row of (r, u) is
    ((r // group) n_funcs + u) group + r % group"""
    pk, _, mem, st = _buf(pfksk)
    pb, batch, _, _ = _buf(ct_b)
    out_a, out_b = _like(ct_a, (batch * n_funcs, n)), _like(ct_a, (batch * n_funcs, n))
    L.check(L.lib().fhe_tlwe_pfks(log_b, d, pk, n_funcs, _buf(ct_a)[0], pb, n_in, n, group, _buf(out_a)[0], _buf(out_b)[0], batch, mem, st), "fhe_tlwe_pfks")
    return out_a, out_b


def circuit_bootstrap(key: TggswKey, cb_log_b, cb_d, pf_log_b, pf_d, pfksk, lwe_a, lwe_b):
    """fhe_tfhe_circuit_bootstrap: TLWE encryptions of bits (pt = bit << 62) -> (rows_a, rows_b) [batch][2 cb_d][n], the rows of one TGGSW
    ciphertext per bit; TggswKey(t, cb_log_b, cb_d, rows_a, rows_b, n) prepares them as CMUX selectors"""
    pk, _, mem, st = _buf(pfksk)
    pb, batch, _, _ = _buf(lwe_b)
    rows_a, rows_b = _like(lwe_a, (batch, 2 * cb_d, key.n)), _like(lwe_a, (batch, 2 * cb_d, key.n))
    L.check(L.lib().fhe_tfhe_circuit_bootstrap(key.t.handle, key._h, cb_log_b, cb_d, pf_log_b, pf_d, pk, _buf(lwe_a)[0], pb, _buf(rows_a)[0],
                                               _buf(rows_b)[0], batch, mem, st), "fhe_tfhe_circuit_bootstrap")
    return rows_a, rows_b


def circuit_bootstrap_steps(key: TggswKey, cb_log_b, cb_d, pf_log_b, pf_d, pfksk, lwe_a, lwe_b, table):
    """The same through the public entries one by one: mod_switch_many, blind_rotate of `table` (cbs_table, where lwe lives),
    sample_extract_many (the first cb_d of 2^nu), pfks with group = cb_d"""
    n, nu = key.n, cbs_nu(cb_d)
    batch = _buf(lwe_b)[1]
    at, bt = TorusContext.mod_switch_many(lwe_a, n, nu), TorusContext.mod_switch_many(lwe_b, n, nu)
    ra, rb = key.blind_rotate(at, bt, table)
    ea, eb = tglwe_sample_extract_many(ra, rb, n, nu)
    ea, eb = ea.reshape(batch, 1 << nu, n)[:, :cb_d], eb.reshape(batch, 1 << nu)[:, :cb_d]
    if _is_torch(ea):
        ea, eb = ea.contiguous().reshape(batch * cb_d, n), eb.contiguous().reshape(batch * cb_d)
    else:
        ea, eb = np.ascontiguousarray(ea).reshape(batch * cb_d, n), np.ascontiguousarray(eb).reshape(batch * cb_d)
    oa, ob = pfks(pf_log_b, pf_d, pfksk, 2, ea, eb, n, n, group=cb_d)
    return oa.reshape(batch, 2 * cb_d, n), ob.reshape(batch, 2 * cb_d, n)


def lut_eval(table_polys, selector_key: TggswKey, first_index, m):
    """A CMUX tree over the 2^m trivial TGLWE ciphertexts (0, table_polys[x]) (tggsw.rs:114-121): level l is ONE fhe_tggsw_cmux call with
    index = first_index + l over 2^(m - l - 1) pairs -- all nodes of a level share the selector of address bit l (bit 0 = least
    significant) -- then sample_extract(0) (tglwe.rs:115-127).  table_polys [2^m][n] encoded torus polynomials, where the key lives.
    -> TLWE (a [1][n], b [1]) under the extracted key whose phase is coefficient 0 of table_polys[address] plus noise"""
    n = selector_key.n
    cnt = _buf(table_polys)[1]
    assert cnt == n << m, "2^m polynomials of n coefficients"
    cur_b = table_polys.reshape(1 << m, n)
    cur_a = _like(table_polys, (1 << m, n))
    if _is_torch(cur_a):
        cur_a.zero_()
    else:
        cur_a[:] = 0
    cont = (lambda x: x.contiguous()) if _is_torch(cur_a) else np.ascontiguousarray
    for level in range(m):
        half = 1 << (m - level - 1)
        pa, pb = cur_a.reshape(half, 2, n), cur_b.reshape(half, 2, n)
        cur_a, cur_b = selector_key.cmux(first_index + level, cont(pa[:, 0]), cont(pb[:, 0]), cont(pa[:, 1]), cont(pb[:, 1]))
    return tglwe_sample_extract(cont(cur_a.reshape(1, n)), cont(cur_b.reshape(1, n)), n, 0)


def lut_eval_plain(table, bits):
    """the plain value of the tree: table[sum bits[l] << l]"""
    return table[sum(int(b) << l for l, b in enumerate(bits))]


def lut_shape(m, n_out, n):
    """fhe_tfhe_lut_shape -> (r, per_acc, n_acc, n_polys): r = min(m, log2 n) address bits rotate, m - r go to a tree; per_acc outputs
    share one of n_acc accumulators; n_polys = n_acc 2^(m - r) packed polynomials"""
    r, per_acc, n_acc, n_polys = C.c_int(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    L.check(L.lib().fhe_tfhe_lut_shape(m, n_out, n, C.byref(r), C.byref(per_acc), C.byref(n_acc), C.byref(n_polys)), "fhe_tfhe_lut_shape")
    return r.value, per_acc.value, n_acc.value, n_polys.value


def lut_pack(table, m, n):
    """fhe_tfhe_lut_pack (host): table [n_out][2^m] uint64 torus words -> polys [n_acc][2^(m - r)][n]: polynomial (g, t) holds
    table[g per_acc + u][t 2^r + i] at coefficient u 2^m + i"""
    table = np.ascontiguousarray(table, dtype=np.uint64)
    n_out = table.size >> m
    assert table.size == n_out << m, "n_out rows of 2^m words"
    r, _, n_acc, n_polys = lut_shape(m, n_out, n)
    polys = np.empty((n_acc, 1 << (m - r), n), dtype=np.uint64)
    L.check(L.lib().fhe_tfhe_lut_pack(table.ctypes.data_as(L.u64p), m, n_out, n, polys.ctypes.data_as(L.u64p)), "fhe_tfhe_lut_pack")
    return polys


def lut_workspace(n, m, n_out, n_lwe_out, batch):
    words = C.c_size_t()
    L.check(L.lib().fhe_tfhe_lut_workspace(n, m, n_out, n_lwe_out, batch, C.byref(words)), "fhe_tfhe_lut_workspace")
    return words.value


def lut_eval_batch(polys, selector_key: TggswKey, first_index, m, n_out, batch, ks=None):
    """fhe_tfhe_lut_eval: ciphertext c reads the packed table `polys` (lut_pack, where the key lives) under the selectors
    first_index + c m + l of selector_key.  ks = (log_b, d, ksk_a, ksk_b, n_lwe_out) adds the TLWE key switch.
    -> (a [batch][n_out][n_lwe_out or n], b [batch][n_out])"""
    pp, _, mem, st = _buf(polys)
    n = selector_key.n
    width = ks[4] if ks else n
    out_a, out_b = _like(polys, (batch, n_out, width)), _like(polys, (batch, n_out))
    log_b, d, pka, pkb = (ks[0], ks[1], _buf(ks[2])[0], _buf(ks[3])[0]) if ks else (0, 0, None, None)
    L.check(L.lib().fhe_tfhe_lut_eval(selector_key.t.handle, selector_key._h, first_index, m, pp, n_out, log_b, d, pka, pkb, ks[4] if ks else 0,
                                      _buf(out_a)[0], _buf(out_b)[0], batch, mem, st), "fhe_tfhe_lut_eval")
    return out_a, out_b


def lut_eval_batch_steps(polys, selector_key: TggswKey, first_index, m, n_out, batch, ks=None):
    """The same through the public entries, ciphertext by ciphertext: fhe_tggsw_cmux with index first_index + c m + l on that
    ciphertext's nodes (tree levels, then the rotation steps with fhe_tglwe_rotate by -2^l), fhe_tglwe_sample_extract at u 2^m,
    fhe_tlwe_key_switch"""
    from .ring import tglwe_rotate, tlwe_key_switch
    n = selector_key.n
    r, per_acc, n_acc, n_polys = lut_shape(m, n_out, n)
    h = m - r
    torch_like = _is_torch(polys)
    cont = (lambda x: x.contiguous()) if torch_like else np.ascontiguousarray
    if torch_like:
        import torch
        stack = torch.stack
    else:
        stack = np.stack
    zeros = _like(polys, (n_polys, n))
    if torch_like:
        zeros.zero_()
    else:
        zeros[:] = 0
    res_a, res_b = [], []
    for c in range(batch):
        base = first_index + c * m
        cur_a, cur_b = zeros, polys.reshape(n_polys, n)
        for v in range(h):
            pa, pb = cur_a.reshape(-1, 2, n), cur_b.reshape(-1, 2, n)
            cur_a, cur_b = selector_key.cmux(base + r + v, cont(pa[:, 0]), cont(pb[:, 0]), cont(pa[:, 1]), cont(pb[:, 1]))
        cur_a, cur_b = cont(cur_a.reshape(n_acc, n)), cont(cur_b.reshape(n_acc, n))
        for l in range(r):
            ra, rb = tglwe_rotate(cur_a, cur_b, n, -(1 << l))
            cur_a, cur_b = selector_key.cmux(base + l, cur_a, cur_b, ra, rb)
        per_u = [tglwe_sample_extract(cur_a, cur_b, n, u << m) for u in range(min(per_acc, n_out))]
        ea = stack([per_u[o % per_acc][0][o // per_acc] for o in range(n_out)])
        eb = stack([per_u[o % per_acc][1][o // per_acc] for o in range(n_out)])
        if ks:
            ea, eb = tlwe_key_switch(ks[0], ks[1], ks[2], ks[3], cont(ea), cont(eb), n, ks[4])
        res_a.append(ea)
        res_b.append(eb)
    return stack(res_a), stack(res_b)
