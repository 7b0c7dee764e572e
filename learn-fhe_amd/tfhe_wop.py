"""Look-up without a padding bit (k = 1) on top of the C ABI: a TLWE ciphertext of an m-bit message x << (64 - m) is split into its bits,
each bit becomes a TGGSW selector, and a packed table is read under them -- fhe_tfhe_wop_selectors and fhe_tfhe_wop_pbs.

  encode             x -> x << (64 - m): the message format, input and output alike
  wop_nu, wop_table  nu = ceil(log2(cb_d + 1)) and the test polynomial of a step (fhe_tfhe_wop_table)
  wop_selectors      the m steps and the private functional key switch in one call; wop_selectors_steps: the public entries chained
  wop_pbs            selectors, TggswKey.fill into a reserved key, lut_eval_batch: one call; wop_pbs_steps: the three chained
  plain_steps        the plain-value model of the step chain on phases (no encryption): bits, corrections, remainders
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .ring import TggswKey, TorusContext, _buf, _is_torch, _like, tglwe_sample_extract, tlwe_key_switch, tlwe_lincomb
from .tfhe_cbs import lut_eval_batch, pfks

M64 = 1 << 64


def encode(x, m):
    """message x < 2^m as a torus word without a padding bit"""
    return (int(x) << (64 - m)) % M64


def wop_nu(cb_d):
    """ceil(log2(cb_d + 1)): cb_d level functions and the correction share one blind rotation"""
    return cb_d.bit_length()


def wop_table(cb_log_b, cb_d, n, log_delta):
    """P[c] = -h_{c mod 2^nu}: h_j = g_j / 2 for j < cb_d, h_{cb_d} = 2^(log_delta - 1) (log_delta < 0: none), 0 above -> [n] uint64"""
    out = np.empty(n, dtype=np.uint64)
    L.check(L.lib().fhe_tfhe_wop_table(cb_log_b, cb_d, n, log_delta, out.ctypes.data_as(L.u64p)), "fhe_tfhe_wop_table")
    return out


def wop_workspace(n, n_lwe, m, cb_d, batch):
    words = C.c_size_t()
    L.check(L.lib().fhe_tfhe_wop_workspace(n, n_lwe, m, cb_d, batch, C.byref(words)), "fhe_tfhe_wop_workspace")
    return words.value


def plain_steps(x_phase, m, n, cb_d):
    """The step chain on a plain phase (an integer mod 2^64), every blind rotation ideal: step l shifts the remainder by m - 1 - l, adds
    2^62, mod-switches to multiples of 2^nu of the 2n positions and reads the sign of the negacyclic rotation; the correction is
    bit << delta_l.  -> (bits [m], remainders [m] (rem_l as step l sees it))"""
    nu, two_n = wop_nu(cb_d), 2 * n
    sh = 64 - two_n.bit_length() + 1 + nu
    rem, bits, rems = x_phase % M64, [], []
    for l in range(m):                                              # noqa: E741
        rems.append(rem)
        s = ((rem << (m - 1 - l)) + (1 << 62)) % M64
        pos = ((((s + (1 << (sh - 1))) % M64) >> sh) << nu) % two_n
        bit = 1 if pos >= n else 0                                  # v X^(-pos): coefficient j is -v[..] once pos + j >= n
        bits.append(bit)
        rem = (rem - (bit << (64 - m + l))) % M64
    return bits, rems


def wop_front(src_a, src_b, cor, n, nu, shift):
    """fhe_tfhe_wop_front: src [batch][n_lwe] / [batch], cor = (cor_a, cor_b) or None -> (rem_a, rem_b, at, bt)"""
    pa, cnt, mem, st = _buf(src_a)
    pb, batch, _, _ = _buf(src_b)
    n_lwe = cnt // batch
    rem_a, rem_b, at, bt = _like(src_a, (batch, n_lwe)), _like(src_a, (batch,)), _like(src_a, (batch, n_lwe)), _like(src_a, (batch,))
    pca, pcb = (_buf(cor[0])[0], _buf(cor[1])[0]) if cor else (None, None)
    L.check(L.lib().fhe_tfhe_wop_front(pa, pb, pca, pcb, n_lwe, batch, n, nu, shift, _buf(rem_a)[0], _buf(rem_b)[0], _buf(at)[0], _buf(bt)[0], mem, st),
            "fhe_tfhe_wop_front")
    return rem_a, rem_b, at, bt


def _ks(ks):
    return (ks[0], ks[1], _buf(ks[2])[0], _buf(ks[3])[0]) if ks else (0, 0, None, None)


def wop_selectors(brk: TggswKey, ks, cb_log_b, cb_d, pf_log_b, pf_d, pfksk, m, lwe_a, lwe_b, want_rem=False):
    """fhe_tfhe_wop_selectors.  ks = (log_b, d, ksk_a, ksk_b): the TLWE key switch n -> n_lwe (None allowed at m = 1).
    -> (rows_a, rows_b) [batch][m][2 cb_d][n], and with want_rem (rem_a [batch][n_lwe], rem_b [batch])"""
    pk, _, mem, st = _buf(pfksk)
    pb, batch, _, _ = _buf(lwe_b)
    n, n_lwe = brk.n, brk.count
    rows_a, rows_b = _like(lwe_a, (batch, m, 2 * cb_d, n)), _like(lwe_a, (batch, m, 2 * cb_d, n))
    rem_a, rem_b = (_like(lwe_a, (batch, n_lwe)), _like(lwe_a, (batch,))) if want_rem else (None, None)
    kl, kd, pka, pkb = _ks(ks)
    L.check(L.lib().fhe_tfhe_wop_selectors(brk.t.handle, brk._h, kl, kd, pka, pkb, cb_log_b, cb_d, pf_log_b, pf_d, pk, m, _buf(lwe_a)[0], pb,
                                           _buf(rows_a)[0], _buf(rows_b)[0], _buf(rem_a)[0] if want_rem else None, _buf(rem_b)[0] if want_rem else None,
                                           batch, mem, st), "fhe_tfhe_wop_selectors")
    return (rows_a, rows_b, rem_a, rem_b) if want_rem else (rows_a, rows_b)


def _where(x, like):
    """the numpy array x where `like` lives"""
    if _is_torch(like):
        import torch
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(like.device).view(like.dtype)
    return np.ascontiguousarray(x)


def wop_selectors_steps(brk: TggswKey, ks, cb_log_b, cb_d, pf_log_b, pf_d, pfksk, m, lwe_a, lwe_b):
    """The same through the public entries one by one: tlwe_lincomb {1, -1}, tlwe_lincomb {2^(m-1-l)} + 2^62, mod_switch_many, blind_rotate
    of wop_table, sample_extract(j), tlwe_lincomb {1} + h_j, tlwe_key_switch, pfks with group = cb_d.
    -> (rows_a, rows_b, rem_a, rem_b, levels_a, levels_b, corrs): levels [batch m cb_d][n] / [batch m cb_d] the pfks inputs in [c][l][j]
    order, corrs the list of (corr_a, corr_b) under the TGLWE key per step that has one"""
    n, n_lwe, nu = brk.n, brk.count, wop_nu(cb_d)
    batch = _buf(lwe_b)[1]
    torch_like = _is_torch(lwe_a)
    if torch_like:
        import torch
        stack = torch.stack
    else:
        stack = np.stack
    rem = (lwe_a.reshape(batch, n_lwe), lwe_b.reshape(batch))
    corr, lev_a, lev_b, corrs = None, [], [], []
    for l in range(m):                                              # noqa: E741
        last = l == m - 1
        if corr is not None:
            rem = tlwe_lincomb([1, -1], [rem, corr])
        s = tlwe_lincomb([1 << (m - 1 - l)], [rem], 1 << 62)
        at, bt = TorusContext.mod_switch_many(s[0], n, nu), TorusContext.mod_switch_many(s[1], n, nu)
        table = _where(wop_table(cb_log_b, cb_d, n, -1 if last else 64 - m + l), lwe_a)
        ra, rb = brk.blind_rotate(at, bt, table)
        step_a, step_b = [], []
        for j in range(cb_d + (0 if last else 1)):
            e = tglwe_sample_extract(ra, rb, n, j)
            h = (1 << (63 - cb_log_b * cb_d + j * cb_log_b)) if j < cb_d else 1 << (64 - m + l - 1)
            e = tlwe_lincomb([1], [e], h)
            if j < cb_d:
                step_a.append(e[0])
                step_b.append(e[1])
            else:
                corrs.append(e)
                corr = tlwe_key_switch(ks[0], ks[1], ks[2], ks[3], e[0], e[1], n, n_lwe)
        lev_a.append(stack(step_a, 1))                               # [batch][cb_d][n]
        lev_b.append(stack(step_b, 1))
    la, lb = stack(lev_a, 1), stack(lev_b, 1)                        # [batch][m][cb_d][..]
    cont = (lambda x: x.contiguous()) if torch_like else np.ascontiguousarray
    la, lb = cont(la).reshape(batch * m * cb_d, n), cont(lb).reshape(batch * m * cb_d)
    oa, ob = pfks(pf_log_b, pf_d, pfksk, 2, la, lb, n, n, group=cb_d)
    return oa.reshape(batch, m, 2 * cb_d, n), ob.reshape(batch, m, 2 * cb_d, n), rem[0], rem[1], la, lb, corrs


def wop_pbs(brk: TggswKey, ks, cb_log_b, cb_d, pf_log_b, pf_d, pfksk, m, lwe_a, lwe_b, sel_key: TggswKey, first_index, polys, n_out, out_ks=None):
    """fhe_tfhe_wop_pbs: lwe -> selectors -> sel_key.fill at first_index -> lut_eval_batch of polys (tfhe_cbs.lut_pack, where lwe lives).
    out_ks = (log_b, d, ksk_a, ksk_b, n_lwe_out) adds the output key switch.  -> (a [batch][n_out][n_lwe_out or n], b [batch][n_out])"""
    pk, _, mem, st = _buf(pfksk)
    pb, batch, _, _ = _buf(lwe_b)
    width = out_ks[4] if out_ks else brk.n
    out_a, out_b = _like(lwe_a, (batch, n_out, width)), _like(lwe_a, (batch, n_out))
    kl, kd, pka, pkb = _ks(ks)
    ol, od, oka, okb = _ks(out_ks)
    L.check(L.lib().fhe_tfhe_wop_pbs(brk.t.handle, brk._h, kl, kd, pka, pkb, cb_log_b, cb_d, pf_log_b, pf_d, pk, m, _buf(lwe_a)[0], pb, sel_key._h,
                                     first_index, _buf(polys)[0], n_out, ol, od, oka, okb, out_ks[4] if out_ks else 0, _buf(out_a)[0], _buf(out_b)[0],
                                     batch, mem, st), "fhe_tfhe_wop_pbs")
    return out_a, out_b


def wop_pbs_steps(brk: TggswKey, ks, cb_log_b, cb_d, pf_log_b, pf_d, pfksk, m, lwe_a, lwe_b, sel_key: TggswKey, first_index, polys, n_out, out_ks=None):
    """The same as three calls: wop_selectors, TggswKey.fill, lut_eval_batch"""
    batch = _buf(lwe_b)[1]
    ra, rb = wop_selectors(brk, ks, cb_log_b, cb_d, pf_log_b, pf_d, pfksk, m, lwe_a, lwe_b)
    sel_key.fill(first_index, ra, rb)
    return lut_eval_batch(polys, sel_key, first_index, m, n_out, batch, out_ks)
