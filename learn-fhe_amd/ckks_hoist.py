"""Harness side of the hoisted CKKS rotations and the double-hoisted diagonal-matrix product (include/fhe_ring.h):
`extend_plain`, the exact lift of encoded plaintexts to qs ++ ps, and the two definitions composed from the library's PUBLIC entries
(extend_bases, ntt, automorphism_eval, pointwise_mul, rescale_k, rescale, rotate_, add_), against which the tests hold
CkksKey.rotate_many and CkksDiagMatrixHoisted.apply bit for bit.  Operands are numpy uint64 arrays or torch CUDA int64 tensors."""
import math

import numpy as np

from .ring import _is_torch


def extend_plain(qs, ps, diags):
    """[terms][L][n] residues over qs of encoded plaintexts -> [terms][L+K][n] over qs ++ ps: the centred integer every coefficient
    stands for (CRT over qs, in (-Q/2, Q/2]) reduced modulo every prime.  Python integers: set-up time only."""
    d = np.asarray(diags, dtype=np.uint64)
    terms, big_l, n = d.shape
    assert big_l == len(qs)
    big_q = math.prod(qs)
    hats = [(big_q // q) * pow(big_q // q, -1, q) for q in qs]
    mods = list(qs) + list(ps)
    out = np.zeros((terms, len(mods), n), dtype=np.uint64)
    for t in range(terms):
        rows = [[int(v) for v in d[t, l]] for l in range(big_l)]
        for c in range(n):
            v = sum(rows[l][c] * hats[l] for l in range(big_l)) % big_q
            if v > big_q // 2:
                v -= big_q
            for l, m in enumerate(mods):
                out[t, l, c] = v % m
    return out


def _cat(parts):
    if _is_torch(parts[0]):
        import torch
        return torch.cat(parts, dim=1).contiguous()
    return np.ascontiguousarray(np.concatenate(parts, axis=1))


def _clone(x):
    return x.clone() if _is_torch(x) else x.copy()


def _rows(like, rows, batch, n):
    """[batch][len(rows)][n] with limb l filled with the constant rows[l], of the kind of `like`"""
    a = np.ascontiguousarray(np.broadcast_to(np.array(rows, dtype=np.uint64)[None, :, None], (batch, len(rows), n)))
    return _as(like, a)


def _as(like, a):
    """a numpy uint64 array as the kind of `like`"""
    a = np.array(a, dtype=np.uint64, order="C")  # a copy: broadcast views are read-only
    if _is_torch(like):
        import torch
        return torch.from_numpy(a.view(np.int64)).to(like.device)
    return a


def _bcast(like, limbs, batch):
    """[limbs][n] (numpy) -> [batch][limbs][n] of the kind of `like`"""
    limbs = np.asarray(limbs, dtype=np.uint64)
    return _as(like, np.broadcast_to(limbs[None], (batch,) + limbs.shape))


def _host(x):
    return x.cpu().numpy().view(np.uint64) if _is_torch(x) else x


def lift(rns, n, ct_b, ct_a):
    """-> (a^, P b^) [batch][L+K][n], evaluation domain over qs ++ ps: a~ = (a || ext(a)), b~ = P b on the q-limbs, zero on the p-limbs"""
    batch = ct_a.shape[0]
    big_p = math.prod(rns.ps)
    a_hat = rns.ntt_(_cat([ct_a, rns.extend_bases(ct_a, n)]), n, extended=True)
    b_hat = rns.ntt_(_cat([ct_b, _rows(ct_b, [0] * rns.K, batch, n)]), n, extended=True)
    # P is the constant polynomial whose every evaluation is P mod q_l
    pb_hat = rns.pointwise_mul_(b_hat, _rows(ct_b, [big_p % q for q in rns.qs] + [0] * rns.K, batch, n), n, extended=True)
    return a_hat, pb_hat


def hoisted_u(rns, n, j, raw_key, a_hat, pb_hat):
    """u_j in the evaluation domain -> (b, a) [batch][L+K][n]; raw_key = (k.b, k.a) [L+K][n] coefficient domain (numpy), None for j = 0"""
    batch = a_hat.shape[0]
    if j == 0:
        big_p = math.prod(rns.ps)
        pa = rns.pointwise_mul_(_clone(a_hat), _rows(a_hat, [big_p % q for q in rns.qs] + [0] * rns.K, batch, n), n, extended=True)
        return _clone(pb_hat), pa
    t = pow(5, j, 2 * n)
    sa = rns.automorphism_eval(a_hat, t, n, extended=True)
    sb = rns.automorphism_eval(pb_hat, t, n, extended=True)
    kb = rns.ntt_(_bcast(a_hat, raw_key[0], batch), n, extended=True)
    ka = rns.ntt_(_bcast(a_hat, raw_key[1], batch), n, extended=True)
    ub = rns.add_(rns.pointwise_mul_(kb, sa, n, extended=True), sb, n, extended=True)
    ua = rns.pointwise_mul_(ka, sa, n, extended=True)
    return ub, ua


def rotate_many_composed(rns, n, amounts, raw_keys, ct_b, ct_a):
    """fhe_ckks_rotate_many from public entries: raw_keys[r] = (k.b, k.a) [L+K][n] coefficient domain for amounts[r] (None for 0)
    -> [(b, a), ...] [batch][L][n]"""
    a_hat, pb_hat = lift(rns, n, ct_b, ct_a)
    outs = []
    for j, raw in zip(amounts, raw_keys):
        if j == 0:  # the entry copies (u_0 has zero p-limbs: rescale_k's base conversion would sit on a rounding tie)
            outs.append((_clone(ct_b), _clone(ct_a)))
            continue
        ub, ua = hoisted_u(rns, n, j, raw, a_hat, pb_hat)
        outs.append((rns.rescale_k(rns.ntt_(ub, n, extended=True, inverse=True), n), rns.rescale_k(rns.ntt_(ua, n, extended=True, inverse=True), n)))
    return outs


def mul_mat_hoisted_composed(rns_hi, rns_lo, n, split, diags, raw_baby, giant_keys, ct_b, ct_a):
    """fhe_ckks_mul_mat_hoisted from public entries.  split {i: [j, ...]}; diags [terms][L+K][n] (numpy) in the order of sorted i,
    sorted j; raw_baby {j: (k.b, k.a) [L+K][n] numpy}; giant_keys {i: CkksKey on rns_lo} -> (b, a) [batch][L-1][n]"""
    batch = ct_a.shape[0]
    a_hat, pb_hat = lift(rns_hi, n, ct_b, ct_a)
    babies = sorted({j for js in split.values() for j in js})
    u = {j: hoisted_u(rns_hi, n, j, raw_baby.get(j), a_hat, pb_hat) for j in babies}
    total, t = None, 0
    for i in sorted(split):
        w = None
        for j in sorted(set(split[i])):
            d_hat = rns_hi.ntt_(_bcast(ct_a, _host(diags)[t], batch), n, extended=True)
            t += 1
            term = [rns_hi.pointwise_mul_(_clone(d_hat), u[j][h], n, extended=True) for h in (0, 1)]
            w = term if w is None else [rns_hi.add_(w[h], term[h], n, extended=True) for h in (0, 1)]
        v = [rns_hi.rescale(rns_hi.rescale_k(rns_hi.ntt_(w[h], n, extended=True, inverse=True), n), n) for h in (0, 1)]
        if i:
            giant_keys[i].rotate_(pow(5, i, 2 * n), v[0], v[1])
        total = v if total is None else [rns_lo.add_(total[h], v[h], n) for h in (0, 1)]
    return total[0], total[1]
