"""Plain model of the packing key switch (k = 1), written from the definition of fhe_tlwe_pack:

  out[g] = sum_{j, i} D_{g,j,i}(X) * pfksk[j (n_in + 1) + i]  in Z_{2^64}[X]/(X^n + 1),   D_{g,j,i}(X) = sum_r digit_j(c_{g,r,i}) X^(r stride)

with c_{g,r,i} = ct_a[g][r][i] for i < n_in and c_{g,r,n_in} = ct_b[g][r]: one digit polynomial per key row and a schoolbook negacyclic
product mod 2^64 per row and half (numpy uint64 wrapping arithmetic; the terms of a zero coefficient are skipped).  It calls neither the
key switch of tfhe_cbs_model nor a rotation: tests/test_tfhe_pack_cpu.py holds it against those."""
import numpy as np

from tfhe_cbs_model import M64, digits


def digit_polys(log_b, d, ct_a, ct_b, n_in, n, count, stride):
    """one pack: ct_a [count][n_in], ct_b [count] -> [d (n_in + 1)][n] uint64, row j (n_in + 1) + i holds digit_j(c_{r,i}) at r stride"""
    assert count >= 1 and stride >= 1 and (count - 1) * stride < n
    ct_a, ct_b = np.asarray(ct_a, dtype=np.uint64).reshape(count, n_in), np.asarray(ct_b, dtype=np.uint64).reshape(count)
    out = np.zeros((d * (n_in + 1), n), dtype=np.uint64)
    for r in range(count):
        dg = digits(log_b, d, list(ct_a[r]) + [ct_b[r]])  # [n_in + 1][d]
        for i in range(n_in + 1):
            for j in range(d):
                out[j * (n_in + 1) + i, r * stride] = np.uint64(dg[i][j] % M64)
    return out


def negacyclic_mul(sparse, dense):
    """sum_p sparse[p] X^p * dense(X) mod (X^n + 1, 2^64), term by term over the nonzero p: X^p dense has dense[k - p] at k >= p and
    -dense[n + k - p] below"""
    n = dense.size
    ext = np.concatenate([dense, np.uint64(0) - dense])  # ext[(k - p) mod 2n]: the sign of a wrap rides along
    nz = np.nonzero(sparse)[0]
    acc = np.zeros(n, dtype=np.uint64)
    k = np.arange(n)
    for s in range(0, nz.size, 64):                       # in slabs: [64][n] words at a time
        p = nz[s:s + 64]
        acc += (sparse[p, None] * ext[(k[None, :] - p[:, None]) % (2 * n)]).sum(axis=0, dtype=np.uint64)
    return acc


def pack(log_b, d, pfksk, ct_a, ct_b, n_in, n, count, stride):
    """pfksk [d (n_in + 1)][1][2][n]; ct_a [packs][count][n_in], ct_b [packs][count] -> (out_a, out_b) [packs][n]"""
    key = np.asarray(pfksk, dtype=np.uint64).reshape(d * (n_in + 1), 2, n)
    ct_a, ct_b = np.asarray(ct_a, dtype=np.uint64).reshape(-1, count, n_in), np.asarray(ct_b, dtype=np.uint64).reshape(-1, count)
    packs = ct_b.shape[0]
    out_a, out_b = np.zeros((packs, n), dtype=np.uint64), np.zeros((packs, n), dtype=np.uint64)
    for g in range(packs):
        dp = digit_polys(log_b, d, ct_a[g], ct_b[g], n_in, n, count, stride)
        for row in range(key.shape[0]):
            out_a[g] += negacyclic_mul(dp[row], key[row, 0])
            out_b[g] += negacyclic_mul(dp[row], key[row, 1])
    return out_a, out_b
