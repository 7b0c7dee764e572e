"""Plain model of the vertically packed table look-up (csrc/tfhe_lut.hpp, fhe_tfhe_lut_eval): the shape, the packing, and the values the
packed polynomials take under an IDEAL tree and rotation -- every CMUX replaced by the choice its selector bit encrypts, on plaintext
polynomials over Z / 2^64 [X] / (X^n + 1).  Python integers and numpy only; runs no library code.

The last section is the CIPHERTEXT-level model (lut_eval_ciphertexts): the same walk on TGLWE ciphertexts under arbitrary TGGSW rows, every
step the exact oracle's (oracle/cref.py) -- what fhe_tfhe_lut_eval must give bit for bit in every exact key form."""
import numpy as np

M64 = 1 << 64


def shape(m, n_out, n):
    """-> (r, h, per_acc, n_acc, n_polys)"""
    log_n = n.bit_length() - 1
    assert n == 1 << log_n and m >= 1 and n_out >= 1
    r = min(m, log_n)
    per_acc = max(1, n >> m)
    n_acc = -(-n_out // per_acc)
    return r, m - r, per_acc, n_acc, n_acc << (m - r)


def pack(table, m, n):
    """table [n_out][2^m] -> polys [n_acc][2^h][n] uint64: polynomial (g, t) holds table[g per_acc + u][t 2^r + i] at coefficient u 2^m + i"""
    table = np.asarray(table, dtype=np.uint64).reshape(-1, 1 << m)
    n_out = table.shape[0]
    r, h, per_acc, n_acc, _ = shape(m, n_out, n)
    polys = np.zeros((n_acc, 1 << h, n), dtype=np.uint64)
    for o in range(n_out):
        g, u = divmod(o, per_acc)
        for t in range(1 << h):
            polys[g, t, (u << m):(u << m) + (1 << r)] = table[o, (t << r):((t + 1) << r)]
    return polys


def rotate(poly, i):
    """poly X^i in Z / 2^64 [X] / (X^n + 1) (tglwe.rs:61-66 on one polynomial), any integer i"""
    n = len(poly)
    k = i % (2 * n)
    out = np.zeros(n, dtype=np.uint64)
    src = np.asarray(poly, dtype=np.uint64)
    pos = (np.arange(n) + k) % (2 * n)
    with np.errstate(over="ignore"):
        out[pos % n] = np.where(pos < n, src, np.uint64(0) - src)
    return out


def accumulators(polys, m, address):
    """the accumulators [n_acc][n] after the ideal tree over bits r .. m - 1 and the ideal rotation by bits 0 .. r - 1"""
    n_acc, leaves, n = polys.shape
    h = leaves.bit_length() - 1
    r = m - h
    out = []
    for g in range(n_acc):
        nodes = [polys[g, t] for t in range(leaves)]
        for v in range(h):
            bit = (address >> (r + v)) & 1
            nodes = [nodes[2 * p + bit] for p in range(len(nodes) // 2)]     # CMUX(bit; even, odd)
        acc = nodes[0]
        for l in range(r):                                                  # noqa: E741
            if (address >> l) & 1:
                acc = rotate(acc, -(1 << l))                                 # CMUX(bit; acc, acc X^(-2^l))
        out.append(acc)
    return np.stack(out)


def lookup(polys, m, n_out, address):
    """-> [n_out] values: coefficient u 2^m of accumulator g for output o = g per_acc + u"""
    n = polys.shape[2]
    per_acc = max(1, n >> m)
    acc = accumulators(polys, m, address)
    return [int(acc[o // per_acc, (o % per_acc) << m]) for o in range(n_out)]


# ---- ciphertext level: learn-fhe_amd/tfhe_cbs.py `lut_eval_batch_steps` step for step, the device entries replaced by the exact oracle ----

def cmux(cref, log_b, d, rows_a, rows_b, c0a, c0b, c1a, c1b):
    """tggsw.rs:114-121: ct0 + external_product(rows, ct1 - ct0); rows_* [2d][n], one ciphertext (uint64 arithmetic wraps)"""
    ea, eb = cref.tggsw_external_product(log_b, d, rows_a, rows_b, c1a - c0a, c1b - c0b)
    return c0a + ea, c0b + eb


def lut_extractions(cref, polys, log_b, d, rows_a, rows_b, first_index, m, n_out, batch, threads=1):
    """polys [n_acc][2^h][n] (pack), rows_a / rows_b [count][2d][n]: the selectors, ciphertext c reads first_index + c m + l.
    -> (a [batch][n_out][n], b [batch][n_out]): the TLWE extractions in front of the key switch.  Ciphertexts are independent: `threads`
    of them run at a time (the oracle's C calls release the interpreter lock)"""
    from concurrent.futures import ThreadPoolExecutor
    polys = np.asarray(polys, dtype=np.uint64)
    n = polys.shape[-1]
    r, h, per_acc, n_acc, n_polys = shape(m, n_out, n)
    assert polys.size == n_polys * n and first_index + batch * m <= len(rows_a)

    def one(c):
        base = first_index + c * m
        cur_a, cur_b = list(np.zeros((n_polys, n), dtype=np.uint64)), list(polys.reshape(n_polys, n))
        for v in range(h):                                                   # tree level v: node p <- CMUX(bit r + v; node 2p, node 2p + 1)
            ka, kb = rows_a[base + r + v], rows_b[base + r + v]
            nxt = [cmux(cref, log_b, d, ka, kb, cur_a[2 * p], cur_b[2 * p], cur_a[2 * p + 1], cur_b[2 * p + 1]) for p in range(len(cur_a) // 2)]
            cur_a, cur_b = [x[0] for x in nxt], [x[1] for x in nxt]
        assert len(cur_a) == n_acc
        for l in range(r):                                                   # noqa: E741  ladder step l: acc <- CMUX(bit l; acc, acc X^(-2^l))
            ka, kb = rows_a[base + l], rows_b[base + l]
            for g in range(n_acc):
                ra, rb = cref.torus_monomial_mul(cur_a[g], -(1 << l)), cref.torus_monomial_mul(cur_b[g], -(1 << l))
                cur_a[g], cur_b[g] = cmux(cref, log_b, d, ka, kb, cur_a[g], cur_b[g], ra, rb)
        ea, eb = np.zeros((n_out, n), dtype=np.uint64), np.zeros(n_out, dtype=np.uint64)
        for o in range(n_out):                                               # output o: coefficient u 2^m of accumulator g
            g, u = divmod(o, per_acc)
            ea[o], eb[o] = cref.tglwe_sample_extract(cur_a[g], cur_b[g], u << m)
        return ea, eb

    if threads > 1 and batch > 1:
        with ThreadPoolExecutor(max_workers=min(threads, batch)) as pool:
            res = list(pool.map(one, range(batch)))
    else:
        res = [one(c) for c in range(batch)]
    return np.stack([x[0] for x in res]), np.stack([x[1] for x in res])


def lut_key_switch(cref, ext_a, ext_b, ks):
    """ks = (log_b, d, ksk_a [n d][n_lwe_out], ksk_b [n d], n_lwe_out): tlwe.rs:144-153 on every extraction -> (a [batch][n_out][n_lwe_out], b)"""
    log_b, d, ksk_a, ksk_b, width = ks
    batch, n_out = ext_b.shape
    oa, ob = np.zeros((batch, n_out, width), dtype=np.uint64), np.zeros((batch, n_out), dtype=np.uint64)
    for c in range(batch):
        for o in range(n_out):
            oa[c, o], ob[c, o] = cref.tlwe_key_switch(log_b, d, ksk_a, ksk_b, ext_a[c, o], int(ext_b[c, o]))
    return oa, ob


def lut_eval_ciphertexts(cref, polys, log_b, d, rows_a, rows_b, first_index, m, n_out, batch, ks=None, threads=1):
    """fhe_tfhe_lut_eval on the CPU -> (a [batch][n_out][n_lwe_out or n], b [batch][n_out])"""
    ea, eb = lut_extractions(cref, polys, log_b, d, rows_a, rows_b, first_index, m, n_out, batch, threads)
    return lut_key_switch(cref, ea, eb, ks) if ks else (ea, eb)
