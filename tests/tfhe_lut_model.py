"""Plain model of the vertically packed table look-up (csrc/tfhe_lut.hpp, fhe_tfhe_lut_eval): the shape, the packing, and the values the
packed polynomials take under an IDEAL tree and rotation -- every CMUX replaced by the choice its selector bit encrypts, on plaintext
polynomials over Z / 2^64 [X] / (X^n + 1).  Python integers and numpy only; runs no library code."""
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
