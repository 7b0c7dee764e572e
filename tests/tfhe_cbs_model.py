"""Plain model of the circuit bootstrap (k = 1): the plaintext rows of the private functional key-switch key, the key switch as an
integer matrix product mod 2^64, the interleaved test polynomial and the whole circuit bootstrap as their composition.  numpy uint64
wrapping arithmetic and Python integers; decomposition, blind rotation, sample extract and encryption are oracle.pyref's
(`fast=True` takes the blind rotation from oracle.cref, the same oracle's C restatement, where pyref's schoolbook products would take
minutes: n = 1024)."""
import numpy as np

from oracle import pyref as P

M64 = 1 << 64


def gadget(log_b, d):
    """g_j = 2^(64 - log_b d + j log_b): Base2Decomposor::<T64>::new(log_b, d) (decompose.rs:66-81)"""
    return list(P.TorusDecomposor(log_b, d).bases)


def nu_of(cb_d):
    nu = 0
    while (1 << nu) < cb_d:
        nu += 1
    return nu


def cbs_table(cb_log_b, cb_d, n):
    """P[c] = T_{c mod 2^nu}[c - c mod 2^nu]; T_j = g_j on n/4 <= c < 3n/4 for j < cb_d, 0 elsewhere and for j >= cb_d"""
    g, funcs = gadget(cb_log_b, cb_d), 1 << nu_of(cb_d)
    tables = [[(g[j] if j < cb_d and n // 4 <= c < 3 * n // 4 else 0) for c in range(n)] for j in range(funcs)]
    return np.array([tables[c % funcs][c - c % funcs] for c in range(n)], dtype=np.uint64)


def out_row(r, u, n_funcs, group):
    return ((r // group) * n_funcs + u) * group + r % group


def digits(log_b, d, values):
    """[len(values)][d] signed digits as Python integers (two's complement undone)"""
    dec = P.TorusDecomposor(log_b, d)
    return [[P.t64_to_i64(x) for x in dec.decompose_scalar(int(v))] for v in values]


def pfksk_plain(log_b, d, sk_in, funcs):
    """plaintext rows [d (n_in + 1)][n_funcs][n]: w_i g_j F_u mod 2^64, w_i = -sk_in[i], w_{n_in} = 1"""
    g = gadget(log_b, d)
    w = [(-int(s)) % M64 for s in sk_in] + [1]
    f = np.asarray(funcs, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return np.stack([f * np.uint64((wi * gj) % M64) for gj in g for wi in w])


def pfks(log_b, d, pfksk, n_funcs, ct_a, ct_b, n_in, n, group=1):
    """out(r, u) = sum_j sum_i digit_j(c_i) pfksk[j (n_in + 1) + i][u] over Z/2^64; pfksk [d (n_in + 1)][n_funcs][2][n] -> (out_a, out_b)
    [batch n_funcs][n] in fhe_tlwe_pfks's row order"""
    key = np.asarray(pfksk, dtype=np.uint64).reshape(d * (n_in + 1), n_funcs * 2 * n)
    ct_a, ct_b = np.asarray(ct_a, dtype=np.uint64).reshape(-1, n_in), np.asarray(ct_b, dtype=np.uint64).reshape(-1)
    batch = ct_b.size
    out_a, out_b = np.zeros((batch * n_funcs, n), dtype=np.uint64), np.zeros((batch * n_funcs, n), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for r in range(batch):
            dg = digits(log_b, d, list(ct_a[r]) + [ct_b[r]])                     # [n_in + 1][d]
            flat = np.array([dg[i][j] % M64 for j in range(d) for i in range(n_in + 1)], dtype=np.uint64)   # digit-major
            acc = np.zeros(key.shape[1], dtype=np.uint64)
            for s in range(0, key.shape[0], 256):                                # in slabs: the product of a whole key is large
                acc += (flat[s:s + 256, None] * key[s:s + 256]).sum(axis=0, dtype=np.uint64)
            acc = acc.reshape(n_funcs, 2, n)
            for u in range(n_funcs):
                out_a[out_row(r, u, n_funcs, group)], out_b[out_row(r, u, n_funcs, group)] = acc[u, 0], acc[u, 1]
    return out_a, out_b


def circuit_bootstrap(brk_log_b, brk_d, brk_a, brk_b, cb_log_b, cb_d, pf_log_b, pf_d, pfksk, lwe_a, lwe_b, fast=False):
    """mod switch to multiples of 2^nu (bootstrapping.rs:99-104), blind rotation of cbs_table (84-96), sample_extract(j) for j < cb_d
    (tglwe.rs:115-127), pfks with group = cb_d -> rows_a, rows_b [batch][2 cb_d][n]"""
    brk_a, brk_b = np.asarray(brk_a, dtype=np.uint64), np.asarray(brk_b, dtype=np.uint64)
    n_lwe, n = brk_a.shape[0], brk_a.shape[-1]
    lwe_a, lwe_b = np.asarray(lwe_a, dtype=np.uint64).reshape(-1, n_lwe), np.asarray(lwe_b, dtype=np.uint64).reshape(-1)
    batch, nu = lwe_b.size, nu_of(cb_d)
    table = cbs_table(cb_log_b, cb_d, n)
    ea, eb = [], []
    for c in range(batch):
        at = [x << nu for x in P.tfhe_mod_switch([int(x) for x in lwe_a[c]], n >> nu)]
        bt = P.tfhe_mod_switch([int(lwe_b[c])], n >> nu)[0] << nu
        if fast:
            from oracle import cref
            ra, rb = cref.tfhe_blind_rotate(brk_log_b, brk_d, brk_a, brk_b, table, np.array([at], dtype=np.uint64), np.array([bt], dtype=np.uint64))
            acc = ([int(x) for x in np.asarray(ra).reshape(n)], [int(x) for x in np.asarray(rb).reshape(n)])
        else:
            brk = [([[int(x) for x in r] for r in brk_a[i]], [[int(x) for x in r] for r in brk_b[i]]) for i in range(n_lwe)]
            acc = P.tfhe_blind_rotate(P.TorusDecomposor(brk_log_b, brk_d), brk, [int(x) for x in table], at, bt)
        for j in range(cb_d):
            xa, xb = P.tglwe_sample_extract(acc[0], acc[1], j)
            ea.append(xa)
            eb.append(xb)
    oa, ob = pfks(pf_log_b, pf_d, pfksk, 2, np.array(ea, dtype=np.uint64), np.array(eb, dtype=np.uint64), n, n, group=cb_d)
    return oa.reshape(batch, 2 * cb_d, n), ob.reshape(batch, 2 * cb_d, n)


def tglwe_phase(s, a, b):
    """b - a s in Z_{2^64}[X]/(X^n + 1) for one ciphertext, s binary -> [n] uint64"""
    from oracle import cref
    return np.asarray(b, dtype=np.uint64) - cref.torus_mul_exact(np.asarray(a, dtype=np.uint64), np.asarray(s, dtype=np.uint64))


def lut_eval_plain(table, bits):
    return table[sum(int(b) << l for l, b in enumerate(bits))]


def _noise(rng, std_dev, shape):
    return np.rint(rng.normal(0.0, std_dev * 2.0 ** 64, size=shape)).astype(np.int64).view(np.uint64)


def _tglwe_encrypt(rng, s, pt, std_dev):
    """tglwe.rs:91-103 for pt [rows][n]: a uniform, b = a s + e + pt; products by oracle.cref -> (a, b)"""
    from oracle import cref
    rows, n = pt.shape
    a = rng.integers(0, 1 << 63, size=(rows, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(rows, n), dtype=np.uint64)
    b = np.stack([cref.torus_mul_exact(a[r], s) for r in range(rows)]) + _noise(rng, std_dev, (rows, n)) + pt
    return a, b


def lut_circuit_worst_error(n, n_lwe, log_b, d, cb_log_b, cb_d, pf_log_b, pf_d, sd_lwe, sd_glwe, log_p, byts, seed=1):
    """The decode-level circuit of tests/test_tfhe_cbs_gpu.py on the CPU, keys and noise drawn here (normal, rounded): the 8 bits of every
    byte are circuit-bootstrapped through the model (blind rotation by oracle.cref), each byte reads a permutation table of 256 entries
    encoded at log_p with one padding bit through a CMUX tree of oracle.cref's external products, and the phase of coefficient 0 is held
    against the table's entry.  -> (worst |phase error|, half-slot, every byte decoded correctly)"""
    from oracle import cref
    rng = np.random.Generator(np.random.PCG64(seed))
    m, log_delta = 8, 64 - (log_p + 1)
    z, s = rng.integers(0, 2, size=n_lwe, dtype=np.uint64), rng.integers(0, 2, size=n, dtype=np.uint64)
    g = np.array(gadget(log_b, d), dtype=np.uint64)
    bra, brb = np.zeros((n_lwe, 2 * d, n), dtype=np.uint64), np.zeros((n_lwe, 2 * d, n), dtype=np.uint64)
    for i in range(n_lwe):                                   # tggsw.rs:79-88 of Rt::constant(z_i)
        a, b = _tglwe_encrypt(rng, s, np.zeros((2 * d, n), dtype=np.uint64), sd_glwe)
        a[:d, 0] += z[i] * g
        b[d:, 0] += z[i] * g
        bra[i], brb[i] = a, b
    one = np.zeros(n, dtype=np.uint64)
    one[0] = 1
    plain = pfksk_plain(pf_log_b, pf_d, s, np.stack([np.uint64(0) - s, one])).reshape(-1, n)
    ka, kb = _tglwe_encrypt(rng, s, plain, sd_glwe)
    pfksk = np.stack([ka, kb], axis=1).reshape(pf_d * (n + 1), 2, 2, n)
    bits = np.array([(x >> l) & 1 for x in byts for l in range(m)], dtype=np.uint64)
    lwe_a = rng.integers(0, 1 << 63, size=(bits.size, n_lwe), dtype=np.uint64) * np.uint64(2)
    lwe_b = lwe_a @ z + _noise(rng, sd_lwe, bits.size) + (bits << np.uint64(62))
    rows_a, rows_b = circuit_bootstrap(log_b, d, bra, brb, cb_log_b, cb_d, pf_log_b, pf_d, pfksk, lwe_a, lwe_b, fast=True)
    table = np.random.Generator(np.random.PCG64(6601)).permutation(256)
    worst, ok = 0, True
    for i, x in enumerate(byts):
        cur = [(np.zeros(n, dtype=np.uint64), np.concatenate([[np.uint64(int(v) << log_delta)], np.zeros(n - 1, dtype=np.uint64)])) for v in table]
        for level in range(m):
            ra, rb = rows_a[i * m + level], rows_b[i * m + level]
            nxt = []
            for k in range(len(cur) // 2):               # tggsw.rs:114-121: ct0 + external_product(sel, ct1 - ct0)
                (a0, b0), (a1, b1) = cur[2 * k], cur[2 * k + 1]
                ea, eb = cref.tggsw_external_product(cb_log_b, cb_d, ra, rb, a1 - a0, b1 - b0)
                nxt.append((a0 + np.asarray(ea, dtype=np.uint64).reshape(n), b0 + np.asarray(eb, dtype=np.uint64).reshape(n)))
            cur = nxt
        phase = int(tglwe_phase(s, cur[0][0], cur[0][1])[0])
        want = int(table[x])
        ok = ok and ((phase + (1 << (log_delta - 1))) % M64) >> log_delta == want
        worst = max(worst, abs(P.t64_to_i64((phase - (want << log_delta)) % M64)))
    return worst, 1 << (log_delta - 1), ok
