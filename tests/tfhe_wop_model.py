"""Plain model of the look-up without a padding bit (k = 1): nu, the half gadget values, the step tables, the step front, the step chain
on plaintext phases, and the chain under keys drawn on the host.  numpy uint64 wrapping arithmetic and Python integers; mod switch, blind
rotation, sample extract, key switch and external product are oracle.pyref's / oracle.cref's, the private functional key switch and the
packing are tfhe_cbs_model's and tfhe_lut_model's."""
import numpy as np

from oracle import pyref as P

import tfhe_cbs_model as CM
import tfhe_lut_model as LM

M64 = 1 << 64

# decode-level parameters of tests/test_tfhe_lut_gpu.py (`LUT`) with the TLWE key switch of DESIGN.md 9.5: gadget (4, 8)
WOP = dict(n=1024, n_lwe=8, log_b=10, d=4, cb_log_b=4, cb_d=6, pf_log_b=7, pf_d=6, sd_lwe=2.0 ** -30, sd_glwe=2.845267479601915e-15,
           ks_log_b=4, ks_d=8, m=8)
BYTES = [0x00, 0xFF, 0xA5, 0x3C, 0x81]


def nu_of(cb_d):
    nu = 0
    while (1 << nu) < cb_d + 1:
        nu += 1
    return nu


def h_values(cb_log_b, cb_d, log_delta):
    """h_j for j < 2^nu: g_j / 2 below cb_d, 2^(log_delta - 1) at cb_d (log_delta < 0: the last step, 0), 0 above"""
    g = CM.gadget(cb_log_b, cb_d)
    assert all(x % 2 == 0 for x in g), "cb_log_b cb_d <= 63"
    h = [x // 2 for x in g] + [(1 << (log_delta - 1)) if log_delta >= 1 else 0]
    return h + [0] * ((1 << nu_of(cb_d)) - len(h))


def wop_table(cb_log_b, cb_d, n, log_delta):
    """P[c] = -h_{c mod 2^nu} as torus words"""
    h = h_values(cb_log_b, cb_d, log_delta)
    return np.array([(-h[c % len(h)]) % M64 for c in range(n)], dtype=np.uint64)


def front(src_a, src_b, cor_a, cor_b, shift, n, nu):
    """One step front on TLWE words: rem = src - cor (cor None: rem = src), s = rem << shift with 2^62 added to b, then the mod switch of
    bootstrapping.rs:99-104 for n >> nu shifted left by nu.  Python integers per word -> (rem_a, rem_b, at, bt) uint64 arrays"""
    def words(src, cor, add):
        rem = [(int(x) - (int(c) if cor is not None else 0)) % M64 for x, c in zip(src.ravel(), cor.ravel() if cor is not None else src.ravel())]
        s = [((r << shift) + add) % M64 for r in rem]
        sw = [(x << nu) % M64 for x in P.tfhe_mod_switch(s, n >> nu)]
        return np.array(rem, dtype=np.uint64).reshape(src.shape), np.array(sw, dtype=np.uint64).reshape(src.shape)
    rem_a, at = words(np.asarray(src_a, dtype=np.uint64), None if cor_a is None else np.asarray(cor_a, dtype=np.uint64), 0)
    rem_b, bt = words(np.asarray(src_b, dtype=np.uint64), None if cor_b is None else np.asarray(cor_b, dtype=np.uint64), 1 << 62)
    return rem_a, rem_b, at, bt


def plain_steps(phase, m, n, cb_log_b, cb_d):
    """The step chain on a plaintext phase (integer mod 2^64) with an ideal blind rotation: position p of the 2n after the mod switch,
    coefficient j of P X^(-p) is P[j + p] below n and -P[j + p - n] above (bootstrapping.rs:84-96), h_j added.
    -> per step (bit, [level phases j < cb_d], correction phase or None, remainder the step saw)"""
    nu, out, rem = nu_of(cb_d), [], phase % M64
    for l in range(m):                                              # noqa: E741
        log_delta = 64 - m + l if l < m - 1 else -1
        table = [int(x) for x in wop_table(cb_log_b, cb_d, n, log_delta)]
        h = h_values(cb_log_b, cb_d, log_delta)
        s = ((rem << (m - 1 - l)) + (1 << 62)) % M64
        p = (P.tfhe_mod_switch([s], n >> nu)[0] << nu) % (2 * n)
        coef = [(table[j + p] if j + p < n else -table[j + p - n]) % M64 for j in range(cb_d + 1)]
        rows = [(coef[j] + h[j]) % M64 for j in range(cb_d + 1)]
        bit = 1 if p >= n else 0
        corr = rows[cb_d] if l < m - 1 else None
        out.append((bit, rows[:cb_d], corr, rem))
        if corr is not None:
            rem = (rem - corr) % M64
    return out


def noise(rng, std_dev, shape):
    return np.rint(rng.normal(0.0, std_dev * 2.0 ** 64, size=shape)).astype(np.int64).view(np.uint64)


def r64(rng, *shape):
    return rng.integers(0, 1 << 63, size=shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)


def keys(rng, n, n_lwe, log_b, d, ks_log_b, ks_d, pf_log_b, pf_d, sd_lwe, sd_glwe):
    """Keys drawn on the host (normal noise, rounded): z [n_lwe], s [n] binary; the bootstrapping key (tggsw.rs:79-88 of z_i under s), the
    TLWE key-switch key s -> z (tlwe.rs:98-109: row j n + i encrypts -s_i g_j under z) and the two-function private functional key"""
    z, s = rng.integers(0, 2, size=n_lwe, dtype=np.uint64), rng.integers(0, 2, size=n, dtype=np.uint64)
    g = np.array(CM.gadget(log_b, d), dtype=np.uint64)
    bra, brb = np.zeros((n_lwe, 2 * d, n), dtype=np.uint64), np.zeros((n_lwe, 2 * d, n), dtype=np.uint64)
    for i in range(n_lwe):
        a, b = CM._tglwe_encrypt(rng, s, np.zeros((2 * d, n), dtype=np.uint64), sd_glwe)
        a[:d, 0] += z[i] * g
        b[d:, 0] += z[i] * g
        bra[i], brb[i] = a, b
    kg = np.array(CM.gadget(ks_log_b, ks_d), dtype=np.uint64)
    with np.errstate(over="ignore"):
        pt = ((np.uint64(0) - s)[None, :] * kg[:, None]).reshape(ks_d * n)
        ksk_a = r64(rng, ks_d * n, n_lwe)
        ksk_b = (ksk_a * z).sum(axis=1, dtype=np.uint64) + noise(rng, sd_lwe, ks_d * n) + pt
    one = np.zeros(n, dtype=np.uint64)
    one[0] = 1
    plain = CM.pfksk_plain(pf_log_b, pf_d, s, np.stack([np.uint64(0) - s, one])).reshape(-1, n)
    ka, kb = CM._tglwe_encrypt(rng, s, plain, sd_glwe)
    pfksk = np.stack([ka, kb], axis=1).reshape(pf_d * (n + 1), 2, 2, n)
    return dict(z=z, s=s, bra=bra, brb=brb, ksk_a=ksk_a, ksk_b=ksk_b, pfksk=pfksk)


def tlwe_encrypt(rng, sk, pt, std_dev):
    pt = np.asarray(pt, dtype=np.uint64)
    a = r64(rng, pt.size, sk.size)
    with np.errstate(over="ignore"):
        return a, (a * sk).sum(axis=1, dtype=np.uint64) + noise(rng, std_dev, pt.size) + pt


def tlwe_phases(sk, a, b):
    with np.errstate(over="ignore"):
        return np.asarray(b, dtype=np.uint64) - (np.asarray(a, dtype=np.uint64) * sk).sum(axis=-1, dtype=np.uint64)


def selectors(K, log_b, d, ks_log_b, ks_d, cb_log_b, cb_d, pf_log_b, pf_d, m, lwe_a, lwe_b):
    """fhe_tfhe_wop_selectors by its definition, blind rotations and key switches by oracle.cref.
    -> (rows_a, rows_b [batch][m][2 cb_d][n], rem_a, rem_b, levels_a [batch m cb_d][n], levels_b, corrs: per step (a [batch][n], b [batch]))"""
    from oracle import cref
    n, n_lwe = K["s"].size, K["z"].size
    lwe_a, lwe_b = np.asarray(lwe_a, dtype=np.uint64).reshape(-1, n_lwe), np.asarray(lwe_b, dtype=np.uint64).reshape(-1)
    batch, nu = lwe_b.size, nu_of(cb_d)
    la, lb = np.zeros((batch, m, cb_d, n), dtype=np.uint64), np.zeros((batch, m, cb_d), dtype=np.uint64)
    src, cor, corrs = (lwe_a, lwe_b), (None, None), []
    for l in range(m):                                              # noqa: E741
        last = l == m - 1
        log_delta = -1 if last else 64 - m + l
        rem_a, rem_b, at, bt = front(src[0], src[1], cor[0], cor[1], m - 1 - l, n, nu)
        ra, rb = cref.tfhe_blind_rotate(log_b, d, K["bra"], K["brb"], wop_table(cb_log_b, cb_d, n, log_delta), at, bt)
        h = h_values(cb_log_b, cb_d, log_delta)
        ca, cb = np.zeros((batch, n), dtype=np.uint64), np.zeros(batch, dtype=np.uint64)
        for c in range(batch):
            for j in range(cb_d + (0 if last else 1)):
                xa, xb = cref.tglwe_sample_extract(ra[c], rb[c], j)
                xb = (int(xb) + h[j]) % M64
                if j < cb_d:
                    la[c, l, j], lb[c, l, j] = xa, xb
                else:
                    ca[c], cb[c] = xa, xb
        src = (rem_a, rem_b)
        if not last:
            corrs.append((ca, cb))
            sw = [cref.tlwe_key_switch(ks_log_b, ks_d, K["ksk_a"], K["ksk_b"], ca[c], int(cb[c])) for c in range(batch)]
            cor = (np.stack([x[0] for x in sw]), np.array([x[1] for x in sw], dtype=np.uint64))
    la, lb = la.reshape(batch * m * cb_d, n), lb.reshape(batch * m * cb_d)
    oa, ob = CM.pfks(pf_log_b, pf_d, K["pfksk"], 2, la, lb, n, n, group=cb_d)
    return oa.reshape(batch, m, 2 * cb_d, n), ob.reshape(batch, m, 2 * cb_d, n), src[0], src[1], la, lb, corrs


def lookup(cb_log_b, cb_d, rows_a, rows_b, polys, m, n):
    """fhe_tfhe_lut_eval for one ciphertext, one output, m <= log2 n (no tree): acc <- CMUX(selector l; acc, acc X^(-2^l)) by oracle.cref's
    external product, then sample_extract(0) -> (a [n], b)"""
    from oracle import cref
    assert (1 << m) <= n
    acc = (np.zeros(n, dtype=np.uint64), np.asarray(polys, dtype=np.uint64).reshape(n).copy())
    for l in range(m):                                              # noqa: E741
        rot = (LM.rotate(acc[0], -(1 << l)), LM.rotate(acc[1], -(1 << l)))
        ea, eb = cref.tggsw_external_product(cb_log_b, cb_d, rows_a[l], rows_b[l], rot[0] - acc[0], rot[1] - acc[1])
        acc = (acc[0] + np.asarray(ea, dtype=np.uint64).reshape(n), acc[1] + np.asarray(eb, dtype=np.uint64).reshape(n))
    xa, xb = cref.tglwe_sample_extract(acc[0], acc[1], 0)
    return xa, int(xb)


def centered(x):
    x %= M64
    return x - M64 if x >= M64 // 2 else x
