"""What a key generator can get wrong without any decryption noticing, as checks on the EXACT noise of its output.  Given the secret
key, the oracle (oracle/cref.py) computes a s and the gadget term of every row exactly, so the noise of every coefficient is an
integer that can be held against the sampler's support, against its law, and against the other rows.  Plain helpers for
tests/test_keygen_rows_gpu.py and tests/test_keygen_checks_cpu.py: nothing here models the generator's keystream, and nothing here
chooses a device -- the law checks run wherever their input lives (numpy arrays on the host, torch tensors where they are).

  dg_weights       the reference's dg(std_dev, n) weights (util/src/misc/distribution.rs:23-46)
  chi2_dg          Pearson's X^2 of integer samples against those weights; chi2_ok: X^2 <= dof + 6 sqrt(2 dof)
  chi2_counts      the same statistic for any bucket counts against any probabilities (uniform buckets, zo)
  ks_normal        Kolmogorov distance to N(0, std_dev); ks_ok: D <= 3 / sqrt(N)
  rows_independent no row repeated, no row zero, no two rows correlated
  *_residual       the centred integer noise of each ciphertext shape
"""
import math

import numpy as np

M64 = 1 << 64


def _is_torch(x):
    return type(x).__module__.startswith("torch")


# ---- laws -------------------------------------------------------------------------------------------------------------------

def _erf_as(x):  # Abramowitz-Stegun 7.1.26, the approximation the reference's `dg` is built on (distribution.rs:30-39)
    p, a1, a2, a3, a4, a5 = 0.3275911, 0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429
    t = 1.0 / (1.0 + p * abs(x))
    pos = 1.0 - (((((a5 * t + a4) * t) + a3) * t + a2) * t + a1) * t * math.exp(-x * x)
    return pos if x >= 0 else -pos


def dg_max(std_dev, n_sigma):
    return int(math.floor(n_sigma * std_dev))


def dg_weights(std_dev, n_sigma):
    """probabilities of -max .. max, max = floor(n_sigma std_dev): cdf(i + 0.5) - cdf(i - 0.5) with the A&S erf, normalised"""
    cdf = lambda x: (1.0 + _erf_as(x / (std_dev * math.sqrt(2)))) / 2.0  # noqa: E731
    mx = dg_max(std_dev, n_sigma)
    w = np.array([cdf(i + 0.5) - cdf(i - 0.5) for i in range(-mx, mx + 1)], dtype=np.float64)
    return w / w.sum()


def chi2_counts(counts, probs, min_expected=5.0):
    """(X^2, dof) of bucket counts against bucket probabilities; buckets are merged inwards from both ends until the outermost
    ones expect at least `min_expected` samples (the usual validity condition of Pearson's approximation)"""
    obs = [float(c) for c in counts]
    total = sum(obs)
    exp = [float(p) * total for p in probs]
    assert len(obs) == len(exp) and total > 0
    while len(exp) > 2 and exp[0] < min_expected:
        exp[1] += exp[0]; obs[1] += obs[0]; del exp[0], obs[0]           # noqa: E702
    while len(exp) > 2 and exp[-1] < min_expected:
        exp[-2] += exp[-1]; obs[-2] += obs[-1]; del exp[-1], obs[-1]     # noqa: E702
    assert min(exp) >= min_expected, "too few samples for a chi-square"
    return sum((o - e) ** 2 / e for o, e in zip(obs, exp)), len(exp) - 1


def chi2_bound(dof):
    return dof + 6.0 * math.sqrt(2.0 * dof)


def chi2_ok(x2, dof):
    return x2 <= chi2_bound(dof)


def bincount(samples, lo, hi):
    """counts of the integers lo .. hi in `samples` (numpy int64 or a torch int64 tensor on any device); anything outside raises"""
    if _is_torch(samples):
        import torch
        s = samples.reshape(-1)
        assert int(s.min()) >= lo and int(s.max()) <= hi, "sample outside [%d, %d]" % (lo, hi)
        return torch.bincount(s - lo, minlength=hi - lo + 1).cpu().numpy()
    s = np.asarray(samples, dtype=np.int64).ravel()
    assert int(s.min()) >= lo and int(s.max()) <= hi, "sample outside [%d, %d]" % (lo, hi)
    return np.bincount(s - lo, minlength=hi - lo + 1)


def chi2_dg(samples_i64, std_dev, n_sigma):
    """(X^2, dof) of integer samples against dg(std_dev, n_sigma) over the bins -max .. max, tails merged to >= 5 expected"""
    mx = dg_max(std_dev, n_sigma)
    return chi2_counts(bincount(samples_i64, -mx, mx), dg_weights(std_dev, n_sigma))


def ks_normal(samples_f64, std_dev):
    """Kolmogorov distance sup |F_N - Phi(. / std_dev)| of the samples (numpy float64, or a torch float64 tensor on any device)"""
    import torch
    x = samples_f64 if _is_torch(samples_f64) else torch.from_numpy(np.ascontiguousarray(samples_f64, dtype=np.float64))
    x = torch.sort(x.reshape(-1).to(torch.float64)).values
    n = x.numel()
    cdf = 0.5 * (1.0 + torch.erf(x / (std_dev * math.sqrt(2.0))))
    steps = torch.arange(n, dtype=torch.float64, device=x.device)
    return float(torch.maximum(((steps + 1.0) / n - cdf).max(), (cdf - steps / n).max()))


def ks_bound(count):
    return 3.0 / math.sqrt(count)


def ks_ok(dist, count):
    return dist <= ks_bound(count)


# ---- rows -------------------------------------------------------------------------------------------------------------------

def as_rows(res, width=256):
    """[rows][n] residuals for rows_independent: rows shorter than `width` (scalar LWE noise, tiny rings) are regrouped, in
    order, into rows of `width`, so that a repeated stretch of noise still shows as a repeated or correlated row"""
    res = np.asarray(res)
    if res.ndim == 2 and res.shape[1] >= width:
        return res
    flat = res.ravel()
    assert flat.size >= 2 * width, "too few residuals to compare rows"
    return flat[: flat.size // width * width].reshape(-1, width)


def rows_independent(res):
    """`res` [rows][n] integer residuals: no two rows equal, no row all zero, and for n >= 256 every pairwise Pearson
    correlation below 6 / sqrt(n) in absolute value (of 64 evenly spaced rows plus the first and last when there are more than
    64).  Returns the worst correlation seen (0.0 when n < 256); raises AssertionError otherwise."""
    res = np.asarray(res)
    assert res.ndim == 2 and res.shape[0] >= 2, res.shape
    rows, n = res.shape
    flat = np.ascontiguousarray(res.astype(np.int64))
    zero = [r for r in range(rows) if not flat[r].any()]
    assert not zero, "all-zero noise in rows %s" % zero[:8]
    seen = {}
    for r in range(rows):
        first = seen.setdefault(flat[r].tobytes(), r)
        assert first == r, "rows %d and %d carry the same noise" % (first, r)
    if n < 256:
        return 0.0
    pick = list(range(rows)) if rows <= 64 else sorted({0, rows - 1} | {(i * rows) // 64 for i in range(64)})
    x = flat[pick].astype(np.float64)
    x -= x.mean(axis=1, keepdims=True)
    norm = np.sqrt((x * x).sum(axis=1, keepdims=True))
    assert norm.min() > 0, "a constant row"
    c = (x / norm) @ (x / norm).T
    np.fill_diagonal(c, 0.0)
    worst = float(np.abs(c).max())
    i, j = np.unravel_index(int(np.abs(c).argmax()), c.shape)
    assert worst < 6.0 / math.sqrt(n), "rows %d and %d correlate: %.4f (limit %.4f)" % (pick[i], pick[j], worst, 6.0 / math.sqrt(n))
    return worst


# ---- exact residuals --------------------------------------------------------------------------------------------------------

def _u64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64))


def centre(v, q):
    """residues mod q (q < 2^63) -> centred int64 in (-q/2, q/2]"""
    v = _u64(v)
    return np.where(v > np.uint64(q // 2), v.astype(np.int64) - np.int64(q), v.astype(np.int64))


def sub_mod(q, x, y):
    x, y = _u64(x), _u64(y)
    return np.where(x >= y, x - y, x + (np.uint64(q) - y))


def rq_mul_rows(q, a, s):
    """a [rows][n] times the one polynomial s [n] in Z_q[X] / (X^n + 1), exactly (oracle products: the transform-based one where
    the oracle's transform exists, the schoolbook one on the smallest rings)"""
    from oracle import cref
    a, s = _u64(a), _u64(s)
    rows, n = a.shape
    if n == 1:
        return cref.pointwise_mul(q, a, np.tile(s, rows)).reshape(rows, n)
    if n < 8:
        return np.stack([cref.schoolbook_mul(q, a[r], s) for r in range(rows)])
    return cref.ntt_mul(q, a, np.tile(s, (rows, 1)), n).reshape(rows, n)


def gadget_bases(q, log_b, d):
    """util/src/misc/decompose.rs:49-64: base_j = 2^(rounding_bits + j log_b) mod q, rounding_bits = max(0, log_q - log_b d)"""
    rb = max(0, (q - 1).bit_length() - log_b * d)
    return [pow(2, rb + j * log_b, q) for j in range(d)]


def scalar_mul_mod(q, v, c):
    """v [..] residues times the constant c mod q, on Python integers"""
    v = np.asarray(v)
    return np.array([(int(x) * int(c)) % q for x in v.ravel()], dtype=np.uint64).reshape(v.shape)


def rlwe_residual(q, sk, a, b, pt=None, on_a=None):
    """rlwe.rs:146-156: e = b - (a - on_a) sk - pt for a, b [rows][n]; pt / on_a [rows][n] or None (the term an RGSW row carries on
    its b / its a, rgsw.rs:100-103).  Centred."""
    a, b = _u64(a), _u64(b)
    if on_a is not None:
        a = sub_mod(q, a, on_a)
    e = sub_mod(q, b, rq_mul_rows(q, a, sk))
    if pt is not None:
        e = sub_mod(q, e, pt)
    return centre(e, q)


def lwe_residual(q, sk, a, b, pt=None):
    """lwe.rs:128-139: e[r] = b[r] - <a[r], sk> - pt[r] over any q < 2^62; the inner products on Python integers.  Centred."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    n = a.shape[1]
    if q * q * n < M64:   # every partial sum fits a word: numpy's integers are exact here
        ip = (a * _u64(sk)[None, :]).sum(axis=1, dtype=np.uint64) % np.uint64(q)
    else:
        s = [int(x) for x in sk]
        ip = np.array([sum(int(x) * y for x, y in zip(row, s)) % q for row in a], dtype=np.uint64)
    e = sub_mod(q, b, ip)
    if pt is not None:
        e = sub_mod(q, e, pt)
    return centre(e, q)


def lwe_ksk_terms(q, log_b, d, sk1):
    """lwe.rs:108-119 `power_up(-sk1).flatten()`: row r = j n1 + i carries -sk1[i] base_j mod q (digit-major)"""
    s = [int(x) for x in sk1]
    return np.array([(-(x * g)) % q for g in gadget_bases(q, log_b, d) for x in s], dtype=np.uint64)


def tlwe_residual(sk, a, b, pt=None):
    """tlwe.rs:122-132 on the torus (wrapping u64): e[r] = b[r] - <a[r], sk> - pt[r] as int64"""
    e = _u64(b) - (_u64(a) @ _u64(sk))
    if pt is not None:
        e = e - _u64(pt)
    return e.view(np.int64)


def tlwe_ksk_terms(log_b, d, sk1):
    """tlwe.rs:100-111: row r = j n1 + i carries -sk1[i] 2^(64 - log_b d + j log_b) on the torus"""
    s = _u64(sk1)
    return np.concatenate([(np.uint64(0) - s) << np.uint64(64 - log_b * d + j * log_b) for j in range(d)])


def torus_shift(pt, bits):
    return _u64(pt) << np.uint64(bits)


def tglwek_residual(k, sk, ct, pt=None, skip=None):
    """tglwe.rs:91-103 at rank k: ct [rows][k + 1][n], sk [k][n]: e = b - sum_c a_c s_c - pt as int64, products by the exact
    oracle.  `skip` = (component, term [rows][n]): a_component carries `term`, which is taken off before the product (the TGGSW
    rows whose message sits on a mask, tggsw.rs:80-87)."""
    from oracle import cref
    ct, sk = _u64(ct), _u64(sk).reshape(k, -1)
    rows, n = ct.shape[0], ct.shape[2]
    e = ct[:, k].copy()
    for c in range(k):
        a = ct[:, c] - skip[1] if skip is not None and skip[0] == c else ct[:, c]
        for r in range(rows):
            e[r] -= cref.torus_mul_exact(a[r], sk[c])
    if pt is not None:
        e = e - _u64(pt)
    return e.view(np.int64)


def tglwe_residual(sk, a, b, pt=None, on_a=None):
    """the k = 1 entries keep mask and body apart: a, b [rows][n]"""
    ct = np.stack([_u64(a), _u64(b)], axis=1)
    return tglwek_residual(1, sk, ct, pt, None if on_a is None else (0, _u64(on_a)))


def ckks_residual(mods, sk_i64, b, a, pt=None):
    """ckks.rs:215-225 (b = -(a s) + e + pt): b, a [rows][limbs][n] over `mods`; the centred b + a s - pt of every limb,
    [limbs][rows][n] -- one integer noise polynomial, so every limb must give the same one"""
    from oracle import cref
    b, a = _u64(b), _u64(a)
    rows, limbs, n = b.shape
    assert limbs == len(mods)
    s = cref.rns_from_i64(mods, np.asarray(sk_i64, dtype=np.int64))
    out = []
    for l, m in enumerate(mods):
        as_ = rq_mul_rows(m, a[:, l], s[l])
        t = b[:, l] + as_
        t = np.where(t >= np.uint64(m), t - np.uint64(m), t)
        if pt is not None:
            t = sub_mod(m, t, _u64(pt)[:, l])
        out.append(centre(t, m))
    return np.stack(out)
