"""GPU tests of the look-up without a padding bit (k = 1): a reserved selector key filled in pieces on a side stream against a prepared
one in every key form; the step front against the model; exact extraction under noise-free keys and 64-bit gadgets; bit identity of
fhe_tfhe_wop_selectors and fhe_tfhe_wop_pbs with the public entries chained in every key form, host memory against device memory; two
rounds of a byte -> byte table at decode level; rejections; the C example."""
import math

import numpy as np
import pytest

import tfhe_wop_model as M

pytestmark = pytest.mark.gpu

WOP, BYTES = M.WOP, M.BYTES

M64 = 1 << 64
U = lambda x: np.array(x, dtype=np.uint64)  # noqa: E731
r64 = M.r64

# the key forms of tests/test_tfhe_lut_gpu.py: (n, log_b, d, NO_F64_EXACT while the key is made); FORM_OF: what fhe_tggsw_key_form must report
# for each, (form, packs_digits): (15, 1) at n = 256 and (10, 2): three 30-bit primes, unpacked; (7, 3): three key pieces through f64
# transforms, and with the switch three 30-bit primes with packed digits; (23, 1): two 60-bit primes
KEY_FORMS = [(256, 15, 1, False), (256, 7, 3, False), (256, 10, 2, False), (1024, 7, 3, False), (1024, 10, 2, False), (1024, 23, 1, False),
             (256, 7, 3, True), (1024, 7, 3, True)]
FORM_OF = dict(zip(KEY_FORMS, [("30", 0), ("x3", 0), ("30", 0), ("x3", 0), ("30", 0), ("60", 0), ("30", 1), ("30", 1)]))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


class steered:
    """the lab switch NO_F64_EXACT while keys are made: it picks the packed three-prime form"""
    def __init__(self, fhe, on):
        self.fhe, self.on = fhe, on

    def __enter__(self):
        if self.on:
            self.fhe.set_option("NO_F64_EXACT", 1)

    def __exit__(self, *exc):
        self.fhe.set_option("NO_F64_EXACT", 0)


# every exact form, and the fft64 form of the rings and gadgets the lab switch does not steer
FILL_FORMS = [f + (False,) for f in KEY_FORMS] + [f + (True,) for f in KEY_FORMS if not f[3]]


@pytest.mark.parametrize("n,log_b,d,no_f64,fft64", FILL_FORMS)
def test_fill_equals_prepare(fhe, torch_cuda, n, log_b, d, no_f64, fft64):
    """reserve(3), then on a side stream fill(1, two ciphertexts) and fill(0, one): fhe_tggsw_cmux under each index gives the bits it gives
    under a key prepared from the same three ciphertexts; a fill past the capacity is rejected"""
    torch = torch_cuda
    rng = np.random.Generator(np.random.PCG64(7700 + n + log_b))
    D = lambda x: dev(torch, x)  # noqa: E731
    ra, rb = D(r64(rng, 3, 2 * d, n)), D(r64(rng, 3, 2 * d, n))
    c0a, c0b, c1a, c1b = (D(r64(rng, 2, n)) for _ in range(4))
    t = fhe.TorusContext()
    with steered(fhe, no_f64):
        prepared = fhe.TggswKey(t, log_b, d, ra, rb, n, fft64=fft64)
        reserved = fhe.TggswKey.reserve(t, log_b, d, n, 3, fft64=fft64)
    want_form = ("fft64", 0) if fft64 else FORM_OF[(n, log_b, d, no_f64)]
    assert (prepared.form, prepared.packs_digits) == want_form and (reserved.form, reserved.packs_digits) == want_form
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        reserved.fill(1, ra[1:3].contiguous(), rb[1:3].contiguous())
        reserved.fill(0, ra[0:1].contiguous(), rb[0:1].contiguous())
        got = [reserved.cmux(i, c0a, c0b, c1a, c1b) for i in range(3)]
        with pytest.raises(fhe.FheError):
            reserved.fill(2, ra[0:2].contiguous(), rb[0:2].contiguous())
        with pytest.raises(fhe.FheError):
            reserved.fill(4, ra[0:0].contiguous(), rb[0:0].contiguous())
    torch.cuda.current_stream().wait_stream(side)
    for i in range(3):
        wa, wb = prepared.cmux(i, c0a, c0b, c1a, c1b)
        assert torch.equal(got[i][0], wa) and torch.equal(got[i][1], wb), i
    if not fft64:                                                   # host rows give the key device rows give
        with steered(fhe, no_f64):
            again = fhe.TggswKey.reserve(t, log_b, d, n, 3)
        again.fill(0, host(ra), host(rb))
        ha, hb = again.cmux(2, c0a, c0b, c1a, c1b)
        assert torch.equal(ha, got[2][0]) and torch.equal(hb, got[2][1])


@pytest.mark.parametrize("n_lwe", [1, 5, 630])
@pytest.mark.parametrize("batch", [1, 3, 69])
def test_front_kernel_bit_exact_vs_model(fhe, torch_cuda, n_lwe, batch):
    """m in 1, 2, 8, 16 at l = 0 (no correction, shift m - 1) and l = m - 1 (a correction, shift 0), n = 256 with nu = 2 and n = 2048 with
    nu = 5; the first words of a and b are 0, 2^64 - 1, and values whose shifted word plus half a position wraps past 2^64"""
    W = fhe.tfhe_wop
    rng = np.random.Generator(np.random.PCG64(7800 + 7 * n_lwe + batch))
    D = lambda x: dev(torch_cuda, x)  # noqa: E731
    for n, nu in ((256, 2), (2048, 5)):
        half = 1 << (64 - (n.bit_length()) + nu - 1)
        for m in (1, 2, 8, 16):
            for l in sorted({0, m - 1}):                            # noqa: E741
                shift = m - 1 - l
                a, b = r64(rng, batch, n_lwe), r64(rng, batch)
                edge = [0, M64 - 1, (M64 - half) >> shift, ((M64 - 1) >> shift), (M64 - half - 1) >> shift]
                for i, v in enumerate(edge):
                    a.ravel()[i % a.size] = v
                    b[i % batch] = (v - ((1 << 62) >> shift)) % M64 if i >= 2 else v
                cor = (r64(rng, batch, n_lwe), r64(rng, batch)) if l else None
                if cor is not None:
                    cor[0].ravel()[0], cor[1][0] = 0, M64 - 1
                want = M.front(a, b, cor[0] if cor else None, cor[1] if cor else None, shift, n, nu)
                got = W.wop_front(D(a), D(b), (D(cor[0]), D(cor[1])) if cor else None, n, nu, shift)
                for w, g, name in zip(want, got, ("rem_a", "rem_b", "at", "bt")):
                    assert np.array_equal(host(g), w), (n, m, l, name)
                if (n_lwe, batch) == (5, 3):                        # host memory: the same bits
                    hgot = W.wop_front(a, b, cor, n, nu, shift)
                    assert all(np.array_equal(h, w) for h, w in zip(hgot, want))


@pytest.fixture(scope="module")
def exact_keys(fhe, torch_cuda):
    """N = 256, n_lwe = 5, bootstrapping, key-switch and private-key-switch gadgets (16, 4): 64 bits, nothing is rounded away; every key at
    std_dev = 0"""
    n, n_lwe, log_b, d = 256, 5, 16, 4
    like = dev(torch_cuda, U([0]))
    t = fhe.TorusContext()
    z, s = fhe.sample_binary(7900, 0, like, n_lwe), fhe.sample_binary(7900, 1, like, n)
    pt = np.zeros((n_lwe, n), dtype=np.uint64)
    pt[:, 0] = host(z)
    ra, rb = fhe.tggsw_encrypt(t, log_b, d, s, dev(torch_cuda, pt), n, 0.0, 7901, 0)
    brk = fhe.TggswKey(t, log_b, d, ra, rb, n)
    pfksk = fhe.tfhe_cbs.pfksk_gen(t, log_b, d, s, s, fhe.tfhe_cbs.pfksk_funcs(s), 0.0, 7902, 0)
    ksk = fhe.tlwe_ksk_gen(log_b, d, z, s, 0.0, 7903, 0)
    return dict(n=n, n_lwe=n_lwe, log_b=log_b, d=d, t=t, z=z, s=s, brk=brk, pfksk=pfksk, ksk=ksk)


@pytest.mark.parametrize("m", [1, 3, 8])
def test_exact_extraction(fhe, torch_cuda, exact_keys, m):
    """messages 0, 2^m - 1 and an alternating pattern with nonzero low bits below 2^(61 - m); cb gadget (4, 3).  Through the chain: every
    level row decrypts to exactly bit g_j, every correction to exactly bit 2^delta.  Through the one call: the same rows bit for bit after
    the (exact) private functional key switch -- row (1, j) has phase bit g_j in coefficient 0 and nothing else, row (0, j) is -S times
    that -- and the returned remainder decrypts to exactly the low bits plus the top bit's term"""
    K, W = exact_keys, fhe.tfhe_wop
    n, n_lwe, cb_log_b, cb_d = K["n"], K["n_lwe"], 4, 3
    top = (1 << m) - 1
    xs = [0, top, 0xAA & top if m > 1 else 1]
    rng = np.random.Generator(np.random.PCG64(7950 + m))
    low = [int(v) | 1 for v in rng.integers(0, 1 << (61 - m), size=3)]
    pts = U([((x << (64 - m)) + e) % M64 for x, e in zip(xs, low)])
    la, lb = fhe.tlwe_sk_encrypt(K["z"], dev(torch_cuda, pts), n_lwe, 3, 0.0, 7951 + m, 0)
    ks = (K["log_b"], K["d"], K["ksk"][0], K["ksk"][1])
    args = (K["brk"], ks, cb_log_b, cb_d, K["log_b"], K["d"], K["pfksk"], m, la, lb)
    ra, rb, rem_a, rem_b = W.wop_selectors(*args, want_rem=True)
    sa, sb, srem_a, srem_b, lev_a, lev_b, corrs = W.wop_selectors_steps(*args)
    assert torch_cuda.equal(ra, sa) and torch_cuda.equal(rb, sb) and torch_cuda.equal(rem_a, srem_a) and torch_cuda.equal(rem_b, srem_b)
    zh, sh, g = host(K["z"]), host(K["s"]), M.CM.gadget(cb_log_b, cb_d)
    lev = M.tlwe_phases(sh, host(lev_a), host(lev_b)).reshape(3, m, cb_d)
    rem = M.tlwe_phases(zh, host(rem_a), host(rem_b))
    rows_a, rows_b = host(ra), host(rb)
    for c, x in enumerate(xs):
        for l in range(m):                                          # noqa: E741
            bit = (x >> l) & 1
            assert [int(v) for v in lev[c, l]] == [bit * g[j] for j in range(cb_d)], (c, l)
            if l < m - 1:
                assert int(M.tlwe_phases(sh, host(corrs[l][0])[c], host(corrs[l][1])[c])) == bit << (64 - m + l), (c, l)
            for j in range(cb_d):
                ph = M.CM.tglwe_phase(sh, rows_a[c, l, cb_d + j], rows_b[c, l, cb_d + j])
                assert int(ph[0]) == bit * g[j] and not ph[1:].any(), (c, l, j)
                with np.errstate(over="ignore"):
                    want = (np.uint64(0) - sh) * np.uint64(bit * g[j])
                assert np.array_equal(M.CM.tglwe_phase(sh, rows_a[c, l, j], rows_b[c, l, j]), want), (c, l, j)
        assert int(rem[c]) == (low[c] + ((x >> (m - 1)) << 63)) % M64, c


@pytest.mark.parametrize("n,log_b,d,no_f64", KEY_FORMS)
def test_bit_identity_with_the_chain(fhe, torch_cuda, n, log_b, d, no_f64):
    """random key rows, n_lwe = 8, the circuit bootstrap's gadget equal to the key's (so the selector key takes the same form), m = 1 and 4
    (and 11 at n = 256: a look-up tree of h = 3), batch 1 and 3.  fhe_tfhe_wop_selectors against the public entries chained; fhe_tfhe_wop_pbs
    with first_index = 2 against the chain's rows prepared by fhe_tggsw_prepare and read by fhe_tfhe_lut_eval, with and without the output
    key switch; exact form and fft64 form (device against device); host memory gives the bits of device memory (exact form)"""
    n_lwe, pf_log_b, pf_d, ks_log_b, ks_d, n_out, first, n_lwe_out = 8, 9, 2, 5, 3, 2, 2, 6
    cb_log_b, cb_d = log_b, d
    rng = np.random.Generator(np.random.PCG64(8000 + n + log_b))
    D = lambda x: dev(torch_cuda, x)  # noqa: E731
    t, W, C = fhe.TorusContext(), fhe.tfhe_wop, fhe.tfhe_cbs
    bra, brb, pfksk = r64(rng, n_lwe, 2 * d, n), r64(rng, n_lwe, 2 * d, n), r64(rng, pf_d * (n + 1), 2, 2, n)
    ksk_a, ksk_b = r64(rng, n * ks_d, n_lwe), r64(rng, n * ks_d)
    oksk_a, oksk_b = r64(rng, n * ks_d, n_lwe_out), r64(rng, n * ks_d)
    dk, dks = D(pfksk), (ks_log_b, ks_d, D(ksk_a), D(ksk_b))
    doks = (ks_log_b, ks_d, D(oksk_a), D(oksk_b), n_lwe_out)
    ms = (1, 4, 11) if n == 256 else (1, 4)
    cap = first + 3 * max(ms)
    with steered(fhe, no_f64):
        brk = {f: fhe.TggswKey(t, log_b, d, D(bra), D(brb), n, fft64=f) for f in (False, True)}
        sel = {f: fhe.TggswKey.reserve(t, cb_log_b, cb_d, n, cap, fft64=f) for f in (False, True)}
    for k in (brk, sel):
        assert (k[False].form, k[False].packs_digits) == FORM_OF[(n, log_b, d, no_f64)] and (k[True].form, k[True].packs_digits) == ("fft64", 0)
    for m in ms:
        polys = C.lut_pack(r64(rng, n_out, 1 << m), m, n)
        dp = D(polys)
        for batch in (1, 3):
            a, b = r64(rng, batch, n_lwe), r64(rng, batch)
            for fft64 in (False, True):
                args = (brk[fft64], dks, cb_log_b, cb_d, pf_log_b, pf_d, dk, m, D(a), D(b))
                ga, gb, ra_, rb_ = W.wop_selectors(*args, want_rem=True)
                sa, sb, sra, srb = W.wop_selectors_steps(*args)[:4]
                assert tuple(ga.shape) == (batch, m, 2 * cb_d, n)
                assert torch_cuda.equal(ga, sa) and torch_cuda.equal(gb, sb), (m, batch, fft64)
                assert torch_cuda.equal(ra_, sra) and torch_cuda.equal(rb_, srb), (m, batch, fft64)
                na, nb = W.wop_selectors(*args)                     # without the remainder: the same rows
                assert torch_cuda.equal(na, ga) and torch_cuda.equal(nb, gb)
                with steered(fhe, no_f64):
                    chain_key = fhe.TggswKey(t, cb_log_b, cb_d, sa.reshape(batch * m, 2 * cb_d, n), sb.reshape(batch * m, 2 * cb_d, n), n, fft64=fft64)
                for oks in (None, doks):
                    pa, pb = W.wop_pbs(*args, sel[fft64], first, dp, n_out, oks)
                    wa, wb = C.lut_eval_batch(dp, chain_key, 0, m, n_out, batch, oks)
                    assert tuple(pa.shape) == (batch, n_out, n_lwe_out if oks else n)
                    assert torch_cuda.equal(pa, wa) and torch_cuda.equal(pb, wb), (m, batch, fft64, oks is not None)
                    ta, tb = W.wop_pbs_steps(*args, sel[fft64], first, dp, n_out, oks)
                    assert torch_cuda.equal(ta, wa) and torch_cuda.equal(tb, wb)
                    if not fft64 and batch == 3 and m == 4:          # host memory (the keys stay device objects)
                        hks, hoks = (ks_log_b, ks_d, ksk_a, ksk_b), ((ks_log_b, ks_d, oksk_a, oksk_b, n_lwe_out) if oks else None)
                        ha, hb = W.wop_pbs(brk[False], hks, cb_log_b, cb_d, pf_log_b, pf_d, pfksk, m, a, b, sel[False], first, polys, n_out, hoks)
                        assert np.array_equal(ha, host(wa)) and np.array_equal(hb, host(wb))
                        if oks is None:
                            hra, hrb, hma, hmb = W.wop_selectors(brk[False], hks, cb_log_b, cb_d, pf_log_b, pf_d, pfksk, m, a, b, want_rem=True)
                            assert np.array_equal(hra, host(ga)) and np.array_equal(hrb, host(gb))
                            assert np.array_equal(hma, host(ra_)) and np.array_equal(hmb, host(rb_))


def test_two_rounds_decode_under_noisy_keys(fhe, torch_cuda):
    """DESIGN.md 9.5's decode-level parameters: the bytes 0x00, 0xFF, 0xA5, 0x3C, 0x81 at x << 56 (no padding bit) go through a fixed
    pseudo-random permutation table with words T[x] << 56, come back under the small key through the output key switch (gadget (4, 8)), and
    go through the same call again: T[x], then T[T[x]], each with its worst phase error below a quarter of the half-slot (2^53)"""
    p, m = WOP, WOP["m"]
    n, n_lwe = p["n"], p["n_lwe"]
    like = dev(torch_cuda, U([0]))
    t, W, C = fhe.TorusContext(), fhe.tfhe_wop, fhe.tfhe_cbs
    z, s = fhe.sample_binary(8100, 0, like, n_lwe), fhe.sample_binary(8100, 1, like, n)
    pt = np.zeros((n_lwe, n), dtype=np.uint64)
    pt[:, 0] = host(z)
    ra, rb = fhe.tggsw_encrypt(t, p["log_b"], p["d"], s, dev(torch_cuda, pt), n, p["sd_glwe"], 8101, 0)
    brk = fhe.TggswKey(t, p["log_b"], p["d"], ra, rb, n)
    pfksk = C.pfksk_gen(t, p["pf_log_b"], p["pf_d"], s, s, C.pfksk_funcs(s), p["sd_glwe"], 8102, 0)
    ksk_a, ksk_b = fhe.tlwe_ksk_gen(p["ks_log_b"], p["ks_d"], z, s, p["sd_lwe"], 8103, 0)
    ks = (p["ks_log_b"], p["ks_d"], ksk_a, ksk_b)
    table = np.random.Generator(np.random.PCG64(7403)).permutation(256)
    polys = dev(torch_cuda, C.lut_pack(U([int(v) << 56 for v in table]).reshape(1, 256), m, n))
    sel = fhe.TggswKey.reserve(t, p["cb_log_b"], p["cb_d"], n, len(BYTES) * m)
    ca, cb = fhe.tlwe_sk_encrypt(z, dev(torch_cuda, U([W.encode(x, m) for x in BYTES])), n_lwe, len(BYTES), p["sd_lwe"], 8104, 0)
    want = list(BYTES)
    for rnd in (1, 2):
        oa, ob = W.wop_pbs(brk, ks, p["cb_log_b"], p["cb_d"], p["pf_log_b"], p["pf_d"], pfksk, m, ca, cb, sel, 0, polys, 1, ks + (n_lwe,))
        ca, cb = oa.reshape(len(BYTES), n_lwe).contiguous(), ob.reshape(len(BYTES)).contiguous()
        want = [int(table[x]) for x in want]
        phases = M.tlwe_phases(host(z), host(ca), host(cb))
        worst = 0
        for w, ph in zip(want, (int(v) for v in phases)):
            err = abs(M.centered(ph - (w << 56)))
            worst = max(worst, err)
            assert ((ph + (1 << 55)) % M64) >> 56 == w, (rnd, hex(w))
        print("round %d: worst phase error 2^%.1f of half-slot 2^55" % (rnd, math.log2(max(worst, 1))))
        assert worst < 1 << 53                                      # a quarter of the half-slot
    assert want == [int(table[int(table[x])]) for x in BYTES]


def test_rejections_on_the_device(fhe, torch_cuda):
    """a selector key of another gadget, ring or context, or too small; outputs that are inputs or keys; a key-switch key missing at m > 1"""
    from learn_fhe_amd.ring import _buf
    n, log_b, d, n_lwe, m, batch = 256, 15, 1, 4, 2, 2
    rng = np.random.Generator(np.random.PCG64(8200))
    D = lambda x: dev(torch_cuda, x)  # noqa: E731
    t, other = fhe.TorusContext(), fhe.TorusContext()
    brk = fhe.TggswKey(t, log_b, d, D(r64(rng, n_lwe, 2 * d, n)), D(r64(rng, n_lwe, 2 * d, n)), n)
    pfksk, ka, kb = D(r64(rng, 2 * (n + 1), 2, 2, n)), D(r64(rng, n * 3, n_lwe)), D(r64(rng, n * 3))
    a, b = D(r64(rng, batch, n_lwe)), D(r64(rng, batch))
    rows_a, rows_b = D(np.zeros((batch, m, 2 * d, n), dtype=np.uint64)), D(np.zeros((batch, m, 2 * d, n), dtype=np.uint64))
    polys = D(fhe.lut_pack(r64(rng, 1, 1 << m), m, n))
    oa, ob = D(np.zeros((batch, 1, n), dtype=np.uint64)), D(np.zeros((batch, 1), dtype=np.uint64))
    P = lambda x: _buf(x)[0]  # noqa: E731
    mem, st, lib = _buf(a)[2], _buf(a)[3], fhe.lib()

    def selectors(th=t.handle, ksa=ka, ra=rows_a, rb=rows_b, mm=m, cb_d=d, cb_log_b=log_b, nb=batch):
        return lib.fhe_tfhe_wop_selectors(th, brk._h, 5, 3, P(ksa) if ksa is not None else None, P(kb), cb_log_b, cb_d, 9, 2, P(pfksk), mm, P(a), P(b),
                                          P(ra), P(rb), None, None, nb, mem, st)
    assert selectors() == 0
    assert selectors(th=other.handle) == 1 and selectors(ksa=None) == 1 and selectors(ra=rows_b) == 1
    assert selectors(ra=a) == 1 and selectors(rb=pfksk) == 1 and selectors(ra=ka) == 1
    assert selectors(mm=0) == 1 and selectors(mm=17) == 6 and selectors(cb_d=0) == 1 and selectors(cb_d=17) == 1 and selectors(cb_log_b=64) == 1
    assert selectors(nb=0) == 0
    assert lib.fhe_tfhe_wop_selectors(t.handle, brk._h, 5, 3, P(ka), P(kb), log_b, d, 9, 2, P(pfksk), m, P(a), P(b), P(rows_a), P(rows_b), P(oa), None,
                                      batch, mem, st) == 1          # one half of the remainder
    good = fhe.TggswKey.reserve(t, log_b, d, n, batch * m + 1)
    small = fhe.TggswKey.reserve(t, log_b, d, n, batch * m - 1)
    gadget = fhe.TggswKey.reserve(t, 7, 3, n, batch * m)
    ring = fhe.TggswKey.reserve(t, log_b, d, 512, batch * m)
    foreign = fhe.TggswKey.reserve(other, log_b, d, n, batch * m)

    def pbs(key=good, first=1, out_a=oa, out_b=ob):
        return lib.fhe_tfhe_wop_pbs(t.handle, brk._h, 5, 3, P(ka), P(kb), log_b, d, 9, 2, P(pfksk), m, P(a), P(b), key._h, first, P(polys), 1, 0, 0, None,
                                    None, 0, P(out_a), P(out_b), batch, mem, st)
    assert pbs() == 0
    assert pbs(first=2) == 1 and pbs(key=small, first=0) == 1 and pbs(key=gadget, first=0) == 1 and pbs(key=ring, first=0) == 1
    assert pbs(key=foreign, first=0) == 1 and pbs(key=brk, first=0) == 1
    assert pbs(out_a=polys) == 1 and pbs(out_b=a) == 1 and pbs(out_a=ob) == 1
    assert lib.fhe_tggsw_key_fill(good._h, 0, None, P(rows_b), 1, mem, st) == 1
    assert lib.fhe_tggsw_key_fill(good._h, batch * m, P(rows_a), P(rows_b), 2, mem, st) == 1
    import ctypes
    h = ctypes.c_void_p()
    assert lib.fhe_tggsw_key_reserve(t.handle, log_b, d, n, 0, 0, ctypes.byref(h)) == 1 and lib.fhe_tggsw_key_reserve(t.handle, log_b, d, 128, 4, 0, ctypes.byref(h)) == 6
    torch_cuda.cuda.synchronize()


def test_c_program_tfhe_wop(tmp_path, fhe):
    """examples/tfhe_wop_demo.c: three encrypted bytes with no padding bit through a byte -> byte table in one call, decrypted in the
    program, from plain C against include/fhe_ring.h alone"""
    import os
    import subprocess
    from conftest import ROOT
    lib_dir = os.path.dirname(fhe.lib_path())
    exe = tmp_path / "tfhe_wop_demo"
    cmd = ["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "tfhe_wop_demo.c"), "-o", str(exe),
           "-L", lib_dir, "-lfhe_ring", "-Wl,--allow-shlib-undefined", "-Wl,-rpath," + lib_dir, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tfhe_wop_demo ok" in r.stdout, r.stdout + r.stderr
