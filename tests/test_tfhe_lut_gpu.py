"""GPU tests of the vertically packed table look-up (fhe_tfhe_lut_eval, k = 1): the exact plain result under noise-free keys for every
shape class (no tree, m = log n, a tree, shared and half-empty accumulators) with a different address per ciphertext; bit identity with
the public entries chained in every key form, with and without the key switch, host memory against device memory; a 256-entry look-up
at decode level on circuit-bootstrapped selectors; the C example."""
import math

import numpy as np
import pytest

import tfhe_lut_model as M

pytestmark = pytest.mark.gpu

M64 = 1 << 64
U = lambda x: np.array(x, dtype=np.uint64)  # noqa: E731


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def r64(rng, *shape):
    return rng.integers(0, 1 << 63, size=shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)


def tlwe_phases(s, a, b):
    """b - <a, s> mod 2^64 for a [..][n], b [..] (tlwe.rs:134-142 before decoding)"""
    with np.errstate(over="ignore"):
        return b - (a * s).sum(axis=-1, dtype=np.uint64)


@pytest.fixture(scope="module")
def exact_keys(fhe, torch_cuda):
    """n = 256, gadget (16, 4): 64 bits, the digits round nothing away; a binary TGLWE key s; every key row made at std_dev = 0"""
    n, log_b, d = 256, 16, 4
    like = dev(torch_cuda, U([0]))
    t = fhe.TorusContext()
    s = fhe.sample_binary(7100, 0, like, n)
    return dict(n=n, log_b=log_b, d=d, t=t, s=s, sh=host(s))


def addresses_for(m, batch):
    """0, 2^m - 1 (a rotation by n - 1 at m = 8) and, behind a tree, one address per leaf (m = 10 at n = 256: the top two bits 0 .. 3);
    every ciphertext of a batch gets a different one"""
    top = (1 << m) - 1
    five = [0, top, top // 3, 2 * (top // 3), top - 2]      # m = 10: 0x000, 0x3FF, 0x155, 0x2AA, 0x3FD: leaves 0, 3, 1, 2, 3
    return {1: [top], 3: [0, top, five[3]], 5: five}[batch]


@pytest.mark.parametrize("batch", [1, 3, 5])
@pytest.mark.parametrize("m,n_out", [(3, 1), (3, 3), (7, 5), (8, 1), (10, 1)])
def test_exact_plain_result(fhe, torch_cuda, exact_keys, m, n_out, batch):
    """every key at std_dev = 0 under a 64-bit gadget: each CMUX returns exactly the ciphertext its selector bit picks, so the phase of
    output o of ciphertext c IS table[o][address_c].  m = 3: no tree, n_out = 3 shares one accumulator; (7, 5): per_acc = 2, three
    accumulators, the last half empty; m = 8 = log n; m = 10: a tree of four leaves per accumulator (levels of two pairs and one)"""
    K = exact_keys
    n, C = K["n"], fhe.tfhe_cbs
    rng = np.random.Generator(np.random.PCG64(7200 + 16 * m + n_out))
    table = r64(rng, n_out, 1 << m)
    addresses = addresses_for(m, batch)
    assert len(set(addresses)) == batch
    if batch == 5 and m == 10:
        assert {a >> 8 for a in addresses} == {0, 1, 2, 3}          # every leaf of the tree is read
    first = 2                                                       # two unused selectors in front
    bits = np.zeros((first + batch * m, n), dtype=np.uint64)
    for c, x in enumerate(addresses):
        for l in range(m):                                          # noqa: E741
            bits[first + c * m + l, 0] = (x >> l) & 1
    bits[:first, 0] = 1
    ra, rb = fhe.tggsw_encrypt(K["t"], K["log_b"], K["d"], K["s"], dev(torch_cuda, bits), n, 0.0, 7201, m)
    sel = fhe.TggswKey(K["t"], K["log_b"], K["d"], ra, rb, n)
    polys = C.lut_pack(table, m, n)
    assert np.array_equal(polys, M.pack(table, m, n))
    try:
        for route in (0, 1, 2):                                     # the library's rule, the ladder extracts, the extraction kernel
            fhe.set_option("LUT_EXTRACT", route)
            oa, ob = C.lut_eval_batch(dev(torch_cuda, polys), sel, first, m, n_out, batch)
            assert tuple(oa.shape) == (batch, n_out, n) and tuple(ob.shape) == (batch, n_out)
            got = tlwe_phases(K["sh"], host(oa), host(ob))
            for c, x in enumerate(addresses):
                want = M.lookup(polys, m, n_out, x)
                assert want == [int(table[o, x]) for o in range(n_out)]
                assert [int(v) for v in got[c]] == want, (route, c, hex(x))
    finally:
        fhe.set_option("LUT_EXTRACT", 0)


# exact key forms fhe_tggsw_prepare can be steered to: (23, 1) at n = 1024: two 60-bit primes; (7, 3): three key pieces through f64 transforms;
# (10, 2), and (15, 1) at n = 256 (bound 2d N 2^(62 + log_b) = 2^87): three 30-bit primes, unpacked (base > 2^7).  The last two entries prepare
# (7, 3) with the f64 route switched off: three 30-bit primes with the digits computed once (the packed form), on a one-wave team (n = 256)
# and on a team of several waves (n = 1024: the per-team LDS stride then carries the digit area).  FORM_OF has what each entry must report
# (fhe_tggsw_key_form): (form, packs_digits); tests/test_tfhe_forms_gpu.py runs every form at every ring size against the oracle
KEY_FORMS = [(256, 15, 1, False), (256, 7, 3, False), (256, 10, 2, False), (1024, 7, 3, False), (1024, 10, 2, False), (1024, 23, 1, False),
             (256, 7, 3, True), (1024, 7, 3, True)]
FORM_OF = dict(zip(KEY_FORMS, [("30", 0), ("x3", 0), ("30", 0), ("x3", 0), ("30", 0), ("60", 0), ("30", 1), ("30", 1)]))


@pytest.mark.parametrize("n,log_b,d,no_f64", KEY_FORMS)
def test_bit_identity_with_the_chain(fhe, torch_cuda, n, log_b, d, no_f64):
    """random key rows; n = 256: m = 10, n_out = 3 (a tree of four leaves on three accumulators, 8 rotation steps), n = 1024: m = 11, n_out
    = 2 (one tree level, 10 rotation steps); batch 3, first_index = 2.  fhe_tfhe_lut_eval against fhe_tggsw_cmux, fhe_tglwe_rotate,
    fhe_tglwe_sample_extract and fhe_tlwe_key_switch chained per ciphertext: the same bits with and without the key switch, in the exact form
    and in the fft64 form (device against device); host memory gives the bits of device memory (exact form); both extraction routes (lab
    switch LUT_EXTRACT) give the same bits"""
    m, n_out = (10, 3) if n == 256 else (11, 2)
    batch, first, n_lwe_out, ks_log_b, ks_d = 3, 2, 8, 4, 3
    rng = np.random.Generator(np.random.PCG64(7300 + n + log_b))
    count = first + batch * m
    ra, rb = r64(rng, count, 2 * d, n), r64(rng, count, 2 * d, n)
    table = r64(rng, n_out, 1 << m)
    ksk_a, ksk_b = r64(rng, n * ks_d, n_lwe_out), r64(rng, n * ks_d)
    t, C = fhe.TorusContext(), fhe.tfhe_cbs
    D = lambda x: dev(torch_cuda, x)  # noqa: E731
    try:
        if no_f64:
            fhe.set_option("NO_F64_EXACT", 1)
        keys = {f: fhe.TggswKey(t, log_b, d, D(ra), D(rb), n, fft64=f) for f in (False, True)}
    finally:
        fhe.set_option("NO_F64_EXACT", 0)
    assert (keys[False].form, keys[False].packs_digits) == FORM_OF[(n, log_b, d, no_f64)] and (keys[True].form, keys[True].packs_digits) == ("fft64", 0)
    polys = C.lut_pack(table, m, n)
    dp, dks = D(polys), (ks_log_b, ks_d, D(ksk_a), D(ksk_b), n_lwe_out)
    for fft64 in (False, True):
        for ks in (None, dks):
            ga, gb = C.lut_eval_batch(dp, keys[fft64], first, m, n_out, batch, ks)
            sa, sb = C.lut_eval_batch_steps(dp, keys[fft64], first, m, n_out, batch, ks)
            assert tuple(ga.shape) == (batch, n_out, n_lwe_out if ks else n) and tuple(sa.shape) == tuple(ga.shape)
            assert torch_cuda.equal(ga, sa) and torch_cuda.equal(gb, sb), (fft64, ks is not None)
            try:
                for route in (1, 2):                                # the ladder extracts / the extraction kernel: the bits of the rule's route
                    fhe.set_option("LUT_EXTRACT", route)
                    ra_, rb_ = C.lut_eval_batch(dp, keys[fft64], first, m, n_out, batch, ks)
                    assert torch_cuda.equal(ra_, ga) and torch_cuda.equal(rb_, gb), (fft64, ks is not None, route)
            finally:
                fhe.set_option("LUT_EXTRACT", 0)
            if not fft64:
                exact = (ga, gb)
                hks = (ks_log_b, ks_d, ksk_a, ksk_b, n_lwe_out) if ks else None
                ha, hb = C.lut_eval_batch(polys, keys[False], first, m, n_out, batch, hks)
                assert np.array_equal(ha, host(ga)) and np.array_equal(hb, host(gb)), ks is not None
    if no_f64:  # the older three-prime kernel: the same bits
        try:
            fhe.set_option("NO_PACKED_DIGITS", 1)
            assert keys[False].packs_digits == 0
            pa, pb = C.lut_eval_batch(dp, keys[False], first, m, n_out, batch, dks)
        finally:
            fhe.set_option("NO_PACKED_DIGITS", 0)
        assert torch_cuda.equal(pa, exact[0]) and torch_cuda.equal(pb, exact[1])   # `exact`: the exact form's call with the key switch


def test_rejections_on_the_device(fhe, torch_cuda):
    """selectors past the key's count, a key of another context, outputs that are inputs"""
    from learn_fhe_amd.ring import _buf
    n, log_b, d, m = 256, 15, 1, 3
    rng = np.random.Generator(np.random.PCG64(7350))
    D = lambda x: dev(torch_cuda, x)  # noqa: E731
    t, other = fhe.TorusContext(), fhe.TorusContext()
    key = fhe.TggswKey(t, log_b, d, D(r64(rng, 7, 2 * d, n)), D(r64(rng, 7, 2 * d, n)), n)
    polys = D(fhe.lut_pack(r64(rng, 1, 1 << m), m, n))
    oa, ob = D(np.zeros((2, 1, n), dtype=np.uint64)), D(np.zeros((2, 1), dtype=np.uint64))
    pp, _, mem, st = _buf(polys)
    call = lambda th, first, batch, a, b: fhe.lib().fhe_tfhe_lut_eval(th, key._h, first, m, pp, 1, 0, 0, None, None, 0, a, b, batch, mem, st)  # noqa: E731
    assert call(t.handle, 1, 2, _buf(oa)[0], _buf(ob)[0]) == 0          # 1 + 2 * 3 = 7 selectors: the whole key
    assert call(t.handle, 2, 2, _buf(oa)[0], _buf(ob)[0]) == 1          # one past the key
    assert call(other.handle, 1, 2, _buf(oa)[0], _buf(ob)[0]) == 1      # the key belongs to another context
    assert call(t.handle, 1, 2, pp, _buf(ob)[0]) == 1 and call(t.handle, 1, 2, _buf(oa)[0], pp) == 1     # an output is the table
    assert call(t.handle, 1, 2, _buf(oa)[0], _buf(oa)[0]) == 1
    assert call(t.handle, 1, 0, None, None) == 0                         # nothing to do


# decode-level parameters of tests/test_tfhe_cbs_gpu.py (DESIGN.md 9.3 derives the noise; 9.4: the depth is m = 8 CMUXes here as there)
LUT = dict(n=1024, n_lwe=8, log_b=10, d=4, cb_log_b=4, cb_d=6, pf_log_b=7, pf_d=6, sd_lwe=2.0 ** -30, sd_glwe=2.845267479601915e-15, log_p=8)


def test_lut_batch_decodes_under_noisy_keys(fhe, torch_cuda):
    """the 3 x 8 bits of 0x00, 0xFF, 0xA5 are circuit-bootstrapped in one call and prepared once with count = 24; ONE lut_eval_batch reads
    a fixed pseudo-random permutation of 0 .. 255 (log_p = 8, one padding bit) for all three; decrypted under the extracted key
    (tlwe.rs:134-142) every result is the table's entry, and the worst phase error stays below a quarter of the half-slot"""
    p = LUT
    n, n_lwe, m, log_delta = p["n"], p["n_lwe"], 8, 64 - (p["log_p"] + 1)
    like = dev(torch_cuda, U([0]))
    t = fhe.TorusContext()
    z, s = fhe.sample_binary(7400, 0, like, n_lwe), fhe.sample_binary(7400, 1, like, n)
    pt = np.zeros((n_lwe, n), dtype=np.uint64)
    pt[:, 0] = host(z)
    ra, rb = fhe.tggsw_encrypt(t, p["log_b"], p["d"], s, dev(torch_cuda, pt), n, p["sd_glwe"], 7401, 0)
    brk = fhe.TggswKey(t, p["log_b"], p["d"], ra, rb, n)
    C = fhe.tfhe_cbs
    pfksk = C.pfksk_gen(t, p["pf_log_b"], p["pf_d"], s, s, C.pfksk_funcs(s), p["sd_glwe"], 7402, 0)
    table = np.random.Generator(np.random.PCG64(7403)).permutation(256)
    words = U([int(v) << log_delta for v in table]).reshape(1, 256)
    byts = [0x00, 0xFF, 0xA5]
    bits = U([(x >> l) & 1 for x in byts for l in range(m)])
    ca, cb = fhe.tlwe_sk_encrypt(z, dev(torch_cuda, bits << np.uint64(62)), n_lwe, bits.size, p["sd_lwe"], 7404, 0)
    sa, sb = C.circuit_bootstrap(brk, p["cb_log_b"], p["cb_d"], p["pf_log_b"], p["pf_d"], pfksk, ca, cb)
    sel = fhe.TggswKey(t, p["cb_log_b"], p["cb_d"], sa, sb, n)
    assert sel.count == len(byts) * m
    oa, ob = C.lut_eval_batch(dev(torch_cuda, C.lut_pack(words, m, n)), sel, 0, m, 1, len(byts))
    phases = tlwe_phases(host(s), host(oa), host(ob)).reshape(len(byts))
    worst = 0
    for x, ph in zip(byts, (int(v) for v in phases)):
        want = int(table[x])
        err = (ph - (want << log_delta)) % M64
        err = err - M64 if err >= M64 // 2 else err
        print("byte %#04x: phase error 2^%.1f" % (x, math.log2(max(abs(err), 1))))
        worst = max(worst, abs(err))
        assert ((ph + (1 << (log_delta - 1))) % M64) >> log_delta == want, hex(x)
    print("worst phase error 2^%.1f of half-slot 2^%d" % (math.log2(max(worst, 1)), log_delta - 1))
    assert worst < 1 << (log_delta - 3)                  # a quarter of the half-slot


def test_c_program_tfhe_lut(tmp_path, fhe):
    """examples/tfhe_lut_demo.c: three encrypted bytes through a 256-entry byte -> byte table in one call, from plain C against
    include/fhe_ring.h alone"""
    import os
    import subprocess
    from conftest import ROOT
    lib_dir = os.path.dirname(fhe.lib_path())
    exe = tmp_path / "tfhe_lut_demo"
    cmd = ["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "tfhe_lut_demo.c"), "-o", str(exe),
           "-L", lib_dir, "-lfhe_ring", "-Wl,--allow-shlib-undefined", "-Wl,-rpath," + lib_dir, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tfhe_lut_demo ok" in r.stdout, r.stdout + r.stderr
