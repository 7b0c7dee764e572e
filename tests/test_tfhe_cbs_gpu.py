"""GPU tests of the circuit bootstrap (k = 1): fhe_tlwe_pfks bit-exact against the model over both digit routes, every tile size, the
row-split and the plain route; fhe_tlwe_pfksk_gen row by row; fhe_tfhe_circuit_bootstrap against the public entries chained and the
model in every key form; the noise-free exactness bound; and a 256-entry CMUX-tree look-up at decode level with device-made keys."""
import math

import numpy as np
import pytest

import keygen_checks as K
import tfhe_cbs_model as M

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


def edge_words(log_b, d):
    """0, 2^63, 2^63 - 1, 2^64 - 1, and values whose digits are all +2^(log_b - 1) resp. -2^(log_b - 1) (a carry through every level)"""
    rb, half = 64 - log_b * d, 1 << (log_b - 1)
    up = sum(half << (rb + j * log_b) for j in range(d)) % M64
    return [0, 1 << 63, (1 << 63) - 1, M64 - 1, up, (-up) % M64, (up + (1 << rb) // 2 - (1 if rb else 0)) % M64]


def pfks_inputs(rng, log_b, d, n_in, n, n_funcs, batch):
    key = r64(rng, d * (n_in + 1), n_funcs, 2, n)
    key[:, :, :, 0] = np.uint64(M64 - 1)                  # whole columns of 2^64 - 1
    key[:, n_funcs - 1, 1, n - 1] = np.uint64(M64 - 1)
    ct_a, ct_b = r64(rng, batch, n_in), r64(rng, batch)
    e = edge_words(log_b, d)
    flat = ct_a.reshape(-1)
    flat[:min(len(e), flat.size)] = U(e)[:flat.size]      # the first ciphertext(s) start with the edge words
    ct_b[0] = np.uint64(e[4])
    ct_b[batch - 1] = np.uint64(e[5])
    return key, ct_a, ct_b


@pytest.mark.parametrize("log_b,d", [(7, 3), (4, 8), (8, 4), (16, 2)])
@pytest.mark.parametrize("n_in,n_funcs,group,batch", [(5, 1, 1, 1), (5, 2, 3, 3), (5, 3, 1, 18), (5, 2, 3, 69), (256, 2, 1, 3), (256, 3, 3, 18),
                                                      (256, 1, 3, 69), (256, 2, 1, 1)])
def test_pfks_bit_exact_vs_model(fhe, torch_cuda, log_b, d, n_in, n_funcs, group, batch):
    """n = 256; n_in + 1 = 6 and 257 rows; batch below one tile (1, 3), across a tile edge (18) and with a ragged last tile (69); byte
    digits (log_b <= 7) and word digits; the library's rule, one block per tile (PFKS_SPLIT = 1) and three row chunks (3) give the
    model's bits; host memory gives the bits of device memory"""
    n = 256
    rng = np.random.Generator(np.random.PCG64(6100 + 1000 * log_b + n_in + 7 * batch + n_funcs))
    key, ct_a, ct_b = pfks_inputs(rng, log_b, d, n_in, n, n_funcs, batch)
    want_a, want_b = M.pfks(log_b, d, key, n_funcs, ct_a, ct_b, n_in, n, group)
    C = fhe.tfhe_cbs
    dk, da, db = dev(torch_cuda, key), dev(torch_cuda, ct_a), dev(torch_cuda, ct_b)
    try:
        for split in (0, 1, 3):
            fhe.set_option("PFKS_SPLIT", split)
            ga, gb = C.pfks(log_b, d, dk, n_funcs, da, db, n_in, n, group)
            assert np.array_equal(host(ga), want_a) and np.array_equal(host(gb), want_b), split
    finally:
        fhe.set_option("PFKS_SPLIT", 0)
    ha, hb = C.pfks(log_b, d, key, n_funcs, ct_a, ct_b, n_in, n, group)
    assert np.array_equal(ha, want_a) and np.array_equal(hb, want_b)


def test_pfks_unaligned_operands_and_rejections(fhe, torch_cuda):
    """a key that is 8 but not 16 bytes aligned takes the one-column route: the same bits; outputs equal to inputs are rejected"""
    log_b, d, n_in, n, n_funcs, batch = 7, 3, 5, 256, 2, 18
    rng = np.random.Generator(np.random.PCG64(6150))
    key, ct_a, ct_b = pfks_inputs(rng, log_b, d, n_in, n, n_funcs, batch)
    want_a, want_b = M.pfks(log_b, d, key, n_funcs, ct_a, ct_b, n_in, n)
    odd = dev(torch_cuda, np.concatenate([U([0]), key.ravel()]))[1:]
    assert odd.data_ptr() % 16 == 8
    da, db = dev(torch_cuda, ct_a), dev(torch_cuda, ct_b)
    ga, gb = fhe.tfhe_cbs.pfks(log_b, d, odd, n_funcs, da, db, n_in, n)
    assert np.array_equal(host(ga), want_a) and np.array_equal(host(gb), want_b)
    try:  # chunks of 2 coefficients: one block walks three chunks (PFKS_SPLIT = 1), or two blocks share them
        fhe.set_option("PFKS_CHUNK", 2)
        for split in (1, 2):
            fhe.set_option("PFKS_SPLIT", split)
            ca, cb = fhe.tfhe_cbs.pfks(log_b, d, dev(torch_cuda, key), n_funcs, da, db, n_in, n)
            assert np.array_equal(host(ca), want_a) and np.array_equal(host(cb), want_b), split
    finally:
        fhe.set_option("PFKS_CHUNK", 0)
        fhe.set_option("PFKS_SPLIT", 0)
    from learn_fhe_amd.ring import _buf
    p, _, mem, st = _buf(ga)
    assert fhe.lib().fhe_tlwe_pfks(log_b, d, _buf(odd)[0], n_funcs, p, _buf(db)[0], n_in, n, 1, p, _buf(gb)[0], batch, mem, st) == 1


def test_pfks_widest_strip(fhe, torch_cuda):
    """n = n_in = 2048, two functions, batch 17 (one full tile and a tile of one), gadget (7, 1): 2049 rows of 8192 words"""
    log_b, d, n_in, n, n_funcs, batch = 7, 1, 2048, 2048, 2, 17
    rng = np.random.Generator(np.random.PCG64(6200))
    key, ct_a, ct_b = pfks_inputs(rng, log_b, d, n_in, n, n_funcs, batch)
    want_a, want_b = M.pfks(log_b, d, key, n_funcs, ct_a, ct_b, n_in, n)
    ga, gb = fhe.tfhe_cbs.pfks(log_b, d, dev(torch_cuda, key), n_funcs, dev(torch_cuda, ct_a), dev(torch_cuda, ct_b), n_in, n)
    assert np.array_equal(host(ga), want_a) and np.array_equal(host(gb), want_b)


def key_rows(key, sk_out):
    """pfksk [rows][n_funcs][2][n] -> phases b - a sk_out, [rows n_funcs][n] uint64"""
    rows, n_funcs, _, n = key.shape
    flat = key.reshape(rows * n_funcs, 2, n)
    return np.stack([M.tglwe_phase(sk_out, flat[r, 0], flat[r, 1]) for r in range(rows * n_funcs)])


def test_pfksk_gen_rows(fhe, torch_cuda):
    """every row decrypted with the secret keys: phase - w_i g_j F_u is exactly 0 at std_dev = 0 and follows the sampler's law at a
    positive one (tests/keygen_checks.py); the masks differ from fhe_tglwe_sk_encrypt's on the same (rng, stream_id)"""
    log_b, d, n_in, n = 6, 3, 9, 256
    like = dev(torch_cuda, U([0]))
    t = fhe.TorusContext()
    sk_in, sk_out = fhe.sample_binary(6300, 0, like, n_in), fhe.sample_binary(6300, 1, like, n)
    C = fhe.tfhe_cbs
    funcs = host(C.pfksk_funcs(sk_out)).reshape(2, n)
    assert np.array_equal(funcs[0], np.uint64(0) - host(sk_out)) and funcs[1, 0] == 1 and not funcs[1, 1:].any()
    three = np.concatenate([funcs, r64(np.random.Generator(np.random.PCG64(6301)), 1, n)])
    plain = M.pfksk_plain(log_b, d, host(sk_in), three).reshape(-1, n)
    key0 = host(C.pfksk_gen(t, log_b, d, sk_in, sk_out, dev(torch_cuda, three), 0.0, 6302, 5)).reshape(d * (n_in + 1), 3, 2, n)
    assert np.array_equal(key_rows(key0, host(sk_out)), plain)
    std_dev = 2.0 ** -40                                            # sigma = 2^24 torus steps
    key1 = host(C.pfksk_gen(t, log_b, d, sk_in, sk_out, dev(torch_cuda, three), std_dev, 6302, 5)).reshape(d * (n_in + 1), 3, 2, n)
    res = (key_rows(key1, host(sk_out)) - plain).view(np.int64)
    K.rows_independent(res)
    dist = K.ks_normal(res.astype(np.float64).ravel(), std_dev * 2.0 ** 64)
    assert K.ks_ok(dist, res.size), dist
    assert np.array_equal(key1[:, :, 0], key0[:, :, 0])              # the masks depend on (rng, stream_id, purpose) alone
    ea, _ = fhe.tglwe_sk_encrypt(t, sk_out, None, n, key0.shape[0] * 3, 0.0, 6302, 5)
    assert not np.array_equal(host(ea).reshape(-1, n), key0[:, :, 0].reshape(-1, n))
    assert not np.intersect1d(host(ea).ravel()[:4096], key0[:, :, 0].ravel()[:4096]).size
    ha = C.pfksk_gen(t, log_b, d, host(sk_in), host(sk_out), three, 0.0, 6302, 5)
    assert np.array_equal(ha.reshape(key0.shape), key0)             # host memory: the same key


# exact key forms fhe_tggsw_prepare can be steered to: (23, 1) at n = 1024: two 60-bit primes; (7, 3): three key pieces through f64
# transforms; (10, 2), and (15, 1) at n = 256 (bound 2^87): three 30-bit primes.  FORM_OF: what fhe_tggsw_key_form must report for each
KEY_FORMS = [(256, 15, 1), (256, 7, 3), (256, 10, 2), (1024, 7, 3), (1024, 10, 2), (1024, 23, 1)]
FORM_OF = dict(zip(KEY_FORMS, ["30", "x3", "30", "x3", "30", "60"]))


@pytest.mark.parametrize("n,log_b,d", KEY_FORMS)
def test_circuit_bootstrap_equals_the_chain_and_the_model(fhe, torch_cuda, n, log_b, d):
    """n_lwe = 8, random key rows, cb gadgets (8, 2), (6, 3), (4, 4) (nu = 1, 2, 2; cb_d = 3 leaves a dead table), batch 1 and 5:
    the fused call, the four public entries chained and the model give the same bits; fft64: fused against chained on the device;
    host memory gives the bits of device memory"""
    n_lwe, pf_log_b, pf_d = 8, 9, 2
    rng = np.random.Generator(np.random.PCG64(6400 + n + log_b))
    bra, brb = r64(rng, n_lwe, 2 * d, n), r64(rng, n_lwe, 2 * d, n)
    pfksk = r64(rng, pf_d * (n + 1), 2, 2, n)
    t, C = fhe.TorusContext(), fhe.tfhe_cbs
    D = lambda x: dev(torch_cuda, x)  # noqa: E731
    dk = D(pfksk)
    keys = {f: fhe.TggswKey(t, log_b, d, D(bra), D(brb), n, fft64=f) for f in (False, True)}
    assert (keys[False].form, keys[True].form) == (FORM_OF[(n, log_b, d)], "fft64")
    for cb_log_b, cb_d in [(8, 2), (6, 3), (4, 4)]:
        table = D(C.cbs_table(cb_log_b, cb_d, n))
        for batch in (1, 5):
            a, b = r64(rng, batch, n_lwe), r64(rng, batch)
            for fft64 in (False, True):
                ga, gb = C.circuit_bootstrap(keys[fft64], cb_log_b, cb_d, pf_log_b, pf_d, dk, D(a), D(b))
                sa, sb = C.circuit_bootstrap_steps(keys[fft64], cb_log_b, cb_d, pf_log_b, pf_d, dk, D(a), D(b), table)
                assert tuple(ga.shape) == (batch, 2 * cb_d, n)
                assert torch_cuda.equal(ga, sa) and torch_cuda.equal(gb, sb), (cb_d, batch, fft64)
                if not fft64:
                    got = (host(ga), host(gb))
            if batch == 1 or (n == 256 and cb_d == 3):
                ma, mb = M.circuit_bootstrap(log_b, d, bra, brb, cb_log_b, cb_d, pf_log_b, pf_d, pfksk, a, b, fast=True)
                assert np.array_equal(got[0], ma) and np.array_equal(got[1], mb), (cb_d, batch)
            if batch == 5 and cb_d == 3:
                ha, hb = C.circuit_bootstrap(keys[False], cb_log_b, cb_d, pf_log_b, pf_d, pfksk, a, b)
                assert np.array_equal(ha, got[0]) and np.array_equal(hb, got[1])


def test_circuit_bootstrap_model_through_pyref(fhe, torch_cuda):
    """n = 256, n_lwe = 8, key gadget (15, 1), cb (6, 3), one ciphertext: the blind rotation of the model through oracle.pyref itself"""
    n, log_b, d, n_lwe, cb_log_b, cb_d, pf_log_b, pf_d = 256, 15, 1, 8, 6, 3, 9, 2
    rng = np.random.Generator(np.random.PCG64(6450))
    bra, brb, pfksk = r64(rng, n_lwe, 2 * d, n), r64(rng, n_lwe, 2 * d, n), r64(rng, pf_d * (n + 1), 2, 2, n)
    a, b = r64(rng, 1, n_lwe), r64(rng, 1)
    D = lambda x: dev(torch_cuda, x)  # noqa: E731
    key = fhe.TggswKey(fhe.TorusContext(), log_b, d, D(bra), D(brb), n)
    ga, gb = fhe.tfhe_cbs.circuit_bootstrap(key, cb_log_b, cb_d, pf_log_b, pf_d, D(pfksk), D(a), D(b))
    ma, mb = M.circuit_bootstrap(log_b, d, bra, brb, cb_log_b, cb_d, pf_log_b, pf_d, pfksk, a, b)
    assert np.array_equal(host(ga), ma) and np.array_equal(host(gb), mb)


def make_keys(fhe, torch_cuda, n, n_lwe, log_b, d, pf_log_b, pf_d, sd_glwe, seed):
    """device-made keys: z (TLWE), s (TGLWE), bootstrapping key of Rt::constant(z_i) (bootstrapping.rs:66-67), pfksk from S's bits to S"""
    like = dev(torch_cuda, U([0]))
    t = fhe.TorusContext()
    z, s = fhe.sample_binary(seed, 0, like, n_lwe), fhe.sample_binary(seed, 1, like, n)
    pt = np.zeros((n_lwe, n), dtype=np.uint64)
    pt[:, 0] = host(z)
    ra, rb = fhe.tggsw_encrypt(t, log_b, d, s, dev(torch_cuda, pt), n, sd_glwe, seed + 1, 0)
    brk = fhe.TggswKey(t, log_b, d, ra, rb, n)
    pfksk = fhe.tfhe_cbs.pfksk_gen(t, pf_log_b, pf_d, s, s, fhe.tfhe_cbs.pfksk_funcs(s), sd_glwe, seed + 2, 0)
    return t, z, s, brk, pfksk


def test_noise_free_rows_are_exact_up_to_the_rounding_bound(fhe, torch_cuda):
    """every key at std_dev = 0, input phase exactly bit << 62, bootstrapping gadget (16, 4) (64 bits: its digits round nothing away): the
    blind rotation returns g_j bit exactly, so row (u, j) has phase
    F_u bit g_j plus the key switch's rounding alone, per coefficient at most (n_in + 1) 2^(63 - pf_log_b pf_d) |F_u|_1 -- derived,
    not measured"""
    n, n_lwe, log_b, d, cb_log_b, cb_d, pf_log_b, pf_d = 256, 8, 16, 4, 6, 3, 8, 4
    t, z, s, brk, pfksk = make_keys(fhe, torch_cuda, n, n_lwe, log_b, d, pf_log_b, pf_d, 0.0, 6500)
    bits = U([0, 1, 1, 0])
    ca, cb = fhe.tlwe_sk_encrypt(z, dev(torch_cuda, bits << np.uint64(62)), n_lwe, 4, 0.0, 6503, 0)
    ra, rb = fhe.tfhe_cbs.circuit_bootstrap(brk, cb_log_b, cb_d, pf_log_b, pf_d, pfksk, ca, cb)
    ra, rb, sh = host(ra).reshape(4, 2 * cb_d, n), host(rb).reshape(4, 2 * cb_d, n), host(s)
    funcs = host(fhe.tfhe_cbs.pfksk_funcs(s)).reshape(2, n)
    g = M.gadget(cb_log_b, cb_d)
    worst = 0
    for c, bit in enumerate(int(x) for x in bits):
        for u in range(2):
            l1 = int(np.abs(funcs[u].view(np.int64)).sum())
            bound = (n + 1) * (1 << (63 - pf_log_b * pf_d)) * l1
            for j in range(cb_d):
                with np.errstate(over="ignore"):
                    want = funcs[u] * np.uint64((bit * g[j]) % M64)
                    err = (M.tglwe_phase(sh, ra[c, u * cb_d + j], rb[c, u * cb_d + j]) - want).view(np.int64)
                worst = max(worst, int(np.abs(err).max()) / bound)
                assert int(np.abs(err).max()) <= bound, (bit, u, j, int(np.abs(err).max()), bound)
    print("worst rounding / bound = %.3f" % worst)


# decode-level parameters (DESIGN.md 9.3 derives the noise): the mod switch drifts by at most 8 (n_lwe + 1) / 2 = 36 of 2n = 2048
# positions against a quarter ring of 256; after m = 8 CMUX levels the phase error has a standard deviation near 2^47.6 against the
# half-slot 2^54
LUT = dict(n=1024, n_lwe=8, log_b=10, d=4, cb_log_b=4, cb_d=6, pf_log_b=7, pf_d=6, sd_lwe=2.0 ** -30, sd_glwe=2.845267479601915e-15, log_p=8)


def test_lut_tree_decodes_under_noisy_keys(fhe, torch_cuda):
    """the 8 bits of 0x00, 0xFF, 0xA5, 0x3C, 0x81 are circuit-bootstrapped in one call, prepared as 40 selectors, and each byte reads a
    fixed pseudo-random permutation of 0 .. 255 (log_p = 8, one padding bit, coefficient 0) through lut_eval; decrypted under the
    extracted key (tlwe.rs:134-142) the result is the table's entry"""
    from oracle import pyref as P
    p = LUT
    n, n_lwe, m, log_delta = p["n"], p["n_lwe"], 8, 64 - (p["log_p"] + 1)
    t, z, s, brk, pfksk = make_keys(fhe, torch_cuda, n, n_lwe, p["log_b"], p["d"], p["pf_log_b"], p["pf_d"], p["sd_glwe"], 6600)
    table = np.random.Generator(np.random.PCG64(6601)).permutation(256)
    polys = np.zeros((256, n), dtype=np.uint64)
    polys[:, 0] = U([int(v) << log_delta for v in table])
    byts = [0x00, 0xFF, 0xA5, 0x3C, 0x81]
    bits = U([(x >> l) & 1 for x in byts for l in range(m)])
    ca, cb = fhe.tlwe_sk_encrypt(z, dev(torch_cuda, bits << np.uint64(62)), n_lwe, bits.size, p["sd_lwe"], 6603, 0)
    ra, rb = fhe.tfhe_cbs.circuit_bootstrap(brk, p["cb_log_b"], p["cb_d"], p["pf_log_b"], p["pf_d"], pfksk, ca, cb)
    sel = fhe.TggswKey(t, p["cb_log_b"], p["cb_d"], ra, rb, n)
    assert sel.count == len(byts) * m
    sh = [int(x) for x in host(s)]
    dpolys = dev(torch_cuda, polys)
    worst = 0
    for i, x in enumerate(byts):
        oa, ob = fhe.tfhe_cbs.lut_eval(dpolys, sel, i * m, m)
        phase = P.tlwe_phase(sh, [int(v) for v in host(oa).reshape(n)], int(host(ob)[0]))
        want = int(table[x])
        assert fhe.tfhe_cbs.lut_eval_plain(table, [(x >> l) & 1 for l in range(m)]) == want
        assert ((phase + (1 << (log_delta - 1))) % M64) >> log_delta == want, hex(x)
        worst = max(worst, abs(P.t64_to_i64((phase - (want << log_delta)) % M64)))
    print("worst phase error 2^%.1f of half-slot 2^%d" % (math.log2(max(worst, 1)), log_delta - 1))
    assert worst < 1 << (log_delta - 3)                  # a quarter of the half-slot


def test_c_program_tfhe_cbs(tmp_path, fhe):
    """examples/tfhe_cbs_demo.c: address bits circuit-bootstrapped, prepared with count = batch, a 16-entry table read through a CMUX
    tree and decrypted, from plain C against include/fhe_ring.h alone"""
    import os
    import subprocess
    from conftest import ROOT
    lib_dir = os.path.dirname(fhe.lib_path())
    exe = tmp_path / "tfhe_cbs_demo"
    cmd = ["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "tfhe_cbs_demo.c"), "-o", str(exe),
           "-L", lib_dir, "-lfhe_ring", "-Wl,--allow-shlib-undefined", "-Wl,-rpath," + lib_dir, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tfhe_cbs_demo ok" in r.stdout, r.stdout + r.stderr
