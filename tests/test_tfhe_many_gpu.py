"""GPU tests of the many-LUT bootstrap (several tables from one blind rotation): fhe_tfhe_mod_switch_many against numpy and the existing
entry, fhe_tglwe_sample_extract_many against fhe_tglwe_sample_extract per index, fhe_tfhe_bootstrap_many in every key form against the
composition of the existing entries and of oracle.pyref, circuits with many-LUT nodes against the node-by-node route, and the 8-bit
adder with one many-LUT node per block at decode level with device-made keys."""
import os
import subprocess

import numpy as np
import pytest

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


def dev32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def r64(rng, *shape):
    return rng.integers(0, 1 << 63, size=shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)


# the four key forms of tests/test_tfhe_circuit_gpu.py: (7, 3) at n = 1024: three key pieces through f64 transforms; (10, 2): three 30-bit
# primes, digits not packed; (7, 2) at n = 2048: three 30-bit primes with packed digits; (23, 1): two 60-bit primes
KEY_FORMS = [(1024, 7, 3, 10), (1024, 10, 2, 8), (2048, 7, 2, 6), (1024, 23, 1, 7)]


def np_mod_switch(v, big_n):
    """bootstrapping.rs:99-104: rounding_shr(v, 64 - log2(2 big_n)) with its wrapping add"""
    bits = np.uint64(64 - big_n.bit_length())
    with np.errstate(over="ignore"):
        return (v + (np.uint64(1) << (bits - np.uint64(1)))) >> bits


@pytest.mark.parametrize("big_n", [256, 2048])
@pytest.mark.parametrize("nu", [0, 1, 2, 4])
def test_mod_switch_many_vs_numpy(fhe, torch_cuda, big_n, nu):
    """0, 1, 2^64 - 1, every rounding midpoint +- 1 of a few slots (first, second, middle, last) and 1000 random words: the reference's
    mod_switch for big_n >> nu, shifted left by nu; nu = 0: the existing entry; host and device memory"""
    rng = np.random.Generator(np.random.PCG64(5000 + big_n + nu))
    width = 1 << (64 - (big_n >> nu).bit_length())          # of one slot of 2 (big_n >> nu) positions
    slots = 2 * (big_n >> nu)
    edge = [s * width + width // 2 + e for s in (0, 1, slots // 2 - 1, slots // 2, slots - 2, slots - 1) for e in (-1, 0, 1)]
    v = np.concatenate([U([0, 1, M64 - 1] + [x % M64 for x in edge]), r64(rng, 1000)])
    want = np_mod_switch(v, big_n >> nu) << np.uint64(nu)
    assert int(want.max()) < 2 * big_n and np.all(want % np.uint64(1 << nu) == 0)
    got = fhe.TorusContext.mod_switch_many(dev(torch_cuda, v), big_n, nu)
    assert np.array_equal(host(got), want)
    assert np.array_equal(fhe.TorusContext.mod_switch_many(v, big_n, nu), want)
    if nu == 0:
        assert np.array_equal(host(fhe.TorusContext.mod_switch(dev(torch_cuda, v), big_n)), want)
    for bad in (5, -1):
        with pytest.raises(fhe.FheError) as e:
            fhe.TorusContext.mod_switch_many(v, big_n, bad)
        assert e.value.code == 1


@pytest.mark.parametrize("batch", [3, 70])
@pytest.mark.parametrize("nu", [0, 1, 3])
@pytest.mark.parametrize("n", [256, 2048])
def test_sample_extract_many_vs_per_index(fhe, torch_cuda, n, nu, batch):
    """out [batch][2^nu][n]: row (c, i) bit-equal to fhe_tglwe_sample_extract with index = i; batch 70: more than one workgroup's waves;
    device and host memory, and a device operand that is 8 but not 16 bytes aligned"""
    rng = np.random.Generator(np.random.PCG64(5100 + n + nu + batch))
    a, b = r64(rng, batch, n), r64(rng, batch, n)
    da, db = dev(torch_cuda, a), dev(torch_cuda, b)
    ga, gb = fhe.tglwe_sample_extract_many(da, db, n, nu)
    ga, gb = host(ga).reshape(batch, 1 << nu, n), host(gb).reshape(batch, 1 << nu)
    for i in range(1 << nu):
        ea, eb = fhe.tglwe_sample_extract(da, db, n, i)
        assert np.array_equal(ga[:, i], host(ea).reshape(batch, n)) and np.array_equal(gb[:, i], host(eb)), i
    assert np.array_equal(gb, b[:, :1 << nu])
    ha, hb = fhe.tglwe_sample_extract_many(a, b, n, nu)
    assert np.array_equal(ha, ga) and np.array_equal(hb, gb)
    if batch == 3:
        odd = dev(torch_cuda, np.concatenate([U([0]), a.ravel()]))[1:]
        assert odd.data_ptr() % 16 == 8
        oa, ob = fhe.tglwe_sample_extract_many(odd, db, n, nu)
        assert np.array_equal(host(oa).reshape(ga.shape), ga) and np.array_equal(host(ob).reshape(gb.shape), gb)


@pytest.mark.parametrize("n,log_b,d,n_lwe", KEY_FORMS)
def test_bootstrap_many_equals_the_composition(fhe, torch_cuda, n, log_b, d, n_lwe):
    """batch 5, nu in {1, 2}, two interleaved tables assigned unevenly, random key rows: bit-equal to fhe_tfhe_mod_switch_many ->
    fhe_tfhe_blind_rotate_tables -> fhe_tglwe_sample_extract(i) per i -> fhe_tlwe_key_switch; fft64 device against device; host memory
    gives the bits of device memory"""
    batch, ks_log_b, ks_d = 5, 4, 5
    rng = np.random.Generator(np.random.PCG64(5200 + log_b + n))
    bra, brb, tables = r64(rng, n_lwe, 2 * d, n), r64(rng, n_lwe, 2 * d, n), r64(rng, 2, n)
    a_raw, b_raw = r64(rng, batch, n_lwe), r64(rng, batch)
    ksa, ksb = r64(rng, n * ks_d, n_lwe), r64(rng, n * ks_d)
    table_of = np.array([1, 0, 1, 1, 1], dtype=np.uint32)
    t = fhe.TorusContext()
    D = lambda x: dev(torch_cuda, x)  # noqa: E731
    dksa, dksb, dtab, da, db, dtof = D(ksa), D(ksb), D(tables), D(a_raw), D(b_raw), dev32(torch_cuda, table_of)
    for nu in (1, 2):
        at, bt = fhe.TorusContext.mod_switch_many(da, n, nu), fhe.TorusContext.mod_switch_many(db, n, nu)
        for fft64 in (False, True):
            key = fhe.TggswKey(t, log_b, d, D(bra), D(brb), n, fft64=fft64)
            ga, gb = key.bootstrap_many(ks_log_b, ks_d, dksa, dksb, dtab, dtof, nu, da, db)
            assert tuple(ga.shape) == (batch, 1 << nu, n_lwe) and tuple(gb.shape) == (batch, 1 << nu)
            ra, rb = key.blind_rotate_tables(at, bt, dtab, dtof)
            for i in range(1 << nu):
                ea, eb = fhe.tglwe_sample_extract(ra, rb, n, i)
                ka, kb = fhe.tlwe_key_switch(ks_log_b, ks_d, dksa, dksb, ea, eb, n, n_lwe)
                assert torch_cuda.equal(ga[:, i], ka.reshape(batch, n_lwe)) and torch_cuda.equal(gb[:, i], kb.reshape(batch)), (nu, fft64, i)
            if not fft64:
                ha, hb = key.bootstrap_many(ks_log_b, ks_d, ksa, ksb, tables, table_of, nu, a_raw, b_raw)
                assert np.array_equal(ha, host(ga).reshape(ha.shape)) and np.array_equal(hb, host(gb).reshape(hb.shape)), nu
    key = fhe.TggswKey(t, log_b, d, D(bra), D(brb), n)
    with pytest.raises(fhe.FheError) as e:
        key.bootstrap_many(ks_log_b, ks_d, ksa, ksb, tables, table_of, 5, a_raw, b_raw)
    assert e.value.code == 1
    bad = table_of.copy()
    bad[batch - 1] = 2
    with pytest.raises(fhe.FheError) as e:
        key.bootstrap_many(ks_log_b, ks_d, ksa, ksb, tables, bad, 1, a_raw, b_raw)
    assert e.value.code == 1


@pytest.mark.parametrize("n,log_b,d,n_lwe", KEY_FORMS)
def test_bootstrap_many_nu0_equals_bootstrap_tables(fhe, torch_cuda, n, log_b, d, n_lwe):
    """log_funcs = 0 is the one-table bootstrap: batch 5, two tables assigned unevenly, random key rows: fhe_tfhe_bootstrap_many bit-equal
    to fhe_tfhe_bootstrap_tables (one composition serves both entries); exact and fft64 on device memory, host memory for the first
    key form"""
    batch, ks_log_b, ks_d = 5, 4, 5
    rng = np.random.Generator(np.random.PCG64(5250 + log_b + n))
    bra, brb, tables = r64(rng, n_lwe, 2 * d, n), r64(rng, n_lwe, 2 * d, n), r64(rng, 2, n)
    a_raw, b_raw = r64(rng, batch, n_lwe), r64(rng, batch)
    ksa, ksb = r64(rng, n * ks_d, n_lwe), r64(rng, n * ks_d)
    table_of = np.array([0, 1, 1, 0, 1], dtype=np.uint32)
    t = fhe.TorusContext()
    D = lambda x: dev(torch_cuda, x)  # noqa: E731
    dksa, dksb, dtab, da, db, dtof = D(ksa), D(ksb), D(tables), D(a_raw), D(b_raw), dev32(torch_cuda, table_of)
    for fft64 in (False, True):
        key = fhe.TggswKey(t, log_b, d, D(bra), D(brb), n, fft64=fft64)
        ga, gb = key.bootstrap_many(ks_log_b, ks_d, dksa, dksb, dtab, dtof, 0, da, db)
        assert tuple(ga.shape) == (batch, 1, n_lwe) and tuple(gb.shape) == (batch, 1)
        wa, wb = key.bootstrap_tables(ks_log_b, ks_d, dksa, dksb, dtab, dtof, da, db)
        assert torch_cuda.equal(ga.reshape(batch, n_lwe), wa.reshape(batch, n_lwe)) and torch_cuda.equal(gb.reshape(batch), wb.reshape(batch)), fft64
        if not fft64 and (n, log_b, d, n_lwe) == KEY_FORMS[0]:
            ha, hb = key.bootstrap_many(ks_log_b, ks_d, ksa, ksb, tables, table_of, 0, a_raw, b_raw)
            assert np.array_equal(ha.reshape(batch, n_lwe), host(wa).reshape(batch, n_lwe)) and np.array_equal(hb.reshape(batch), host(wb).reshape(batch))


def test_bootstrap_many_equals_pyref_piece_by_piece(fhe, torch_cuda):
    """n = 256, n_lwe = 6, gadget (15, 1): oracle.pyref composed -- tfhe_mod_switch for n >> nu shifted left, tfhe_blind_rotate on the
    ciphertext's table, tglwe_sample_extract(i), tlwe_key_switch"""
    from oracle import pyref as P
    n, log_b, d, n_lwe, batch, ks_log_b, ks_d = 256, 15, 1, 6, 3, 4, 5
    rng = np.random.Generator(np.random.PCG64(5300))
    bra, brb, tables = r64(rng, n_lwe, 2 * d, n), r64(rng, n_lwe, 2 * d, n), r64(rng, 2, n)
    a_raw, b_raw = r64(rng, batch, n_lwe), r64(rng, batch)
    ksa, ksb = r64(rng, n * ks_d, n_lwe), r64(rng, n * ks_d)
    table_of = np.array([1, 0, 1], dtype=np.uint32)
    D = lambda x: dev(torch_cuda, x)  # noqa: E731
    key = fhe.TggswKey(fhe.TorusContext(), log_b, d, D(bra), D(brb), n)
    dec, ksdec = P.TorusDecomposor(log_b, d), P.TorusDecomposor(ks_log_b, ks_d)
    brk = [([[int(x) for x in r] for r in bra[i]], [[int(x) for x in r] for r in brb[i]]) for i in range(n_lwe)]
    pka, pkb = [[int(x) for x in r] for r in ksa], [int(x) for x in ksb]
    for nu in (1, 2):
        ga, gb = key.bootstrap_many(ks_log_b, ks_d, D(ksa), D(ksb), D(tables), dev32(torch_cuda, table_of), nu, D(a_raw), D(b_raw))
        ga, gb = host(ga).reshape(batch, 1 << nu, n_lwe), host(gb).reshape(batch, 1 << nu)
        for c in range(batch):
            at = [x << nu for x in P.tfhe_mod_switch([int(x) for x in a_raw[c]], n >> nu)]
            bt = P.tfhe_mod_switch([int(b_raw[c])], n >> nu)[0] << nu
            acc = P.tfhe_blind_rotate(dec, brk, [int(x) for x in tables[table_of[c]]], at, bt)
            for i in range(1 << nu):
                ea, eb = P.tglwe_sample_extract(acc[0], acc[1], i)
                xa, xb = P.tlwe_key_switch(ksdec, pka, pkb, ea, eb)
                assert [int(x) for x in ga[c, i]] == xa and int(gb[c, i]) == xb, (nu, c, i)


def many_netlist(T):
    """3 inputs, 5 nodes over 3 levels: a v = 1 node (n0) feeding a v = 2 node (n1, from outputs 0 and 1) and a v = 0 node (n2, from
    output 1: fan-out from output 1) of the same level, the many-LUT node first; dead outputs (n1's outputs 1 and 2: only the dead
    node reads output 1), one dead many-LUT node (n3), weights -1 and 4, non-zero constants; outputs: n1's output 3, an input, n2,
    n1's output 0, n4 (a v = 0 node on n1's output 3 and n2)"""
    b = T.Builder()
    i0, i1, i2 = b.input(), b.input(), b.input()
    f0, f1, f2, f3 = (lambda v: v), (lambda v: 2 * v + 1), (lambda v: v % 3), (lambda v: v >> 1)
    n0 = b.node_many([(i0, 1), (i1, 1)], (f0, f1))
    n1 = b.node_many([(n0[0], 1), (n0[1], -1), (i2, 1)], (f0, f1, f2, f3), constant=31)
    n2 = b.node([(n0[1], 4), (i2, -1)], f2, constant=5)
    b.node_many([(n1[1], 1), (i0, 1)], (f1, f0))
    n4 = b.node([(n1[3], 1), (n2, -1)], f1)
    return b, [n1[3], i1, n2, n1[0], n4]


@pytest.mark.parametrize("n,log_b,d,n_lwe,batch", [(256, 15, 1, 6, 3), (1024, 7, 3, 6, 5)])
def test_many_circuit_equals_node_by_node(fhe, torch_cuda, n, log_b, d, n_lwe, batch):
    """fhe_tfhe_circuit_run on a handle of fhe_tfhe_circuit_create_many bit-equal to fhe_tlwe_lincomb + fhe_tfhe_bootstrap /
    fhe_tfhe_bootstrap_many per node, in the exact key form and in fft64, and to the same call with every operand in host memory"""
    T = fhe.tfhe_circuit
    ks_log_b, ks_d, log_p, padding = 4, 5, 4, 1
    b, outputs = many_netlist(T)
    c = b.compile(outputs, log_p, padding, n)
    assert c.many and c.info() == {"levels": 3, "live_nodes": 4, "max_width": 2} and c.levels() == [1, 2, 2, 0, 3]
    assert c.info_many() == {"live_outputs": 6, "max_rows": 3}
    rng = np.random.Generator(np.random.PCG64(5400 + n))
    bra, brb, tables = r64(rng, n_lwe, 2 * d, n), r64(rng, n_lwe, 2 * d, n), r64(rng, c.n_tables, n)
    ksa, ksb = r64(rng, n * ks_d, n_lwe), r64(rng, n * ks_d)
    in_a, in_b = r64(rng, 3, batch, n_lwe), r64(rng, 3, batch)
    t = fhe.TorusContext()
    D = lambda x: dev(torch_cuda, x)  # noqa: E731
    for fft64 in (False, True):
        key = fhe.TggswKey(t, log_b, d, D(bra), D(brb), n, fft64=fft64)
        oa, ob = c.run(key, ks_log_b, ks_d, D(ksa), D(ksb), (D(in_a), D(in_b)), batch, tables=D(tables))
        na, nb = c.run_nodes(key, ks_log_b, ks_d, D(ksa), D(ksb), (D(in_a), D(in_b)), batch, tables=D(tables))
        assert torch_cuda.equal(oa, na.reshape(oa.shape)) and torch_cuda.equal(ob, nb.reshape(ob.shape)), fft64
        oa, ob = host(oa).reshape(5, batch, n_lwe), host(ob).reshape(5, batch)
        assert np.array_equal(oa[1], in_a[1]) and np.array_equal(ob[1], in_b[1])      # the output that names an input
        if not fft64:
            ha, hb = c.run(key, ks_log_b, ks_d, ksa, ksb, (in_a, in_b), batch, tables=tables)
            assert np.array_equal(ha, oa) and np.array_equal(hb, ob)


def test_nu0_netlist_through_either_create(fhe, torch_cuda):
    """a netlist without many-LUT nodes: the handle of fhe_tfhe_circuit_create_many gives the bits of the handle of
    fhe_tfhe_circuit_create"""
    import ctypes as C
    T = fhe.tfhe_circuit
    n, log_b, d, n_lwe, batch, ks_log_b, ks_d = 256, 15, 1, 6, 3, 4, 5
    b = T.Builder()
    i0, i1, i2 = b.input(), b.input(), b.input()
    n0 = b.node([(i0, 1), (i1, 1)], lambda v: v)
    n1 = b.node([(i1, 4), (i2, -1)], lambda v: 2 * v + 1, constant=5)
    n2 = b.node([(n0, 1), (n1, -1)], lambda v: v % 3)
    b.node([(n1, 1), (n0, 1)], lambda v: v)
    outputs = [n2, i1, n0]
    c = b.compile(outputs, 4, 1, n)
    assert not c.many
    # the same arrays through the other create
    flat = [(b._ref(w), k) for terms, _, _ in b.nodes for w, k in terms]
    tarr = (T._Term * len(flat))()
    for i, (w, k) in enumerate(flat):
        tarr[i].wire, tarr[i].weight = w, k
    narr = (T._Node * len(b.nodes))()
    first = 0
    for i, (terms, table, constant) in enumerate(b.nodes):
        narr[i].first_term, narr[i].n_terms, narr[i].table, narr[i].constant = first, len(terms), table, (constant << 59) % M64
        first += len(terms)
    oarr = (C.c_uint32 * 3)(*[b._ref(w) for w in outputs])
    h = C.c_void_p()
    fhe._lib.check(fhe.lib().fhe_tfhe_circuit_create_many(narr, len(b.nodes), tarr, len(flat), 3, c.n_tables, oarr, 3, C.byref(h)), "create_many")
    try:
        rng = np.random.Generator(np.random.PCG64(5500))
        bra, brb, tables = r64(rng, n_lwe, 2 * d, n), r64(rng, n_lwe, 2 * d, n), r64(rng, c.n_tables, n)
        ksa, ksb = r64(rng, n * ks_d, n_lwe), r64(rng, n * ks_d)
        in_a, in_b = r64(rng, 3, batch, n_lwe), r64(rng, 3, batch)
        D = lambda x: dev(torch_cuda, x)  # noqa: E731
        key = fhe.TggswKey(fhe.TorusContext(), log_b, d, D(bra), D(brb), n)
        oa, ob = c.run(key, ks_log_b, ks_d, D(ksa), D(ksb), (D(in_a), D(in_b)), batch, tables=D(tables))
        ma, mb = T.run_circuit(h, 3, 3, D(tables), key, ks_log_b, ks_d, D(ksa), D(ksb), (D(in_a), D(in_b)), batch)
        assert torch_cuda.equal(oa, ma) and torch_cuda.equal(ob, mb)
    finally:
        fhe.lib().fhe_tfhe_circuit_destroy(h)


def test_many_adder_decodes_with_device_made_keys(fhe, torch_cuda):
    """radix_add(4, 2, 2, many=True) at decode level: n = 1024, n_lwe = 12, gadget (7, 3), key switch (4, 5), log_p 4, padding 1; keys
    from fhe_tggsw_encrypt and fhe_tlwe_ksk_gen at the reference's two standard deviations (bootstrapping.rs:144-148).  32 random byte
    pairs plus (255, 255), (0, 0), (255, 1); every block decrypts (tlwe.rs:134-142) to the plain model's value.  Margin by
    construction: the worst-case mod-switch drift at v = 1 is 2 (n_lwe + 1) / 2 = 13 of 2n = 2048 positions against a half-slot of
    n / 2p = 32."""
    from oracle import pyref as P
    T = fhe.tfhe_circuit
    n, n_lwe, log_b, d, ks_log_b, ks_d, log_p, padding = 1024, 12, 7, 3, 4, 5, 4, 1
    sd_lwe, sd_glwe = 1.339775301998614e-7, 2.845267479601915e-15
    log_delta = 64 - (log_p + padding)
    like = dev(torch_cuda, U([0]))
    t = fhe.TorusContext()
    z, s = fhe.sample_binary(910, 0, like, n_lwe), fhe.sample_binary(910, 1, like, n)
    zh = [int(x) for x in host(z)]
    pt = np.zeros((n_lwe, n), dtype=np.uint64)
    pt[:, 0] = host(z)                                            # Rt::constant(z_i) (bootstrapping.rs:66-67)
    ra, rb = fhe.tggsw_encrypt(t, log_b, d, s, dev(torch_cuda, pt), n, sd_glwe, 911, 0)
    key = fhe.TggswKey(t, log_b, d, ra, rb, n)
    ksa, ksb = fhe.tlwe_ksk_gen(ks_log_b, ks_d, z, s, sd_lwe, 912, 0)
    rng = np.random.Generator(np.random.PCG64(5600))
    xs = np.concatenate([rng.integers(0, 256, size=32), [255, 0, 255]])
    ys = np.concatenate([rng.integers(0, 256, size=32), [255, 0, 1]])
    batch = len(xs)
    blocks = [(xs >> (2 * i)) & 3 for i in range(4)] + [(ys >> (2 * i)) & 3 for i in range(4)]   # [8][batch], x first
    msgs = U([(int(v) << log_delta) % M64 for row in blocks for v in row])
    ca, cb = fhe.tlwe_sk_encrypt(z, dev(torch_cuda, msgs), n_lwe, 8 * batch, sd_lwe, 913, 0)
    b, _, _, outs = T.radix_add(4, 2, 2, many=True)
    add = b.compile(outs, log_p, padding, n)
    assert add.info()["live_nodes"] == 4 and add.info()["levels"] == 4
    oa, ob = add.run(key, ks_log_b, ks_d, ksa, ksb, (ca, cb), batch)
    oa, ob = host(oa).reshape(4, batch, n_lwe), host(ob).reshape(4, batch)
    got = [[((P.tlwe_phase(zh, [int(v) for v in oa[o][i]], int(ob[o][i])) + (1 << (log_delta - 1))) % M64) >> log_delta for i in range(batch)]
           for o in range(4)]
    want = b.evaluate(blocks, log_p, padding, outs)
    assert [list(map(int, w)) for w in want] == got
    assert [sum(got[i][j] << (2 * i) for i in range(4)) for j in range(batch)] == [int(v) for v in (xs + ys) & 255]


def test_c_program_tfhe_many(tmp_path, fhe):
    """examples/tfhe_many_demo.c: the two-byte adder through many-LUT nodes from plain C, decrypting in the program"""
    from conftest import ROOT
    lib_dir = os.path.dirname(fhe.lib_path())
    exe = tmp_path / "tfhe_many_demo"
    cmd = ["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "tfhe_many_demo.c"), "-o", str(exe),
           "-L", lib_dir, "-lfhe_ring", "-Wl,--allow-shlib-undefined", "-Wl,-rpath," + lib_dir, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tfhe_many_demo ok" in r.stdout, r.stdout + r.stderr
