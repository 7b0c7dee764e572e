"""GPU tests of the TFHE look-up-table circuits: the blind rotation and the bootstrap with one table per ciphertext
(fhe_tfhe_blind_rotate_tables, fhe_tfhe_bootstrap_tables) in every key form against the exact oracle and against the shared-table entries,
fhe_tlwe_lincomb against numpy, fhe_tfhe_circuit_run against the node-by-node composition of the public entries and of oracle.pyref,
and the 8-bit adder and comparison at decode level with device-made keys (scheme/tfhe/src/bootstrapping.rs:118-165)."""
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


# which form fhe_tggsw_prepare gives a gadget (its rules, include/fhe_ring.h): (7, 3) at n = 1024: three key pieces through f64
# transforms; (10, 2): three 30-bit primes, digits not packed (base > 2^7); (7, 2) at n = 2048: three 30-bit primes with packed digits
# ((7, 4) at n = 256 goes to the f64 pieces, so the packed case is the n = 2048 entry of
# test_packed_digit_blind_rotation_equals_the_unpacked_one's list); (23, 1): two 60-bit primes
KEY_FORMS = [(1024, 7, 3, 10), (1024, 10, 2, 8), (2048, 7, 2, 6), (1024, 23, 1, 7)]


@pytest.mark.parametrize("n,log_b,d,n_lwe", KEY_FORMS)
def test_tables_entries_vs_oracle_and_shared_entry(fhe, cref, torch_cuda, n, log_b, d, n_lwe):
    """batch 7, three tables assigned unevenly (table 1 serves one ciphertext): every ciphertext bit-equal to the oracle's bootstrap
    with its own table and to the shared-table entries called per table; the same in host memory; fft64 mode device against device."""
    batch, ks_log_b, ks_d = 7, 4, 5
    rng = np.random.Generator(np.random.PCG64(4000 + log_b + n))
    bra, brb, tables = r64(rng, n_lwe, 2 * d, n), r64(rng, n_lwe, 2 * d, n), r64(rng, 3, n)
    a_raw, b_raw = r64(rng, batch, n_lwe), r64(rng, batch)
    ksa, ksb = r64(rng, n * ks_d, n_lwe), r64(rng, n * ks_d)
    table_of = np.array([0, 0, 2, 0, 2, 1, 2], dtype=np.uint32)
    t = fhe.TorusContext()
    D = lambda x: dev(torch_cuda, x)  # noqa: E731
    dksa, dksb, dtab, da, db, dtof = D(ksa), D(ksb), D(tables), D(a_raw), D(b_raw), dev32(torch_cuda, table_of)
    at, bt = fhe.TorusContext.mod_switch(da, n), fhe.TorusContext.mod_switch(db, n)
    for fft64 in (False, True):
        key = fhe.TggswKey(t, log_b, d, D(bra), D(brb), n, fft64=fft64)
        ga, gb = key.bootstrap_tables(ks_log_b, ks_d, dksa, dksb, dtab, dtof, da, db)
        ra, rb = key.blind_rotate_tables(at, bt, dtab, dtof)
        ga, gb, ra, rb = host(ga).reshape(batch, n_lwe), host(gb), host(ra).reshape(batch, n), host(rb).reshape(batch, n)
        for k in range(3):
            sel = np.nonzero(table_of == k)[0]
            sa, sb = key.bootstrap(ks_log_b, ks_d, dksa, dksb, dtab[k], da, db)          # the existing entry, v = tables[k], whole batch
            xa, xb = key.blind_rotate(at, bt, dtab[k])
            assert np.array_equal(ga[sel], host(sa).reshape(batch, n_lwe)[sel]) and np.array_equal(gb[sel], host(sb)[sel]), (fft64, k)
            assert np.array_equal(ra[sel], host(xa).reshape(batch, n)[sel]) and np.array_equal(rb[sel], host(xb).reshape(batch, n)[sel]), (fft64, k)
            if not fft64:
                ea, eb = cref.tfhe_bootstrap(log_b, d, ks_log_b, ks_d, bra, brb, ksa, ksb, tables[k], a_raw[sel], b_raw[sel], threads=8)
                assert np.array_equal(ga[sel], ea) and np.array_equal(gb[sel], eb), ("oracle", k)
        if not fft64:  # every operand in host memory: the same bits; an index out of range is refused before anything runs
            ha, hb = key.bootstrap_tables(ks_log_b, ks_d, ksa, ksb, tables, table_of, a_raw, b_raw)
            assert np.array_equal(ha, ga) and np.array_equal(hb, gb)
            qa, qb = key.blind_rotate_tables(host(at), host(bt), tables, table_of)
            assert np.array_equal(qa, ra) and np.array_equal(qb, rb)
            bad = table_of.copy()
            bad[batch - 1] = 3
            for call in (lambda: key.bootstrap_tables(ks_log_b, ks_d, ksa, ksb, tables, bad, a_raw, b_raw),
                         lambda: key.blind_rotate_tables(host(at), host(bt), tables, bad)):
                with pytest.raises(fhe.FheError) as e:
                    call()
                assert e.value.code == 1


def test_tables_across_team_and_workgroup_boundaries(fhe, cref, torch_cuda):
    """batch 1100 over 5 tables: the first and last ciphertext and both sides of the 64 and 256 boundaries against the oracle, the whole
    batch against the shared-table entry called once per table"""
    n, log_b, d, n_lwe, batch, ks_log_b, ks_d = 1024, 7, 3, 6, 1100, 4, 5
    rng = np.random.Generator(np.random.PCG64(4100))
    bra, brb, tables = r64(rng, n_lwe, 2 * d, n), r64(rng, n_lwe, 2 * d, n), r64(rng, 5, n)
    a_raw, b_raw = r64(rng, batch, n_lwe), r64(rng, batch)
    ksa, ksb = r64(rng, n * ks_d, n_lwe), r64(rng, n * ks_d)
    table_of = rng.integers(0, 5, size=batch, dtype=np.uint32)
    table_of[[0, 63, 64, 255, 256, batch - 1]] = [4, 0, 3, 1, 2, 4]
    t = fhe.TorusContext()
    D = lambda x: dev(torch_cuda, x)  # noqa: E731
    key = fhe.TggswKey(t, log_b, d, D(bra), D(brb), n)
    dksa, dksb, dtab, da, db = D(ksa), D(ksb), D(tables), D(a_raw), D(b_raw)
    ga, gb = key.bootstrap_tables(ks_log_b, ks_d, dksa, dksb, dtab, dev32(torch_cuda, table_of), da, db)
    ga, gb = host(ga).reshape(batch, n_lwe), host(gb)
    for k in range(5):
        sel = table_of == k
        sa, sb = key.bootstrap(ks_log_b, ks_d, dksa, dksb, dtab[k], da, db)
        assert np.array_equal(ga[sel], host(sa).reshape(batch, n_lwe)[sel]) and np.array_equal(gb[sel], host(sb)[sel]), k
    for i in (0, 1, 63, 64, 255, 256, 1023, 1024, batch - 1):
        ea, eb = cref.tfhe_bootstrap(log_b, d, ks_log_b, ks_d, bra, brb, ksa, ksb, tables[table_of[i]], a_raw[i:i + 1], b_raw[i:i + 1])
        assert np.array_equal(ga[i], ea[0]) and int(gb[i]) == int(eb[0]), i


@pytest.mark.parametrize("k", [1, 16])
def test_tlwe_lincomb_vs_numpy(fhe, torch_cuda, k):
    """wrapping uint64 arithmetic: negative weights, the extremes of int32, a constant of 2^64 - 1 (on b only); device and host memory"""
    n, batch = 37, 5
    rng = np.random.Generator(np.random.PCG64(4200 + k))
    cts = [(r64(rng, batch, n), r64(rng, batch)) for _ in range(k)]
    w = [int(x) for x in rng.integers(-9, 10, size=k)]
    w = [x if x else -3 for x in w]
    w[0] = -(1 << 31)
    if k > 1:
        w[1], w[2] = (1 << 31) - 1, -1
    const = M64 - 1
    with np.errstate(over="ignore"):
        ea, eb = np.zeros((batch, n), dtype=np.uint64), np.full(batch, const, dtype=np.uint64)
        for x, (a, b) in zip(w, cts):
            ea += np.uint64(x % M64) * a
            eb += np.uint64(x % M64) * b
    oa, ob = fhe.tlwe_lincomb(w, [(dev(torch_cuda, a), dev(torch_cuda, b)) for a, b in cts], const)
    assert np.array_equal(host(oa).reshape(batch, n), ea) and np.array_equal(host(ob), eb)
    ha, hb = fhe.tlwe_lincomb(w, cts, const)
    assert np.array_equal(ha, ea) and np.array_equal(hb, eb)


def hand_made_netlist(T):
    """3 inputs, 6 nodes over 3 levels: fan-out (n0, n1, n3), a dead node (n5), weights -1 and 4, a non-zero constant, 3 tables;
    outputs: a node, an input, the same node again, a node of the middle level"""
    b = T.Builder()
    i0, i1, i2 = b.input(), b.input(), b.input()
    t0, t1, t2 = b.table(lambda v: v), b.table(lambda v: 2 * v + 1), b.table(lambda v: v % 3)
    n0 = b.node([(i0, 1), (i1, 1)], t0)
    n1 = b.node([(i1, 4), (i2, -1)], t1, constant=5)
    n2 = b.node([(n0, 1), (n1, -1)], t2)
    n3 = b.node([(n0, 1), (i2, 4)], t0, constant=31)
    n4 = b.node([(n2, 1), (n3, 1), (i0, -1)], t1)
    b.node([(n1, 1), (n3, 1)], t2)
    return b, [n4, i1, n4, n2]


@pytest.mark.parametrize("n,log_b,d,n_lwe,batch", [(256, 15, 1, 6, 3), (1024, 7, 3, 6, 5)])
def test_circuit_equals_node_by_node(fhe, torch_cuda, n, log_b, d, n_lwe, batch):
    """fhe_tfhe_circuit_run bit-equal to fhe_tlwe_lincomb + fhe_tfhe_bootstrap per node (exact key form -- three 30-bit primes at the
    small shape, the f64 pieces at n = 1024 -- and fft64), to the same call with every operand in host memory and, at the small shape,
    to oracle.pyref composed per live node.  Random key rows, key-switch rows and tables."""
    from oracle import pyref as P
    T = fhe.tfhe_circuit
    ks_log_b, ks_d, log_p, padding = 4, 5, 4, 1
    b, outputs = hand_made_netlist(T)
    c = b.compile(outputs, log_p, padding, n)
    assert c.info() == {"levels": 3, "live_nodes": 5, "max_width": 2} and c.levels() == [1, 1, 2, 2, 3, 0]
    rng = np.random.Generator(np.random.PCG64(4300 + n))
    bra, brb, tables = r64(rng, n_lwe, 2 * d, n), r64(rng, n_lwe, 2 * d, n), r64(rng, 3, n)
    ksa, ksb = r64(rng, n * ks_d, n_lwe), r64(rng, n * ks_d)
    in_a, in_b = r64(rng, 3, batch, n_lwe), r64(rng, 3, batch)
    t = fhe.TorusContext()
    D = lambda x: dev(torch_cuda, x)  # noqa: E731
    for fft64 in (False, True):
        key = fhe.TggswKey(t, log_b, d, D(bra), D(brb), n, fft64=fft64)
        oa, ob = c.run(key, ks_log_b, ks_d, D(ksa), D(ksb), (D(in_a), D(in_b)), batch, tables=D(tables))
        na, nb = c.run_nodes(key, ks_log_b, ks_d, D(ksa), D(ksb), (D(in_a), D(in_b)), batch, tables=D(tables))
        assert torch_cuda.equal(oa, na.reshape(oa.shape)) and torch_cuda.equal(ob, nb.reshape(ob.shape)), fft64
        oa, ob = host(oa).reshape(4, batch, n_lwe), host(ob).reshape(4, batch)
        assert np.array_equal(oa[1], in_a[1]) and np.array_equal(ob[1], in_b[1])      # the output that names an input
        assert np.array_equal(oa[0], oa[2]) and np.array_equal(ob[0], ob[2])          # the repeated output
        if not fft64:
            ha, hb = c.run(key, ks_log_b, ks_d, ksa, ksb, (in_a, in_b), batch, tables=tables)
            assert np.array_equal(ha, oa) and np.array_equal(hb, ob)
            exact = (oa, ob)
    if n > 256:
        return
    # oracle.pyref, node after node (dead node skipped: nothing reads it)
    dec, ksdec = P.TorusDecomposor(log_b, d), P.TorusDecomposor(ks_log_b, ks_d)
    brk = [([[int(x) for x in r] for r in bra[i]], [[int(x) for x in r] for r in brb[i]]) for i in range(n_lwe)]
    pka, pkb = [[int(x) for x in r] for r in ksa], [int(x) for x in ksb]
    log_delta = 64 - (log_p + padding)
    live = c.levels()
    for bi in range(batch):
        vals = []

        def get(w):
            return ([int(x) for x in in_a[w.index][bi]], int(in_b[w.index][bi])) if w.is_input else vals[w.index]

        for g, (terms, table, constant) in enumerate(b.nodes):
            if not live[g]:
                vals.append(None)
                continue
            sa, sb = [0] * n_lwe, (constant << log_delta) % M64
            for w, k in terms:
                xa, xb = get(w)
                sa, sb = [(s + k * x) % M64 for s, x in zip(sa, xa)], (sb + k * xb) % M64
            acc = P.tfhe_blind_rotate(dec, brk, [int(x) for x in tables[table]], P.tfhe_mod_switch(sa, n), P.tfhe_mod_switch([sb], n)[0])
            ea, eb = P.tglwe_sample_extract(acc[0], acc[1], 0)
            vals.append(P.tlwe_key_switch(ksdec, pka, pkb, ea, eb))
        for o, w in enumerate(outputs):
            xa, xb = get(w)
            assert [int(x) for x in exact[0][o][bi]] == xa and int(exact[1][o][bi]) == xb, (bi, o)


def test_adder_and_equality_decode_with_device_made_keys(fhe, torch_cuda):
    """The 8-bit adder (4 blocks of 2 message + 2 carry bits) and radix_eq at decode level: n = 256, n_lwe = 16, gadget (7, 3), key
    switch (4, 5), log_p 4, padding 1; keys from fhe_tggsw_encrypt and fhe_tlwe_ksk_gen at the reference's two standard deviations
    (bootstrapping.rs:144-148), inputs from fhe_tlwe_sk_encrypt.  32 random byte pairs plus (255, 255), (0, 0), (255, 1); every output
    block decrypts (tlwe.rs:134-142) to the plain model's value.  Margin by construction: the mod-switch drift has a standard
    deviation of sqrt((n_lwe / 2 + 1) / 12) ~ 0.9 of 2N = 512 positions against a half-slot of 8; gadget and key-switch errors
    are near 2^-16 of the torus against a half-slot of 2^-6."""
    from oracle import pyref as P
    T = fhe.tfhe_circuit
    n, n_lwe, log_b, d, ks_log_b, ks_d, log_p, padding = 256, 16, 7, 3, 4, 5, 4, 1
    sd_lwe, sd_glwe = 1.339775301998614e-7, 2.845267479601915e-15
    p, log_delta = 1 << log_p, 64 - (log_p + padding)
    like = dev(torch_cuda, U([0]))
    t = fhe.TorusContext()
    z, s = fhe.sample_binary(900, 0, like, n_lwe), fhe.sample_binary(900, 1, like, n)
    zh = [int(x) for x in host(z)]
    pt = np.zeros((n_lwe, n), dtype=np.uint64)
    pt[:, 0] = host(z)                                            # Rt::constant(z_i) (bootstrapping.rs:66-67)
    ra, rb = fhe.tggsw_encrypt(t, log_b, d, s, dev(torch_cuda, pt), n, sd_glwe, 901, 0)
    key = fhe.TggswKey(t, log_b, d, ra, rb, n)
    ksa, ksb = fhe.tlwe_ksk_gen(ks_log_b, ks_d, z, s, sd_lwe, 902, 0)
    rng = np.random.Generator(np.random.PCG64(4400))
    xs = np.concatenate([rng.integers(0, 256, size=32), [255, 0, 255]])
    ys = np.concatenate([rng.integers(0, 256, size=32), [255, 0, 1]])
    batch = len(xs)
    blocks = [(xs >> (2 * i)) & 3 for i in range(4)] + [(ys >> (2 * i)) & 3 for i in range(4)]   # [8][batch], x first
    msgs = U([(int(v) << log_delta) % M64 for row in blocks for v in row])
    ca, cb = fhe.tlwe_sk_encrypt(z, dev(torch_cuda, msgs), n_lwe, 8 * batch, sd_lwe, 903, 0)

    def decrypt(oa, ob):
        oa, ob = host(oa).reshape(-1, batch, n_lwe), host(ob).reshape(-1, batch)
        return [[((P.tlwe_phase(zh, [int(v) for v in oa[o][i]], int(ob[o][i])) + (1 << (log_delta - 1))) % M64) >> log_delta for i in range(batch)]
                for o in range(oa.shape[0])]

    b, _, _, outs = T.radix_add(4, 2, 2)
    add = b.compile(outs, log_p, padding, n)
    got = decrypt(*add.run(key, ks_log_b, ks_d, ksa, ksb, (ca, cb), batch))
    want = b.evaluate(blocks, log_p, padding, outs)
    assert [list(map(int, w)) for w in want] == got
    assert [sum(got[i][j] << (2 * i) for i in range(4)) for j in range(batch)] == [int(v) for v in (xs + ys) & 255]
    b, _, _, eq = T.radix_eq(4, 2)
    cmp_ = b.compile([eq], log_p, padding, n)
    got = decrypt(*cmp_.run(key, ks_log_b, ks_d, ksa, ksb, (ca, cb), batch))
    assert got == [[int(v) for v in (xs == ys)]] and got[0][-3:] == [1, 1, 0]
    assert p == 16


def test_key_outlives_its_context(fhe, torch_cuda):
    """A prepared key destroyed AFTER its context (the order a garbage-collected reference cycle may pick) frees its rows on the device
    it was prepared on, without reading the context: no HIP error is left behind for the next launch to report."""
    n, log_b, d, n_lwe = 256, 7, 3, 6
    rng = np.random.Generator(np.random.PCG64(4500))
    rows = dev(torch_cuda, r64(rng, n_lwe, 2 * d, n))
    for fft64 in (False, True):
        t = fhe.TorusContext()
        key = fhe.TggswKey(t, log_b, d, rows, rows, n, fft64=fft64)
        t.__del__()
        np.zeros(1 << 16, dtype=np.uint64).fill(M64 - 1)     # (a chance for the allocator to hand the context's memory out again)
        key.__del__()
        x = dev(torch_cuda, r64(rng, 64))
        assert np.array_equal(host(fhe.TorusContext.mod_switch(x, n)), ((host(x) + np.uint64(1 << 54)) >> np.uint64(55)))


def test_c_program_tfhe_circuit(tmp_path, fhe):
    """examples/tfhe_circuit_demo.c: device-made keys, encryption, the adder's netlist and fhe_tfhe_circuit_run on host buffers from plain C"""
    from conftest import ROOT
    lib_dir = os.path.dirname(fhe.lib_path())
    exe = tmp_path / "tfhe_circuit_demo"
    cmd = ["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "tfhe_circuit_demo.c"), "-o", str(exe),
           "-L", lib_dir, "-lfhe_ring", "-Wl,--allow-shlib-undefined", "-Wl,-rpath," + lib_dir, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tfhe_circuit_demo ok" in r.stdout, r.stdout + r.stderr
