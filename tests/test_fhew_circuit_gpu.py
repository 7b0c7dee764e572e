"""FHEW gate circuits on the device (fhe_fhew_circuit_run): a levelled netlist in one call against the same netlist run gate by gate
through ring.Fhew (fhe_lwe_lincomb + fhe_fhew_bootstrap) -- bit for bit: the bootstrap draws nothing and the linear parts are exact
mod Q -- and against the truth at decrypt level.  The reference's `single_key_testing_param` (fhew/boolean.rs:225-239), keys made on
the device as in test_keygen_gpu.py::test_whole_bootstrapping_key_made_on_the_device."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = lambda x: [int(v) for v in np.asarray(x).ravel()]  # noqa: E731
U = lambda x: np.array(x, dtype=np.uint64)  # noqa: E731


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


class Keys:
    pass


@pytest.fixture(scope="module")
def K(fhe):
    import torch
    from oracle import pyref as P
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    k = Keys()
    log_q, log_n, log_b, d, w = 28, 9, 7, 4, 10
    n_lwe, q_ks, kb, kd = 100, 1 << 16, 4, 4
    n = 1 << log_n
    q = next(P.two_adic_primes(log_q, log_n + 1))
    like = dev(torch, U([0]))
    ctx = fhe.NttContext(q)
    z_i = host(fhe.sample_dg(0, 3.2, 6, 910, 0, like, (n,))).view(np.int64)
    s_i = host(fhe.sample_dg(0, 3.2, 6, 910, 1, like, (n_lwe,))).view(np.int64)
    zq = lambda v, m: dev(torch, U([int(x) % m for x in v]))  # noqa: E731
    z_q, z_ks, s_ks = zq(z_i, q), zq(z_i, q_ks), zq(s_i, q_ks)
    mono = np.zeros((n_lwe, n), dtype=np.uint64)
    for j, sj in enumerate(s_i):
        e = int(sj) % (2 * n)
        mono[j, e % n] = 1 if e < n else q - 1
    ra, rb = fhe.rgsw_encrypt(ctx, log_b, d, z_q, dev(torch, mono), n, 911, 0)
    ts = P.ak_t(n, w)
    aks = [fhe.rlwe_ksk_gen(ctx, log_b, d, z_q, None, t, n, 912, i) for i, t in enumerate(ts)]
    ak_a = torch.stack([x[0] for x in aks]).contiguous()
    ak_b = torch.stack([x[1] for x in aks]).contiguous()
    ksk_a, ksk_b = fhe.lwe_ksk_gen(q_ks, kb, kd, s_ks, z_ks, 913, 0)
    gk = fhe.GadgetKey(ctx, log_b, d, ra, rb, n, rgsw=True)
    ga = fhe.GadgetKey(ctx, log_b, d, ak_a, ak_b, n, rgsw=False)
    k.bk = fhe.BootstrapKey(ctx, gk, ga, ts, w)
    k.ev = fhe.Fhew(k.bk, q_ks, kb, kd, ksk_a, ksk_b)
    k.ev_host = fhe.Fhew(k.bk, q_ks, kb, kd, host(ksk_a).copy(), host(ksk_b).copy())
    k.torch, k.q, k.n, k.like = torch, q, n, like
    delta = q / 4.0
    z = [int(v) for v in z_i]
    stream = [0]

    def encrypt(rows):
        """rows [wires][batch] of bits -> (a [wires][batch][n], b [wires][batch]) (lwe.rs:128-139)"""
        stream[0] += 1
        rows = np.asarray(rows)
        pt = dev(torch, U([P.zq_from_f64(q, float(m) * delta) for m in rows.ravel()]))
        a, b = fhe.lwe_sk_encrypt(q, z_q, pt, n, rows.size, 914, stream[0])
        return a.reshape(rows.shape + (n,)), b.reshape(rows.shape)

    def decrypt(a, b):
        """-> bits, the shape of b"""
        a, b = np.asarray(a).reshape(-1, n), np.asarray(b)
        out = []
        for i in range(a.shape[0]):
            m = P.zq_from_f64(4, float(P.lwe_decrypt(q, z, L(a[i]), int(b.ravel()[i]))) / delta)
            assert m in (0, 1), m
            out.append(m)
        return np.array(out).reshape(b.shape)

    k.encrypt, k.decrypt = encrypt, decrypt
    return k


def gate_by_gate(K, c, outs, in_a, in_b):
    """the netlist through ring.Fhew, one gate bootstrap after the other -> (a [outputs][batch][n], b [outputs][batch])"""
    res = c.evaluate_fhew(K.ev, [(in_a[i], in_b[i]) for i in range(in_a.shape[0])], outs)
    return K.torch.stack([r[0].reshape(in_a.shape[1:]) for r in res]), K.torch.stack([r[1].reshape(in_b.shape[1:]) for r in res])


def truth(c, outs, rows):
    """evaluate_plain per batch entry -> [outputs][batch]"""
    rows = np.asarray(rows)
    cols = [c.evaluate_plain([bool(v) for v in rows[:, j]], outs) for j in range(rows.shape[1])]
    return np.array(cols, dtype=np.int64).T


def byte_bits(vals):
    return [[(v >> i) & 1 for v in vals] for i in range(8)]


def from_bits(bits):
    """[8][batch] -> [batch] integers"""
    return [sum(int(bits[i][j]) << i for i in range(len(bits))) for j in range(len(bits[0]))]


def test_every_op_and_inversion_bit_for_bit(fhe, K):
    """level 1: the six two-input gates under all 4 inversion patterns and majority under all 8; level 2 reads level-1 wires plain and
    inverted (and an input); outputs: every gate, a wire twice, an inverted gate, a bare and an inverted input.  Batch = the 8 input
    combinations.  Device memory and host memory."""
    torch = K.torch
    c = fhe.Circuit()
    x, y, z = c.input(), c.input(), c.input()
    two = (c.and_, c.nand, c.or_, c.nor, c.xor, c.xnor)
    inv = lambda w, f: ~w if f else w  # noqa: E731
    l1 = [op(inv(x, p & 1), inv(y, p >> 1)) for op in two for p in range(4)]
    l1 += [c.majority(inv(x, p & 1), inv(y, (p >> 1) & 1), inv(z, p >> 2)) for p in range(8)]
    l2 = [two[i % 6](l1[2 * i], ~l1[2 * i + 1]) for i in range(16)]
    l2 += [c.majority(~l1[0], l1[13], ~z), c.xor(~l1[30], x)]
    outs = l1 + l2 + [l1[3], l1[3], ~l2[0], ~l2[16], y, ~z]
    cc = c.compile(outs)
    assert cc.info() == {"levels": 2, "live_gates": 50, "max_width": 32}
    rows = [[(m >> i) & 1 for m in range(8)] for i in range(3)]
    in_a, in_b = K.encrypt(rows)
    out_a, out_b = cc.run(K.ev, (in_a, in_b), 8)
    K.bk.check(out_a)  # the status path of a device-memory run: FHE_OK
    ref_a, ref_b = gate_by_gate(K, c, outs, in_a, in_b)
    assert torch.equal(out_b, ref_b) and torch.equal(out_a, ref_a)
    exp = truth(c, outs, rows)
    assert np.array_equal(K.decrypt(host(out_a), host(out_b)), exp)
    assert len(set(map(tuple, exp[:50]))) > 20  # (the gates do differ)
    # host memory: inputs, outputs and keys mirrored once; the same bits
    h_a, h_b = cc.run(K.ev_host, (host(in_a).copy(), host(in_b).copy()), 8)
    assert np.array_equal(h_a, host(out_a)) and np.array_equal(h_b, host(out_b))


@pytest.mark.parametrize("op,xs,ys", [("add", [255, 255, 0, 100, 0], [1, 255, 0, 57, 200]), ("mul", [255, 0, 13], [255, 77, 19])])
def test_bytes_bit_for_bit(fhe, K, op, xs, ys):
    """`FhewU8::wrapping_add` at batch 5 (255 + 1, 255 + 255, 0 + 0 among them), `wrapping_mul` at batch 3 (uint8.rs:88-90, 119-131)"""
    from learn_fhe_amd import circuit as C
    c = fhe.Circuit()
    x, y = c.input_u8(), c.input_u8()
    outs = C.u8_wrapping_add(c, x, y) if op == "add" else C.u8_wrapping_mul(c, x, y)
    cc = c.compile(outs)
    rows = byte_bits(xs) + byte_bits(ys)
    in_a, in_b = K.encrypt(rows)
    out_a, out_b = cc.run(K.ev, (in_a, in_b), len(xs))
    ref_a, ref_b = gate_by_gate(K, c, outs, in_a, in_b)
    K.bk.check(out_a)
    assert K.torch.equal(out_b, ref_b) and K.torch.equal(out_a, ref_a)
    got = from_bits(K.decrypt(host(out_a), host(out_b)))
    assert got == [((a + b) if op == "add" else (a * b)) & 255 for a, b in zip(xs, ys)]


def plain_levels(c, outs):
    """levels and pruning restated on the builder's netlist: {gate: level} of the live gates"""
    live, stack = set(), [w.index for w in outs if not w.is_input]
    while stack:
        g = stack.pop()
        if g not in live:
            live.add(g)
            stack += [w.index for w in c.gates[g][1] if not w.is_input]
    lv = {}
    for g in sorted(live):
        lv[g] = 1 + max(0 if w.is_input else lv[w.index] for w in c.gates[g][1])
    return lv


@pytest.mark.parametrize("xv,yv", [(200, 7), (5, 9)])
def test_div_rem_in_one_call(fhe, K, xv, yv):
    """`FhewU8::div_rem` (uint8.rs:133-152), the deepest circuit and the one that uses `select`: a nonzero divisor, and a dividend below
    the divisor; decrypt level.  info() against the netlist's own depth and size: the whole chain ran inside the one call."""
    from learn_fhe_amd import circuit as C
    c = fhe.Circuit()
    x, y = c.input_u8(), c.input_u8()
    qt, rm = C.u8_div_rem(c, x, y)
    outs = qt + rm
    cc = c.compile(outs)
    lv = plain_levels(c, outs)
    info = cc.info()
    assert info["levels"] == max(lv.values()) and info["live_gates"] == len(lv) and info["levels"] > 100 and info["live_gates"] > 300
    assert cc.levels() == [lv.get(g, 0) for g in range(len(c.gates))]
    in_a, in_b = K.encrypt(byte_bits([xv]) + byte_bits([yv]))
    out_a, out_b = cc.run(K.ev, (in_a, in_b), 1)
    K.bk.check(out_a)
    bits = K.decrypt(host(out_a), host(out_b))
    assert (from_bits(bits[:8])[0], from_bits(bits[8:])[0]) == divmod(xv, yv)


def test_batch_one_and_levels_of_one_gate(fhe, K):
    """a chain of three xors at batch 1: every level is ONE ciphertext, the shape fhe_blind_rotate_split decides about"""
    c = fhe.Circuit()
    x, y, z = c.input(), c.input(), c.input()
    outs = [c.xor(c.xor(c.xor(x, y), ~z), x)]
    cc = c.compile(outs)
    assert cc.info() == {"levels": 3, "live_gates": 3, "max_width": 1}
    for m in (0b110, 0b011):
        rows = [[(m >> i) & 1] for i in range(3)]
        in_a, in_b = K.encrypt(rows)
        out_a, out_b = cc.run(K.ev, (in_a, in_b), 1)
        ref_a, ref_b = gate_by_gate(K, c, outs, in_a, in_b)
        assert K.torch.equal(out_b, ref_b) and K.torch.equal(out_a, ref_a)
        assert K.decrypt(host(out_a), host(out_b)).tolist() == truth(c, outs, rows).tolist()
    K.bk.check(out_a)
    assert K.bk.split(1) >= 1


def test_no_live_gate_and_unaligned_operands(fhe, K):
    """outputs taken at level 0 (no gate runs: the output kernel alone), and operands that are 8 but not 16 bytes aligned (the
    one-coefficient-per-lane form of both kernels): the same bits as the aligned call"""
    torch = K.torch
    c = fhe.Circuit()
    x, y = c.input(), c.input()
    cc0 = c.compile([~x, y, x])
    in_a, in_b = K.encrypt([[0, 1, 1], [1, 0, 1]])
    o_a, o_b = cc0.run(K.ev, (in_a, in_b), 3)
    nx = K.ev.not_((in_a[0], in_b[0]))
    assert torch.equal(o_a[0], nx[0]) and torch.equal(o_b[0], nx[1]) and torch.equal(o_a[1], in_a[1]) and torch.equal(o_b[2], in_b[0])
    outs = [c.nand(~x, y), ~c.xor(x, ~y)]
    cc = c.compile(outs)
    a_a, a_b = cc.run(K.ev, (in_a, in_b), 3)
    pad = torch.zeros(in_a.numel() + 1, dtype=in_a.dtype, device=in_a.device)
    pad[1:] = in_a.reshape(-1)
    shifted = pad[1:].reshape(in_a.shape)
    assert shifted.data_ptr() % 16 == 8 and shifted.is_contiguous()
    u_a, u_b = cc.run(K.ev, (shifted, in_b), 3)
    assert torch.equal(u_a, a_a) and torch.equal(u_b, a_b)
    assert K.decrypt(host(a_a), host(a_b)).tolist() == truth(c, outs, [[0, 1, 1], [1, 0, 1]]).tolist()
    K.bk.check(a_a)


def test_c_program_adds_two_encrypted_bytes(tmp_path, fhe):
    """examples/fhew_circuit_demo.c: keys, encryption, the adder's netlist and fhe_fhew_circuit_run on host buffers from plain C"""
    from conftest import ROOT
    lib_dir = os.path.dirname(fhe.lib_path())
    exe = tmp_path / "fhew_circuit_demo"
    cmd = ["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "fhew_circuit_demo.c"), "-o", str(exe),
           "-L", lib_dir, "-lfhe_ring", "-Wl,--allow-shlib-undefined", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fhew_circuit_demo ok" in r.stdout, r.stdout + r.stderr
    assert "255 + 1 = 0 (mod 256)" in r.stdout and "255 + 255 = 254 (mod 256)" in r.stdout and "100 + 57 = 157 (mod 256)" in r.stdout
