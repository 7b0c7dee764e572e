"""No-GPU checks of the TFHE look-up-table circuits: fhe_tfhe_circuit_create's validation, pruning and levelling through the library
(host only), the encoded tables against the reference's `table` (scheme/tfhe/src/bootstrapping.rs:118-128), and the plain-value model of
the radix arithmetic over every pair of bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest


def test_new_symbols_are_exported(fhe):
    lib = fhe.lib()
    for name in ("fhe_tfhe_blind_rotate_tables", "fhe_tfhe_bootstrap_tables", "fhe_tlwe_lincomb", "fhe_tfhe_circuit_create",
                 "fhe_tfhe_circuit_destroy", "fhe_tfhe_circuit_info", "fhe_tfhe_circuit_levels", "fhe_tfhe_circuit_run"):
        assert hasattr(lib, name), name


def _create(fhe, nodes, terms, n_inputs, n_tables, outputs, n_terms=None, n_outputs=None):
    """nodes: (first_term, n_terms, constant, table); terms: (wire, weight) -> (status, handle value)"""
    T = fhe.tfhe_circuit
    narr = (T._Node * max(1, len(nodes)))()
    for i, (f, k, c, t) in enumerate(nodes):
        narr[i].first_term, narr[i].n_terms, narr[i].constant, narr[i].table = f, k, c, t
    tarr = (T._Term * max(1, len(terms)))()
    for i, (w, x) in enumerate(terms):
        tarr[i].wire, tarr[i].weight = w, x
    oarr = (C.c_uint32 * max(1, len(outputs)))(*outputs)
    h = C.c_void_p(0xdead)
    rc = fhe.lib().fhe_tfhe_circuit_create(narr, len(nodes), tarr, len(terms) if n_terms is None else n_terms, n_inputs, n_tables, oarr,
                                           len(outputs) if n_outputs is None else n_outputs, C.byref(h))
    if rc == 0:
        fhe.lib().fhe_tfhe_circuit_destroy(h)
    return rc, h.value


def test_create_rejects_every_invalid_netlist(fhe):
    """each case of include/fhe_ring.h: FHE_ERR_INVALID and no handle"""
    terms = [(0, 1), (1, -1), (2, 4)]
    nodes = [(0, 2, 7, 0), (1, 2, 0, 1)]
    assert _create(fhe, nodes, terms, 2, 2, [3, 0])[0] == 0
    bad = {
        "term range outside terms": dict(n_terms=2),
        "first_term past the end": dict(nodes=[(1 << 31, 2, 0, 0)], outputs=[0]),
        "n_terms == 0": dict(nodes=[(0, 0, 0, 0)], outputs=[2]),
        "n_terms > 16": dict(nodes=[(0, 17, 0, 0)], terms=[(0, 1)] * 17, outputs=[2]),
        "forward wire": dict(nodes=[(0, 2, 0, 0)], terms=[(0, 1), (2, 1)], outputs=[2]),
        "wire out of range": dict(nodes=[(0, 2, 0, 0)], terms=[(0, 1), (1 << 30, 1)], outputs=[2]),
        "weight of 0": dict(nodes=[(0, 2, 0, 0)], terms=[(0, 1), (1, 0)], outputs=[2]),
        "table >= n_tables": dict(n_tables=1),
        "n_inputs == 0": dict(n_inputs=0),
        "n_outputs == 0": dict(n_outputs=0),
        "output out of range": dict(outputs=[4]),
        "more than 2^24 wires": dict(nodes=[], terms=[], n_inputs=(1 << 24) + 1, outputs=[0]),
        "n_tables > 65536": dict(n_tables=65537),
    }
    for why, change in bad.items():
        args = dict(nodes=nodes, terms=terms, n_inputs=2, n_tables=2, outputs=[3, 0])
        args.update(change)
        rc, h = _create(fhe, **args)
        assert rc == 1 and not h, why
    assert _create(fhe, [(0, 16, 0, 0)], [(0, 1)] * 16, 2, 65536, [2])[0] == 0
    assert fhe.lib().fhe_tfhe_circuit_create(None, 0, None, 0, 1, 1, (C.c_uint32 * 1)(0), 1, None) == 1
    assert fhe.lib().fhe_tfhe_circuit_info(None, None, None, None) == 1


def test_radix_add_levels_and_pruning(fhe):
    T = fhe.tfhe_circuit
    b, x, y, outs = T.radix_add(4, 2, 2)
    assert len(b.nodes) == 8 and b.n_inputs == 8 and len(b.tables) == 2
    c = b.compile(outs, 4, 1, 256)
    assert c.info() == {"levels": 4, "live_nodes": 7, "max_width": 2}
    assert c.levels() == [1, 1, 2, 2, 3, 3, 4, 0]          # the last carry is dropped
    # naming the last carry as an output keeps it
    assert b.compile(outs + [T.Wire(b, False, 7)], 4, 1, 256).info() == {"levels": 4, "live_nodes": 8, "max_width": 2}


def test_lut_is_the_reference_table_encoded(fhe):
    """bootstrapping.rs:118-128: table[0] on n / 2p coefficients, every further value on n / p, -table[0] on the last n / 2p; encoded as
    tlwe.rs:113-116 (value << log_delta).  Mod p (what decoding reads) every coefficient is the reference's; the last n / 2p are the
    torus negation of the first, -(table[0] << log_delta) mod 2^64, so that a phase just below 0 comes back as table[0] with a clear
    padding bit (the negacyclic wrap negates them once more)."""
    T = fhe.tfhe_circuit
    for n, log_p in [(256, 4), (1024, 4), (2048, 3)]:
        p, m, ld = 1 << log_p, n >> log_p, 64 - log_p - 1
        for f in (lambda v: v, lambda v: 2 * v, lambda v: v % 2, lambda v: 5):
            v = T.lut(f, log_p, 1, n)
            assert v.shape == (n,) and v.dtype == np.uint64
            want = [f(0) % p] * (m // 2) + [f(x) % p for x in range(1, p) for _ in range(m)] + [(-f(0)) % p] * (m // 2)
            assert [(int(x) >> ld) % p for x in v] == want and all(int(x) & ((1 << ld) - 1) == 0 for x in v)
            assert all(int(x) >> ld < p for x in v[:n - m // 2])                                   # padding bit clear on table values
            assert all((int(x) + int(v[0])) % (1 << 64) == 0 for x in v[n - m // 2:])              # the wrap gives table[0] exactly


def _bytes_as_blocks():
    a, b = np.arange(65536) >> 8, np.arange(65536) & 255
    return a, b, [(a >> (2 * i)) & 3 for i in range(4)] + [(b >> (2 * i)) & 3 for i in range(4)]


def test_radix_add_plain_model_all_byte_pairs(fhe):
    T = fhe.tfhe_circuit
    a, b, blocks = _bytes_as_blocks()
    bld, _, _, outs = T.radix_add(4, 2, 2)
    got = bld.evaluate(blocks, 4, 1, outs)
    assert all(int(o.max()) <= 3 and int(o.min()) >= 0 for o in got)
    assert np.array_equal(sum(o.astype(np.int64) << (2 * i) for i, o in enumerate(got)), (a + b) & 255)
    carry = bld.evaluate(blocks, 4, 1)[7]                   # the node create drops
    assert np.array_equal(carry, (a + b) >> 8)


def test_radix_eq_plain_model_all_byte_pairs(fhe):
    T = fhe.tfhe_circuit
    a, b, blocks = _bytes_as_blocks()
    bld, _, _, eq = T.radix_eq(4, 2)
    assert np.array_equal(bld.evaluate(blocks, 4, 1, [eq])[0], (a == b).astype(np.int64))
    c = bld.compile([eq], 4, 1, 256)
    assert c.info() == {"levels": 2, "live_nodes": 5, "max_width": 4} and c.n_tables == 2


def test_bivariate_plain_model(fhe):
    T = fhe.tfhe_circuit
    bld, x, y, w = T.bivariate(lambda u, v: (u * v + 1) % 16, 2)
    assert bld.nodes[0][0] == [(x, 4), (y, 1)]
    u, v = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
    assert np.array_equal(bld.evaluate([u.ravel(), v.ravel()], 4, 1, [w])[0], (u * v + 1).ravel() % 16)


def test_negative_weight_constant_and_padding_half(fhe):
    """x = constant + sum weight * wire over Z_2p: a weight of -1 with a non-zero constant, and sums that land in the padding half
    (x >= p) come out as -table[x - p], an element of Z_2p"""
    T = fhe.tfhe_circuit
    b = T.Builder()
    i0, i1 = b.input(), b.input()
    f = lambda v: (3 * v + 1) % 16  # noqa: E731
    n0 = b.node([(i0, 1), (i1, -1)], f, constant=5)
    n1 = b.node([(n0, 1), (i0, 4)], lambda v: v)
    for u in range(16):
        for v in range(16):
            x = (5 + u - v) % 32
            want0 = f(x) if x < 16 else (-f(x - 16)) % 32
            y = (want0 + 4 * u) % 32
            want1 = y if y < 16 else (-(y - 16)) % 32
            got = b.evaluate([u, v], 4, 1, [n0, n1])
            assert (int(got[0]), int(got[1])) == (want0, want1), (u, v)
    assert int(b.evaluate([0, 5], 4, 1, [n0])[0]) == f(0)               # 5 + 0 - 5 = 0
    assert int(b.evaluate([15, 3], 4, 1, [n0])[0]) == (-f(1)) % 32      # 5 + 15 - 3 = 17: the padding half, negated
    c = b.compile([n1], 4, 1, 256)
    assert c.info() == {"levels": 2, "live_nodes": 2, "max_width": 1}


def test_netlist_compiler_as_a_host_program(tmp_path):
    """tests/tfhe_circuit_host_test.cpp: csrc/tfhe_circuit.hpp alone (no HIP, no library) on random netlists against a restatement,
    the slot numbering's invariants, the rejected cases; a stand-alone program under AddressSanitizer and UBSan, run as its own process"""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "tfhe_circuit_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(here, "tfhe_circuit_host_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "tfhe_circuit_host_test ok" in out.stdout, out.stdout + out.stderr
