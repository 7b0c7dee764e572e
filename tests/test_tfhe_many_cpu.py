"""No-GPU checks of the many-LUT bootstrap (several tables from one blind rotation): the netlist compiler with many-LUT nodes as a host
program, fhe_tfhe_circuit_create_many's wire numbering, liveness per output and rejections through the library (host only), the
interleaved table against the ordinary ones, and the plain-value model of the adder with one many-LUT node per block over every pair
of bytes."""
import ctypes as C
import os
import subprocess

import numpy as np


def test_new_symbols_are_exported(fhe):
    lib = fhe.lib()
    for name in ("fhe_tfhe_mod_switch_many", "fhe_tglwe_sample_extract_many", "fhe_tfhe_bootstrap_many", "fhe_tfhe_circuit_create_many",
                 "fhe_tfhe_circuit_info_many"):
        assert hasattr(lib, name), name


def test_many_compiler_as_a_host_program(tmp_path):
    """tests/tfhe_many_host_test.cpp: csrc/tfhe_circuit.hpp alone (no HIP, no library): the plan at log_funcs = 0 against
    tfhe_circuit_compile field by field, mixed log_funcs against a restatement, liveness per output, the rejected cases; a stand-alone
    program under AddressSanitizer and UBSan, run as its own process"""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "tfhe_many_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(here, "tfhe_many_host_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "tfhe_many_host_test ok" in out.stdout, out.stdout + out.stderr


def _create_many(fhe, nodes, terms, n_inputs, n_tables, outputs):
    """nodes: (first_term, n_terms, constant, table, log_funcs); terms: (wire, weight) -> (status, info, info_many, levels) or (status,)"""
    T = fhe.tfhe_circuit
    narr = (T._Node * max(1, len(nodes)))()
    for i, (f, k, c, t, v) in enumerate(nodes):
        narr[i].first_term, narr[i].n_terms, narr[i].constant, narr[i].table, narr[i].pad = f, k, c, t, v
    tarr = (T._Term * max(1, len(terms)))()
    for i, (w, x) in enumerate(terms):
        tarr[i].wire, tarr[i].weight = w, x
    oarr = (C.c_uint32 * max(1, len(outputs)))(*outputs)
    h = C.c_void_p(0xdead)
    lib = fhe.lib()
    rc = lib.fhe_tfhe_circuit_create_many(narr, len(nodes), tarr, len(terms), n_inputs, n_tables, oarr, len(outputs), C.byref(h))
    if rc != 0:
        assert not h.value
        return (rc,)
    a, b, c, d, e = (C.c_size_t() for _ in range(5))
    assert lib.fhe_tfhe_circuit_info(h, C.byref(a), C.byref(b), C.byref(c)) == 0 and lib.fhe_tfhe_circuit_info_many(h, C.byref(d), C.byref(e)) == 0
    lv = (C.c_uint32 * max(1, len(nodes)))()
    assert lib.fhe_tfhe_circuit_levels(h, lv) == 0
    lib.fhe_tfhe_circuit_destroy(h)
    return rc, (a.value, b.value, c.value), (d.value, e.value), list(lv)[:len(nodes)]


# 2 inputs; node 0: v = 1 (wires 2, 3); node 1: v = 0 (wire 4); node 2: v = 2 (wires 5 .. 8); node 3: v = 1 (wires 9, 10), nothing reads it
MIXED_NODES = [(0, 2, 0, 0, 1), (2, 2, 7, 1, 0), (4, 2, 0, 2, 2), (6, 1, 0, 0, 1)]
MIXED_TERMS = [(0, 1), (1, 1), (3, 1), (0, -1), (2, 4), (4, 1), (8, 1)]


def test_create_many_numbers_wires_and_prunes_outputs(fhe):
    """levels, live nodes, widest level in nodes | live outputs, most key-switch rows of a level | level of every node"""
    assert _create_many(fhe, MIXED_NODES, MIXED_TERMS, 2, 3, [8, 1]) == (0, (3, 3, 1), (4, 2), [1, 2, 3, 0])
    assert _create_many(fhe, MIXED_NODES, MIXED_TERMS, 2, 3, [3]) == (0, (1, 1, 1), (1, 1), [1, 0, 0, 0])       # output 1 alone: one row
    assert _create_many(fhe, MIXED_NODES, MIXED_TERMS, 2, 3, [10, 9, 5]) == (0, (4, 4, 1), (7, 2), [1, 2, 3, 4])
    assert _create_many(fhe, MIXED_NODES, MIXED_TERMS, 2, 3, [0]) == (0, (0, 0, 0), (0, 0), [0, 0, 0, 0])


def test_create_many_rejections(fhe):
    ok = dict(nodes=MIXED_NODES, terms=MIXED_TERMS, n_inputs=2, n_tables=3, outputs=[8])
    assert _create_many(fhe, **ok)[0] == 0

    def change(**kw):
        args = dict(ok)
        args.update(kw)
        return _create_many(fhe, **args)

    def with_node(g, v):
        nodes = list(MIXED_NODES)
        nodes[g] = nodes[g][:4] + (v,)
        return nodes

    def with_term(k, w):
        terms = list(MIXED_TERMS)
        terms[k] = (w, terms[k][1])
        return terms

    assert change(nodes=with_node(2, 5)) == (1,)                      # log_funcs = 5
    assert change(nodes=with_node(2, 4))[0] == 0
    assert change(terms=with_term(2, 4)) == (1,)                      # node 1 naming its own first wire
    assert change(terms=with_term(4, 5)) == (1,)                      # node 2 naming its own first wire ...
    assert change(terms=with_term(4, 7)) == (1,)                      # ... and a further output of its own
    assert change(terms=with_term(4, 4))[0] == 0
    assert change(outputs=[11]) == (1,)                               # beyond the last wire (10)
    assert change(outputs=[10])[0] == 0
    assert change(n_tables=2) == (1,)
    # the existing create ignores the field: one wire per node, so wire 8 does not exist
    T = fhe.tfhe_circuit
    narr = (T._Node * 4)()
    for i, (f, k, c, t, v) in enumerate(MIXED_NODES):
        narr[i].first_term, narr[i].n_terms, narr[i].constant, narr[i].table, narr[i].pad = f, k, c, t, v
    tarr = (T._Term * 7)()
    for i, (w, x) in enumerate(MIXED_TERMS):
        tarr[i].wire, tarr[i].weight = w, x
    h = C.c_void_p()
    assert fhe.lib().fhe_tfhe_circuit_create(narr, 4, tarr, 7, 2, 3, (C.c_uint32 * 1)(8), 1, C.byref(h)) == 1
    assert fhe.lib().fhe_tfhe_circuit_create_many(None, 0, None, 0, 1, 1, (C.c_uint32 * 1)(0), 1, None) == 1
    assert fhe.lib().fhe_tfhe_circuit_info_many(None, None, None) == 1


def test_wire_cap_counts_output_wires(fhe):
    """2^20 nodes of 16 outputs over one input: 2^24 + 1 wires"""
    T = fhe.tfhe_circuit
    big = 1 << 20
    narr = (T._Node * big)()
    proto = T._Node(0, 1, 0, 0, 4)
    for i in range(big):
        narr[i] = proto
    tarr = (T._Term * 1)()
    tarr[0].wire, tarr[0].weight = 0, 1
    h = C.c_void_p()
    lib = fhe.lib()
    assert lib.fhe_tfhe_circuit_create_many(narr, big, tarr, 1, 1, 1, (C.c_uint32 * 1)(0), 1, C.byref(h)) == 1 and not h.value
    assert lib.fhe_tfhe_circuit_create_many(narr, big - 1, tarr, 1, 1, 1, (C.c_uint32 * 1)(0), 1, C.byref(h)) == 0
    lib.fhe_tfhe_circuit_destroy(h)


def test_lut_many_interleaves_the_ordinary_tables(fhe):
    T = fhe.tfhe_circuit
    fs = (lambda v: v, lambda v: 2 * v + 1, lambda v: v % 3, lambda v: 5)
    for n, log_p in [(256, 4), (1024, 4), (2048, 3)]:
        for f in fs:
            assert np.array_equal(T.lut_many([f], log_p, 1, n), T.lut(f, log_p, 1, n))                  # one function: lut itself
        v = T.lut_many(fs, log_p, 1, n)                                                                 # v = 2
        assert v.shape == (n,) and v.dtype == np.uint64
        luts = [T.lut(f, log_p, 1, n) for f in fs]
        assert all(int(v[c]) == int(luts[c % 4][c - c % 4]) for c in range(n))
        # after a rotation by a multiple of 4, coefficient i holds f_i of the slot the rotation lands in, negated through the wrap
        p, m, ld = 1 << log_p, n >> log_p, 64 - log_p - 1
        for x in range(2 * p):
            for r in {(x * m) % (2 * n), (x * m + m // 2 - 4) % (2 * n), (x * m - m // 2) % (2 * n)}:    # centre and both edges of slot x
                for i, f in enumerate(fs):
                    c = (r + i) % (2 * n)
                    coeff = int(v[c]) if c < n else (-int(v[c - n])) % (1 << 64)
                    want = (f(x % p) % p) << ld
                    assert coeff == (want if x < p else (-want) % (1 << 64)), (n, x, r, i)
    pair = T.lut_many(fs[:2], 4, 1, 256)
    assert all(int(pair[c]) == int(T.lut(fs[c % 2], 4, 1, 256)[c - c % 2]) for c in range(256))


def _bytes_as_blocks():
    a, b = np.arange(65536) >> 8, np.arange(65536) & 255
    return a, b, [(a >> (2 * i)) & 3 for i in range(4)] + [(b >> (2 * i)) & 3 for i in range(4)]


def test_radix_add_many_plain_model_all_byte_pairs(fhe):
    T = fhe.tfhe_circuit
    a, b, blocks = _bytes_as_blocks()
    bld, _, _, outs = T.radix_add(4, 2, 2, many=True)
    assert len(bld.nodes) == 4 and bld.n_inputs == 8 and len(bld.tables) == 1 and [bld.log_funcs(g) for g in range(4)] == [1, 1, 1, 1]
    assert bld.first_wires() == [8, 10, 12, 14, 16]
    got = bld.evaluate(blocks, 4, 1, outs)
    assert all(int(o.max()) <= 3 and int(o.min()) >= 0 for o in got)
    assert np.array_equal(sum(o.astype(np.int64) << (2 * i) for i, o in enumerate(got)), (a + b) & 255)
    every = bld.evaluate(blocks, 4, 1)                       # every output in wire order: msg_0, carry_0, msg_1, ...
    assert len(every) == 8 and np.array_equal(every[7], (a + b) >> 8) and np.array_equal(every[6], got[3])
    # the same values as the two-table adder, wire for wire
    old, _, _, old_outs = T.radix_add(4, 2, 2)
    assert all(np.array_equal(u, v) for u, v in zip(old.evaluate(blocks, 4, 1), every))
    c = bld.compile(outs, 4, 1, 256)
    assert c.many and c.info() == {"levels": 4, "live_nodes": 4, "max_width": 1}             # 4 blind rotations, against 7
    assert c.info_many() == {"live_outputs": 7, "max_rows": 2} and c.levels() == [1, 2, 3, 4]  # the last carry has no slot
    assert old.compile(old_outs, 4, 1, 256).info() == {"levels": 4, "live_nodes": 7, "max_width": 2}


def test_default_radix_add_is_unchanged(fhe):
    T = fhe.tfhe_circuit
    b, x, y, outs = T.radix_add(4, 2, 2)
    assert len(b.nodes) == 8 and len(b.tables) == 2 and all(callable(f) for f in b.tables)
    assert [(len(t), tab, c) for t, tab, c in b.nodes] == [(2, 0, 0), (2, 1, 0)] + [(3, 0, 0), (3, 1, 0)] * 3
    c = b.compile(outs, 4, 1, 256)
    assert not c.many and c.info_many() == {"live_outputs": 7, "max_rows": 2}
    assert [b._ref(w) for w in outs] == [8, 10, 12, 14]


def test_evaluate_many_node_in_the_padding_half(fhe):
    """output i of a many-LUT node is table_i[x] for x < p and (-table_i[x - p]) mod 2p otherwise"""
    T = fhe.tfhe_circuit
    b = T.Builder()
    i0, i1 = b.input(), b.input()
    f, g = (lambda v: (3 * v + 1) % 16), (lambda v: v >> 1)
    o0, o1 = b.node_many([(i0, 1), (i1, -1)], (f, g), constant=5)
    n1 = b.node([(o1, 4), (i0, 1)], lambda v: v)
    for u in range(16):
        for v in range(16):
            x = (5 + u - v) % 32
            w0, w1 = (f(x), g(x)) if x < 16 else ((-f(x - 16)) % 32, (-g(x - 16)) % 32)
            y = (4 * w1 + u) % 32
            got = b.evaluate([u, v], 4, 1, [o0, o1, n1])
            assert [int(t) for t in got] == [w0, w1, y if y < 16 else (-(y - 16)) % 32], (u, v)
