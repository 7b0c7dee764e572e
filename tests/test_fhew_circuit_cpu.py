"""FHEW gate circuits without a device: the netlist compiler behind fhe_fhew_circuit_create (validation, pruning, levels) and the
builder's `FhewBool` / `FhewU8` arithmetic (scheme/fhew/src/fhew/boolean.rs:134-176, fhew/uint8.rs:50-163) on plain values --
exhaustively: the 65 536 pairs of bytes are evaluated at once, case k in bit k of every wire's value."""
import ctypes as C

import pytest

INVALID = 1  # FHE_ERR_INVALID
NOT = 0x80000000
PAIRS = 1 << 16
ONES = (1 << PAIRS) - 1


def create(fhe, gates, n_inputs, outputs, n_gates=None, n_outputs=None):
    """fhe_fhew_circuit_create on raw arrays -> (status, handle)"""
    from learn_fhe_amd.circuit import _Gate
    arr = (_Gate * max(1, len(gates)))()
    for i, (op, i0, i1, i2) in enumerate(gates):
        arr[i].op = op
        arr[i].inp[0], arr[i].inp[1], arr[i].inp[2] = i0, i1, i2
    outs = (C.c_uint32 * max(1, len(outputs)))(*outputs)
    h = C.c_void_p()
    rc = fhe.lib().fhe_fhew_circuit_create(arr, len(gates) if n_gates is None else n_gates, n_inputs, outs,
                                           len(outputs) if n_outputs is None else n_outputs, C.byref(h))
    return rc, h


def test_validation(fhe):
    lib = fhe.lib()
    AND, MAJ = 0, 6
    ok = [(AND, 0, 1, 0)]
    rc, h = create(fhe, ok, 2, [2])
    assert rc == 0 and h
    lib.fhe_fhew_circuit_destroy(h)
    for gates, n_in, outs in [
        ([(7, 0, 1, 0)], 2, [2]),                 # unknown op
        ([(255, 0, 1, 0)], 2, [2]),
        ([(AND, 0, 2, 0)], 2, [2]),               # a gate reading its own wire
        ([(AND, 0, 3, 0), (AND, 0, 1, 0)], 2, [2]),  # forward reference
        ([(AND, 0, 1 | NOT, 0), (AND, 4 | NOT, 1, 0)], 2, [3]),  # ... under an inversion flag
        ([(MAJ, 0, 1, 9)], 2, [2]),               # the third input of majority counts
        ([(AND, 0, 1, 0)], 2, [3]),               # output out of range
        ([(AND, 0, 1, 0)], 2, [3 | NOT]),
        ([(AND, 0, 1, 0)], 2, []),                # n_outputs == 0
        ([(AND, 0, 0, 0)], 0, [0]),               # n_inputs == 0
    ]:
        rc, h = create(fhe, gates, n_in, outs)
        assert rc == INVALID and not h, (gates, n_in, outs)
    # the two-input ops ignore in[2]
    rc, h = create(fhe, [(AND, 0, 1, 0x7fffffff)], 2, [2])
    assert rc == 0
    lib.fhe_fhew_circuit_destroy(h)
    # more than 2^24 wires: refused before anything is read (2^24 itself is the last admissible count)
    assert create(fhe, [], (1 << 24) + 1, [0])[0] == INVALID
    assert create(fhe, ok, 1 << 24, [0])[0] == INVALID
    rc, h = create(fhe, [], 1 << 24, [(1 << 24) - 1])
    assert rc == 0
    lib.fhe_fhew_circuit_destroy(h)
    assert lib.fhe_fhew_circuit_create(None, 0, 1, None, 1, C.byref(C.c_void_p())) == INVALID
    assert lib.fhe_fhew_circuit_create(None, 0, 1, (C.c_uint32 * 1)(0), 1, None) == INVALID
    # an inverted input as the only output: no gate, no level
    c = fhe.Circuit()
    x = c.input()
    cc = c.compile([~x])
    assert cc.info() == {"levels": 0, "live_gates": 0, "max_width": 0} and cc.levels() == []
    # ... and with gates around that no output needs
    c.and_(x, ~x)
    cc = c.compile([~x])
    assert cc.info() == {"levels": 0, "live_gates": 0, "max_width": 0} and cc.levels() == [0]


def check_level_invariant(c, cc):
    """every live gate sits one above the highest of its inputs (inputs at level 0); a live gate's inputs are live"""
    lv = cc.levels()
    assert len(lv) == len(c.gates)
    for g, (op, ws) in enumerate(c.gates):
        if lv[g] == 0:
            continue
        ins = [0 if w.is_input else lv[w.index] for w in ws]
        assert all(w.is_input or lv[w.index] > 0 for w in ws)
        assert lv[g] == 1 + max(ins), g
    info = cc.info()
    live = [x for x in lv if x]
    assert info["live_gates"] == len(live) and info["levels"] == (max(live) if live else 0)
    assert info["max_width"] == (max(live.count(x) for x in set(live)) if live else 0)
    return lv


def test_levels_and_pruning_of_the_adders(fhe):
    """carry c_i = (a & b) | (t & c_(i-1)) sits at level 2i - 1, sum_7 = t_7 ^ c_7 at level 14 (boolean.rs:145-150, uint8.rs:65-76)"""
    from learn_fhe_amd import circuit as K
    c = fhe.Circuit()
    x, y = c.input_u8(), c.input_u8()
    s, carry = K.u8_overflowing_add(c, x, y)
    assert len(c.gates) == 37
    full = c.compile(s + [carry])
    assert full.info()["live_gates"] == 37 and full.info()["levels"] == 15
    lv = check_level_invariant(c, full)
    assert lv[carry.index] == 15 and lv[s[7].index] == 14 and all(lv)
    wrap = c.compile(s)  # wrapping_add: the last carry's three gates serve no output
    assert wrap.info()["live_gates"] == 34 and wrap.info()["levels"] == 14
    lv = check_level_invariant(c, wrap)
    assert [g for g, x in enumerate(lv) if x == 0] == [34, 35, 36]
    c2 = fhe.Circuit()
    x, y = c2.input_u8(), c2.input_u8()
    out = K.u8_wrapping_add(c2, x, y)
    assert c2.compile(out).info() == wrap.info()


def test_level_invariant_everywhere(fhe):
    from learn_fhe_amd import circuit as K
    for build in (lambda c, x, y: K.u8_wrapping_mul(c, x, y), lambda c, x, y: sum(K.u8_div_rem(c, x, y), []),
                  lambda c, x, y: K.u8_wrapping_sub(c, x, y), lambda c, x, y: K.u8_wrapping_neg(c, x) + [~y[0], y[1], y[1]],
                  lambda c, x, y: [c.select(x[0], x[1], ~y[0]), c.majority(x[0], ~x[1], y[2]), c.xnor(c.nor(x[0], y[0]), c.nand(x[1], ~y[1]))]):
        c = fhe.Circuit()
        x, y = c.input_u8(), c.input_u8()
        check_level_invariant(c, c.compile(build(c, x, y)))


# ---- the builder's arithmetic on plain values ------------------------------------------------------------------------------------

def sliced_inputs():
    """x = k & 255, y = k >> 8 for case k, bit-sliced: the value of input bit i is an int whose bit k is that bit in case k"""
    xs, ys = [0] * 8, [0] * 8
    for i in range(8):
        xs[i] = sum(1 << k for k in range(PAIRS) if (k >> i) & 1)
        ys[i] = sum(1 << k for k in range(PAIRS) if (k >> (8 + i)) & 1)
    return xs, ys


@pytest.fixture(scope="module")
def sliced():
    return sliced_inputs()


def unslice(bits):
    """per case k the integer whose bit i is bit k of bits[i]"""
    cols = [format(b, "0%db" % PAIRS)[::-1] for b in bits]
    return [sum((cols[i][k] == "1") << i for i in range(len(bits))) for k in range(PAIRS)]


def eval_pairs(fhe, build, sliced, extra=()):
    c = fhe.Circuit()
    x, y = c.input_u8(), c.input_u8()
    ex = [c.input() for _ in extra]
    outs = build(c, x, y, *ex)
    vals = c.evaluate_plain(sliced[0] + sliced[1] + [ONES if e else 0 for e in extra], outs, ones=ONES)
    return unslice(vals)


def test_wrapping_add_sub_mul_exhaustive(fhe, sliced):
    from learn_fhe_amd import circuit as K
    for fn, ref in ((K.u8_wrapping_add, lambda x, y: x + y), (K.u8_wrapping_sub, lambda x, y: x - y), (K.u8_wrapping_mul, lambda x, y: x * y)):
        got = eval_pairs(fhe, fn, sliced)
        assert got == [ref(k & 255, k >> 8) & 255 for k in range(PAIRS)], fn.__name__


def test_overflowing_and_carrying_exhaustive(fhe, sliced):
    from learn_fhe_amd import circuit as K
    flat = lambda r: r[0] + [r[1]]  # noqa: E731  9 bits: the byte, then the carry / borrow
    got = eval_pairs(fhe, lambda c, x, y: flat(K.u8_overflowing_add(c, x, y)), sliced)
    assert got == [(k & 255) + (k >> 8) for k in range(PAIRS)]
    got = eval_pairs(fhe, lambda c, x, y: flat(K.u8_overflowing_sub(c, x, y)), sliced)
    assert got == [((k & 255) - (k >> 8)) & 511 for k in range(PAIRS)]
    for cin in (0, 1):
        got = eval_pairs(fhe, lambda c, x, y, ci: flat(K.u8_carrying_add(c, x, y, ci)), sliced, extra=(cin,))
        assert got == [(k & 255) + (k >> 8) + cin for k in range(PAIRS)]
        got = eval_pairs(fhe, lambda c, x, y, bi: flat(K.u8_borrowing_sub(c, x, y, bi)), sliced, extra=(cin,))
        assert got == [((k & 255) - (k >> 8) - cin) & 511 for k in range(PAIRS)]


def test_neg_and_not_all_values(fhe, sliced):
    from learn_fhe_amd import circuit as K
    got = eval_pairs(fhe, lambda c, x, y: K.u8_wrapping_neg(c, x) + K.u8_not(c, x), sliced)
    assert got[:256] == [((-x) & 255) | ((x ^ 255) << 8) for x in range(256)]


def div_rem_formula(x, y):
    """uint8.rs:133-152 transcribed on integers: r gains one bit per step; d = r + (-y) over as many bits as r has, the carry runs on
    through the remaining bits of -y; carry set: r <- d"""
    neg = (-y) & 255
    q = r = 0
    for i in range(8):
        width = i + 1
        r = (r << 1) | ((x >> (7 - i)) & 1)
        d, carry = r, 0
        total = (r & 1) + (neg & 1)
        d, carry = (d & ~1) | (total & 1), total >> 1
        for j in range(1, 8):
            nb = (neg >> j) & 1
            if j < width:
                total = ((r >> j) & 1) + nb + carry
                d, carry = (d & ~(1 << j)) | ((total & 1) << j), total >> 1
            else:
                carry &= nb
        if carry:
            r = d
        q = (q << 1) | carry
    return q, r


def test_div_rem_exhaustive(fhe, sliced):
    from learn_fhe_amd import circuit as K
    got = eval_pairs(fhe, lambda c, x, y: sum(K.u8_div_rem(c, x, y), []), sliced)
    for k in range(PAIRS):
        x, y = k & 255, k >> 8
        q, r = got[k] & 255, got[k] >> 8
        if y:
            assert (q, r) == divmod(x, y), (x, y)
        assert (q, r) == div_rem_formula(x, y), (x, y)  # a zero divisor gives what the reference's circuit gives
    assert div_rem_formula(200, 0) == (got[200] & 255, got[200] >> 8)


def test_bits_and_plain_bools(fhe):
    """boolean.rs:215-223, its truth tables; evaluate_plain on Python bools; every gate type and the inversion flag"""
    from learn_fhe_amd import circuit as K
    F, T = False, True
    tt = {K.bit_overflowing_add: [(F, F), (T, F), (T, F), (F, T)], K.bit_overflowing_sub: [(F, F), (T, F), (T, T), (F, F)],
          K.bit_carrying_add: [(F, F), (T, F), (T, F), (F, T), (T, F), (F, T), (F, T), (T, T)],
          K.bit_borrowing_sub: [(F, F), (T, F), (T, T), (F, F), (T, T), (F, F), (F, T), (T, T)]}
    for fn, table in tt.items():
        k = 2 if len(table) == 4 else 3
        for m in range(1 << k):
            c = fhe.Circuit()
            ws = [c.input() for _ in range(k)]
            assert tuple(c.evaluate_plain([bool((m >> i) & 1) for i in range(k)], list(fn(c, *ws)))) == table[m]
    for m in range(8):
        a, b, d = [bool((m >> i) & 1) for i in range(3)]
        c = fhe.Circuit()
        x, y, z = c.input(), c.input(), c.input()
        outs = [c.and_(x, y), c.nand(x, y), c.or_(x, y), c.nor(x, y), c.xor(x, y), c.xnor(x, y), c.majority(x, y, z), c.not_(x),
                c.select(x, y, z), c.and_(~x, y), c.majority(~x, y, ~z)]
        exp = [a and b, not (a and b), a or b, not (a or b), a != b, a == b, (a + b + d) >= 2, not a, (d if a else b),
               (not a) and b, ((not a) + b + (not d)) >= 2]
        assert c.evaluate_plain([a, b, d], outs) == [bool(e) for e in exp]


def test_netlist_compiler_as_a_host_program(tmp_path):
    """tests/fhew_circuit_host_test.cpp: csrc/fhew_circuit.hpp alone (no HIP, no library) on random netlists against a restatement,
    the slot numbering's invariants, the rejected cases"""
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "fhew_circuit_host_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(here, "fhew_circuit_host_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "fhew_circuit_host_test ok" in out.stdout, out.stdout + out.stderr
