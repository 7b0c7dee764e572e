"""FHEW gate circuits: a builder for netlists of `Fhew` gates (scheme/fhew/src/fhew.rs:27-29, 59-67), the bit and byte arithmetic
of `FhewBool` / `FhewU8` (scheme/fhew/src/fhew/boolean.rs:134-176, fhew/uint8.rs:50-163) gate for gate on top of it, and the
binding of fhe_fhew_circuit_*: a compiled netlist runs in ONE library call, a level of gates across the whole batch at a time.

    c = Circuit()
    x, y = c.input_u8(), c.input_u8()
    add = c.compile(u8_wrapping_add(c, x, y))
    out_a, out_b = add.run(fhew, (in_a, in_b), batch)      # in_a [16][batch][N], in_b [16][batch]
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .ring import _buf, _like

AND, NAND, OR, NOR, XOR, XNOR, MAJORITY = range(7)  # FHE_GATE_*
OP_NAMES = ("and", "nand", "or", "nor", "xor", "xnor", "majority")
WIRE_NOT = 0x80000000  # FHE_WIRE_NOT


class Wire:
    """A reference to a wire of one Circuit: an input or a gate output, possibly inverted (`~w` is free: fhew.rs:27-29)."""
    __slots__ = ("circuit", "is_input", "index", "inverted")

    def __init__(self, circuit, is_input, index, inverted=False):
        self.circuit, self.is_input, self.index, self.inverted = circuit, is_input, index, inverted

    def __invert__(self):
        return Wire(self.circuit, self.is_input, self.index, not self.inverted)

    def __repr__(self):
        return "%s%s%d" % ("~" if self.inverted else "", "in" if self.is_input else "g", self.index)


class _Gate(C.Structure):  # fhe_fhew_gate
    _fields_ = [("op", C.c_uint8), ("pad", C.c_uint8 * 3), ("inp", C.c_uint32 * 3)]


class Circuit:
    """Netlist builder.  Gates are recorded in the order they are made (a topological order by construction)."""

    def __init__(self):
        self.n_inputs = 0
        self.gates = []  # (op, (Wire, ...))

    # ---- wires --------------------------------------------------------------------------------------------------------
    def input(self):
        self.n_inputs += 1
        return Wire(self, True, self.n_inputs - 1)

    def input_u8(self):
        """eight inputs, least significant bit first (fhew/uint8.rs:17-20)"""
        return [self.input() for _ in range(8)]

    def _gate(self, op, *ws):
        for w in ws:
            assert isinstance(w, Wire) and w.circuit is self, "a wire of another circuit"
        self.gates.append((op, ws))
        return Wire(self, False, len(self.gates) - 1)

    def and_(self, a, b): return self._gate(AND, a, b)                  # noqa: E704
    def nand(self, a, b): return self._gate(NAND, a, b)                 # noqa: E704
    def or_(self, a, b): return self._gate(OR, a, b)                    # noqa: E704
    def nor(self, a, b): return self._gate(NOR, a, b)                   # noqa: E704
    def xor(self, a, b): return self._gate(XOR, a, b)                   # noqa: E704
    def xnor(self, a, b): return self._gate(XNOR, a, b)                 # noqa: E704
    def majority(self, a, b, c): return self._gate(MAJORITY, a, b, c)   # noqa: E704

    @staticmethod
    def not_(a):
        return ~a

    def select(self, c, f, t):
        """fhew/boolean.rs:135-137: (!c & f) | (c & t)"""
        return self.or_(self.and_(~c, f), self.and_(c, t))

    # ---- the netlist in the library's numbering -----------------------------------------------------------------------
    def _ref(self, w):
        return (w.index if w.is_input else self.n_inputs + w.index) | (WIRE_NOT if w.inverted else 0)

    def netlist(self, outputs):
        """-> (gates [(op, in0, in1, in2)], outputs [ref]): wire w < n_inputs is input w, wire n_inputs + g gate g"""
        gates = [(op,) + tuple(self._ref(w) for w in ws) + (0,) * (3 - len(ws)) for op, ws in self.gates]
        return gates, [self._ref(w) for w in outputs]

    def compile(self, outputs):
        return CompiledCircuit(self, list(outputs))

    # ---- evaluation without the library -------------------------------------------------------------------------------
    def evaluate(self, inputs, outputs, ops):
        """The netlist gate by gate over any value type: ops.and_ .. ops.majority and ops.not_ (every gate, dead ones included)."""
        assert len(inputs) == self.n_inputs
        vals = []

        def get(w):
            v = inputs[w.index] if w.is_input else vals[w.index]
            return ops.not_(v) if w.inverted else v

        fns = (ops.and_, ops.nand, ops.or_, ops.nor, ops.xor, ops.xnor, ops.majority)
        for op, ws in self.gates:
            vals.append(fns[op](*[get(w) for w in ws]))
        return [get(w) for w in outputs]

    def evaluate_plain(self, bits, outputs, ones=1):
        """The netlist on plain values.  ones = 1: Python bools in, bools out.  A wider `ones` mask evaluates that many cases at once:
        every value is an int whose bit k belongs to case k (inversion = xor with `ones`)."""
        outs = self.evaluate([int(b) for b in bits], outputs, _PlainOps(ones))
        return [bool(v) for v in outs] if ones == 1 else outs

    def evaluate_fhew(self, fhew, inputs, outputs):
        """The netlist one gate bootstrap after the other through ring.Fhew (what a compiled circuit replaces): inputs and results
        are (a [batch][N], b [batch]) pairs."""
        return self.evaluate(list(inputs), outputs, fhew)


class _PlainOps:
    def __init__(self, ones):
        self.ones = ones

    def not_(self, a): return a ^ self.ones                                     # noqa: E704
    def and_(self, a, b): return a & b                                          # noqa: E704
    def nand(self, a, b): return (a & b) ^ self.ones                            # noqa: E704
    def or_(self, a, b): return a | b                                           # noqa: E704
    def nor(self, a, b): return (a | b) ^ self.ones                             # noqa: E704
    def xor(self, a, b): return a ^ b                                           # noqa: E704
    def xnor(self, a, b): return a ^ b ^ self.ones                              # noqa: E704
    def majority(self, a, b, c): return (a & b) | (b & c) | (c & a)             # noqa: E704


class CompiledCircuit:
    """fhe_fhew_circuit: the netlist validated, pruned to the gates an output depends on, and levelled."""

    def __init__(self, circuit: Circuit, outputs):
        self.circuit, self.outputs = circuit, outputs
        gates, outs = circuit.netlist(outputs)
        self.n_inputs, self.n_gates, self.n_outputs = circuit.n_inputs, len(gates), len(outs)
        arr = (_Gate * max(1, len(gates)))()
        for i, (op, i0, i1, i2) in enumerate(gates):
            arr[i].op = op
            arr[i].inp[0], arr[i].inp[1], arr[i].inp[2] = i0, i1, i2
        oarr = (C.c_uint32 * max(1, len(outs)))(*outs)
        self._h = C.c_void_p()
        L.check(L.lib().fhe_fhew_circuit_create(arr, len(gates), circuit.n_inputs, oarr, len(outs), C.byref(self._h)), "fhe_fhew_circuit_create")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and L is not None and getattr(L, "lib", None):  # (module globals are gone at interpreter shutdown)
            L.lib().fhe_fhew_circuit_destroy(h)

    @property
    def handle(self):
        return self._h

    def info(self):
        lv, live, width = C.c_size_t(), C.c_size_t(), C.c_size_t()
        L.check(L.lib().fhe_fhew_circuit_info(self._h, C.byref(lv), C.byref(live), C.byref(width)), "fhe_fhew_circuit_info")
        return {"levels": lv.value, "live_gates": live.value, "max_width": width.value}

    def levels(self):
        """level of every gate of the netlist, 0 = dropped"""
        out = (C.c_uint32 * max(1, self.n_gates))()
        L.check(L.lib().fhe_fhew_circuit_levels(self._h, out), "fhe_fhew_circuit_levels")
        return list(out)[:self.n_gates]

    def run(self, fhew, inputs, batch):
        """fhe_fhew_circuit_run with the keys of a ring.Fhew.  inputs = (in_a [n_inputs][batch][N], in_b [n_inputs][batch]), numpy
        uint64 (host path) or CUDA tensors (device path: asynchronous, fhew.bk.check() reports the data-dependent conditions)
        -> (out_a [n_outputs][batch][N], out_b [n_outputs][batch])."""
        in_a, in_b = inputs
        n = fhew.n
        pa, cnt, mem, st = _buf(in_a)
        pb, cntb, _, _ = _buf(in_b)
        assert cnt == self.n_inputs * batch * n and cntb == self.n_inputs * batch
        pka, _, kmem, _ = _buf(fhew.ksk_a)
        pkb, _, _, _ = _buf(fhew.ksk_b)
        assert kmem == mem, "keys and ciphertexts in the same kind of memory"
        out_a, out_b = _like(in_a, (self.n_outputs, batch, n)), _like(in_a, (self.n_outputs, batch))
        poa, _, _, _ = _buf(out_a)
        pob, _, _, _ = _buf(out_b)
        L.check(L.lib().fhe_fhew_circuit_run(self._h, fhew.bk._h, fhew.q_ks, fhew.ks_log_b, fhew.ks_d, pka, pkb, pa, pb, poa, pob, batch, mem, st),
                "fhe_fhew_circuit_run")
        return out_a, out_b


# ---- FhewBool arithmetic, gate for gate (fhew/boolean.rs:139-163): every function returns (result, carry or borrow) -------------

def bit_overflowing_add(c, a, b):
    return c.xor(a, b), c.and_(a, b)


def bit_carrying_add(c, a, b, carry):
    t = c.xor(a, b)
    s = c.xor(t, carry)
    return s, c.or_(c.and_(a, b), c.and_(t, carry))


def bit_overflowing_sub(c, a, b):
    return c.xor(a, b), c.and_(~a, b)


def bit_borrowing_sub(c, a, b, borrow):
    t = c.xor(a, b)
    d = c.xor(t, borrow)
    return d, c.or_(c.and_(~a, b), c.and_(~t, borrow))


# ---- FhewU8 arithmetic, gate for gate (fhew/uint8.rs:33-163): a byte is a list of 8 wires, least significant first --------------

def u8_not(c, x):
    return [~b for b in x]


def u8_wrapping_neg(c, x):
    """uint8.rs:51-63"""
    carry = ~x[0]
    out = [x[0]]
    for i in range(1, 8):
        s, carry = bit_overflowing_add(c, ~x[i], carry)
        out.append(s)
    return out


def u8_overflowing_add(c, x, y):
    """uint8.rs:65-76 -> (sum, carry)"""
    out, carry = [], None
    for i in range(8):
        s, carry = bit_carrying_add(c, x[i], y[i], carry) if carry is not None else bit_overflowing_add(c, x[i], y[i])
        out.append(s)
    return out, carry


def u8_carrying_add(c, x, y, carry):
    """uint8.rs:78-86 -> (sum, carry)"""
    out = []
    for i in range(8):
        s, carry = bit_carrying_add(c, x[i], y[i], carry)
        out.append(s)
    return out, carry


def u8_wrapping_add(c, x, y):
    return u8_overflowing_add(c, x, y)[0]


def u8_overflowing_sub(c, x, y):
    """uint8.rs:92-103 -> (difference, borrow)"""
    out, borrow = [], None
    for i in range(8):
        d, borrow = bit_borrowing_sub(c, x[i], y[i], borrow) if borrow is not None else bit_overflowing_sub(c, x[i], y[i])
        out.append(d)
    return out, borrow


def u8_borrowing_sub(c, x, y, borrow):
    """uint8.rs:105-113 -> (difference, borrow)"""
    out = []
    for i in range(8):
        d, borrow = bit_borrowing_sub(c, x[i], y[i], borrow)
        out.append(d)
    return out, borrow


def u8_wrapping_sub(c, x, y):
    return u8_overflowing_sub(c, x, y)[0]


def u8_wrapping_mul(c, x, y):
    """uint8.rs:119-131: column i sums the partial products x[j] & y[i - j] (made lazily, one in front of each addition) through the
    running carries of the columns before it"""
    carries = [None] * 7
    out = []
    for i in range(8):
        s = c.and_(x[0], y[i])
        for j in range(1, i + 1):
            tj = c.and_(x[j], y[i - j])
            if carries[j - 1] is not None:
                s, carries[j - 1] = bit_carrying_add(c, s, tj, carries[j - 1])
            else:
                s, carries[j - 1] = bit_overflowing_add(c, s, tj)
        out.append(s)
    return out


def u8_div_rem(c, x, y):
    """uint8.rs:133-152: restoring division, the remainder growing one bit per step -> (quotient, remainder)"""
    neg = u8_wrapping_neg(c, y)
    q, r = [], []
    for i in range(8):
        r.insert(0, x[7 - i])
        d = list(r)
        d[0], carry = bit_overflowing_add(c, d[0], neg[0])
        for j in range(1, 8):
            if j < len(d):
                d[j], carry = bit_carrying_add(c, d[j], neg[j], carry)
            else:
                carry = c.and_(carry, neg[j])
        r = [c.select(carry, rk, dk) for rk, dk in zip(r, d)]
        q.insert(0, carry)
    return q, r
