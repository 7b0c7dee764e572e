"""TFHE look-up-table circuits: a builder for netlists of programmable bootstraps (scheme/tfhe/src/bootstrapping.rs:78-82 through the
tables of 118-128) over free TLWE arithmetic (tlwe.rs:22-75), radix integers of message + carry blocks, bivariate functions and
comparisons on top of it, and the binding of fhe_tfhe_circuit_*: a compiled netlist runs in ONE library call, a level of nodes across
the whole batch at a time, every job through the table of its node.

    b, x, y, outs = radix_add(4, 2, 2)                      # two bytes as 4 blocks of 2 message + 2 carry bits
    add = b.compile(outs, log_p=4, padding=1, n=1024)
    out_a, out_b = add.run(key, ks_log_b, ks_d, ksk_a, ksk_b, (in_a, in_b), batch)   # in_a [8][batch][n_lwe], in_b [8][batch]

Messages live in Z_p, p = 2^log_p, under `padding` = 1 extra bit: a phase is a value x of Z_2p times 2^(64 - log_p - 1).  A node computes
x = constant + sum weight * wire over Z_2p and bootstraps it: table[x] for x < p and, the test polynomial being negacyclic,
-table[x - p] when the sum lands in the padding half.

A many-LUT node (Builder.node_many, radix_add(..., many=True)) serves 2^v functions of the same sum from ONE blind rotation
(PBSmanyLUT): the sum is mod-switched to multiples of 2^v, the node's table interleaves the functions' tables (lut_many) and outputs
0 .. 2^v - 1 are extracted.  The mod-switch drift grows by 2^v: with a binary key of dimension n_lwe the worst case is
2^v (n_lwe + 1) / 2 of 2n positions and must stay below the half-slot n / 2p -- the caller's condition.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .ring import _buf, _like

MAX_TERMS = 16


def table_values(f, log_p):
    """the p values of a function table: f over Z_p, reduced mod p"""
    p = 1 << log_p
    return [int(f(v)) % p for v in range(p)]


def lut(f, log_p, padding, n):
    """bootstrapping.rs:118-128 `table(log_p, big_n, f)` encoded as `Tglwe::encode` does (tglwe.rs:80-84, tlwe.rs:113-116: value <<
    log_delta): table[0] on the first n / 2p coefficients, every further value on n / p, -table[0] on the last n / 2p.
    The negation is taken ON THE TORUS, -(table[0] << log_delta), where the reference negates in Z_p first: the two differ in the
    padding bit alone, so they decode alike (tlwe.rs:134-142 reads mod p).  A phase of 0 whose noise is negative reads the last
    coefficients through the negacyclic wrap: with the torus negation it yields table[0] itself, with the Z_p one table[0] + p -- a
    set padding bit that decoding drops but the next node of a circuit would add into its sum.
    -> [n] uint64"""
    p, log_delta = 1 << log_p, 64 - (log_p + padding)
    m = n >> log_p
    assert m >= 2 and m << log_p == n, "n / p must be an even count of coefficients per value"
    tt = table_values(f, log_p)
    vals = [tt[0]] * (m // 2)
    for x in tt[1:]:
        vals += [x] * m
    vals += [-tt[0]] * (m // 2)
    return np.array([(x << log_delta) % (1 << 64) for x in vals], dtype=np.uint64)


def lut_many(fs, log_p, padding, n):
    """The test polynomial of a many-LUT bootstrap (PBSmanyLUT): 2^v = len(fs) functions served by ONE blind rotation.  With L_i =
    lut(fs[i], ...), coefficient c is L_{c mod 2^v}[c - (c mod 2^v)]: after a rotation by a multiple of 2^v (mod_switch_many), coefficient i
    holds fs[i] of the message, negated on the torus through the negacyclic wrap exactly as lut does.  n / 2p must be a multiple of 2^v.
    One function: lut itself.  -> [n] uint64"""
    funcs = len(fs)
    assert funcs >= 1 and funcs & (funcs - 1) == 0 and funcs <= 16, "1, 2, 4, 8 or 16 functions"
    assert (n >> (log_p + 1)) % funcs == 0 and n >> (log_p + 1), "n / 2p must be a multiple of the number of functions"
    luts = [lut(f, log_p, padding, n) for f in fs]
    c = np.arange(n)
    return np.stack(luts)[c % funcs, c - c % funcs]


class Wire:
    """A reference to a wire of one Builder: an input or output `out` of a node (0 unless the node is a many-LUT node)."""
    __slots__ = ("builder", "is_input", "index", "out")

    def __init__(self, builder, is_input, index, out=0):
        self.builder, self.is_input, self.index, self.out = builder, is_input, index, out

    def __repr__(self):
        return "%s%d%s" % ("in" if self.is_input else "n", self.index, ".%d" % self.out if self.out else "")


class _Term(C.Structure):  # fhe_tfhe_term
    _fields_ = [("wire", C.c_uint32), ("weight", C.c_int32)]


class _Node(C.Structure):  # fhe_tfhe_node
    _fields_ = [("first_term", C.c_uint32), ("n_terms", C.c_uint32), ("constant", C.c_uint64), ("table", C.c_uint32), ("pad", C.c_uint32)]


class Builder:
    """Netlist builder.  Nodes are recorded in the order they are made (a topological order by construction); tables are functions
    over Z_p, numbered in the order they are registered (the same function object is registered once)."""

    def __init__(self):
        self.n_inputs = 0
        self.nodes = []   # (terms [(Wire, weight)], table index, constant in message units)
        self.tables = []  # functions over Z_p

    def input(self):
        self.n_inputs += 1
        return Wire(self, True, self.n_inputs - 1)

    def table(self, f):
        for i, g in enumerate(self.tables):
            if g is f:
                return i
        self.tables.append(f)
        return len(self.tables) - 1

    def node(self, terms, table, constant=0):
        """bootstrap(table, constant + sum weight * wire); terms: (Wire, weight) pairs; table: an index from table() or a function;
        constant: in message units (an element of Z_2p)."""
        terms = [(w, int(k)) for w, k in terms]
        for w, _ in terms:
            assert isinstance(w, Wire) and w.builder is self, "a wire of another builder"
        if callable(table):
            table = self.table(table)
        self.nodes.append((terms, int(table), int(constant)))
        return Wire(self, False, len(self.nodes) - 1)

    def table_many(self, fs):
        """registers the functions of one many-LUT node as ONE table (a tuple; the same function objects in the same order: once)"""
        fs = tuple(fs)
        for i, g in enumerate(self.tables):
            if isinstance(g, tuple) and len(g) == len(fs) and all(a is b for a, b in zip(g, fs)):
                return i
        self.tables.append(fs)
        return len(self.tables) - 1

    def node_many(self, terms, fs, constant=0):
        """ONE bootstrap that yields fs[0](x), fs[1](x), ... of x = constant + sum weight * wire: a many-LUT node (len(fs) = 2^v <= 16
        functions, one interleaved table, one blind rotation).  The mod-switch drift is 2^v times that of node().  -> list of wires"""
        fs = tuple(fs)
        assert len(fs) in (1, 2, 4, 8, 16)
        w0 = self.node(terms, self.table_many(fs), constant)
        return [Wire(self, False, w0.index, i) for i in range(len(fs))]

    def log_funcs(self, g):
        """v of node g: 0 for a node(), log2 of the number of functions of a node_many()"""
        f = self.tables[self.nodes[g][1]]
        return len(f).bit_length() - 1 if isinstance(f, tuple) else 0

    def first_wires(self):
        """[n_nodes + 1]: the netlist wire of every node's output 0 (node g owns 2^v_g consecutive wires); last = number of wires"""
        out, w = [], self.n_inputs
        for g in range(len(self.nodes)):
            out.append(w)
            w += 1 << self.log_funcs(g)
        return out + [w]

    def _ref(self, w, first=None):
        return w.index if w.is_input else (first or self.first_wires())[w.index] + w.out

    def compile(self, outputs, log_p, padding, n):
        return CompiledTfheCircuit(self, list(outputs), log_p, padding, n)

    # ---- evaluation without the library -------------------------------------------------------------------------------------
    def evaluate(self, inputs, log_p, padding, outputs=None):
        """The plain-value model: inputs are integers or numpy integer arrays (one case per element), read mod 2p.  Every wire carries
        an element of Z_2p (message + padding bit); a node yields table[x] for a sum x < p and (-table[x - p]) mod 2p for x >= p; output
        i of a many-LUT node yields the same through the table of its function i.
        -> the values of `outputs` (default: every output of every node, in wire order), elements of Z_2p."""
        assert padding == 1 and len(inputs) == self.n_inputs
        p = 1 << log_p
        ins = [np.asarray(v, dtype=np.int64) % (2 * p) for v in inputs]
        tabs = [[np.array(table_values(g, log_p), dtype=np.int64) for g in (f if isinstance(f, tuple) else (f,))] for f in self.tables]
        vals = []

        def get(w):
            return ins[w.index] if w.is_input else vals[w.index][w.out]

        for terms, table, constant in self.nodes:
            x = np.int64(constant)
            for w, k in terms:
                x = x + k * get(w)
            x = x % (2 * p)
            vals.append([np.where(x < p, tab[x % p], (-tab[x % p]) % (2 * p)) for tab in tabs[table]])
        if outputs is None:
            outputs = [Wire(self, False, g, i) for g in range(len(self.nodes)) for i in range(1 << self.log_funcs(g))]
        return [get(w) for w in outputs]


class CompiledTfheCircuit:
    """fhe_tfhe_circuit: the netlist validated, pruned to the nodes an output depends on, and levelled; with its encoded tables."""

    def __init__(self, builder: Builder, outputs, log_p, padding, n):
        self.builder, self.outputs, self.log_p, self.padding, self.n = builder, outputs, log_p, padding, n
        log_delta = 64 - (log_p + padding)
        fw = builder.first_wires()
        flat = [(builder._ref(w, fw), k) for terms, _, _ in builder.nodes for w, k in terms]
        tarr = (_Term * max(1, len(flat)))()
        for i, (w, k) in enumerate(flat):
            tarr[i].wire, tarr[i].weight = w, k
        narr = (_Node * max(1, len(builder.nodes)))()
        first = 0
        self.log_funcs = [builder.log_funcs(g) for g in range(len(builder.nodes))]
        for i, (terms, table, constant) in enumerate(builder.nodes):
            narr[i].first_term, narr[i].n_terms, narr[i].table = first, len(terms), table
            narr[i].constant = ((constant % (2 << log_p)) << log_delta) % (1 << 64)
            narr[i].pad = self.log_funcs[i]            # fhe_tfhe_node_many's log_funcs
            first += len(terms)
        outs = [builder._ref(w, fw) for w in outputs]
        oarr = (C.c_uint32 * max(1, len(outs)))(*outs)
        self.n_inputs, self.n_nodes, self.n_outputs, self.n_tables = builder.n_inputs, len(builder.nodes), len(outs), len(builder.tables)
        self.tables = (np.stack([lut_many(f, log_p, padding, n) if isinstance(f, tuple) else lut(f, log_p, padding, n) for f in builder.tables])
                       if builder.tables else np.zeros((0, n), dtype=np.uint64))
        self._h = C.c_void_p()
        self.many = any(self.log_funcs)                # a many-LUT node anywhere: the create that reads log_funcs
        create = L.lib().fhe_tfhe_circuit_create_many if self.many else L.lib().fhe_tfhe_circuit_create
        L.check(create(narr, len(builder.nodes), tarr, len(flat), builder.n_inputs, self.n_tables, oarr, len(outs), C.byref(self._h)),
                "fhe_tfhe_circuit_create_many" if self.many else "fhe_tfhe_circuit_create")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and L is not None and getattr(L, "lib", None):  # (module globals are gone at interpreter shutdown)
            L.lib().fhe_tfhe_circuit_destroy(h)

    @property
    def handle(self):
        return self._h

    def info(self):
        lv, live, width = C.c_size_t(), C.c_size_t(), C.c_size_t()
        L.check(L.lib().fhe_tfhe_circuit_info(self._h, C.byref(lv), C.byref(live), C.byref(width)), "fhe_tfhe_circuit_info")
        return {"levels": lv.value, "live_nodes": live.value, "max_width": width.value}

    def info_many(self):
        """fhe_tfhe_circuit_info_many: live outputs (rows of the wire table) and those of the level that has most (key-switch rows per
        ciphertext of the batch); equal to info()'s live_nodes and max_width without many-LUT nodes"""
        live, rows = C.c_size_t(), C.c_size_t()
        L.check(L.lib().fhe_tfhe_circuit_info_many(self._h, C.byref(live), C.byref(rows)), "fhe_tfhe_circuit_info_many")
        return {"live_outputs": live.value, "max_rows": rows.value}

    def levels(self):
        """level of every node of the netlist, 0 = dropped"""
        out = (C.c_uint32 * max(1, self.n_nodes))()
        L.check(L.lib().fhe_tfhe_circuit_levels(self._h, out), "fhe_tfhe_circuit_levels")
        return list(out)[:self.n_nodes]

    def run(self, key, ks_log_b, ks_d, ksk_a, ksk_b, inputs, batch, tables=None):
        """fhe_tfhe_circuit_run under a ring.TggswKey.  inputs = (in_a [n_inputs][batch][n_lwe], in_b [n_inputs][batch]), numpy uint64
        (host path) or CUDA tensors (device path, asynchronous); tables: the encoded tables in the same kind of memory (default: this
        circuit's own, uploaded when the inputs are tensors) -> (out_a [n_outputs][batch][n_lwe], out_b [n_outputs][batch])."""
        return run_circuit(self._h, self.n_inputs, self.n_outputs, self.tables if tables is None else tables, key, ks_log_b, ks_d, ksk_a, ksk_b,
                           inputs, batch)

    def run_nodes(self, key, ks_log_b, ks_d, ksk_a, ksk_b, inputs, batch, tables=None):
        """The same netlist one node after the other through ring.tlwe_lincomb and TggswKey.bootstrap (what a compiled circuit
        replaces; every node, dead ones included).  Same arguments and result as run()."""
        from .ring import tlwe_lincomb
        in_a, in_b = inputs
        tables = _same_memory(self.tables if tables is None else tables, in_a)
        log_delta = 64 - (self.log_p + self.padding)
        b = self.builder
        vals = []

        def get(w):
            return (in_a[w.index], in_b[w.index]) if w.is_input else vals[w.index][w.out]

        for g, (terms, table, constant) in enumerate(b.nodes):
            s = tlwe_lincomb([k for _, k in terms], [get(w) for w, _ in terms], ((constant % (2 << self.log_p)) << log_delta) % (1 << 64))
            if not self.log_funcs[g]:
                vals.append([key.bootstrap(ks_log_b, ks_d, ksk_a, ksk_b, tables[table], s[0], s[1])])
                continue
            # a many-LUT node: one call, every ciphertext through the node's interleaved table
            oa, ob = key.bootstrap_many(ks_log_b, ks_d, ksk_a, ksk_b, tables, _table_of(table, batch, in_a), self.log_funcs[g], s[0], s[1])
            if isinstance(oa, np.ndarray):
                vals.append([(np.ascontiguousarray(oa[:, i]), np.ascontiguousarray(ob[:, i])) for i in range(1 << self.log_funcs[g])])
            else:
                vals.append([(oa[:, i].contiguous(), ob[:, i].contiguous()) for i in range(1 << self.log_funcs[g])])
        outs = [get(w) for w in self.outputs]
        if isinstance(in_a, np.ndarray):
            return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
        import torch
        return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


def _same_memory(tables, like):
    if isinstance(like, np.ndarray) or not isinstance(tables, np.ndarray):
        return tables
    import torch
    return torch.from_numpy(np.ascontiguousarray(tables).view(np.int64)).to(like.device)


def _table_of(table, batch, like):
    """[batch] copies of one table index in the memory of `like`"""
    if isinstance(like, np.ndarray):
        return np.full(batch, table, dtype=np.uint32)
    import torch
    return torch.full((batch,), table, dtype=torch.int32, device=like.device)


def run_circuit(handle, n_inputs, n_outputs, tables, key, ks_log_b, ks_d, ksk_a, ksk_b, inputs, batch):
    in_a, in_b = inputs
    n_lwe = key.count
    tables = _same_memory(tables, in_a)
    pa, cnt, mem, st = _buf(in_a)
    pb, cntb, _, _ = _buf(in_b)
    assert cnt == n_inputs * batch * n_lwe and cntb == n_inputs * batch
    pka, _, kmem, _ = _buf(ksk_a)
    pt, _, tmem, _ = _buf(tables)
    assert kmem == mem and tmem == mem, "keys, tables and ciphertexts in the same kind of memory"
    out_a, out_b = _like(in_a, (n_outputs, batch, n_lwe)), _like(in_a, (n_outputs, batch))
    L.check(L.lib().fhe_tfhe_circuit_run(handle, key.t.handle, key._h, ks_log_b, ks_d, pka, _buf(ksk_b)[0], pt, pa, pb, _buf(out_a)[0],
                                         _buf(out_b)[0], batch, mem, st), "fhe_tfhe_circuit_run")
    return out_a, out_b


# ---- arithmetic in the style of bootstrapping.rs:141-165: one table per function, message + carry blocks --------------------------

def radix_add(blocks, msg_bits, carry_bits, b=None, x=None, y=None, many=False):
    """x + y over `blocks` blocks of msg_bits message bits under carry_bits of head room (log_p = msg_bits + carry_bits), least
    significant block first: per block one message table and one carry table of x_i + y_i + carry_{i-1}.  The last block's carry is
    emitted like the others (no output names it: create drops it).  b: the builder to extend (default: a new one); x, y: lists of
    wires (default: fresh inputs, x first).  many: ONE many-LUT node (message, carry) per block instead of two nodes -- `blocks` blind
    rotations instead of 2 blocks - 1, at twice the mod-switch drift (node_many).  -> (builder, x, y, message wires)"""
    mask = (1 << msg_bits) - 1
    assert 2 * mask + 1 < (1 << (msg_bits + carry_bits)), "x_i + y_i + carry must stay below p"
    b = Builder() if b is None else b
    x = [b.input() for _ in range(blocks)] if x is None else x
    y = [b.input() for _ in range(blocks)] if y is None else y
    f_msg, f_carry = _fn("msg%d" % msg_bits, lambda v: v & mask), _fn("carry%d" % msg_bits, lambda v: v >> msg_bits)
    outs, carry = [], None
    if many:
        for i in range(blocks):
            msg, carry = b.node_many([(x[i], 1), (y[i], 1)] + ([(carry, 1)] if carry is not None else []), (f_msg, f_carry))
            outs.append(msg)
        return b, x, y, outs
    t_msg, t_carry = b.table(f_msg), b.table(f_carry)
    for i in range(blocks):
        terms = [(x[i], 1), (y[i], 1)] + ([(carry, 1)] if carry is not None else [])
        outs.append(b.node(terms, t_msg))
        carry = b.node(terms, t_carry)
    return b, x, y, outs


_FNS = {}


def _fn(name, f):
    """one function object per name, so that Builder.table() registers a table once however often an arithmetic helper runs"""
    return _FNS.setdefault(name, f)


def bivariate(f, msg_bits, b=None, x=None, y=None, name=None):
    """f(x, y) of two msg_bits-bit wires in ONE bootstrap: the sum 2^msg_bits x + y (weights 2^msg_bits and 1) through the table
    v -> f(v >> msg_bits, v & mask); needs log_p >= 2 msg_bits.  -> (builder, x, y, wire)"""
    mask = (1 << msg_bits) - 1
    b = Builder() if b is None else b
    x = b.input() if x is None else x
    y = b.input() if y is None else y
    g = lambda v: f(v >> msg_bits, v & mask)  # noqa: E731
    return b, x, y, b.node([(x, 1 << msg_bits), (y, 1)], _fn(name, g) if name else g)


def radix_eq(blocks, msg_bits, b=None, x=None, y=None):
    """x == y over `blocks` blocks: one equality flag per block (bivariate), then one table on their sum (blocks < p).
    -> (builder, x, y, wire)"""
    b = Builder() if b is None else b
    x = [b.input() for _ in range(blocks)] if x is None else x
    y = [b.input() for _ in range(blocks)] if y is None else y
    flags = [bivariate(lambda u, v: int(u == v), msg_bits, b, x[i], y[i], name="eq%d" % msg_bits)[3] for i in range(blocks)]
    return b, x, y, b.node([(w, 1) for w in flags], _fn("all%d" % blocks, lambda v: int(v == blocks)))
