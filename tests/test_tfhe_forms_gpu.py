"""Every form a prepared fhe_tggsw_key can take (csrc/torus_forms.hpp: Form60, Form30 unpacked and packed, FormF fft64 and x3) at every ring
size N = 256 .. 2048, each against the exact oracle (oracle/cref.py) bit for bit: the external product, the blind rotation with one table
and with a table per ciphertext, and the table look-up (one tree level plus the ladder from the accumulators; the ladder from the shared
polynomials), with and without its key switch.  The cells are the table CELLS; every test first asks the key which form it took
(fhe_tggsw_key_form), so a change of the host's rule fails here instead of silently moving a cell to another kernel.  Batches are chosen so
that the one-wave teams (four to a workgroup) leave idle teams behind the team set-up."""
import functools

import numpy as np
import pytest

import tfhe_lut_model as M

LOG_NS = (8, 9, 10, 11)

# (form, packs digits, log_n, log_b, d, NO_F64_EXACT set while the key is made), each derived from the rule in fhe_tggsw_prepare:
#   bound_bits = ilog2(2d) + 1 + log_n + 62 + log_b: > 88 two 60-bit primes, else three 30-bit primes; in front of both, x3 where
#   2d N 2^log_b <= 2^21, log_b <= 7, log_n <= 10 and the lab switch NO_F64_EXACT is off; a 30-bit key packs digits where log_b <= 7, 2d <= 8
CELLS = (
    # two 60-bit primes: (23, 1), bound_bits = 87 + log_n > 88
    [("60", 0, ln, 23, 1, False) for ln in LOG_NS]
    # three 30-bit primes, unpacked by rule: (10, 2), bound_bits = 75 + log_n <= 88; log_b > 7 excludes x3 and packing
    + [("30", 0, ln, 10, 2, False) for ln in LOG_NS]
    # three 30-bit primes, packed: (7, 3) is x3 by default up to log_n = 10: NO_F64_EXACT; at log_n = 11 no switch is needed; (7, 4): 2d = 8,
    # the largest packed gadget and the largest LDS carve-up (four one-wave teams at log_n = 9, one team of four waves at log_n = 11)
    + [("30", 1, ln, 7, 3, True) for ln in (8, 9, 10)] + [("30", 1, 11, 7, 2, False), ("30", 1, 9, 7, 4, True), ("30", 1, 11, 7, 4, False)]
    # three key pieces through f64 transforms: (7, 3), 6 N 2^7 <= 2^21 up to log_n = 10 (the host never picks it at log_n = 11)
    + [("x3", 0, ln, 7, 3, False) for ln in (8, 9, 10)]
    # fft64: (6, 3) with key words below 2^10 in magnitude: every partial sum is an integer below 2^53, the mode is exact
    + [("fft64", 0, ln, 6, 3, False) for ln in LOG_NS]
)
CELL_IDS = ["%s%s-n%d-b%dd%d" % (c[0], "pk" if c[1] else "", 1 << c[2], c[3], c[4]) for c in CELLS]
cells = pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
gpu = pytest.mark.gpu

KS = (4, 3, 8)  # the look-up's key switch: (log_b, d, n_lwe_out), the small shape of test_tfhe_lut_gpu.py::test_bit_identity_with_the_chain


def test_the_table_covers_every_form_at_every_ring_size():
    """five form variants x log_n 8 .. 11, less x3 at log_n = 11 (fhe_tggsw_prepare asks log_n <= 10 of it): nothing else may be absent"""
    variants = [("60", 0), ("30", 0), ("30", 1), ("x3", 0), ("fft64", 0)]
    want = {(f, p, ln) for f, p in variants for ln in LOG_NS} - {("x3", 0, 11)}
    assert len(want) == 19
    assert {(c[0], c[1], c[2]) for c in CELLS} == want
    assert len(set(CELLS)) == len(CELLS) and len(set(CELL_IDS)) == len(CELLS)
    assert ("30", 1, 9, 7, 4, True) in CELLS and ("30", 1, 11, 7, 4, False) in CELLS     # 2d = 8 on both team shapes
    for form, packed, ln, log_b, d, no_f64 in CELLS:                                      # the rule, restated once: the device confirms it
        bound_bits = (2 * d).bit_length() - 1 + 1 + ln + 62 + log_b
        x3 = (2 * d) << (ln + log_b) <= 1 << 21 and log_b <= 7 and log_b * d <= 31 and 2 * d <= 16 and ln <= 10 and not no_f64
        rule = "fft64" if form == "fft64" else "x3" if x3 else "30" if bound_bits <= 88 and log_b <= 28 else "60"
        assert rule == form and packed == int(rule == "30" and log_b <= 7 and 2 * d <= 8), (form, ln, log_b, d)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def host(t):
    return t.cpu().numpy().view(np.uint64)


def r64(rng, *shape):
    return rng.integers(0, 1 << 63, size=shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)


def extreme_digits(log_b, d):
    """the torus value whose every digit is -2^(log_b - 1), the most negative balanced digit (test_torus_gpu.py)"""
    half = 1 << (log_b - 1)
    return np.uint64((-sum(half << (64 - log_b * (j + 1)) for j in range(d))) % (1 << 64))


@functools.lru_cache(maxsize=None)
def key_rows(cell, count, salt):
    """rows_a, rows_b [count][2d][n]: uniform 64-bit words, row 0 of entry 1 all -2^63 (fft64: words in [-2^10, 2^10), that row all -2^10).
    Made once per (cell, use) and left unchanged."""
    form, _, log_n, log_b, d, _ = cell
    n = 1 << log_n
    rng = np.random.Generator(np.random.PCG64([9100, salt, log_n, log_b, d, CELLS.index(cell)]))
    if form == "fft64":
        ra = rng.integers(-(1 << 10), 1 << 10, size=(count, 2 * d, n), dtype=np.int64).view(np.uint64)
        rb = rng.integers(-(1 << 10), 1 << 10, size=(count, 2 * d, n), dtype=np.int64).view(np.uint64)
        ra[1, 0, :] = np.int64(-(1 << 10)).view(np.uint64)
    else:
        ra, rb = r64(rng, count, 2 * d, n), r64(rng, count, 2 * d, n)
        ra[1, 0, :] = np.uint64(1 << 63)
    ra.setflags(write=False)
    rb.setflags(write=False)
    return ra, rb


def make_key(fhe, torch, cell, ra, rb):
    """the key of a cell, and FIRST the assertion that it is the cell's form"""
    form, packed, log_n, log_b, d, no_f64 = cell
    D = lambda x: torch.from_numpy(np.array(x, dtype=np.uint64).view(np.int64)).cuda()  # noqa: E731  (a copy: the shared inputs are read-only)
    try:
        fhe.set_option("NO_F64_EXACT", int(no_f64))
        key = fhe.TggswKey(fhe.TorusContext(), log_b, d, D(ra), D(rb), 1 << log_n, fft64=form == "fft64")
    finally:
        fhe.set_option("NO_F64_EXACT", 0)
    assert (key.form, key.packs_digits) == (form, packed), "the host's rule moved this cell: %r" % (cell,)
    return key, D


def packed_runs(fhe, key, packed, run):
    """run() as the key is; a packed cell once more with the lab switch NO_PACKED_DIGITS, which the key must report -> the results"""
    outs = [run()]
    if packed:
        try:
            fhe.set_option("NO_PACKED_DIGITS", 1)
            assert key.packs_digits == 0 and key.form == "30"
            outs.append(run())
        finally:
            fhe.set_option("NO_PACKED_DIGITS", 0)
        assert key.packs_digits == 1
    return outs


@gpu
def test_key_form_rejects_null_outputs(fhe, torch_cuda):
    import ctypes as C
    cell = CELLS[0]
    key, _ = make_key(fhe, torch_cuda, cell, *key_rows(cell, 2, 0))
    form, packs = C.c_int(-1), C.c_int(-1)
    lib = fhe.lib()
    assert lib.fhe_tggsw_key_form(key._h, None, C.byref(packs)) == 1 and lib.fhe_tggsw_key_form(key._h, C.byref(form), None) == 1
    assert (form.value, packs.value) == (-1, -1)
    assert lib.fhe_tggsw_key_form(key._h, C.byref(form), C.byref(packs)) == 0 and (form.value, packs.value) == (0, 0)


@gpu
@pytest.mark.parametrize("cell", [c for c in CELLS if not c[1]], ids=[i for c, i in zip(CELLS, CELL_IDS) if not c[1]])
def test_external_product(fhe, cref, torch_cuda, cell):
    """tggsw.rs:100-112 on the four forms that run it (a packed key runs the unpacked product: the `30` cells): a key of three entries read at
    index 1 (a wrong first_index * per stride reads another entry), batch 5 (one-wave teams: a second workgroup with three idle teams), torus
    words 0, -1, -2^63, 2^63 - 1 and a ciphertext of extreme digits"""
    form, packed, log_n, log_b, d, _ = cell
    n, batch, count, index = 1 << log_n, 5, 3, 1
    ra, rb = key_rows(cell, count, 1)
    key, D = make_key(fhe, torch_cuda, cell, ra, rb)
    rng = np.random.Generator(np.random.PCG64([9200, log_n, log_b]))
    ca, cb = r64(rng, batch, n), r64(rng, batch, n)
    ca[0, :5] = [0, (1 << 64) - 1, 1 << 63, (1 << 63) - 1, 1]
    cb[1, :] = extreme_digits(log_b, d)
    a, b = D(ca), D(cb)
    key.external_product_(index, a, b)
    ha, hb = host(a).reshape(batch, n), host(b).reshape(batch, n)
    for i in range(batch):
        ea, eb = cref.tggsw_external_product(log_b, d, ra[index], rb[index], ca[i], cb[i])
        assert np.array_equal(ha[i], ea) and np.array_equal(hb[i], eb), (cell, i)


N_LWE, BATCH = 5, 5


@functools.lru_cache(maxsize=None)
def rotation_inputs(cell):
    """tables [2][n] (the first half of table 0: extreme digits), a_tilde [5][5] with 0 (the CMUX short-circuits), N (pure negation) and
    2N - 1, b_tilde [5] with 0 and 2N - 1; row 3 carries all three special rotations: it is the batch of one"""
    _, _, log_n, log_b, d, _ = cell
    n = 1 << log_n
    rng = np.random.Generator(np.random.PCG64([9300, log_n, log_b, d]))
    tables = r64(rng, 2, n)
    tables[0, : n // 2] = extreme_digits(log_b, d)
    a_t = rng.integers(0, 2 * n, size=(BATCH, N_LWE), dtype=np.uint64)
    b_t = rng.integers(0, 2 * n, size=BATCH, dtype=np.uint64)
    a_t[0, 0], a_t[1, 1], a_t[2, 4] = 0, n, 2 * n - 1
    a_t[3, :3] = [0, n, 2 * n - 1]
    a_t[4, :] = 0                                                # every CMUX of this one short-circuits
    b_t[0], b_t[4] = 0, 2 * n - 1
    for x in (tables, a_t, b_t):
        x.setflags(write=False)
    return tables, a_t, b_t


@functools.lru_cache(maxsize=None)
def rotation_oracle(cell, table):
    """cref.tfhe_blind_rotate of all five ciphertexts through tables[table], once per cell"""
    from oracle import cref
    _, _, _, log_b, d, _ = cell
    ra, rb = key_rows(cell, N_LWE, 2)
    tables, a_t, b_t = rotation_inputs(cell)
    ea, eb = cref.tfhe_blind_rotate(log_b, d, ra, rb, tables[table], a_t, b_t, threads=8)
    ea.setflags(write=False)
    eb.setflags(write=False)
    return ea, eb


@gpu
@cells
def test_blind_rotation(fhe, torch_cuda, cell):
    """bootstrapping.rs:84-96, n_lwe = 5: batch 5 (one-wave teams: two workgroups, three idle teams in the second; else five workgroups) and
    batch 1 (three idle teams beside the working one); packed cells also with NO_PACKED_DIGITS: EVERY run against the oracle"""
    form, packed, log_n, log_b, d, _ = cell
    n = 1 << log_n
    key, D = make_key(fhe, torch_cuda, cell, *key_rows(cell, N_LWE, 2))
    tables, a_t, b_t = rotation_inputs(cell)
    ea, eb = rotation_oracle(cell, 0)
    assert not ea[4].any() and np.array_equal(eb[4], M.rotate(tables[0], -int(b_t[4])))        # (0, v X^-b) untouched
    for rows in (slice(0, BATCH), slice(3, 4)):
        batch = rows.stop - rows.start
        outs = packed_runs(fhe, key, packed, lambda: key.blind_rotate(D(a_t[rows]), D(b_t[rows]), D(tables[0])))
        assert len(outs) == 1 + packed
        for run, (oa, ob) in enumerate(outs):
            ha, hb = host(oa).reshape(batch, n), host(ob).reshape(batch, n)
            for i in range(batch):
                assert np.array_equal(ha[i], ea[rows][i]) and np.array_equal(hb[i], eb[rows][i]), (cell, batch, "unpacked" if run else "as made", i)


@gpu
@cells
def test_blind_rotation_with_a_table_per_ciphertext(fhe, torch_cuda, cell):
    """fhe_tfhe_blind_rotate_tables: two tables, table_of = [1, 0, 1, 1, 0]; each ciphertext against the oracle's rotation of ITS table"""
    form, packed, log_n, log_b, d, _ = cell
    n = 1 << log_n
    key, D = make_key(fhe, torch_cuda, cell, *key_rows(cell, N_LWE, 2))
    tables, a_t, b_t = rotation_inputs(cell)
    table_of = [1, 0, 1, 1, 0]
    idx = torch_cuda.tensor(table_of, dtype=torch_cuda.int32, device="cuda")
    want = [rotation_oracle(cell, 0), rotation_oracle(cell, 1)]
    outs = packed_runs(fhe, key, packed, lambda: key.blind_rotate_tables(D(a_t), D(b_t), D(tables), idx))
    for run, (oa, ob) in enumerate(outs):
        ha, hb = host(oa).reshape(BATCH, n), host(ob).reshape(BATCH, n)
        for i, tb in enumerate(table_of):
            assert np.array_equal(ha[i], want[tb][0][i]) and np.array_equal(hb[i], want[tb][1][i]), (cell, "unpacked" if run else "as made", i, tb)


@gpu
@pytest.mark.parametrize("tree", [True, False], ids=["tree", "no-tree"])
@cells
def test_table_look_up(fhe, cref, torch_cuda, cell, tree):
    """fhe_tfhe_lut_eval, batch 3, first_index = 1 (one unused selector in front).  tree: m = log_n + 1, n_out = 2: one tree level, then a
    ladder of log_n steps from the accumulators (six ladder teams, six level teams), without and with the key switch; no tree: m = 3, n_out =
    1: the ladder starts from the shared polynomials (three teams).  Against tfhe_lut_model.lut_eval_ciphertexts (the walk of
    lut_eval_batch_steps on the oracle's entries; validated in test_tfhe_lut_cpu.py), packed cells also with NO_PACKED_DIGITS"""
    form, packed, log_n, log_b, d, _ = cell
    n, batch, first = 1 << log_n, 3, 1
    m, n_out = (log_n + 1, 2) if tree else (3, 1)
    ra, rb = key_rows(cell, first + batch * m, 3 if tree else 4)
    key, D = make_key(fhe, torch_cuda, cell, ra, rb)
    rng = np.random.Generator(np.random.PCG64([9400, log_n, log_b, d, m]))
    table = r64(rng, n_out, 1 << m)
    table[0, :3] = extreme_digits(log_b, d)
    polys = fhe.tfhe_cbs.lut_pack(table, m, n)
    assert np.array_equal(polys, M.pack(table, m, n))
    ks_log_b, ks_d, width = KS
    ksk_a, ksk_b = r64(rng, n * ks_d, width), r64(rng, n * ks_d)
    ext = M.lut_extractions(cref, polys, log_b, d, ra, rb, first, m, n_out, batch, threads=batch)
    for ks in ((None, (ks_log_b, ks_d, ksk_a, ksk_b, width)) if tree else (None,)):
        want_a, want_b = M.lut_key_switch(cref, ext[0], ext[1], ks) if ks else ext
        dks = (ks[0], ks[1], D(ks[2]), D(ks[3]), ks[4]) if ks else None
        outs = packed_runs(fhe, key, packed, lambda: fhe.tfhe_cbs.lut_eval_batch(D(polys), key, first, m, n_out, batch, dks))
        assert len(outs) == 1 + packed
        for run, (oa, ob) in enumerate(outs):
            assert tuple(oa.shape) == want_a.shape and tuple(ob.shape) == want_b.shape
            ha, hb = host(oa), host(ob)
            for c in range(batch):
                assert np.array_equal(ha[c], want_a[c]) and np.array_equal(hb[c], want_b[c]), (cell, m, ks is not None, "unpacked" if run else "as made", c)
