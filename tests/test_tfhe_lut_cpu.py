"""No-GPU checks of the vertically packed table look-up: csrc/tfhe_lut.hpp as a host program (shape, packing, extraction indices,
workspace, rejections), the packing of header, library and Python model against each other, the model's ideal tree and rotation against
the table for every address, and the library's exports and host-only entries."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tfhe_lut_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_SYMBOLS = ("fhe_tfhe_lut_shape", "fhe_tfhe_lut_pack", "fhe_tfhe_lut_workspace", "fhe_tfhe_lut_eval")


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/tfhe_lut_host_test.cpp: a stand-alone program under AddressSanitizer and UBSan, run as its own process"""
    exe = str(tmp_path_factory.mktemp("lut") / "tfhe_lut_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(HERE, "tfhe_lut_host_test.cpp")])
    return exe


def demo_table(m, n_out):
    """the table of `tfhe_lut_host_test pack`: T[o][x] = (o << 32) + x + 1"""
    return (np.arange(n_out, dtype=np.uint64)[:, None] << np.uint64(32)) + np.arange(1 << m, dtype=np.uint64)[None, :] + np.uint64(1)


def test_new_symbols_are_exported(fhe):
    lib = fhe.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    for name in ("lut_shape", "lut_pack", "lut_eval_batch", "lut_eval_batch_steps"):
        assert hasattr(fhe, name) and hasattr(fhe.tfhe_cbs, name), name


def test_host_header_as_a_program(host_exe):
    out = subprocess.run([host_exe], capture_output=True, text=True)
    assert out.returncode == 0 and "tfhe_lut_host_test ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("m,n_out,n", [(3, 3, 256), (7, 5, 256), (8, 1, 256), (10, 3, 256), (8, 8, 1024), (12, 2, 1024)])
def test_packing_header_library_and_model_agree(fhe, host_exe, m, n_out, n):
    table = demo_table(m, n_out)
    want = M.pack(table, m, n)
    r, h, per_acc, n_acc, n_polys = M.shape(m, n_out, n)
    assert fhe.lut_shape(m, n_out, n) == (r, per_acc, n_acc, n_polys)
    out = subprocess.run([host_exe, "pack", str(m), str(n_out), str(n)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert np.array_equal(np.array([int(x) for x in out.stdout.split()], dtype=np.uint64), want.ravel())
    got = fhe.lut_pack(table, m, n)
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("m", [3, 8, 10])
def test_model_reads_the_table_at_every_address(m):
    """A check of the MODEL alone (it runs no library code): packed polynomials, ideal tree over the high bits, ideal rotation by the low
    bits, coefficient u 2^m -- for ALL 2^m addresses at n = 256, with n_out chosen so that accumulators are shared (m = 3: 5 of 32
    places), exactly filled (m = 8) and behind a tree of four leaves (m = 10); the last accumulator is partly empty wherever it can be"""
    n, n_out = 256, {3: 5, 8: 2, 10: 2}[m]
    rng = np.random.Generator(np.random.PCG64(7000 + m))
    table = rng.integers(0, 1 << 63, size=(n_out, 1 << m), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    polys = M.pack(table, m, n)
    for address in range(1 << m):
        assert M.lookup(polys, m, n_out, address) == [int(table[o, address]) for o in range(n_out)], address


@pytest.mark.parametrize("m,n_out", [(10, 2), (3, 5)])
def test_ciphertext_model_reads_the_table_under_trivial_selectors(cref, m, n_out):
    """A check of the CIPHERTEXT-level model (tfhe_lut_model.lut_eval_ciphertexts: the walk of lut_eval_batch_steps on the exact oracle's
    external product, rotation, extraction and key switch) against the plain model: selectors that are TRIVIAL TGGSW ciphertexts -- every row
    zero, plus bit x base_j on the gadget diagonal -- under the 64-bit gadget (16, 4), which rounds nothing away, make every CMUX exactly the
    choice its bit encodes; the output phases b - <a, s> (under any key s: a stays 0) are then M.lookup's values.  n = 256; m = 10: a tree of
    four leaves per accumulator, then 8 ladder steps; m = 3: no tree, five outputs share one accumulator; two unused selectors in front"""
    n, log_b, d, first = 256, 16, 4, 2
    rng = np.random.Generator(np.random.PCG64(7050 + m))
    table = rng.integers(0, 1 << 63, size=(n_out, 1 << m), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n_out, 1 << m), dtype=np.uint64)
    polys = M.pack(table, m, n)
    top = (1 << m) - 1
    addresses = [0, top, top // 3, 2 * (top // 3), top - 2]                  # m = 10: leaves 0, 3, 1, 2, 3
    batch = len(addresses)
    bases = [1 << (64 - log_b * d + j * log_b) for j in range(d)]           # decompose.rs:66-81: least significant digit first
    rows_a, rows_b = np.zeros((first + batch * m, 2 * d, n), dtype=np.uint64), np.zeros((first + batch * m, 2 * d, n), dtype=np.uint64)
    bits = [1] * first + [(x >> l) & 1 for x in addresses for l in range(m)]  # noqa: E741
    for i, bit in enumerate(bits):
        for j, base in enumerate(bases):                                    # tggsw.rs:73-88: m g_j on a in rows 0 .. d, on b in rows d .. 2d
            rows_a[i, j, 0] = rows_b[i, d + j, 0] = np.uint64(bit * base)
    oa, ob = M.lut_eval_ciphertexts(cref, polys, log_b, d, rows_a, rows_b, first, m, n_out, batch, threads=4)
    assert oa.shape == (batch, n_out, n) and ob.shape == (batch, n_out)
    s = rng.integers(0, 2, size=n, dtype=np.uint64)
    phases = ob - (oa * s).sum(axis=-1, dtype=np.uint64)
    for c, x in enumerate(addresses):
        want = M.lookup(polys, m, n_out, x)
        assert want == [int(table[o, x]) for o in range(n_out)]
        assert [int(v) for v in phases[c]] == want, hex(x)
    # the key switch of the model is the oracle's, output by output
    ks = (4, 3, rng.integers(0, 1 << 63, size=(n * 3, 6), dtype=np.uint64), rng.integers(0, 1 << 63, size=n * 3, dtype=np.uint64), 6)
    ka, kb = M.lut_eval_ciphertexts(cref, polys, log_b, d, rows_a, rows_b, first, m, n_out, 2, ks=ks)
    assert ka.shape == (2, n_out, 6) and kb.shape == (2, n_out)
    wa, wb = cref.tlwe_key_switch(4, 3, ks[2], ks[3], oa[1, n_out - 1], int(ob[1, n_out - 1]))
    assert np.array_equal(ka[1, n_out - 1], wa) and int(kb[1, n_out - 1]) == wb


def test_model_rotation_is_negacyclic():
    p = np.arange(1, 9, dtype=np.uint64)
    assert list(M.rotate(p, -3)) == [4, 5, 6, 7, 8, M.M64 - 1, M.M64 - 2, M.M64 - 3]     # X^-k: coefficient j + k comes to j unsigned
    assert list(M.rotate(p, 1)) == [M.M64 - 8, 1, 2, 3, 4, 5, 6, 7]
    assert np.array_equal(M.rotate(M.rotate(p, -5), 5), p) and np.array_equal(M.rotate(p, 16), p)


def test_library_rejections_need_no_device(fhe):
    lib, buf = fhe.lib(), np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data_as(fhe._lib.u64p)
    r, a, b, c = C.c_int(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    shape = lambda m, n_out, n: lib.fhe_tfhe_lut_shape(m, n_out, n, C.byref(r), C.byref(a), C.byref(b), C.byref(c))  # noqa: E731
    assert shape(8, 8, 1024) == 0 and (r.value, a.value, b.value, c.value) == (8, 4, 2, 2)
    assert shape(10, 3, 256) == 0 and (r.value, a.value, b.value, c.value) == (8, 1, 3, 12)
    assert lib.fhe_tfhe_lut_shape(10, 3, 256, None, None, None, None) == 0
    assert shape(0, 1, 256) == 1 and shape(3, 0, 256) == 1 and shape(3, 1, 1000) == 1
    assert shape(3, 1, 128) == 6 and shape(3, 1, 4096) == 6 and shape(19, 1, 256) == 6 and shape(18, 65, 256) == 6
    assert lib.fhe_tfhe_lut_pack(None, 3, 1, 256, p) == 1 and lib.fhe_tfhe_lut_pack(p, 3, 1, 256, None) == 1
    assert lib.fhe_tfhe_lut_pack(p, 0, 1, 256, p) == 1 and lib.fhe_tfhe_lut_pack(p, 3, 1, 128, p) == 6
    words = C.c_size_t()
    assert lib.fhe_tfhe_lut_workspace(256, 10, 3, 8, 5, C.byref(words)) == 0 and words.value == 2 * 45 * 256 + 15 * 256 + 45 + 15
    assert fhe.tfhe_cbs.lut_workspace(1024, 8, 8, 0, 3) == 2 * 6 * 1024 + 6
    assert lib.fhe_tfhe_lut_workspace(256, 10, 3, 8, 5, None) == 1 and lib.fhe_tfhe_lut_workspace(1000, 10, 3, 8, 5, C.byref(words)) == 1
    assert lib.fhe_tfhe_lut_workspace(256, 19, 3, 8, 5, C.byref(words)) == 6
    v = C.c_void_p(buf.ctypes.data)
    assert lib.fhe_tfhe_lut_eval(None, None, 0, 8, v, 1, 0, 0, None, None, 0, v, v, 1, 0, None) == 1
