"""No-GPU checks of the circuit bootstrap: csrc/tfhe_cbs.hpp as a host program (table, row mapping, rejections), its table against the
Python model, the library's exports and host-only entries, and the plain model of the key switch against a direct restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tfhe_cbs_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_SYMBOLS = ("fhe_tlwe_pfksk_gen", "fhe_tlwe_pfks", "fhe_tfhe_cbs_table", "fhe_tfhe_cbs_workspace", "fhe_tfhe_circuit_bootstrap")


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/tfhe_cbs_host_test.cpp: a stand-alone program under AddressSanitizer and UBSan, run as its own process"""
    exe = str(tmp_path_factory.mktemp("cbs") / "tfhe_cbs_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(HERE, "tfhe_cbs_host_test.cpp")])
    return exe


def test_new_symbols_are_exported(fhe):
    lib = fhe.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


def test_host_header_as_a_program(host_exe):
    out = subprocess.run([host_exe], capture_output=True, text=True)
    assert out.returncode == 0 and "tfhe_cbs_host_test ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("cb_d", [1, 2, 3, 4, 16])
def test_table_header_library_and_model_agree(fhe, host_exe, cb_d):
    log_b, n = (4 if cb_d == 16 else 5), 256
    want = M.cbs_table(log_b, cb_d, n)
    out = subprocess.run([host_exe, "table", str(log_b), str(cb_d), str(n)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert np.array_equal(np.array([int(x) for x in out.stdout.split()], dtype=np.uint64), want)
    assert np.array_equal(fhe.tfhe_cbs.cbs_table(log_b, cb_d, n), want)
    # the table is lut_many of f_j(0) = 0, f_j(1) = g_j on raw torus values: slot 1 of p = 2 spans n/4 .. 3n/4
    g, funcs = M.gadget(log_b, cb_d), 1 << M.nu_of(cb_d)
    assert fhe.tfhe_cbs.cbs_nu(cb_d) == M.nu_of(cb_d)
    for c in (0, n // 4 - 1, n // 4, n // 2 + 1, 3 * n // 4 - 1, 3 * n // 4, n - 1):
        j = c % funcs
        assert int(want[c]) == (g[j] if j < cb_d and n // 4 <= c - j < 3 * n // 4 else 0)


def test_library_rejections_need_no_device(fhe):
    lib, buf = fhe.lib(), np.zeros(2048, dtype=np.uint64)
    p = buf.ctypes.data_as(fhe._lib.u64p)
    assert lib.fhe_tfhe_cbs_table(4, 0, 1024, p) == 1 and lib.fhe_tfhe_cbs_table(4, 17, 1024, p) == 1
    assert lib.fhe_tfhe_cbs_table(4, 16, 256, p) == 0 and lib.fhe_tfhe_cbs_table(4, 16, 32, p) == 1 and lib.fhe_tfhe_cbs_table(4, 2, 4096, p) == 6
    v = C.c_void_p(buf.ctypes.data)
    assert lib.fhe_tlwe_pfks(7, 3, v, 5, v, v, 8, 256, 1, v, v, 4, 0, None) == 1           # n_funcs = 5
    assert lib.fhe_tlwe_pfks(7, 3, v, 2, v, v, 8, 256, 3, v, v, 4, 0, None) == 1           # batch no multiple of group
    assert lib.fhe_tlwe_pfks(7, 3, None, 2, v, v, 8, 256, 1, v, v, 4, 0, None) == 1
    w = C.c_void_p(buf.ctypes.data + 8192)
    assert lib.fhe_tlwe_pfks(7, 3, v, 2, v, v, 8, 256, 1, w, w, 4, 0, None) == 1           # out_a == out_b, any memory
    x, y = C.c_void_p(buf.ctypes.data + 64), C.c_void_p(buf.ctypes.data + 128)
    assert lib.fhe_tlwe_pfks(7, 3, v, 2, x, y, 8, 256, 1, x, w, 4, 1, None) == 1           # device memory: out_a is ct_a
    assert lib.fhe_tlwe_pfks(7, 3, v, 2, x, y, 8, 256, 1, w, v, 4, 1, None) == 1           # device memory: out_b is the key
    assert lib.fhe_tlwe_pfks(32, 2, v, 2, v, v, 8, 256, 1, v, v, 4, 0, None) == 6
    assert lib.fhe_tlwe_pfks(7, 3, v, 2, v, v, 8, 256, 1, v, v, 0, 0, None) == 0           # nothing to do
    words = C.c_size_t()
    assert lib.fhe_tfhe_cbs_workspace(1024, 630, 3, 5, C.byref(words)) == 0 and words.value == 2 * 5 * 1024 + 15 * 1024 + 5 * 630 + 5 + 15
    assert lib.fhe_tfhe_cbs_workspace(1000, 630, 3, 5, C.byref(words)) == 1 and lib.fhe_tfhe_cbs_workspace(1024, 0, 3, 5, C.byref(words)) == 1
    assert lib.fhe_tfhe_cbs_workspace(128, 8, 3, 5, C.byref(words)) == 6 and lib.fhe_tfhe_cbs_workspace(1024, 8, 17, 5, C.byref(words)) == 1
    assert lib.fhe_tfhe_circuit_bootstrap(None, None, 4, 2, 7, 3, v, v, v, v, v, 1, 0, None) == 1
    assert lib.fhe_set_option(b"PFKS_CHUNK", 64) == 0 and lib.fhe_set_option(b"PFKS_CHUNK", 0) == 0
    assert lib.fhe_set_option(b"PFKS_SPLIT", 3) == 0 and lib.fhe_set_option(b"PFKS_SPLIT", 0) == 0


def test_model_key_switch_against_a_direct_sum():
    """A check of the MODEL alone (it runs no library code and passes with or without the feature): the GPU tests hold the library
    against this model, so the model is held against the definition here.
    pfks of the model (vectorised) against the definition term by term on Python integers, and the phase of its output under a
    noise-free key: F_u times the input phase up to the rounding bound (n_in + 1) 2^(63 - log_b d) |F_u|_1"""
    rng = np.random.Generator(np.random.PCG64(6000))
    log_b, d, n_in, n, n_funcs, batch = 5, 3, 3, 8, 2, 2
    key = rng.integers(0, 1 << 63, size=(d * (n_in + 1), n_funcs, 2, n), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    ct_a = rng.integers(0, 1 << 63, size=(batch, n_in), dtype=np.uint64) * np.uint64(2)
    ct_b = rng.integers(0, 1 << 63, size=batch, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    oa, ob = M.pfks(log_b, d, key, n_funcs, ct_a, ct_b, n_in, n, group=2)
    for r in range(batch):
        dg = M.digits(log_b, d, list(ct_a[r]) + [ct_b[r]])
        for u in range(n_funcs):
            for half, out in ((0, oa), (1, ob)):
                want = [sum(dg[i][j] * int(key[j * (n_in + 1) + i, u, half, k]) for j in range(d) for i in range(n_in + 1)) % M.M64 for k in range(n)]
                assert [int(x) for x in out[M.out_row(r, u, n_funcs, 2)]] == want
    # plaintext rows as a noise-free key with a = 0: the output's b is the phase
    sk_in = np.array([1, 0, 1], dtype=np.uint64)
    funcs = np.array([[3, 0, M.M64 - 1, 0, 0, 2, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0]], dtype=np.uint64)
    plain = M.pfksk_plain(log_b, d, sk_in, funcs)
    key = np.zeros((d * (n_in + 1), n_funcs, 2, n), dtype=np.uint64)
    key[:, :, 1] = plain
    oa, ob = M.pfks(log_b, d, key, n_funcs, ct_a, ct_b, n_in, n)
    assert not oa.any()
    for r in range(batch):
        phase = (int(ct_b[r]) - sum(int(a) * int(s) for a, s in zip(ct_a[r], sk_in))) % M.M64
        for u in range(n_funcs):
            l1 = sum(abs(M.P.t64_to_i64(int(x))) for x in funcs[u])
            for k in range(n):
                err = M.P.t64_to_i64((int(ob[r * n_funcs + u, k]) - M.P.t64_to_i64(int(funcs[u, k])) * phase) % M.M64)
                assert abs(err) <= (n_in + 1) * (1 << (63 - log_b * d)) * l1


def test_lut_eval_plain(fhe):
    table = list(range(100, 116))
    for x in range(16):
        bits = [(x >> l) & 1 for l in range(4)]
        assert fhe.tfhe_cbs.lut_eval_plain(table, bits) == table[x] == M.lut_eval_plain(table, bits)
