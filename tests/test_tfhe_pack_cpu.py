"""No-GPU checks of the packing key switch: the header's declarations and the library's exports, csrc/tfhe_pack.hpp as a host program
(the exactness bound, the chunk rule, the lab switch's clamp, the argument checks), and the model of tests/tfhe_pack_model.py against
the key switch of tfhe_cbs_model followed by rotations and a sum."""
import os
import re
import subprocess

import numpy as np
import pytest

import tfhe_cbs_model as CM
import tfhe_pack_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENTRIES = ("fhe_tlwe_pack_key_prepare", "fhe_tlwe_pack_key_destroy", "fhe_tlwe_pack")


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/tfhe_pack_host_test.cpp: a stand-alone program under AddressSanitizer and UBSan, run as its own process"""
    exe = str(tmp_path_factory.mktemp("pack") / "tfhe_pack_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(HERE, "tfhe_pack_host_test.cpp")])
    return exe


def test_entries_are_declared_and_exported(fhe):
    with open(os.path.join(ROOT, "include", "fhe_ring.h")) as f:
        header = f.read()
    assert "typedef struct fhe_tlwe_pack_key fhe_tlwe_pack_key;" in header
    lib = fhe.lib()
    for name in ENTRIES:
        assert re.search(r"\b(int|void)\s+%s\(" % name, header), name
        assert hasattr(lib, name), name
    assert lib.fhe_set_option(b"PACK_SPLIT", 3) == 0 and lib.fhe_set_option(b"PACK_SPLIT", 0) == 0
    for name in (b"PACK_ROUTE", b"PACK_SLAB"):
        assert lib.fhe_set_option(name, 2) == 0 and lib.fhe_set_option(name, 0) == 0
    f = fhe.tfhe_pack.pack_funcs(16)
    assert f.shape == (1, 16) and f.dtype == np.uint64 and f[0, 0] == 1 and not f[0, 1:].any()


def test_library_rejections_need_no_device(fhe):
    import ctypes as C
    lib, buf = fhe.lib(), np.zeros(64, dtype=np.uint64)
    v, h = C.c_void_p(buf.ctypes.data), C.c_void_p()
    assert lib.fhe_tlwe_pack_key_prepare(None, 7, 3, v, 8, 256, 0, None, C.byref(h)) == 1 and not h.value
    assert lib.fhe_tlwe_pack(None, None, v, v, 1, 1, 1, v, v, 0, None) == 1
    lib.fhe_tlwe_pack_key_destroy(None)


def test_host_header_as_a_program(host_exe):
    out = subprocess.run([host_exe], capture_output=True, text=True)
    assert out.returncode == 0 and "tfhe_pack_host_test ok" in out.stdout, out.stdout + out.stderr


def rotate(poly, k):
    """poly X^k in Z_{2^64}[X]/(X^n + 1), 0 <= k < n (tglwe.rs:61-66)"""
    n = poly.size
    out = np.empty_like(poly)
    out[k:] = poly[:n - k]
    out[:k] = np.uint64(0) - poly[n - k:]
    return out


@pytest.mark.parametrize("log_b,d", [(4, 2), (9, 3)])
@pytest.mark.parametrize("count,stride", [(1, 1), (1, 3), (5, 1), (5, 3), (16, 1)])  # (16, 3) is not admissible: 45 >= 16
def test_model_against_key_switch_rotation_and_sum(log_b, d, count, stride):
    """A check of the MODEL alone (it runs no library code): n = 16, n_in = 3, two packs"""
    n, n_in, packs = 16, 3, 2
    rng = np.random.Generator(np.random.PCG64(9000 + 100 * log_b + 10 * count + stride))
    key = rng.integers(0, 1 << 63, size=(d * (n_in + 1), 1, 2, n), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    ct_a = rng.integers(0, 1 << 63, size=(packs, count, n_in), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(packs, count, n_in), dtype=np.uint64)
    ct_b = rng.integers(0, 1 << 63, size=(packs, count), dtype=np.uint64) * np.uint64(2)
    ct_a[0, 0, :3] = np.array([0, 1 << 63, (1 << 64) - 1], dtype=np.uint64)
    got_a, got_b = M.pack(log_b, d, key, ct_a, ct_b, n_in, n, count, stride)
    ka, kb = CM.pfks(log_b, d, key, 1, ct_a.reshape(-1, n_in), ct_b.reshape(-1), n_in, n)
    ka, kb = ka.reshape(packs, count, n), kb.reshape(packs, count, n)
    for g in range(packs):
        want_a, want_b = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        for r in range(count):
            want_a += rotate(ka[g, r], r * stride)
            want_b += rotate(kb[g, r], r * stride)
        assert np.array_equal(got_a[g], want_a) and np.array_equal(got_b[g], want_b), g


def test_inadmissible_position_is_refused_by_the_model():
    with pytest.raises(AssertionError):
        M.digit_polys(4, 2, np.zeros((16, 3), dtype=np.uint64), np.zeros(16, dtype=np.uint64), 3, 16, 16, 3)
