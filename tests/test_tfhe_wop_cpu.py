"""No-GPU checks of the look-up without a padding bit: csrc/tfhe_wop.hpp as a host program (nu, tables, row order, workspace, rejections),
its tables against the library and the Python model, the library's exports and harness names, the step chain on plaintext phases, and the
first round of the decode-level test through the CPU model."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import tfhe_lut_model as LM
import tfhe_wop_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_SYMBOLS = ("fhe_tggsw_key_reserve", "fhe_tggsw_key_fill", "fhe_tfhe_wop_table", "fhe_tfhe_wop_workspace", "fhe_tfhe_wop_selectors",
               "fhe_tfhe_wop_pbs")

WOP, BYTES = M.WOP, M.BYTES


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/tfhe_wop_host_test.cpp: a stand-alone program under AddressSanitizer and UBSan, run as its own process"""
    exe = str(tmp_path_factory.mktemp("wop") / "tfhe_wop_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(HERE, "tfhe_wop_host_test.cpp")])
    return exe


def test_new_symbols_and_harness_names(fhe):
    lib = fhe.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    for name in ("wop_table", "wop_selectors", "wop_pbs", "encode", "plain_steps", "wop_selectors_steps", "wop_pbs_steps", "wop_workspace"):
        assert hasattr(fhe.tfhe_wop, name), name
    assert hasattr(fhe.TggswKey, "reserve") and hasattr(fhe.TggswKey, "fill")
    assert fhe.tfhe_wop.encode(0xA5, 8) == 0xA5 << 56 and fhe.tfhe_wop.encode(1, 1) == 1 << 63 and fhe.tfhe_wop.encode(0xFFFF, 16) == 0xFFFF << 48


def test_host_header_as_a_program(host_exe):
    out = subprocess.run([host_exe], capture_output=True, text=True)
    assert out.returncode == 0 and "tfhe_wop_host_test ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("cb_d", [1, 2, 3, 4, 7, 8, 16])
@pytest.mark.parametrize("log_delta", [56, 63, -1])
def test_table_header_library_and_model_agree(fhe, host_exe, cb_d, log_delta):
    log_b, n = (3 if cb_d == 16 else 7), 256
    want = M.wop_table(log_b, cb_d, n, log_delta)
    out = subprocess.run([host_exe, "table", str(log_b), str(cb_d), str(n), str(log_delta)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert np.array_equal(np.array([int(x) for x in out.stdout.split()], dtype=np.uint64), want)
    assert np.array_equal(fhe.tfhe_wop.wop_table(log_b, cb_d, n, log_delta), want)
    assert fhe.tfhe_wop.wop_nu(cb_d) == M.nu_of(cb_d)
    g = M.CM.gadget(log_b, cb_d)
    for c in range(2 << M.nu_of(cb_d)):
        j = c % (1 << M.nu_of(cb_d))
        h = g[j] // 2 if j < cb_d else ((1 << (log_delta - 1)) if j == cb_d and log_delta > 0 else 0)
        assert int(want[c]) == (-h) % M.M64


def test_library_rejections_need_no_device(fhe):
    lib, buf = fhe.lib(), np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data_as(fhe._lib.u64p)
    table = lambda log_b, d, n, ld: lib.fhe_tfhe_wop_table(log_b, d, n, ld, p)  # noqa: E731
    assert table(4, 3, 256, 56) == 0 and table(3, 16, 2048, -1) == 0 and table(9, 7, 256, 1) == 0
    assert table(4, 0, 256, 56) == 1 and table(3, 17, 256, 56) == 1 and table(8, 8, 256, 56) == 1 and table(4, 3, 1000, 56) == 1
    assert table(4, 3, 256, 0) == 1 and table(4, 3, 256, 64) == 1 and lib.fhe_tfhe_wop_table(4, 3, 256, 56, None) == 1
    assert table(3, 16, 64, 56) == 1 and table(4, 3, 128, 56) == 6 and table(4, 3, 4096, 56) == 6
    words = C.c_size_t()
    ws = lambda n, n_lwe, m, d, batch: lib.fhe_tfhe_wop_workspace(n, n_lwe, m, d, batch, C.byref(words))  # noqa: E731
    base = 2 * 3 * 256 + 27 * 256 + 3 * 5 + 3 + 27
    assert ws(256, 5, 3, 3, 3) == 0 and words.value == base + base % 2 + 3 * 256 + 3 * 256 + 2 * 3 * 5 + 3 * 3
    assert fhe.tfhe_wop.wop_workspace(256, 5, 3, 3, 3) == words.value
    assert ws(256, 5, 0, 3, 3) == 1 and ws(256, 0, 3, 3, 3) == 1 and ws(256, 5, 3, 17, 3) == 1 and ws(1000, 5, 3, 3, 3) == 1
    assert lib.fhe_tfhe_wop_workspace(256, 5, 3, 3, 3, None) == 1
    assert ws(256, 5, 17, 3, 3) == 6 and ws(128, 5, 3, 3, 3) == 6 and ws(256, 5, 16, 16, 1 << 23) == 6
    v = C.c_void_p(buf.ctypes.data)
    assert lib.fhe_tfhe_wop_selectors(None, None, 4, 8, v, v, 4, 3, 7, 3, v, 8, v, v, v, v, None, None, 1, 0, None) == 1
    assert lib.fhe_tfhe_wop_pbs(None, None, 4, 8, v, v, 4, 3, 7, 3, v, 8, v, v, None, 0, v, 1, 0, 0, None, None, 0, v, v, 1, 0, None) == 1
    h = C.c_void_p()
    assert lib.fhe_tggsw_key_reserve(None, 7, 3, 256, 4, 0, C.byref(h)) == 1 and not h.value
    assert lib.fhe_tggsw_key_reserve(None, 7, 3, 256, 4, 0, None) == 1
    assert lib.fhe_tggsw_key_fill(None, 0, v, v, 1, 0, None) == 1
    form, packs = C.c_int(-1), C.c_int(-1)
    assert lib.fhe_tggsw_key_form(None, C.byref(form), C.byref(packs)) == 1 and (form.value, packs.value) == (-1, -1)
    assert lib.fhe_tggsw_key_form(None, None, None) == 1
    # (a key needs a device: NULL outputs beside a live key are rejected in tests/test_tfhe_forms_gpu.py)
    assert hasattr(fhe.TggswKey, "form") and hasattr(fhe.TggswKey, "packs_digits")


@pytest.mark.parametrize("m", [1, 2, 8, 16])
def test_step_chain_on_plaintext_phases(fhe, m):
    """A check of the definition on plain phases (ideal blind rotation): every level row is bit g_j, every correction bit 2^delta_l, the
    remainder of step l is the message without its bits below l, for messages 0, 2^m - 1, alternating patterns and a random one, with noise
    of both signs just inside what the caller's condition allows: |e| 2^(m-1) + drift < quarter ring"""
    n, cb_log_b, cb_d = 256, 4, 3
    g = M.CM.gadget(cb_log_b, cb_d)
    top = (1 << m) - 1
    rng = np.random.Generator(np.random.PCG64(7500 + m))
    room = (1 << (62 - (m - 1))) - (1 << (64 - m - 4))              # a quarter of the ring before the shift, less a sixteenth of a slot
    for x in {0, top, 0xAAAA & top, 0x5555 & top, int(rng.integers(0, top + 1))}:
        for e in (0, room, -room, 12345, -1):
            phase = ((x << (64 - m)) + e) % M.M64
            steps = M.plain_steps(phase, m, n, cb_log_b, cb_d)
            assert [s[0] for s in steps] == [(x >> l) & 1 for l in range(m)], (hex(x), e)
            for l, (bit, rows, corr, rem) in enumerate(steps):      # noqa: E741
                assert rows == [bit * g[j] for j in range(cb_d)]
                assert corr == (bit << (64 - m + l) if l < m - 1 else None)
                assert rem == (((x >> l) << (64 - m + l)) + e) % M.M64
            bits, rems = fhe.tfhe_wop.plain_steps(phase, m, n, cb_d)     # the harness's own plain model
            assert bits == [s[0] for s in steps] and rems == [s[3] for s in steps]


def test_model_front_against_its_parts():
    """A check of the MODEL alone: the fused front equals subtraction, shift + 2^62 and oracle.pyref's mod switch done one after another,
    at the words where the mod switch rounds up across 2^64"""
    n, nu, shift = 256, 2, 3
    src = np.array([[0, M.M64 - 1, (1 << 61) - 1, 1 << 60, (M.M64 >> shift) - 1]], dtype=np.uint64)
    cor = np.array([[0, 0, 5, M.M64 - 7, 0]], dtype=np.uint64)
    rem_a, rem_b, at, bt = M.front(src, np.array([M.M64 - 1], dtype=np.uint64), cor, np.array([1], dtype=np.uint64), shift, n, nu)
    sh = 64 - 9 + nu
    for i in range(5):
        r = (int(src[0, i]) - int(cor[0, i])) % M.M64
        s = (r << shift) % M.M64
        assert int(rem_a[0, i]) == r and int(at[0, i]) == ((((s + (1 << (sh - 1))) % M.M64) >> sh) << nu)
    assert int(at[0, 4]) == 0                                       # (2^64 - 8) + half wraps: position 2n = 0
    r = M.M64 - 2
    s = ((r << shift) + (1 << 62)) % M.M64
    assert int(rem_b[0]) == r and int(bt[0]) == ((((s + (1 << (sh - 1))) % M.M64) >> sh) << nu)


def test_first_round_decodes_in_the_cpu_model():
    """The decode-level test's first round on the CPU: keys and noise drawn on the host, the five bytes at x << 56 with no padding bit, the
    selectors by the model of fhe_tfhe_wop_selectors (blind rotations and key switches by oracle.cref), the table T[x] << 56 of a fixed
    pseudo-random permutation read through eight CMUXes, the output switched to the small key.  Every byte decodes to T[x]; the worst phase
    error stays below a quarter of the half-slot (2^53)"""
    p, m = WOP, WOP["m"]
    n, n_lwe = p["n"], p["n_lwe"]
    rng = np.random.Generator(np.random.PCG64(7600))
    K = M.keys(rng, n, n_lwe, p["log_b"], p["d"], p["ks_log_b"], p["ks_d"], p["pf_log_b"], p["pf_d"], p["sd_lwe"], p["sd_glwe"])
    table = np.random.Generator(np.random.PCG64(7403)).permutation(256)
    polys = LM.pack(np.array([int(v) << 56 for v in table], dtype=np.uint64).reshape(1, 256), m, n)
    la, lb = M.tlwe_encrypt(rng, K["z"], [x << 56 for x in BYTES], p["sd_lwe"])
    ra, rb, rem_a, rem_b, _, _, _ = M.selectors(K, p["log_b"], p["d"], p["ks_log_b"], p["ks_d"], p["cb_log_b"], p["cb_d"], p["pf_log_b"], p["pf_d"],
                                                m, la, lb)
    from oracle import cref
    worst = 0
    for c, x in enumerate(BYTES):
        top = M.centered(int(M.tlwe_phases(K["z"], rem_a[c], rem_b[c])) - ((x >> 7) << 63))
        assert abs(top) < 1 << 55, hex(x)                            # the remainder holds the top bit alone
        xa, xb = M.lookup(p["cb_log_b"], p["cb_d"], ra[c], rb[c], polys, m, n)
        oa, ob = cref.tlwe_key_switch(p["ks_log_b"], p["ks_d"], K["ksk_a"], K["ksk_b"], xa, xb)
        phase = int(M.tlwe_phases(K["z"], oa, np.uint64(ob)))
        want = int(table[x])
        err = M.centered(phase - (want << 56))
        print("byte %#04x: phase error 2^%.1f" % (x, math.log2(max(abs(err), 1))))
        worst = max(worst, abs(err))
        assert ((phase + (1 << 55)) % M.M64) >> 56 == want, hex(x)
    print("worst phase error 2^%.1f of half-slot 2^55" % math.log2(max(worst, 1)))
    assert worst < 1 << 53
