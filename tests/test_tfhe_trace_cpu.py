"""No-GPU checks of the TGLWE automorphism key switch, trace and ring packing: the header's declarations and the library's exports, the
rejections that need no device, csrc/tfhe_trace.hpp as a host program against tables from Python, and the model of
tests/tfhe_trace_model.py against the identities of include/fhe_ring.h and the error bound of DESIGN.md 9.10."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import tfhe_mul_model as MM
import tfhe_trace_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
M64 = 1 << 64
ENTRIES = ("fhe_tglwe_atk_gen", "fhe_tglwe_atk_prepare", "fhe_tglwe_atk_destroy", "fhe_tglwe_automorphism", "fhe_tglwe_trace", "fhe_tlwe_ring_pack")
INVALID, UNSUPPORTED = 1, 6


def test_entries_are_declared_and_exported(fhe, tmp_path):
    with open(os.path.join(ROOT, "include", "fhe_ring.h")) as f:
        header = f.read()
    assert "typedef struct fhe_tglwe_auto_key fhe_tglwe_auto_key;" in header
    lib = fhe.lib()
    for name in ENTRIES:
        assert re.search(r"\b(int|void)\s+%s\(" % name, header), name
        assert hasattr(lib, name), name
    for name in ("atk_gen", "AutoKey", "automorphism", "trace", "ring_pack", "embed", "galois_set", "ring_pack_composed", "trace_composed", "matvec",
                 "matvec_plain"):
        assert hasattr(fhe.tfhe_trace, name), name
    assert fhe.tfhe_trace.galois_set(256) == [3, 5, 9, 17, 33, 65, 129, 257] and fhe.galois_set(16) == [3, 5, 9, 17]
    assert fhe.tfhe_trace.matvec_plain([[1, -2, 3], [0, 1, 1]], [4, 5, -6]) == [-24, -1]
    # the header is still C99, with the new symbols used
    src = tmp_path / "use.c"
    src.write_text('#include "fhe_ring.h"\n'
                   "int use(const fhe_torus_ctx *t, fhe_tglwe_auto_key *k, const uint32_t *gs, uint64_t *p, const fhe_rng *r) {\n"
                   "    int rc = fhe_tglwe_atk_gen(t, 7, 5, p, 256, gs, 1, 0.0, r, 0, p, p, FHE_MEM_HOST, 0);\n"
                   "    rc |= fhe_tglwe_atk_prepare(t, 7, 5, p, p, 256, gs, 1, FHE_MEM_HOST, 0, &k);\n"
                   "    rc |= fhe_tglwe_automorphism(t, k, 3, p, p, p, p, 1, FHE_MEM_HOST, 0);\n"
                   "    rc |= fhe_tglwe_trace(t, k, 0, 8, p, p, p, p, 1, FHE_MEM_HOST, 0);\n"
                   "    rc |= fhe_tlwe_ring_pack(t, k, p, p, 8, 1, p, p, FHE_MEM_HOST, 0);\n"
                   "    fhe_tglwe_atk_destroy(k);\n"
                   "    return rc;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "use.o")])


def test_library_rejections_need_no_device(fhe):
    lib = fhe.lib()
    bufs = [np.full(64, 0x5a5a5a5a5a5a5a5a, dtype=np.uint64) for _ in range(6)]
    v = [C.c_void_p(b.ctypes.data) for b in bufs]
    fake = v[5]  # stands for a context, a generator or a key: no entry may look inside before it has refused
    h = C.c_void_p()
    gs = lambda *g: (C.c_uint32 * len(g))(*g)  # noqa: E731
    # NULL pointers
    assert lib.fhe_tglwe_atk_gen(None, 7, 5, v[0], 256, gs(3), 1, 0.0, fake, 0, v[1], v[2], 0, None) == INVALID
    assert lib.fhe_tglwe_atk_gen(fake, 7, 5, None, 256, gs(3), 1, 0.0, fake, 0, v[1], v[2], 0, None) == INVALID
    assert lib.fhe_tglwe_atk_gen(fake, 7, 5, v[0], 256, None, 1, 0.0, fake, 0, v[1], v[2], 0, None) == INVALID
    assert lib.fhe_tglwe_atk_gen(fake, 7, 5, v[0], 256, gs(3), 1, 0.0, None, 0, v[1], v[2], 0, None) == INVALID
    assert lib.fhe_tglwe_atk_gen(fake, 7, 5, v[0], 256, gs(3), 1, 0.0, fake, 0, v[1], None, 0, None) == INVALID
    assert lib.fhe_tglwe_atk_prepare(None, 7, 5, v[0], v[1], 256, gs(3), 1, 0, None, C.byref(h)) == INVALID and not h.value
    assert lib.fhe_tglwe_atk_prepare(fake, 7, 5, None, v[1], 256, gs(3), 1, 0, None, C.byref(h)) == INVALID and not h.value
    assert lib.fhe_tglwe_atk_prepare(fake, 7, 5, v[0], v[1], 256, None, 1, 0, None, C.byref(h)) == INVALID and not h.value
    assert lib.fhe_tglwe_atk_prepare(fake, 7, 5, v[0], v[1], 256, gs(3), 1, 0, None, None) == INVALID
    assert lib.fhe_tglwe_automorphism(None, fake, 3, v[0], v[1], v[2], v[3], 1, 0, None) == INVALID
    assert lib.fhe_tglwe_automorphism(fake, None, 3, v[0], v[1], v[2], v[3], 1, 0, None) == INVALID
    assert lib.fhe_tglwe_trace(None, fake, 0, 8, v[0], v[1], v[2], v[3], 1, 0, None) == INVALID
    assert lib.fhe_tglwe_trace(fake, None, 0, 8, v[0], v[1], v[2], v[3], 1, 0, None) == INVALID
    assert lib.fhe_tlwe_ring_pack(None, fake, v[0], v[1], 8, 1, v[2], v[3], 0, None) == INVALID
    assert lib.fhe_tlwe_ring_pack(fake, None, v[0], v[1], 8, 1, v[2], v[3], 0, None) == INVALID
    lib.fhe_tglwe_atk_destroy(None)
    # another ring
    for n in (0, 128, 300, 4096):
        assert lib.fhe_tglwe_atk_gen(fake, 7, 5, v[0], n, gs(3), 1, 0.0, fake, 0, v[1], v[2], 0, None) == INVALID, n
        assert lib.fhe_tglwe_atk_prepare(fake, 7, 5, v[0], v[1], n, gs(3), 1, 0, None, C.byref(h)) == INVALID and not h.value, n
    # an even g, g >= 2n, a g twice, an empty set
    for bad, n_g in ((gs(2), 1), (gs(3, 512), 2), (gs(513), 1), (gs(3, 5, 3), 3), (gs(3), 0)):
        assert lib.fhe_tglwe_atk_gen(fake, 7, 5, v[0], 256, bad, n_g, 0.0, fake, 0, v[1], v[2], 0, None) == INVALID
        assert lib.fhe_tglwe_atk_prepare(fake, 7, 5, v[0], v[1], 256, bad, n_g, 0, None, C.byref(h)) == INVALID and not h.value
    # gadgets outside the admission rule
    for log_b, d, n in ((0, 5, 256), (7, 0, 256), (13, 5, 256), (43, 1, 2048), (46, 1, 256), (65, 1, 256)):
        assert lib.fhe_tglwe_atk_gen(fake, log_b, d, v[0], n, gs(3), 1, 0.0, fake, 0, v[1], v[2], 0, None) == UNSUPPORTED, (log_b, d, n)
        assert lib.fhe_tglwe_atk_prepare(fake, log_b, d, v[0], v[1], n, gs(3), 1, 0, None, C.byref(h)) == UNSUPPORTED and not h.value, (log_b, d, n)
    for b in bufs:
        assert (b == np.uint64(0x5a5a5a5a5a5a5a5a)).all(), "a refused call wrote"


# ---- the model -----------------------------------------------------------------------------------------------------------------

LOG_B, D = 8, 8


def make_key(rng, rnd, sk, gs, log_b, d, e_key=0):
    n = len(sk)
    plain = M.atk_plain(log_b, d, sk, gs)
    key = {}
    for q, g in enumerate(gs):
        rows = [MM.encrypt(rng, sk, [int(v) for v in plain[q, j]], [rnd.randrange(-e_key, e_key + 1) for _ in range(n)] if e_key else None)
                for j in range(d)]
        key[g] = (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]))
    return key


def tlwe_encrypt(rng, sk, m, e=0):
    """a TLWE ciphertext under the coefficients of sk: sample_extract(0) of a TGLWE encryption of the constant m + e"""
    n = len(sk)
    return M.sample_extract0(MM.encrypt(rng, sk, [(m + e) % M64] + [0] * (n - 1)))


@pytest.mark.parametrize("n", [16, 32, 64])
def test_model_autks_phase_is_the_permuted_phase(n):
    rng, rnd = np.random.Generator(np.random.PCG64(9700 + n)), random.Random(9700 + n)
    sk = rng.integers(0, 2, size=n, dtype=np.uint64)
    gs = [3, 5, n + 1, 2 * n - 1]
    key = make_key(rng, rnd, sk, gs, LOG_B, D)
    pt = [rnd.randrange(M64) for _ in range(n)]
    ct = MM.encrypt(rng, sk, pt)
    for g in gs:
        oa, ob = M.autks(LOG_B, D, key, g, ct)
        assert MM.phase(oa, ob, sk) == M.sigma(pt, g), g
    assert M.sigma(pt, 2 * n - 1) == [pt[0]] + [(-v) % M64 for v in pt[:0:-1]]  # X -> X^-1


@pytest.mark.parametrize("n", [16, 64])
def test_model_trace_full_and_partial(n):
    rng, rnd = np.random.Generator(np.random.PCG64(9710 + n)), random.Random(9710 + n)
    sk = rng.integers(0, 2, size=n, dtype=np.uint64)
    key = make_key(rng, rnd, sk, M.galois_set(n), LOG_B, D)
    pt = [rnd.randrange(M64) for _ in range(n)]
    ct = MM.encrypt(rng, sk, pt)
    ln = M.log2(n)
    oa, ob = M.trace(LOG_B, D, key, ct, 0, ln)
    assert MM.phase(oa, ob, sk) == [(n * pt[0]) % M64] + [0] * (n - 1)
    for lo in (1, ln - 2, ln - 1):  # keeps the multiples of 2^(hi - lo), times 2^(hi - lo)
        k = 1 << (ln - lo)
        oa, ob = M.trace(LOG_B, D, key, ct, lo, ln)
        assert MM.phase(oa, ob, sk) == [(k * pt[i]) % M64 if i % k == 0 else 0 for i in range(n)], lo


@pytest.mark.parametrize("n", [16, 32])
def test_model_ring_pack_and_embed(n):
    rng, rnd = np.random.Generator(np.random.PCG64(9720 + n)), random.Random(9720 + n)
    sk = rng.integers(0, 2, size=n, dtype=np.uint64)
    key = make_key(rng, rnd, sk, M.galois_set(n), LOG_B, D)
    for count in (1, 2, 4, n):
        ms = [rnd.randrange(M64) for _ in range(count)]
        cts = [tlwe_encrypt(rng, sk, m) for m in ms]
        for ct in cts:
            assert M.sample_extract0(M.embed(*ct)) == ([int(v) for v in ct[0]], int(ct[1]))
        oa, ob = M.ring_pack(LOG_B, D, key, cts)
        want = [0] * n
        for r, m in enumerate(ms):
            want[r * (n // count)] = (n * m) % M64
        assert MM.phase(oa, ob, sk) == want, count


@pytest.mark.parametrize("count", [1, 4, 64])
def test_model_error_bound_with_noise(count):
    """gadget (7, 5), n = 64, key and input noise up to 2^20: every coefficient of the pack's phase is inside trace_error_bound"""
    n, log_b, d, e_max = 64, 7, 5, 1 << 20
    rng, rnd = np.random.Generator(np.random.PCG64(9730 + count)), random.Random(9730 + count)
    sk = rng.integers(0, 2, size=n, dtype=np.uint64)
    key = make_key(rng, rnd, sk, M.galois_set(n), log_b, d, e_key=e_max)
    ms = [rnd.randrange(-8, 8) << 50 for _ in range(count)]
    cts = [tlwe_encrypt(rng, sk, m, rnd.randrange(-e_max, e_max + 1)) for m in ms]
    oa, ob = M.ring_pack(log_b, d, key, cts)
    bound = M.trace_error_bound(n, log_b, d, M.log2(n), e_max, e_max)
    assert bound < 1 << 49, "the bound itself must leave the message readable"
    ph = MM.phase(oa, ob, sk)
    want = [0] * n
    for r, m in enumerate(ms):
        want[r * (n // count)] = n * m
    assert max(abs(MM.centred((ph[i] - want[i]) % M64)) for i in range(n)) <= bound


def test_index_table_is_a_signed_permutation():
    for n in (16, 256):
        for g in M.galois_set(n) + [2 * n - 1]:
            tab = M.index_table(n, g)
            assert sorted(t for t, _ in tab) == list(range(n)), (n, g)
    assert M.index_table(8, 3) == [(0, False), (3, False), (6, False), (1, True), (4, True), (7, True), (2, False), (5, False)]


def test_no_new_kernel_spills():
    """profiles/kernel_inventory.txt (the compiler's resource report, gfx950): the trace and merge kernels at the four rings, scratch 0"""
    with open(os.path.join(ROOT, "profiles", "kernel_inventory.txt")) as f:
        rows = [l.split() for l in f if l.startswith("tfhe_trace_api ")]
    team = [r for r in rows if "tglwe_trace_kernel" in r[1] or "tglwe_merge_kernel" in r[1]]
    assert len(team) == 8 and any("atk_plain_kernel" in r[1] for r in rows)
    for r in rows:  # unit name vgpr sgpr scratch_bytes static_lds_bytes vgpr_spill sgpr_spill
        assert (r[4], r[6], r[7]) == ("0", "0", "0"), r


def host_vectors(path):
    lines = []
    for n in (256, 512, 1024, 2048):
        for g in M.galois_set(n) + [2 * n - 1]:
            tab = M.index_table(n, g)
            lines.append("auto %d %d %s" % (n, g, " ".join("%d" % (t * 2 + int(s)) for t, s in tab)))
        for c in range(M.log2(n) + 1):
            for v in range(1, c + 1):
                lv = 1 << v
                lines.append("level %d %d %d %d %d %d" % (n, c, v, lv + 1, n // lv, (1 << c) // lv))
            lines.append("plan %d %d %d %d" % (n, c, ((1 << c) // 2 + ((1 << c) // 4 if c > 2 else 0)) * 2 * n if c > 1 else 0, M.log2(n) - c))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_host_header_as_a_program(tmp_path):
    """tests/tfhe_trace_host_test.cpp: a stand-alone program under AddressSanitizer and UBSan, run as its own process"""
    exe, vec = str(tmp_path / "tfhe_trace_host_test"), str(tmp_path / "vectors.txt")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(HERE, "tfhe_trace_host_test.cpp")])
    host_vectors(vec)
    out = subprocess.run([exe, vec], capture_output=True, text=True)
    assert out.returncode == 0 and "tfhe_trace_host_test ok" in out.stdout, out.stdout + out.stderr
