"""No-GPU checks of the hoisted CKKS rotations and the double-hoisted diagonal-matrix product: the header's declarations and the
library's exports, the rejections that need no device, csrc/ckks_hoist.hpp as a host program against tables from Python, and the
model of tests/ckks_hoist_model.py in Python integers: against the reference's `rotate` on the inputs the GPU test compares the
device with fhe_ckks_rotate on, and at the level of decrypted plaintexts."""
import ctypes as C
import math
import os
import random
import re
import subprocess

import numpy as np

import ckks_hoist_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENTRIES = ("fhe_rns_automorphism_eval", "fhe_ckks_rotate_many", "fhe_ckks_diag_matrix_prepare_hoisted", "fhe_ckks_diag_matrix_hoisted_destroy",
           "fhe_ckks_mul_mat_hoisted")
INVALID, UNSUPPORTED, NO_DEVICE = 1, 6, 7


def test_entries_are_declared_and_exported(fhe, tmp_path):
    with open(os.path.join(ROOT, "include", "fhe_ring.h")) as f:
        header = f.read()
    assert "typedef struct fhe_ckks_diag_matrix_hoisted fhe_ckks_diag_matrix_hoisted;" in header
    lib = fhe.lib()
    for name in ENTRIES:
        assert re.search(r"\b(int|void)\s+%s\(" % name, header), name
        assert hasattr(lib, name), name
    for name in ("extend_plain", "rotate_many_composed", "mul_mat_hoisted_composed"):
        assert hasattr(fhe.ckks_hoist, name), name
    assert hasattr(fhe.RnsContext, "automorphism_eval") and hasattr(fhe.CkksKey, "rotate_many") and hasattr(fhe, "CkksDiagMatrixHoisted")
    # the header states that these are not the reference's bits, and the property that holds instead
    assert "NOT the bits of fhe_ckks_rotate" in header and "b + rescale_k(x) exactly" in header
    # the header is still C99, with the new symbols used
    src = tmp_path / "use.c"
    src.write_text('#include "fhe_ring.h"\n'
                   "int use(const fhe_rns_ctx *r, const fhe_ckks_key *const *keys, const uint32_t *idx, const uint8_t *present, uint64_t *p,\n"
                   "        uint64_t *const *outs) {\n"
                   "    fhe_ckks_diag_matrix_hoisted *m = 0;\n"
                   "    int rc = fhe_rns_automorphism_eval(r, 1, 5, p, p + 64, 16, 1, FHE_MEM_HOST, 0);\n"
                   "    rc |= fhe_ckks_rotate_many(r, 16, idx, keys, 2, p, p, outs, outs, 1, FHE_MEM_HOST, 0);\n"
                   "    rc |= fhe_ckks_diag_matrix_prepare_hoisted(r, r, 16, idx, 1, idx, 2, present, p, keys, keys, FHE_MEM_HOST, &m);\n"
                   "    rc |= fhe_ckks_mul_mat_hoisted(m, p, p, p, p, 1, FHE_MEM_HOST, 0);\n"
                   "    fhe_ckks_diag_matrix_hoisted_destroy(m);\n"
                   "    return rc;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "use.o")])


def test_library_rejections_need_no_device(fhe, cref):
    lib = fhe.lib()
    sentinel = 0x5a5a5a5a5a5a5a5a
    bufs = [np.full(256, sentinel, dtype=np.uint64) for _ in range(5)]
    v = [C.c_void_p(b.ctypes.data) for b in bufs]
    h = C.c_void_p()
    one, two = (C.c_uint32 * 1)(0), (C.c_uint32 * 2)(0, 1)
    nokey = (C.c_void_p * 2)(None, None)
    outs = (C.c_void_p * 2)(v[2], v[3])
    primes = cref.two_adic_primes(50, 5, 5)
    host = fhe.RnsContext(primes[:3], primes[3:], device=-1)  # a host-only context: every compute entry refuses it
    r = host.handle
    # NULL pointers
    assert lib.fhe_rns_automorphism_eval(None, 0, 5, v[0], v[1], 16, 1, 0, None) == INVALID
    assert lib.fhe_rns_automorphism_eval(r, 0, 5, None, v[1], 16, 1, 0, None) == INVALID
    assert lib.fhe_rns_automorphism_eval(r, 0, 5, v[0], None, 16, 1, 0, None) == INVALID
    assert lib.fhe_rns_automorphism_eval(r, 0, 5, v[0], v[0], 16, 1, 0, None) == INVALID   # in == out
    assert lib.fhe_rns_automorphism_eval(r, 0, 5, v[0], v[1], 12, 1, 0, None) == INVALID   # n not a power of two
    assert lib.fhe_rns_automorphism_eval(r, 0, 5, v[0], v[1], 16, 1, 0, None) == NO_DEVICE
    assert lib.fhe_ckks_rotate_many(None, 16, two, nokey, 2, v[0], v[1], outs, outs, 1, 0, None) == INVALID
    assert lib.fhe_ckks_rotate_many(r, 16, None, nokey, 2, v[0], v[1], outs, outs, 1, 0, None) == INVALID
    assert lib.fhe_ckks_rotate_many(r, 16, two, None, 2, v[0], v[1], outs, outs, 1, 0, None) == INVALID
    assert lib.fhe_ckks_rotate_many(r, 16, two, nokey, 2, v[0], v[1], None, outs, 1, 0, None) == INVALID
    assert lib.fhe_ckks_rotate_many(r, 16, two, nokey, -1, v[0], v[1], outs, outs, 1, 0, None) == INVALID
    assert lib.fhe_ckks_rotate_many(r, 12, two, nokey, 2, v[0], v[1], outs, outs, 1, 0, None) == INVALID
    assert lib.fhe_ckks_rotate_many(r, 16, two, nokey, 2, v[0], v[1], outs, outs, 1, 0, None) == NO_DEVICE
    assert lib.fhe_ckks_diag_matrix_prepare_hoisted(None, r, 16, one, 1, one, 1, bytes([1]), v[0], nokey, nokey, 0, C.byref(h)) == INVALID and not h.value
    assert lib.fhe_ckks_diag_matrix_prepare_hoisted(r, None, 16, one, 1, one, 1, bytes([1]), v[0], nokey, nokey, 0, C.byref(h)) == INVALID and not h.value
    assert lib.fhe_ckks_diag_matrix_prepare_hoisted(r, r, 16, one, 1, one, 1, bytes([1]), v[0], nokey, nokey, 0, None) == INVALID
    assert lib.fhe_ckks_diag_matrix_prepare_hoisted(r, r, 12, one, 1, one, 1, bytes([1]), v[0], nokey, nokey, 0, C.byref(h)) == INVALID and not h.value
    assert lib.fhe_ckks_diag_matrix_prepare_hoisted(r, r, 16, one, 1, one, 1, bytes([1]), v[0], nokey, nokey, 0, C.byref(h)) == NO_DEVICE and not h.value
    assert lib.fhe_ckks_mul_mat_hoisted(None, v[0], v[1], v[2], v[3], 1, 0, None) == INVALID
    lib.fhe_ckks_diag_matrix_hoisted_destroy(None)
    assert all(int(b[0]) == sentinel and int(b[-1]) == sentinel and (b == b[0]).all() for b in bufs)  # nothing was written


def host_vectors(path):
    lines = []
    for log_n in (0, 1, 2, 4, 7, 9):
        n = 1 << log_n
        for t in sorted({5 % (2 * n), 25 % (2 * n), 2 * n - 1, pow(5, 3, 2 * n)}):
            if t & 1:
                lines.append("pi %d %d %s" % (log_n, t, " ".join(map(str, M.pi_table(log_n, t)))))
    for bits, f in ((50, 1 << 20), (54, 1 << 20), (55, 1 << 18), (60, 256), (61, 64), (62, 16)):
        lines.append("fold %d %d" % (bits, f))
    for n, big_l, k, batch in ((16, 3, 2, 2), (1 << 15, 8, 8, 8), (16, 0, 2, 1), (16, 3, 2, 0), (1 << 30, 3, 2, 1), (16, 3, 2, 1 << 28)):
        lk, ok = big_l + k, int(bool(n) and big_l > 0 and batch > 0 and n < (1 << 30) and batch < (1 << 30) // max(2 * (big_l + k), 1))
        e, b = 0, batch * lk * n
        p = b + batch * big_l * n
        lines.append("rot %d %d %d %d %d %d %d %d %d" % (n, big_l, k, batch, ok, e, b, p, p + 2 * batch * lk * n))
    for n, big_l, k, batch, ng in ((16, 3, 2, 2, 2), (1 << 15, 8, 8, 8, 4), (16, 1, 2, 1, 1), (16, 3, 2, 1, 0), (16, 3, 2, 1 << 26, 4), (128, 3, 2, 2, 2)):
        lk = big_l + k
        ok = int(big_l >= 2 and batch > 0 and ng > 0 and ng < (1 << 30) // (2 * lk) and batch < (1 << 30) // (2 * lk * max(ng, 1)))
        b = batch * lk * n
        w = b + batch * big_l * n
        x = w + ng * 2 * batch * lk * n
        tmp = x + ng * 2 * batch * big_l * n
        lines.append("mat %d %d %d %d %d %d 0 %d %d %d %d %d" % (n, big_l, k, batch, ng, ok, b, w, x, tmp, tmp + 2 * batch * (big_l - 1) * n))
    for ng, nb, present in ((2, 3, "111111"), (2, 2, "0111"), (1, 4, "0000"), (3, 2, "100001")):
        rows = [[j for j in range(nb) if present[i * nb + j] == "1"] for i in range(ng)]
        start = [sum(len(r) for r in rows[:i]) for i in range(ng + 1)]
        flat = [j for r in rows for j in r]
        lines.append("terms %d %d %s %d %d %s" % (ng, nb, present, len(flat), max(len(r) for r in rows), " ".join(map(str, start + flat))))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_host_header_as_a_program(tmp_path):
    """tests/ckks_hoist_host_test.cpp: a stand-alone program under AddressSanitizer and UBSan, run as its own process"""
    exe, vec = str(tmp_path / "ckks_hoist_host_test"), str(tmp_path / "vectors.txt")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(HERE, "ckks_hoist_host_test.cpp")])
    host_vectors(vec)
    out = subprocess.run([exe, vec], capture_output=True, text=True)
    assert out.returncode == 0 and "ckks_hoist_host_test ok" in out.stdout, out.stdout + out.stderr


def test_pi_table_is_the_transform_of_the_automorphism():
    """the order the tables above assume, from the reference's transform itself: ntt(sigma_t x)[k] == ntt(x)[pi_t(k)]"""
    from oracle import pyref as P
    log_n = 4
    n = 1 << log_n
    q = next(P.two_adic_primes(50, log_n + 1))
    rnd = random.Random(5)
    x = [rnd.randrange(q) for _ in range(n)]
    fx = P.nega_cyclic_ntt(q, x)
    for t in (5, 25, 2 * n - 1):
        pi = M.pi_table(log_n, t)
        assert P.nega_cyclic_ntt(q, P.automorphism(q, x, t)) == [fx[pi[k]] for k in range(n)], t


def test_no_new_kernel_spills():
    """profiles/kernel_inventory.txt (the compiler's resource report, gfx950): the new kernels, scratch 0, no LDS"""
    with open(os.path.join(ROOT, "profiles", "kernel_inventory.txt")) as f:
        rows = [l.split() for l in f if l.startswith("ckks_hoist_api ")]
    for name in ("ckks_hoist_mac_kernelILb0", "ckks_hoist_mac_kernelILb1", "ckks_hoist_rot_kernel", "ckks_hoist_scale_kernel", "rns_automorphism_eval_kernel"):
        assert any(name in r[1] for r in rows), name
    for r in rows:  # unit name vgpr sgpr scratch_bytes static_lds_bytes vgpr_spill sgpr_spill
        assert (r[4], r[6]) == ("0", "0"), r  # no scratch, no vector register spilled
        if "ckks_hoist" in r[1] or "automorphism_eval" in r[1]:
            assert r[5] == "0", r
        # (scalar registers: the counting instantiation of the accumulation keeps four in lanes of a vector register)
        assert int(r[7]) <= (4 if "ckks_hoist_mac_kernelILb1" in r[1] else 0), r


def to_ints(a):
    return [[int(v) for v in row] for row in a]


def test_model_rotate_many_equals_the_reference_rotate_on_the_seeded_inputs():
    """Python integers, reference functions only: on the inputs of ckks_hoist_model.cleared_inputs no coefficient of `a` sits on a
    rounding tie of the base conversion, so extending before sigma gives the bits of the reference's `rotate`.  The GPU test's
    device == fhe_ckks_rotate check runs on exactly these inputs."""
    from oracle import pyref as P
    c = M.CLEARED
    gen = P.two_adic_primes(c["bits"], c["log_n"] + 1)
    qs, ps, keys, cb, ca = M.cleared_inputs([next(gen) for _ in range(c["L"] + c["K"])])
    n, O = 1 << c["log_n"], M.Ops(P)
    for i in range(c["batch"]):
        b, a = to_ints(cb[i]), to_ints(ca[i])
        raw = [(to_ints(keys[j][0]), to_ints(keys[j][1])) for j in c["amounts"]]
        got = M.rotate_many(O, qs, ps, [0] + c["amounts"], [None] + raw, b, a)
        assert (got[0][0], got[0][1]) == (b, a)  # amount 0 is a copy
        for (gb, ga), j, key in zip(got[1:], c["amounts"], raw):
            wb, wa = P.ckks_rotate(qs, ps, key[0], key[1], pow(5, j, 2 * n), b, a)
            assert gb == [list(r) for r in wb] and ga == [list(r) for r in wa], (i, j)


def test_model_hoisted_product_decrypts_to_the_matrix_product(fhe):
    """Decrypt level, Python integers, n = 16, L = 3, K = 2, 50-bit primes: a three-diagonal matrix, diagonals from extend_plain.
    Secret zo(0.5); the ciphertext carries noise in [-6, 6].  The keys carry none: with K < L the key switch multiplies key noise by
    about Q / P = 2^50, the scale itself, so this base only works with exact keys (the GPU decode test has P > Q and noisy keys).
    Scale 2^50 and f64 encoding leave about 2^-40 per slot; the bound is 2^-30, the reference's for this operation."""
    from oracle import pyref as P
    log_n, bits, big_l, big_k = 4, 50, 3, 2
    n, slots = 1 << log_n, 1 << (log_n - 1)
    gen = P.two_adic_primes(bits, log_n + 1)
    primes = [next(gen) for _ in range(big_l + big_k)]
    qs, ps = primes[:big_l], primes[big_l:]
    ql, qps, big_p, scale = qs[:-1], qs + ps, math.prod(ps), qs[-1]
    rnd = random.Random(99)
    nrng = np.random.Generator(np.random.PCG64(3))
    w = np.exp(2j * np.pi * np.array([pow(5, k, 2 * n) for k in range(slots)]) / (2 * n))
    V = w[:, None] ** np.arange(slots)[None, :]

    def encode(m):
        z = V.conj().T @ m / slots
        return [int(round(float(x) * scale)) for x in list(z.real) + list(z.imag)]

    def decode(coeffs, sc):
        return V @ np.array([coeffs[c] / sc + 1j * (coeffs[slots + c] / sc) for c in range(slots)])

    lift = lambda mods, v: [[x % q for x in v] for q in mods]  # noqa: E731
    sk = [rnd.choice([-1, 0, 0, 1]) for _ in range(n)]

    def encrypt(mods, pt_big, noise):
        a = [[rnd.randrange(q) for _ in range(n)] for q in mods]
        e = [rnd.randint(-noise, noise) for _ in range(n)]
        a_s = P.rns_mul(mods, a, lift(mods, sk))
        return [[(-x + ee + p) % q for x, ee, p in zip(row, e, pt_big)] for q, row in zip(mods, a_s)], a

    def decrypt(mods, b, a):
        a_s = P.rns_mul(mods, a, lift(mods, sk))
        big_q = math.prod(mods)
        out = []
        for c in range(n):
            v = sum(((rb[c] + ra[c]) % q) * (big_q // q) * pow(big_q // q, -1, q) for q, rb, ra in zip(mods, b, a_s)) % big_q
            out.append(v - big_q if v > big_q // 2 else v)
        return out

    rot_key = lambda mods_q, idx: encrypt(mods_q + ps, [x * big_p for x in P.sk_automorphism(sk, pow(5, idx, 2 * n))], 0)  # noqa: E731
    diag = {d: nrng.uniform(0, 1, slots) * np.exp(2j * np.pi * nrng.uniform(0, 1, slots)) for d in (0, 1, 2, slots - 2)}
    msg = nrng.uniform(0, 1, slots) + 1j * nrng.uniform(0, 1, slots)
    want = sum(diag[d] * np.roll(msg, -d) for d in diag)
    split = {0: [0, 1], 2: [0], 6: [0]}  # 0, 1 | 2 | 6 = slots - 2: a baby step with a key, two giant steps with keys
    assert sorted(i + j for i, js in split.items() for j in js) == sorted(diag)
    terms = [(i, j) for i in sorted(split) for j in sorted(split[i])]
    pts = np.array([lift(qs, encode(np.roll(diag[i + j], i))) for i, j in terms], dtype=np.uint64)
    diags = to_ints3(fhe.ckks_hoist.extend_plain(qs, ps, pts))
    # extend_plain: the same centred integers modulo every prime
    for t, (i, j) in enumerate(terms):
        big = encode(np.roll(diag[i + j], i))
        assert diags[t] == lift(qps, big)
    ctb, cta = encrypt(qs, encode(msg), 6)
    raw_baby = {j: rot_key(qs, j) for j in {j for js in split.values() for j in js} if j}
    raw_giant = {i: rot_key(ql, i) for i in split if i}
    ob, oa = M.mul_mat_hoisted(M.Ops(P), qs, ps, split, diags, raw_baby, raw_giant, ctb, cta)
    got = decode(decrypt(ql, ob, oa), scale * scale / qs[-1])
    err = max(np.max(np.abs(got.real - want.real)), np.max(np.abs(got.imag - want.imag)))
    print("model, hoisted product: max slot error 2^%.1f" % math.log2(err))
    assert err < 2.0 ** -30


def to_ints3(a):
    return [to_ints(x) for x in a]
