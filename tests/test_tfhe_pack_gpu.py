"""GPU tests of the packing key switch (k = 1): fhe_tlwe_pack bit-exact against the model of tests/tfhe_pack_model.py and against the
composed route (fhe_tlwe_pfks, fhe_tglwe_rotate, sums) in both memory kinds, every digit width, every ring, both internal routes
(PACK_ROUTE), every schedule of the lab switch PACK_SPLIT, several launch groups (PACK_SLAB) and on both sides of the exactness bound;
the decode level with device-made keys; rejections; a side stream; the C demo."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import tfhe_cbs_model as CM
import tfhe_pack_model as M

pytestmark = pytest.mark.gpu

M64 = 1 << 64
U = lambda x: np.array(x, dtype=np.uint64)  # noqa: E731


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def r64(rng, *shape):
    return rng.integers(0, 1 << 63, size=shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)


def edge_words(log_b, d):
    """0, 2^63, 2^63 - 1, 2^64 - 1, values whose digits are all +2^(log_b - 1) resp. -2^(log_b - 1) (a carry through every level), and the
    rounding ties: half a unit of the last digit above and just below"""
    rb, half = 64 - log_b * d, 1 << (log_b - 1)
    up = sum(half << (rb + j * log_b) for j in range(d)) % M64
    tie = (1 << rb) // 2
    return [0, 1 << 63, (1 << 63) - 1, M64 - 1, up, (-up) % M64, (up + tie - (1 if rb else 0)) % M64, tie, (tie - 1) % M64, (M64 - tie) % M64]


def inputs(rng, log_b, d, n_in, n, count, packs):
    key = r64(rng, d * (n_in + 1), 1, 2, n)
    key[:, 0, :, 0] = np.uint64(M64 - 1)                  # whole columns of 2^64 - 1 and of 2^63
    key[:, 0, 1, n - 1] = np.uint64(1 << 63)
    ct_a, ct_b = r64(rng, packs, count, n_in), r64(rng, packs, count)
    e = edge_words(log_b, d)
    flat = ct_a.reshape(-1)
    flat[:min(len(e), flat.size)] = U(e)[:flat.size]      # the first ciphertext(s) start with the edge words
    ct_b[0, 0] = np.uint64(e[4])
    ct_b[packs - 1, count - 1] = np.uint64(e[5])
    return key, ct_a, ct_b


def run_both_memories(fhe, torch, t, log_b, d, n_in, n, count, stride, key, ct_a, ct_b, composed=True):
    """-> the model's (out_a, out_b); asserts the library's bits on device and host memory, and the composed route's"""
    P = fhe.tfhe_pack
    want_a, want_b = M.pack(log_b, d, key, ct_a, ct_b, n_in, n, count, stride)
    dk, da, db = dev(torch, key), dev(torch, ct_a), dev(torch, ct_b)
    pk = P.PackKey(t, log_b, d, dk, n_in, n)
    try:
        for route in (0, 1, 2):  # the library's rule, the transforms, the scalar product
            fhe.set_option("PACK_ROUTE", route)
            ga, gb = P.pack(pk, da, db, count, stride)
            assert np.array_equal(host(ga), want_a) and np.array_equal(host(gb), want_b), ("device memory", route)
    finally:
        fhe.set_option("PACK_ROUTE", 0)
    hk = P.PackKey(t, log_b, d, key, n_in, n)
    ha, hb = P.pack(hk, ct_a, ct_b, count, stride)
    assert np.array_equal(ha, want_a) and np.array_equal(hb, want_b), "host memory"
    if composed:
        ca, cb = P.pack_composed(log_b, d, dk, da, db, n_in, n, count, stride)
        assert np.array_equal(host(ca), want_a) and np.array_equal(host(cb), want_b), "composed route"
    pk.destroy()
    hk.destroy()
    return want_a, want_b


@pytest.mark.parametrize("log_b,d", [(4, 1), (7, 3), (9, 2), (16, 4)])
@pytest.mark.parametrize("n_in", [5, 8])
@pytest.mark.parametrize("count,stride,packs", [(1, 1, 1), (3, 1, 2), (3, 85, 1), (256, 1, 1), (16, 16, 3)])
def test_pack_bit_exact_vs_model_and_composed(fhe, torch_cuda, log_b, d, n_in, count, stride, packs):
    """n = 256: byte, 16-bit and 32-bit digits; one input, a few, the last admissible stride, a full ring, several packs"""
    n = 256
    rng = np.random.Generator(np.random.PCG64(9100 + 1000 * log_b + 10 * n_in + count + stride))
    key, ct_a, ct_b = inputs(rng, log_b, d, n_in, n, count, packs)
    run_both_memories(fhe, torch_cuda, fhe.TorusContext(), log_b, d, n_in, n, count, stride, key, ct_a, ct_b)


@pytest.mark.parametrize("n,n_in,log_b,d,count,stride", [(512, 8, 7, 3, 512, 1), (1024, 8, 7, 3, 1024, 1), (2048, 16, 8, 2, 17, 120)])
def test_pack_every_ring(fhe, torch_cuda, n, n_in, log_b, d, count, stride):
    """the other team shapes: one wave of 8 coefficients per lane (512), four and eight waves of 4 per lane (1024, 2048)"""
    rng = np.random.Generator(np.random.PCG64(9200 + n))
    key, ct_a, ct_b = inputs(rng, log_b, d, n_in, n, count, 1)
    run_both_memories(fhe, torch_cuda, fhe.TorusContext(), log_b, d, n_in, n, count, stride, key, ct_a, ct_b)


def test_every_schedule_gives_the_same_bits(fhe, torch_cuda):
    """n = 256, n_in = 8, (7, 3): 27 key rows as one chunk, two, three and 27 chunks of one row (atomic adds into zeroed outputs), and
    the library's rule: all equal to the model"""
    n, n_in, log_b, d, count = 256, 8, 7, 3, 256
    rng = np.random.Generator(np.random.PCG64(9300))
    key, ct_a, ct_b = inputs(rng, log_b, d, n_in, n, count, 2)
    want_a, want_b = M.pack(log_b, d, key, ct_a, ct_b, n_in, n, count, 1)
    pk = fhe.PackKey(fhe.TorusContext(), log_b, d, dev(torch_cuda, key), n_in, n)
    da, db = dev(torch_cuda, ct_a), dev(torch_cuda, ct_b)
    try:
        fhe.set_option("PACK_ROUTE", 1)
        for split in (1, 2, 3, 27, 0):
            fhe.set_option("PACK_SPLIT", split)
            ga, gb = fhe.pack(pk, da, db, count, 1)
            assert np.array_equal(host(ga), want_a) and np.array_equal(host(gb), want_b), split
    finally:
        fhe.set_option("PACK_SPLIT", 0)
        fhe.set_option("PACK_ROUTE", 0)
    pk.destroy()


def test_bound_edges(fhe, torch_cuda):
    """log_b = 31, d = 2 at n = 2048 (the tightest bound of the two primes: 4095 rows per chunk) with n_in = 8 (18 rows: one chunk) and
    with n_in = 2047 (4096 rows: the rule must cut, even under PACK_SPLIT = 1), inputs at the digit extremes; both equal to the model"""
    n, log_b, d = 2048, 31, 2
    t = fhe.TorusContext()
    rng = np.random.Generator(np.random.PCG64(9400))
    key, ct_a, ct_b = inputs(rng, log_b, d, 8, n, 17, 1)
    ct_a[0, 1, :] = np.uint64(edge_words(log_b, d)[4])      # every digit of a whole ciphertext at +2^30, and of another at -2^30
    ct_a[0, 2, :] = np.uint64(edge_words(log_b, d)[5])
    run_both_memories(fhe, torch_cuda, t, log_b, d, 8, n, 17, 120, key, ct_a, ct_b)
    n_in, count, stride = 2047, 2, 1500
    key, ct_a, ct_b = inputs(rng, log_b, d, n_in, n, count, 1)
    ct_a[0, 1, :] = np.uint64(edge_words(log_b, d)[4])
    want_a, want_b = M.pack(log_b, d, key, ct_a, ct_b, n_in, n, count, stride)
    pk = fhe.PackKey(t, log_b, d, dev(torch_cuda, key), n_in, n)
    da, db = dev(torch_cuda, ct_a), dev(torch_cuda, ct_b)
    try:
        fhe.set_option("PACK_ROUTE", 1)  # two inputs would take the scalar product: the bound is the transforms'
        for split in (1, 0):
            fhe.set_option("PACK_SPLIT", split)
            ga, gb = fhe.pack(pk, da, db, count, stride)
            assert np.array_equal(host(ga), want_a) and np.array_equal(host(gb), want_b), split
        fhe.set_option("PACK_ROUTE", 2)
        ga, gb = fhe.pack(pk, da, db, count, stride)
        assert np.array_equal(host(ga), want_a) and np.array_equal(host(gb), want_b), "scalar product"
    finally:
        fhe.set_option("PACK_SPLIT", 0)
        fhe.set_option("PACK_ROUTE", 0)
    pk.destroy()


def test_unaligned_device_pointers(fhe, torch_cuda):
    """inputs, key and outputs that are 8 but not 16 bytes aligned: the same bits"""
    from learn_fhe_amd.ring import _buf
    n, n_in, log_b, d, count, stride, packs = 256, 5, 7, 3, 3, 85, 2
    rng = np.random.Generator(np.random.PCG64(9500))
    key, ct_a, ct_b = inputs(rng, log_b, d, n_in, n, count, packs)
    want_a, want_b = M.pack(log_b, d, key, ct_a, ct_b, n_in, n, count, stride)
    odd = lambda a: dev(torch_cuda, np.concatenate([U([0]), a.ravel()]))[1:]  # noqa: E731
    dk, da, db = odd(key), odd(ct_a), odd(ct_b)
    oa, ob = odd(np.zeros(packs * n, dtype=np.uint64)), odd(np.zeros(packs * n, dtype=np.uint64))
    assert all(x.data_ptr() % 16 == 8 for x in (dk, da, db, oa, ob))
    t = fhe.TorusContext()
    pk = fhe.PackKey(t, log_b, d, dk, n_in, n)
    P = lambda x: _buf(x)[0]  # noqa: E731
    try:
        for route in (1, 2):
            fhe.set_option("PACK_ROUTE", route)
            oa.zero_()
            ob.zero_()
            assert fhe.lib().fhe_tlwe_pack(t.handle, pk._h, P(da), P(db), count, stride, packs, P(oa), P(ob), _buf(da)[2], _buf(da)[3]) == 0
            assert np.array_equal(host(oa).reshape(packs, n), want_a) and np.array_equal(host(ob).reshape(packs, n), want_b), route
    finally:
        fhe.set_option("PACK_ROUTE", 0)
    pk.destroy()


def test_several_launch_groups(fhe, torch_cuda):
    """five packs in groups of two (PACK_SLAB = 2: two full groups and one of one pack, the scratch reused, inputs and outputs offset
    by the group's first pack) on both routes: the model's bits"""
    n, n_in, log_b, d, count, stride, packs = 256, 5, 9, 2, 7, 36, 5
    rng = np.random.Generator(np.random.PCG64(9550))
    key, ct_a, ct_b = inputs(rng, log_b, d, n_in, n, count, packs)
    want_a, want_b = M.pack(log_b, d, key, ct_a, ct_b, n_in, n, count, stride)
    pk = fhe.PackKey(fhe.TorusContext(), log_b, d, dev(torch_cuda, key), n_in, n)
    da, db = dev(torch_cuda, ct_a), dev(torch_cuda, ct_b)
    try:
        fhe.set_option("PACK_SLAB", 2)
        for route in (1, 2):
            fhe.set_option("PACK_ROUTE", route)
            ga, gb = fhe.pack(pk, da, db, count, stride)
            assert np.array_equal(host(ga), want_a) and np.array_equal(host(gb), want_b), route
    finally:
        fhe.set_option("PACK_SLAB", 0)
        fhe.set_option("PACK_ROUTE", 0)
    pk.destroy()


def test_rejections_write_nothing(fhe, torch_cuda):
    """(count - 1) stride >= n, count = 0, stride = 0, out_a == out_b, an output that is an input, a key of another context: each returns
    FHE_ERR_INVALID and leaves the outputs as they were; packs = 0 is FHE_OK and touches nothing; prepare's rejections"""
    from learn_fhe_amd.ring import _buf
    n, n_in, log_b, d, count, packs = 256, 5, 7, 3, 4, 2
    rng = np.random.Generator(np.random.PCG64(9600))
    D = lambda x: dev(torch_cuda, x)  # noqa: E731
    t, other = fhe.TorusContext(), fhe.TorusContext()
    dk = D(r64(rng, d * (n_in + 1), 1, 2, n))
    pk, foreign = fhe.PackKey(t, log_b, d, dk, n_in, n), fhe.PackKey(other, log_b, d, dk, n_in, n)
    a_np, b_np = r64(rng, packs, n, n_in), r64(rng, packs, n)   # room for count = n, so that no admitted call reads past them
    a, b = D(a_np), D(b_np)
    mark_a, mark_b = r64(rng, packs, n), r64(rng, packs, n)
    oa, ob = D(mark_a), D(mark_b)
    P = lambda x: _buf(x)[0]  # noqa: E731
    mem, st, lib = _buf(a)[2], _buf(a)[3], fhe.lib()

    def call(th=t.handle, key=pk, cnt=count, stride=1, out_a=oa, out_b=ob, ca=a, cb=b, nb=packs):
        return lib.fhe_tlwe_pack(th, key._h, P(ca), P(cb), cnt, stride, nb, P(out_a), P(out_b), mem, st)
    assert call(cnt=4, stride=86) == 1 and call(cnt=2, stride=256) == 1 and call(cnt=257) == 1    # (count - 1) stride >= n
    assert call(cnt=0) == 1 and call(stride=0) == 1
    assert call(out_b=oa) == 1                                                                      # out_a == out_b
    assert call(out_a=a) == 1 and call(out_b=a) == 1 and call(out_a=b) == 1 and call(out_b=b) == 1  # an output is an input
    assert call(key=foreign) == 1 and call(th=other.handle) == 1 and call(th=None) == 1             # a key of another context
    assert call(nb=0) == 0
    assert lib.fhe_tlwe_pack(t.handle, pk._h, None, P(b), count, 1, packs, P(oa), P(ob), mem, st) == 1
    torch_cuda.cuda.synchronize()
    assert np.array_equal(host(oa), mark_a) and np.array_equal(host(ob), mark_b)
    assert np.array_equal(host(a), a_np) and np.array_equal(host(b), b_np)
    # host memory: out_a == out_b
    ha = np.zeros((packs, n), dtype=np.uint64)
    hp = ctypes.c_void_p(ha.ctypes.data)
    assert lib.fhe_tlwe_pack(t.handle, pk._h, ctypes.c_void_p(a_np.ctypes.data), ctypes.c_void_p(b_np.ctypes.data), count, 1, packs, hp, hp, 0, None) == 1
    assert not ha.any()
    assert call() == 0 and call(cnt=1, stride=1 << 40) == 0                                         # and the admitted call runs
    h = ctypes.c_void_p()

    def prepare(lb=log_b, dd=d, ring=n, rows_in=n_in, key=dk):
        return lib.fhe_tlwe_pack_key_prepare(t.handle, lb, dd, P(key) if key is not None else None, rows_in, ring, mem, st, ctypes.byref(h))
    assert prepare(lb=7, dd=10) == 1 and not h.value                 # log_b d > 64
    assert prepare(lb=32, dd=2) == 6 and not h.value                 # log_b > 31
    assert prepare(ring=128) == 1 and prepare(ring=4096) == 1 and prepare(ring=255) == 1 and prepare(rows_in=0) == 1 and prepare(key=None) == 1
    torch_cuda.cuda.synchronize()


def test_off_the_default_stream(fhe, torch_cuda):
    """the key's rows and the inputs are produced on a side stream immediately before prepare and the call, both on that stream"""
    torch = torch_cuda
    n, n_in, log_b, d, count, stride, packs = 1024, 8, 7, 3, 64, 16, 3
    rng = np.random.Generator(np.random.PCG64(9700))
    key, ct_a, ct_b = inputs(rng, log_b, d, n_in, n, count, packs)
    want_a, want_b = M.pack(log_b, d, key, ct_a, ct_b, n_in, n, count, stride)
    mask = r64(rng, 1)[0]
    xk, xa, xb = dev(torch, key ^ mask), dev(torch, ct_a ^ mask), dev(torch, ct_b ^ mask)
    dmask = int(np.array([mask], dtype=np.uint64).view(np.int64)[0])
    t = fhe.TorusContext()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        spin = torch.zeros(1 << 24, dtype=torch.int64, device="cuda")
        for _ in range(8):
            spin += 1                                   # work in front, so that the operands are late
        dk = xk ^ dmask
        pk = fhe.PackKey(t, log_b, d, dk, n_in, n)
        da, db = xa ^ dmask, xb ^ dmask
        ga, gb = fhe.pack(pk, da, db, count, stride)
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(host(ga), want_a) and np.array_equal(host(gb), want_b)


def make_keys(fhe, torch, t, n, n_in, log_b, d, std_dev, seed):
    like = dev(torch, U([0]))
    z, s = fhe.sample_binary(seed, 0, like, n_in), fhe.sample_binary(seed, 1, like, n)
    pfksk = fhe.tfhe_cbs.pfksk_gen(t, log_b, d, z, s, fhe.pack_funcs(n, like), std_dev, seed + 1, 2)
    return z, s, pfksk


def test_noise_free_key_packs_exactly_up_to_the_rounding_bound(fhe, torch_cuda):
    """keys at std_dev = 0, n = 256, n_in = 8, gadget (8, 4): 16 messages m_r << 60 at stride 16.  The phase at 16 r is the input's phase
    up to the rounding of the digits, at most (n_in + 1) 2^(63 - log_b d) (the bound test_noise_free_rows_are_exact_up_to_the_rounding_bound
    derives, |F|_1 = 1); every other coefficient's phase is exactly 0; sample_extract(16 r) decrypts to m_r"""
    from oracle import pyref as P
    n, n_in, log_b, d, count, stride = 256, 8, 8, 4, 16, 16
    t = fhe.TorusContext()
    z, s, pfksk = make_keys(fhe, torch_cuda, t, n, n_in, log_b, d, 0.0, 9800)
    msgs = [(5 * r + 3) % 16 for r in range(count)]
    ca, cb = fhe.tlwe_sk_encrypt(z, dev(torch_cuda, U([m << 60 for m in msgs])), n_in, count, 0.0, 9803, 0)
    pk = fhe.PackKey(t, log_b, d, pfksk, n_in, n)
    oa, ob = fhe.pack(pk, ca, cb, count, stride)
    zh, sh = host(z), host(s)
    phase = CM.tglwe_phase(sh, host(oa).reshape(n), host(ob).reshape(n))
    bound = (n_in + 1) * (1 << (63 - log_b * d))
    ha, hb = host(ca).reshape(count, n_in), host(cb)
    for r in range(count):
        in_phase = P.tlwe_phase([int(x) for x in zh], [int(x) for x in ha[r]], int(hb[r]))
        assert in_phase == msgs[r] << 60
        err = P.t64_to_i64((int(phase[r * stride]) - in_phase) % M64)
        assert abs(err) <= bound, (r, err, bound)
        ea, eb = fhe.tglwe_sample_extract(oa, ob, n, r * stride)
        got = P.tlwe_phase([int(x) for x in sh], [int(x) for x in host(ea).reshape(n)], int(host(eb)[0]))
        assert ((got + (1 << 59)) % M64) >> 60 == msgs[r]
    rest = np.ones(n, dtype=bool)
    rest[::stride] = False
    assert not phase[rest].any()


def test_noisy_key_decodes(fhe, torch_cuda):
    """the key-switch parameters of the decode-level look-up test (n = 1024, n_in = 8, gadget (7, 6), key noise 2.845e-15, input noise
    2^-30): 16 four-bit messages at stride 64 decode after rounding to 4 bits, in the TGLWE phase and after sample_extract"""
    from oracle import pyref as P
    n, n_in, log_b, d, count, stride = 1024, 8, 7, 6, 16, 64
    t = fhe.TorusContext()
    z, s, pfksk = make_keys(fhe, torch_cuda, t, n, n_in, log_b, d, 2.845267479601915e-15, 9900)
    msgs = [(7 * r + 1) % 16 for r in range(count)]
    ca, cb = fhe.tlwe_sk_encrypt(z, dev(torch_cuda, U([m << 60 for m in msgs])), n_in, count, 2.0 ** -30, 9903, 0)
    pk = fhe.PackKey(t, log_b, d, pfksk, n_in, n)
    oa, ob = fhe.pack(pk, ca, cb, count, stride)
    sh = host(s)
    phase = CM.tglwe_phase(sh, host(oa).reshape(n), host(ob).reshape(n))
    assert [((int(phase[r * stride]) + (1 << 59)) % M64) >> 60 for r in range(count)] == msgs
    rest = np.ones(n, dtype=bool)
    rest[::stride] = False
    assert int(np.abs(phase[rest].view(np.int64)).max()) < 1 << 59   # error only
    ea, eb = fhe.tglwe_sample_extract(oa, ob, n, 5 * stride)
    got = P.tlwe_phase([int(x) for x in sh], [int(x) for x in host(ea).reshape(n)], int(host(eb)[0]))
    assert ((got + (1 << 59)) % M64) >> 60 == msgs[5]


def test_c_program_tfhe_pack(tmp_path, fhe):
    """examples/tfhe_pack_demo.c: 8 byte-sized messages encrypted as TLWE, packed at stride n / 8 and decrypted from the TGLWE phase in the
    program, from plain C against include/fhe_ring.h alone"""
    from conftest import ROOT
    lib_dir = os.path.dirname(fhe.lib_path())
    exe = tmp_path / "tfhe_pack_demo"
    cmd = ["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "tfhe_pack_demo.c"), "-o", str(exe),
           "-L", lib_dir, "-lfhe_ring", "-Wl,--allow-shlib-undefined", "-Wl,-rpath," + lib_dir, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tfhe_pack_demo ok" in r.stdout, r.stdout + r.stderr
    assert r.stdout.split("\n")[0] == "messages: 17 200 3 255 0 128 64 99"
