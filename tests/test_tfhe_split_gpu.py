"""The split TFHE blind rotation (csrc/torus_split_kernels.hpp): a cluster of G = 2 or 6 workgroups per ciphertext must give the bits of the
one-workgroup kernel (lab switch TFHE_SPLIT = 0) and of the exact oracle (oracle/cref.py), in every way a call reaches it, with a clean
status after every call; keys that are not eligible must not move.  The common shape is N = 1024 with the gadget (7, 3), the x3 form; key
rows as in test_tfhe_forms_gpu.py (uniform 64-bit words, one row all -2^63), the accumulator driven to extreme digits."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, LOG_B, D = 1024, 7, 3
GS = (2, 6)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def cus(torch_cuda):
    return torch_cuda.cuda.get_device_properties(0).multi_processor_count


def host(t):
    return t.cpu().numpy().view(np.uint64)


def dev(torch, x):
    return torch.from_numpy(np.array(x, dtype=np.uint64).view(np.int64)).cuda()  # (a copy: the shared inputs are read-only)


def r64(rng, *shape):
    return rng.integers(0, 1 << 63, size=shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)


def extreme_digits(log_b, d):
    """the torus value whose every digit is -2^(log_b - 1), the most negative balanced digit (test_torus_gpu.py)"""
    half = 1 << (log_b - 1)
    return np.uint64((-sum(half << (64 - log_b * (j + 1)) for j in range(d))) % (1 << 64))


@functools.lru_cache(maxsize=None)
def key_rows(n, log_b, d, count, small=False):
    """rows_a, rows_b [count][2d][n]: uniform 64-bit words, row 0 of entry 1 all -2^63 (small, for fft64: words in [-2^10, 2^10))"""
    rng = np.random.Generator(np.random.PCG64([9600, n, log_b, d, count]))
    if small:
        ra = rng.integers(-(1 << 10), 1 << 10, size=(count, 2 * d, n), dtype=np.int64).view(np.uint64)
        rb = rng.integers(-(1 << 10), 1 << 10, size=(count, 2 * d, n), dtype=np.int64).view(np.uint64)
        ra[1, 0, :] = np.int64(-(1 << 10)).view(np.uint64)
    else:
        ra, rb = r64(rng, count, 2 * d, n), r64(rng, count, 2 * d, n)
        ra[1, 0, :] = np.uint64(1 << 63)
    ra.setflags(write=False)
    rb.setflags(write=False)
    return ra, rb


@functools.lru_cache(maxsize=None)
def inputs(n, log_b, d, n_lwe, batch):
    """tables [2][n] (the first half of table 0: extreme digits), a_tilde [batch][n_lwe], b_tilde [batch].  The LAST row, the one the oracle
    checks, starts with a~ = 0 (the skipped step), 1 and 2N - 1; row 0 has a 0 elsewhere, so that the members of different clusters count
    their hand-offs differently."""
    rng = np.random.Generator(np.random.PCG64([9700, n, log_b, d, n_lwe, batch]))
    tables = r64(rng, 2, n)
    tables[0, : n // 2] = extreme_digits(log_b, d)
    a_t = rng.integers(1, 2 * n, size=(batch, n_lwe), dtype=np.uint64)
    b_t = rng.integers(0, 2 * n, size=batch, dtype=np.uint64)
    a_t[-1, :3] = [0, 1, 2 * n - 1]
    a_t[0, n_lwe - 1] = 0
    b_t[-1] = 2 * n - 1
    for x in (tables, a_t, b_t):
        x.setflags(write=False)
    return tables, a_t, b_t


@functools.lru_cache(maxsize=None)
def oracle_last(n, log_b, d, n_lwe, batch, table):
    """the exact rotation of the last ciphertext of inputs(...) through tables[table]"""
    from oracle import cref
    ra, rb = key_rows(n, log_b, d, n_lwe)
    tables, a_t, b_t = inputs(n, log_b, d, n_lwe, batch)
    ea, eb = cref.tfhe_blind_rotate(log_b, d, ra, rb, tables[table], a_t[-1:], b_t[-1:])
    return ea[0], eb[0]


def make_key(fhe, torch, n, log_b, d, count, form="x3"):
    ra, rb = key_rows(n, log_b, d, count, small=form == "fft64")
    key = fhe.TggswKey(fhe.TorusContext(), log_b, d, dev(torch, ra), dev(torch, rb), n, fft64=form == "fft64")
    assert key.form == form, "the host's rule moved this key"
    return key


def under(fhe, key, g, batch, want_g, run, like=True):
    """run() under TFHE_SPLIT = g: the query must say want_g, and the status must be clean afterwards (on the stream of the first output)"""
    try:
        fhe.set_option("TFHE_SPLIT", g)
        assert key.split(batch) == want_g, (g, batch)
        out = run()
        key.check(out[0] if like else None)
        return out
    finally:
        fhe.set_option("TFHE_SPLIT", -1)


def same(x, y):
    return all(np.array_equal(host(p), host(q)) for p, q in zip(x, y))


@pytest.mark.parametrize("which", ["one", "three", "fits", "over"])
@pytest.mark.parametrize("g", GS)
def test_forced_split_matches_one_workgroup_and_the_oracle(fhe, cref, torch_cuda, cus, g, which):
    """n_lwe = 5; batch 1 (the first run of the kernel there is), 3, CUs // G (the largest that splits) and CUs // G + 1 (the query says
    1 and the one-workgroup kernel runs: still right)"""
    batch = {"one": 1, "three": 3, "fits": cus // g, "over": cus // g + 1}[which]
    n_lwe = 5
    key = make_key(fhe, torch_cuda, N, LOG_B, D, n_lwe)
    tables, a_t, b_t = inputs(N, LOG_B, D, n_lwe, batch)
    run = lambda: key.blind_rotate(dev(torch_cuda, a_t), dev(torch_cuda, b_t), dev(torch_cuda, tables[0]))  # noqa: E731
    base = under(fhe, key, 0, batch, 1, run)
    got = under(fhe, key, g, batch, g if batch * g <= cus else 1, run)
    assert same(got, base)
    ea, eb = oracle_last(N, LOG_B, D, n_lwe, batch, 0)
    assert np.array_equal(host(got[0])[-1], ea) and np.array_equal(host(got[1])[-1], eb)


@pytest.mark.parametrize("g", GS)
def test_a_table_per_ciphertext(fhe, cref, torch_cuda, g):
    batch, n_lwe = 3, 5
    key = make_key(fhe, torch_cuda, N, LOG_B, D, n_lwe)
    tables, a_t, b_t = inputs(N, LOG_B, D, n_lwe, batch)
    idx = torch_cuda.tensor([1, 0, 1], dtype=torch_cuda.int32, device="cuda")
    run = lambda: key.blind_rotate_tables(dev(torch_cuda, a_t), dev(torch_cuda, b_t), dev(torch_cuda, tables), idx)  # noqa: E731
    base = under(fhe, key, 0, batch, 1, run)
    got = under(fhe, key, g, batch, g, run)
    assert same(got, base)
    ea, eb = oracle_last(N, LOG_B, D, n_lwe, batch, 1)
    assert np.array_equal(host(got[0])[-1], ea) and np.array_equal(host(got[1])[-1], eb)


@pytest.mark.parametrize("g", GS)
def test_host_memory(fhe, cref, torch_cuda, g):
    """numpy operands: mirrored, the timeout would come back in the return value (a word of the call's own); the key's word stays clean"""
    batch, n_lwe = 3, 5
    key = make_key(fhe, torch_cuda, N, LOG_B, D, n_lwe)
    tables, a_t, b_t = inputs(N, LOG_B, D, n_lwe, batch)
    run = lambda: key.blind_rotate(np.array(a_t), np.array(b_t), np.array(tables[0]))  # noqa: E731
    base = under(fhe, key, 0, batch, 1, run, like=False)
    got = under(fhe, key, g, batch, g, run, like=False)
    assert all(np.array_equal(np.asarray(p).view(np.uint64), np.asarray(q).view(np.uint64)) for p, q in zip(got, base))
    ea, eb = oracle_last(N, LOG_B, D, n_lwe, batch, 0)
    ga, gb = (np.asarray(x).view(np.uint64).reshape(batch, N) for x in got)
    assert np.array_equal(ga[-1], ea) and np.array_equal(gb[-1], eb)


@pytest.mark.parametrize("g", GS)
def test_a_side_stream(fhe, cref, torch_cuda, g):
    torch = torch_cuda
    batch, n_lwe = 3, 5
    key = make_key(fhe, torch, N, LOG_B, D, n_lwe)
    tables, a_t, b_t = inputs(N, LOG_B, D, n_lwe, batch)
    a, b, v = dev(torch, a_t), dev(torch, b_t), dev(torch, tables[0])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = under(fhe, key, g, batch, g, lambda: key.blind_rotate(a, b, v))  # the status check waits for the side stream
    side.synchronize()
    ea, eb = oracle_last(N, LOG_B, D, n_lwe, batch, 0)
    assert np.array_equal(host(got[0])[-1], ea) and np.array_equal(host(got[1])[-1], eb)
    assert same(got, under(fhe, key, 0, batch, 1, lambda: key.blind_rotate(a, b, v)))


@pytest.mark.parametrize("g", GS)
def test_two_calls_back_to_back(fhe, torch_cuda, g):
    """two calls on one stream with no wait between them: the second takes the workspace the first releases, control words included"""
    torch = torch_cuda
    n_lwe = 5
    key = make_key(fhe, torch, N, LOG_B, D, n_lwe)
    t1, a1, b1 = inputs(N, LOG_B, D, n_lwe, 3)
    t2, a2, b2 = inputs(N, LOG_B, D, n_lwe, 1)
    ops = [(dev(torch, a1), dev(torch, b1), dev(torch, t1[0])), (dev(torch, np.repeat(a2, 3, axis=0)), dev(torch, np.repeat(b2, 3)), dev(torch, t2[1]))]
    run = lambda: [t for o in ops for t in key.blind_rotate(*o)]  # noqa: E731
    base = under(fhe, key, 0, 3, 1, run)
    got = under(fhe, key, g, 3, g, run)
    key.check(got[2])
    assert same(got, base)
    assert not np.array_equal(host(got[0]), host(got[2]))


@pytest.mark.parametrize("g", GS)
def test_gadget_of_four_limbs(fhe, cref, torch_cuda, g):
    """(7, 2): 2d = 4 forward transforms per output"""
    batch, n_lwe, d = 3, 5, 2
    key = make_key(fhe, torch_cuda, N, LOG_B, d, n_lwe)
    tables, a_t, b_t = inputs(N, LOG_B, d, n_lwe, batch)
    run = lambda: key.blind_rotate(dev(torch_cuda, a_t), dev(torch_cuda, b_t), dev(torch_cuda, tables[0]))  # noqa: E731
    base = under(fhe, key, 0, batch, 1, run)
    got = under(fhe, key, g, batch, g, run)
    assert same(got, base)
    ea, eb = oracle_last(N, LOG_B, d, n_lwe, batch, 0)
    assert np.array_equal(host(got[0])[-1], ea) and np.array_equal(host(got[1])[-1], eb)


def test_a_long_walk(fhe, torch_cuda):
    """n_lwe = 630, batch 2, both G against the one-workgroup kernel: slab parity and epochs over hundreds of hand-offs"""
    batch, n_lwe = 2, 630
    key = make_key(fhe, torch_cuda, N, LOG_B, D, n_lwe)
    tables, a_t, b_t = inputs(N, LOG_B, D, n_lwe, batch)
    run = lambda: key.blind_rotate(dev(torch_cuda, a_t), dev(torch_cuda, b_t), dev(torch_cuda, tables[0]))  # noqa: E731
    base = under(fhe, key, 0, batch, 1, run)
    for g in GS:
        assert same(under(fhe, key, g, batch, g, run), base), g


def test_through_the_bootstraps(fhe, torch_cuda):
    """fhe_tfhe_bootstrap and fhe_tfhe_bootstrap_many at batch 2 reach the rotation through blind_rotate_dev: the same bits under 0, 2, 6"""
    torch = torch_cuda
    batch, n_lwe, ks_log_b, ks_d = 2, 5, 4, 3
    key = make_key(fhe, torch, N, LOG_B, D, n_lwe)
    rng = np.random.Generator(np.random.PCG64([9800]))
    ksk_a, ksk_b = dev(torch, r64(rng, N * ks_d, n_lwe)), dev(torch, r64(rng, N * ks_d))
    tables = r64(rng, 2, N)
    tables[0, : N // 2] = extreme_digits(LOG_B, D)
    lwe_a, lwe_b = dev(torch, r64(rng, batch, n_lwe)), dev(torch, r64(rng, batch))
    tb, idx = dev(torch, tables), torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    one = lambda: key.bootstrap(ks_log_b, ks_d, ksk_a, ksk_b, tb[0], lwe_a, lwe_b)  # noqa: E731
    many = lambda: key.bootstrap_many(ks_log_b, ks_d, ksk_a, ksk_b, tb, idx, 1, lwe_a, lwe_b)  # noqa: E731
    for run in (one, many):
        base = under(fhe, key, 0, batch, 1, run)
        for g in GS:
            assert same(under(fhe, key, g, batch, g, run), base), g
    # host memory: the bootstrap's own status word
    hone = lambda: key.bootstrap(ks_log_b, ks_d, host(ksk_a), host(ksk_b), np.array(tables[0]), host(lwe_a), host(lwe_b))  # noqa: E731
    base = under(fhe, key, 0, batch, 1, hone, like=False)
    got = under(fhe, key, 6, batch, 6, hone, like=False)
    assert all(np.array_equal(np.asarray(p).view(np.uint64), np.asarray(q).view(np.uint64)) for p, q in zip(got, base))


@pytest.mark.parametrize("form,n,log_b,d", [("60", 1024, 23, 1), ("30", 1024, 10, 2), ("fft64", 1024, 6, 3), ("x3", 512, 7, 3)],
                         ids=["60", "30", "fft64", "x3-n512"])
def test_keys_that_are_not_eligible_stay_where_they_are(fhe, torch_cuda, form, n, log_b, d):
    batch, n_lwe = 3, 5
    key = make_key(fhe, torch_cuda, n, log_b, d, n_lwe, form)
    tables, a_t, b_t = inputs(n, log_b, d, n_lwe, batch)
    run = lambda: key.blind_rotate(dev(torch_cuda, a_t), dev(torch_cuda, b_t), dev(torch_cuda, tables[0]))  # noqa: E731
    base = under(fhe, key, 0, batch, 1, run)
    for g in GS:
        assert same(under(fhe, key, g, batch, 1, run), base)
