"""The pass-0 side of the wave-local transforms (csrc/ntt14w.hpp) deals every thread coefficient pairs (i, i + 1) and moves them
with 16-byte accesses.  Bit-exact against the oracle (oracle/cref.py) for what that addressing could break: N = 2^12, 2^13, 2^14,
an input whose value encodes its own position next to random input, forward alone, inverse alone on oracle evaluations, the ring
product (its right operand is transformed out of place), batch sizes 1, 3 and one above 512, a slice that starts at an odd
polynomial of a larger buffer, and the rejection of operands that are not 16-byte aligned."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOG_NS = (12, 13, 14)
Q60 = 1152921504606748673  # cfg2: two-operand twiddles (ArithDS)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def to_dev(torch, a):
    return torch.from_numpy(a.view(np.int64)).cuda()


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


def moduli(cref, log_n):
    """both arithmetic policies of the wave-local kernels: 60 bits (ArithDS) and 45 bits (Shoup)"""
    return (Q60, cref.two_adic_primes(45, log_n + 1, 1)[0])


def inputs(q, n, batch, seed):
    """(name, array): position-coded (value = 1 + index in the whole buffer, far below q) and uniform random"""
    coded = np.arange(1, n * batch + 1, dtype=np.uint64)
    rng = np.random.Generator(np.random.PCG64(seed))
    return (("coded", coded), ("random", rng.integers(0, q, size=n * batch, dtype=np.uint64)))


def same(got, exp, n, what):
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, "%s: %d mismatches, first at (polynomial, coefficient) %s: got %s, expected %s" % (
        what, bad.size, [(int(i) // n, int(i) % n) for i in bad[:8]], got[bad[:8]].tolist(), exp[bad[:8]].tolist())


@pytest.mark.parametrize("log_n", LOG_NS)
@pytest.mark.parametrize("batch", (1, 3, 515))
def test_forward_and_inverse_alone(fhe, cref, torch_cuda, log_n, batch):
    n = 1 << log_n
    for q in moduli(cref, log_n):
        ctx = fhe.NttContext(q)
        for name, a in inputs(q, n, batch, 100 * log_n + batch):
            what = "N=2^%d q=%d batch=%d %s" % (log_n, q, batch, name)
            exp = cref.ntt_fwd(q, a, n, threads=8)
            d = to_dev(torch_cuda, a)
            ctx.ntt_(d, n)
            same(to_host(d), exp, n, "forward " + what)
            # inverse alone on the oracle's evaluations: on the coded input a wrong value names the coefficient that arrived instead
            d = to_dev(torch_cuda, exp)
            ctx.intt_(d, n)
            same(to_host(d), a, n, "inverse " + what)


@pytest.mark.parametrize("log_n", LOG_NS)
@pytest.mark.parametrize("batch", (1, 3, 515))
def test_ring_product(fhe, cref, torch_cuda, log_n, batch):
    """fhe_ntt_mul: b goes through the out-of-place forward (2^12: then the multiplying inverse; 2^13, 2^14: the fused kernel)"""
    n = 1 << log_n
    for q in moduli(cref, log_n):
        if batch > 3 and q != Q60:
            continue  # the large batch once per size
        ctx = fhe.NttContext(q)
        (_, coded), (_, rnd) = inputs(q, n, batch, 7 * log_n + batch)
        for a, b in ((coded, rnd), (rnd, coded)):
            da, db = to_dev(torch_cuda, a), to_dev(torch_cuda, b)
            ctx.mul_(da, db, n)
            same(to_host(da), cref.ntt_mul(q, a, b, n), n, "product N=2^%d q=%d batch=%d" % (log_n, q, batch))
            same(to_host(db), b, n, "right operand untouched")


@pytest.mark.parametrize("log_n", LOG_NS)
def test_out_of_place_forward(fhe, cref, torch_cuda, log_n):
    """a = 1 makes the product the right operand itself: forward out of place, times the evaluations of 1, inverse"""
    n, batch = 1 << log_n, 5
    for q in moduli(cref, log_n):
        ctx = fhe.NttContext(q)
        one = np.zeros(n * batch, dtype=np.uint64)
        one[0::n] = 1
        for name, b in inputs(q, n, batch, 31 + log_n):
            da, db = to_dev(torch_cuda, one), to_dev(torch_cuda, b)
            ctx.mul_(da, db, n)
            same(to_host(da), b, n, "1 * b N=2^%d q=%d %s" % (log_n, q, name))


@pytest.mark.parametrize("log_n", LOG_NS)
def test_slice_at_odd_polynomial(fhe, cref, torch_cuda, log_n):
    """three polynomials from polynomial 1 of a buffer of five; the neighbours stay as they were"""
    n, q = 1 << log_n, Q60
    ctx = fhe.NttContext(q)
    for name, buf in inputs(q, n, 5, 55 + log_n):
        d = to_dev(torch_cuda, buf)
        view = d[n:4 * n]
        ctx.ntt_(view, n)
        exp = buf.copy()
        exp[n:4 * n] = cref.ntt_fwd(q, buf[n:4 * n], n)
        same(to_host(d), exp, n, "forward on a slice, N=2^%d %s" % (log_n, name))
        ctx.intt_(view, n)
        same(to_host(d), buf, n, "inverse on a slice, N=2^%d %s" % (log_n, name))
        other = to_dev(torch_cuda, buf)
        ctx.mul_(view, other[2 * n:5 * n], n)  # both operands start inside their buffers
        exp = buf.copy()
        exp[n:4 * n] = cref.ntt_mul(q, buf[n:4 * n], buf[2 * n:5 * n], n)
        same(to_host(d), exp, n, "product on slices, N=2^%d %s" % (log_n, name))


@pytest.mark.parametrize("log_n", LOG_NS)
def test_misaligned_source_is_rejected(fhe, cref, torch_cuda, log_n):
    """the out-of-place forward reads 16 bytes per lane: a right operand 8 bytes off a 16-byte boundary is FHE_ERR_INVALID and
    nothing is written; the same values at an aligned address go through"""
    n, q, batch = 1 << log_n, Q60, 2
    ctx = fhe.NttContext(q)
    (_, a), (_, b) = inputs(q, n, batch, 77 + log_n)
    room = torch_cuda.zeros(n * batch + 2, dtype=torch_cuda.int64, device="cuda")
    assert room.data_ptr() % 16 == 0
    off = room[1:1 + n * batch]
    off.copy_(to_dev(torch_cuda, b))
    assert off.data_ptr() % 16 == 8
    da = to_dev(torch_cuda, a)
    with pytest.raises(fhe.FheError) as e:
        ctx.mul_(da, off, n)
    assert e.value.code == 1  # FHE_ERR_INVALID
    same(to_host(da), a, n, "left operand after the rejected call")
    ok = room[2:2 + n * batch]
    ok.copy_(to_dev(torch_cuda, b))
    ctx.mul_(da, ok, n)
    same(to_host(da), cref.ntt_mul(q, a, b, n), n, "aligned right operand")


@pytest.mark.parametrize("log_n", (12, 13, 14, 15))
def test_misaligned_polynomials_are_rejected(fhe, cref, torch_cuda, log_n):
    """the operand transformed in place is read and written 16 bytes per lane as well: forward, inverse and the product (fused at
    2^13 .. 2^15) reject an `a` that is 8 bytes off and leave it as it was"""
    n, batch = 1 << log_n, 2
    q = Q60 if log_n <= 14 else cref.two_adic_primes(60, log_n + 1, 1)[0]  # q - 1 = 2^15 (2^45 - 3): no 2^16-th root
    ctx = fhe.NttContext(q)
    (_, a), (_, b) = inputs(q, n, batch, 91 + log_n)
    room = torch_cuda.zeros(n * batch + 2, dtype=torch_cuda.int64, device="cuda")
    off = room[1:1 + n * batch]
    off.copy_(to_dev(torch_cuda, a))
    assert off.data_ptr() % 16 == 8
    db = to_dev(torch_cuda, b)
    for call in (lambda: ctx.ntt_(off, n), lambda: ctx.intt_(off, n), lambda: ctx.mul_(off, db, n)):
        with pytest.raises(fhe.FheError) as e:
            call()
        assert e.value.code == 1  # FHE_ERR_INVALID
        same(to_host(off), a, n, "operand after the rejected call, N=2^%d" % log_n)
    same(to_host(db), b, n, "right operand")
