"""CKKS polynomial evaluation on the device (include/fhe_ring.h fhe_ckks_lincomb, fhe_ckks_mul_eval, fhe_ckks_poly_prepare / _apply):
bit-exact against the big-integer model of tests/ckks_poly_model.py and against the composition of the small public entries, and at
decode level against numpy.

Measured on the MI355X: the figures are printed by every decode-level test before it asserts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ckks_poly_model as PM  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID = 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def poly(fhe):
    return fhe.ckks_poly


def dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.complex128 else a.view(np.int64)).cuda()


def host(t):
    a = t.cpu().numpy()
    return a if a.dtype == np.complex128 else a.view(np.uint64)


def limbs_of(arr, b):
    """[batch][limbs][n] uint64 -> the model's list of limbs of ciphertext b"""
    return [[int(v) for v in row] for row in arr[b]]


def random_ct(rng, mods, batch, limbs, n, fill="random"):
    """one half [batch][limbs][n]: reduced on the first len(mods) limbs, arbitrary words on the limbs nobody may read"""
    out = rng.integers(0, 1 << 62, (batch, limbs, n), dtype=np.uint64)
    for l, q in enumerate(mods):
        out[:, l] = {"random": out[:, l] % np.uint64(q), "max": np.uint64(q - 1), "zero": np.uint64(0)}[fill]
    return out


# ---- 1. fhe_ckks_lincomb against the model --------------------------------------------------------------------------------------------
def base(cref, kind, log_n, ell):
    from oracle import pyref as P
    if kind == "ckks55":
        qs, ps = P.ckks_primes(log_n, 55, ell)
        return qs, ps[:1]
    bits = {"b60": 60, "b31": 31, "b62": 62}[kind]
    pr = cref.two_adic_primes(bits, log_n + 1, ell + 1)
    return list(pr[:ell]), list(pr[ell:])


def lincomb_case(fhe, poly, torch, cref, kind, n, batch, terms, ell, real, fill, seed, memory="device"):
    log_n = n.bit_length() - 1
    qs, ps = base(cref, kind, log_n, ell)
    scale = qs[-1]
    rns = fhe.RnsContext(qs, ps)
    rng = np.random.Generator(np.random.PCG64(seed))
    limbs = [ell + (j % 3) for j in range(terms)]  # mixed, the smallest exactly ell
    cts = [(random_ct(rng, qs, batch, lj, n, fill), random_ct(rng, qs, batch, lj, n, fill)) for lj in limbs]
    if real:
        # 0, a negative constant, |k| just under q_0, then random ones
        mults = [np.nextafter((qs[0] - 1) / scale, 0.0), -0.37, 0.0, -np.nextafter((qs[0] - 1) / scale, 0.0)] + list(rng.uniform(-2, 2, 16))
        c0 = -0.625
    else:
        mults = [qs[0] - 1, -1, 0, -(qs[0] - 1), 2, -2] + [int(v) for v in rng.integers(-1 << 62, 1 << 62, 16)]
        c0 = 1.0 - 2.0 ** -40
    mults = mults[:terms]
    put = (lambda a: dev(torch, a)) if memory == "device" else (lambda a: a)
    gb, ga = poly.lincomb(rns, [(put(b), put(a)) for b, a in cts], n, real, mults, c0, scale)
    gb, ga = (host(gb), host(ga)) if memory == "device" else (gb, ga)
    assert gb.shape == (batch, ell - 1 if real else ell, n)
    for b in range(batch):
        wb, wa = PM.lincomb(qs, [(limbs_of(cb, b), limbs_of(ca, b)) for cb, ca in cts], real, mults, c0, scale)
        assert np.array_equal(gb[b], np.array(wb, dtype=np.uint64)), "b half, ciphertext %d" % b
        assert np.array_equal(ga[b], np.array(wa, dtype=np.uint64)), "a half, ciphertext %d" % b


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("ell", [2, 5])
@pytest.mark.parametrize("terms", [1, 2, 16])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [2, 16, 4096])
def test_lincomb_equals_the_model(fhe, poly, torch_cuda, cref, n, batch, terms, ell, real):
    """pseudo-Mersenne 55-bit chain (the rescale constants every CKKS parameter set of the reference uses); n = 2 and 16 lie below, 4096 on
    the wave-local transform sizes -- the linear combination itself is size-blind, the sizes are the ones its neighbours differ at"""
    lincomb_case(fhe, poly, torch_cuda, cref, "ckks55", n, batch, terms, ell, real, "random", 7 * n + terms)


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("fill", ["max", "zero"])
@pytest.mark.parametrize("kind", ["b60", "b31", "b62", "ckks55"])
def test_lincomb_edges_of_the_moduli(fhe, poly, torch_cuda, cref, kind, fill, real):
    """every input q - 1 (the largest unreduced sum: 16 terms of (q - 1)^2) or 0, on a 60-bit and a 31-bit base, and on primes in
    [2^61, 2^62), which take the route that reduces every product"""
    lincomb_case(fhe, poly, torch_cuda, cref, kind, 16, 3, 16, 5, real, fill, 99)


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("kind", ["b60", "b31", "b62"])
def test_lincomb_other_bases(fhe, poly, torch_cuda, cref, kind, real):
    lincomb_case(fhe, poly, torch_cuda, cref, kind, 16, 3, 16, 5, real, "random", 5)
    lincomb_case(fhe, poly, torch_cuda, cref, kind, 4096, 1, 2, 2, real, "random", 6)


@pytest.mark.parametrize("real", [False, True])
def test_lincomb_host_memory_and_in_place(fhe, poly, torch_cuda, cref, real):
    lincomb_case(fhe, poly, torch_cuda, cref, "ckks55", 16, 3, 16, 5, real, "random", 11, memory="host")
    if real:
        return
    from oracle import pyref as P
    n, ell, batch = 16, 3, 2
    qs, ps = P.ckks_primes(4, 55, ell)
    rns = fhe.RnsContext(qs, ps[:1])
    rng = np.random.Generator(np.random.PCG64(12))
    x = (random_ct(rng, qs, batch, ell, n), random_ct(rng, qs, batch, ell, n))
    y = (random_ct(rng, qs, batch, ell + 1, n), random_ct(rng, qs, batch, ell + 1, n))
    dx, dy = (dev(torch_cuda, x[0]), dev(torch_cuda, x[1])), (dev(torch_cuda, y[0]), dev(torch_cuda, y[1]))
    wb, wa = poly.lincomb(rns, [dx, dy], n, False, [2, -1], 0.5, qs[-1])
    poly.lincomb(rns, [dx, dy], n, False, [2, -1], 0.5, qs[-1], out=dx)   # in place: the output is input 0 (limbs == l)
    assert torch_cuda.equal(dx[0], wb) and torch_cuda.equal(dx[1], wa)


def test_lincomb_refusals(fhe, poly, torch_cuda):
    from oracle import pyref as P
    from learn_fhe_amd import _lib
    lib = _lib.lib()
    n, ell = 16, 3
    qs, ps = P.ckks_primes(4, 55, ell)
    rns, one = fhe.RnsContext(qs, ps[:1]), fhe.RnsContext(qs[:1], ps[:1])
    t = dev(torch_cuda, np.zeros((1, ell, n), dtype=np.uint64))
    o = dev(torch_cuda, np.zeros((1, ell, n), dtype=np.uint64))
    vp = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def call(h=rns.handle, real=0, k=1, limbs=ell, c=1.0, c0=0.0, scale=qs[-1], ptr=vp(t), out=vp(o), batch=1, kmax=17):
        bs = (C.c_void_p * kmax)(*[ptr.value] * kmax)
        return lib.fhe_ckks_lincomb(h, real, k, bs, bs, (C.c_int * kmax)(*[limbs] * kmax), (C.c_int64 * kmax)(*[1] * kmax), (C.c_double * kmax)(*[c] * kmax),
                                    c0, scale, out, out, n, batch, _lib.MEM_DEVICE, None)

    assert call() == 0 and call(real=1) == 0 and call(k=16) == 0
    assert call(batch=0) == 0
    assert call(k=17) == INVALID and call(k=0) == INVALID
    assert call(limbs=ell - 1) == INVALID
    assert call(h=None) == INVALID and call(ptr=C.c_void_p(0)) == INVALID and call(out=None) == INVALID
    assert call(real=1, c=float("nan")) == INVALID and call(c0=float("inf")) == INVALID
    assert call(real=1, c=2.0 ** 72) == INVALID                     # scale > 2^54: |c scale| >= 2^126
    assert call(real=0, c=float("nan")) == 0                        # integer mode never reads the real multipliers
    assert call(h=one.handle, real=1, limbs=1) == INVALID           # l < 2 in real mode
    assert call(h=one.handle, real=0, limbs=1) == 0
    assert call(scale=0) == INVALID


# ---- a small scheme instance ----------------------------------------------------------------------------------------------------------
class Instance:
    def __init__(self, fhe, torch, log_n, big_l, seed=900):
        from oracle import pyref as P
        self.fhe, self.torch, self.seed = fhe, torch, seed
        self.n, self.l, self.L = 1 << log_n, 1 << (log_n - 1), big_l
        self.qs, self.ps = P.ckks_primes(log_n, 55, big_l)
        self.scale = self.qs[-1]
        self.ctx = {lv: fhe.RnsContext(self.qs[:lv], self.ps) for lv in range(1, big_l + 1)}
        like = dev(torch, np.zeros(1, dtype=np.uint64))
        self.sk = fhe.sample_zo(0.5, seed, 0, like, self.n)
        self.rlk = self.ctx[big_l].ksk_gen(self.sk, None, self.n, seed + 1, 0)
        self._keys, self._enc = {}, None

    def cut_key(self, lv):
        return tuple(self.torch.cat([k[:lv], k[self.L:]]).contiguous() for k in self.rlk)

    def key(self, lv):
        if lv not in self._keys:
            self._keys[lv] = self.fhe.CkksKey(self.ctx[lv], *self.cut_key(lv), self.n)
        return self._keys[lv]

    @property
    def enc(self):
        if self._enc is None:
            self._enc = self.fhe.CkksEncoder(self.n)
        return self._enc

    def random_ct(self, batch, lv, seed):
        rng = np.random.Generator(np.random.PCG64(seed))
        return tuple(dev(self.torch, random_ct(rng, self.qs[:lv], batch, lv, self.n)) for _ in range(2))

    def encrypt(self, m, lv):
        ctx = self.ctx[lv]
        pk_b, pk_a = ctx.sk_encrypt(self.sk, None, self.n, 1, self.seed + 2, 0)
        pt = self.enc.encode(ctx, self.scale, dev(self.torch, np.ascontiguousarray(m, dtype=np.complex128)))
        return ctx.pk_encrypt(pk_b[0].contiguous(), pk_a[0].contiguous(), pt, self.n, m.shape[0], self.seed + 3, 0)

    def constant(self, c, lv):
        """`Ckks::encode` of the constant slot vector c on lv limbs: [1][lv][n]"""
        return self.enc.encode(self.ctx[lv], self.scale, dev(self.torch, np.full((1, self.l), c, dtype=np.complex128)))

    def decode(self, lv, cb, ca):
        return host(self.enc.decode(self.ctx[lv], self.scale, self.ctx[lv].decrypt(self.sk, cb, ca, self.n)))

    def evaluator(self, plan, top, extra_levels=0):
        lv = [self.ctx[x] for x in range(top, top - plan.depth - 1 - extra_levels, -1)]
        kb, ka = self.cut_key(top)
        return self.fhe.CkksPolyEval(plan, lv, self.scale, kb, ka, self.n)


_INSTANCES = {}


def instance(fhe, torch, log_n, big_l):
    if (log_n, big_l) not in _INSTANCES:
        _INSTANCES[(log_n, big_l)] = Instance(fhe, torch, log_n, big_l)
    return _INSTANCES[(log_n, big_l)]


# ---- 2. fhe_ckks_mul_eval ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,with_c", [(1, False), (2, False), (1, True), (2, True)])
@pytest.mark.parametrize("log_n", [4, 12])
def test_mul_eval_equals_mul_then_lincomb(fhe, poly, torch_cuda, log_n, alpha, with_c):
    """operands on 5 and 4 limbs in the evaluation domain, the product on 4: the bits of fhe_ckks_mul on the prefix slices followed by
    the integer-mode fhe_ckks_lincomb {alpha, -1}; the subtrahend sits on 4 limbs, one more than the result"""
    inst = instance(fhe, torch_cuda, log_n, 5)
    n = inst.n
    x, y, c = inst.random_ct(2, 5, 21), inst.random_ct(2, 4, 22), inst.random_ct(2, 4, 23)
    xe = tuple(inst.ctx[5].ntt_(t.clone(), n) for t in x)
    ye = tuple(inst.ctx[4].ntt_(t.clone(), n) for t in y)
    gb, ga = poly.mul_eval(inst.key(4), xe, ye, alpha, c if with_c else None)
    wb, wa = inst.key(4).mul(x[0][:, :4].contiguous(), x[1][:, :4].contiguous(), y[0], y[1])
    if alpha == 2 or with_c:
        cts = [(wb, wa)] + ([c] if with_c else [])
        wb, wa = poly.lincomb(inst.ctx[3], cts, n, False, [alpha, -1][:len(cts)], 0.0, inst.scale)
    assert gb.shape == (2, 3, n)
    assert torch_cuda.equal(gb, wb) and torch_cuda.equal(ga, wa)
    if log_n == 4 and alpha == 2 and with_c:   # .. and the big-integer model, once
        qs, ps = inst.qs[:4], inst.ps
        kb, ka = (host(k) for k in inst.cut_key(4))
        for b in range(2):
            mb, ma = PM.mul_eval(qs, ps, limbs_of(kb[None], 0), limbs_of(ka[None], 0), (limbs_of(host(x[0]), b), limbs_of(host(x[1]), b)),
                                 (limbs_of(host(y[0]), b), limbs_of(host(y[1]), b)), alpha, (limbs_of(host(c[0]), b), limbs_of(host(c[1]), b)))
            assert np.array_equal(host(gb)[b], np.array(mb, dtype=np.uint64)) and np.array_equal(host(ga)[b], np.array(ma, dtype=np.uint64))


# ---- 3. fhe_ckks_poly_apply against the op-by-op composition ---------------------------------------------------------------------------
def series(degree, seed=3):
    return np.random.Generator(np.random.PCG64(seed + degree)).uniform(-1, 1, degree + 1)


@pytest.mark.parametrize("degree", [1, 7, 8, 31])
@pytest.mark.parametrize("log_n", [4, 12])
def test_apply_equals_the_composition(fhe, poly, torch_cuda, log_n, degree):
    """batch 2, more levels handed over than the plan needs; every register of the composition is a fresh fhe_ckks_mul (which transforms
    its four operands again) or fhe_ckks_lincomb call"""
    plan = fhe.CkksPolyPlan(series(degree), 0)
    top = plan.depth + 2
    inst = instance(fhe, torch_cuda, log_n, 9)
    assert top <= inst.L
    cb, ca = inst.random_ct(2, top, 40 + degree)
    gb, ga = inst.evaluator(plan, top, extra_levels=1).apply(cb, ca)
    wb, wa = poly.replay_composed(plan.ops, lambda lv: inst.ctx[lv], inst.key, cb, ca, inst.n, inst.scale)
    assert gb.shape == (2, top - plan.depth, inst.n)
    assert torch_cuda.equal(gb, wb) and torch_cuda.equal(ga, wa)
    if degree == 7 and log_n == 4:   # host memory: the same bits
        ev = fhe.CkksPolyEval(plan, [inst.ctx[x] for x in range(top, top - plan.depth - 1, -1)], inst.scale, *(host(k) for k in inst.cut_key(top)), inst.n)
        hb, ha = ev.apply(host(cb), host(ca))
        assert isinstance(hb, np.ndarray) and np.array_equal(hb, host(gb)) and np.array_equal(ha, host(ga))


def test_apply_monomial_basis_and_eval_mod_ops(fhe, poly, torch_cuda):
    inst = instance(fhe, torch_cuda, 4, 12)
    for plan in (fhe.CkksPolyPlan(series(8), 1), fhe.eval_mod_plan(4, 2, 31)):
        top = plan.depth + 1
        cb, ca = inst.random_ct(2, top, 77)
        gb, ga = inst.evaluator(plan, top).apply(cb, ca)
        wb, wa = poly.replay_composed(plan.ops, lambda lv: inst.ctx[lv], inst.key, cb, ca, inst.n, inst.scale)
        assert torch_cuda.equal(gb, wb) and torch_cuda.equal(ga, wa)


def test_prepare_refusals(fhe, poly, torch_cuda):
    inst = instance(fhe, torch_cuda, 4, 9)
    plan = fhe.CkksPolyPlan(series(7), 0)
    top = plan.depth + 1
    chain = [inst.ctx[x] for x in range(top, 0, -1)]
    kb, ka = inst.cut_key(top)
    fhe.CkksPolyEval(plan, chain, inst.scale, kb, ka, inst.n)
    for bad in (chain[:-1], [chain[0]] + chain[2:] + [chain[-1]], [inst.ctx[top - 1]] + chain[1:]):
        with pytest.raises(fhe.FheError):
            fhe.CkksPolyEval(plan, bad, inst.scale, kb, ka, inst.n)
    with pytest.raises(fhe.FheError):
        fhe.CkksPolyEval(plan, chain, 0, kb, ka, inst.n)
    with pytest.raises(fhe.FheError):   # a constant out of range for this scale
        fhe.CkksPolyEval(fhe.CkksPolyPlan([0.0, 2.0 ** 80], 0), chain, inst.scale, kb, ka, inst.n)
    from learn_fhe_amd import _lib
    assert _lib.lib().fhe_ckks_poly_apply(None, None, None, None, None, 1, _lib.MEM_DEVICE, None) == INVALID


# ---- 4. decode level --------------------------------------------------------------------------------------------------------------------
def real_slots(inst, batch, seed, lo=-1.0, hi=1.0):
    return np.random.Generator(np.random.PCG64(seed)).uniform(lo, hi, (batch, inst.l)).astype(np.complex128)


def horner(inst, mono, m, top):
    """Horner with the entries the library had before: fhe_ckks_mul_plain on an encoded constant, fhe_rns_add of an encoded constant
    (to the b half), fhe_ckks_mul with the input on contiguous prefix slices.  Depth = the degree."""
    n = inst.n
    xb, xa = inst.encrypt(m, top)
    d = len(mono) - 1
    lv = top
    ab, aa = inst.ctx[lv].mul_plain(inst.constant(mono[d], lv), xb, xa, n)
    lv -= 1
    for j in range(d - 1, -1, -1):
        pt = inst.constant(mono[j], lv).expand(m.shape[0], lv, n).contiguous()
        inst.ctx[lv].add_(ab, pt, n)
        if j == 0:
            break
        ab, aa = inst.key(lv).mul(ab, aa, xb[:, :lv].contiguous(), xa[:, :lv].contiguous())
        lv -= 1
    return inst.decode(lv, ab, aa)


@pytest.mark.parametrize("degree", [3, 7])
def test_decode_small_degrees_against_horner(fhe, poly, torch_cuda, degree):
    """n = 32, L = depth + 2 for the new path; the same slots through Horner (which needs degree + 1 limbs) give the yardstick: the new
    path may be 8 times worse, since the two schedules multiply noise at different places.
    Measured (MI355X): degree 3 new 2^-38.92 / Horner 2^-38.84; degree 7 new 2^-38.34 / Horner 2^-37.74."""
    c = series(degree, 11)
    plan = fhe.CkksPolyPlan(c, 0)
    inst = instance(fhe, torch_cuda, 5, 12)
    m = real_slots(inst, 2, 60 + degree)
    want = np.polynomial.chebyshev.chebval(m.real, c)
    e_h = float(np.max(np.abs(horner(inst, np.polynomial.chebyshev.cheb2poly(c), m, degree + 2) - want)))
    top = plan.depth + 2
    gb, ga = inst.evaluator(plan, top).apply(*inst.encrypt(m, top))
    e_n = float(np.max(np.abs(inst.decode(top - plan.depth, gb, ga) - want)))
    print("degree %d: decode error new path 2^%.2f, Horner on the old entries 2^%.2f" % (degree, np.log2(e_n), np.log2(e_h)))
    assert e_n <= 8 * e_h


def test_decode_degree_31(fhe, poly, torch_cuda):
    """bound 2^-30 max(1, sum |c_j|): the reference's own precision for its deepest CKKS circuit (bootstrapping.rs:137) times the series'
    gain.  Measured (MI355X): 2^-35.47 against the bound 2^-25.89."""
    c = series(31, 11)
    plan = fhe.CkksPolyPlan(c, 0)
    inst = instance(fhe, torch_cuda, 5, 12)
    top = plan.depth + 2
    m = real_slots(inst, 2, 91)
    gb, ga = inst.evaluator(plan, top).apply(*inst.encrypt(m, top))
    e = float(np.max(np.abs(inst.decode(top - plan.depth, gb, ga) - np.polynomial.chebyshev.chebval(m.real, c))))
    bound = 2.0 ** -30 * max(1.0, float(np.sum(np.abs(c))))
    print("degree 31: decode error 2^%.2f, bound 2^%.2f" % (np.log2(e), np.log2(bound)))
    assert e <= bound


def test_eval_mod_decode(fhe, poly, torch_cuda):
    """n = 32, K = 4, r = 2, degree 31: t = eps + I -> about eps.  Against the f64 evaluation of the same ops the bound is the degree-31
    bound times 4^r (a doubling 2 y^2 - 1, |y| <= 1, at most quadruples an error); that f64 evaluation is within 1e-6 of eps.
    Measured (MI355X): 2^-38.75 against the bound 2^-24.62."""
    K, r, degree = 4, 2, 31
    ops, c = poly.eval_mod_ops(K, r, degree)
    plan = fhe.CkksPolyPlan.from_ops(ops)
    inst = instance(fhe, torch_cuda, 5, 12)
    top = plan.depth + 2
    assert top <= inst.L
    rng = np.random.Generator(np.random.PCG64(17))
    eps = rng.uniform(-2.0 ** -10, 2.0 ** -10, (2, inst.l))
    t = eps + rng.integers(-K, K + 1, (2, inst.l))
    f64 = poly.replay_f64(ops, t)
    assert float(np.max(np.abs(f64 - eps))) < 1e-6
    gb, ga = inst.evaluator(plan, top).apply(*inst.encrypt(t.astype(np.complex128), top))
    e = float(np.max(np.abs(inst.decode(top - plan.depth, gb, ga) - f64)))
    bound = 2.0 ** -30 * max(1.0, float(np.sum(np.abs(c)))) * 4 ** r
    print("eval_mod: decode error against the f64 evaluation 2^%.2f, bound 2^%.2f" % (np.log2(e), np.log2(bound)))
    assert e <= bound


# ---- 5. the C demo ----------------------------------------------------------------------------------------------------------------------
def test_c_demo(fhe, tmp_path):
    """examples/ckks_poly_demo.c: a degree-7 Chebyshev series on encrypted slots from plain C, decode checked"""
    from conftest import ROOT
    lib_dir = os.path.dirname(fhe.lib_path())
    exe = tmp_path / "ckks_poly_demo"
    cmd = ["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "ckks_poly_demo.c"), "-o", str(exe),
           "-L", lib_dir, "-lfhe_ring", "-lm", "-Wl,--allow-shlib-undefined", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ckks_poly_demo ok" in r.stdout, r.stdout + r.stderr
