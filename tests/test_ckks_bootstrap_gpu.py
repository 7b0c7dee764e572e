"""The CKKS bootstrap on the device (include/fhe_ring.h fhe_ckks_cjk_gen, fhe_ckks_mod_raise, fhe_ckks_conj_split / _join,
fhe_ckks_bootstrap_*): the three glue kernels bit-exact against the big-integer model of tests/ckks_bootstrap_model.py, the one call
bit-exact against the seven public calls chained by hand, and at decode level against the float64 replay of the eval_mod plan on the
exact decryption of the raised ciphertext.

Measured on the MI355X: every decode-level test prints its figures before it asserts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ckks_bootstrap_model as BM  # noqa: E402
import ckks_encode_model as Mo  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID = 1
K_MOD, R_MOD, DEGREE = 8, 3, 31


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def boot(fhe):
    return fhe.ckks_bootstrap


def dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.complex128 else a.view(np.int64)).cuda()


def host(t):
    a = t.cpu().numpy()
    return a if a.dtype == np.complex128 else a.view(np.uint64)


def unaligned(torch, a):
    """the same values at an address that is 8 but not 16 bytes aligned: the kernels' one-coefficient route"""
    flat = torch.empty(a.size + 1, dtype=torch.int64, device="cuda")
    view = flat[1:]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1)))
    assert view.data_ptr() % 16 == 8
    return view.view(*a.shape)


def bases(cref, kind, log_n, ell):
    from oracle import pyref as P
    if kind == "ckks55":
        qs, ps = P.ckks_primes(log_n, 55, ell)
        return qs, ps[:1]
    first, rest = {"q60_over_30": (60, 30), "q30_over_60": (30, 60)}[kind]
    lo = cref.two_adic_primes(rest, log_n + 1, ell)
    return cref.two_adic_primes(first, log_n + 1, 1) + lo[:ell - 1], lo[ell - 1:]


# ---- 1. mod_raise ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ckks55", "q60_over_30", "q30_over_60"])
@pytest.mark.parametrize("in_limbs", [1, 3])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [2, 32, 4096])
def test_mod_raise_equals_the_model(fhe, boot, torch_cuda, cref, n, batch, in_limbs, kind):
    """random residues of q0 with 0, 1, (q0 - 1) / 2, (q0 + 1) / 2 and q0 - 1 planted, on a 55-bit chain, a 60-bit q0 over 30-bit limbs
    (|v| exceeds the limb many times over) and a 30-bit q0 over 60-bit limbs; limbs above 0 of the input hold words nobody may read;
    device memory (16-byte aligned and not) and host memory give the bits of the model"""
    log_n = n.bit_length() - 1
    qs, ps = bases(cref, kind, max(log_n, 1), 4)
    q0 = qs[0]
    rns = fhe.RnsContext(qs, ps)
    rng = np.random.Generator(np.random.PCG64(1000 * n + 10 * batch + in_limbs))
    planted = [0, 1, (q0 - 1) // 2, (q0 + 1) // 2, q0 - 1]
    halves = []
    for h in range(2):
        a = rng.integers(0, 1 << 62, (batch, in_limbs, n), dtype=np.uint64)
        a[:, 0] %= np.uint64(q0)
        flat = a[:, 0].reshape(-1)
        pos = rng.permutation(flat.size)[:len(planted)]
        for p, v in zip(pos, planted[h:] + planted[:h]):
            flat[p] = v
        a[:, 0] = flat.reshape(batch, n)
        halves.append(a)
    want = [np.array([BM.mod_raise([int(v) for v in a[b, 0]], q0, qs) for b in range(batch)], dtype=np.uint64) for a in halves]
    gb, ga = boot.mod_raise(rns, dev(torch_cuda, halves[0]), dev(torch_cuda, halves[1]), n)
    assert gb.shape == (batch, len(qs), n)
    assert np.array_equal(host(gb), want[0]) and np.array_equal(host(ga), want[1])
    hb, ha = boot.mod_raise(rns, halves[0], halves[1], n)
    assert isinstance(hb, np.ndarray) and np.array_equal(hb, want[0]) and np.array_equal(ha, want[1])
    ub, ua = boot.mod_raise(rns, unaligned(torch_cuda, halves[0]), unaligned(torch_cuda, halves[1]), n)
    assert np.array_equal(host(ub), want[0]) and np.array_equal(host(ua), want[1])


# ---- 2. split / join ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", [1, 4])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [2, 32, 4096])
def test_split_and_join_equal_the_model(fhe, boot, torch_cuda, cref, n, batch, ell):
    """the stacked layout, the shift by n/2 and its signs against the model limb by limb; join(split(x, cx)) = 2 x bit for bit; host
    memory and unaligned device memory give the same bits"""
    log_n = n.bit_length() - 1
    qs, ps = bases(cref, "ckks55", max(log_n, 1), ell)
    rns = fhe.RnsContext(qs, ps)
    rng = np.random.Generator(np.random.PCG64(77 * n + batch + ell))
    mod = np.array(qs, dtype=np.uint64)[None, :, None]
    x = [rng.integers(0, 1 << 62, (batch, ell, n), dtype=np.uint64) % mod for _ in range(4)]   # ct_b, ct_a, cj_b, cj_a
    x[0][0, 0, :2] = (0, qs[0] - 1)
    x[2][0, 0, :2] = (qs[0] - 1, 0)
    d = [dev(torch_cuda, a) for a in x]
    sb, sa = boot.conj_split(rns, d[0], d[1], d[2], d[3], n)
    assert sb.shape == (2 * batch, ell, n)
    for got, ct, cj in ((host(sb), x[0], x[2]), (host(sa), x[1], x[3])):
        for b in range(batch):
            for l, q in enumerate(qs):
                r, j = BM.split([int(v) for v in ct[b, l]], [int(v) for v in cj[b, l]], q)
                assert np.array_equal(got[b, l], np.array(r, dtype=np.uint64)), "R, ciphertext %d limb %d" % (b, l)
                assert np.array_equal(got[batch + b, l], np.array(j, dtype=np.uint64)), "J, ciphertext %d limb %d" % (b, l)
    jb, ja = boot.conj_join(rns, sb, sa, n)
    assert jb.shape == (batch, ell, n)
    for got, ct, st in ((host(jb), x[0], host(sb)), (host(ja), x[1], host(sa))):
        assert np.array_equal(got, (2 * (ct.astype(object))) % mod.astype(object))
        for b in range(batch):
            for l, q in enumerate(qs):
                want = BM.join([int(v) for v in st[b, l]], [int(v) for v in st[batch + b, l]], q)
                assert np.array_equal(got[b, l], np.array(want, dtype=np.uint64))
    hb, ha = boot.conj_split(rns, x[0], x[1], x[2], x[3], n)
    assert isinstance(hb, np.ndarray) and np.array_equal(hb, host(sb)) and np.array_equal(ha, host(sa))
    kb, ka = boot.conj_join(rns, hb, ha, n)
    assert np.array_equal(kb, host(jb)) and np.array_equal(ka, host(ja))
    u = [unaligned(torch_cuda, a) for a in x]
    ub, ua = boot.conj_split(rns, u[0], u[1], u[2], u[3], n)
    assert torch_cuda.equal(ub, sb) and torch_cuda.equal(ua, sa)
    vb, va = boot.conj_join(rns, unaligned(torch_cuda, host(sb)), unaligned(torch_cuda, host(sa)), n)
    assert torch_cuda.equal(vb, jb) and torch_cuda.equal(va, ja)


# ---- a small scheme instance: every stage of a bootstrap prepared once ------------------------------------------------------------------
def sparse_secret(n, weight, seed):
    """a ternary secret of Hamming weight exactly `weight` as two's-complement i64"""
    rng = np.random.Generator(np.random.PCG64(seed))
    s = np.zeros(n, dtype=np.int64)
    s[rng.permutation(n)[:weight]] = rng.choice(np.array([-1, 1]), weight)
    assert int(np.count_nonzero(s)) == weight
    return s


def cut(key, lv, full):
    import torch
    return key if lv == full else torch.cat([key[:lv], key[full:]]).contiguous()


class Instance:
    def __init__(self, fhe, torch, log_n, seed=1200):
        from oracle import pyref as P
        boot = fhe.ckks_bootstrap
        self.fhe, self.torch, self.seed = fhe, torch, seed
        self.n, self.l = 1 << log_n, 1 << (log_n - 1)
        self.enc = fhe.CkksEncoder(self.n)
        self.p_c2s, self.p_s2c = fhe.CkksLinearPlan(self.enc, 2, True), fhe.CkksLinearPlan(self.enc, 2, False)
        d_mod = fhe.eval_mod_plan(K_MOD, R_MOD, DEGREE).depth
        self.depth = self.p_c2s.depth + d_mod + self.p_s2c.depth
        self.L = L = self.depth + 2
        self.qs, self.ps = P.ckks_primes(log_n, 55, L)
        self.scale, self.q0 = self.qs[-1], self.qs[0]
        self.ctx = {lv: fhe.RnsContext(self.qs[:lv], self.ps) for lv in range(1, L + 1)}
        self.s = sparse_secret(self.n, min(12, self.n // 2), seed)
        self.sk = dev(torch, self.s.view(np.uint64))
        top = self.ctx[L]
        self.L1, self.L2 = L - self.p_c2s.depth, L - self.p_c2s.depth - d_mod
        self.rot = {j: fhe.rtk_gen(top, self.sk, self.n, j, seed + 1, j) for j in sorted(set(self.p_c2s.rotations) | set(self.p_s2c.rotations))}
        self.rlk = top.ksk_gen(self.sk, None, self.n, seed + 2, 0)
        self.cjk = boot.cjk_gen(top, self.sk, self.n, seed + 3, 0)
        self.plan = boot.bootstrap_eval_mod_plan(K_MOD, R_MOD, DEGREE, self.q0, self.scale)
        assert self.plan.depth == d_mod
        self.c2s = self.transform(self.p_c2s, L)
        self.evaluator = self.make_evaluator(self.L1)
        self.s2c = self.transform(self.p_s2c, self.L2)
        self.levels = [self.ctx[lv] for lv in range(L, L - self.depth - 1, -1)]
        self.bs = fhe.CkksBootstrapper(self.levels, self.c2s, self.evaluator, self.s2c, self.cjk[0], self.cjk[1], self.n)
        self.cj_key = fhe.CkksKey(self.ctx[self.L1], cut(self.cjk[0], self.L1, L), cut(self.cjk[1], self.L1, L), self.n)

    def transform(self, plan, top, ctx=None):
        ctx = self.ctx if ctx is None else ctx
        keys = {j: (cut(self.rot[j][0], top, self.L), cut(self.rot[j][1], top, self.L)) for j in plan.rotations}
        return self.fhe.CkksLinearTransform(plan, [ctx[lv] for lv in range(top, top - plan.depth - 1, -1)], self.scale, keys)

    def make_evaluator(self, top):
        lv = [self.ctx[x] for x in range(top, top - self.plan.depth - 1, -1)]
        return self.fhe.CkksPolyEval(self.plan, lv, self.scale, cut(self.rlk[0], top, self.L), cut(self.rlk[1], top, self.L), self.n)

    def encrypt(self, m, lv):
        ctx = self.ctx[lv]
        pk_b, pk_a = ctx.sk_encrypt(self.sk, None, self.n, 1, self.seed + 4, 0)
        pt = self.enc.encode(ctx, self.scale, dev(self.torch, np.ascontiguousarray(m, dtype=np.complex128)))
        return ctx.pk_encrypt(pk_b[0].contiguous(), pk_a[0].contiguous(), pt, self.n, m.shape[0], self.seed + 5, 0)

    def decode(self, lv, cb, ca):
        return host(self.enc.decode(self.ctx[lv], self.scale, self.ctx[lv].decrypt(self.sk, cb, ca, self.n)))


_INSTANCES = {}


def instance(fhe, torch, log_n):
    if log_n not in _INSTANCES:
        _INSTANCES[log_n] = Instance(fhe, torch, log_n)
    return _INSTANCES[log_n]


# ---- 3. cjk_gen -----------------------------------------------------------------------------------------------------------------------
def test_cjk_gen_conjugates(fhe, boot, torch_cuda):
    """scheme/ckks/src/ckks.rs `conjugate` test: fhe_ckks_rotate(t = -1) with the key of fhe_ckks_cjk_gen decodes to the conjugate slots
    within the reference's 2^-40, n = 32; host and device memory make the same key.  Measured (MI355X): 2^-47.31."""
    inst = instance(fhe, torch_cuda, 5)
    lv = 3
    ctx = inst.ctx[lv]
    kb, ka = boot.cjk_gen(ctx, inst.sk, inst.n, 31, 0)
    xb, xa = boot.cjk_gen(ctx, host(inst.sk), inst.n, 31, 0)
    assert np.array_equal(xb, host(kb)) and np.array_equal(xa, host(ka))
    rng = np.random.Generator(np.random.PCG64(8))
    m = rng.uniform(0, 1, (2, inst.l)) + 1j * rng.uniform(0, 1, (2, inst.l))
    cb, ca = inst.encrypt(m, lv)
    fhe.CkksKey(ctx, kb, ka, inst.n).rotate_(-1, cb, ca)
    e = float(np.max(np.abs(inst.decode(lv, cb, ca) - np.conj(m))))
    print("conjugate with the device-made key: decode error 2^%.2f (bound 2^-40)" % np.log2(e))
    assert e < 2.0 ** -40


# ---- 4. the one call against the seven ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("log_n", [3, 5])
def test_apply_equals_the_composition(fhe, boot, torch_cuda, log_n, batch):
    """55-bit chain, L = depth + 2, linear plans with r = 2, K = 8, r = 3, degree 31; the input has two limbs of which only limb 0 is
    reduced (and read).  Batch 3: the stacked batch 2 * batch is neither even in the halves' sizes nor a power of two."""
    inst = instance(fhe, torch_cuda, log_n)
    n = inst.n
    rng = np.random.Generator(np.random.PCG64(50 + log_n + batch))
    ct = [rng.integers(0, 1 << 62, (batch, 2, n), dtype=np.uint64) for _ in range(2)]
    for a in ct:
        a[:, 0] %= np.uint64(inst.q0)
    cb, ca = dev(torch_cuda, ct[0]), dev(torch_cuda, ct[1])
    gb, ga = inst.bs.apply(cb, ca)
    wb, wa = boot.replay_composed(inst.ctx[inst.L], inst.c2s, inst.cj_key, inst.evaluator, inst.s2c, cb, ca, n)
    assert inst.bs.depth == inst.depth and inst.bs.out_limbs == 2
    assert gb.shape == (batch, 2, n)
    assert torch_cuda.equal(gb, wb) and torch_cuda.equal(ga, wa)
    if log_n == 3 and batch == 3:   # host memory: the same bits
        hb, ha = inst.bs.apply(ct[0], ct[1])
        assert isinstance(hb, np.ndarray) and np.array_equal(hb, host(gb)) and np.array_equal(ha, host(ga))


# ---- 5. decode level ------------------------------------------------------------------------------------------------------------------
def test_bootstrap_decodes(fhe, boot, torch_cuda):
    """n = 32, L = 17, batch 2, a ternary secret of Hamming weight exactly 12: t = b + a s of the raised ciphertext has |t| <= 6.5 q0, so
    |eps + I| < K = 8 by construction (asserted from the exact host decryption all the same).  Slots with |Re|, |Im| <= 2^-11 are
    encrypted on all 17 limbs and read on limb 0.  The model is z'_j = post sin(2 pi t_j / q0) / (2 pi) by replay_f64 of the plan's ops
    and m' = sfft(z').  Bounds, composed from bounds the project already holds:
        max |decoded - m'| <= l (E_mod + K 2^-30) + 2^-30,   E_mod = 2^-30 max(1, sum |c_j|) 4^r   (test_eval_mod_decode's),
    K 2^-30 the reference's coeff_to_slot_to_coeff tolerance at slot magnitude K, l the infinity norm of sfft; and separately
        max |m' - m| <= l (2 pi)^2 2^-30 / 6 + 1e-9,   the cubic term of the sine at |eps| <= 2^-10.
    Measured (MI355X): max |eps + I| 3.0; decoded against the model 2^-34.33 (bound 2^-18.65); model against the message 6.1e-11 (bound
    9.9e-8); decoded against the message 2^-33.72."""
    inst = instance(fhe, torch_cuda, 5)
    n, l, L, q0, scale = inst.n, inst.l, inst.L, inst.q0, inst.scale
    assert (n, L) == (32, 17)
    rng = np.random.Generator(np.random.PCG64(23))
    m = rng.uniform(-2.0 ** -11, 2.0 ** -11, (2, l)) + 1j * rng.uniform(-2.0 ** -11, 2.0 ** -11, (2, l))
    cb, ca = inst.encrypt(m, L)
    # the exact t of the raised ciphertext, from limb 0 alone and from the device's own decryption of what mod_raise made
    rb, ra = boot.mod_raise(inst.ctx[L], cb, ca, n)
    dec = host(inst.ctx[L].decrypt(inst.sk, rb, ra, n))
    s = [int(v) for v in inst.s]
    z_new = np.zeros((2, l), dtype=np.complex128)
    ops = inst.plan.ops
    worst_t = 0.0
    for b in range(2):
        b0 = [BM.centred(int(v), q0) for v in host(cb)[b, 0]]
        a0 = [BM.centred(int(v), q0) for v in host(ca)[b, 0]]
        t = [x + y for x, y in zip(b0, BM.negacyclic_int(a0, s))]
        for lv, q in enumerate(inst.qs):
            assert [v % q for v in t] == [int(v) for v in dec[b, lv]], "limb %d of the raised ciphertext" % lv
        worst_t = max(worst_t, max(abs(v) for v in t) / q0)
        x = np.array([2.0 * v / scale for v in t])
        y = fhe.ckks_poly.replay_f64(ops, x)
        z_new[b] = y[:l] + 1j * y[l:]
    assert worst_t < K_MOD, "|eps + I| = %.3f" % worst_t
    want = np.array([[complex(v) for v in Mo.sfft([Mo.mpc(complex(z)) for z in row])] for row in z_new])
    gb, ga = inst.bs.apply(cb, ca)
    assert gb.shape == (2, L - inst.depth, n)
    got = inst.decode(L - inst.depth, gb, ga)
    _, coeffs = fhe.ckks_poly.eval_mod_ops(K_MOD, R_MOD, DEGREE)
    e_mod = 2.0 ** -30 * max(1.0, float(np.sum(np.abs(coeffs)))) * 4 ** R_MOD
    bound = l * (e_mod + K_MOD * 2.0 ** -30) + 2.0 ** -30
    e = float(np.max(np.abs(got - want)))
    e_sine = float(np.max(np.abs(want - m)))
    bound_sine = l * (2 * np.pi) ** 2 * 2.0 ** -30 / 6 + 1e-9
    print("bootstrap n=32 L=17: max |eps + I| %.3f; decode error against the model 2^%.2f (bound 2^%.2f); model against the message %.3g (bound %.3g); "
          "decoded against the message 2^%.2f" % (worst_t, np.log2(e), np.log2(bound), e_sine, bound_sine, np.log2(float(np.max(np.abs(got - m))))))
    inst.enc.status(cb)
    assert e <= bound
    assert e_sine <= bound_sine


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_prepare_and_apply_refusals(fhe, boot, torch_cuda):
    from learn_fhe_amd import _lib
    lib = _lib.lib()
    inst = instance(fhe, torch_cuda, 3)
    n = inst.n
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def prepare(levels, c2s, evaluator, s2c, kb=inst.cjk[0], ka=inst.cjk[1]):
        h = C.c_void_p()
        lv = (C.c_void_p * len(levels))(*[c.handle for c in levels])
        rc = lib.fhe_ckks_bootstrap_prepare(lv, len(levels), n, c2s._h, evaluator._h, s2c._h, vp(kb) if kb is not None else None,
                                            vp(ka) if ka is not None else None, _lib.MEM_DEVICE, C.byref(h))
        assert (rc == 0) == bool(h.value)
        if h.value:
            lib.fhe_ckks_bootstrap_destroy(h)
        return rc

    assert prepare(inst.levels, inst.c2s, inst.evaluator, inst.s2c) == 0                               # the good call
    assert prepare(inst.levels[:-1], inst.c2s, inst.evaluator, inst.s2c) == INVALID                    # levels shortened by one
    off = inst.make_evaluator(inst.L1 - 1)
    assert prepare(inst.levels, inst.c2s, off, inst.s2c) == INVALID                                    # eval prepared one level off
    other = {lv: fhe.RnsContext(inst.qs[:lv], inst.ps) for lv in range(1, inst.L2 + 1)}
    assert prepare(inst.levels, inst.c2s, inst.evaluator, inst.transform(inst.p_s2c, inst.L2, other)) == INVALID   # s2c from another chain
    assert prepare(inst.levels, inst.c2s, inst.evaluator, inst.s2c, kb=None) == INVALID                # a NULL key
    assert prepare(inst.levels, inst.c2s, inst.evaluator, inst.s2c, ka=None) == INVALID
    assert prepare(inst.levels, inst.s2c, inst.evaluator, inst.c2s) == INVALID                         # the transforms swapped
    ct = dev(torch_cuda, np.zeros((1, 1, n), dtype=np.uint64))
    out = dev(torch_cuda, np.zeros((1, 2, n), dtype=np.uint64))
    D = _lib.MEM_DEVICE
    assert lib.fhe_ckks_bootstrap_apply(None, vp(ct), vp(ct), 1, vp(out), vp(out), 1, D, None) == INVALID
    assert lib.fhe_ckks_bootstrap_apply(inst.bs._h, None, vp(ct), 1, vp(out), vp(out), 1, D, None) == INVALID
    assert lib.fhe_ckks_bootstrap_apply(inst.bs._h, vp(ct), vp(ct), 0, vp(out), vp(out), 1, D, None) == INVALID
    assert lib.fhe_ckks_bootstrap_apply(inst.bs._h, None, None, 1, None, None, 0, D, None) == 0        # batch == 0
    assert lib.fhe_ckks_mod_raise(inst.ctx[2].handle, None, None, 1, None, None, n, 0, D, None) == 0
    assert lib.fhe_ckks_conj_split(inst.ctx[2].handle, None, None, None, None, None, None, n, 0, D, None) == 0
    assert lib.fhe_ckks_conj_join(inst.ctx[2].handle, None, None, None, None, n, 0, D, None) == 0


# ---- 7. the C demo --------------------------------------------------------------------------------------------------------------------
def test_c_demo(fhe, tmp_path):
    """examples/ckks_bootstrap_demo.c: the whole path from plain C at n = 32, decode checked"""
    from conftest import ROOT
    lib_dir = os.path.dirname(fhe.lib_path())
    exe = tmp_path / "ckks_bootstrap_demo"
    cmd = ["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "ckks_bootstrap_demo.c"), "-o", str(exe),
           "-L", lib_dir, "-lfhe_ring", "-lm", "-Wl,--allow-shlib-undefined", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ckks_bootstrap_demo ok" in r.stdout, r.stdout + r.stderr
