"""CKKS slot_to_coeff / coeff_to_slot made and applied on the device (include/fhe_ring.h fhe_ckks_linear_*, fhe_ckks_rtk_gen):
scheme/ckks/src/bootstrapping.rs:23-31, 56-88 over sfft.rs:75-99 and util/src/misc/matrix.rs, against the exact model of
tests/ckks_linear_model.py, against the hand-made chain of fhe_ckks_mul_mat, and end to end as the reference's own
`coeff_to_slot_to_coeff` (bootstrapping.rs:121-141)."""
import ctypes as C
import os
import sys
from math import log2

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ckks_encode_model as Mo  # noqa: E402
import ckks_linear_model as LM  # noqa: E402
import keygen_checks as K  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID = 1
DG_MAX = 19  # dg(3.2, 6): floor(6 * 3.2)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.complex128 else a.view(np.int64)).cuda()


def host(t):
    a = t.cpu().numpy()
    return a if a.dtype == np.complex128 else a.view(np.uint64)


def cut(key, lv, full):
    """a key [full + K][n] over qs[:full] ++ ps -> the same rows over qs[:lv] ++ ps"""
    if lv == full:
        return key
    if isinstance(key, np.ndarray):
        return np.ascontiguousarray(np.concatenate([key[:lv], key[full:]]))
    import torch
    return torch.cat([key[:lv], key[full:]]).contiguous()


def err_bits(x):
    return float(Mo.M.log(x, 2)) if x > 0 else float("-inf")


# ---- 4. the matrices against the model ----------------------------------------------------------------------------------------------
VALUE_CASES = [(l, r) for l in (2, 4, 16, 32) for r in sorted({1, 3, l.bit_length() - 1})] + [(512, 3)]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("l,r", VALUE_CASES)
def test_matrix_values_against_the_model(fhe, torch_cuda, l, r, inverse):
    """every read-back entry within 2^-93 of the 300-bit model, per component: a chunk entry is a sum of at most 3^(r-1) products of
    r table values (each within 2^-100, modulus <= 1) plus dd rounding near 2^-104 per operation, so 3^(r-1) r 2^-100 < 2^-93 for
    r <= 4; for the dense r = log2 l > 4 every entry is a sum of at most l products of log2 l values: l log2 l 2^-100.  l = 32 with
    r = 5 forward is the Vandermonde matrix of sfft.rs:125-134, checked here against its definition as well."""
    log_l = l.bit_length() - 1
    bound = Mo.mpf(2) ** -93 if min(r, log_l) <= 4 else Mo.mpf(l * log_l) * Mo.mpf(2) ** -100
    enc = fhe.CkksEncoder(2 * l)
    plan = fhe.CkksLinearPlan(enc, r, inverse)
    mats = LM.chunked(l, r, inverse)
    assert plan.depth == len(mats)
    worst = Mo.mpf(0)
    for k, m in enumerate(mats):
        m = LM.normalised(m, l)
        idx, _, _ = plan.matrix(k)
        assert idx == sorted(m)
        got = plan.diags(k)
        for s, d in enumerate(idx):
            for c in range(l):
                g, w = LM.from_dd4(got[s, c]), m[d][c]
                worst = max(worst, abs(g.real - w.real), abs(g.imag - w.imag))
    print("linear plan l=%d r=%d inverse=%d: worst matrix entry error 2^%.1f (bound 2^%.1f)" % (l, r, inverse, err_bits(worst), err_bits(bound)))
    assert worst < bound
    if l == 32 and r == 5 and not inverse:
        got, (idx, _, _) = plan.diags(0), plan.matrix(0)
        for i, t in enumerate(Mo.w(l)):
            row = Mo.bit_reverse([t ** e for e in range(l)])
            for j in range(l):
                g = LM.from_dd4(got[idx.index((j - i) % l), i])
                assert max(abs(g.real - row[j].real), abs(g.imag - row[j].imag)) < bound


# ---- a small scheme instance shared by the tests below --------------------------------------------------------------------------
class Instance:
    def __init__(self, fhe, torch, log_n, big_l, log_qi=55, seed=700):
        from oracle import pyref as P
        self.fhe, self.torch, self.seed = fhe, torch, seed
        self.n, self.l, self.L = 1 << log_n, 1 << (log_n - 1), big_l
        self.qs, self.ps = P.ckks_primes(log_n, log_qi, big_l)
        self.scale = self.qs[-1]
        self.enc = fhe.CkksEncoder(self.n)
        self.ctx = {lv: fhe.RnsContext(self.qs[:lv], self.ps) for lv in range(1, big_l + 1)}
        like = dev(torch, np.zeros(1, dtype=np.uint64))
        self.sk = fhe.sample_zo(0.5, seed, 0, like, self.n)
        self.keys = {}

    def rot_keys(self, indices):
        """ckks.rs:174-184: one key per rotation index over the full chain"""
        for j in indices:
            if j not in self.keys:
                self.keys[j] = self.fhe.rtk_gen(self.ctx[self.L], self.sk, self.n, j, self.seed + 1, j)
        return {j: self.keys[j] for j in indices}

    def encrypt(self, m):
        top = self.ctx[self.L]
        pk_b, pk_a = top.sk_encrypt(self.sk, None, self.n, 1, self.seed + 2, 0)
        pt = self.enc.encode(top, self.scale, dev(self.torch, m))
        return top.pk_encrypt(pk_b[0].contiguous(), pk_a[0].contiguous(), pt, self.n, m.shape[0], self.seed + 3, 0)

    def decode(self, lv, cb, ca):
        return host(self.enc.decode(self.ctx[lv], self.scale, self.ctx[lv].decrypt(self.sk, cb, ca, self.n)))

    def slots(self, batch, seed):
        rng = np.random.Generator(np.random.PCG64(seed))
        return rng.uniform(0, 1, (batch, self.l)) + 1j * rng.uniform(0, 1, (batch, self.l))

    def hand_chain(self, plan, top, cb, ca):
        """bootstrapping.rs:81-108 composed by hand: per matrix the read-back diagonals rotated in numpy (`diag_rot`), encoded by
        fhe_ckks_encode, one CkksDiagMatrix with keys cut to its two levels, applied last to first"""
        fhe, torch = self.fhe, self.torch
        lv = top
        for k in reversed(range(plan.depth)):
            idx, _, split = plan.matrix(k)
            vals = plan.diags(k)
            hi, lo = self.ctx[lv], self.ctx[lv - 1]
            terms = [(i, j) for i in sorted(split) for j in sorted(split[i])]
            rot = np.stack([np.roll(vals[idx.index(i + j)], i, axis=0) for i, j in terms])   # [c] <- [(c - i) mod l]
            d_hi = np.ascontiguousarray(rot[..., 0] + 1j * rot[..., 2])
            d_lo = np.ascontiguousarray(rot[..., 1] + 1j * rot[..., 3])
            pts = self.enc.encode(hi, self.scale, dev(torch, d_hi), dev(torch, d_lo))
            mk = lambda ctx, x, at: fhe.CkksKey(ctx, cut(self.keys[x][0], at, self.L), cut(self.keys[x][1], at, self.L), self.n)  # noqa: E731
            keys_hi = {j: mk(hi, j, lv) for j in {j for js in split.values() for j in js} if j}
            keys_lo = {i: mk(lo, i, lv - 1) for i in split if i}
            cb, ca = fhe.CkksDiagMatrix(hi, lo, self.n, split, pts, keys_hi, keys_lo).apply(cb, ca)
            lv -= 1
        return cb, ca

    def transform(self, plan, top, keys=None):
        keys = self.rot_keys(plan.rotations) if keys is None else keys
        keys = {j: (cut(kb, top, self.L), cut(ka, top, self.L)) for j, (kb, ka) in keys.items()}
        return self.fhe.CkksLinearTransform(plan, [self.ctx[lv] for lv in range(top, top - plan.depth - 1, -1)], self.scale, keys)


_INSTANCES = {}


def instance(fhe, torch, log_n, big_l):
    key = (log_n, big_l)
    if key not in _INSTANCES:
        _INSTANCES[key] = Instance(fhe, torch, log_n, big_l)
    return _INSTANCES[key]


# ---- 5. device diag_rot + encode against the host rotation ------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,big_l,r,inverse", [(6, 4, 2, False), (6, 4, 2, True), (11, 6, 4, False)])
def test_apply_equals_the_hand_made_chain(fhe, torch_cuda, log_n, big_l, r, inverse):
    """the transform's apply on a batch of 2 ciphertexts equals, bit for bit, the chain of CkksDiagMatrix built from the read-back
    diagonals rotated on the host.  log_n = 11 lies beyond the reference's own test (log_n <= 9): its decode error has no reference
    figure and is printed, not asserted."""
    inst = instance(fhe, torch_cuda, log_n, big_l)
    plan = fhe.CkksLinearPlan(inst.enc, r, inverse)
    inst.rot_keys(plan.rotations)
    m0 = inst.slots(2, 5)
    cb, ca = inst.encrypt(m0)
    gb, ga = inst.transform(plan, big_l).apply(cb, ca)
    wb, wa = inst.hand_chain(plan, big_l, cb, ca)
    assert gb.shape == (2, big_l - plan.depth, inst.n)
    assert torch_cuda.equal(gb, wb) and torch_cuda.equal(ga, wa)
    inst.enc.status(cb)
    if log_n == 11:
        got = inst.decode(big_l - plan.depth, gb, ga)[0]
        want = Mo.sfft(Mo.bit_reverse([Mo.mpc(complex(v)) for v in m0[0]]))
        e = max(max(abs(Mo.mpf(float(g.real)) - w.real), abs(Mo.mpf(float(g.imag)) - w.imag)) for g, w in zip(got, want))
        print("slot_to_coeff (log_n = 11, L = 6, r = 4): decode error 2^%.1f (not asserted: beyond the reference's range)" % err_bits(e))


# ---- 6. rtk_gen -------------------------------------------------------------------------------------------------------------------
def test_rtk_gen_rows(fhe, cref, torch_cuda):
    """ckks.rs:174-184: the key for j is an encryption of P sk(X^(5^j mod 2n)) under sk over qs ++ ps: b + a s - P sk' is one small
    integer polynomial on every limb (keygen_checks.ckks_residual), within dg(3.2, 6)'s support, not zero; j is taken mod l; j = 0
    mod l is refused; host and device memory give the same bits"""
    from oracle import pyref as P
    from learn_fhe_amd import _lib
    prime = lambda bits: cref.two_adic_primes(bits, 7, 1)[0]  # noqa: E731
    n, l = 64, 32
    qs, ps = [prime(60), prime(50), prime(45)], [prime(62), prime(55)]
    mods = qs + ps
    rns = fhe.RnsContext(qs, ps)
    like = dev(torch_cuda, np.zeros(1, dtype=np.uint64))
    sk = fhe.sample_zo(0.5, 41, 0, like, n)
    s = host(sk).view(np.int64)
    big_p = 1
    for p in ps:
        big_p *= p
    seen = []
    for sid, j in enumerate((1, l - 1, l + 3, -1)):
        kb, ka = fhe.rtk_gen(rns, sk, n, j, 42, sid)
        spr = np.array(P.sk_automorphism([int(v) for v in s], pow(5, j % l, 2 * n)), dtype=np.int64)
        term = np.stack([K.scalar_mul_mod(m, np.mod(spr, m).astype(np.uint64), big_p % m) for m in mods])
        res = K.ckks_residual(mods, s, host(kb)[None], host(ka)[None], term[None])
        for i in range(len(mods)):
            assert np.array_equal(res[i], res[0]), "j=%d: limb %d disagrees with limb 0" % (j, i)
            assert int(host(ka)[i].max()) < mods[i]
        assert 0 < int(np.abs(res[0]).max()) <= DG_MAX
        seen.append(res[0, 0])
        xb, xa = fhe.rtk_gen(rns, host(sk), n, j, 42, sid)
        assert np.array_equal(xb, host(kb)) and np.array_equal(xa, host(ka))
    K.rows_independent(np.stack(seen))
    lib = _lib.lib()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = dev(torch_cuda, np.zeros((5, n), dtype=np.uint64))
    rng = fhe.Rng(seed=42)
    for j in (0, l, -l, 3 * l):
        assert lib.fhe_ckks_rtk_gen(rns.handle, vp(sk), n, j, rng._h, 0, vp(out), vp(out), _lib.MEM_DEVICE, None) == INVALID
    assert lib.fhe_ckks_rtk_gen(rns.handle, vp(sk), n, 1, rng._h, 0, None, vp(out), _lib.MEM_DEVICE, None) == INVALID


# ---- 7. the reference's coeff_to_slot_to_coeff ------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [2, 5, 9])
def test_reference_coeff_to_slot_to_coeff(fhe, torch_cuda, log_n):
    """bootstrapping.rs:121-141 with (log_qi, L, r) = (55, 8, 3) on device entries only: sample_zo, rtk_gen for the union of both
    plans, pk_encrypt(encode(m0)), slot_to_coeff -> sfft(bit_reverse(m0)), coeff_to_slot -> m0, both to the reference's 2^-30"""
    big_l, r = 8, 3
    inst = instance(fhe, torch_cuda, log_n, big_l)
    fwd, inv = fhe.CkksLinearPlan(inst.enc, r, False), fhe.CkksLinearPlan(inst.enc, r, True)
    inst.rot_keys(sorted(set(fwd.rotations) | set(inv.rotations)))
    m0 = inst.slots(1, 55)
    cb, ca = inst.encrypt(m0)
    b1, a1 = inst.transform(fwd, big_l).apply(cb, ca)
    mid = big_l - fwd.depth
    b2, a2 = inst.transform(inv, mid).apply(b1, a1)
    m1 = Mo.sfft(Mo.bit_reverse([Mo.mpc(complex(v)) for v in m0[0]]))
    err = lambda got, want: max(max(abs(Mo.mpf(float(g.real)) - w.real), abs(Mo.mpf(float(g.imag)) - w.imag)) for g, w in zip(got, want))  # noqa: E731
    e1 = err(inst.decode(mid, b1, a1)[0], m1)
    e2 = err(inst.decode(mid - inv.depth, b2, a2)[0], [Mo.mpc(complex(v)) for v in m0[0]])
    print("coeff_to_slot_to_coeff log_n=%d: slot_to_coeff error 2^%.1f, coeff_to_slot error 2^%.1f" % (log_n, err_bits(e1), err_bits(e2)))
    inst.enc.status(cb)
    assert e1 < Mo.mpf(2) ** -30
    assert e2 < Mo.mpf(2) ** -30


# ---- 8. host-memory operands ------------------------------------------------------------------------------------------------------
def test_host_memory_gives_the_same_bits(fhe, torch_cuda):
    inst = instance(fhe, torch_cuda, 6, 4)
    plan = fhe.CkksLinearPlan(inst.enc, 2, False)
    keys = inst.rot_keys(plan.rotations)
    cb, ca = inst.encrypt(inst.slots(2, 8))
    gb, ga = inst.transform(plan, 4).apply(cb, ca)
    t_host = inst.transform(plan, 4, {j: (host(kb), host(ka)) for j, (kb, ka) in keys.items()})
    hb, ha = t_host.apply(host(cb), host(ca))
    assert isinstance(hb, np.ndarray) and np.array_equal(hb, host(gb)) and np.array_equal(ha, host(ga))


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(fhe, torch_cuda):
    from learn_fhe_amd import _lib
    lib = _lib.lib()
    inst = instance(fhe, torch_cuda, 6, 4)
    n, big_l = inst.n, 4
    plan = fhe.CkksLinearPlan(inst.enc, 2, False)
    assert plan.depth == 3
    keys = inst.rot_keys(plan.rotations)
    idx = sorted(keys)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def prepare(plan_h, ctxs, idx, out=True):
        h = C.c_void_p()
        lv = (C.c_void_p * len(ctxs))(*[c.handle for c in ctxs])
        kb = (C.c_void_p * len(idx))(*[vp(keys[j][0]).value for j in idx])
        ka = (C.c_void_p * len(idx))(*[vp(keys[j][1]).value for j in idx])
        rc = lib.fhe_ckks_linear_transform_prepare(plan_h, lv, len(ctxs), inst.scale, (C.c_uint32 * len(idx))(*idx), kb, ka, len(idx), _lib.MEM_DEVICE,
                                                   C.byref(h) if out else None)
        assert rc != 0 and not h.value or rc == 0 and h.value
        if h.value:
            lib.fhe_ckks_linear_transform_destroy(h)
        return rc

    chain = [inst.ctx[lv] for lv in (4, 3, 2, 1)]
    assert prepare(plan.handle, chain, idx) == 0                                    # the good call
    assert prepare(plan.handle, chain, idx[:-1]) == INVALID                         # a missing rotation key
    assert prepare(plan.handle, chain[:-1], idx) == INVALID                         # a level chain one short
    assert prepare(plan.handle, [chain[0], chain[2], chain[2], chain[3]], idx) == INVALID   # not the prefix chain
    other_ps = fhe.RnsContext(inst.qs[:3], inst.ps[:-1])
    assert prepare(plan.handle, [chain[0], other_ps, chain[2], chain[3]], idx) == INVALID   # different ps
    host_ctx = [fhe.RnsContext(inst.qs[:lv], inst.ps, device=-1) for lv in (4, 3, 2, 1)]
    assert prepare(plan.handle, host_ctx, idx) == INVALID                           # contexts on no device, the encoder on one
    assert prepare(plan.handle, [host_ctx[0]] + chain[1:], idx) == INVALID
    host_plan = fhe.CkksLinearPlan(fhe.CkksEncoder(n, device=-1), 2, False)
    assert prepare(host_plan.handle, chain, idx) == INVALID                         # .. and the other way round
    assert prepare(None, chain, idx) == INVALID
    assert prepare(plan.handle, chain, idx, out=False) == INVALID                   # NULL out
    short = instance(fhe, torch_cuda, 6, 4)
    assert prepare(plan.handle, [short.ctx[lv] for lv in (3, 2, 1)] + [short.ctx[1]], idx) == INVALID  # L < depth + 1
    t = inst.transform(plan, big_l)
    cb, ca = inst.encrypt(inst.slots(1, 9))
    ob = dev(torch_cuda, np.zeros((1, 1, n), dtype=np.uint64))
    apply = lambda *a: lib.fhe_ckks_linear_transform_apply(t._h, *a, _lib.MEM_DEVICE, None)  # noqa: E731
    assert apply(vp(cb), vp(ca), None, vp(ob), 1) == INVALID                        # NULL outputs
    assert apply(vp(cb), vp(ca), vp(ob), None, 1) == INVALID
    assert apply(None, vp(ca), vp(ob), vp(ob), 1) == INVALID
    assert apply(None, None, None, None, 0) == 0                                    # batch == 0
    assert lib.fhe_ckks_linear_transform_apply(None, vp(cb), vp(ca), vp(ob), vp(ob), 1, _lib.MEM_DEVICE, None) == INVALID
