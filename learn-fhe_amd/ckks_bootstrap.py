"""CKKS bootstrap glue (include/fhe_ring.h fhe_ckks_cjk_gen, fhe_ckks_mod_raise, fhe_ckks_conj_split / _join,
fhe_ckks_eval_mod_plan_create, fhe_ckks_bootstrap_*): ctypes wrappers, the bootstrapper that keeps its borrowed stages alive, and the
composition of the seven public calls that one fhe_ckks_bootstrap_apply must equal bit for bit."""
from __future__ import annotations

import ctypes as C

from . import _lib as L
from .ckks_poly import CkksPolyEval, CkksPolyPlan
from .ring import CkksKey, CkksLinearTransform, RnsContext, _buf, _like, _rng


def cjk_gen(rns: RnsContext, sk, n, seed, stream_id):
    """scheme/ckks/src/ckks.rs:169-172 `Ckks::cjk_gen` -> (ksk_b, ksk_a) [L+K][n] for the conjugation X -> X^-1."""
    ps, _, mem, st = _buf(sk)
    kb, ka = _like(sk, (rns.L + rns.K, n)), _like(sk, (rns.L + rns.K, n))
    L.check(L.lib().fhe_ckks_cjk_gen(rns.handle, ps, n, _rng(seed), stream_id, _buf(kb)[0], _buf(ka)[0], mem, st), "fhe_ckks_cjk_gen")
    return kb, ka


def mod_raise(rns: RnsContext, ct_b, ct_a, n):
    """fhe_ckks_mod_raise: [batch][in_limbs][n], limb 0 read -> (b, a) [batch][rns.L][n]"""
    pb, cnt, mem, st = _buf(ct_b)
    in_limbs = int(ct_b.shape[-2])
    batch = cnt // (in_limbs * n)
    ob, oa = _like(ct_b, (batch, rns.L, n)), _like(ct_b, (batch, rns.L, n))
    L.check(L.lib().fhe_ckks_mod_raise(rns.handle, pb, _buf(ct_a)[0], in_limbs, _buf(ob)[0], _buf(oa)[0], n, batch, mem, st), "fhe_ckks_mod_raise")
    return ob, oa


def conj_split(rns: RnsContext, ct_b, ct_a, cj_b, cj_a, n):
    """fhe_ckks_conj_split: ct and its conjugate, [batch][rns.L][n] each -> (b, a) [2 batch][rns.L][n]: rows [0, batch) = ct + cj, rows
    [batch, 2 batch) = -X^(n/2) (ct - cj)"""
    pb, cnt, mem, st = _buf(ct_b)
    batch = cnt // (rns.L * n)
    ob, oa = _like(ct_b, (2 * batch, rns.L, n)), _like(ct_b, (2 * batch, rns.L, n))
    L.check(L.lib().fhe_ckks_conj_split(rns.handle, pb, _buf(ct_a)[0], _buf(cj_b)[0], _buf(cj_a)[0], _buf(ob)[0], _buf(oa)[0], n, batch, mem, st),
            "fhe_ckks_conj_split")
    return ob, oa


def conj_join(rns: RnsContext, in_b, in_a, n):
    """fhe_ckks_conj_join: [2 batch][rns.L][n] (rows [0, batch) = R', the rest J') -> (b, a) [batch][rns.L][n] = R' + X^(n/2) J'"""
    pb, cnt, mem, st = _buf(in_b)
    batch = cnt // (2 * rns.L * n)
    ob, oa = _like(in_b, (batch, rns.L, n)), _like(in_b, (batch, rns.L, n))
    L.check(L.lib().fhe_ckks_conj_join(rns.handle, pb, _buf(in_a)[0], _buf(ob)[0], _buf(oa)[0], n, batch, mem, st), "fhe_ckks_conj_join")
    return ob, oa


def eval_mod_plan_c(K, r, degree, pre=1.0, post=1.0):
    """fhe_ckks_eval_mod_plan_create as a CkksPolyPlan (host only): slots x -> post / (2 pi) sin(2 pi pre x) where |pre x| <= K"""
    plan = CkksPolyPlan.__new__(CkksPolyPlan)
    plan._h = C.c_void_p()
    L.check(L.lib().fhe_ckks_eval_mod_plan_create(K, r, degree, C.c_double(pre), C.c_double(post), C.byref(plan._h)), "fhe_ckks_eval_mod_plan_create")
    d, o, g = C.c_int(), C.c_int(), C.c_int()
    L.check(L.lib().fhe_ckks_poly_plan_info(plan._h, C.byref(d), C.byref(o), C.byref(g)), "fhe_ckks_poly_plan_info")
    plan.depth, plan.n_ops, plan.n_regs = d.value, o.value, g.value
    return plan


def bootstrap_eval_mod_plan(K, r, degree, q0, scale):
    """the eval_mod plan of a bootstrap: slots 2 t / scale with t = c + q0 I -> about c / scale (pre = scale / (2 q0), post = q0 / scale)"""
    return eval_mod_plan_c(K, r, degree, scale / (2.0 * q0), q0 / float(scale))


class CkksBootstrapper:
    """fhe_ckks_bootstrap_prepare / _apply: levels (RnsContexts over qs[:L], qs[:L-1], ..), the coeff_to_slot transform on levels[0:],
    the eval_mod evaluator on levels[c2s depth:], the slot_to_coeff transform after it, and ONE conjugation key (cjk_b, cjk_a) [L+K][n]
    over levels[0].  Keeps the stages and the contexts alive."""

    def __init__(self, levels, c2s: CkksLinearTransform, evaluator: CkksPolyEval, s2c: CkksLinearTransform, cjk_b, cjk_a, n):
        self.levels, self.c2s, self.evaluator, self.s2c, self.n = list(levels), c2s, evaluator, s2c, n
        lv = (C.c_void_p * len(self.levels))(*[c.handle for c in self.levels])
        pb, _, mem, _ = _buf(cjk_b)
        self._h = C.c_void_p()
        L.check(L.lib().fhe_ckks_bootstrap_prepare(lv, len(self.levels), n, c2s._h, evaluator._h, s2c._h, pb, _buf(cjk_a)[0], mem, C.byref(self._h)),
                "fhe_ckks_bootstrap_prepare")
        d, o = C.c_int(), C.c_int()
        L.check(L.lib().fhe_ckks_bootstrap_info(self._h, C.byref(d), C.byref(o)), "fhe_ckks_bootstrap_info")
        self.depth, self.out_limbs = d.value, o.value

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and L is not None and getattr(L, "lib", None):  # (module globals are gone at interpreter shutdown)
            L.lib().fhe_ckks_bootstrap_destroy(h)

    def apply(self, ct_b, ct_a):
        """[batch][in_limbs][n], limb 0 read -> (b, a) [batch][L - depth][n] over levels[depth]"""
        pb, cnt, mem, st = _buf(ct_b)
        in_limbs = int(ct_b.shape[-2])
        batch = cnt // (in_limbs * self.n)
        ob, oa = _like(ct_b, (batch, self.out_limbs, self.n)), _like(ct_b, (batch, self.out_limbs, self.n))
        L.check(L.lib().fhe_ckks_bootstrap_apply(self._h, pb, _buf(ct_a)[0], in_limbs, _buf(ob)[0], _buf(oa)[0], batch, mem, st), "fhe_ckks_bootstrap_apply")
        return ob, oa


def replay_composed(top: RnsContext, c2s: CkksLinearTransform, cj_key: CkksKey, evaluator: CkksPolyEval, s2c: CkksLinearTransform, ct_b, ct_a, n):
    """the seven public calls by hand: what fhe_ckks_bootstrap_apply must equal bit for bit.  cj_key: the conjugation key cut down to and
    prepared on the context the coeff_to_slot transform ends on"""
    rb, ra = mod_raise(top, ct_b, ct_a, n)
    wb, wa = c2s.apply(rb, ra)
    cb, ca = (wb.clone(), wa.clone()) if hasattr(wb, "clone") else (wb.copy(), wa.copy())
    cj_key.rotate_(-1, cb, ca)
    sb, sa = conj_split(cj_key.rns, wb, wa, cb, ca, n)
    pb, pa = evaluator.apply(sb, sa)
    jb, ja = conj_join(evaluator.levels[evaluator.plan.depth], pb, pa, n)
    return s2c.apply(jb, ja)
