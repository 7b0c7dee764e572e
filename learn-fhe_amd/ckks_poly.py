"""CKKS polynomial evaluation (include/fhe_ring.h fhe_ckks_lincomb, fhe_ckks_mul_eval, fhe_ckks_poly_*): ctypes wrappers, the
float64 replay of an exported plan, and the `eval_mod` recipe (the scaled-sine modular reduction of a bootstrap) as a plan."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from .ring import CkksKey, RnsContext, _buf, _like

MUL, LIN = 0, 1
MAX_TERMS = 16


class PolyOp(C.Structure):
    """fhe_ckks_poly_op"""
    _fields_ = [("kind", C.c_int32), ("dst", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("alpha", C.c_int32), ("c", C.c_int32),
                ("mode", C.c_int32), ("n_terms", C.c_int32), ("src", C.c_int32 * 16), ("coef", C.c_double * 16), ("c0", C.c_double)]


def mul_op(dst, a, b, alpha=1, c=-1):
    return {"kind": MUL, "dst": dst, "a": a, "b": b, "alpha": alpha, "c": c}


def lin_op(dst, mode, terms, c0=0.0):
    """terms: [(register, multiplier)]; mode 0 = integer multipliers, no level; 1 = real multipliers, one level"""
    return {"kind": LIN, "dst": dst, "mode": mode, "terms": [(int(s), float(v)) for s, v in terms], "c0": float(c0)}


def _to_struct(op):
    o = PolyOp()
    o.kind, o.dst, o.c = op["kind"], op["dst"], -1
    if op["kind"] == MUL:
        o.a, o.b, o.alpha, o.c = op["a"], op["b"], op["alpha"], op["c"]
    else:
        o.mode, o.n_terms, o.c0 = op["mode"], len(op["terms"]), op["c0"]
        assert len(op["terms"]) <= MAX_TERMS
        for j, (s, v) in enumerate(op["terms"]):
            o.src[j], o.coef[j] = s, v
    return o


def _from_struct(o):
    if o.kind == MUL:
        return mul_op(o.dst, o.a, o.b, o.alpha, o.c)
    return lin_op(o.dst, o.mode, [(o.src[j], o.coef[j]) for j in range(o.n_terms)], o.c0)


def scaled_constant(c, scale, q):
    """trunc(c * scale) mod q, negative values as q - |k| mod q (fhe_ckks_scaled_constant)"""
    out = C.c_uint64()
    L.check(L.lib().fhe_ckks_scaled_constant(C.c_double(c), C.c_uint64(scale), C.c_uint64(q), C.byref(out)), "fhe_ckks_scaled_constant")
    return out.value


class CkksPolyPlan:
    """A host-only schedule (no GPU needed).  CkksPolyPlan(coeffs, basis) builds the baby-step / giant-step schedule of a Chebyshev
    (basis 0) or monomial (basis 1) series; CkksPolyPlan.from_ops(ops) takes a list of mul_op / lin_op records."""

    def __init__(self, coeffs, basis=0, _ops=None):
        self._h = C.c_void_p()
        if _ops is not None:
            arr = (PolyOp * len(_ops))(*[_to_struct(o) for o in _ops])
            L.check(L.lib().fhe_ckks_poly_plan_from_ops(arr, len(_ops), C.byref(self._h)), "fhe_ckks_poly_plan_from_ops")
        else:
            c = np.ascontiguousarray(coeffs, dtype=np.float64)
            L.check(L.lib().fhe_ckks_poly_plan_create(c.ctypes.data_as(C.POINTER(C.c_double)), len(c) - 1, basis, C.byref(self._h)),
                    "fhe_ckks_poly_plan_create")
        d, o, r = C.c_int(), C.c_int(), C.c_int()
        L.check(L.lib().fhe_ckks_poly_plan_info(self._h, C.byref(d), C.byref(o), C.byref(r)), "fhe_ckks_poly_plan_info")
        self.depth, self.n_ops, self.n_regs = d.value, o.value, r.value

    @classmethod
    def from_ops(cls, ops):
        return cls(None, _ops=list(ops))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and L is not None and getattr(L, "lib", None):  # (module globals are gone at interpreter shutdown)
            L.lib().fhe_ckks_poly_plan_destroy(h)

    @property
    def handle(self):
        return self._h

    @property
    def ops(self):
        arr = (PolyOp * self.n_ops)()
        L.check(L.lib().fhe_ckks_poly_plan_ops(self._h, arr, self.n_ops), "fhe_ckks_poly_plan_ops")
        return [_from_struct(o) for o in arr]


def depths(ops):
    """the level offset of every register of an op list: {register: depth}"""
    d = {0: 0}
    for o in ops:
        if o["kind"] == MUL:
            d[o["dst"]] = max(d[o["a"]], d[o["b"]]) + 1
        else:
            d[o["dst"]] = max(d[s] for s, _ in o["terms"]) + o["mode"]
    return d


def replay_f64(ops, x):
    """the op list evaluated in float64 on the points x: what the slots of the result hold up to the scheme's noise"""
    reg = {0: np.asarray(x, dtype=np.float64)}
    for o in ops:
        if o["kind"] == MUL:
            v = o["alpha"] * (reg[o["a"]] * reg[o["b"]])
            reg[o["dst"]] = v - reg[o["c"]] if o["c"] >= 0 else v
        else:
            v = np.full_like(reg[0], o["c0"])
            for s, k in o["terms"]:
                v = v + k * reg[s]
            reg[o["dst"]] = v
    return reg[ops[-1]["dst"]]


def transform_counts(ops):
    """(fused, composed): limb-vector transforms per ciphertext as multiples of the limb count at each op's level, i.e. the number of
    POLYNOMIAL transforms (forward + inverse, the key switch's own left out: both routes do the same there).  Fused: 2 forward per
    register that feeds a MUL, 3 inverse per MUL.  Composed (fhe_ckks_mul per MUL): 4 forward + 3 inverse per MUL."""
    feeds = set()
    muls = 0
    for o in ops:
        if o["kind"] == MUL:
            feeds.update((o["a"], o["b"]))
            muls += 1
    return 2 * len(feeds) + 3 * muls, 7 * muls


def lincomb(rns: RnsContext, cts, n, real, mults, c0, scale, out=None):
    """fhe_ckks_lincomb: cts [(b, a)], each [batch][limbs_j][n] with limbs_j >= rns.L -> (b, a) on rns.L (integer mode) or rns.L - 1 limbs"""
    k = len(cts)
    pb, cnt, mem, st = _buf(cts[0][0])
    limbs = [int(b.shape[-2]) for b, _ in cts]
    batch = cnt // (limbs[0] * n)
    lo = rns.L - 1 if real else rns.L
    ob, oa = out if out is not None else (_like(cts[0][0], (batch, lo, n)), _like(cts[0][0], (batch, lo, n)))
    bs = (C.c_void_p * k)(*[_buf(b)[0] for b, _ in cts])
    as_ = (C.c_void_p * k)(*[_buf(a)[0] for _, a in cts])
    im = (C.c_int64 * k)(*([0] * k if real else [int(v) for v in mults]))
    cm = (C.c_double * k)(*([float(v) for v in mults] if real else [0.0] * k))
    L.check(L.lib().fhe_ckks_lincomb(rns.handle, int(bool(real)), k, bs, as_, (C.c_int * k)(*limbs), im, cm, C.c_double(c0), C.c_uint64(scale),
                                     _buf(ob)[0], _buf(oa)[0], n, batch, mem, st), "fhe_ckks_lincomb")
    return ob, oa


def mul_eval(key: CkksKey, x, y, alpha=1, c=None):
    """fhe_ckks_mul_eval: x, y (b, a) in the evaluation domain on >= L limbs; c (b, a) coefficient domain on >= L - 1 limbs or None"""
    rns, n = key.rns, key.n
    pxb, cnt, mem, st = _buf(x[0])
    xl, yl = int(x[0].shape[-2]), int(y[0].shape[-2])
    batch = cnt // (xl * n)
    ob, oa = _like(x[0], (batch, rns.L - 1, n)), _like(x[0], (batch, rns.L - 1, n))
    cb, ca, cl = (_buf(c[0])[0], _buf(c[1])[0], int(c[0].shape[-2])) if c is not None else (None, None, 0)
    L.check(L.lib().fhe_ckks_mul_eval(rns.handle, key.handle, pxb, _buf(x[1])[0], xl, _buf(y[0])[0], _buf(y[1])[0], yl, alpha, cb, ca, cl, _buf(ob)[0],
                                      _buf(oa)[0], batch, mem, st), "fhe_ckks_mul_eval")
    return ob, oa


class CkksPolyEval:
    """fhe_ckks_poly_prepare / fhe_ckks_poly_apply: a plan bound to RnsContexts over qs[:L], qs[:L-1], .. (at least plan.depth + 1) and
    ONE relinearisation key (rlk_b, rlk_a) [L+K][n] over levels[0].  Keeps the contexts alive."""

    def __init__(self, plan: CkksPolyPlan, levels, scale, rlk_b, rlk_a, n):
        self.plan, self.levels, self.n = plan, list(levels), n
        lv = (C.c_void_p * len(self.levels))(*[c.handle for c in self.levels])
        pb, _, mem, _ = _buf(rlk_b)
        self._h = C.c_void_p()
        L.check(L.lib().fhe_ckks_poly_prepare(plan.handle, lv, len(self.levels), C.c_uint64(scale), pb, _buf(rlk_a)[0], n, mem, C.byref(self._h)),
                "fhe_ckks_poly_prepare")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and L is not None and getattr(L, "lib", None):  # (module globals are gone at interpreter shutdown)
            L.lib().fhe_ckks_poly_eval_destroy(h)

    def apply(self, ct_b, ct_a):
        """[batch][L][n] over levels[0] -> (b, a) [batch][L - depth][n]"""
        pb, cnt, mem, st = _buf(ct_b)
        lv = self.levels[0].L
        batch = cnt // (lv * self.n)
        ob, oa = _like(ct_b, (batch, lv - self.plan.depth, self.n)), _like(ct_b, (batch, lv - self.plan.depth, self.n))
        L.check(L.lib().fhe_ckks_poly_apply(self._h, pb, _buf(ct_a)[0], _buf(ob)[0], _buf(oa)[0], batch, mem, st), "fhe_ckks_poly_apply")
        return ob, oa


def replay_composed(ops, ctx_of, key_of, ct_b, ct_a, n, scale):
    """the op list through the small public entries: fhe_ckks_mul on contiguous prefix slices and fhe_ckks_lincomb.  ctx_of(limbs) ->
    RnsContext, key_of(limbs) -> CkksKey on it.  What fhe_ckks_poly_apply must equal bit for bit."""
    top = int(ct_b.shape[-2])
    d = depths(ops)
    reg = {0: (ct_b, ct_a)}
    cut = lambda t, lv: t if t.shape[-2] == lv else (t[:, :lv].contiguous() if hasattr(t, "contiguous") else np.ascontiguousarray(t[:, :lv]))  # noqa: E731
    for o in ops:
        if o["kind"] == MUL:
            lv = top - max(d[o["a"]], d[o["b"]])
            (xb, xa), (yb, ya) = reg[o["a"]], reg[o["b"]]
            out = key_of(lv).mul(cut(xb, lv), cut(xa, lv), cut(yb, lv), cut(ya, lv))
            if o["alpha"] == 2 or o["c"] >= 0:
                cts = [out] + ([reg[o["c"]]] if o["c"] >= 0 else [])
                out = lincomb(ctx_of(lv - 1), cts, n, False, [o["alpha"], -1][:len(cts)], 0.0, scale)
        else:
            lv = top - max(d[s] for s, _ in o["terms"])
            out = lincomb(ctx_of(lv), [reg[s] for s, _ in o["terms"]], n, bool(o["mode"]), [v for _, v in o["terms"]], o["c0"], scale)
        reg[o["dst"]] = out
    return reg[ops[-1]["dst"]]


def eval_mod_ops(K, r, degree):
    """The scaled-sine modular reduction as an op list: slots t = eps + I (|I| <= K an integer, eps small) -> about eps.
       1. u = t / K                                       one real-mode LIN;
       2. y = the degree-`degree` Chebyshev interpolant of cos(2 pi (K u - 1/4) / 2^r) on u in [-1, 1], by the fixed schedule;
       3. r double-angle steps y <- 2 y^2 - 1             a MUL with alpha = 2 and an integer LIN adding -1 each:
                                                          y = cos(2 pi t - pi / 2) = sin(2 pi t) ~ 2 pi eps;
       4. the factor 1 / (2 pi)                           one real-mode LIN.
    Returns (ops, series coefficients)."""
    f = lambda u: np.cos(2.0 * math.pi * (K * u - 0.25) / 2.0 ** r)  # noqa: E731
    coeffs = np.polynomial.chebyshev.chebinterpolate(f, degree)
    series = CkksPolyPlan(coeffs, 0).ops
    ops = [lin_op(1, 1, [(0, 1.0 / K)], 0.0)]
    shift = lambda g: g + 1  # noqa: E731  (the series' input is register 1)
    for o in series:
        if o["kind"] == MUL:
            ops.append(mul_op(shift(o["dst"]), shift(o["a"]), shift(o["b"]), o["alpha"], shift(o["c"]) if o["c"] >= 0 else -1))
        else:
            ops.append(lin_op(shift(o["dst"]), o["mode"], [(shift(s), v) for s, v in o["terms"]], o["c0"]))
    y = ops[-1]["dst"]
    nxt = max(o["dst"] for o in ops) + 1
    for _ in range(r):
        ops.append(mul_op(nxt, y, y, 2, -1))
        ops.append(lin_op(nxt + 1, 0, [(nxt, 1)], -1.0))
        y, nxt = nxt + 1, nxt + 2
    ops.append(lin_op(nxt, 1, [(y, 1.0 / (2.0 * math.pi))], 0.0))
    return ops, coeffs


def eval_mod_plan(K, r, degree):
    """eval_mod_ops as a CkksPolyPlan.  The rest of a bootstrap -- mod_raise, the conjugate split after coeff_to_slot, the recombination
    -- is the caller's."""
    return CkksPolyPlan.from_ops(eval_mod_ops(K, r, degree)[0])
