"""The exact model of the CKKS linear transforms for tests/test_ckks_linear_*.py: scheme/ckks/src/sfft.rs:75-99 (`sfft_fmats`,
`sifft_fmats`), util/src/misc/matrix.rs:71-83 (`inv`), 94-123 (`mul_assign`, `product`) and the chunking of
scheme/ckks/src/bootstrapping.rs:23-31, restated in the 300-bit mpmath of tests/ckks_encode_model.py.  A matrix is a dict
{diagonal index: [l values]} with dense[c][(c + d) % l] = diag_d[c] (matrix.rs:87-91); nothing here is ever dense except `to_dense`,
which the self-check alone uses.  Indices are kept as the reference keeps them (an `inv` maps 0 to l); `normalised` folds them mod l,
which is what the library reports."""
import ckks_encode_model as Mo

mpc = Mo.mpc
ZERO, ONE = mpc(0), mpc(1)


def broadcast(n, pattern):
    """util/src/avec.rs:20-22"""
    return [pattern[i % len(pattern)] for i in range(n)]


def rot(v, j):
    """avec.rs:28-31 `rot_iter(j)`: position c reads c + j"""
    n = len(v)
    return [v[(c + j) % n] for c in range(n)]


def sfft_fmats(n):
    """sfft.rs:75-94"""
    out = []
    for log_k in range(n.bit_length() - 1):
        m = 1 << (n.bit_length() - 2 - log_k)
        w = Mo.w(2 * m)
        diag_zero = broadcast(n, [ONE] * m + [-t for t in w])
        if log_k == 0:
            out.append({0: diag_zero, n - m: broadcast(n, w + [ONE] * m)})
        else:
            out.append({0: diag_zero, n - m: broadcast(n, [ZERO] * m + [ONE] * m), m: broadcast(n, w + [ZERO] * m)})
    return out


def inv(mat, n):
    """matrix.rs:71-83"""
    return {n - j: [v.conjugate() / 2 for v in rot(d, n - j)] for j, d in mat.items()}


def sifft_fmats(n):
    """sfft.rs:97-99"""
    return [inv(m, n) for m in reversed(sfft_fmats(n))]


def mul(a, b, n):
    """matrix.rs:94-107: pairs in the order of the cartesian product of the two sorted maps, summed per output index"""
    out = {}
    for i in sorted(a):
        for j in sorted(b):
            rb = rot(b[j], i)
            term = [x * y for x, y in zip(a[i], rb)]
            k = (i + j) % n
            out[k] = term if k not in out else [s + t for s, t in zip(out[k], term)]
    return out


def product(mats, n):
    """matrix.rs:110-123: left to right; one item is returned as it is"""
    acc = dict(mats[0])
    for m in mats[1:]:
        acc = mul(acc, m, n)
    return acc


def chunked(n, r, inverse=False):
    """bootstrapping.rs:24-25: the product of every chunk of r"""
    f = sifft_fmats(n) if inverse else sfft_fmats(n)
    return [product(f[c:c + r], n) for c in range(0, len(f), r)]


def normalised(mat, n):
    """indices mod n (distinct indices of one matrix never meet: an `inv` has l only where it has no 0)"""
    out = {}
    for d, v in mat.items():
        assert d % n not in out
        out[d % n] = v
    return out


def rotation_union(mats, n, split):
    """bootstrapping.rs:61-64 over `split` = bsgs_split, on normalised indices: ascending non-zero i and j of every matrix"""
    out = set()
    for m in mats:
        _, s = split(sorted(normalised(m, n)))
        out |= set(s) | {j for js in s.values() for j in js}
    return sorted(out - {0})


def to_dense(mat, n):
    dense = [[ZERO] * n for _ in range(n)]
    for d, v in mat.items():
        for c in range(n):
            dense[c][(c + d) % n] = v[c]
    return dense


def from_dd4(a):
    """one read-back element (re_hi, re_lo, im_hi, im_lo) -> mpc"""
    return mpc(Mo.from_dd(a[0], a[1]), Mo.from_dd(a[2], a[3]))
