// Host check that the lazy forward butterfly of learn-fhe_amd/csrc/arith.hpp (ArithDS<B>::ct_lazy, mul_raw, fold1) follows the bounds
// its compile-time schedule (DsLazy<B>) proves.  For every layer of the schedule -- every state: folding or not, with the largest
// value the schedule admits on the way in -- the butterfly runs on
//     X = the largest admitted input (and 0, and random values below it),
//     Y = 2^64 - 1, 0 and random 64-bit values (a multiplicand may be anything),
//     twiddle words at their maxima (a0 = b0 = 2^(B-31) - 1, a1 = b1 = 2^31 - 1) and the split form of real residues w < q,
//     c = the largest admitted c, c = 1 and a real modulus of the width,
// and the same steps are redone in unsigned __int128: no intermediate may reach 2^64 (the one wrapping operation, the final
// subtraction, must have a true value in [0, 2^64)), the outputs must stay below what the schedule states for the next layer, and
// with a real twiddle they must be congruent to x + w y and x - w y mod q.  A schedule whose span is one layer too long fails here.
// Built by tests/test_ds_lazy_cpu.py with the HIP compiler's host pass only (no GPU).  Exit code 0 = all checks passed.
#include <cstdio>
#include <cstdlib>

#include "../learn-fhe_amd/csrc/arith.hpp"

using fhe::u64;
typedef unsigned __int128 u128;

static u64 rng_state = 0x9e3779b97f4a7c15ull;
static u64 rnd() {  // SplitMix64
    u64 z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static u64 rnd_below(u128 bound) { return (u64)((((u128)rnd() << 64) | rnd()) % bound); }

static long fails = 0, checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { if (fails < 20) { printf("FAIL line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

// the butterfly's steps in 128 bits; returns false if an intermediate reaches 2^64
template <int B>
static bool model(bool foldx, u128 X, u128 Y, const uint4 &w, u64 c, u128 q, u64 K, u128 &Xo, u128 &Yo) {
    const u128 CAP = (u128)1 << 64, W = ((u128)1 << 32) - 1;
    u128 x = X;
    if (foldx) x = (X & (((u128)1 << B) - 1)) + (X >> B) * c;
    const u128 y0 = Y & W, y1 = Y >> 32;
    const u128 s1a = (u128)w.y * y0, s1 = s1a + (u128)w.w * y1;
    const u128 s0a = (u128)w.x * y0 + x, s0 = s0a + (u128)w.z * y1;
    const u128 v = (s1 & W) * ((u128)1 << (B - 31)) + s0;
    const u128 r = (s1 >> 32) * (2 * (u128)c) + v;
    const u128 off = 2 * x + (u128)K * q;  // taken mod 2^64 by the code: only off - r has to be a 64-bit value
    if (x >= CAP || s1 >= CAP || s0 >= CAP || v >= CAP || r >= CAP || off < r || off - r >= CAP) return false;
    Xo = r; Yo = off - r;
    return true;
}

template <int B>
static void run_one(int layer, u64 X, u64 Y, const uint4 &w, u64 c, bool real_w, u64 wval) {
    typedef fhe::ArithDS<B> A;
    typedef fhe::DsLazy<B> L;
    const u64 q = (u64(1) << B) - c;
    fhe::DsK m{};
    m.q = q; m.q2 = 2 * q; m.q4 = 4 * q; m.c = (unsigned)c; m.c2 = (unsigned)(2 * c); m.pw = 1u << (B - 31); m.qk = L::K * q;
    const bool foldx = L::fold_before(layer);
    u128 Xm = 0, Ym = 0;
    const bool ok = model<B>(foldx, X, Y, w, c, q, L::K, Xm, Ym);
    CHECK(ok, "B=%d layer %d: an intermediate reaches 2^64 (X=%llx Y=%llx c=%llu)", B, layer, X, Y, c);
    if (!ok) return;
    u64 Xg = X, Yg = Y;
    if (foldx) A::template ct_lazy<true>(Xg, Yg, w, m);
    else A::template ct_lazy<false>(Xg, Yg, w, m);
    CHECK((u128)Xg == Xm && (u128)Yg == Ym, "B=%d layer %d: code and model differ (X=%llx Y=%llx)", B, layer, X, Y);
    CHECK(Xm <= L::in_max(layer + 1) && Ym <= L::in_max(layer + 1), "B=%d layer %d: output above the schedule's bound", B, layer);
    if (real_w) {
        const u128 wy = (u128)wval * (Y % q) % q;
        CHECK(Xm % q == (X % q + wy) % q, "B=%d layer %d: X' != x + w y (mod q)", B, layer);
        CHECK(Ym % q == (X % q + q - wy) % q, "B=%d layer %d: Y' != x - w y (mod q)", B, layer);
    }
}

template <int B>
static void run_width(u64 c_real) {
    typedef fhe::ArithDS<B> A;
    typedef fhe::DsLazy<B> L;
    const u64 cs[3] = {(u64)L::CMAX, 1, c_real};
    const uint4 wmax{(1u << (B - 31)) - 1, 0x7fffffffu, (1u << (B - 31)) - 1, 0x7fffffffu};
    for (int ci = 0; ci < 3; ++ci) {
        const u64 c = cs[ci], q = (u64(1) << B) - c;
        for (int layer = 0; layer < L::MAX_LAYERS; ++layer) {
            const u128 in = L::in_max(layer);
            CHECK(in < ((u128)1 << 64), "B=%d layer %d: the schedule's own bound is not a 64-bit value", B, layer);
            u64 xs[6] = {(u64)in, 0, (u64)in - 1, rnd_below(in + 1), rnd_below(in + 1), rnd_below(in + 1)};
            u64 ys[6] = {~u64(0), 0, u64(1) << 63, 0xffffffffull, rnd(), rnd()};
            for (u64 X : xs)
                for (u64 Y : ys) {
                    run_one<B>(layer, X, Y, wmax, c, false, 0);
                    for (int t = 0; t < 4; ++t) {  // real table values: any residue below q in the split form, the extremes included
                        const u64 wv = t == 0 ? q - 1 : t == 1 ? 1 : rnd_below(q);
                        run_one<B>(layer, X, Y, A::split(wv, q), c, true, wv);
                    }
                }
        }
        // ... and the folds are needed: where the schedule folds, the unfolded butterfly on the largest input leaves 64 bits for some
        // admitted (y, c) -- so a schedule that folded one layer later would fail the checks above
        if (ci == 0)
            for (int layer = 0; layer < L::MAX_LAYERS; ++layer)
                if (L::fold_before(layer)) {
                    bool all_fit = true;
                    for (u64 cc : {(u64)L::CMAX, u64(1)})
                        for (u64 Y : {~u64(0), u64(0)}) {
                            u128 a, b;
                            all_fit = all_fit && model<B>(false, L::in_max(layer), Y, wmax, cc, ((u128)1 << B) - cc, L::K, a, b);
                        }
                    CHECK(!all_fit, "B=%d layer %d: folds although the unfolded butterfly fits", B, layer);
                }
        // the outputs of every transform length the kernels run become canonical with one fold and one conditional subtraction
        fhe::DsK m{};
        m.q = q; m.c = (unsigned)c;
        for (int n = 12; n <= L::MAX_LAYERS; ++n) {
            const u64 f = A::fold1((u64)L::in_max(n), m);
            CHECK(f < 2 * q, "B=%d: outputs of %d layers fold to %llx >= 2q", B, n, f);
        }
    }
}

int main() {
    run_width<60>(98303);  // 2^60 - 98303: the headline modulus
    run_width<55>(1u << 16 | 1);
    run_width<54>(77823);  // 2^54 - 77823
    // the schedule as derived: 60 bits fold the X inputs before every second layer from layer 2 on, the narrower widths never
    for (int l = 0; l < 16; ++l) {
        CHECK(fhe::DsLazy<60>::fold_before(l) == (l >= 2 && l % 2 == 0), "60 bits: fold before layer %d", l);
        CHECK(!fhe::DsLazy<55>::fold_before(l) && !fhe::DsLazy<54>::fold_before(l), "54 / 55 bits: fold before layer %d", l);
    }
    if (fails) { printf("%ld of %ld checks FAILED\n", fails, checks); return 1; }
    printf("%ld checks passed\n", checks);
    return 0;
}
