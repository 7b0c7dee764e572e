// Host driver of learn-fhe_amd/csrc/dd.hpp (tests/test_ckks_encode_cpu.py): the double-double arithmetic the encoder kernels use,
// run by plain g++ without a GPU.  Commands on stdin, hex floats both ways:
//   F l            then l lines "re_hi re_lo im_hi im_lo": prints sifft (l lines), then sfft of that output (l lines)
//   I s hi lo      the signed 128-bit integer (-1)^s (hi 2^64 + lo): prints from_i128 as "hi lo", then to_i128 of it as "ok s hi lo"
//   D hi lo        a dd: prints to_i128 (fraction dropped toward zero) as "ok s hi lo"
//   W s k w0 .. w(k-1)   a k-word magnitude (little endian): prints from_words as "hi lo"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../learn-fhe_amd/csrc/dd.hpp"

using namespace fhe::ddm;

static void print_i128(i128 v, bool ok) {
    const bool negative = v < 0;
    const u128 mag = negative ? (u128)0 - (u128)v : (u128)v;
    std::printf("%d %d %llu %llu\n", ok ? 1 : 0, negative ? 1 : 0, (u64)(mag >> 64), (u64)mag);
}

int main() {
    char cmd[8];
    while (std::scanf("%7s", cmd) == 1) {
        if (cmd[0] == 'F') {
            unsigned l;
            if (std::scanf("%u", &l) != 1 || l == 0 || (l & (l - 1))) return 2;
            std::vector<cdd> z(l), tw(4 * (size_t)l);
            std::vector<unsigned> pow5(l / 2 ? l / 2 : 1);
            for (unsigned i = 0; i < l; ++i)
                if (std::scanf("%la %la %la %la", &z[i].re.hi, &z[i].re.lo, &z[i].im.hi, &z[i].im.lo) != 4) return 2;
            twiddle_table(l, tw.data());
            pow5_table(l, pow5.data());
            sifft_host(z.data(), l, tw.data(), pow5.data());
            for (unsigned i = 0; i < l; ++i) std::printf("%a %a %a %a\n", z[i].re.hi, z[i].re.lo, z[i].im.hi, z[i].im.lo);
            sfft_host(z.data(), l, tw.data(), pow5.data());
            for (unsigned i = 0; i < l; ++i) std::printf("%a %a %a %a\n", z[i].re.hi, z[i].re.lo, z[i].im.hi, z[i].im.lo);
        } else if (cmd[0] == 'I') {
            int s;
            u64 hi, lo;
            if (std::scanf("%d %llu %llu", &s, &hi, &lo) != 3) return 2;
            const u128 mag = ((u128)hi << 64) | lo;
            const i128 v = s ? -(i128)mag : (i128)mag;
            const dd x = from_i128(v);
            std::printf("%a %a\n", x.hi, x.lo);
            bool ok;
            const i128 back = to_i128(x, ok);
            print_i128(back, ok);
        } else if (cmd[0] == 'D') {
            dd x;
            if (std::scanf("%la %la", &x.hi, &x.lo) != 2) return 2;
            bool ok;
            const i128 v = to_i128(x, ok);
            print_i128(v, ok);
        } else if (cmd[0] == 'W') {
            int s, k;
            if (std::scanf("%d %d", &s, &k) != 2 || k < 1 || k > 64) return 2;
            std::vector<u64> w(k);
            for (int i = 0; i < k; ++i)
                if (std::scanf("%llu", &w[i]) != 1) return 2;
            const dd x = from_words(w.data(), k, s != 0);
            std::printf("%a %a\n", x.hi, x.lo);
        } else {
            return 2;
        }
    }
    return 0;
}
