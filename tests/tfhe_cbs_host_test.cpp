// csrc/tfhe_cbs.hpp alone (no HIP, no library): the test polynomial of the circuit bootstrap, the output-row mapping of the private
// functional key switch, the workspace and the argument checks.  A stand-alone program (AddressSanitizer + UBSan in
// tests/test_tfhe_cbs_cpu.py).  `tfhe_cbs_host_test table <log_b> <d> <n>` prints the table, one word per line, for the Python model
// to compare; without arguments it runs the checks and prints "tfhe_cbs_host_test ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../learn-fhe_amd/csrc/tfhe_cbs.hpp"

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static int checks() {
    using namespace fhe;
    // nu and the gadget
    const int want_nu[17] = {0, 0, 1, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4};
    for (int d = 1; d <= 16; ++d) CHECK(cbs_nu(d) == want_nu[d]);
    CHECK(cbs_gadget(7, 3, 0) == (uint64_t(1) << 43) && cbs_gadget(7, 3, 2) == (uint64_t(1) << 57) && cbs_gadget(4, 16, 0) == 1);
    // the table, restated: every coefficient from the definition
    for (int d : {1, 2, 3, 4, 16}) {
        for (size_t n : {size_t(256), size_t(1024), size_t(2048)}) {
            const int log_b = d == 16 ? 4 : 6;
            std::vector<uint64_t> t(n, ~uint64_t(0));
            CHECK(cbs_table(log_b, d, n, t.data()) == FHE_OK);
            const size_t funcs = size_t(1) << cbs_nu(d);
            for (size_t c = 0; c < n; ++c) {
                const size_t j = c % funcs, base = c - j;
                const bool in = base >= n / 4 && base < 3 * n / 4 && j < (size_t)d;
                CHECK(t[c] == (in ? uint64_t(1) << (64 - log_b * d + (int)j * log_b) : 0));
            }
            CHECK(t[0] == 0 && t[n / 4] == cbs_gadget(log_b, d, 0) && t[3 * n / 4 - funcs] == cbs_gadget(log_b, d, 0) && t[3 * n / 4] == 0);
        }
    }
    // the row mapping is a permutation of 0 .. batch n_funcs - 1, and group = d with two functions is the TGGSW order
    for (size_t group : {size_t(1), size_t(2), size_t(3)})
        for (size_t n_funcs : {size_t(1), size_t(2), size_t(3)}) {
            const size_t batch = 4 * group;
            std::vector<int> seen(batch * n_funcs, 0);
            for (size_t r = 0; r < batch; ++r)
                for (size_t u = 0; u < n_funcs; ++u) {
                    const size_t o = pfks_out_row(r, u, n_funcs, group);
                    CHECK(o < seen.size() && !seen[o]);
                    seen[o] = 1;
                }
            for (size_t r = 0; r < batch; ++r) CHECK(group != 1 || pfks_out_row(r, 1 % n_funcs, n_funcs, 1) == r * n_funcs + 1 % n_funcs);
        }
    for (size_t b = 0; b < 3; ++b)
        for (size_t j = 0; j < 3; ++j)
            for (size_t u = 0; u < 2; ++u) CHECK(pfks_out_row(b * 3 + j, u, 2, 3) == b * 6 + u * 3 + j);
    // rejections
    CHECK(cbs_check(4, 0, 1024) == FHE_ERR_INVALID && cbs_check(4, 17, 1024) == FHE_ERR_INVALID && cbs_check(3, 16, 1024) == FHE_OK);
    CHECK(cbs_check(4, 16, 256) == FHE_OK);                     // n / 4 = 64, 2^nu = 16
    CHECK(cbs_check(4, 16, 32) == FHE_ERR_INVALID);             // n / 4 = 8 is no multiple of 2^nu = 16: the shape that fails
    CHECK(cbs_check(4, 8, 32) == FHE_ERR_UNSUPPORTED);          // n / 4 = 8 = 2^nu: only the ring is too small
    CHECK(cbs_check(4, 2, 4096) == FHE_ERR_UNSUPPORTED && cbs_check(4, 2, 1000) == FHE_ERR_INVALID && cbs_check(9, 8, 1024) == FHE_ERR_INVALID);
    std::vector<uint64_t> t(32);
    CHECK(cbs_table(4, 16, 32, t.data()) == FHE_ERR_INVALID && cbs_table(4, 2, 256, nullptr) == FHE_ERR_INVALID);
    CHECK(pfks_check(7, 3, 2, 1024, 1024, 3, 9) == FHE_OK && pfks_check(7, 3, 2, 1024, 1024, 3, 10) == FHE_ERR_INVALID);  // batch % group
    CHECK(pfks_check(7, 3, 5, 8, 256, 1, 4) == FHE_ERR_INVALID && pfks_check(7, 3, 0, 8, 256, 1, 4) == FHE_ERR_INVALID);   // n_funcs
    CHECK(pfks_check(7, 3, 4, 8, 256, 1, 4) == FHE_OK && pfks_check(7, 3, 1, 8, 256, 0, 4) == FHE_ERR_INVALID);
    CHECK(pfks_check(7, 10, 1, 8, 256, 1, 4) == FHE_ERR_INVALID && pfks_check(32, 2, 1, 8, 256, 1, 4) == FHE_ERR_UNSUPPORTED);
    CHECK(pfks_check(7, 3, 1, 0, 256, 1, 4) == FHE_ERR_INVALID && pfks_check(7, 3, 1, 8, 0, 1, 4) == FHE_ERR_INVALID);
    // sizes
    CHECK(pfksk_words(3, 1024, 2, 1024) == size_t(3) * 1025 * 4096);
    CHECK(cbs_workspace(1024, 630, 3, 5) == 2 * 5 * 1024 + 15 * 1024 + 5 * 630 + 5 + 15);
    std::printf("tfhe_cbs_host_test ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 5 && !std::strcmp(argv[1], "table")) {
        const int log_b = std::atoi(argv[2]), d = std::atoi(argv[3]);
        const size_t n = (size_t)std::atol(argv[4]);
        std::vector<uint64_t> t(n);
        const int rc = fhe::cbs_table(log_b, d, n, t.data());
        if (rc != FHE_OK) { std::printf("status %d\n", rc); return 2; }
        for (uint64_t v : t) std::printf("%llu\n", (unsigned long long)v);
        return 0;
    }
    return checks();
}
