// csrc/tfhe_split.hpp as a stand-alone host program (built with -fsanitize=address,undefined by tests/test_tfhe_split_cpu.py): the role
// map of a cluster, the rule that decides whether a blind rotation splits, and the workspace sizes.  Prints "tfhe_split_host_test ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../learn-fhe_amd/csrc/tfhe_split.hpp"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main() {
    using namespace fhe;
    const int forms[4] = {FHE_TGGSW_FORM_60, FHE_TGGSW_FORM_30, FHE_TGGSW_FORM_FFT64, FHE_TGGSW_FORM_X3};
    const size_t cus_list[4] = {256, 304, 64, 7};

    // the role map covers every (output, piece) exactly once; members of even rank hold shares of output 0, of odd rank of output 1
    // (the kernel's gather relies on that)
    for (int G : {2, 6}) {
        std::vector<int> seen(6, 0);
        for (int rank = 0; rank < G; ++rank) {
            const TfheSplitRole r = tfhe_split_role(G, rank);
            CHECK(r.output == 0 || r.output == 1);
            CHECK(r.output == (rank & 1));
            CHECK(r.pieces != 0 && (r.pieces & ~7u) == 0);
            for (int p = 0; p < 3; ++p)
                if (r.pieces >> p & 1) ++seen[(size_t)(r.output * 3 + p)];
            if (G == 2) CHECK(r.pieces == 7u);
            if (G == 6) CHECK(r.pieces == 1u << (rank / 2));
        }
        for (int c = 0; c < 6; ++c) CHECK(seen[(size_t)c] == 1);
    }

    // option values
    for (long v : {-1L, 0L, 2L, 6L}) CHECK(tfhe_split_value_ok(v));
    for (long v : {-2L, 1L, 3L, 4L, 5L, 7L, 8L, 12L, 1L << 40}) CHECK(!tfhe_split_value_ok(v));

    for (size_t cus : cus_list) {
        // every form but x3, and x3 at every ring but N = 1024: one workgroup whatever the option
        for (int form : forms)
            for (int log_n = 0; log_n <= 16; ++log_n) {
                if (form == FHE_TGGSW_FORM_X3 && log_n == 10) continue;
                for (long opt : {-1L, 0L, 2L, 6L})
                    for (size_t batch : {size_t(0), size_t(1), size_t(3), cus / 6, cus / 2, cus, size_t(4096)}) CHECK(tfhe_split_g(form, log_n, batch, cus, opt) == 1);
            }
        // the eligible key
        const int X3 = FHE_TGGSW_FORM_X3;
        for (size_t batch = 0; batch <= 2 * cus + 2; ++batch) {
            CHECK(tfhe_split_g(X3, 10, batch, cus, 0) == 1);                                     // never split
            for (int G : {2, 6}) {                                                               // forced: that G exactly where batch * G fits
                const int want = batch >= 1 && batch * (size_t)G <= cus ? G : 1;
                CHECK(tfhe_split_g(X3, 10, batch, cus, G) == want);
            }
            const int rule = tfhe_split_g(X3, 10, batch, cus, -1);                              // the rule: an admissible G, or 1
            CHECK(rule == 1 || rule == 2 || rule == 6);
            CHECK(rule == 1 || (batch >= 1 && batch * (size_t)rule <= cus));
            for (long bad : {1L, 3L, 4L, 8L, -2L}) CHECK(tfhe_split_g(X3, 10, batch, cus, bad) == 1);  // (fhe_set_option refuses them)
        }
        CHECK(tfhe_split_g(X3, 10, cus / 2 + 1, cus, -1) == 1);
        // batches that no product with G may wrap around
        for (long opt : {-1L, 2L, 6L}) {
            CHECK(tfhe_split_g(X3, 10, ~size_t(0), cus, opt) == 1);
            CHECK(tfhe_split_g(X3, 10, ~size_t(0) / 2 + 1, cus, opt) == 1);
            CHECK(tfhe_split_g(X3, 10, ~size_t(0) / 6 + 1, cus, opt) == 1);
        }
    }

    // workspace: one 64-byte control line per cluster, then 2 (parity) x batch x G slabs of n 8-byte words
    CHECK(TFHE_SPLIT_CTL_BYTES == 64);
    for (size_t batch : {size_t(1), size_t(3), size_t(42), size_t(128)})
        for (int G : {2, 6}) {
            const size_t n = 1024;
            CHECK(tfhe_split_ctl_bytes(batch) == 64 * batch);
            CHECK(tfhe_split_ctl_bytes(batch) % 16 == 0);  // the slabs behind it take 16-byte accesses
            CHECK(tfhe_split_slab_bytes(batch, G, n) == 2 * (size_t)G * n * 8 * batch);
            CHECK(tfhe_split_ws_bytes(batch, G, n) == 64 * batch + 2 * batch * (size_t)G * 8192);
            // the last byte a member touches: parity 1, last cluster, last member, last word
            const size_t last = (batch * (size_t)G * n + (batch - 1) * (size_t)G * n + (size_t)(G - 1) * n + n) * 8;
            CHECK(last == tfhe_split_slab_bytes(batch, G, n));
        }
    CHECK(tfhe_split_ws_bytes(1, 2, 1024) == 64 + 32768);
    CHECK(tfhe_split_ws_bytes(42, 6, 1024) == 42 * 64 + 42 * 98304);

    std::printf("tfhe_split_host_test ok\n");
    return 0;
}
