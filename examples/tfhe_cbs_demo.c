/* A 16-entry table read at an encrypted 4-bit address from plain C: include/fhe_ring.h and libfhe_ring.so only.  The four address bits
 * arrive as TLWE ciphertexts (pt = bit << 62, scheme/tfhe/src/tlwe.rs:122-132); ONE call of fhe_tfhe_circuit_bootstrap turns them into
 * the rows of four TGGSW ciphertexts (tggsw.rs:79-88), fhe_tggsw_prepare makes them CMUX selectors, and a CMUX tree (tggsw.rs:114-121)
 * over 16 trivial TGLWE ciphertexts -- level l is one fhe_tggsw_cmux call with selector l over 2^(3 - l) pairs -- leaves the entry in
 * coefficient 0; sample_extract(0) (tglwe.rs:115-127) and decryption under the TGLWE key's coefficients (tlwe.rs:134-142) follow.
 * Parameters (those of the library's decode-level test): N = 1024, n_lwe = 8, bootstrapping gadget (10, 4), selector gadget (4, 6)
 * (nu = 3: the mod switch drifts by at most 8 (N_LWE + 1) / 2 = 36 of 2 N = 2048 positions against a quarter ring of 256), key-switch
 * gadget (7, 6) (201.5 MB of key); table entries at log_p = 4 under one padding bit (half-slot 2^58).
 * build: gcc -std=c99 -O2 -I include examples/tfhe_cbs_demo.c -L learn-fhe_amd/lib -lfhe_ring -Wl,-rpath,$PWD/learn-fhe_amd/lib \
 *            -Wl,--allow-shlib-undefined -o tfhe_cbs_demo */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fhe_ring.h"

#define N 1024
#define N_LWE 8
#define LOG_B 10
#define D 4
#define CB_LOG_B 4
#define CB_D 6
#define PF_LOG_B 7
#define PF_D 6
#define M 4
#define ENTRIES (1 << M)
#define LOG_P 4
#define LOG_DELTA (64 - LOG_P - 1)
#define ADDRESSES 3
#define SD_LWE 9.313225746154785e-10
#define SD_GLWE 2.845267479601915e-15

#define CHECK(call)                                                                                  \
    do {                                                                                             \
        int rc_ = (call);                                                                            \
        if (rc_ != FHE_OK) { fprintf(stderr, "%s: %d (hip %d)\n", #call, rc_, fhe_last_hip_error()); return 1; } \
    } while (0)

int main(void) {
    fhe_torus_ctx *t = NULL;
    fhe_rng *rng = NULL;
    CHECK(fhe_torus_ctx_create(0, &t));
    CHECK(fhe_rng_create_from_seed(2027, &rng));
    /* z: the TLWE key, s: the TGLWE key, both binary; brk_i = TGGSW(z_i) under s (bootstrapping.rs:59-76) */
    static uint64_t z[N_LWE], s[N], pt[N_LWE * N], funcs[2 * N];
    CHECK(fhe_sample_binary(rng, 1, z, N_LWE, FHE_MEM_HOST, NULL));
    CHECK(fhe_sample_binary(rng, 2, s, N, FHE_MEM_HOST, NULL));
    for (int i = 0; i < N_LWE; ++i) pt[(size_t)i * N] = z[i];
    const size_t brk_words = (size_t)N_LWE * 2 * D * N, key_words = (size_t)PF_D * (N + 1) * 2 * 2 * N;
    uint64_t *ra = malloc(brk_words * 8), *rb = malloc(brk_words * 8), *pfksk = malloc(key_words * 8);
    if (!ra || !rb || !pfksk) return 1;
    CHECK(fhe_tggsw_encrypt(t, LOG_B, D, s, pt, N, N_LWE, SD_GLWE, rng, 3, ra, rb, FHE_MEM_HOST, NULL));
    fhe_tggsw_key *brk = NULL;
    CHECK(fhe_tggsw_prepare(t, LOG_B, D, ra, rb, N, N_LWE, FHE_MEM_HOST, &brk));
    /* the key-switch key from the extracted key (the coefficients of s) to s, for F_0 = -S and F_1 = 1 */
    for (int k = 0; k < N; ++k) funcs[k] = (uint64_t)0 - s[k];
    funcs[N] = 1;
    CHECK(fhe_tlwe_pfksk_gen(t, PF_LOG_B, PF_D, s, N, s, N, funcs, 2, SD_GLWE, rng, 4, pfksk, FHE_MEM_HOST, NULL));

    /* the table and the addresses; bit l of address k is ciphertext k * M + l */
    const unsigned table[ENTRIES] = {7, 2, 13, 0, 9, 15, 4, 11, 1, 14, 6, 3, 12, 8, 5, 10};
    const unsigned address[ADDRESSES] = {0, 6, 15};
    static uint64_t msg[ADDRESSES * M], lwe_a[ADDRESSES * M * N_LWE], lwe_b[ADDRESSES * M];
    for (int k = 0; k < ADDRESSES; ++k)
        for (int l = 0; l < M; ++l) msg[k * M + l] = (uint64_t)((address[k] >> l) & 1) << 62;
    CHECK(fhe_tlwe_sk_encrypt(z, msg, N_LWE, ADDRESSES * M, SD_LWE, rng, 5, lwe_a, lwe_b, FHE_MEM_HOST, NULL));

    /* circuit bootstrap: 12 TLWE bits -> the rows of 12 TGGSW ciphertexts, prepared with count = batch */
    const size_t sel_words = (size_t)ADDRESSES * M * 2 * CB_D * N;
    uint64_t *sa = malloc(sel_words * 8), *sb = malloc(sel_words * 8);
    if (!sa || !sb) return 1;
    size_t ws_words = 0;
    CHECK(fhe_tfhe_cbs_workspace(N, N_LWE, CB_D, ADDRESSES * M, &ws_words));
    CHECK(fhe_tfhe_circuit_bootstrap(t, brk, CB_LOG_B, CB_D, PF_LOG_B, PF_D, pfksk, lwe_a, lwe_b, sa, sb, ADDRESSES * M, FHE_MEM_HOST, NULL));
    fhe_tggsw_key *sel = NULL;
    CHECK(fhe_tggsw_prepare(t, CB_LOG_B, CB_D, sa, sb, N, ADDRESSES * M, FHE_MEM_HOST, &sel));

    static uint64_t cur_a[ENTRIES * N], cur_b[ENTRIES * N], c0a[ENTRIES / 2 * N], c0b[ENTRIES / 2 * N], c1a[ENTRIES / 2 * N], c1b[ENTRIES / 2 * N];
    static uint64_t out_a[N], out_b[1];
    int bad = 0;
    for (int k = 0; k < ADDRESSES; ++k) {
        memset(cur_a, 0, sizeof cur_a);
        memset(cur_b, 0, sizeof cur_b);
        for (int x = 0; x < ENTRIES; ++x) cur_b[(size_t)x * N] = (uint64_t)table[x] << LOG_DELTA;   /* trivial TGLWE (0, entry) */
        for (int l = 0; l < M; ++l) {
            const int half = ENTRIES >> (l + 1);
            for (int i = 0; i < half; ++i) {
                memcpy(c0a + (size_t)i * N, cur_a + (size_t)(2 * i) * N, N * 8);
                memcpy(c0b + (size_t)i * N, cur_b + (size_t)(2 * i) * N, N * 8);
                memcpy(c1a + (size_t)i * N, cur_a + (size_t)(2 * i + 1) * N, N * 8);
                memcpy(c1b + (size_t)i * N, cur_b + (size_t)(2 * i + 1) * N, N * 8);
            }
            CHECK(fhe_tggsw_cmux(t, sel, (size_t)(k * M + l), c0a, c0b, c1a, c1b, cur_a, cur_b, (size_t)half, FHE_MEM_HOST, NULL));
        }
        CHECK(fhe_tglwe_sample_extract(cur_a, cur_b, N, 0, out_a, out_b, 1, FHE_MEM_HOST, NULL));
        uint64_t phase = out_b[0];
        for (int j = 0; j < N; ++j) phase -= out_a[j] * s[j];
        const unsigned got = (unsigned)((phase + ((uint64_t)1 << (LOG_DELTA - 1))) >> LOG_DELTA);
        printf("table[%u] = %u\n", address[k], got);
        if (got != table[address[k]]) bad = 1;
    }
    if (bad) { fprintf(stderr, "wrong entry\n"); return 1; }
    printf("tfhe_cbs_demo ok: %d bits circuit-bootstrapped in one call (%zu words of scratch), %d CMUXes per look-up\n", ADDRESSES * M, ws_words, ENTRIES - 1);
    fhe_tggsw_key_destroy(sel);
    fhe_tggsw_key_destroy(brk);
    fhe_rng_destroy(rng); fhe_torus_ctx_destroy(t);
    free(ra); free(rb); free(pfksk); free(sa); free(sb);
    return 0;
}
