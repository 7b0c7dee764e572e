/* Three encrypted bytes through a 256-entry byte -> byte table in ONE call, from plain C: include/fhe_ring.h and libfhe_ring.so only.
 * The 3 x 8 address bits arrive as TLWE ciphertexts (pt = bit << 62, scheme/tfhe/src/tlwe.rs:122-132), ordered [byte][bit]; one call of
 * fhe_tfhe_circuit_bootstrap turns them into the rows of 24 TGGSW ciphertexts (tggsw.rs:79-88) and fhe_tggsw_prepare with count = 24
 * makes them CMUX selectors.  The table is packed vertically (fhe_tfhe_lut_pack): m = 8 address bits, n_out = 8 output bits, N = 1024, so
 * per_acc = 4 output bits share one accumulator and there are 2 accumulators; fhe_tfhe_lut_eval then spends 8 CMUXes per accumulator --
 * acc <- CMUX(selector l; acc, acc X^(-2^l)) -- where a CMUX tree would spend 255 per output bit, every byte under its own selectors.
 * Output bit o of byte c comes back as a TLWE ciphertext of (bit << 62) under the TGLWE key's coefficients (tlwe.rs:134-142): the form
 * the circuit bootstrap takes, so look-ups chain.  Parameters: those of the library's decode-level test (N = 1024, n_lwe = 8,
 * bootstrapping gadget (10, 4), selector gadget (4, 6), key-switch gadget (7, 6)).
 * build: gcc -std=c99 -O2 -I include examples/tfhe_lut_demo.c -L learn-fhe_amd/lib -lfhe_ring -Wl,-rpath,$PWD/learn-fhe_amd/lib \
 *            -Wl,--allow-shlib-undefined -o tfhe_lut_demo */
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
#define M 8
#define ENTRIES (1 << M)
#define N_OUT 8
#define BYTES 3
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
    CHECK(fhe_rng_create_from_seed(2028, &rng));
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
    for (int k = 0; k < N; ++k) funcs[k] = (uint64_t)0 - s[k];
    funcs[N] = 1;
    CHECK(fhe_tlwe_pfksk_gen(t, PF_LOG_B, PF_D, s, N, s, N, funcs, 2, SD_GLWE, rng, 4, pfksk, FHE_MEM_HOST, NULL));

    /* the byte -> byte table (an affine map followed by a bit rotation: a permutation of 0 .. 255) and its eight bit planes */
    static unsigned sbox[ENTRIES];
    static uint64_t table[N_OUT * ENTRIES];
    for (int x = 0; x < ENTRIES; ++x) {
        const unsigned y = (unsigned)(x * 167 + 99) & 0xff;
        sbox[x] = ((y << 3) | (y >> 5)) & 0xff;
        for (int o = 0; o < N_OUT; ++o) table[(size_t)o * ENTRIES + x] = (uint64_t)((sbox[x] >> o) & 1) << 62;
    }
    int r = 0;
    size_t per_acc = 0, n_acc = 0, n_polys = 0, ws_words = 0;
    CHECK(fhe_tfhe_lut_shape(M, N_OUT, N, &r, &per_acc, &n_acc, &n_polys));
    if (r != 8 || per_acc != 4 || n_acc != 2 || n_polys != 2) { fprintf(stderr, "unexpected shape\n"); return 1; }
    uint64_t *polys = malloc(n_polys * N * 8);
    if (!polys) return 1;
    CHECK(fhe_tfhe_lut_pack(table, M, N_OUT, N, polys));
    CHECK(fhe_tfhe_lut_workspace(N, M, N_OUT, 0, BYTES, &ws_words));

    /* the encrypted bytes: bit l of byte c is ciphertext c * M + l */
    const unsigned bytes[BYTES] = {0x00, 0xFF, 0xA5};
    static uint64_t msg[BYTES * M], lwe_a[BYTES * M * N_LWE], lwe_b[BYTES * M];
    for (int c = 0; c < BYTES; ++c)
        for (int l = 0; l < M; ++l) msg[c * M + l] = (uint64_t)((bytes[c] >> l) & 1) << 62;
    CHECK(fhe_tlwe_sk_encrypt(z, msg, N_LWE, BYTES * M, SD_LWE, rng, 5, lwe_a, lwe_b, FHE_MEM_HOST, NULL));

    /* circuit bootstrap: 24 TLWE bits -> the rows of 24 TGGSW ciphertexts, prepared once */
    const size_t sel_words = (size_t)BYTES * M * 2 * CB_D * N;
    uint64_t *sa = malloc(sel_words * 8), *sb = malloc(sel_words * 8);
    if (!sa || !sb) return 1;
    CHECK(fhe_tfhe_circuit_bootstrap(t, brk, CB_LOG_B, CB_D, PF_LOG_B, PF_D, pfksk, lwe_a, lwe_b, sa, sb, BYTES * M, FHE_MEM_HOST, NULL));
    fhe_tggsw_key *sel = NULL;
    CHECK(fhe_tggsw_prepare(t, CB_LOG_B, CB_D, sa, sb, N, BYTES * M, FHE_MEM_HOST, &sel));

    /* the look-up: one call for the three bytes, no key switch (the results stay under the extracted key) */
    static uint64_t out_a[BYTES * N_OUT * N], out_b[BYTES * N_OUT];
    CHECK(fhe_tfhe_lut_eval(t, sel, 0, M, polys, N_OUT, 0, 0, NULL, NULL, 0, out_a, out_b, BYTES, FHE_MEM_HOST, NULL));
    int bad = 0;
    for (int c = 0; c < BYTES; ++c) {
        unsigned got = 0;
        for (int o = 0; o < N_OUT; ++o) {
            const uint64_t *a = out_a + ((size_t)c * N_OUT + o) * N;
            uint64_t phase = out_b[c * N_OUT + o];
            for (int j = 0; j < N; ++j) phase -= a[j] * s[j];
            got |= (unsigned)(((phase + ((uint64_t)1 << 61)) >> 62) & 1) << o;
        }
        printf("table[0x%02x] = 0x%02x\n", bytes[c], got);
        if (got != sbox[bytes[c]]) bad = 1;
    }
    if (bad) { fprintf(stderr, "wrong entry\n"); return 1; }
    printf("tfhe_lut_demo ok: %d bytes, %d output bits each, %zu accumulators of %d CMUXes per byte (%zu words of scratch)\n", BYTES, N_OUT, n_acc, M,
           ws_words);
    fhe_tggsw_key_destroy(sel);
    fhe_tggsw_key_destroy(brk);
    fhe_rng_destroy(rng); fhe_torus_ctx_destroy(t);
    free(ra); free(rb); free(pfksk); free(sa); free(sb); free(polys);
    return 0;
}
