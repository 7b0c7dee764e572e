/* Three encrypted bytes with NO padding bit through a byte -> byte table in ONE call, and through the same call again, from plain C:
 * include/fhe_ring.h and libfhe_ring.so only.  A byte x arrives as ONE TLWE ciphertext of x << 56 (scheme/tfhe/src/tlwe.rs:122-132).
 * fhe_tfhe_wop_pbs splits it into its eight bits with one blind rotation per bit -- the rotation that yields the bit's TGGSW selector rows
 * also yields the correction that removes the bit from the remainder --, fills the selectors into a key reserved once
 * (fhe_tggsw_key_reserve: no allocation, copy or host wait per call), reads the packed table (fhe_tfhe_lut_pack) with eight CMUXes and
 * switches the result back to the small key.  The table holds T[x] << 56, so the output has the input's format and goes straight back in.
 * Parameters: those of the library's decode-level test (N = 1024, n_lwe = 8, bootstrapping gadget (10, 4), selector gadget (4, 6),
 * private key-switch gadget (7, 6), TLWE key-switch gadget (4, 8)).
 * build: gcc -std=c99 -O2 -I include examples/tfhe_wop_demo.c -L learn-fhe_amd/lib -lfhe_ring -Wl,-rpath,$PWD/learn-fhe_amd/lib \
 *            -Wl,--allow-shlib-undefined -o tfhe_wop_demo */
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
#define KS_LOG_B 4
#define KS_D 8
#define M 8
#define ENTRIES (1 << M)
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
    CHECK(fhe_rng_create_from_seed(2029, &rng));
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
    /* the TLWE key switch from the extracted key (s) to z: the corrections between the steps and the output */
    static uint64_t ksk_a[(size_t)N * KS_D * N_LWE], ksk_b[(size_t)N * KS_D];
    CHECK(fhe_tlwe_ksk_gen(KS_LOG_B, KS_D, z, N_LWE, s, N, SD_LWE, rng, 5, ksk_a, ksk_b, FHE_MEM_HOST, NULL));

    /* the byte -> byte table (an affine map followed by a bit rotation: a permutation of 0 .. 255) as words T[x] << 56 */
    static unsigned sbox[ENTRIES];
    static uint64_t table[ENTRIES], polys[N];
    for (int x = 0; x < ENTRIES; ++x) {
        const unsigned y = (unsigned)(x * 167 + 99) & 0xff;
        sbox[x] = ((y << 3) | (y >> 5)) & 0xff;
        table[x] = (uint64_t)sbox[x] << 56;
    }
    size_t n_polys = 0, ws_words = 0;
    CHECK(fhe_tfhe_lut_shape(M, 1, N, NULL, NULL, NULL, &n_polys));
    if (n_polys != 1) { fprintf(stderr, "unexpected shape\n"); return 1; }
    CHECK(fhe_tfhe_lut_pack(table, M, 1, N, polys));
    CHECK(fhe_tfhe_wop_workspace(N, N_LWE, M, CB_D, BYTES, &ws_words));

    /* the selector key, reserved once for BYTES x M selectors */
    fhe_tggsw_key *sel = NULL;
    CHECK(fhe_tggsw_key_reserve(t, CB_LOG_B, CB_D, N, BYTES * M, 0, &sel));

    /* the encrypted bytes: one ciphertext each, no padding bit */
    const unsigned bytes[BYTES] = {0x00, 0xFF, 0xA5};
    static uint64_t msg[BYTES], ct_a[BYTES * N_LWE], ct_b[BYTES], out_a[BYTES * N_LWE], out_b[BYTES];
    for (int c = 0; c < BYTES; ++c) msg[c] = (uint64_t)bytes[c] << 56;
    CHECK(fhe_tlwe_sk_encrypt(z, msg, N_LWE, BYTES, SD_LWE, rng, 6, ct_a, ct_b, FHE_MEM_HOST, NULL));

    unsigned want[BYTES];
    for (int c = 0; c < BYTES; ++c) want[c] = bytes[c];
    int bad = 0;
    for (int round = 1; round <= 2; ++round) {
        CHECK(fhe_tfhe_wop_pbs(t, brk, KS_LOG_B, KS_D, ksk_a, ksk_b, CB_LOG_B, CB_D, PF_LOG_B, PF_D, pfksk, M, ct_a, ct_b, sel, 0, polys, 1, KS_LOG_B, KS_D,
                               ksk_a, ksk_b, N_LWE, out_a, out_b, BYTES, FHE_MEM_HOST, NULL));
        for (int c = 0; c < BYTES; ++c) {
            uint64_t phase = out_b[c];
            for (int j = 0; j < N_LWE; ++j) phase -= out_a[c * N_LWE + j] * z[j];
            const unsigned got = (unsigned)((phase + ((uint64_t)1 << 55)) >> 56);
            printf("round %d: 0x%02x -> 0x%02x\n", round, want[c], got);
            if (got != sbox[want[c]]) bad = 1;
            want[c] = sbox[want[c]];
        }
        memcpy(ct_a, out_a, sizeof(out_a));
        memcpy(ct_b, out_b, sizeof(out_b));
    }
    if (bad) { fprintf(stderr, "wrong entry\n"); return 1; }
    printf("tfhe_wop_demo ok: %d bytes, two rounds, %d blind rotations and %d CMUXes per byte and round (%zu words of scratch for the selectors)\n", BYTES, M,
           M, ws_words);
    fhe_tggsw_key_destroy(sel);
    fhe_tggsw_key_destroy(brk);
    fhe_rng_destroy(rng); fhe_torus_ctx_destroy(t);
    free(ra); free(rb); free(pfksk);
    return 0;
}
