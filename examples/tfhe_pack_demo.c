/* Eight encrypted bytes packed into one TGLWE ciphertext from plain C: include/fhe_ring.h and libfhe_ring.so only.  The bytes arrive as
 * TLWE ciphertexts (pt = byte << 56, scheme/tfhe/src/tlwe.rs:122-132) under a key z of N_IN bits; the packing key is
 * fhe_tlwe_pfksk_gen's key for the one function F = 1 from z to the TGLWE key s; fhe_tlwe_pack_key_prepare transforms it once, and ONE
 * call of fhe_tlwe_pack puts input r at coefficient r N / 8 of one TGLWE ciphertext (tglwe.rs:91-103), 2 N words instead of
 * 8 (N_IN + 1).  The program decrypts the phase b - a s itself (a negacyclic product by the binary key) and rounds to 8 bits.
 * Parameters: N = 1024, N_IN = 16, key-switch gadget (7, 6): the digits round away 2^21 per input coefficient; key noise 2.8e-15 and
 * input noise 2^-30 leave the phase error far below the half-slot 2^55.
 * build: gcc -std=c99 -O2 -I include examples/tfhe_pack_demo.c -L learn-fhe_amd/lib -lfhe_ring -Wl,-rpath,$PWD/learn-fhe_amd/lib \
 *            -Wl,--allow-shlib-undefined -o tfhe_pack_demo */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "fhe_ring.h"

#define N 1024
#define N_IN 16
#define LOG_B 7
#define D 6
#define COUNT 8
#define STRIDE (N / COUNT)
#define LOG_DELTA 56
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
    /* z: the TLWE key, s: the TGLWE key, both binary; the packing key switches from z to s under the identity function */
    static uint64_t z[N_IN], s[N], funcs[N];
    CHECK(fhe_sample_binary(rng, 1, z, N_IN, FHE_MEM_HOST, NULL));
    CHECK(fhe_sample_binary(rng, 2, s, N, FHE_MEM_HOST, NULL));
    funcs[0] = 1;
    const size_t key_words = (size_t)D * (N_IN + 1) * 2 * N;
    uint64_t *pfksk = malloc(key_words * 8);
    if (!pfksk) return 1;
    CHECK(fhe_tlwe_pfksk_gen(t, LOG_B, D, z, N_IN, s, N, funcs, 1, SD_GLWE, rng, 3, pfksk, FHE_MEM_HOST, NULL));
    fhe_tlwe_pack_key *key = NULL;
    CHECK(fhe_tlwe_pack_key_prepare(t, LOG_B, D, pfksk, N_IN, N, FHE_MEM_HOST, NULL, &key));

    const unsigned bytes[COUNT] = {17, 200, 3, 255, 0, 128, 64, 99};
    static uint64_t msg[COUNT], ct_a[COUNT * N_IN], ct_b[COUNT], out_a[N], out_b[N];
    for (int r = 0; r < COUNT; ++r) msg[r] = (uint64_t)bytes[r] << LOG_DELTA;
    CHECK(fhe_tlwe_sk_encrypt(z, msg, N_IN, COUNT, SD_LWE, rng, 4, ct_a, ct_b, FHE_MEM_HOST, NULL));
    CHECK(fhe_tlwe_pack(t, key, ct_a, ct_b, COUNT, STRIDE, 1, out_a, out_b, FHE_MEM_HOST, NULL));

    /* phase = b - a s in Z_{2^64}[X]/(X^N + 1): X^j X^k = -X^(j + k - N) past the end */
    static uint64_t phase[N];
    for (int k = 0; k < N; ++k) phase[k] = out_b[k];
    for (int j = 0; j < N; ++j) {
        if (!s[j]) continue;
        for (int k = 0; k < N; ++k) {
            if (j + k < N) phase[j + k] -= out_a[k];
            else phase[j + k - N] += out_a[k];
        }
    }
    int bad = 0;
    printf("messages:");
    for (int r = 0; r < COUNT; ++r) {
        const unsigned got = (unsigned)((phase[r * STRIDE] + ((uint64_t)1 << (LOG_DELTA - 1))) >> LOG_DELTA);
        printf(" %u", got);
        if (got != bytes[r]) bad = 1;
    }
    printf("\n");
    /* everywhere else the phase is error only */
    uint64_t worst = 0;
    for (int k = 0; k < N; ++k) {
        if (k % STRIDE == 0) continue;
        const uint64_t mag = (int64_t)phase[k] < 0 ? (uint64_t)0 - phase[k] : phase[k];
        if (mag > worst) worst = mag;
    }
    if (worst >> (LOG_DELTA - 1)) bad = 1;
    if (bad) { fprintf(stderr, "wrong message or an error above the half-slot\n"); return 1; }
    printf("tfhe_pack_demo ok: %d TLWE ciphertexts of %d words packed into one TGLWE of %d words in one call\n", COUNT, N_IN + 1, 2 * N);
    fhe_tlwe_pack_key_destroy(key);
    fhe_rng_destroy(rng); fhe_torus_ctx_destroy(t);
    free(pfksk);
    return 0;
}
