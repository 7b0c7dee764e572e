/* Eight TLWE ciphertexts into one TGLWE ciphertext through automorphisms, from plain C: include/fhe_ring.h and libfhe_ring.so only.
 * The inputs are TLWE ciphertexts (pt = value << 48, scheme/tfhe/src/tlwe.rs:122-132) under the N bits of the TGLWE key s itself.
 * fhe_tglwe_atk_gen makes the log2 N = 8 automorphism keys g = 3, 5, ..., 257 (8 x 5 rows of N words: the packing key of fhe_tlwe_pack
 * for the same ring has 5 x 257 rows), fhe_tlwe_ring_pack merges the inputs pairwise over three levels and traces the rest away: value
 * r sits at coefficient r N / 8 of the result, multiplied by N, and every other coefficient holds error only.  The program decrypts
 * b - a s itself and rounds to the scale N 2^48.
 * Parameters: N = 256, gadget (7, 5), every noise 2^-50: N err_in + (N - 1) ks (include/fhe_ring.h) is about 2^44,
 * far below the half-slot 2^55.
 * build: gcc -std=c99 -O2 -I include examples/tfhe_trace_demo.c -L learn-fhe_amd/lib -lfhe_ring -Wl,-rpath,$PWD/learn-fhe_amd/lib \
 *            -Wl,--allow-shlib-undefined -lm -o tfhe_trace_demo */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "fhe_ring.h"

#define N 256
#define LOG_N 8
#define LOG_B 7
#define D 5
#define M 8
#define LOG_DELTA 48
#define SD 8.881784197001252e-16

#define CHECK(call)                                                                                  \
    do {                                                                                             \
        int rc_ = (call);                                                                            \
        if (rc_ != FHE_OK) { fprintf(stderr, "%s: %d (hip %d)\n", #call, rc_, fhe_last_hip_error()); return 1; } \
    } while (0)

int main(void) {
    fhe_torus_ctx *t = NULL;
    fhe_rng *rng = NULL;
    CHECK(fhe_torus_ctx_create(0, &t));
    CHECK(fhe_rng_create_from_seed(2030, &rng));
    static uint64_t s[N];
    CHECK(fhe_sample_binary(rng, 1, s, N, FHE_MEM_HOST, NULL));
    uint32_t gs[LOG_N];
    for (int u = 1; u <= LOG_N; ++u) gs[u - 1] = ((uint32_t)1 << u) + 1;
    static uint64_t atk_a[LOG_N * D * N], atk_b[LOG_N * D * N];
    CHECK(fhe_tglwe_atk_gen(t, LOG_B, D, s, N, gs, LOG_N, SD, rng, 2, atk_a, atk_b, FHE_MEM_HOST, NULL));
    fhe_tglwe_auto_key *key = NULL;
    CHECK(fhe_tglwe_atk_prepare(t, LOG_B, D, atk_a, atk_b, N, gs, LOG_N, FHE_MEM_HOST, NULL, &key));

    const int xs[M] = {3, -7, 0, 5, -1, 7, 2, -8};
    static uint64_t pt[M], ct_a[M * N], ct_b[M], out_a[N], out_b[N];
    for (int r = 0; r < M; ++r) pt[r] = (uint64_t)(int64_t)xs[r] << LOG_DELTA;
    CHECK(fhe_tlwe_sk_encrypt(s, pt, N, M, SD, rng, 3, ct_a, ct_b, FHE_MEM_HOST, NULL));
    CHECK(fhe_tlwe_ring_pack(t, key, ct_a, ct_b, M, 1, out_a, out_b, FHE_MEM_HOST, NULL));

    /* phase = b - a s in Z[X]/(X^N + 1), words mod 2^64 */
    static uint64_t phase[N];
    for (int i = 0; i < N; ++i) phase[i] = out_b[i];
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            if (!s[j]) continue;
            if (i + j < N) phase[i + j] -= out_a[i];
            else phase[i + j - N] += out_a[i];
        }
    const int shift = LOG_DELTA + LOG_N;
    int bad = 0;
    printf("coefficient : value");
    for (int i = 0; i < N; ++i) {
        const long got = (long)((int64_t)(phase[i] + ((uint64_t)1 << (shift - 1))) >> shift);
        const long want = i % (N / M) == 0 ? xs[i / (N / M)] : 0;
        if (got != want) ++bad;
        if (i % (N / M) == 0) printf("  %d : %ld", i, got);
    }
    printf("\n");
    if (bad) { fprintf(stderr, "%d coefficients decode wrongly\n", bad); return 1; }
    printf("tfhe_trace_demo ok: %d TLWE ciphertexts in one TGLWE ciphertext under %d key rows (the packing key switch needs %d)\n", M, LOG_N * D,
           D * (N + 1));
    fhe_tglwe_atk_destroy(key);
    fhe_rng_destroy(rng); fhe_torus_ctx_destroy(t);
    return 0;
}
