/* A three-diagonal matrix times encrypted CKKS slots through the double-hoisted product, from plain C: include/fhe_ring.h and
 * libfhe_ring.so only.  Keys (scheme/ckks/src/ckks.rs:139-184), `Ckks::encode` of the message over qs and of the diagonals over
 * qs ++ ps (the lifted plaintexts fhe_ckks_diag_matrix_prepare_hoisted takes: the same integers reduced modulo every prime, which a
 * context whose qs are qs ++ ps encodes), ONE call of fhe_ckks_mul_mat_hoisted on host buffers, decryption and decode.
 * build: gcc -std=c99 -O2 -I include examples/ckks_hoist_demo.c -L learn-fhe_amd/lib -lfhe_ring -lm -Wl,-rpath,$PWD/learn-fhe_amd/lib \
 *            -Wl,--allow-shlib-undefined -o ckks_hoist_demo */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "fhe_ring.h"

#define LOG_N 5
#define N (1 << LOG_N)
#define SLOTS (N / 2)
#define L 4
#define K 4
#define TERMS 3

#define CHECK(call)                                                                                  \
    do {                                                                                             \
        int rc_ = (call);                                                                            \
        if (rc_ != FHE_OK) { fprintf(stderr, "%s: %d (hip %d)\n", #call, rc_, fhe_last_hip_error()); return 1; } \
    } while (0)

int main(void) {
    /* ckks.rs:20-35: the first L primes are qs, the next K are ps; one more serves as the (unused) special base of the encoding context */
    uint64_t primes[L + K + 1];
    if (fhe_two_adic_primes(55, LOG_N + 1, L + K + 1, primes) != L + K + 1) return 1;
    const uint64_t scale = primes[L - 1];
    fhe_rns_ctx *hi = NULL, *lo = NULL, *wide = NULL;
    CHECK(fhe_rns_ctx_create(primes, L, primes + L, K, 0, &hi));
    CHECK(fhe_rns_ctx_create(primes, L - 1, primes + L, K, 0, &lo));
    CHECK(fhe_rns_ctx_create(primes, L + K, primes + L + K, 1, 0, &wide));
    fhe_rng *rng = NULL;
    CHECK(fhe_rng_create_from_seed(11, &rng));
    static uint64_t sk[N], pk_b[L * N], pk_a[L * N], kb[(L + K) * N], ka[(L + K) * N];
    CHECK(fhe_sample_zo(0.5, rng, 1, sk, N, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_sk_encrypt(hi, 0, sk, NULL, N, 1, rng, 2, pk_b, pk_a, FHE_MEM_HOST, NULL));
    /* the diagonals 0, 1 and 4 split into the giant steps {0, 4} and the baby steps {0, 1}: terms (0, 0), (0, 1), (4, 0) */
    const uint32_t giant[2] = {0, 4}, baby[2] = {0, 1};
    const uint8_t present[4] = {1, 1, 1, 0};
    const int term_i[TERMS] = {0, 0, 4}, term_j[TERMS] = {0, 1, 0};
    fhe_ckks_key *baby_keys[2] = {NULL, NULL}, *giant_keys[2] = {NULL, NULL};
    CHECK(fhe_ckks_rtk_gen(hi, sk, N, 1, rng, 3, kb, ka, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_ksk_prepare(hi, kb, ka, N, FHE_MEM_HOST, &baby_keys[1]));
    CHECK(fhe_ckks_rtk_gen(lo, sk, N, 4, rng, 4, kb, ka, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_ksk_prepare(lo, kb, ka, N, FHE_MEM_HOST, &giant_keys[1]));
    /* the matrix: dense[c][(c + d) mod SLOTS] = diag_d[c]; term (i, j) carries diag_{i + j} rotated by -i (bootstrapping.rs:101) */
    static double diag[TERMS][SLOTS * 2], rot[SLOTS * 2], m[SLOTS * 2], want[SLOTS * 2], got[SLOTS * 2];
    for (int t = 0; t < TERMS; ++t)
        for (int c = 0; c < SLOTS; ++c) {
            diag[t][2 * c] = cos(0.3 * c + t) * 0.5;
            diag[t][2 * c + 1] = sin(0.7 * c - t) * 0.5;
        }
    for (int c = 0; c < SLOTS; ++c) { m[2 * c] = (double)c / SLOTS; m[2 * c + 1] = 1.0 - (double)c / SLOTS; want[2 * c] = want[2 * c + 1] = 0.0; }
    for (int t = 0; t < TERMS; ++t)
        for (int c = 0; c < SLOTS; ++c) {
            const int s = (c + term_i[t] + term_j[t]) % SLOTS;
            want[2 * c] += diag[t][2 * c] * m[2 * s] - diag[t][2 * c + 1] * m[2 * s + 1];
            want[2 * c + 1] += diag[t][2 * c] * m[2 * s + 1] + diag[t][2 * c + 1] * m[2 * s];
        }
    fhe_ckks_encoder *enc = NULL;
    CHECK(fhe_ckks_encoder_create(N, 0, &enc));
    static uint64_t diags[TERMS * (L + K) * N], pt[L * N], ct_b[L * N], ct_a[L * N], out_b[L * N], out_a[L * N];
    for (int t = 0; t < TERMS; ++t) {
        for (int c = 0; c < SLOTS; ++c) {
            const int s = (c - term_i[t] + SLOTS) % SLOTS;
            rot[2 * c] = diag[t][2 * s];
            rot[2 * c + 1] = diag[t][2 * s + 1];
        }
        CHECK(fhe_ckks_encode(enc, wide, scale, rot, NULL, 1, diags + (size_t)t * (L + K) * N, FHE_MEM_HOST, NULL));
    }
    fhe_ckks_diag_matrix_hoisted *mat = NULL;
    CHECK(fhe_ckks_diag_matrix_prepare_hoisted(hi, lo, N, giant, 2, baby, 2, present, diags, (const fhe_ckks_key *const *)baby_keys,
                                               (const fhe_ckks_key *const *)giant_keys, FHE_MEM_HOST, &mat));
    CHECK(fhe_ckks_encode(enc, hi, scale, m, NULL, 1, pt, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_pk_encrypt(hi, pk_b, pk_a, pt, N, 1, rng, 5, ct_b, ct_a, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_mul_mat_hoisted(mat, ct_b, ct_a, out_b, out_a, 1, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_decrypt(lo, sk, out_b, out_a, N, 1, pt, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_decode(enc, lo, scale, pt, 1, got, NULL, FHE_MEM_HOST, NULL));  /* scale^2 / q_last = scale */
    double worst = 0.0;
    for (int c = 0; c < 2 * SLOTS; ++c)
        if (fabs(got[c] - want[c]) > worst) worst = fabs(got[c] - want[c]);
    printf("three diagonals, %d slots, %d + %d primes: worst slot error %.3g\n", SLOTS, L, K, worst);
    fhe_ckks_diag_matrix_hoisted_destroy(mat);
    fhe_ckks_key_destroy(baby_keys[1]);
    fhe_ckks_key_destroy(giant_keys[1]);
    fhe_ckks_encoder_destroy(enc);
    fhe_rns_ctx_destroy(wide);
    fhe_rns_ctx_destroy(lo);
    fhe_rns_ctx_destroy(hi);
    if (!(worst < 1e-7)) { fprintf(stderr, "slot error too large\n"); return 1; }   /* 2^-23: far above the scheme's noise, far below a wrong term */
    printf("ckks_hoist_demo ok\n");
    return 0;
}
