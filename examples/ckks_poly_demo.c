/* A degree-7 Chebyshev series on encrypted CKKS slots from plain C: include/fhe_ring.h and libfhe_ring.so only.  Keys
 * (scheme/ckks/src/ckks.rs:139-166), `Ckks::encode` and `pk_encrypt` (ckks.rs:186-198, 227-238), the plan of the series, the evaluator
 * over the caller's per-level contexts, ONE call of fhe_ckks_poly_apply on host buffers, decryption and decode (ckks.rs:200-213, 240-248).
 * build: gcc -std=c99 -O2 -I include examples/ckks_poly_demo.c -L learn-fhe_amd/lib -lfhe_ring -lm -Wl,-rpath,$PWD/learn-fhe_amd/lib \
 *            -Wl,--allow-shlib-undefined -o ckks_poly_demo */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "fhe_ring.h"

#define LOG_N 5
#define N (1 << LOG_N)
#define SLOTS (N / 2)
#define DEGREE 7
#define MAX_L 16
#define BATCH 2

#define CHECK(call)                                                                                  \
    do {                                                                                             \
        int rc_ = (call);                                                                            \
        if (rc_ != FHE_OK) { fprintf(stderr, "%s: %d (hip %d)\n", #call, rc_, fhe_last_hip_error()); return 1; } \
    } while (0)

/* sum_j c_j T_j(x) by Clenshaw's recurrence */
static double chebval(const double *c, int degree, double x) {
    double b1 = 0.0, b2 = 0.0;
    for (int j = degree; j >= 1; --j) { const double t = 2.0 * x * b1 - b2 + c[j]; b2 = b1; b1 = t; }
    return x * b1 - b2 + c[0];
}

int main(void) {
    /* a sigmoid-like odd series plus a constant: 1/2 + sum of odd terms */
    const double coeffs[DEGREE + 1] = {0.5, 0.59, 0.0, -0.12, 0.0, 0.04, 0.0, -0.01};
    fhe_ckks_poly_plan *plan = NULL;
    CHECK(fhe_ckks_poly_plan_create(coeffs, DEGREE, 0, &plan));
    int depth = 0, n_ops = 0, n_regs = 0;
    CHECK(fhe_ckks_poly_plan_info(plan, &depth, &n_ops, &n_regs));
    const int L = depth + 2;
    if (L > MAX_L) return 1;
    /* scheme/ckks/src/ckks.rs:20-35: the first L primes are qs, the next L are ps */
    uint64_t primes[2 * MAX_L];
    if (fhe_two_adic_primes(55, LOG_N + 1, 2 * L, primes) != 2 * L) return 1;
    const uint64_t scale = primes[L - 1];
    fhe_rns_ctx *levels[MAX_L];
    for (int s = 0; s <= depth; ++s) CHECK(fhe_rns_ctx_create(primes, L - s, primes + L, L, 0, &levels[s]));
    fhe_rng *rng = NULL;
    CHECK(fhe_rng_create_from_seed(7, &rng));
    static uint64_t sk[N], pk_b[MAX_L * N], pk_a[MAX_L * N], rlk_b[2 * MAX_L * N], rlk_a[2 * MAX_L * N];
    CHECK(fhe_sample_zo(0.5, rng, 1, sk, N, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_sk_encrypt(levels[0], 0, sk, NULL, N, 1, rng, 2, pk_b, pk_a, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_ksk_gen(levels[0], sk, NULL, N, rng, 3, rlk_b, rlk_a, FHE_MEM_HOST, NULL));
    fhe_ckks_poly_eval *eval = NULL;
    CHECK(fhe_ckks_poly_prepare(plan, (const fhe_rns_ctx *const *)levels, depth + 1, scale, rlk_b, rlk_a, N, FHE_MEM_HOST, &eval));
    /* slots in [-1, 1] */
    static double m[BATCH * SLOTS * 2], got[BATCH * SLOTS * 2];
    for (int i = 0; i < BATCH * SLOTS; ++i) { m[2 * i] = -1.0 + 2.0 * (double)i / (BATCH * SLOTS - 1); m[2 * i + 1] = 0.0; }
    fhe_ckks_encoder *enc = NULL;
    CHECK(fhe_ckks_encoder_create(N, 0, &enc));
    static uint64_t pt[BATCH * MAX_L * N], ct_b[BATCH * MAX_L * N], ct_a[BATCH * MAX_L * N], out_b[BATCH * MAX_L * N], out_a[BATCH * MAX_L * N];
    CHECK(fhe_ckks_encode(enc, levels[0], scale, m, NULL, BATCH, pt, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_pk_encrypt(levels[0], pk_b, pk_a, pt, N, BATCH, rng, 4, ct_b, ct_a, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_poly_apply(eval, ct_b, ct_a, out_b, out_a, BATCH, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_decrypt(levels[depth], sk, out_b, out_a, N, BATCH, pt, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_decode(enc, levels[depth], scale, pt, BATCH, got, NULL, FHE_MEM_HOST, NULL));
    double worst = 0.0;
    for (int i = 0; i < BATCH * SLOTS; ++i) {
        const double e = fabs(got[2 * i] - chebval(coeffs, DEGREE, m[2 * i]));
        if (e > worst) worst = e;
        if (fabs(got[2 * i + 1]) > worst) worst = fabs(got[2 * i + 1]);
    }
    printf("degree %d, depth %d, %d ops over %d registers, %d -> %d limbs: worst slot error %.3g\n", DEGREE, depth, n_ops, n_regs, L, L - depth, worst);
    fhe_ckks_poly_eval_destroy(eval);
    fhe_ckks_poly_plan_destroy(plan);
    fhe_ckks_encoder_destroy(enc);
    for (int s = 0; s <= depth; ++s) fhe_rns_ctx_destroy(levels[s]);
    if (!(worst < 1e-7)) { fprintf(stderr, "slot error too large\n"); return 1; }   /* 2^-23: far above the scheme's noise, far below a wrong term */
    printf("ckks_poly_demo ok\n");
    return 0;
}
