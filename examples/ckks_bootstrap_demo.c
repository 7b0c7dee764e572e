/* A CKKS bootstrap from plain C at n = 32: include/fhe_ring.h and libfhe_ring.so only.  Contexts for every level, the encoder, the two
 * linear plans (`coeff_to_slot`, `slot_to_coeff`: scheme/ckks/src/bootstrapping.rs:23-31) with their rotation keys, the eval_mod plan
 * with the bootstrap's factors, the relinearisation and conjugation keys (scheme/ckks/src/ckks.rs:163-172), the three prepared stages
 * bound by fhe_ckks_bootstrap_prepare; then `Ckks::encode`, `pk_encrypt` on ONE limb (a ciphertext at the bottom of its chain), ONE
 * call of fhe_ckks_bootstrap_apply on host buffers, decryption and decode on the refreshed limbs.
 * build: gcc -std=c99 -O2 -I include examples/ckks_bootstrap_demo.c -L learn-fhe_amd/lib -lfhe_ring -lm -Wl,-rpath,$PWD/learn-fhe_amd/lib \
 *            -Wl,--allow-shlib-undefined -o ckks_bootstrap_demo */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fhe_ring.h"

#define LOG_N 5
#define N (1 << LOG_N)
#define SLOTS (N / 2)
#define MAX_L 20
#define MAX_ROT 32
#define BATCH 2
#define K_MOD 8
#define R_MOD 3
#define DEGREE 31
#define WEIGHT 12 /* |t| <= (WEIGHT + 1) / 2 q0 = 6.5 q0 < K_MOD q0 */

#define CHECK(call)                                                                                  \
    do {                                                                                             \
        int rc_ = (call);                                                                            \
        if (rc_ != FHE_OK) { fprintf(stderr, "%s: %d (hip %d)\n", #call, rc_, fhe_last_hip_error()); return 1; } \
    } while (0)

/* a key [full + K][N] over qs[0 .. full) ++ ps -> the rows over qs[0 .. lv) ++ ps */
static void cut_key(const uint64_t *key, int full, int lv, int k, uint64_t *out) {
    memcpy(out, key, (size_t)lv * N * sizeof(uint64_t));
    memcpy(out + (size_t)lv * N, key + (size_t)full * N, (size_t)k * N * sizeof(uint64_t));
}

static uint64_t rot_b[MAX_ROT][2 * MAX_L * N], rot_a[MAX_ROT][2 * MAX_L * N], cut_b[MAX_ROT][2 * MAX_L * N], cut_a[MAX_ROT][2 * MAX_L * N];

int main(void) {
    fhe_ckks_encoder *enc = NULL;
    CHECK(fhe_ckks_encoder_create(N, 0, &enc));
    fhe_ckks_linear_plan *p_c2s = NULL, *p_s2c = NULL;
    CHECK(fhe_ckks_linear_plan_create(enc, 2, 1, &p_c2s));
    CHECK(fhe_ckks_linear_plan_create(enc, 2, 0, &p_s2c));
    int d_c2s = 0, d_s2c = 0, n_c2s = 0, n_s2c = 0, d_mod = 0;
    CHECK(fhe_ckks_linear_plan_info(p_c2s, &d_c2s, &n_c2s));
    CHECK(fhe_ckks_linear_plan_info(p_s2c, &d_s2c, &n_s2c));
    /* the depth of the eval_mod plan does not depend on its factors */
    fhe_ckks_poly_plan *probe = NULL, *plan = NULL;
    CHECK(fhe_ckks_eval_mod_plan_create(K_MOD, R_MOD, DEGREE, 1.0, 1.0, &probe));
    CHECK(fhe_ckks_poly_plan_info(probe, &d_mod, NULL, NULL));
    fhe_ckks_poly_plan_destroy(probe);
    const int depth = d_c2s + d_mod + d_s2c, L = depth + 2, L1 = L - d_c2s, L2 = L1 - d_mod;
    if (L > MAX_L || n_c2s > MAX_ROT || n_s2c > MAX_ROT) return 1;
    /* scheme/ckks/src/ckks.rs:20-35: the first L primes are qs, the next L are ps */
    uint64_t primes[2 * MAX_L];
    if (fhe_two_adic_primes(55, LOG_N + 1, 2 * L, primes) != 2 * L) return 1;
    const uint64_t q0 = primes[0], scale = primes[L - 1];
    CHECK(fhe_ckks_eval_mod_plan_create(K_MOD, R_MOD, DEGREE, (double)scale / (2.0 * (double)q0), (double)q0 / (double)scale, &plan));
    fhe_rns_ctx *levels[MAX_L];
    for (int s = 0; s <= depth; ++s) CHECK(fhe_rns_ctx_create(primes, L - s, primes + L, L, 0, &levels[s]));
    fhe_rns_ctx *bottom = NULL; /* the one-limb context the input lives on */
    CHECK(fhe_rns_ctx_create(primes, 1, primes + L, L, 0, &bottom));
    fhe_rng *rng = NULL;
    CHECK(fhe_rng_create_from_seed(11, &rng));
    /* a ternary secret of Hamming weight exactly WEIGHT (two's-complement i64) */
    static uint64_t sk[N];
    uint64_t state = 0x9E3779B97F4A7C15ull;
    for (int placed = 0; placed < WEIGHT;) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        const int pos = (int)(state >> 59);
        if (sk[pos]) continue;
        sk[pos] = (state >> 40) & 1 ? 1 : (uint64_t)-1;
        ++placed;
    }
    /* keys over the full chain: rotations of both plans, relinearisation, conjugation */
    static uint64_t rlk_b[2 * MAX_L * N], rlk_a[2 * MAX_L * N], cjk_b[2 * MAX_L * N], cjk_a[2 * MAX_L * N], tmp_b[2 * MAX_L * N], tmp_a[2 * MAX_L * N];
    uint32_t r_c2s[MAX_ROT], r_s2c[MAX_ROT];
    const uint64_t *kb[MAX_ROT], *ka[MAX_ROT];
    CHECK(fhe_ckks_linear_plan_rotations(p_c2s, r_c2s, n_c2s));
    CHECK(fhe_ckks_linear_plan_rotations(p_s2c, r_s2c, n_s2c));
    fhe_ckks_linear_transform *c2s = NULL, *s2c = NULL;
    for (int i = 0; i < n_c2s; ++i) {
        CHECK(fhe_ckks_rtk_gen(levels[0], sk, N, r_c2s[i], rng, 100 + r_c2s[i], rot_b[i], rot_a[i], FHE_MEM_HOST, NULL));
        kb[i] = rot_b[i]; ka[i] = rot_a[i];
    }
    CHECK(fhe_ckks_linear_transform_prepare(p_c2s, (const fhe_rns_ctx *const *)levels, d_c2s + 1, scale, r_c2s, kb, ka, n_c2s, FHE_MEM_HOST, &c2s));
    for (int i = 0; i < n_s2c; ++i) { /* generated over the full chain, cut down to the level slot_to_coeff starts on */
        CHECK(fhe_ckks_rtk_gen(levels[0], sk, N, r_s2c[i], rng, 200 + r_s2c[i], rot_b[i], rot_a[i], FHE_MEM_HOST, NULL));
        cut_key(rot_b[i], L, L2, L, cut_b[i]); cut_key(rot_a[i], L, L2, L, cut_a[i]);
        kb[i] = cut_b[i]; ka[i] = cut_a[i];
    }
    CHECK(fhe_ckks_linear_transform_prepare(p_s2c, (const fhe_rns_ctx *const *)(levels + d_c2s + d_mod), d_s2c + 1, scale, r_s2c, kb, ka, n_s2c, FHE_MEM_HOST,
                                            &s2c));
    CHECK(fhe_ckks_ksk_gen(levels[0], sk, NULL, N, rng, 3, rlk_b, rlk_a, FHE_MEM_HOST, NULL));
    cut_key(rlk_b, L, L1, L, tmp_b); cut_key(rlk_a, L, L1, L, tmp_a);
    fhe_ckks_poly_eval *eval = NULL;
    CHECK(fhe_ckks_poly_prepare(plan, (const fhe_rns_ctx *const *)(levels + d_c2s), d_mod + 1, scale, tmp_b, tmp_a, N, FHE_MEM_HOST, &eval));
    CHECK(fhe_ckks_cjk_gen(levels[0], sk, N, rng, 4, cjk_b, cjk_a, FHE_MEM_HOST, NULL));
    fhe_ckks_bootstrap *bs = NULL;
    CHECK(fhe_ckks_bootstrap_prepare((const fhe_rns_ctx *const *)levels, depth + 1, N, c2s, eval, s2c, cjk_b, cjk_a, FHE_MEM_HOST, &bs));
    int got_depth = 0, out_limbs = 0;
    CHECK(fhe_ckks_bootstrap_info(bs, &got_depth, &out_limbs));
    if (got_depth != depth || out_limbs != L - depth) return 1;
    /* small slots: |Re|, |Im| <= 2^-11, so every encoded coefficient is below 2^-10 q0 */
    static double m[BATCH * SLOTS * 2], got[BATCH * SLOTS * 2];
    for (int i = 0; i < BATCH * SLOTS * 2; ++i) m[i] = ldexp(-1.0 + 2.0 * (double)((i * 7) % 31) / 30.0, -11);
    static uint64_t pt[BATCH * MAX_L * N], pk_b[N], pk_a[N], ct_b[BATCH * N], ct_a[BATCH * N], out_b[BATCH * MAX_L * N], out_a[BATCH * MAX_L * N];
    CHECK(fhe_ckks_sk_encrypt(bottom, 0, sk, NULL, N, 1, rng, 5, pk_b, pk_a, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_encode(enc, bottom, scale, m, NULL, BATCH, pt, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_pk_encrypt(bottom, pk_b, pk_a, pt, N, BATCH, rng, 6, ct_b, ct_a, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_bootstrap_apply(bs, ct_b, ct_a, 1, out_b, out_a, BATCH, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_decrypt(levels[depth], sk, out_b, out_a, N, BATCH, pt, FHE_MEM_HOST, NULL));
    CHECK(fhe_ckks_decode(enc, levels[depth], scale, pt, BATCH, got, NULL, FHE_MEM_HOST, NULL));
    double worst = 0.0;
    for (int i = 0; i < BATCH * SLOTS * 2; ++i)
        if (fabs(got[i] - m[i]) > worst) worst = fabs(got[i] - m[i]);
    /* the bound of the decode-level test (tests/test_ckks_bootstrap_gpu.py): l (E_mod + K 2^-30) + 2^-30 with E_mod = 2^-30 * 4^r * sum |c_j|,
     * the series' coefficients summing to less than 4 (|cos| <= 1: c_0 <= 1 and the rest decay like Bessel functions of 2 pi K / 2^r), plus the
     * sine's cubic term l (2 pi)^2 2^-30 / 6 */
    const double two30 = ldexp(1.0, -30);
    const double bound = SLOTS * (two30 * 64.0 * 4.0 + K_MOD * two30) + two30 + SLOTS * 39.4784176 * two30 / 6.0 + 1e-9;
    printf("n = %d, %d -> %d limbs through depth %d (%d + %d + %d): worst slot error %.3g (bound %.3g)\n", N, L, out_limbs, depth, d_c2s, d_mod, d_s2c, worst, bound);
    fhe_ckks_bootstrap_destroy(bs);
    fhe_ckks_poly_eval_destroy(eval);
    fhe_ckks_linear_transform_destroy(c2s);
    fhe_ckks_linear_transform_destroy(s2c);
    fhe_ckks_poly_plan_destroy(plan);
    fhe_ckks_linear_plan_destroy(p_c2s);
    fhe_ckks_linear_plan_destroy(p_s2c);
    fhe_ckks_encoder_destroy(enc);
    fhe_rng_destroy(rng);
    fhe_rns_ctx_destroy(bottom);
    for (int s = 0; s <= depth; ++s) fhe_rns_ctx_destroy(levels[s]);
    if (!(worst <= bound)) { fprintf(stderr, "slot error too large\n"); return 1; }
    printf("ckks_bootstrap_demo ok\n");
    return 0;
}
