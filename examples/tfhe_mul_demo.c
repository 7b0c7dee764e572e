/* The inner product of two encrypted vectors from plain C: include/fhe_ring.h and libfhe_ring.so only.  The entries arrive as TLWE
 * ciphertexts (pt = value << 52, scheme/tfhe/src/tlwe.rs:122-132) under a key z of N_IN bits.  fhe_tlwe_pack puts x_r at coefficient r
 * of one TGLWE ciphertext and, from the inputs [y_0, 0, ..., 0, -y_{M-1}, ..., -y_1] (negated word by word; the zeros are all-zero
 * ciphertexts), -y_r at coefficient N - r of another.  ONE call of fhe_tglwe_mul multiplies the two as polynomials -- X^r X^(N - r) = -1
 * brings x_r y_r to coefficient 0 --, fhe_tglwe_sample_extract(0) takes that coefficient out as a TLWE ciphertext under the TGLWE key's
 * bits, and the program decrypts b - <a, s> itself and rounds to the scale.
 * Parameters: N = 256, N_IN = 16, packing gadget (8, 7), relinearisation gadget (7, 7), every noise 2^-55: the error terms of the product
 * (include/fhe_ring.h) stay far below the half-slot 2^51.
 * build: gcc -std=c99 -O2 -I include examples/tfhe_mul_demo.c -L learn-fhe_amd/lib -lfhe_ring -Wl,-rpath,$PWD/learn-fhe_amd/lib \
 *            -Wl,--allow-shlib-undefined -lm -o tfhe_mul_demo */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "fhe_ring.h"

#define N 256
#define N_IN 16
#define PF_LOG_B 8
#define PF_D 7
#define RL_LOG_B 7
#define RL_D 7
#define M 8
#define LOG_DELTA 52
#define SD 2.7755575615628914e-17

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
    /* z: the TLWE key, s: the TGLWE key, both binary */
    static uint64_t z[N_IN], s[N], funcs[N];
    CHECK(fhe_sample_binary(rng, 1, z, N_IN, FHE_MEM_HOST, NULL));
    CHECK(fhe_sample_binary(rng, 2, s, N, FHE_MEM_HOST, NULL));
    funcs[0] = 1;
    uint64_t *pfksk = malloc((size_t)PF_D * (N_IN + 1) * 2 * N * 8);
    if (!pfksk) return 1;
    CHECK(fhe_tlwe_pfksk_gen(t, PF_LOG_B, PF_D, z, N_IN, s, N, funcs, 1, SD, rng, 3, pfksk, FHE_MEM_HOST, NULL));
    fhe_tlwe_pack_key *pack_key = NULL;
    CHECK(fhe_tlwe_pack_key_prepare(t, PF_LOG_B, PF_D, pfksk, N_IN, N, FHE_MEM_HOST, NULL, &pack_key));
    static uint64_t rlk_a[RL_D * N], rlk_b[RL_D * N];
    CHECK(fhe_tglwe_rlk_gen(t, RL_LOG_B, RL_D, s, N, SD, rng, 4, rlk_a, rlk_b, FHE_MEM_HOST, NULL));
    fhe_tglwe_relin_key *relin_key = NULL;
    CHECK(fhe_tglwe_rlk_prepare(t, RL_LOG_B, RL_D, rlk_a, rlk_b, N, FHE_MEM_HOST, NULL, &relin_key));

    const int xs[M] = {3, -7, 0, 5, -1, 7, 2, -4}, ys[M] = {-6, 2, 7, 4, -3, 1, -7, 5};
    long want = 0;
    for (int r = 0; r < M; ++r) want += (long)xs[r] * ys[r];
    static uint64_t mx[M], my[M], xa[M * N_IN], xb[M], ya[M * N_IN], yb[M];
    for (int r = 0; r < M; ++r) { mx[r] = (uint64_t)(int64_t)xs[r] << LOG_DELTA; my[r] = (uint64_t)(int64_t)ys[r] << LOG_DELTA; }
    CHECK(fhe_tlwe_sk_encrypt(z, mx, N_IN, M, SD, rng, 5, xa, xb, FHE_MEM_HOST, NULL));
    CHECK(fhe_tlwe_sk_encrypt(z, my, N_IN, M, SD, rng, 6, ya, yb, FHE_MEM_HOST, NULL));

    /* position 0: y_0; position N - r: -y_r; everything between: the all-zero ciphertext */
    static uint64_t ra[N * N_IN], rb[N];
    for (int i = 0; i < N_IN; ++i) ra[i] = ya[i];
    rb[0] = yb[0];
    for (int r = 1; r < M; ++r) {
        for (int i = 0; i < N_IN; ++i) ra[(size_t)(N - r) * N_IN + i] = (uint64_t)0 - ya[r * N_IN + i];
        rb[N - r] = (uint64_t)0 - yb[r];
    }
    static uint64_t px_a[N], px_b[N], py_a[N], py_b[N], prod_a[N], prod_b[N], out_a[N], out_b[1];
    CHECK(fhe_tlwe_pack(t, pack_key, xa, xb, M, 1, 1, px_a, px_b, FHE_MEM_HOST, NULL));
    CHECK(fhe_tlwe_pack(t, pack_key, ra, rb, N, 1, 1, py_a, py_b, FHE_MEM_HOST, NULL));
    CHECK(fhe_tglwe_mul(t, relin_key, px_a, px_b, py_a, py_b, LOG_DELTA, prod_a, prod_b, 1, FHE_MEM_HOST, NULL));
    CHECK(fhe_tglwe_sample_extract(prod_a, prod_b, N, 0, out_a, out_b, 1, FHE_MEM_HOST, NULL));

    uint64_t phase = out_b[0];
    for (int i = 0; i < N; ++i)
        if (s[i]) phase -= out_a[i];
    const long got = (long)((int64_t)(phase + ((uint64_t)1 << (LOG_DELTA - 1))) >> LOG_DELTA);
    const int64_t err = (int64_t)(phase - ((uint64_t)(int64_t)want << LOG_DELTA));
    printf("inner product: %ld (plain: %ld), phase error 2^%.1f of a half-slot 2^%d\n", got, want,
           err ? __builtin_log2((double)(err < 0 ? -err : err)) : 0.0, LOG_DELTA - 1);
    if (got != want) { fprintf(stderr, "wrong inner product\n"); return 1; }
    printf("tfhe_mul_demo ok: %d products and their sum in one ciphertext product, no bootstrap\n", M);
    fhe_tglwe_rlk_destroy(relin_key);
    fhe_tlwe_pack_key_destroy(pack_key);
    fhe_rng_destroy(rng); fhe_torus_ctx_destroy(t);
    free(pfksk);
    return 0;
}
