/* `FhewU8::wrapping_add` (scheme/fhew/src/fhew/uint8.rs:65-90) from plain C: include/fhe_ring.h and libfhe_ring.so only.  The keys of
 * scheme/fhew/src/bootstrapping.rs:122-146 `key_gen` at the reference's `single_key_testing_param` (fhew/boolean.rs:225-239), two
 * bytes encrypted bit by bit (uint8.rs:17-20), the ripple adder of boolean.rs:139-150 written down as a gate netlist, ONE call of
 * fhe_fhew_circuit_run on host buffers for BATCH pairs of bytes, decryption (lwe.rs:141-149).
 * build: gcc -std=c99 -O2 -I include examples/fhew_circuit_demo.c -L learn-fhe_amd/lib -lfhe_ring -Wl,-rpath,$PWD/learn-fhe_amd/lib \
 *            -Wl,--allow-shlib-undefined -o fhew_circuit_demo */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "fhe_ring.h"

#define LOG_N 9
#define N (1 << LOG_N)
#define LOG_B 7
#define D 4
#define N_LWE 100
#define Q_KS (1u << 16)
#define KS_LOG_B 4
#define KS_D 4
#define W 10
#define BATCH 3

#define CHECK(call)                                                                                  \
    do {                                                                                             \
        int rc_ = (call);                                                                            \
        if (rc_ != FHE_OK) { fprintf(stderr, "%s: %d (hip %d)\n", #call, rc_, fhe_last_hip_error()); return 1; } \
    } while (0)

static uint64_t to_zq(int64_t v, uint64_t q) { return v < 0 ? q - (uint64_t)(-v) % q : (uint64_t)v % q; }
static uint64_t round_div(uint64_t q, double k) { const double x = (double)q / k; return (uint64_t)(x + 0.5) % q; }

static fhe_fhew_gate gate(int op, uint32_t a, uint32_t b) {
    fhe_fhew_gate g = {0, {0, 0, 0}, {0, 0, 0}};
    g.op = (uint8_t)op; g.in[0] = a; g.in[1] = b;
    return g;
}

int main(void) {
    uint64_t q = 0;
    if (fhe_two_adic_primes(28, LOG_N + 1, 1, &q) != 1) return 1;
    fhe_ctx *ctx = NULL;
    fhe_rng *rng = NULL;
    CHECK(fhe_ctx_create(q, 0, &ctx));
    CHECK(fhe_rng_create_from_seed(2024, &rng));
    /* secret keys: the ring key z and the LWE key s, dg(3.2, 6) (rlwe.rs:94-96, lwe.rs:103-106) */
    static uint64_t z_i[N], s_i[N_LWE], z_q[N], z_ks[N], s_ks[N_LWE];
    CHECK(fhe_sample_dg(0, 3.2, 6, rng, 1, z_i, N, FHE_MEM_HOST, NULL));
    CHECK(fhe_sample_dg(0, 3.2, 6, rng, 2, s_i, N_LWE, FHE_MEM_HOST, NULL));
    for (int i = 0; i < N; ++i) { z_q[i] = to_zq((int64_t)z_i[i], q); z_ks[i] = to_zq((int64_t)z_i[i], Q_KS); }
    for (int i = 0; i < N_LWE; ++i) s_ks[i] = to_zq((int64_t)s_i[i], Q_KS);
    /* brk_j = RGSW(X^(s_j)) (bootstrapping.rs:131-136), ak = automorphism keys for [-g, g, .., g^w] (86-89), LWE key-switching key z -> s */
    uint64_t *mono = calloc((size_t)N_LWE * N, 8), *ra = malloc((size_t)N_LWE * 2 * D * N * 8), *rb = malloc((size_t)N_LWE * 2 * D * N * 8);
    uint64_t *aa = malloc((size_t)(W + 1) * D * N * 8), *ab = malloc((size_t)(W + 1) * D * N * 8);
    uint64_t *ksa = malloc((size_t)N * KS_D * N_LWE * 8), *ksb = malloc((size_t)N * KS_D * 8);
    if (!mono || !ra || !rb || !aa || !ab || !ksa || !ksb) return 1;
    for (int j = 0; j < N_LWE; ++j) {
        const int64_t e = (((int64_t)s_i[j] % (2 * N)) + 2 * N) % (2 * N);
        mono[(size_t)j * N + e % N] = e < N ? 1 : q - 1;
    }
    CHECK(fhe_rgsw_encrypt(ctx, LOG_B, D, z_q, mono, N, N_LWE, rng, 3, ra, rb, FHE_MEM_HOST, NULL));
    int64_t ak_t[W + 1];
    {
        int64_t x = 1;
        ak_t[0] = -5;
        for (int i = 1; i <= W; ++i) { x = x * 5 % (2 * N); ak_t[i] = x >= N ? x - 2 * N : x; }
    }
    for (int i = 0; i <= W; ++i)
        CHECK(fhe_rlwe_ksk_gen(ctx, LOG_B, D, z_q, NULL, ak_t[i], N, rng, 100 + i, aa + (size_t)i * D * N, ab + (size_t)i * D * N, FHE_MEM_HOST, NULL));
    CHECK(fhe_lwe_ksk_gen(Q_KS, KS_LOG_B, KS_D, s_ks, N_LWE, z_ks, N, rng, 4, ksa, ksb, FHE_MEM_HOST, NULL));
    fhe_key *brk = NULL, *ak = NULL;
    fhe_bootstrap_key *bk = NULL;
    CHECK(fhe_rgsw_prepare(ctx, LOG_B, D, ra, rb, N, N_LWE, FHE_MEM_HOST, &brk));
    CHECK(fhe_ksk_prepare(ctx, LOG_B, D, aa, ab, N, W + 1, FHE_MEM_HOST, &ak));
    CHECK(fhe_bootstrap_key_create(ctx, brk, ak, ak_t, W, &bk));

    /* the netlist: inputs x_0 .. x_7, y_0 .. y_7 (wires 0 .. 15), then uint8.rs:65-76 gate for gate; the last carry is left out */
    fhe_fhew_gate gates[37];
    uint32_t sum[8], carry = 0;
    size_t ng = 0;
#define EMIT(op, a, b) (gates[ng] = gate(op, a, b), (uint32_t)(16 + ng++))
    for (uint32_t i = 0; i < 8; ++i) {
        const uint32_t t = EMIT(FHE_GATE_XOR, i, 8 + i);
        if (i == 0) { sum[0] = t; carry = EMIT(FHE_GATE_AND, i, 8 + i); continue; }
        sum[i] = EMIT(FHE_GATE_XOR, t, carry);
        const uint32_t g0 = EMIT(FHE_GATE_AND, i, 8 + i), g1 = EMIT(FHE_GATE_AND, t, carry);
        carry = EMIT(FHE_GATE_OR, g0, g1);
    }
    fhe_fhew_circuit *circuit = NULL;
    size_t levels = 0, live = 0, width = 0;
    CHECK(fhe_fhew_circuit_create(gates, ng, 16, sum, 8, &circuit));
    CHECK(fhe_fhew_circuit_info(circuit, &levels, &live, &width));
    if (ng != 37 || live != 34 || levels != 14) { fprintf(stderr, "netlist: %zu gates, %zu live, %zu levels\n", ng, live, levels); return 1; }

    /* encrypt: bit i of byte k of x in slot [i][k], of y in slot [8 + i][k] (lwe.rs:128-139 with m * Q/4) */
    const uint8_t xs[BATCH] = {255, 255, 100}, ys[BATCH] = {1, 255, 57};
    const uint64_t q4 = round_div(q, 4.0);
    static uint64_t pt[16 * BATCH], in_a[16 * BATCH * N], in_b[16 * BATCH], out_a[8 * BATCH * N], out_b[8 * BATCH];
    for (int i = 0; i < 8; ++i)
        for (int k = 0; k < BATCH; ++k) {
            pt[i * BATCH + k] = ((xs[k] >> i) & 1) ? q4 : 0;
            pt[(8 + i) * BATCH + k] = ((ys[k] >> i) & 1) ? q4 : 0;
        }
    CHECK(fhe_lwe_sk_encrypt(q, z_q, pt, N, 16 * BATCH, rng, 5, in_a, in_b, FHE_MEM_HOST, NULL));
    CHECK(fhe_fhew_circuit_run(circuit, bk, Q_KS, KS_LOG_B, KS_D, ksa, ksb, in_a, in_b, out_a, out_b, BATCH, FHE_MEM_HOST, NULL));

    /* decrypt: b - <a, z> is m * Q/4 + noise */
    int bad = 0;
    for (int k = 0; k < BATCH; ++k) {
        unsigned got = 0;
        for (int i = 0; i < 8; ++i) {
            const uint64_t *a = out_a + ((size_t)i * BATCH + k) * N;
            uint64_t dot = 0;
            for (int j = 0; j < N; ++j) dot = (dot + (uint64_t)((unsigned __int128)a[j] * z_q[j] % q)) % q;
            const uint64_t phase = (out_b[i * BATCH + k] + q - dot) % q;
            const unsigned m = (unsigned)((double)phase / ((double)q / 4.0) + 0.5) % 4;
            if (m > 1) bad = 1;
            got |= (m & 1u) << i;
        }
        printf("%u + %u = %u (mod 256)\n", xs[k], ys[k], got);
        if (got != ((unsigned)xs[k] + ys[k]) % 256u) bad = 1;
    }
    if (bad) { fprintf(stderr, "wrong sum\n"); return 1; }
    printf("fhew_circuit_demo ok: %zu gates in %zu levels (widest %zu), one call for %d pairs of bytes\n", live, levels, width, BATCH);
    fhe_fhew_circuit_destroy(circuit);
    fhe_bootstrap_key_destroy(bk);
    fhe_key_destroy(brk); fhe_key_destroy(ak);
    fhe_rng_destroy(rng); fhe_ctx_destroy(ctx);
    free(mono); free(ra); free(rb); free(aa); free(ab); free(ksa); free(ksb);
    return 0;
}
