/* Two encrypted bytes added from plain C with ONE blind rotation per block: include/fhe_ring.h and libfhe_ring.so only.  The radix
 * arithmetic of examples/tfhe_circuit_demo.c (scheme/tfhe/src/bootstrapping.rs:118-165: log_p = 4 message bits under one padding bit; a
 * byte is 4 blocks of 2 message bits with 2 bits of carry room) through many-LUT nodes: per block ONE node whose interleaved table
 * serves the message function and the carry function of x_i + y_i + carry_{i-1} -- 4 blind rotations where the two-table netlist
 * spends 7.  The sum is mod-switched to even positions, so the drift doubles: at most 2 (N_LWE + 1) / 2 = 13 of 2 N = 2048 positions
 * against a half-slot of N / 2 P = 32.  Keys as `Bootstrapping::key_gen` makes them (bootstrapping.rs:59-76), from the device key
 * generators; ONE call of fhe_tfhe_circuit_run on host buffers for BATCH pairs of bytes; decryption (tlwe.rs:134-142).
 * build: gcc -std=c99 -O2 -I include examples/tfhe_many_demo.c -L learn-fhe_amd/lib -lfhe_ring -Wl,-rpath,$PWD/learn-fhe_amd/lib \
 *            -Wl,--allow-shlib-undefined -o tfhe_many_demo */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "fhe_ring.h"

#define N 1024
#define N_LWE 12
#define LOG_B 7
#define D 3
#define KS_LOG_B 4
#define KS_D 5
#define LOG_P 4
#define PADDING 1
#define LOG_DELTA (64 - LOG_P - PADDING)
#define P (1 << LOG_P)
#define BLOCKS 4
#define MSG_BITS 2
#define BATCH 3
#define SD_LWE 1.339775301998614e-7
#define SD_GLWE 2.845267479601915e-15

#define CHECK(call)                                                                                  \
    do {                                                                                             \
        int rc_ = (call);                                                                            \
        if (rc_ != FHE_OK) { fprintf(stderr, "%s: %d (hip %d)\n", #call, rc_, fhe_last_hip_error()); return 1; } \
    } while (0)

static unsigned f_msg(unsigned v) { return v & ((1u << MSG_BITS) - 1); }
static unsigned f_carry(unsigned v) { return v >> MSG_BITS; }

/* coefficient c of bootstrapping.rs:118-128 `table`, encoded (tlwe.rs:113-116); the last half block is the torus negation of the first */
static uint64_t table_at(unsigned (*f)(unsigned), int c) {
    const int m = N >> LOG_P;
    if (c >= N - m / 2) return (uint64_t)0 - ((uint64_t)(f(0) % P) << LOG_DELTA);
    return (uint64_t)(f((unsigned)((c + m / 2) / m)) % P) << LOG_DELTA;
}

int main(void) {
    fhe_torus_ctx *t = NULL;
    fhe_rng *rng = NULL;
    CHECK(fhe_torus_ctx_create(0, &t));
    CHECK(fhe_rng_create_from_seed(2026, &rng));
    /* z: the TLWE key, s: the TGLWE key, both binary; brk_i = TGGSW(z_i) under s; ksk = Tlwe::ksk_gen(z, s) */
    static uint64_t z[N_LWE], s[N], pt[N_LWE * N];
    CHECK(fhe_sample_binary(rng, 1, z, N_LWE, FHE_MEM_HOST, NULL));
    CHECK(fhe_sample_binary(rng, 2, s, N, FHE_MEM_HOST, NULL));
    for (int i = 0; i < N_LWE; ++i) pt[(size_t)i * N] = z[i];
    uint64_t *ra = malloc((size_t)N_LWE * 2 * D * N * 8), *rb = malloc((size_t)N_LWE * 2 * D * N * 8);
    uint64_t *ksa = malloc((size_t)N * KS_D * N_LWE * 8), *ksb = malloc((size_t)N * KS_D * 8);
    if (!ra || !rb || !ksa || !ksb) return 1;
    CHECK(fhe_tggsw_encrypt(t, LOG_B, D, s, pt, N, N_LWE, SD_GLWE, rng, 3, ra, rb, FHE_MEM_HOST, NULL));
    CHECK(fhe_tlwe_ksk_gen(KS_LOG_B, KS_D, z, N_LWE, s, N, SD_LWE, rng, 4, ksa, ksb, FHE_MEM_HOST, NULL));
    fhe_tggsw_key *brk = NULL;
    CHECK(fhe_tggsw_prepare(t, LOG_B, D, ra, rb, N, N_LWE, FHE_MEM_HOST, &brk));

    /* ONE interleaved table: even coefficients from the message table, odd ones from the carry table, each taken at the even
     * coefficient below: after a rotation by an even amount coefficient 0 holds the message function, coefficient 1 the carry */
    static uint64_t table[N];
    for (int c = 0; c < N; ++c) table[c] = table_at(c & 1 ? f_carry : f_msg, c & ~1);

    /* the netlist: inputs x_0 .. x_3, y_0 .. y_3 (wires 0 .. 7); block i is node i with log_funcs = 1 and owns wires 8 + 2 i (message)
     * and 9 + 2 i (carry); the last carry is named by no output and gets no extraction and no key switch */
    fhe_tfhe_node_many nodes[BLOCKS];
    fhe_tfhe_term terms[3 * BLOCKS];
    uint32_t sum[BLOCKS];
    size_t nt = 0;
    for (uint32_t i = 0; i < BLOCKS; ++i) {
        nodes[i].many.first_term = (uint32_t)nt;
        terms[nt].wire = i; terms[nt++].weight = 1;
        terms[nt].wire = BLOCKS + i; terms[nt++].weight = 1;
        if (i) { terms[nt].wire = 2 * BLOCKS + 2 * (i - 1) + 1; terms[nt++].weight = 1; }
        nodes[i].many.n_terms = (uint32_t)nt - nodes[i].many.first_term;
        nodes[i].many.constant = 0;
        nodes[i].many.table = 0;
        nodes[i].many.log_funcs = 1;
        sum[i] = 2 * BLOCKS + 2 * i;
    }
    fhe_tfhe_circuit *circuit = NULL;
    size_t levels = 0, live = 0, width = 0, live_outputs = 0, max_rows = 0;
    CHECK(fhe_tfhe_circuit_create_many(&nodes[0].node, BLOCKS, terms, nt, 2 * BLOCKS, 1, sum, BLOCKS, &circuit));
    CHECK(fhe_tfhe_circuit_info(circuit, &levels, &live, &width));
    CHECK(fhe_tfhe_circuit_info_many(circuit, &live_outputs, &max_rows));
    if (live != 4 || levels != 4 || width != 1 || live_outputs != 7 || max_rows != 2) {
        fprintf(stderr, "netlist: %zu live, %zu levels, %zu live outputs\n", live, levels, live_outputs);
        return 1;
    }

    /* encrypt: block i of byte k of x in slot [i][k], of y in slot [BLOCKS + i][k] */
    const uint8_t xs[BATCH] = {255, 255, 100}, ys[BATCH] = {1, 255, 57};
    static uint64_t msg[2 * BLOCKS * BATCH], in_a[2 * BLOCKS * BATCH * N_LWE], in_b[2 * BLOCKS * BATCH], out_a[BLOCKS * BATCH * N_LWE], out_b[BLOCKS * BATCH];
    for (int i = 0; i < BLOCKS; ++i)
        for (int k = 0; k < BATCH; ++k) {
            msg[i * BATCH + k] = (uint64_t)((xs[k] >> (MSG_BITS * i)) & 3) << LOG_DELTA;
            msg[(BLOCKS + i) * BATCH + k] = (uint64_t)((ys[k] >> (MSG_BITS * i)) & 3) << LOG_DELTA;
        }
    CHECK(fhe_tlwe_sk_encrypt(z, msg, N_LWE, 2 * BLOCKS * BATCH, SD_LWE, rng, 5, in_a, in_b, FHE_MEM_HOST, NULL));
    CHECK(fhe_tfhe_circuit_run(circuit, t, brk, KS_LOG_B, KS_D, ksa, ksb, table, in_a, in_b, out_a, out_b, BATCH, FHE_MEM_HOST, NULL));

    /* decrypt: round(b - <a, z>) to a multiple of 2^LOG_DELTA */
    int bad = 0;
    for (int k = 0; k < BATCH; ++k) {
        unsigned got = 0;
        for (int i = 0; i < BLOCKS; ++i) {
            const uint64_t *a = out_a + ((size_t)i * BATCH + k) * N_LWE;
            uint64_t phase = out_b[i * BATCH + k];
            for (int j = 0; j < N_LWE; ++j) phase -= a[j] * z[j];
            const unsigned m = (unsigned)((phase + ((uint64_t)1 << (LOG_DELTA - 1))) >> LOG_DELTA);
            if (m > 3) bad = 1;
            got |= (m & 3u) << (MSG_BITS * i);
        }
        printf("%u + %u = %u (mod 256)\n", xs[k], ys[k], got);
        if (got != ((unsigned)xs[k] + ys[k]) % 256u) bad = 1;
    }
    if (bad) { fprintf(stderr, "wrong sum\n"); return 1; }
    printf("tfhe_many_demo ok: %zu blind rotations in %zu levels for %zu live outputs, one call for %d pairs of bytes\n", live, levels, live_outputs, BATCH);
    fhe_tfhe_circuit_destroy(circuit);
    fhe_tggsw_key_destroy(brk);
    fhe_rng_destroy(rng); fhe_torus_ctx_destroy(t);
    free(ra); free(rb); free(ksa); free(ksb);
    return 0;
}
