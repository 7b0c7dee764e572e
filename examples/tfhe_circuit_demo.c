/* Two encrypted bytes added from plain C: include/fhe_ring.h and libfhe_ring.so only.  The pattern of the reference's TFHE test
 * (scheme/tfhe/src/bootstrapping.rs:118-165: log_p = 4 message bits under one padding bit, one table per function) used as radix
 * arithmetic: a byte is 4 blocks of 2 message bits with 2 bits of carry room; per block one message table and one carry table of
 * x_i + y_i + carry_{i-1}.  Keys as `Bootstrapping::key_gen` makes them (bootstrapping.rs:59-76), from the device key generators; ONE
 * call of fhe_tfhe_circuit_run on host buffers for BATCH pairs of bytes; decryption (tlwe.rs:134-142).
 * build: gcc -std=c99 -O2 -I include examples/tfhe_circuit_demo.c -L learn-fhe_amd/lib -lfhe_ring -Wl,-rpath,$PWD/learn-fhe_amd/lib \
 *            -Wl,--allow-shlib-undefined -o tfhe_circuit_demo */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "fhe_ring.h"

#define N 256
#define N_LWE 16
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

/* bootstrapping.rs:118-128 `table`, encoded (tlwe.rs:113-116); the last half block is the torus negation of the first, so that a
 * phase just below 0 wraps to table[0] with a clear padding bit */
static void make_table(unsigned (*f)(unsigned), uint64_t *out) {
    const int m = N >> LOG_P;
    int k = 0;
    for (int i = 0; i < m / 2; ++i) out[k++] = (uint64_t)(f(0) % P) << LOG_DELTA;
    for (unsigned v = 1; v < P; ++v)
        for (int i = 0; i < m; ++i) out[k++] = (uint64_t)(f(v) % P) << LOG_DELTA;
    for (int i = 0; i < m / 2; ++i) out[k++] = (uint64_t)0 - ((uint64_t)(f(0) % P) << LOG_DELTA);
}

int main(void) {
    fhe_torus_ctx *t = NULL;
    fhe_rng *rng = NULL;
    CHECK(fhe_torus_ctx_create(0, &t));
    CHECK(fhe_rng_create_from_seed(2025, &rng));
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

    /* the netlist: inputs x_0 .. x_3, y_0 .. y_3 (wires 0 .. 7); per block a message node (table 0) and a carry node (table 1) over the
     * same terms; the last carry is emitted like the others and dropped by create */
    static uint64_t tables[2 * N];
    make_table(f_msg, tables);
    make_table(f_carry, tables + N);
    fhe_tfhe_node nodes[2 * BLOCKS];
    fhe_tfhe_term terms[2 * 3 * BLOCKS];
    uint32_t sum[BLOCKS], carry = 0;
    size_t nn = 0, nt = 0;
    for (uint32_t i = 0; i < BLOCKS; ++i) {
        for (int which = 0; which < 2; ++which) {
            fhe_tfhe_node nd = {0, 0, 0, 0, 0};
            nd.first_term = (uint32_t)nt;
            terms[nt].wire = i; terms[nt++].weight = 1;
            terms[nt].wire = BLOCKS + i; terms[nt++].weight = 1;
            if (i) { terms[nt].wire = carry; terms[nt++].weight = 1; }
            nd.n_terms = (uint32_t)nt - nd.first_term;
            nd.table = (uint32_t)which;
            nodes[nn] = nd;
            if (which == 0) sum[i] = (uint32_t)(2 * BLOCKS + nn);
            ++nn;
        }
        carry = (uint32_t)(2 * BLOCKS + nn - 1);
    }
    fhe_tfhe_circuit *circuit = NULL;
    size_t levels = 0, live = 0, width = 0;
    CHECK(fhe_tfhe_circuit_create(nodes, nn, terms, nt, 2 * BLOCKS, 2, sum, BLOCKS, &circuit));
    CHECK(fhe_tfhe_circuit_info(circuit, &levels, &live, &width));
    if (nn != 8 || live != 7 || levels != 4 || width != 2) { fprintf(stderr, "netlist: %zu nodes, %zu live, %zu levels\n", nn, live, levels); return 1; }

    /* encrypt: block i of byte k of x in slot [i][k], of y in slot [BLOCKS + i][k] */
    const uint8_t xs[BATCH] = {255, 255, 100}, ys[BATCH] = {1, 255, 57};
    static uint64_t msg[2 * BLOCKS * BATCH], in_a[2 * BLOCKS * BATCH * N_LWE], in_b[2 * BLOCKS * BATCH], out_a[BLOCKS * BATCH * N_LWE], out_b[BLOCKS * BATCH];
    for (int i = 0; i < BLOCKS; ++i)
        for (int k = 0; k < BATCH; ++k) {
            msg[i * BATCH + k] = (uint64_t)((xs[k] >> (MSG_BITS * i)) & 3) << LOG_DELTA;
            msg[(BLOCKS + i) * BATCH + k] = (uint64_t)((ys[k] >> (MSG_BITS * i)) & 3) << LOG_DELTA;
        }
    CHECK(fhe_tlwe_sk_encrypt(z, msg, N_LWE, 2 * BLOCKS * BATCH, SD_LWE, rng, 5, in_a, in_b, FHE_MEM_HOST, NULL));
    CHECK(fhe_tfhe_circuit_run(circuit, t, brk, KS_LOG_B, KS_D, ksa, ksb, tables, in_a, in_b, out_a, out_b, BATCH, FHE_MEM_HOST, NULL));

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
    printf("tfhe_circuit_demo ok: %zu nodes in %zu levels (widest %zu), one call for %d pairs of bytes\n", live, levels, width, BATCH);
    fhe_tfhe_circuit_destroy(circuit);
    fhe_tggsw_key_destroy(brk);
    fhe_rng_destroy(rng); fhe_torus_ctx_destroy(t);
    free(ra); free(rb); free(ksa); free(ksb);
    return 0;
}
