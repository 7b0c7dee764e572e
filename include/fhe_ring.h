/* fhe_ring.h -- C ABI of the MI355X (gfx950) polynomial-ring backend.
 *
 * Drop-in boundary for the ring hot path of han0110/learn-fhe's `util` crate.  The reference has no
 * FFI layer; the seam these entry points replace is the three crate-private functions in
 * util/src/ring/fft/zq.rs:14-36 (called only from util/src/ring.rs:140-144, 180-184, 256-264) plus the
 * pure helpers listed per function below.  A Rust `util` fork would bind them with one `extern "C"`
 * block (INTEGRATION.md shows it).
 *
 * Conventions
 *   - all ring data are flat little-endian uint64_t arrays of fully reduced values in [0, q);
 *     a batch of polynomials is contiguous, [batch][n];
 *   - `mem` says where every data pointer of the call lives: FHE_MEM_DEVICE = HBM of the context's device
 *     (the measured path: nothing is copied), FHE_MEM_HOST = pageable host memory (the library stages
 *     through its own device buffers and synchronises before returning);
 *   - `stream` is a hipStream_t (NULL = the default stream); device calls are asynchronous on it;
 *   - every function returns an int status (FHE_OK == 0) where the reference would panic; nothing aborts;
 *   - contexts and key handles are immutable after creation and may be shared between host threads.
 *   - there is NO CPU compute fallback: a context created with device < 0 only serves the host-side
 *     queries (primes, generator, twiddles) and every compute call on it returns FHE_ERR_NO_DEVICE.
 */
#ifndef FHE_RING_H
#define FHE_RING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    FHE_OK = 0,
    FHE_ERR_INVALID = 1,      /* null pointer, n not a power of two, bad parameter (ring.rs:62 assert) */
    FHE_ERR_NOT_PRIME = 2,    /* NTT requested for a non-prime modulus (fft/zq.rs:44: missing map key) */
    FHE_ERR_NO_ROOT = 3,      /* n > 2^(s-1): no primitive 2n-th root (fft.rs:45 slice out of bounds) */
    FHE_ERR_MODULUS = 4,      /* operands over different moduli (zq.rs:145/177/185/193 assert_eq) */
    FHE_ERR_HIP = 5,          /* a HIP runtime call failed; fhe_last_hip_error() has the code */
    FHE_ERR_UNSUPPORTED = 6,  /* valid in the reference, outside what this build implements (q >= 2^62, n > 2^17) */
    FHE_ERR_NO_DEVICE = 7,    /* compute call on a host-only context */
    FHE_ERR_TIMEOUT = 8       /* a bounded wait between the workgroups of one launch ran out (split FHEW or TFHE blind rotation): no output written */
};

typedef enum { FHE_MEM_HOST = 0, FHE_MEM_DEVICE = 1 } fhe_mem;

typedef struct fhe_ctx fhe_ctx; /* one prime modulus: s, g, omega, twiddle tables (host + HBM) */

const char *fhe_version(void);
int fhe_last_hip_error(void);
/* Device scratch of the entry points comes from a private stream-ordered pool per device (never the device's default pool);
 * freed blocks are kept for the next call up to 4 GiB.  fhe_trim() returns everything that is not in use to the driver. */
int fhe_trim(void);
/* Lab switches.  Routes that a faster one replaced stay in the library so that tests can compare the two bit for bit; NONE changes a
 * result.  Each is read ONCE from the environment (FHE_RING_<NAME>) and afterwards only through this call: the library never calls
 * getenv on a call path.  Names: "NO_EDGE" (key switch at N = 2^15 on whole transforms), "NO_LIMB_MAJOR" (linear dispatch order over
 * several moduli), "NO_W12" (2^12 / 2^13 rings on the generic kernels), "NO_FUSED_MUL" (ring product as forward + multiplying
 * inverse), "SMALL_BATCH" (FHEW: 4 coefficients per lane up to this batch, 8 above; -1 = the library's rule), "NO_F64_EXACT" (TFHE: eligible keys on the three-prime integer path instead of the three-piece f64 one), "NO_PACKED_DIGITS" (TFHE blind
 * rotation: digits decomposed once per prime instead of once per CMUX), "FHEW_COMPOSED" (FHEW keys prepared while it is set run the
 * composed route at n = 128 .. 2048 too, instead of the fused kernels), "BR_SPLIT" (FHEW blind rotation: workgroups per ciphertext;
 * -1 = the library's rule, 0 = never split, 2 / 4 / 8 = that many wherever the call admits it -- fused route, n = 1024 or 2048,
 * batch x value <= compute units of the device -- and one workgroup per ciphertext elsewhere; any other value: FHE_ERR_INVALID;
 * fhe_blind_rotate_split tells what a call will run), "PFKS_SPLIT" (fhe_tlwe_pfks: 0 = the library's rule, 1 = one block walks all
 * input rows of its tile, k >= 2 = k blocks share them and add their partial sums), "PFKS_CHUNK" (fhe_tlwe_pfks: input coefficients whose digits a block
 * keeps in LDS at a time; 0 = the library's rule), "LUT_EXTRACT" (fhe_tfhe_lut_eval: 0 = the library's rule, 1 = the rotation ladder writes the
 * extractions from its registers, 2 = a kernel of its own reads the stored accumulators), "TFHE_SPLIT" (TFHE blind rotation: workgroups per
 * ciphertext; -1 = the library's rule, 0 = never split, 2 / 6 = that many wherever the call is eligible -- a key in the x3 form at
 * n = 1024, batch x value <= compute units of the device -- and one workgroup per ciphertext elsewhere; any other value:
 * FHE_ERR_INVALID; fhe_tfhe_blind_rotate_split tells what a call will run), "NO_RANKK_FUSED" (rank-k TGGSW keys prepared while it is
 * set take the composed route where the fused kernels would serve them: fhe_tggswk_form_for), "PACK_SPLIT" (fhe_tlwe_pack: 0 = the library's
 * rule, k >= 1 = k chunks of key rows per pack, clamped to what exactness needs and to one row per chunk), "PACK_ROUTE" (fhe_tlwe_pack:
 * 0 = the library's rule, 1 = the transforms, 2 = the scalar digits x key product and one rotate-and-add kernel), "PACK_SLAB"
 * (fhe_tlwe_pack: packs per launch group; 0 = what 256 MiB of scratch hold, s >= 1 = at most s).  Unknown name: FHE_ERR_INVALID. */
int fhe_set_option(const char *name, long value);

/* Entry points that take a modulus instead of a context (fhe_rq_*, fhe_decompose, fhe_automorphism, fhe_monomial_mul,
 * fhe_lwe_*, fhe_rlwe_sample_extract, fhe_torus_decompose, fhe_tfhe_mod_switch, fhe_tglwe_sample_extract, fhe_tlwe_key_switch)
 * run on the device their FHE_MEM_DEVICE operands live on, whatever the caller's current device is; `stream` must belong to
 * that device.  With FHE_MEM_HOST they run on the current device. */

/* ---- scalar / setup (host only) -------------------------------------------------------------- */
/* util/src/zq.rs:337-342 `is_prime` */
int fhe_is_prime(uint64_t q);
/* util/src/zq.rs:325-329 `two_adic_primes(bits, log_n).take(count)`; returns how many were written */
int fhe_two_adic_primes(int bits, int log_n, int count, uint64_t *out);

/* util/src/ring/fft/zq.rs:49-67 `twiddle(q)` / `compute_twiddle`: validates q prime, derives
 * s = trailing_zeros(q-1), g = smallest quadratic non-residue (zq.rs:99-105), omega = g^((q-1)>>s),
 * and the bit-reversed tables.  device >= 0: tables are uploaded to that GPU; device < 0: host-only. */
int fhe_ctx_create(uint64_t q, int device, fhe_ctx **out);
void fhe_ctx_destroy(fhe_ctx *ctx);
int fhe_ctx_info(const fhe_ctx *ctx, uint64_t *q, int *s, uint64_t *g, uint64_t *omega);
/* first `count` entries of the reference's twiddle table (inverse != 0: the inverse table) */
int fhe_ctx_twiddles(const fhe_ctx *ctx, int inverse, uint64_t *out, size_t count);

/* ---- transforms ------------------------------------------------------------------------------ */
/* util/src/ring/fft/zq.rs:27-30 `nega_cyclic_ntt_in_place` (= ring.rs:140-144 `to_evaluation`):
 * natural-order coefficients -> bit-reversed-order evaluations, in place, for `batch` polynomials. */
int fhe_ntt_fwd(const fhe_ctx *ctx, uint64_t *a, size_t n, size_t batch, fhe_mem mem, void *stream);
/* util/src/ring/fft/zq.rs:32-36 `nega_cyclic_intt_in_place` (= ring.rs:180-184 `to_coefficient`). */
int fhe_ntt_inv(const fhe_ctx *ctx, uint64_t *a, size_t n, size_t batch, fhe_mem mem, void *stream);
/* util/src/ring/fft/zq.rs:14-19 `nega_cyclic_ntt_mul_assign` (= ring.rs:256-264 `Rq *= &Rq`):
 * a[k] <- a[k] * b[k] in Z_q[X]/(X^n+1), coefficient domain in and out.
 * Device memory, n = 2^12 .. 2^15 (and the two 2^14 halves a 2^15 RNS transform is split into): the transforms read and write
 * every polynomial 16 bytes per lane, so `a` and `b` must be 16-byte aligned (any allocation and any whole-polynomial offset
 * into one is); a pointer that is not is rejected with FHE_ERR_INVALID before anything is written.  That holds for fhe_ntt_fwd /
 * fhe_ntt_inv / fhe_ntt_mul and for every entry point that hands a FHE_MEM_DEVICE operand to these transforms (in place, or out
 * of place as `b` here and the fhe_rns_* / fhe_ckks_* products and key preparation).  Rings above 2^15 read their operands
 * 8 bytes per lane in a first pass of their own and carry no such requirement. */
int fhe_ntt_mul(const fhe_ctx *ctx, uint64_t *a, const uint64_t *b, size_t n, size_t batch, fhe_mem mem,
                void *stream);
/* util/src/ring.rs:328-358 `Rq` + / - / unary - and 359-366 scalar `*= Zq` (zq.rs:156-196), element-wise over `len`
 * values of any modulus q < 2^62 (either basis: the operations are the same on coefficients and on evaluations);
 * `out` may alias an input.  fhe_rq_from_i64: util/src/zq.rs:63-69 `Zq::from_i64` (rem_euclid), the conversion
 * `Rq *= &AVec<i64>` (ring.rs:272-282) applies to its right-hand side before the product. */
int fhe_rq_add(uint64_t q, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t len, fhe_mem mem, void *stream);
int fhe_rq_sub(uint64_t q, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t len, fhe_mem mem, void *stream);
int fhe_rq_neg(uint64_t q, const uint64_t *a, uint64_t *out, size_t len, fhe_mem mem, void *stream);
int fhe_rq_scalar_mul(uint64_t q, const uint64_t *a, uint64_t scalar, uint64_t *out, size_t len, fhe_mem mem, void *stream);
int fhe_rq_from_i64(uint64_t q, const int64_t *in, uint64_t *out, size_t len, fhe_mem mem, void *stream);
/* util/src/ring.rs:266-270 evaluation-domain `MulAssign`: a[i] <- a[i] * b[i] mod q, len elements. */
int fhe_pointwise_mul(const fhe_ctx *ctx, uint64_t *a, const uint64_t *b, size_t len, fhe_mem mem, void *stream);

/* ---- gadget decomposition, automorphism, monomial (any modulus q < 2^62, on the current HIP device) ---- */
/* util/src/misc/decompose.rs:42-46 `Base2Decomposor::<Zq>::new(q, log_b, d).decompose(poly)`:
 * in [polys][n] -> out [polys][d][n], digit j of coefficient i of polynomial p at out[(p*d + j)*n + i],
 * least-significant digit first, digits in [-B/2, B/2] mod q exactly as decompose.rs:91-112 produces them. */
int fhe_decompose(uint64_t q, int log_b, int d, const uint64_t *in, size_t n, size_t polys, uint64_t *out, fhe_mem mem,
                  void *stream);
/* util/src/avec.rs:34-50 `automorphism(t)`: X -> X^t, t taken mod 2n; out must not alias in. */
int fhe_automorphism(uint64_t q, int64_t t, const uint64_t *in, uint64_t *out, size_t n, size_t batch, fhe_mem mem,
                     void *stream);
/* util/src/ring.rs:299-313 `Rq *= X^k`, k taken mod 2n; out must not alias in. */
int fhe_monomial_mul(uint64_t q, int64_t k, const uint64_t *in, uint64_t *out, size_t n, size_t batch, fhe_mem mem,
                     void *stream);

/* ---- prepared gadget keys (device resident, evaluation domain) ---------------------------------------- */
typedef struct fhe_key fhe_key;
/* `count` RGSW ciphertexts (scheme/fhew/src/rgsw.rs:37-47, 84-105): rows_a / rows_b = the a / b polynomials of the
 * 2d RLWE rows of each, [count][2d][n], coefficient domain.  n = any power of two 1 .. 2^ctx's table size (2^17 at most; FHE_ERR_NO_ROOT
 * above the modulus's two-adicity): 128 .. 2048 run the fused kernels, every other n (and every n of a key prepared while the lab
 * switch "FHEW_COMPOSED" is set) whole-batch launches -- digits, transforms, multiply-accumulate -- over chunks of the batch.  The
 * gadget products, key switches, automorphisms and blind rotations below take the sizes of their keys. */
int fhe_rgsw_prepare(const fhe_ctx *ctx, int log_b, int d, const uint64_t *rows_a, const uint64_t *rows_b, size_t n,
                     size_t count, fhe_mem mem, fhe_key **out);
/* `count` RLWE key-switching / automorphism keys (scheme/fhew/src/rlwe.rs:43-66, 109-132): [count][d][n], n as above. */
int fhe_ksk_prepare(const fhe_ctx *ctx, int log_b, int d, const uint64_t *rows_a, const uint64_t *rows_b, size_t n,
                    size_t count, fhe_mem mem, fhe_key **out);
void fhe_key_destroy(fhe_key *key);

/* scheme/fhew/src/rgsw.rs:116-128 `Rgsw::external_product(param, rgsw[index], ct)` for `batch` RLWE ciphertexts
 * (ct_a, ct_b: [batch][n], coefficient domain, in place). */
int fhe_external_product(const fhe_ctx *ctx, const fhe_key *rgsw, size_t index, uint64_t *ct_a, uint64_t *ct_b,
                         size_t batch, fhe_mem mem, void *stream);
/* scheme/fhew/src/rgsw.rs:130-150 `Rgsw::internal_product(param, ct0 = rgsw[index], ct1)`: RGSW x RGSW -> RGSW.  The reference
 * transforms ct0's rows once and takes, for every one of ct1's 2d RLWE rows, the evaluation-domain dot product with that row's
 * digits -- i.e. the external product of ct0 with each row of ct1.  ct0 is a prepared key (its rows already sit in the
 * evaluation domain, exactly what lines 136-137 compute); ct1_a / ct1_b: [count][2d][n] (coefficient domain, the layout
 * fhe_rgsw_prepare takes), replaced in place by the rows of the product, for `count` right-hand RGSW ciphertexts. */
int fhe_rgsw_internal_product(const fhe_ctx *ctx, const fhe_key *rgsw, size_t index, uint64_t *ct1_a, uint64_t *ct1_b,
                              size_t count, fhe_mem mem, void *stream);
/* scheme/fhew/src/rlwe.rs:177-186 `Rlwe::key_switch(param, ksk[index], ct)`. */
int fhe_rlwe_key_switch(const fhe_ctx *ctx, const fhe_key *ksk, size_t index, uint64_t *ct_a, uint64_t *ct_b,
                        size_t batch, fhe_mem mem, void *stream);
/* scheme/fhew/src/rlwe.rs:188-191 `Rlwe::automorphism(param, ak[index] (exponent t), ct)`. */
int fhe_rlwe_automorphism(const fhe_ctx *ctx, const fhe_key *ak, size_t index, int64_t t, uint64_t *ct_a,
                          uint64_t *ct_b, size_t batch, fhe_mem mem, void *stream);

/* ---- LMKCDEY blind rotation --------------------------------------------------------------------------- */
typedef struct fhe_bootstrap_key fhe_bootstrap_key;
/* scheme/fhew/src/bootstrapping.rs:93-113 `BootstrappingKey{brk, ak}` (the LWE ksk belongs to the "next" row):
 * brk = n_lwe prepared RGSW ciphertexts, ak = w+1 prepared automorphism keys with exponents ak_t[0..w]
 * (= [-g, g, g^2, .., g^w] mod 2n, bootstrapping.rs:86-89).  The handles must outlive the bootstrap key.  n >= 2: at n = 1 the
 * reference panics (an empty i_minus, bootstrapping.rs:191, 215), here FHE_ERR_INVALID; so are brk and ak prepared for different
 * routes (one with the lab switch "FHEW_COMPOSED", one without, at n = 128 .. 2048). */
int fhe_bootstrap_key_create(const fhe_ctx *ctx, const fhe_key *brk, const fhe_key *ak, const int64_t *ak_t, int w,
                             fhe_bootstrap_key **out);
void fhe_bootstrap_key_destroy(fhe_bootstrap_key *bk);
/* Waits for everything enqueued on `stream`, then FHE_ERR_INVALID if an asynchronous (device-memory) fhe_blind_rotate /
 * fhe_fhew_bootstrap on this key met an LWE coefficient that is not an odd residue mod 2n since the word was last cleared,
 * FHE_ERR_TIMEOUT if a split blind rotation gave up a wait (fhe_blind_rotate_split), else FHE_OK; clear != 0 resets the word. */
int fhe_bootstrap_key_status(const fhe_bootstrap_key *bk, void *stream, int clear);
/* Workgroups per ciphertext (*g_out = 1, 2, 4 or 8) that fhe_blind_rotate / fhe_fhew_bootstrap would use for this key and batch
 * under the current options ("BR_SPLIT") on the context's device.  Above 1 a cluster of workgroups shares the digit transforms of
 * every step of one ciphertext's walk and hands partial sums over inside the launch: lower latency at batches that leave the chip
 * idle, bit-identical results.  Its waits are bounded: one that runs out writes no output and the call reports FHE_ERR_TIMEOUT
 * (host-memory calls in their return value, device-memory calls through fhe_bootstrap_key_status). */
int fhe_blind_rotate_split(const fhe_bootstrap_key *bk, size_t batch, int *g_out);
/* scheme/fhew/src/bootstrapping.rs:158-209 `blind_rotate(param, brk, ak, f, LweCiphertext(a, b))` for a batch:
 * lwe_a [batch][n_lwe] and lwe_b [batch] are taken mod 2n (after mod_switch_odd); f = LUT polynomial(s),
 * f_stride = 0 (one f) or n (one per ciphertext); out_a/out_b [batch][n] = the rotated accumulator.
 * ops_out/nops_out (host pointers, may be NULL): the walk of blind_rotate_core per ciphertext,
 * [batch][n_lwe + n + 2] entries, bit 31 set = automorphism ak[idx], clear = external product brk[idx].
 * lwe_b is reduced mod 2n; every lwe_a entry must already be an ODD residue below 2n (what `mod_switch_odd`, lwe.rs:94-99,
 * produces): anything else makes the reference index out of its log map and panic (bootstrapping.rs:221), here FHE_ERR_INVALID.
 * That check is data dependent.  Host-memory calls (and calls that ask for the walk) report it in their return value; DEVICE-memory
 * calls stay asynchronous like every other entry point -- they return once the work is enqueued and record the condition in a
 * sticky status word of the bootstrap key, which fhe_bootstrap_key_status reads (the same holds for fhe_fhew_bootstrap, which
 * ends with this call). */
int fhe_blind_rotate(const fhe_bootstrap_key *bk, const uint64_t *lwe_a, const uint64_t *lwe_b, const uint64_t *f,
                     size_t f_stride, uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem, void *stream,
                     uint32_t *ops_out, uint32_t *nops_out);

/* ---- the LWE side of the FHEW gate ------------------------------------------- */
/* util/src/zq.rs:128-140 via scheme/fhew/src/lwe.rs:90-99: `mod_switch(q_prime)` (odd = 0) / `mod_switch_odd` (odd != 0)
 * for `count` values over q: the reference's f64 arithmetic and rounding reproduced with IEEE double operations. */
int fhe_lwe_mod_switch(uint64_t q, uint64_t q_prime, const uint64_t *in, uint64_t *out, size_t count, int odd, fhe_mem mem,
                       void *stream);
/* scheme/fhew/src/lwe.rs:151-160 `Lwe::key_switch` over q < 2^32: ksk_a [d*n_in][n_out], ksk_b [d*n_in], rows digit-major. */
int fhe_lwe_key_switch(uint64_t q, int log_b, int d, const uint64_t *ksk_a, const uint64_t *ksk_b, const uint64_t *ct_a,
                       const uint64_t *ct_b, size_t n_in, size_t n_out, uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem,
                       void *stream);
/* scheme/fhew/src/lwe.rs:22-75 (Add / Sub / Neg / double on LweCiphertext): out = sum_{t<k} coef[t] * in[t] + addend over
 * q < 2^62, k <= 4: the linear part of the gates (scheme/fhew/src/fhew.rs:27-29 `not`, 61-69 Table 1). */
int fhe_lwe_lincomb(uint64_t q, int k, const int64_t *coef, const uint64_t *const *in, uint64_t addend, uint64_t *out, size_t count,
                    fhe_mem mem, void *stream);
/* scheme/fhew/src/rlwe.rs:193-202 `Rlwe::sample_extract(ct, index)`; `addend` (< q) is added to b. */
int fhe_rlwe_sample_extract(uint64_t q, const uint64_t *ct_a, const uint64_t *ct_b, size_t n, size_t index, uint64_t addend,
                            uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem, void *stream);
/* scheme/fhew/src/bootstrapping.rs:149-155 `Bootstrapping::bootstrap(bk, f, ct)` for a batch of LWE ciphertexts under the
 * ring key (ct_a [batch][N], ct_b [batch] over Q): mod_switch(q_ks) -> Lwe::key_switch -> mod_switch_odd(2N) ->
 * blind_rotate -> sample_extract(0) (+ addend on b: Fhew::op's Q/8, scheme/fhew/src/fhew.rs:39).  One gate bootstrap. */
int fhe_fhew_bootstrap(const fhe_bootstrap_key *bk, uint64_t q_ks, int ks_log_b, int ks_d, const uint64_t *lwe_ksk_a,
                       const uint64_t *lwe_ksk_b, const uint64_t *f, size_t f_stride, uint64_t addend, const uint64_t *ct_a,
                       const uint64_t *ct_b, uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem, void *stream);

/* ---- RNS rings (CKKS) ------------------------------------------------------------------------------------ */
typedef struct fhe_rns_ctx fhe_rns_ctx;   /* bases qs (L primes) and ps (K primes): util/src/ring/rns.rs:278-322 `Rns` */
typedef struct fhe_ckks_key fhe_ckks_key; /* a key-switching key over qs ++ ps, evaluation domain, device resident */
/* `Rns::new(qs).with_ps(ps)` both ways (Q->P for extend_bases, P->Q for rescale_k) plus one transform context per
 * prime.  All L+K primes must be distinct (rns.rs:25, 84 asserts).  L, K <= 32. */
int fhe_rns_ctx_create(const uint64_t *qs, int L, const uint64_t *ps, int K, int device, fhe_rns_ctx **out);
void fhe_rns_ctx_destroy(fhe_rns_ctx *rns);
/* Evaluation-domain residency for `RnsRq`: util/src/ring/rns.rs:40-49 `to_evaluation` /
 * `to_coefficient` limb by limb in ONE launch, and rns.rs:148-158 the evaluation-basis product.  `extended` = 0:
 * polynomials over qs, [batch][L][n]; != 0: over qs ++ ps, [batch][L+K][n].  A caller keeps operands in the evaluation
 * basis on the device across mul -> relinearize -> rescale instead of transforming per operation. */
int fhe_rns_ntt_fwd(const fhe_rns_ctx *rns, int extended, uint64_t *a, size_t n, size_t batch, fhe_mem mem, void *stream);
int fhe_rns_ntt_inv(const fhe_rns_ctx *rns, int extended, uint64_t *a, size_t n, size_t batch, fhe_mem mem, void *stream);
int fhe_rns_pointwise_mul(const fhe_rns_ctx *rns, int extended, uint64_t *a, const uint64_t *b, size_t n, size_t batch, fhe_mem mem,
                          void *stream);
/* util/src/ring/rns.rs:83-91 `RnsRq::extend_bases(ps)`: in [batch][L][n] over qs -> out [batch][K][n], the new
 * p-limbs (fast base conversion with the reference's f64 rounding correction, rns.rs:331-345). */
int fhe_rns_extend_bases(const fhe_rns_ctx *rns, const uint64_t *in, uint64_t *out, size_t n, size_t batch, fhe_mem mem,
                         void *stream);
/* util/src/ring/rns.rs:93-97 `RnsRq::switch_bases`: the same polynomial over the OTHER base (extend_bases, old limbs dropped).
 * to_qs = 0: in [batch][L][n] over qs -> out [batch][K][n] over ps; to_qs != 0: in [batch][K][n] over ps -> out [batch][L][n] over qs. */
int fhe_rns_switch_bases(const fhe_rns_ctx *rns, int to_qs, const uint64_t *in, uint64_t *out, size_t n, size_t batch, fhe_mem mem,
                         void *stream);
/* util/src/ring/rns.rs:103-118 `rescale_k(K)` of a polynomial over qs ++ ps: in [batch][L+K][n] -> out [batch][L][n]. */
int fhe_rns_rescale_k(const fhe_rns_ctx *rns, const uint64_t *in, uint64_t *out, size_t n, size_t batch, fhe_mem mem,
                      void *stream);
/* key-switching key (scheme/ckks/src/ckks.rs:86-88, 143-161): ksk_b, ksk_a [L+K][n], coefficient domain. */
int fhe_ckks_ksk_prepare(const fhe_rns_ctx *rns, const uint64_t *ksk_b, const uint64_t *ksk_a, size_t n, fhe_mem mem,
                         fhe_ckks_key **out);
void fhe_ckks_key_destroy(fhe_ckks_key *key);
/* scheme/ckks/src/ckks.rs:284-293 `Ckks::key_switch(param, ksk, CkksCiphertext(ct_b, ct_a))`, in place, for `batch`
 * ciphertexts: ct_b, ct_a [batch][L][n] over qs, coefficient domain.  n up to 2^17. */
int fhe_ckks_key_switch(const fhe_rns_ctx *rns, const fhe_ckks_key *key, uint64_t *ct_b, uint64_t *ct_a, size_t batch,
                        fhe_mem mem, void *stream);
/* ---- the key switch with its RNS limbs sharded over devices -------------------------------
 * `Ckks::key_switch` (scheme/ckks/src/ckks.rs:284-293) is limb-wise except for its two base conversions.  Every device holds the
 * context and the prepared key (replicated: 8 MiB at cfg4) and OWNS the q-limbs [q_lo, q_hi) and the p-limbs [p_lo, p_hi); all devices
 * own equally many p-limbs (np divides K).  Per batch of ciphertexts:
 *   1. fhe_ckks_shard_products  local: ct.a (all L q-limbs, replicated at staging) -> the two key products on the owned limbs;
 *   2. the caller ALL-GATHERS prod_p over the devices -- the one exchange of the path: an RCCL all-gather in the caller's own
 *      communicator, or hipMemcpyPeerAsync into each peer's gather buffer (examples/multi_gpu_ckks_demo.c); contribution of the
 *      device that owns p-limbs [p_lo, p_hi) goes to slot p_lo / np;
 *   3. fhe_ckks_shard_finish    local: rescale_k on the owned q-limbs against all K gathered p-limbs (+ ct.b's owned limbs).
 * The library links neither RCCL nor peer copies: step 2 sits between two calls, where the caller's communicator already lives.
 * Bases of pseudo-Mersenne primes of one bit length only (every CkksParam of the reference): FHE_ERR_UNSUPPORTED otherwise. */
typedef struct fhe_ckks_shard fhe_ckks_shard;
int fhe_ckks_shard_create(const fhe_rns_ctx *rns, const fhe_ckks_key *key, int q_lo, int q_hi, int p_lo, int p_hi, fhe_ckks_shard **out);
void fhe_ckks_shard_destroy(fhe_ckks_shard *shard);
/* ct_a [batch][L][n] -> prod_q [2][batch][nq][n], prod_p [2][batch][np][n] (part 0: ksk.b * a~, part 1: ksk.a * a~; an internal
 * coefficient-domain form that only fhe_ckks_shard_finish reads) */
int fhe_ckks_shard_products(const fhe_ckks_shard *shard, const uint64_t *ct_a, uint64_t *prod_q, uint64_t *prod_p, size_t batch, fhe_mem mem,
                            void *stream);
/* prod_q (stage 1), gathered_p [K / np][2][batch][np][n], ct_b [batch][nq][n] (ct.b's owned limbs, or NULL) -> out_b, out_a
 * [batch][nq][n]: the owned limbs of the switched ciphertext, bit-identical to fhe_ckks_key_switch's */
int fhe_ckks_shard_finish(const fhe_ckks_shard *shard, const uint64_t *prod_q, const uint64_t *gathered_p, const uint64_t *ct_b,
                          uint64_t *out_b, uint64_t *out_a, size_t batch, fhe_mem mem, void *stream);
/* util/src/ring/rns.rs:99-101 `RnsRq::rescale()` = rescale_k(1) over qs alone: drops the last q-limb (the K == 1 branch of
 * rns.rs:104-111, NOT centred).  in [batch][L][n] -> out [batch][L-1][n]; L >= 2. */
int fhe_rns_rescale(const fhe_rns_ctx *rns, const uint64_t *in, uint64_t *out, size_t n, size_t batch, fhe_mem mem, void *stream);
/* util/src/ring/rns.rs:254-270 `RnsRq += RnsRq`, `-= RnsRq`, unary `-` in either basis (what `CkksCiphertext` + / - do on both
 * components: ckks.rs `add_sub`): a <- a + b, a - b, -a over [batch][limbs][n]; extended = 0: qs, 1: qs ++ ps. */
int fhe_rns_add(const fhe_rns_ctx *rns, int extended, uint64_t *a, const uint64_t *b, size_t n, size_t batch, fhe_mem mem, void *stream);
int fhe_rns_sub(const fhe_rns_ctx *rns, int extended, uint64_t *a, const uint64_t *b, size_t n, size_t batch, fhe_mem mem, void *stream);
int fhe_rns_neg(const fhe_rns_ctx *rns, int extended, uint64_t *a, size_t n, size_t batch, fhe_mem mem, void *stream);
/* scheme/ckks/src/ckks.rs:127-129 `automorphism(t)` of an RnsRq (util/src/avec.rs:34-50 on every limb): in, out [batch][L][n],
 * in != out.  t is taken mod 2n; CKKS only uses odd t (5^j, -1) and an even t returns FHE_ERR_UNSUPPORTED. */
int fhe_rns_automorphism(const fhe_rns_ctx *rns, int64_t t, const uint64_t *in, uint64_t *out, size_t n, size_t batch, fhe_mem mem,
                         void *stream);
/* scheme/ckks/src/ckks.rs:274-282 `Ckks::rotate` (key = rtk for j, t = 5^j mod 2n = `param.pow5(j)`) and `Ckks::conjugate`
 * (key = cjk, t = -1): automorphism of both halves, then the key switch.  ct_b, ct_a [batch][L][n], in place. */
int fhe_ckks_rotate(const fhe_rns_ctx *rns, const fhe_ckks_key *key, int64_t t, uint64_t *ct_b, uint64_t *ct_a, size_t batch, fhe_mem mem,
                    void *stream);
/* scheme/ckks/src/ckks.rs:250-263 `Ckks::mul(param, rlk, ct0, ct1)`: tensor, relinearisation (ckks.rs:265-272) and the closing
 * `rescale()`.  ct0_*, ct1_* [batch][L][n] over qs, coefficient domain -> out_b, out_a [batch][L-1][n] over qs[0..L-1).
 * The inputs are transformed once and stay in the evaluation domain through the tensor (7 L transforms + the key switch where
 * the reference's four `Rq * Rq` take 12 L).  A ciphertext on fewer limbs multiplies through an fhe_rns_ctx over that prefix of
 * qs (rns.rs:148-158 multiplies on the intersection of the two limb sets). */
int fhe_ckks_mul(const fhe_rns_ctx *rns, const fhe_ckks_key *rlk, const uint64_t *ct0_b, const uint64_t *ct0_a, const uint64_t *ct1_b,
                 const uint64_t *ct1_a, uint64_t *out_b, uint64_t *out_a, size_t batch, fhe_mem mem, void *stream);


/* ---- TFHE torus path (row T), k = 1: fused kernels (any rank k: the fhe_*k_* entries further down) ---------- */
/* Torus data are uint64_t values of Z/2^64 (util/src/torus.rs `T64`).  Where the reference multiplies torus polynomials
 * with an f64 FFT (util/src/ring/fft/c64.rs:11-56, error <= 2^(64+log_b+log_n-53), c64.rs:186-208), this backend returns
 * the EXACT product (both operands read as signed 64-bit integers, as c64.rs:23-27 does): never less exact than the
 * reference, identical at decode level. */
typedef struct fhe_torus_ctx fhe_torus_ctx;   /* two 60-bit NTT primes + CRT constants */
typedef struct fhe_tggsw_key fhe_tggsw_key;   /* prepared TGGSW ciphertexts (bootstrapping key) */
int fhe_torus_ctx_create(int device, fhe_torus_ctx **out);
void fhe_torus_ctx_destroy(fhe_torus_ctx *t);
/* util/src/misc/decompose.rs:66-81, 114-135 `Base2Decomposor::<T64>::new(log_b, d).decompose(poly)`: [polys][n] ->
 * [polys][d][n] signed digits as two's-complement uint64_t, least significant first.  Bit-exact. */
int fhe_torus_decompose(int log_b, int d, const uint64_t *in, size_t n, size_t polys, uint64_t *out, fhe_mem mem, void *stream);
/* util/src/ring.rs:315-320 `Rt *= &Rt`: a <- a * b in Z_{2^64}[X]/(X^n+1), exact; |b_i| < 2^log_bound_b with
 * n * 2^(64 + log_bound_b) < 2^118 (gadget digits, small secrets: what the reference's FFT product is used for). */
int fhe_torus_mul(const fhe_torus_ctx *t, uint64_t *a, const uint64_t *b, int log_bound_b, size_t n, size_t batch, fhe_mem mem,
                  void *stream);
/* `count` TGGSW ciphertexts (scheme/tfhe/src/tggsw.rs:44-88): rows_a / rows_b [count][2d][n].  n = 256 .. 2048.  The exact products run on
 * one of three forms chosen from the gadget: key words cut into three signed pieces through f64 transforms whose rounded results are exact
 * (2d n 2^log_b <= 2^21, base <= 2^7: BASELINE config 5), three 30-bit NTT primes (2d n 2^(62 + log_b) < 2^88), two 60-bit primes
 * (< 2^118; beyond that FHE_ERR_UNSUPPORTED).  All three give the same bits. */
int fhe_tggsw_prepare(const fhe_torus_ctx *t, int log_b, int d, const uint64_t *rows_a, const uint64_t *rows_b, size_t n, size_t count,
                      fhe_mem mem, fhe_tggsw_key **out);
void fhe_tggsw_key_destroy(fhe_tggsw_key *key);
/* The same key prepared for the f64 FFT product the reference itself computes with (util/src/ring/fft/c64.rs:11-56: fold N reals into
 * N/2 complex values, transform, multiply, transform back, `f64_mod_u64`).  Every entry point below that takes the key (external
 * product, cmux, blind rotation, bootstrap) then runs that mode: one pass of half-size complex transforms where the exact path runs
 * three passes of 30-bit ones.  NOT exact and not bit-reproducible against anything (the reference's own low bits depend on its
 * libm): per product |result - exact| <= 2^(64 + log_b + log2 n - 53), the reference's own bound (c64.rs:186-208); decode-level
 * results agree.  The exact mode (fhe_tggsw_prepare) stays the default and the parity checker. */
int fhe_tggsw_prepare_fft64(const fhe_torus_ctx *t, int log_b, int d, const uint64_t *rows_a, const uint64_t *rows_b, size_t n, size_t count,
                            fhe_mem mem, fhe_tggsw_key **out);
/* A key of capacity `count` for ciphertexts that are fresh in every call (CMUX selectors out of a circuit bootstrap), where
 * fhe_tggsw_prepare's allocation, copy, null stream and host wait per call would be in the way.  The form is the one fhe_tggsw_prepare
 * chooses for (log_b, d, n), or with fft64 != 0 the one of fhe_tggsw_prepare_fft64; the contents are undefined until filled.  Status
 * as those entries. */
int fhe_tggsw_key_reserve(const fhe_torus_ctx *t, int log_b, int d, size_t n, size_t count, int fft64, fhe_tggsw_key **out);
/* Transforms `count` ciphertexts, rows_a / rows_b [count][2d][n] of the key's ring and gadget, into the slots first_index ..
 * first_index + count - 1 of `key`, on `stream`.  FHE_MEM_DEVICE calls neither allocate with hipMalloc nor wait on the host (scratch is
 * stream ordered).  Afterwards every entry that takes the key gives, for the filled indices, the bits it gives under fhe_tggsw_prepare /
 * _prepare_fft64 of the same rows.  The caller orders the fill against work on OTHER streams that still reads those slots.
 * first_index + count beyond the key's capacity, a NULL key, NULL rows with count > 0: FHE_ERR_INVALID. */
int fhe_tggsw_key_fill(fhe_tggsw_key *key, size_t first_index, const uint64_t *rows_a, const uint64_t *rows_b, size_t count, fhe_mem mem,
                       void *stream);
/* Which form a prepared or reserved key is in (read-only; for tests and tools: every exact form gives the same bits). */
enum {
    FHE_TGGSW_FORM_60 = 0,     /* two 60-bit NTT primes */
    FHE_TGGSW_FORM_30 = 1,     /* three 30-bit NTT primes */
    FHE_TGGSW_FORM_FFT64 = 2,  /* the f64 FFT product of fhe_tggsw_prepare_fft64 (not exact) */
    FHE_TGGSW_FORM_X3 = 3      /* three key pieces through f64 transforms, exact */
};
/* *form: one of FHE_TGGSW_FORM_*.  *packs_digits: 1 exactly when a blind rotation or a look-up ladder launched NOW on this key would run
 * the 30-bit CMUX whose digits are computed once and parked as bytes (form 30, base <= 2^7, 2d <= 8, lab switch NO_PACKED_DIGITS off: the
 * switch is read as the launch reads it), else 0.  A NULL key or a NULL output: FHE_ERR_INVALID.  Touches no device. */
int fhe_tggsw_key_form(const fhe_tggsw_key *key, int *form, int *packs_digits);
/* Workgroups per ciphertext (*g_out = 1, 2 or 6) that a blind rotation of `batch` ciphertexts under brk would use with the options as
 * they are ("TFHE_SPLIT"): fhe_tfhe_blind_rotate, _tables and every entry that contains one (fhe_tfhe_bootstrap, _tables, _many, the
 * circuits, the circuit bootstrap, fhe_tfhe_wop_pbs) ask the same rule.  Above 1 a cluster of workgroups owns each ciphertext: each
 * member computes one output of every CMUX (2) or one key piece of one output (6) and the members add each other's shares inside the
 * launch -- lower latency at batches that leave the chip idle, bit-identical results.  Eligible: a key in the x3 form at n = 1024 and
 * batch x G <= compute units.  The waits are bounded: one that runs out writes no output and the call reports FHE_ERR_TIMEOUT --
 * fhe_tfhe_blind_rotate, _tables, fhe_tfhe_bootstrap, _tables and _many on host memory in their return value (a word of the call's own),
 * everything else through fhe_tggsw_key_status.  Touches no device beyond the context's compute-unit count.  A NULL argument, or a key
 * of another context: FHE_ERR_INVALID. */
int fhe_tfhe_blind_rotate_split(const fhe_torus_ctx *t, const fhe_tggsw_key *brk, size_t batch, int *g_out);
/* Waits for everything enqueued on `stream`, then FHE_ERR_TIMEOUT if a split blind rotation of a device-memory call on this key gave up
 * a wait since the word was last cleared, else FHE_OK; clear != 0 resets the word (in stream order).  The word lives with the key;
 * host-memory calls neither set nor clear it.  A key in a form that never splits is always FHE_OK. */
int fhe_tggsw_key_status(const fhe_tggsw_key *key, void *stream, int clear);
/* scheme/tfhe/src/tggsw.rs:100-112 `Tggsw::external_product(param, key[index], ct)`, in place on [batch][n] a / b. */
int fhe_tggsw_external_product(const fhe_torus_ctx *t, const fhe_tggsw_key *key, size_t index, uint64_t *ct_a, uint64_t *ct_b,
                               size_t batch, fhe_mem mem, void *stream);
/* scheme/tfhe/src/bootstrapping.rs:99-104 `mod_switch`: rounding_shr(v, 64 - log2(2 big_n)) for `count` torus values. */
int fhe_tfhe_mod_switch(const uint64_t *in, uint64_t *out, size_t count, size_t big_n, fhe_mem mem, void *stream);
/* scheme/tfhe/src/tggsw.rs:114-121 `Tggsw::cmux(key[index], ct0, ct1)` = ct0 + external_product(key[index], ct1 - ct0) for `batch`
 * pairs of TGLWE ciphertexts, [batch][n] each; out may alias ct0 or ct1. */
int fhe_tggsw_cmux(const fhe_torus_ctx *t, const fhe_tggsw_key *key, size_t index, const uint64_t *ct0_a, const uint64_t *ct0_b,
                   const uint64_t *ct1_a, const uint64_t *ct1_b, uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem, void *stream);
/* scheme/tfhe/src/tglwe.rs:61-66 `TglweCiphertext::rotate(i)`: both halves times X^i (util/src/ring.rs:299-313 on T64), any
 * integer i (taken mod 2n); ct, out [batch][n], out != ct. */
int fhe_tglwe_rotate(const uint64_t *ct_a, const uint64_t *ct_b, size_t n, int64_t i, uint64_t *out_a, uint64_t *out_b, size_t batch,
                     fhe_mem mem, void *stream);
/* scheme/tfhe/src/bootstrapping.rs:84-96 `blind_rotate`: n_lwe CMUXes (tggsw.rs:114-121) per ciphertext.  a_tilde
 * [batch][n_lwe], b_tilde [batch]: mod-switched TLWE ciphertexts; v [n]: the encoded test polynomial; out [batch][n]. */
int fhe_tfhe_blind_rotate(const fhe_torus_ctx *t, const fhe_tggsw_key *brk, const uint64_t *a_tilde, const uint64_t *b_tilde,
                          const uint64_t *v, uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem, void *stream);
/* scheme/tfhe/src/tglwe.rs:115-127 `Tglwe::sample_extract(ct, index)`. */
int fhe_tglwe_sample_extract(const uint64_t *ct_a, const uint64_t *ct_b, size_t n, size_t index, uint64_t *out_a, uint64_t *out_b,
                             size_t batch, fhe_mem mem, void *stream);
/* scheme/tfhe/src/tlwe.rs:144-153 `Tlwe::key_switch`: ksk_a [n_in*d][n_out], ksk_b [n_in*d], rows digit-major. */
int fhe_tlwe_key_switch(int log_b, int d, const uint64_t *ksk_a, const uint64_t *ksk_b, const uint64_t *ct_a, const uint64_t *ct_b,
                        size_t n_in, size_t n_out, uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem, void *stream);
/* scheme/tfhe/src/bootstrapping.rs:78-82 `Bootstrapping::bootstrap(bsk, v, ct)` for `batch` TLWE ciphertexts in one call:
 * mod switch (99-104) -> blind rotation (84-96) -> sample_extract(0) -> key switch, on `stream`.  lwe_a [batch][n_lwe], lwe_b
 * [batch] (n_lwe = number of TGGSW ciphertexts in brk), v [n] the encoded test polynomial, ksk as in fhe_tlwe_key_switch with
 * n_in = n, n_out = n_lwe; out_a [batch][n_lwe], out_b [batch].  Bit-identical to the four calls above chained. */
int fhe_tfhe_bootstrap(const fhe_torus_ctx *t, const fhe_tggsw_key *brk, int ks_log_b, int ks_d, const uint64_t *ksk_a,
                       const uint64_t *ksk_b, const uint64_t *v, const uint64_t *lwe_a, const uint64_t *lwe_b, uint64_t *out_a,
                       uint64_t *out_b, size_t batch, fhe_mem mem, void *stream);
/* scheme/tfhe/src/bootstrapping.rs:84-96 `blind_rotate` with one test polynomial PER CIPHERTEXT (bootstrapping.rs:118-128 `table` builds
 * one per function, 141-165 bootstraps through three of them): tables [n_tables][n] encoded, table_of [batch]; ciphertext i rotates
 * tables[table_of[i]].  n_tables <= 65536.  The result for ciphertext i is bit-identical, in every key form, to fhe_tfhe_blind_rotate
 * with v = tables[table_of[i]].  Host memory: an index >= n_tables is FHE_ERR_INVALID.  Device memory: the caller guarantees
 * table_of[i] < n_tables; the kernels clamp nothing. */
int fhe_tfhe_blind_rotate_tables(const fhe_torus_ctx *t, const fhe_tggsw_key *brk, const uint64_t *a_tilde, const uint64_t *b_tilde,
                                 const uint64_t *tables, size_t n_tables, const uint32_t *table_of, uint64_t *out_a, uint64_t *out_b,
                                 size_t batch, fhe_mem mem, void *stream);
/* scheme/tfhe/src/bootstrapping.rs:78-82 `Bootstrapping::bootstrap` through tables[table_of[i]] for ciphertext i; tables and indices as
 * above, everything else as fhe_tfhe_bootstrap, whose bits it reproduces table by table. */
int fhe_tfhe_bootstrap_tables(const fhe_torus_ctx *t, const fhe_tggsw_key *brk, int ks_log_b, int ks_d, const uint64_t *ksk_a,
                              const uint64_t *ksk_b, const uint64_t *tables, size_t n_tables, const uint32_t *table_of,
                              const uint64_t *lwe_a, const uint64_t *lwe_b, uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem,
                              void *stream);
/* scheme/tfhe/src/tlwe.rs:22-75 (Add, Sub, Neg and scalar Mul on `TlweCiphertext`, composed): out = constant + sum_{j < k} weight[j] * ct_j
 * over Z/2^64, wrapping; in_a[j] [batch][n], in_b[j] [batch]; the constant is added to b only.  1 <= k <= 16.  out must not overlap an
 * input. */
int fhe_tlwe_lincomb(int k, const int32_t *weight, const uint64_t *const *in_a, const uint64_t *const *in_b, uint64_t constant,
                     uint64_t *out_a, uint64_t *out_b, size_t n, size_t batch, fhe_mem mem, void *stream);

/* ---- TFHE torus path at any TGLWE rank k (the reference's `TglweParam::n`: tglwe.rs:11-35; its TGLWE / TGGSW tests run at k = 2,
 * N = 256, base 2^8, d = 8: tglwe.rs:138-166, tggsw.rs:134-181) ------------------------------------------------------------- */
/* A rank-k TGLWE ciphertext is ONE buffer [k + 1][n]: a_0 .. a_{k-1}, b (tglwe.rs:49-50 `TglweCiphertext(AVec<Rt>, Rt)`); a TGGSW
 * ciphertext is (k + 1) d of them in the order tggsw.rs:80-87 builds (message on a_0: d rows, .., on a_{k-1}, on b).  Products are
 * the exact ones of the k = 1 entries; k = 1 through these entries gives bit-identical results.  1 <= k <= 8, n = 2 .. 2^15. */
typedef struct fhe_tggswk_key fhe_tggswk_key;
/* The form a prepared rank-k key is in.  Both are exact: every entry below gives the same bits on either.  X3: fused kernels, one launch
 * per entry with the ciphertext in registers (three key pieces through f64 transforms, as FHE_TGGSW_FORM_X3 at k = 1); a key takes it
 * exactly when k = 2 or 3, n = 256 .. 1024, log_b <= 7, log_b d <= 31, (k + 1) d <= 16, (k + 1) d n 2^log_b <= 2^21 and the lab switch
 * "NO_RANKK_FUSED" is 0.  COMPOSED: streaming kernels around batched transforms, any admitted rank and ring. */
enum {
    FHE_TGGSWK_FORM_COMPOSED = 0,
    FHE_TGGSWK_FORM_X3 = 1
};
/* rows [count][(k + 1) d][k + 1][n] -> prepared (evaluation-domain) key; FHE_ERR_INVALID: k < 1, n not a power of two, log_b outside
 * 1 .. 63, d outside 1 .. 64; FHE_ERR_UNSUPPORTED: k > 8, n outside 2 .. 2^15, (k + 1) d n 2^(62 + log_b) >= 2^118 */
int fhe_tggswk_prepare(const fhe_torus_ctx *t, int k, int log_b, int d, const uint64_t *rows, size_t n, size_t count, fhe_mem mem,
                       fhe_tggswk_key **out);
void fhe_tggswk_key_destroy(fhe_tggswk_key *key);
/* *form: FHE_TGGSWK_FORM_*, the form `key` was prepared in */
int fhe_tggswk_key_form(const fhe_tggswk_key *key, int *form);
/* *form: the form fhe_tggswk_prepare would give a key of this shape if it were called now (the lab switch is read at this call).  Host
 * only: no device is needed.  FHE_ERR_INVALID / FHE_ERR_UNSUPPORTED on the arguments fhe_tggswk_prepare refuses with them. */
int fhe_tggswk_form_for(int k, size_t n, int log_b, int d, int *form);
/* tggsw.rs:100-112 `Tggsw::external_product(param, key[index], ct)`, in place on ct [batch][k + 1][n] */
int fhe_tggswk_external_product(const fhe_torus_ctx *t, const fhe_tggswk_key *key, size_t index, uint64_t *ct, size_t batch, fhe_mem mem,
                                void *stream);
/* tggsw.rs:114-121 `Tggsw::cmux(key[index], ct0, ct1)`; [batch][k + 1][n] each, out may alias ct0 or ct1 */
int fhe_tggswk_cmux(const fhe_torus_ctx *t, const fhe_tggswk_key *key, size_t index, const uint64_t *ct0, const uint64_t *ct1, uint64_t *out,
                    size_t batch, fhe_mem mem, void *stream);
/* tglwe.rs:61-66 `TglweCiphertext::rotate(i)`; ct, out [batch][k + 1][n], out != ct */
int fhe_tglwek_rotate(const uint64_t *ct, int k, size_t n, int64_t i, uint64_t *out, size_t batch, fhe_mem mem, void *stream);
/* tglwe.rs:115-127 `Tglwe::sample_extract(ct, index)`: a TLWE ciphertext of dimension k n: out_a [batch][k n], out_b [batch] */
int fhe_tglwek_sample_extract(const uint64_t *ct, int k, size_t n, size_t index, uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem,
                              void *stream);
/* bootstrapping.rs:84-96 `blind_rotate`: a_tilde [batch][n_lwe], b_tilde [batch] mod-switched, v [n] encoded -> out [batch][k + 1][n] */
int fhe_tfhek_blind_rotate(const fhe_torus_ctx *t, const fhe_tggswk_key *brk, const uint64_t *a_tilde, const uint64_t *b_tilde, const uint64_t *v,
                           uint64_t *out, size_t batch, fhe_mem mem, void *stream);
/* bootstrapping.rs:78-82 `Bootstrapping::bootstrap`: mod switch -> blind rotation -> sample_extract(0) -> key switch with
 * n_in = k n, n_out = n_lwe (ksk_a [k n ks_d][n_lwe], ksk_b [k n ks_d]); lwe_a, out_a [batch][n_lwe], lwe_b, out_b [batch] */
int fhe_tfhek_bootstrap(const fhe_torus_ctx *t, const fhe_tggswk_key *brk, int ks_log_b, int ks_d, const uint64_t *ksk_a, const uint64_t *ksk_b,
                        const uint64_t *v, const uint64_t *lwe_a, const uint64_t *lwe_b, uint64_t *out_a, uint64_t *out_b, size_t batch,
                        fhe_mem mem, void *stream);
/* fhe_tfhek_blind_rotate with one test polynomial PER CIPHERTEXT: tables [n_tables][n] encoded, table_of [batch] (NULL: every ciphertext
 * takes tables[0]); ciphertext i rotates tables[table_of[i]] and gets the bits of fhe_tfhek_blind_rotate with that table, in either key
 * form.  n_tables <= 65536.  Host memory: an index >= n_tables is FHE_ERR_INVALID.  Device memory: the caller guarantees
 * table_of[i] < n_tables; the kernels clamp nothing. */
int fhe_tfhek_blind_rotate_tables(const fhe_torus_ctx *t, const fhe_tggswk_key *brk, const uint64_t *a_tilde, const uint64_t *b_tilde,
                                  const uint64_t *tables, size_t n_tables, const uint32_t *table_of, uint64_t *out, size_t batch, fhe_mem mem,
                                  void *stream);
/* fhe_tfhek_bootstrap through tables[table_of[i]] for ciphertext i; tables and indices as above */
int fhe_tfhek_bootstrap_tables(const fhe_torus_ctx *t, const fhe_tggswk_key *brk, int ks_log_b, int ks_d, const uint64_t *ksk_a,
                               const uint64_t *ksk_b, const uint64_t *tables, size_t n_tables, const uint32_t *table_of, const uint64_t *lwe_a,
                               const uint64_t *lwe_b, uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem, void *stream);

/* ---- key material on the device ------------------------------------------------- */
/* Randomness.  Every producer below draws from an `fhe_rng`: a 256-bit ChaCha20 key.  Value i of a draw is a word of ChaCha20
 * block (i / words per block) -- counter based: every GPU lane finds its value without shared state, a draw is reproducible and
 * order independent -- under a PER-CALL key derived from (generator key, stream_id, the entry point's purpose tag), so different
 * entry points never share keystream even when a caller reuses a stream id: a secret key drawn with fhe_sample_binary(rng, 7) has
 * nothing in common with the public mask of fhe_tlwe_sk_encrypt(rng, 7).  What the caller MUST still guarantee: two calls of the
 * SAME entry point on the same generator use different stream ids (equal ids reproduce the same mask and the same noise:
 * b1 - b2 = pt1 - pt2).  Pass FHE_STREAM_AUTO to let the generator number the calls itself (fresh id per call, from its own
 * counter, in the upper half of the id space: keep explicit ids below 2^63 when mixing both).  The reference draws from
 * `thread_rng()`; draws are not parity relevant.  These entry points are validated at decrypt level, and row by row: with the secret
 * key known, the exact noise of every coefficient they produce is checked against the sampler's support and law, the gadget term
 * of every digit, limb and component exactly, and no two rows of a key may share noise (tests/test_keygen_rows_gpu.py).
 *   fhe_rng_create(key32, &rng): key32 = 32 bytes of caller entropy, or NULL = 32 bytes from the operating system (getrandom),
 *                                what the reference's thread_rng() is seeded with.
 *   fhe_rng_create_from_seed:    TESTS AND REPRODUCIBLE RUNS ONLY -- 64 bits of entropy stretched to a key (SplitMix64); keys made
 *                                from it are as strong as the seed, never stronger.
 *   fhe_chacha20_block:          the block function alone (host), for known-answer tests: ChaCha20 in the original layout, 64-bit
 *                                block counter and 64-bit nonce (RFC 8439's function with its 32/96-bit split undone). */
typedef struct fhe_rng fhe_rng;
#define FHE_STREAM_AUTO UINT64_MAX
int fhe_rng_create(const uint8_t *key32, fhe_rng **out);
int fhe_rng_create_from_seed(uint64_t seed, fhe_rng **out);
void fhe_rng_destroy(fhe_rng *rng);
int fhe_chacha20_block(const uint8_t *key32, uint64_t nonce, uint64_t counter, uint8_t *out64);
/* util/src/zq.rs:91-93 `Zq::sample_uniform`: `count` values uniform in [0, q) */
int fhe_sample_uniform(uint64_t q, const fhe_rng *rng, uint64_t stream_id, uint64_t *out, size_t count, fhe_mem mem, void *stream);
/* util/src/torus.rs `T64::sample_uniform`: uniform 64-bit torus values */
int fhe_sample_torus(const fhe_rng *rng, uint64_t stream_id, uint64_t *out, size_t count, fhe_mem mem, void *stream);
/* util/src/misc/distribution.rs:23-46 `dg(std_dev, n)` (weights from the reference's erf approximation, support
 * [-floor(n std_dev), floor(n std_dev)]) as `Zq::sample_i64` (zq.rs:95-97); q = 0: plain two's-complement integers */
int fhe_sample_dg(uint64_t q, double std_dev, int n_sigma, const fhe_rng *rng, uint64_t stream_id, uint64_t *out, size_t count, fhe_mem mem,
                  void *stream);
/* util/src/misc/decompose.rs:35-40 `power_up`: out[p][j] = in[p] * 2^(rounding_bits + j log_b) mod q, [polys][d][n] */
int fhe_power_up(uint64_t q, int log_b, int d, const uint64_t *in, size_t n, size_t polys, uint64_t *out, fhe_mem mem, void *stream);
/* scheme/fhew/src/rlwe.rs:146-156 `Rlwe::sk_encrypt` for `batch` plaintexts (pt [batch][n] or NULL = zeros): a uniform,
 * e <- dg(3.2, 6), b = a sk + e + pt.  sk [n]: the secret key as Zq values (`Zq::from_i64` of its coefficients).  n = 1 is taken
 * (Z_q itself, as in fhe_mul); the key and share producers below need n >= 2. */
int fhe_rlwe_sk_encrypt(const fhe_ctx *ctx, const uint64_t *sk, const uint64_t *pt, size_t n, size_t batch, const fhe_rng *rng, uint64_t stream_id, uint64_t *ct_a, uint64_t *ct_b, fhe_mem mem, void *stream);
/* rlwe.rs:237-249 `Rlwe::share_encrypt(param, a, sk, pt)`: b = a sk + e + pt for a GIVEN mask a -- what the multi-party protocol of
 * rlwe.rs:205-324 is made of: `pk_share_gen` (pt NULL, a = the common reference string), `ksk_share_gen` / `ak_share_gen` (one row per
 * call of the gadget), `share_decrypt` (pt NULL, a = the ciphertext's mask); the merges are fhe_rq_sum / fhe_rq_sub.  a [a_rows][n] with
 * a_rows = rows or 1 (one polynomial shared by every row); sk [n] as Zq values; pt [rows][n] or NULL; out_b [rows][n]. */
int fhe_rlwe_share_encrypt(const fhe_ctx *ctx, const uint64_t *a, size_t a_rows, const uint64_t *sk, const uint64_t *pt, size_t n, size_t rows,
                           const fhe_rng *rng, uint64_t stream_id, uint64_t *out_b, fhe_mem mem, void *stream);
/* rlwe.rs:158-170 `Rlwe::pk_encrypt`: u <- zo(0.5), e0, e1 <- dg(3.2, 6) per ciphertext; a = pk.a u + e0, b = pk.b u + e1 + pt.  pk_a, pk_b
 * [n] (rlwe.rs:98-101 `pk_gen` = fhe_rlwe_sk_encrypt of zero, or a merged multi-party key); pt [batch][n] or NULL. */
int fhe_rlwe_pk_encrypt(const fhe_ctx *ctx, const uint64_t *pk_a, const uint64_t *pk_b, const uint64_t *pt, size_t n, size_t batch, const fhe_rng *rng,
                        uint64_t stream_id, uint64_t *ct_a, uint64_t *ct_b, fhe_mem mem, void *stream);
/* rlwe.rs:172-175 `Rlwe::decrypt`: pt = b - a sk; [batch][n]; pt may alias ct_b. */
int fhe_rlwe_decrypt(const fhe_ctx *ctx, const uint64_t *sk, const uint64_t *ct_a, const uint64_t *ct_b, size_t n, size_t batch, uint64_t *pt,
                     fhe_mem mem, void *stream);
/* scheme/fhew/src/rgsw.rs:84-105 `Rgsw::sk_encrypt` of `count` plaintext polynomials (pt [count][n], `Rgsw::encode`d):
 * rows_a / rows_b [count][2d][n], the layout fhe_rgsw_prepare takes. */
int fhe_rgsw_encrypt(const fhe_ctx *ctx, int log_b, int d, const uint64_t *sk, const uint64_t *pt, size_t n, size_t count,
                     const fhe_rng *rng, uint64_t stream_id, uint64_t *rows_a, uint64_t *rows_b, fhe_mem mem, void *stream);
/* rgsw.rs:75-83 `Rgsw::pk_encrypt`: as fhe_rgsw_encrypt with the 2d encryptions of zero made by fhe_rlwe_pk_encrypt (what the reference's
 * RGSW tests encrypt with; `Bootstrapping::key_share_gen`, bootstrapping.rs:277-283, under the merged public key). */
int fhe_rgsw_pk_encrypt(const fhe_ctx *ctx, int log_b, int d, const uint64_t *pk_a, const uint64_t *pk_b, const uint64_t *pt, size_t n, size_t count,
                        const fhe_rng *rng, uint64_t stream_id, uint64_t *rows_a, uint64_t *rows_b, fhe_mem mem, void *stream);
/* scheme/fhew/src/rlwe.rs:109-120 `Rlwe::ksk_gen(param, sk0, sk1)` (t = 0) and 122-132 `Rlwe::ak_gen(param, t, sk0)` (t != 0,
 * sk1 ignored: the key switches sk0(X^t) back to sk0): rows_a / rows_b [d][n], the layout fhe_ksk_prepare takes. */
int fhe_rlwe_ksk_gen(const fhe_ctx *ctx, int log_b, int d, const uint64_t *sk0, const uint64_t *sk1, int64_t t, size_t n,
                     const fhe_rng *rng, uint64_t stream_id, uint64_t *rows_a, uint64_t *rows_b, fhe_mem mem, void *stream);
/* scheme/fhew/src/lwe.rs:128-139 `Lwe::sk_encrypt` for `rows` plaintexts over any modulus q < 2^62 (pt [rows] or NULL = zeros):
 * out_a [rows][n] uniform, out_b[r] = <a[r], sk> + pt[r] + e[r], e <- dg(3.2, 6). */
int fhe_lwe_sk_encrypt(uint64_t q, const uint64_t *sk, const uint64_t *pt, size_t n, size_t rows, const fhe_rng *rng, uint64_t stream_id,
                       uint64_t *out_a, uint64_t *out_b, fhe_mem mem, void *stream);
/* scheme/fhew/src/lwe.rs:108-119 `Lwe::ksk_gen(param, sk0, sk1)`: ksk_a [n1 d][n0], ksk_b [n1 d] (digit-major rows), the layout
 * fhe_lwe_key_switch / fhe_fhew_bootstrap take with n_in = n1, n_out = n0. */
int fhe_lwe_ksk_gen(uint64_t q, int log_b, int d, const uint64_t *sk0, size_t n0, const uint64_t *sk1, size_t n1, const fhe_rng *rng, uint64_t stream_id, uint64_t *ksk_a, uint64_t *ksk_b, fhe_mem mem, void *stream);
/* lwe.rs:169-183 `Lwe::sk_share_encrypt(param, a, sk, pt)` / 197-207 `share_decrypt` (pt NULL): b[r] = <a[r], sk> + pt[r] + e[r] for GIVEN
 * masks a [rows][n] (a common reference string, or a ciphertext's mask); the merges (lwe.rs:185-195, 209-212) are sums (fhe_rq_sum). */
int fhe_lwe_share_encrypt(uint64_t q, const uint64_t *a, const uint64_t *sk, const uint64_t *pt, size_t n, size_t rows, const fhe_rng *rng,
                          uint64_t stream_id, uint64_t *out_b, fhe_mem mem, void *stream);
/* lwe.rs:214-226 `Lwe::ksk_share_gen(param, crs, sk0, sk1)`: crs [n1 d][n0] is the ksk_a every party (and the merged key) uses; out_b [n1 d];
 * the merged key-switching key is (crs, fhe_rq_sum of the shares) (lwe.rs:228-237). */
int fhe_lwe_ksk_share_gen(uint64_t q, int log_b, int d, const uint64_t *crs, const uint64_t *sk0, size_t n0, const uint64_t *sk1, size_t n1,
                          const fhe_rng *rng, uint64_t stream_id, uint64_t *out_b, fhe_mem mem, void *stream);
/* util/src/ring.rs:328-341 `Rq: Sum`: out[i] = sum_k in[k][i] mod q, in [count][len] (callers used to loop fhe_rq_add) */
int fhe_rq_sum(uint64_t q, const uint64_t *in, size_t len, size_t count, uint64_t *out, fhe_mem mem, void *stream);
/* ---- CKKS key material (scheme/ckks/src/ckks.rs:139-183, 215-225).  Secret keys are two's-complement i64 vectors. */
/* util/src/misc/distribution.rs:10-21 `zo(rho)` (ckks.rs:139-141 `Ckks::sk_gen`: rho = 0.5): -1 / +1 / 0 as i64 */
int fhe_sample_zo(double rho, const fhe_rng *rng, uint64_t stream_id, uint64_t *out, size_t count, fhe_mem mem, void *stream);
/* ckks.rs:215-225 `Ckks::sk_encrypt` for `batch` plaintexts over qs (extended = 0) or qs ++ ps: b = -(a sk) + e + pt, a uniform,
 * e <- dg(3.2, 6).  pt [batch][limbs][n] or NULL (zeros: ckks.rs:143-146 `pk_gen`); out_b, out_a [batch][limbs][n]. */
int fhe_ckks_sk_encrypt(const fhe_rns_ctx *rns, int extended, const uint64_t *sk, const uint64_t *pt, size_t n, size_t batch, const fhe_rng *rng, uint64_t stream_id, uint64_t *out_b, uint64_t *out_a, fhe_mem mem, void *stream);
/* ckks.rs:154-161 `Ckks::ksk_gen(param, sk, sk_prime)` -> ksk_b, ksk_a [L+K][n] for fhe_ckks_ksk_prepare.  sk_prime NULL: sk^2
 * (ckks.rs:163-166 `rlk_gen`), squared on the device -- exact while n max|sk_i|^2 < q_0 / 2 (every `zo` key), checked: FHE_ERR_INVALID otherwise; `cjk_gen` / `rtk_gen` (ckks.rs:168-183): sk_prime = sk(X^t), t = -1 / 5^j. */
int fhe_ckks_ksk_gen(const fhe_rns_ctx *rns, const uint64_t *sk, const uint64_t *sk_prime, size_t n, const fhe_rng *rng, uint64_t stream_id,
                     uint64_t *ksk_b, uint64_t *ksk_a, fhe_mem mem, void *stream);

/* ckks.rs:227-238 `Ckks::pk_encrypt` for `batch` plaintexts over qs: u <- zo(0.5), e0, e1 <- dg(3.2, 6) per ciphertext; a = pk.a u + e0,
 * b = pk.b u + e1 + pt.  pk_b, pk_a [L][n]: ckks.rs:143-146 `pk_gen` = fhe_ckks_sk_encrypt with pt NULL.  pt [batch][L][n] or NULL. */
int fhe_ckks_pk_encrypt(const fhe_rns_ctx *rns, const uint64_t *pk_b, const uint64_t *pk_a, const uint64_t *pt, size_t n, size_t batch,
                        const fhe_rng *rng, uint64_t stream_id, uint64_t *out_b, uint64_t *out_a, fhe_mem mem, void *stream);
/* ckks.rs:240-248 `Ckks::decrypt`: pt = b + a sk over qs; sk [n] i64; ct_b, ct_a, pt [batch][L][n]; pt may alias ct_b.  (A ciphertext on
 * fewer limbs decrypts through an fhe_rns_ctx over that prefix of qs.) */
int fhe_ckks_decrypt(const fhe_rns_ctx *rns, const uint64_t *sk, const uint64_t *ct_b, const uint64_t *ct_a, size_t n, size_t batch, uint64_t *pt,
                     fhe_mem mem, void *stream);
/* ckks.rs:250-253 `Ckks::mul_constant` after its `encode` (fhe_ckks_encode below): (pt * b, pt * a).rescale().  pt
 * [pt_batch][L][n] encoded plaintexts, pt_batch = 1 (one constant for the batch) or batch; ct [batch][L][n] -> out [batch][L-1][n]. */
int fhe_ckks_mul_plain(const fhe_rns_ctx *rns, const uint64_t *pt, size_t pt_batch, const uint64_t *ct_b, const uint64_t *ct_a, uint64_t *out_b,
                       uint64_t *out_a, size_t n, size_t batch, fhe_mem mem, void *stream);

/* ---- scheme/ckks/src/bootstrapping.rs:90-108 `Bootstrapping::mul_mat`: a diagonal-sparse plaintext matrix times a ciphertext by
 * baby-step / giant-step (index sets: util/src/misc/matrix.rs:45-52, 125-150),
 *     out = sum_i rotate_i( sum_{j in js(i)} mul_constant(diag_rot(i, j), rotate_j(ct)) ),          rotate_0 = identity,
 * as one entry over a matrix prepared once.  Bit-identical to the composition of fhe_ckks_rotate, fhe_ckks_mul_plain and fhe_rns_add
 * in the reference's order, with every operand transformed once: the sum over j runs in the evaluation domain on limbs 0 .. L-2 and
 * is rescaled once per giant step (only the last limb keeps every term on its own).
 *   rns_hi      the context of the input ciphertext, L >= 2 limbs;
 *   rns_lo      the caller's context over the prefix qs[0 .. L-1) with the same ps on the same device (FHE_ERR_INVALID otherwise): the
 *               level the giant steps and the result live on;
 *   giant, baby the i of the split and the union of all j, each strictly ascending, 0 allowed (no rotation); the rotation amounts
 *               5^i, 5^j mod 2n (`CkksParam::pow5`) are computed here;
 *   present     [n_giant][n_baby], non-zero where (i, j) is a term; no term at all is FHE_ERR_INVALID;
 *   diags       [terms][L][n], row-major over the present (i, j): `Ckks::encode(diag_rot(i, j))`, coefficient domain over rns_hi's qs
 *               (fhe_ckks_encode makes them; the rotation of the diagonal by -i stays with the caller).  Transformed once and kept on the
 *               device;
 *   baby_keys   [n_baby] rotation keys for j prepared on rns_hi, NULL where j == 0;
 *   giant_keys  [n_giant] rotation keys for i prepared on rns_lo (the same coefficient-domain key with limb L-1 removed: what the
 *               reference's key switch uses at the lower level, rns.rs:148-158), NULL where i == 0.
 * A missing key or one bound to another context is FHE_ERR_INVALID.  The keys are BORROWED: they and both contexts must outlive the
 * matrix.  `mem` says where `diags` lives. */
typedef struct fhe_ckks_diag_matrix fhe_ckks_diag_matrix;
int fhe_ckks_diag_matrix_prepare(const fhe_rns_ctx *rns_hi, const fhe_rns_ctx *rns_lo, size_t n, const uint32_t *giant, int n_giant,
                                 const uint32_t *baby, int n_baby, const uint8_t *present, const uint64_t *diags,
                                 const fhe_ckks_key *const *baby_keys, const fhe_ckks_key *const *giant_keys, fhe_mem mem,
                                 fhe_ckks_diag_matrix **out);
void fhe_ckks_diag_matrix_destroy(fhe_ckks_diag_matrix *m);
/* ct_b, ct_a [batch][L][n] over rns_hi, coefficient domain -> out_b, out_a [batch][L-1][n] over rns_lo; host or device memory; runs on
 * `stream` with a stream-ordered workspace of 8 n batch (2 n_baby L + 2 (n_giant + 1) (L - 1) + 2 terms) bytes (+ the key switch's
 * own).  batch == 0 returns FHE_OK. */
int fhe_ckks_mul_mat(const fhe_ckks_diag_matrix *m, const uint64_t *ct_b, const uint64_t *ct_a, uint64_t *out_b, uint64_t *out_a, size_t batch,
                     fhe_mem mem, void *stream);

/* ---- hoisted CKKS rotations and the double-hoisted diagonal-matrix product --------------------------------------
 * Opt-in entries beside fhe_ckks_rotate and fhe_ckks_mul_mat, which keep the reference's bits.  The entries below are NOT the
 * reference's `rotate` / `mul_mat`: they extend the ciphertext to qs || ps BEFORE the automorphism (the reference after it), so that
 * one extension and one set of forward transforms serve every rotation of a ciphertext.
 *
 * Notation: n the ring degree, qs (L primes) and ps (K primes) the bases of the context, P = prod ps, sigma_t the automorphism
 * X -> X^t, t_j = 5^j mod 2n, ext = fhe_rns_extend_bases (with its f64 correction), (*) the ring product limb by limb over qs || ps.
 * For a ciphertext (b, a) over qs, coefficient domain:
 *     a~ = (a || ext(a)),     b~ = P b  (limb q_l: (P mod q_l) b_l; the p-limbs are zero),
 *     u_0 = (b~, P a),
 *     u_j = ( sigma_{t_j}(b~) + k_j.b (*) sigma_{t_j}(a~),  k_j.a (*) sigma_{t_j}(a~) )     for j != 0 with the rotation key (k_j.b, k_j.a).
 *
 * fhe_rns_automorphism_eval: sigma_t on polynomials that already are in the evaluation domain (extended = 0: [batch][L][n] over qs,
 * 1: [batch][L+K][n] over qs ++ ps), in != out.  A pure permutation of the n evaluation points of every limb, no signs: with psi the
 * 2n-th root of the transform, index k of fhe_rns_ntt_fwd's output holds the value at psi^(2 brev(k) + 1) (fhe_ctx_twiddles documents
 * the table that gives this order), and the output's value at psi^e is the input's value at psi^(e t).  For every x
 *     automorphism_eval(ntt_fwd(x)) == ntt_fwd(fhe_rns_automorphism(x))     bit for bit.
 * t is taken mod 2n; an even t returns FHE_ERR_UNSUPPORTED. */
int fhe_rns_automorphism_eval(const fhe_rns_ctx *rns, int extended, int64_t t, const uint64_t *in, uint64_t *out, size_t n, size_t batch,
                              fhe_mem mem, void *stream);
/* Single hoisting: `count` rotations of ONE ciphertext batch.
 *     out_r = ( rescale_k(u_r.b), rescale_k(u_r.a) ),     u_r of amount amounts[r] with keys[r],     rescale_k = fhe_rns_rescale_k.
 * One ext, L + K forward transforms of a~ and L of b~ for the whole call; per rotation the permutation fused into the product with
 * the key, 2 (L + K) inverse transforms and two rescale_k.  amounts[r] == 0 takes no key (keys[r] may be NULL) and copies the input
 * (P b divided by P is b; u_0 has zero p-limbs, the one input that puts rescale_k's base conversion on a rounding tie, so it is not run).
 *   ct_b, ct_a    [batch][L][n] over qs, coefficient domain; n up to the limit of fhe_ckks_key_switch;
 *   keys          [count] rotation keys prepared on `rns` for this n (fhe_ckks_ksk_prepare); a missing key or one of another context
 *                 or ring is FHE_ERR_INVALID and nothing is written;
 *   out_b, out_a  [count] pointers to [batch][L][n], none overlapping the inputs or one another.
 * NOT the bits of fhe_ckks_rotate, which extends sigma(a).  What holds instead: P b + x divided by P is b + rescale_k(x) exactly, so
 * out_r == fhe_ckks_rotate(keys[r], t_r) wherever no coefficient of a lies within f64 error of a rounding tie of the base conversion
 * (ext commutes with sigma but for the sign of that correction), and out_r decrypts to the same plaintext everywhere: the two differ
 * by a multiple of Q in a~, which the key switch absorbs into its noise.  Stream-ordered workspace: 8 n batch (3 (L + K) + L) bytes. */
int fhe_ckks_rotate_many(const fhe_rns_ctx *rns, size_t n, const uint32_t *amounts, const fhe_ckks_key *const *keys, int count,
                         const uint64_t *ct_b, const uint64_t *ct_a, uint64_t *const *out_b, uint64_t *const *out_a, size_t batch, fhe_mem mem,
                         void *stream);
/* Double hoisting: the diagonal-matrix product with the baby-step sums kept in qs || ps.  The arguments are those of
 * fhe_ckks_diag_matrix_prepare / fhe_ckks_mul_mat with ONE difference: `diags` is [terms][L+K][n] over qs ++ ps, the plaintexts lifted
 * exactly to the extended base (the centred integer coefficients reduced modulo every prime of qs and ps), coefficient domain.  They
 * are transformed once at prepare and kept on the device (8 terms (L + K) n bytes).  For giant step i, D_ij the diagonal of term (i, j):
 *     w_i = sum_{j in js(i)} D_ij (*) u_j      on both halves, over qs || ps,
 *     v_i = rescale( rescale_k(w_i) )          fhe_rns_rescale_k, then fhe_rns_rescale on rns_hi: L - 1 limbs,
 *     out = sum_i rotate_i(v_i),               rotate_0 = identity; fhe_ckks_rotate on rns_lo with giant_keys, as fhe_ckks_mul_mat.
 * Transforms per call, the giant steps' key switches apart: 2 L + K forward, 2 (L + K) n_giant inverse; no per-term product on the
 * last limb.  The result is not the bits of fhe_ckks_mul_mat (fewer roundings, at other places); it decrypts to the same product.
 * Stream-ordered workspace of fhe_ckks_mul_mat_hoisted, in bytes:
 *     8 n batch ( (L + K) + L + 2 n_giant (L + K) + 2 n_giant L + 2 (L - 1) )
 * (a~ | b~ | w, later the v_i | rescale_k(w) | one giant step's automorphism), + the giant steps' key switch's own. */
typedef struct fhe_ckks_diag_matrix_hoisted fhe_ckks_diag_matrix_hoisted;
int fhe_ckks_diag_matrix_prepare_hoisted(const fhe_rns_ctx *rns_hi, const fhe_rns_ctx *rns_lo, size_t n, const uint32_t *giant, int n_giant,
                                         const uint32_t *baby, int n_baby, const uint8_t *present, const uint64_t *diags,
                                         const fhe_ckks_key *const *baby_keys, const fhe_ckks_key *const *giant_keys, fhe_mem mem,
                                         fhe_ckks_diag_matrix_hoisted **out);
void fhe_ckks_diag_matrix_hoisted_destroy(fhe_ckks_diag_matrix_hoisted *m);
int fhe_ckks_mul_mat_hoisted(const fhe_ckks_diag_matrix_hoisted *m, const uint64_t *ct_b, const uint64_t *ct_a, uint64_t *out_b, uint64_t *out_a,
                             size_t batch, fhe_mem mem, void *stream);

/* ---- CKKS encode / decode: scheme/ckks/src/ckks.rs:186-213 `Ckks::encode` / `Ckks::decode` over scheme/ckks/src/sfft.rs:7-72, in
 * double-double arithmetic (an unevaluated sum of two f64, about 106 bits) in place of the reference's 256-bit software floats
 * (util/src/complex/f256.rs).  Complex slots travel as two f64 arrays: `*_hi` [batch][l][2] (re, im: the memory of a complex128
 * array), l = n / 2, and `*_lo` of the same shape with the low words.  A `*_lo` may be NULL: as an input it means zeros, as an output
 * only the f64-rounded value is kept.  Device-memory (FHE_MEM_DEVICE) `*_hi` / `*_lo` pointers must be 16-byte aligned (one complex
 * element per access); host arrays have no such requirement.  Transforms agree with exact arithmetic to about 2^-100 of the largest
 * slot. */
typedef struct fhe_ckks_encoder fhe_ckks_encoder; /* one ring degree n on one device: the twiddle table of sfft.rs:57-72 `w()` */
/* sfft.rs:57-72 `w(l)`: the 4 l powers of cis(pi / (2 l)) as dd pairs, each component within 2^-100 of the true value (computed per
 * entry from the first octant, never by a running product), and the powers of 5 mod 4 l.  n = 2 .. 2^15 a power of two, anything else
 * (n = 1, n > 2^15 included) FHE_ERR_INVALID.  device >= 0: tables uploaded to that GPU; device < 0: host-only, serves
 * fhe_ckks_encoder_twiddles alone (every compute entry returns FHE_ERR_INVALID on it). */
int fhe_ckks_encoder_create(size_t n, int device, fhe_ckks_encoder **out);
void fhe_ckks_encoder_destroy(fhe_ckks_encoder *enc);
/* the first `count` <= 4 l entries of the table: out [count][4] = (re_hi, re_lo, im_hi, im_lo) */
int fhe_ckks_encoder_twiddles(const fhe_ckks_encoder *enc, double *out, size_t count);
/* Waits for everything enqueued on `stream`, then FHE_ERR_INVALID if an asynchronous (device-memory) fhe_ckks_encode met a slot that
 * is not finite or has |z scale| >= 2^126 (`BigInt::from(&F256)` would go on, f256.rs:213-239; here the coefficient is written as 0),
 * or an fhe_ckks_decode a centred value beyond the f64 range, since the word was last cleared; else FHE_OK.  clear != 0 resets the
 * word.  Host-memory calls report (and clear) it in their own return value.  An encoder has ONE word: a host-memory call, or a status
 * query on one stream, also reports and clears what an asynchronous call on ANOTHER stream has set by then, and misses what it sets
 * later -- callers that mix streams or memory kinds on one encoder and need the flag attributed use one encoder per stream (the
 * tables are small) or query the status between the calls. */
int fhe_ckks_encoder_status(const fhe_ckks_encoder *enc, void *stream, int clear);
/* sfft.rs:21-35 `sifft` / sfft.rs:7-19 `sfft` (crate-private in the reference), in place on `batch` messages */
int fhe_ckks_sifft(const fhe_ckks_encoder *enc, double *z_hi, double *z_lo, size_t batch, fhe_mem mem, void *stream);
int fhe_ckks_sfft(const fhe_ckks_encoder *enc, double *z_hi, double *z_lo, size_t batch, fhe_mem mem, void *stream);
/* ckks.rs:186-198 `Ckks::encode`: z = sifft(m); coefficient i <- BigInt::from(z_i.re * scale), coefficient l + i <- BigInt::from(z_i.im *
 * scale) (the fraction dropped toward zero, f256.rs:213-239), reduced into every limb of rns's qs (`RnsRq::from_bigint`).  pt
 * [batch][L][n], coefficient domain: what fhe_ckks_pk_encrypt, fhe_ckks_mul_plain and fhe_ckks_diag_matrix_prepare take.  `scale` is
 * explicit because the reference's is qs.last() of the FULL chain (ckks.rs:27) whatever level `rns` is on.  enc and rns on different
 * devices, scale == 0, a NULL m_hi or pt: FHE_ERR_INVALID. */
int fhe_ckks_encode(const fhe_ckks_encoder *enc, const fhe_rns_ctx *rns, uint64_t scale, const double *m_hi, const double *m_lo, size_t batch,
                    uint64_t *pt, fhe_mem mem, void *stream);
/* ckks.rs:200-213 `Ckks::decode`: every coefficient's residues over rns's L limbs -> the centred integer in (-Q/2, Q/2]
 * (`into_bigint`, exact multi-word arithmetic) -> dd -> / scale -> sfft.  pt [batch][L][n] as fhe_ckks_decrypt gives it. */
int fhe_ckks_decode(const fhe_ckks_encoder *enc, const fhe_rns_ctx *rns, uint64_t scale, const uint64_t *pt, size_t batch, double *m_hi,
                    double *m_lo, fhe_mem mem, void *stream);

/* ---- CKKS linear transforms `slot_to_coeff` / `coeff_to_slot`: scheme/ckks/src/bootstrapping.rs:23-31 `BootstrappingParam::new`,
 * bootstrapping.rs:56-88 `key_gen` / `mul_mats`, over the factor matrices of scheme/ckks/src/sfft.rs:75-99 and the arithmetic of
 * util/src/misc/matrix.rs:45-52, 71-83, 94-150 `DiagSparseMatrix`.  A PLAN holds the matrices of one direction in double-double on the
 * encoder's device: `sfft_fmats(l)` (inverse = 0, slot_to_coeff) or `sifft_fmats(l)` (inverse != 0, coeff_to_slot), l = n / 2, filled by a
 * kernel from the encoder's twiddle table and folded left to right over every chunk of r by one product launch each
 * (matrix.rs:94-123).  Which diagonals a product has is structural, as in the reference: a diagonal whose values cancel stays.
 * Diagonal INDICES ARE NORMALISED mod l.  The reference leaves index l (not 0) on an inverse chunk of a single factor (`inv` maps 0 to
 * l, matrix.rs:77, and `product` of one item never reduces it) and then key-switches for the identity rotation 5^l = 1 mod 2n; here
 * that diagonal is index 0 and costs no key switch: other noise, the same message.
 *   r >= 1 the chunk size of bootstrapping.rs:25 (r >= log2 l: one dense matrix); r < 1, a NULL enc or out: FHE_ERR_INVALID;
 *   n = 2 (l = 1, no factor at all) and a matrix of more than 2^26 elements (2 GiB): FHE_ERR_UNSUPPORTED.
 * On a host-only encoder (device < 0) the plan answers the structure queries alone.  The encoder is BORROWED and must outlive the plan. */
typedef struct fhe_ckks_linear_plan fhe_ckks_linear_plan;
int fhe_ckks_linear_plan_create(const fhe_ckks_encoder *enc, int r, int inverse, fhe_ckks_linear_plan **out);
void fhe_ckks_linear_plan_destroy(fhe_ckks_linear_plan *plan);
/* depth = the number of matrices ceil(log2 l / r); n_rot = the size of `key_gen`'s rotation set for this direction (either may be NULL) */
int fhe_ckks_linear_plan_info(const fhe_ckks_linear_plan *plan, int *depth, int *n_rot);
/* bootstrapping.rs:61-64: the first `count` <= n_rot of the ascending union of the non-zero giant and baby steps of all matrices */
int fhe_ckks_linear_plan_rotations(const fhe_ckks_linear_plan *plan, uint32_t *out, int count);
/* matrix k (0 .. depth-1, the reference's list order): the number of diagonals, the k `DiagSparseMatrix::bsgs` chooses
 * (matrix.rs:45-52: fewest distinct non-zero rotations, the smallest k on a tie; 1 where 0 is the only index) and the sizes of its split;
 * then diag [n_diag] ascending, giant [n_giant] and baby [n_baby] ascending, present [n_giant][n_baby] (any may be NULL) */
int fhe_ckks_linear_plan_matrix_info(const fhe_ckks_linear_plan *plan, int k, int *n_diag, uint32_t *bsgs_k, int *n_giant, int *n_baby);
int fhe_ckks_linear_plan_matrix_split(const fhe_ckks_linear_plan *plan, int k, uint32_t *diag, uint32_t *giant, uint32_t *baby, uint8_t *present);
/* the values of matrix k to HOST memory: out [n_diag][l][4] = (re_hi, re_lo, im_hi, im_lo), diagonal d at position c = dense[c][(c + d) mod l]
 * (matrix.rs:87-91); FHE_ERR_INVALID on a host-only plan */
int fhe_ckks_linear_plan_diags(const fhe_ckks_linear_plan *plan, int k, double *out);
/* ckks.rs:174-184 `Ckks::rtk_gen(param, sk, j)`: j is taken mod l = n / 2 (j = 0 mod l: FHE_ERR_INVALID, the identity has no key),
 * sk(X^(5^j)) is formed on the device from the i64 key (avec.rs:34-50) and handed to fhe_ckks_ksk_gen: ksk_b, ksk_a [L+K][n]. */
int fhe_ckks_rtk_gen(const fhe_rns_ctx *rns, const uint64_t *sk, size_t n, int64_t j, const fhe_rng *rng, uint64_t stream_id, uint64_t *ksk_b,
                     uint64_t *ksk_a, fhe_mem mem, void *stream);
/* bootstrapping.rs:81-88 `mul_mats` prepared once: the matrices of `plan` applied last to first, step s (matrix depth-1-s) taking a
 * ciphertext from levels[s] to levels[s + 1].
 *   levels   [n_levels >= depth + 1] the caller's contexts over qs[0 .. L), qs[0 .. L-1), ..: the same ps, all on the device of the plan's
 *            encoder (the rule of fhe_ckks_diag_matrix_prepare for rns_hi / rns_lo); L >= depth + 1;
 *   scale    of `Ckks::encode` (ckks.rs:27: qs.last() of the full chain);
 *   rot, ksk_b, ksk_a   n_rot rotation indices (taken mod l) and for each ONE coefficient-domain key [L+K][n] over levels[0]
 *            (fhe_ckks_rtk_gen); as in the reference one key per index serves every level: the copy a step uses is the same rows with the
 *            dropped q-limbs removed.  Baby steps of step s are prepared on levels[s], giant steps on levels[s + 1], each (level, index)
 *            once.  `mem` says where the keys live.  Every index of fhe_ckks_linear_plan_rotations must be there.
 * Every `diag_rot(i, j)[c] = diag_{i+j}[(c - i) mod l]` (bootstrapping.rs:101) is encoded on the device with the rotation folded into the
 * encode kernels' loads: the prepared plaintexts have the bits fhe_ckks_encode gives for the rotated diagonal.  A missing index,
 * mismatched contexts, too few levels, a host-only plan or a NULL argument: FHE_ERR_INVALID, nothing stays allocated.  The contexts are
 * BORROWED; the plan and the caller's keys are not needed after the call. */
typedef struct fhe_ckks_linear_transform fhe_ckks_linear_transform;
int fhe_ckks_linear_transform_prepare(const fhe_ckks_linear_plan *plan, const fhe_rns_ctx *const *levels, int n_levels, uint64_t scale,
                                      const uint32_t *rot, const uint64_t *const *ksk_b, const uint64_t *const *ksk_a, int n_rot, fhe_mem mem,
                                      fhe_ckks_linear_transform **out);
void fhe_ckks_linear_transform_destroy(fhe_ckks_linear_transform *t);
/* ct_b, ct_a [batch][L][n] over levels[0] -> out_b, out_a [batch][L - depth][n] over levels[depth], host or device memory, on `stream`:
 * bit-identical to chaining fhe_ckks_mul_mat by hand.  batch == 0 returns FHE_OK. */
int fhe_ckks_linear_transform_apply(const fhe_ckks_linear_transform *t, const uint64_t *ct_b, const uint64_t *ct_a, uint64_t *out_b,
                                    uint64_t *out_a, size_t batch, fhe_mem mem, void *stream);

/* ---- CKKS polynomial evaluation: a Chebyshev (or monomial) series on encrypted slots in one call.  NO REFERENCE LINE: `Ckks` has no
 * such function (bootstrapping.rs stops before the modular reduction).  The pieces keep the reference's conventions: products are
 * scheme/ckks/src/ckks.rs:250-263 `Ckks::mul` with its closing `rescale()`, the rescale is util/src/ring/rns.rs:99-111 (the K == 1 branch,
 * NOT centred), and a real constant c becomes the integer trunc(c * scale), the fraction dropped toward zero as ckks.rs:186-198
 * `Ckks::encode` drops it (exact here: c is an f64, so mantissa * scale fits 128 bits).  A constant slot vector is the constant
 * polynomial, so adding one touches coefficient 0 of the b half only.  Every ciphertext is taken to carry the scale `scale`: a product or
 * a real-mode combination leaves scale^2 / q_last, which the reference too treats as scale (all primes of a chain have one bit length).
 *
 * fhe_ckks_scaled_constant: trunc(c * scale) reduced into [0, q), negative values as q - |k| mod q.  c not finite or |c * scale| >= 2^126:
 * FHE_ERR_INVALID. */
int fhe_ckks_scaled_constant(double c, uint64_t scale, uint64_t q, uint64_t *out);
/* ONE launch combines n_terms <= 16 ciphertexts with a constant.  Ciphertext j is ct_b[j], ct_a[j] [batch][limbs[j]][n], coefficient
 * domain, limbs[j] >= l = the limb count of rns; only limbs 0 .. l of each are read (the level drop, exact in RNS, nothing is repacked).
 *   real == 0   out = sum_j imul[j] ct_j + k0 e0, k0 = trunc(c0 scale); out_b, out_a [batch][l][n]; no level is consumed (cmul unused);
 *   real != 0   out = rescale( sum_j k_j ct_j + k0 scale e0 ), k_j = trunc(cmul[j] scale); out [batch][l - 1][n]; l >= 2 (imul unused).
 * The sum is accumulated unreduced in 128 bits and reduced once per output where every modulus is below 2^61, product by product
 * otherwise: the same residues either way.  An output may alias an input only with real == 0 and limbs[j] == l (the same layout).
 * A NULL argument, limbs[j] < l, n_terms outside 1 .. 16, a constant that is not finite or has |c scale| >= 2^126, scale == 0, l < 2 with
 * real != 0: FHE_ERR_INVALID.  batch == 0: FHE_OK.  The per-limb constants are made on the host per call and the call waits for the stream
 * before it returns (fhe_ckks_poly_apply uploads its constants once and does not). */
int fhe_ckks_lincomb(const fhe_rns_ctx *rns, int real, int n_terms, const uint64_t *const *ct_b, const uint64_t *const *ct_a, const int *limbs,
                     const int64_t *imul, const double *cmul, double c0, uint64_t scale, uint64_t *out_b, uint64_t *out_a, size_t n, size_t batch,
                     fhe_mem mem, void *stream);
/* fhe_ckks_mul whose operands already ARE in the evaluation domain (fhe_rns_ntt_fwd of both halves) on x_limbs, y_limbs >= L limbs, read
 * on the prefix 0 .. L of rns; then, after the closing rescale, out = alpha out - ct_c with alpha in {1, 2} and ct_c (c_b, c_a
 * [batch][c_limbs][n], coefficient domain, c_limbs >= L - 1, or both NULL: nothing subtracted).  Bit-identical to fhe_ckks_mul on the
 * prefix-sliced operands followed by the integer-mode fhe_ckks_lincomb {alpha, -1}.  out_b, out_a [batch][L - 1][n]. */
int fhe_ckks_mul_eval(const fhe_rns_ctx *rns, const fhe_ckks_key *rlk, const uint64_t *x_b, const uint64_t *x_a, int x_limbs, const uint64_t *y_b,
                      const uint64_t *y_a, int y_limbs, int alpha, const uint64_t *c_b, const uint64_t *c_a, int c_limbs, uint64_t *out_b, uint64_t *out_a,
                      size_t batch, fhe_mem mem, void *stream);
/* The PLAN: a host-only schedule (no GPU is touched) over registers; register 0 is the input ciphertext and every other register is
 * written exactly once, before it is read.  One op is one record:
 *   kind == FHE_POLY_MUL   dst = alpha * (a * b) - c        a, b, c registers, alpha in {1, 2}, c == -1: nothing subtracted;
 *   kind == FHE_POLY_LIN   dst = sum_{j < n_terms} coef[j] * src[j] + c0      mode 0: integer multipliers (coef[j] holds the integer), no
 *                          level consumed; mode 1: real multipliers, one level consumed (fhe_ckks_lincomb's two modes).
 * Fields a kind does not use are 0 (c: -1).  The level offset ("depth") of a register follows from the list: depth(0) = 0, a MUL gives
 * max(depth a, depth b) + 1, a LIN max over its sources + mode; an op runs on the limbs its shallowest-level operand has and reads the
 * others by prefix.  The result is the dst of the LAST op and is the deepest register.
 * fhe_ckks_poly_plan_create builds the fixed baby-step / giant-step (Paterson-Stockmeyer) schedule of sum_j coeffs[j] T_j(x), x in
 * [-1, 1] (basis 0, Chebyshev) or sum_j coeffs[j] x^j (basis 1), 0 <= degree <= 255:
 *   - k = the smallest power of two >= 2 with k^2 >= degree + 1;
 *   - powers T_i are made on demand by T_{a+b} = 2 T_a T_b - T_{a-b}, a the largest power of two below i (T_{2a} = 2 T_a^2 - 1 as a MUL
 *     with alpha = 2 and an integer LIN adding -1; x^{a+b} = x^a x^b), so T_i sits at depth ceil(log2 i);
 *   - the series is split recursively at the largest giant m = 2^j k <= its degree, p = quo T_m + rem (T_{m+i} = 2 T_m T_i - T_{m-i}), into
 *     blocks of degree < k: a block is ONE real-mode LIN of baby powers, and a split is ONE MUL quo * T_m with the block of -rem as its
 *     subtrahend;
 *   - a term with coeffs[j] == 0.0 is left out structurally (a power nobody needs is never computed), an all-zero block is skipped
 *     together with its product or subtrahend, and a constant series (degree 0, or everything else zero) is the single real-mode op
 *     0.0 * input + c0.
 * The depth is at most ceil(log2(degree + 1)) + 2.  fhe_ckks_poly_plan_from_ops takes a caller-made list (how the eval_mod recipe wraps a
 * series in its scaling and double-angle steps) and checks the rules above; anything else is FHE_ERR_INVALID, as are degree > 255, a
 * coefficient that is not finite and a NULL argument. */
enum { FHE_POLY_MUL = 0, FHE_POLY_LIN = 1 };
typedef struct {
    int32_t kind, dst;
    int32_t a, b, alpha, c;   /* MUL */
    int32_t mode, n_terms;    /* LIN */
    int32_t src[16];
    double coef[16];
    double c0;
} fhe_ckks_poly_op;
typedef struct fhe_ckks_poly_plan fhe_ckks_poly_plan;
int fhe_ckks_poly_plan_create(const double *coeffs, int degree, int basis, fhe_ckks_poly_plan **out);
int fhe_ckks_poly_plan_from_ops(const fhe_ckks_poly_op *ops, int n_ops, fhe_ckks_poly_plan **out);
void fhe_ckks_poly_plan_destroy(fhe_ckks_poly_plan *plan);
/* the multiplicative depth (= levels the evaluation consumes), the number of ops and of registers, the input included (any may be NULL) */
int fhe_ckks_poly_plan_info(const fhe_ckks_poly_plan *plan, int *depth, int *n_ops, int *n_regs);
/* the first `count` <= n_ops records in execution order */
int fhe_ckks_poly_plan_ops(const fhe_ckks_poly_plan *plan, fhe_ckks_poly_op *out, int count);
/* The plan bound to the caller's contexts: levels [n_levels >= depth + 1], levels[s] over qs[0 .. L - s) with the same ps on the same
 * device (the rule of fhe_ckks_linear_transform_prepare), L >= depth + 1; `scale` of `Ckks::encode`; rlk_b, rlk_a ONE coefficient-domain
 * relinearisation key [L + K][n] over levels[0] (`mem` says where it lives), cut down to every level a MUL runs on by removing the dropped
 * q-limb rows and prepared once per level.  Every constant is reduced per (op, limb) here and uploaded.  The contexts are BORROWED; the
 * plan and the caller's key are not needed after the call.  Mismatched contexts, too few levels, a constant out of range or a NULL
 * argument: FHE_ERR_INVALID, nothing stays allocated. */
typedef struct fhe_ckks_poly_eval fhe_ckks_poly_eval;
int fhe_ckks_poly_prepare(const fhe_ckks_poly_plan *plan, const fhe_rns_ctx *const *levels, int n_levels, uint64_t scale, const uint64_t *rlk_b,
                          const uint64_t *rlk_a, size_t n, fhe_mem mem, fhe_ckks_poly_eval **out);
void fhe_ckks_poly_eval_destroy(fhe_ckks_poly_eval *eval);
/* ct_b, ct_a [batch][L][n] over levels[0], coefficient domain -> out_b, out_a [batch][L - depth][n] over levels[depth]; host or device
 * memory, on `stream`, nothing waits.  Bit-identical to replaying the op list through fhe_ckks_mul (on contiguous prefix slices) and
 * fhe_ckks_lincomb.  Every register that feeds a MUL is forward-transformed ONCE and kept in the evaluation domain for all its uses (its
 * prefix limbs serve the lower levels); a register that only feeds LIN ops is never transformed.  Stream-ordered workspace, in 8-byte
 * words: 2 batch n (L - depth(g)) for every register g but the input and the result, the same again for every register that feeds a MUL,
 * and 5 batch n l_max for the running product (l_max = the limbs of the highest-level MUL), plus the key switch's own.  batch == 0
 * returns FHE_OK. */
int fhe_ckks_poly_apply(const fhe_ckks_poly_eval *eval, const uint64_t *ct_b, const uint64_t *ct_a, uint64_t *out_b, uint64_t *out_a, size_t batch,
                        fhe_mem mem, void *stream);

/* ---- CKKS bootstrap: `mod_raise`, the conjugate split after `coeff_to_slot`, `eval_mod` on both halves, the join, `slot_to_coeff`, as
 * single entries and as ONE call.  NO REFERENCE LINE: scheme/ckks/src/bootstrapping.rs ends at `coeff_to_slot` / `slot_to_coeff`.  The
 * conventions are the reference's: `Ckks::encode` (ckks.rs:186-198) puts Re z_i scale in coefficient i and Im z_i scale in coefficient
 * l + i (l = n / 2, z = sifft(m)); `Ckks::conjugate` (ckks.rs:279-282) is fhe_ckks_rotate with t = -1 and the key of `Ckks::cjk_gen`.
 * With D = scale and q_0 = qs[0], a ciphertext that is meaningful mod q_0 decrypts after fhe_ckks_mod_raise to t = c + e + q_0 I (c the
 * encoded coefficients, I an integer polynomial, |I_j| <= (|sk|_1 + 1) / 2); coeff_to_slot leaves w_i = (t_i + i t_{l+i}) / D in the slots
 * (in some order, which the slot-wise steps do not care about); R = ct + conj(ct) holds 2 t_i / D and J = -X^(n/2) (ct - conj(ct)) holds
 * 2 t_{l+i} / D (X^(n/2) multiplies every slot by i because 5^k = 1 mod 4: an exact negacyclic shift by n/2, no level, no noise);
 * eval_mod with pre = D / (2 q_0) and post = q_0 / D maps both to about c_j / D; out = R' + X^(n/2) J' holds z again and slot_to_coeff
 * returns m.
 *
 * ckks.rs:169-172 `Ckks::cjk_gen(param, sk)`: sk(X^-1) is formed on the device from the i64 key (avec.rs:34-50, as fhe_ckks_rtk_gen forms
 * sk(X^(5^j))) and handed to fhe_ckks_ksk_gen: ksk_b, ksk_a [L+K][n].  n = 2 .. a power of two. */
int fhe_ckks_cjk_gen(const fhe_rns_ctx *rns, const uint64_t *sk, size_t n, const fhe_rng *rng, uint64_t stream_id, uint64_t *ksk_b, uint64_t *ksk_a,
                     fhe_mem mem, void *stream);
/* ct_b, ct_a [batch][in_limbs][n], of which ONLY limb 0 (residues mod q_0 = the first modulus of rns) is read -> out_b, out_a
 * [batch][L][n] over rns: every residue lifted to its centred integer in (-q_0 / 2, q_0 / 2] and reduced into every q-limb, a negative
 * value v as q_l - (|v| mod q_l) with 0 staying 0.  Right for any base: |v| may exceed a smaller q_l many times over.  in_limbs < 1, a NULL
 * argument, n not a ring degree of rns: FHE_ERR_INVALID.  batch == 0: FHE_OK. */
int fhe_ckks_mod_raise(const fhe_rns_ctx *rns, const uint64_t *ct_b, const uint64_t *ct_a, int in_limbs, uint64_t *out_b, uint64_t *out_a, size_t n,
                       size_t batch, fhe_mem mem, void *stream);
/* ct = (ct_b, ct_a) and its conjugate cj = (cj_b, cj_a) (fhe_ckks_rotate with t = -1 on a copy of ct), each [batch][L][n] over the q-limbs
 * of rns -> out_b, out_a [2 batch][L][n]: rows [0, batch) hold R = ct + cj, rows [batch, 2 batch) hold J = -X^(n/2) (ct - cj), one stacked
 * batch for ONE fhe_ckks_poly_apply.  The outputs must not overlap the inputs. */
int fhe_ckks_conj_split(const fhe_rns_ctx *rns, const uint64_t *ct_b, const uint64_t *ct_a, const uint64_t *cj_b, const uint64_t *cj_a, uint64_t *out_b,
                        uint64_t *out_a, size_t n, size_t batch, fhe_mem mem, void *stream);
/* the inverse layout: in_b, in_a [2 batch][L][n] (rows [0, batch) = R', rows [batch, 2 batch) = J') -> out_b, out_a [batch][L][n] =
 * R' + X^(n/2) J'.  fhe_ckks_conj_join of fhe_ckks_conj_split(x, cx) is 2 x exactly.  NULL argument, n not a ring degree of rns:
 * FHE_ERR_INVALID; batch == 0: FHE_OK (both entries). */
int fhe_ckks_conj_join(const fhe_rns_ctx *rns, const uint64_t *in_b, const uint64_t *in_a, uint64_t *out_b, uint64_t *out_a, size_t n, size_t batch,
                       fhe_mem mem, void *stream);
/* The scaled-sine modular reduction as a plan, host only (no GPU is touched): slots x -> post / (2 pi) sin(2 pi pre x), right where
 * |pre x| <= K.
 *   1. u = (pre / K) x                                  one real-mode LIN;
 *   2. y = the degree-`degree` Chebyshev interpolant of cos(2 pi (K u - 1/4) / 2^r) at the degree + 1 Chebyshev nodes of the first kind
 *      (the definition numpy.polynomial.chebyshev.chebinterpolate uses), through fhe_ckks_poly_plan_create's own schedule;
 *   3. r double-angle steps y <- 2 y^2 - 1              a MUL with alpha = 2 and an integer LIN adding -1 each;
 *   4. the factor post / (2 pi)                         one real-mode LIN.
 * With pre = post = 1 slots t = eps + I (I an integer, |t| <= K) come out as about eps; a bootstrap passes pre = scale / (2 q_0) and
 * post = q_0 / scale (above).  K < 1, r < 0 (or more steps than a plan holds), degree outside 1 .. 255, a factor that is not finite, a
 * NULL out: FHE_ERR_INVALID. */
int fhe_ckks_eval_mod_plan_create(int K, int r, int degree, double pre, double post, fhe_ckks_poly_plan **out);
/* The bootstrapper: the caller's prepared stages bound together.
 *   levels   [n_levels >= depth + 1], levels[s] over qs[0 .. L - s) with the same ps on the same device (the rule of
 *            fhe_ckks_linear_transform_prepare); depth = d_c2s + d_mod + d_s2c, the depths of the three stages;
 *   c2s, eval, s2c   the coeff_to_slot transform, the eval_mod evaluator and the slot_to_coeff transform, prepared on levels[0 ..],
 *            levels[d_c2s ..] and levels[d_c2s + d_mod ..]: the SAME context objects (checked by identity) and the same n.  BORROWED, as are
 *            the contexts: all must outlive the bootstrapper;
 *   cjk_b, cjk_a   ONE coefficient-domain conjugation key [L + K][n] over levels[0] (fhe_ckks_cjk_gen; `mem` says where it lives), cut
 *            down to levels[d_c2s] by removing the dropped q-limb rows and prepared once; not needed after the call.
 * Too few levels, stages bound to other contexts or another n, mismatched contexts or a NULL argument: FHE_ERR_INVALID, nothing stays
 * allocated. */
typedef struct fhe_ckks_bootstrap fhe_ckks_bootstrap;
int fhe_ckks_bootstrap_prepare(const fhe_rns_ctx *const *levels, int n_levels, size_t n, const fhe_ckks_linear_transform *c2s,
                               const fhe_ckks_poly_eval *eval, const fhe_ckks_linear_transform *s2c, const uint64_t *cjk_b, const uint64_t *cjk_a,
                               fhe_mem mem, fhe_ckks_bootstrap **out);
void fhe_ckks_bootstrap_destroy(fhe_ckks_bootstrap *bs);
/* the levels the call consumes and the limbs L - depth of its result (either may be NULL) */
int fhe_ckks_bootstrap_info(const fhe_ckks_bootstrap *bs, int *depth, int *out_limbs);
/* ct_b, ct_a [batch][in_limbs][n] (limb 0 read) -> out_b, out_a [batch][L - depth][n] over levels[depth]; host or device memory, on
 * `stream`, nothing waits.  Bit-identical to chaining the public entries by hand: fhe_ckks_mod_raise, fhe_ckks_linear_transform_apply,
 * fhe_ckks_rotate (t = -1) on a copy, fhe_ckks_conj_split, fhe_ckks_poly_apply on the stacked 2 batch ciphertexts,
 * fhe_ckks_conj_join, fhe_ckks_linear_transform_apply.  Stream-ordered workspace, in 8-byte words, with L1 = L - d_c2s and L2 = L1 - d_mod:
 * 2 batch n L for the raised ciphertext, 2 batch n L1 each for the slots and their conjugate, 4 batch n L1 for the stacked pair,
 * 4 batch n L2 for the reduced pair and 2 batch n L2 for the joined ciphertext, every block released in stream order as soon as its last
 * reader is enqueued: at most batch n max(2 L + 2 L1, 8 L1) live at once, plus the running stage's own.  A NULL bootstrapper or argument,
 * in_limbs < 1: FHE_ERR_INVALID.  batch == 0 returns FHE_OK. */
int fhe_ckks_bootstrap_apply(const fhe_ckks_bootstrap *bs, const uint64_t *ct_b, const uint64_t *ct_a, int in_limbs, uint64_t *out_b, uint64_t *out_a,
                             size_t batch, fhe_mem mem, void *stream);

/* ---- TFHE key material, k = 1 (rank k: fhe_tglwek_sk_encrypt / fhe_tggswk_encrypt at the end).  Draws are counter based (ChaCha20, as above): reproducible per
 * (generator key, stream_id), checked at decode level like the reference's own tests (its draws are unseeded). */
/* util/src/misc/distribution.rs:49-54 `tdg(std_dev)`: torus Gaussian noise (Box-Muller deviate, fractional part scaled by 2^64) */
int fhe_sample_tdg(double std_dev, const fhe_rng *rng, uint64_t stream_id, uint64_t *out, size_t count, fhe_mem mem, void *stream);
/* distribution.rs `binary()` (scheme/tfhe/src/tlwe.rs:96-98 `Tlwe::sk_gen`): one uniform bit per output word */
int fhe_sample_binary(const fhe_rng *rng, uint64_t stream_id, uint64_t *out, size_t count, fhe_mem mem, void *stream);
/* scheme/tfhe/src/tlwe.rs:122-132 `Tlwe::sk_encrypt` for `rows` plaintexts (pt [rows] or NULL): out_a [rows][n], out_b [rows] */
int fhe_tlwe_sk_encrypt(const uint64_t *sk, const uint64_t *pt, size_t n, size_t rows, double std_dev, const fhe_rng *rng, uint64_t stream_id,
                        uint64_t *out_a, uint64_t *out_b, fhe_mem mem, void *stream);
/* scheme/tfhe/src/tlwe.rs:100-111 `Tlwe::ksk_gen(param, sk0, sk1)`: ksk_a [n1 d][n0], ksk_b [n1 d] (digit-major), the layout
 * fhe_tlwe_key_switch / fhe_tfhe_bootstrap take with n_in = n1, n_out = n0 */
int fhe_tlwe_ksk_gen(int log_b, int d, const uint64_t *sk0, size_t n0, const uint64_t *sk1, size_t n1, double std_dev, const fhe_rng *rng, uint64_t stream_id, uint64_t *ksk_a, uint64_t *ksk_b, fhe_mem mem, void *stream);
/* scheme/tfhe/src/tglwe.rs:91-103 `Tglwe::sk_encrypt`: ct_a uniform, ct_b = ct_a * sk + e + pt, [rows][n]; sk [n] binary; pt NULL = zeros.
 * The product a * sk is the exact integer product of row T. */
int fhe_tglwe_sk_encrypt(const fhe_torus_ctx *t, const uint64_t *sk, const uint64_t *pt, size_t n, size_t rows, double std_dev, const fhe_rng *rng, uint64_t stream_id, uint64_t *ct_a, uint64_t *ct_b, fhe_mem mem, void *stream);
/* scheme/tfhe/src/tggsw.rs:73-88 `Tggsw::sk_encrypt` for `count` plaintext polynomials pt [count][n] (bootstrapping.rs:64-69: the
 * constants z_i): rows_a, rows_b [count][2d][n], the layout fhe_tggsw_prepare takes */
int fhe_tggsw_encrypt(const fhe_torus_ctx *t, int log_b, int d, const uint64_t *sk, const uint64_t *pt, size_t n, size_t count, double std_dev,
                      const fhe_rng *rng, uint64_t stream_id, uint64_t *rows_a, uint64_t *rows_b, fhe_mem mem, void *stream);

/* tglwe.rs:91-103 `Tglwe::sk_encrypt` at rank k: sk [k n] binary (the TLWE key that `as_rings` cuts into k rings, tglwe.rs:40-44);
 * pt [rows][n] or NULL; ct [rows][k + 1][n] with b = sum_j a_j s_j + e + pt */
int fhe_tglwek_sk_encrypt(const fhe_torus_ctx *t, int k, const uint64_t *sk, const uint64_t *pt, size_t n, size_t rows, double std_dev,
                          const fhe_rng *rng, uint64_t stream_id, uint64_t *ct, fhe_mem mem, void *stream);
/* tggsw.rs:73-88 `Tggsw::sk_encrypt` at rank k of pt [count][n]: rows [count][(k + 1) d][k + 1][n], the layout fhe_tggswk_prepare takes */
int fhe_tggswk_encrypt(const fhe_torus_ctx *t, int k, int log_b, int d, const uint64_t *sk, const uint64_t *pt, size_t n, size_t count,
                       double std_dev, const fhe_rng *rng, uint64_t stream_id, uint64_t *rows, fhe_mem mem, void *stream);

/* ---- FHEW gate circuits: scheme/fhew/src/fhew/boolean.rs:134-176 and fhew/uint8.rs:50-163 (`FhewU8::wrapping_add` .. `div_rem`) build
 * arithmetic out of `Fhew::{and, nand, or, nor, xor, xnor, majority}` (fhew.rs:59-67) and `Fhew::not` (fhew.rs:27-29), one gate
 * bootstrap after the other.  Here such a composition is a NETLIST, prepared once and run in one call: the gates of one level, across
 * the whole batch, form one batch of gate bootstraps, and nothing on the host sits between two levels. */
typedef struct fhe_fhew_circuit fhe_fhew_circuit;
enum { FHE_GATE_AND = 0, FHE_GATE_NAND = 1, FHE_GATE_OR = 2, FHE_GATE_NOR = 3, FHE_GATE_XOR = 4, FHE_GATE_XNOR = 5, FHE_GATE_MAJORITY = 6 };
typedef struct { uint8_t op; uint8_t pad[3]; uint32_t in[3]; } fhe_fhew_gate;   /* op: FHE_GATE_AND, NAND, OR, NOR, XOR, XNOR, MAJORITY */
#define FHE_WIRE_NOT 0x80000000u   /* on a wire reference: take `Fhew::not` of it (fhew.rs:27-29), a free linear step */
/* Wire w < n_inputs is input w, wire n_inputs + g the output of gate g; a gate reads wires below its own only (topological order);
 * the two-input ops ignore in[2]; outputs[] may repeat a wire, name an input and carry FHE_WIRE_NOT.  The netlist is validated
 * (unknown op, forward or out-of-range reference, n_inputs == 0, n_outputs == 0, more than 2^24 wires: FHE_ERR_INVALID), gates no
 * output depends on are dropped (the reference computes a few: the last carries of uint8.rs:65-76 and 119-131), and every live gate
 * gets the level 1 + max(level of its inputs), inputs at level 0.  Host only: needs no device. */
int  fhe_fhew_circuit_create(const fhe_fhew_gate *gates, size_t n_gates, size_t n_inputs,
                             const uint32_t *outputs, size_t n_outputs, fhe_fhew_circuit **out);
void fhe_fhew_circuit_destroy(fhe_fhew_circuit *c);
/* levels, gates that are kept, gates of the widest level (each pointer may be NULL) */
int  fhe_fhew_circuit_info(const fhe_fhew_circuit *c, size_t *n_levels, size_t *n_live_gates, size_t *max_width);
int  fhe_fhew_circuit_levels(const fhe_fhew_circuit *c, uint32_t *level_of_gate /* [n_gates], 0 = dead */);
/* The netlist on `batch` ciphertexts per wire, exactly the composition of fhew.rs:27-29 and 59-67 it describes: bit-identical to running
 * the gates one by one through fhe_lwe_lincomb and fhe_fhew_bootstrap with addend = round(Q / 8).  Keys as for fhe_fhew_bootstrap.
 * Per level ONE pass over (gates of the level) x batch ciphertexts: a front kernel (gather, signed sums, inversions, mod_switch to
 * q_ks, per-ciphertext look-up rows), key switch, mod_switch_odd, blind rotation (the split route where fhe_blind_rotate_split says
 * so), sample extract straight into the wire table.  The outputs must not overlap the inputs.  Device-memory calls are asynchronous
 * and report the blind rotations' data-dependent conditions through fhe_bootstrap_key_status; host-memory calls mirror inputs and
 * outputs once and report them in the return value.  Ring degree below 4: FHE_ERR_UNSUPPORTED (the look-up rows have runs of n / 4). */
int fhe_fhew_circuit_run(const fhe_fhew_circuit *c, const fhe_bootstrap_key *bk, uint64_t q_ks, int ks_log_b, int ks_d,
                         const uint64_t *lwe_ksk_a, const uint64_t *lwe_ksk_b,
                         const uint64_t *in_a  /* [n_inputs][batch][N] */,  const uint64_t *in_b  /* [n_inputs][batch] */,
                         uint64_t *out_a       /* [n_outputs][batch][N] */, uint64_t *out_b       /* [n_outputs][batch] */,
                         size_t batch, fhe_mem mem, void *stream);

/* ---- TFHE look-up-table circuits: scheme/tfhe/src/bootstrapping.rs:118-165 bootstraps a `log_p`-bit message with one padding bit through
 * a table per function (`identity`, `double`, `parity`).  Arithmetic in that style -- radix integers of message + carry blocks,
 * comparisons, a bivariate function through 4x + y -- is a NETLIST of two steps: a free integer combination of TLWE ciphertexts
 * (tlwe.rs:22-75) and one programmable bootstrap (bootstrapping.rs:78-82) through the table of the node.  Prepared once, run in one call:
 * the nodes of one level, across the whole batch, form one batch of bootstraps, each job with its own table. */
typedef struct fhe_tfhe_circuit fhe_tfhe_circuit;
typedef struct { uint32_t wire; int32_t weight; } fhe_tfhe_term;
typedef struct { uint32_t first_term, n_terms; uint64_t constant; uint32_t table; uint32_t pad; } fhe_tfhe_node;
/* Wire w < n_inputs is input w, wire n_inputs + g is node g = bootstrap(tables[table], constant + sum of weight * wire over
 * terms[first_term .. first_term + n_terms - 1]); a node reads wires below its own only; outputs[] may repeat a wire or name an input.
 * FHE_ERR_INVALID (and no handle) for: a term range outside terms, n_terms == 0 or > 16, a forward or out-of-range wire, a weight of 0,
 * table >= n_tables, n_inputs == 0, n_outputs == 0, more than 2^24 wires, n_tables > 65536.  Nodes no output depends on are dropped;
 * every live node gets the level 1 + max(level of its inputs), inputs at level 0.  Host only: needs no device. */
int  fhe_tfhe_circuit_create(const fhe_tfhe_node *nodes, size_t n_nodes, const fhe_tfhe_term *terms, size_t n_terms, size_t n_inputs,
                             size_t n_tables, const uint32_t *outputs, size_t n_outputs, fhe_tfhe_circuit **out);
void fhe_tfhe_circuit_destroy(fhe_tfhe_circuit *c);
/* levels, nodes that are kept, nodes of the widest level (each pointer may be NULL) */
int  fhe_tfhe_circuit_info(const fhe_tfhe_circuit *c, size_t *n_levels, size_t *n_live_nodes, size_t *max_width);
int  fhe_tfhe_circuit_levels(const fhe_tfhe_circuit *c, uint32_t *level_of_node /* [n_nodes], 0 = dead */);
/* The netlist on `batch` ciphertexts per wire: bit-identical, in every key form, to running the live nodes one by one through
 * fhe_tlwe_lincomb and fhe_tfhe_bootstrap with v = tables[table].  Per level ONE pass over (nodes of the level) x batch jobs: a front
 * kernel (gather, weighted sum + constant, `mod_switch` of bootstrapping.rs:99-104, the table index of every job), the blind rotation
 * with a table per ciphertext (84-96), sample_extract(0) (tglwe.rs:115-127), the key switch (tlwe.rs:144-153) straight into the wire
 * table; then one copy of the output wires.  tables [n_tables][n] with the n_tables of create; keys as for fhe_tfhe_bootstrap.  The
 * outputs must not overlap the inputs.  Device-memory calls are asynchronous; host-memory calls mirror inputs, tables and outputs once. */
int fhe_tfhe_circuit_run(const fhe_tfhe_circuit *c, const fhe_torus_ctx *t, const fhe_tggsw_key *brk, int ks_log_b, int ks_d,
                         const uint64_t *ksk_a, const uint64_t *ksk_b, const uint64_t *tables /* [n_tables][n] */,
                         const uint64_t *in_a  /* [n_inputs][batch][n_lwe] */,  const uint64_t *in_b  /* [n_inputs][batch] */,
                         uint64_t *out_a       /* [n_outputs][batch][n_lwe] */, uint64_t *out_b       /* [n_outputs][batch] */,
                         size_t batch, fhe_mem mem, void *stream);

/* ---- Many-LUT programmable bootstrap: several tables from ONE blind rotation (PBSmanyLUT, Chillotti-Ligier-Orfila-Tap 2021) over the
 * reference's pieces, scheme/tfhe/src/bootstrapping.rs:78-128 and tglwe.rs:115-127.  v = log_funcs, 0 <= v <= 4, is the log2 of the number
 * of functions one rotation serves: the ciphertext is mod-switched to multiples of 2^v, ONE test polynomial that interleaves the 2^v
 * tables, P[c] = L_{c mod 2^v}[c - (c mod 2^v)] (L_i the ordinary table of function i: n / (2p) must be a multiple of 2^v), is rotated,
 * and coefficients 0 .. 2^v - 1 are extracted: coefficient i holds f_i of the message.  NOT bit-identical to an ordinary bootstrap
 * through L_i (the accumulator differs); the two agree at decode level.  The mod-switch drift grows by 2^v: with a binary key of
 * dimension n_lwe the worst case is 2^v (n_lwe + 1) / 2 of 2n positions against a half-slot of n / (2p) -- the caller's condition. */
/* bootstrapping.rs:99-104 `mod_switch` to multiples of 2^log_funcs: rounding_shr(v, 64 - log2(2 big_n) + log_funcs) << log_funcs, i.e.
 * the reference's mod_switch for big_n >> log_funcs, shifted left.  log_funcs = 0: the bits of fhe_tfhe_mod_switch.  log_funcs > 4 or
 * 2^log_funcs > big_n: FHE_ERR_INVALID. */
int fhe_tfhe_mod_switch_many(const uint64_t *in, uint64_t *out, size_t count, size_t big_n, int log_funcs, fhe_mem mem, void *stream);
/* tglwe.rs:115-127 `sample_extract(ct, i)` for i = 0 .. 2^log_funcs - 1 in one pass that reads every ciphertext once: ct_a, ct_b
 * [batch][n] -> out_a [batch][2^log_funcs][n], out_b [batch][2^log_funcs]; row (c, i) has the bits of fhe_tglwe_sample_extract with
 * index = i.  log_funcs > 4 or 2^log_funcs > n: FHE_ERR_INVALID; 2^log_funcs * batch beyond 31 bits: FHE_ERR_UNSUPPORTED. */
int fhe_tglwe_sample_extract_many(const uint64_t *ct_a, const uint64_t *ct_b, size_t n, int log_funcs, uint64_t *out_a, uint64_t *out_b,
                                  size_t batch, fhe_mem mem, void *stream);
/* bootstrapping.rs:78-82 `Bootstrapping::bootstrap` with 2^log_funcs outputs per ciphertext: fhe_tfhe_mod_switch_many, 99-104 ->
 * fhe_tfhe_blind_rotate_tables, 84-96, on the INTERLEAVED tables [n_tables][n], table_of [batch] -> fhe_tglwe_sample_extract with
 * index = i, i < 2^log_funcs, tglwe.rs:115-127 -> fhe_tlwe_key_switch, tlwe.rs:144-153: out_a [batch][2^log_funcs][n_lwe], out_b [batch][2^log_funcs], bit-identical to
 * those calls chained, in every key form (fft64: on the same device).  Everything else as fhe_tfhe_bootstrap_tables.  log_funcs > 4:
 * FHE_ERR_INVALID; 2^log_funcs * batch beyond 31 bits: FHE_ERR_UNSUPPORTED. */
int fhe_tfhe_bootstrap_many(const fhe_torus_ctx *t, const fhe_tggsw_key *brk, int ks_log_b, int ks_d, const uint64_t *ksk_a,
                            const uint64_t *ksk_b, const uint64_t *tables, size_t n_tables, const uint32_t *table_of, int log_funcs,
                            const uint64_t *lwe_a, const uint64_t *lwe_b, uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem,
                            void *stream);
/* A node of fhe_tfhe_circuit_create_many under either name: `many.log_funcs` is `node.pad`, the same 24 bytes. */
typedef union {
    fhe_tfhe_node node;
    struct { uint32_t first_term, n_terms; uint64_t constant; uint32_t table; uint32_t log_funcs; } many;
} fhe_tfhe_node_many;
/* fhe_tfhe_circuit_create with many-LUT nodes (bootstrapping.rs:78-128, tglwe.rs:115-127): the node's fourth 32-bit field is log_funcs.
 * Node g = ONE blind rotation of tables[table], an interleaved table of 2^log_funcs functions, and owns 2^log_funcs consecutive wires:
 * the wire of (g, i) is n_inputs + sum_{h < g} 2^log_funcs_h + i; a node reads wires below its own first wire only.  Rejections: those
 * of fhe_tfhe_circuit_create, and log_funcs > 4; the cap of 2^24 wires counts output wires.  A node is live when any of its outputs
 * is; only live OUTPUTS get a place in the wire table, an extraction and a key-switch row.  With every log_funcs == 0 the circuit is
 * that of fhe_tfhe_circuit_create.  _run, _info, _levels and _destroy take the handle; per level _run launches the front with a shift
 * per node, the blind rotation (one job per NODE), one extraction pass over the live outputs and the key switch (one row per live
 * OUTPUT); the workspace is sized inside.  Bit-identical to the live nodes one by one through fhe_tlwe_lincomb and
 * fhe_tfhe_bootstrap_many. */
int  fhe_tfhe_circuit_create_many(const fhe_tfhe_node *nodes, size_t n_nodes, const fhe_tfhe_term *terms, size_t n_terms, size_t n_inputs,
                                  size_t n_tables, const uint32_t *outputs, size_t n_outputs, fhe_tfhe_circuit **out);
/* bootstrapping.rs:78-128, tglwe.rs:115-127: live outputs (rows of the wire table) and those of the level that has most (the widest
 * batch of key-switch rows is max_rows * batch); fhe_tfhe_circuit_info's max_width stays in nodes.  Each pointer may be NULL. */
int  fhe_tfhe_circuit_info_many(const fhe_tfhe_circuit *c, size_t *n_live_outputs, size_t *max_rows);

/* ---- circuit bootstrap (k = 1): a computed TLWE bit becomes the TGGSW selector of fhe_tggsw_cmux (tggsw.rs:114-121) ----
 * Gadget throughout: Base2Decomposor::<T64>::new(log_b, d) (decompose.rs:66-81, 114-135), g_j = 2^(64 - log_b d + j log_b), digits
 * those of fhe_torus_decompose, least significant first; rows of a digit x key product are digit-major (row = j rows_in + i, as in
 * fhe_tlwe_key_switch, tlwe.rs:144-153).
 *
 * Private functional key-switch key.  sk_in [n_in]: the binary key of the TLWE ciphertexts to switch (tlwe.rs:122-132); sk_out [n]: the
 * TGLWE key (tglwe.rs:91-103); funcs [n_funcs][n], 1 <= n_funcs <= 4: plaintext polynomials F_u as integer words (the circuit
 * bootstrap takes F_0 = -S, F_1 = 1).  pfksk [d (n_in + 1)][n_funcs][2][n]: at word offset ((j (n_in + 1) + i) n_funcs + u) 2 n stand
 * a [n], then b [n], of a TGLWE encryption under sk_out (b = a s + e + pt, tglwe.rs:91-103) of pt = w_i g_j F_u mod 2^64, w_i =
 * -sk_in[i] for i < n_in and w_{n_in} = 1 (the row of the ciphertext's b): b - a sk_out - pt is the drawn error of every row.  Draws
 * come under a purpose tag of this entry's own: no keystream is shared with fhe_tglwe_sk_encrypt on the same (rng, stream_id).
 * n: a ring the torus context serves; log_b d > 64, n_funcs outside 1 .. 4: FHE_ERR_INVALID. */
int fhe_tlwe_pfksk_gen(const fhe_torus_ctx *t, int log_b, int d, const uint64_t *sk_in, size_t n_in, const uint64_t *sk_out, size_t n,
                       const uint64_t *funcs, int n_funcs, double std_dev, const fhe_rng *rng, uint64_t stream_id, uint64_t *pfksk, fhe_mem mem,
                       void *stream);
/* The private functional key switch TLWE -> TGLWE (tlwe.rs:144-153's product against rows that are TGLWE ciphertexts, tglwe.rs:91-103).
 * With c = (ct_a[r][0 .. n_in - 1], ct_b[r]) of input r: out(r, u) = sum_j sum_i digit_j(c_i) * pfksk[j (n_in + 1) + i][u] over Z/2^64
 * on both halves, a TGLWE ciphertext whose phase is F_u times the phase of input r, plus the rounding of the digits.  ct_a
 * [batch][n_in], ct_b [batch]; out_a, out_b [batch n_funcs][n]; the row of (r, u) is ((r / group) n_funcs + u) group + r % group:
 * group = 1 is the plain [batch][n_funcs] order, group = d' with n_funcs = 2 the row order of a TGGSW ciphertext of d' levels
 * (tggsw.rs:79-88).  batch must be a multiple of group.  The outputs must not overlap the inputs or the key: FHE_MEM_DEVICE calls whose
 * out_a or out_b equals ct_a, ct_b or pfksk, and any call with out_a == out_b, return FHE_ERR_INVALID.  log_b > 31: FHE_ERR_UNSUPPORTED.
 * Every schedule (tile, row split, lab switch "PFKS_SPLIT") gives the same bits. */
int fhe_tlwe_pfks(int log_b, int d, const uint64_t *pfksk, int n_funcs, const uint64_t *ct_a, const uint64_t *ct_b, size_t n_in, size_t n,
                  size_t group, uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem, void *stream);
/* The test polynomial of the circuit bootstrap, the pattern of bootstrapping.rs:118-128 on raw torus values f_j(0) = 0, f_j(1) = g_j:
 * out[c] = T_{c mod 2^nu}[c - c mod 2^nu], nu = ceil(log2 cb_d), T_j[c] = g_j of (cb_log_b, cb_d) for n/4 <= c < 3n/4 and j < cb_d,
 * 0 elsewhere.  out [n], host memory.  cb_d outside 1 .. 16 or n/4 no multiple of 2^nu: FHE_ERR_INVALID; n outside 256 .. 2048:
 * FHE_ERR_UNSUPPORTED. */
int fhe_tfhe_cbs_table(int cb_log_b, int cb_d, size_t n, uint64_t *out);
/* Stream-ordered scratch of fhe_tfhe_circuit_bootstrap in 64-bit words (plus the n words of the table).  n no power of two, n_lwe = 0,
 * cb_d outside 1 .. 16: FHE_ERR_INVALID; n outside 256 .. 2048: FHE_ERR_UNSUPPORTED. */
int fhe_tfhe_cbs_workspace(size_t n, size_t n_lwe, int cb_d, size_t batch, size_t *words);
/* Circuit bootstrap in one call.  lwe_a [batch][n_lwe], lwe_b [batch]: TLWE encryptions (tlwe.rs:122-132) of a bit, pt = bit << 62.
 * Steps, all on `stream`: fhe_tfhe_mod_switch_many with nu = ceil(log2 cb_d) (bootstrapping.rs:99-104) -> fhe_tfhe_blind_rotate of
 * fhe_tfhe_cbs_table (84-96) -> sample_extract(j), j < cb_d (tglwe.rs:115-127; no TLWE key switch) -> fhe_tlwe_pfks with group =
 * cb_d under the two-function key pfksk (F_0 = -S, F_1 = 1; n_in = n; gadget (pf_log_b, pf_d)).  rows_a, rows_b [batch][2 cb_d][n]:
 * the rows of `batch` TGGSW ciphertexts of the bits in Tggsw::sk_encrypt's order (tggsw.rs:79-88), ready for fhe_tggsw_prepare /
 * fhe_tggsw_prepare_fft64 with count = batch.  Bit-identical to the four entries chained, in every exact key form (fft64: on the same
 * device).  The rows must not overlap an input: rows_a == rows_b, and FHE_MEM_DEVICE calls whose rows_a or rows_b equals lwe_a, lwe_b
 * or pfksk, return FHE_ERR_INVALID. */
int fhe_tfhe_circuit_bootstrap(const fhe_torus_ctx *t, const fhe_tggsw_key *brk, int cb_log_b, int cb_d, int pf_log_b, int pf_d,
                               const uint64_t *pfksk, const uint64_t *lwe_a, const uint64_t *lwe_b, uint64_t *rows_a, uint64_t *rows_b,
                               size_t batch, fhe_mem mem, void *stream);

/* ---- Encrypted table look-up with vertical packing (k = 1), every ciphertext under its own selectors ---------------------------------
 * A plaintext table T[o][x] of torus words, o < n_out outputs and x < 2^m addresses, shared by the batch, is read by ciphertext c under
 * the m TGGSW selectors of a prepared key at index first_index + c m + l, l = 0 the least significant address bit: the layout that
 * fhe_tfhe_circuit_bootstrap on bits ordered [c][l] followed by fhe_tggsw_prepare / _prepare_fft64 with count = batch m produces.
 *
 * Shape.  r = min(m, log2 n) address bits rotate a packed polynomial, h = m - r go to a CMUX tree; per_acc = max(1, n / 2^m) outputs
 * share one accumulator, n_acc = ceil(n_out / per_acc) accumulators, n_polys = n_acc 2^h polynomials.  Any output pointer may be NULL.
 * m < 1, n_out < 1, n no power of two: FHE_ERR_INVALID; n outside 256 .. 2048, h > 10, n_polys > 65536: FHE_ERR_UNSUPPORTED. */
int fhe_tfhe_lut_shape(int m, size_t n_out, size_t n, int *r, size_t *per_acc, size_t *n_acc, size_t *n_polys);
/* Packing, host memory only.  table [n_out][2^m] -> polys [n_acc][2^h][n]: polynomial (g, t) holds T[g per_acc + u][t 2^r + i] at
 * coefficient u 2^m + i, every other coefficient is 0.  Status as fhe_tfhe_lut_shape; a NULL pointer: FHE_ERR_INVALID. */
int fhe_tfhe_lut_pack(const uint64_t *table, int m, size_t n_out, size_t n, uint64_t *polys);
/* Stream-ordered scratch of fhe_tfhe_lut_eval in 64-bit words; n_lwe_out = 0: no key switch.  Status as fhe_tfhe_lut_shape; a batch whose
 * launches would pass 2^31 - 1 teams: FHE_ERR_UNSUPPORTED. */
int fhe_tfhe_lut_workspace(size_t n, int m, size_t n_out, size_t n_lwe_out, size_t batch, size_t *words);
/* The look-up in one call, all on `stream`.  Per ciphertext c and accumulator g: (1) tree level v = 0 .. h - 1 applies CMUX(selector r + v;
 * even, odd) (tggsw.rs:114-121) to neighbouring polynomials, starting from the trivial ciphertexts (0, polys[g][t]); (2) for l = 0 ..
 * r - 1, acc <- CMUX(selector l; acc, acc X^(-2^l)) (the rotation of fhe_tglwe_rotate with i = -2^l): coefficient u 2^m of the phase
 * is then T[g per_acc + u][address]; (3) sample_extract at u 2^m (tglwe.rs:115-127) for every output; (4) when ksk_a is not NULL,
 * fhe_tlwe_key_switch with (ks_log_b, ks_d, ksk_a, ksk_b) from n to n_lwe_out (tlwe.rs:144-153).  polys: fhe_tfhe_lut_pack's, where
 * the outputs live.  out_a [batch][n_out][n_lwe_out] ([batch][n_out][n] without key switch), out_b [batch][n_out].  Bit-identical per
 * ciphertext to fhe_tggsw_cmux with that ciphertext's index, fhe_tglwe_rotate, fhe_tglwe_sample_extract and fhe_tlwe_key_switch chained,
 * in every exact key form (fft64: on the same device).  The depth is m CMUXes, as for a tree over all m bits.
 * first_index + batch m > the key's count, a key of another context, ksk_b without ksk_a (or the reverse), out_a == out_b, and
 * FHE_MEM_DEVICE calls whose out_a or out_b equals polys, ksk_a or ksk_b: FHE_ERR_INVALID; shapes as fhe_tfhe_lut_shape. */
int fhe_tfhe_lut_eval(const fhe_torus_ctx *t, const fhe_tggsw_key *sel_key, size_t first_index, int m, const uint64_t *polys, size_t n_out,
                      int ks_log_b, int ks_d, const uint64_t *ksk_a, const uint64_t *ksk_b, size_t n_lwe_out, uint64_t *out_a, uint64_t *out_b,
                      size_t batch, fhe_mem mem, void *stream);

/* ---- Look-up without a padding bit (k = 1): an m-bit TLWE message -> its bits as selectors -> T[message] ----------------------------------
 * Input: TLWE ciphertexts under the key brk encrypts (dimension n_lwe) with phase x << (64 - m) + noise, 0 <= x < 2^m, NO padding bit;
 * bit l of x stands at delta_l = 64 - m + l.  nu = ceil(log2(cb_d + 1)); h_j = g_j / 2 for j < cb_d (g_j of the circuit bootstrap's
 * gadget), h_{cb_d} = 2^(delta_l - 1).  Steps l = 0 .. m - 1, all on `stream`, each after the one before:
 *   (1) rem_l = rem_{l-1} - corr_{l-1} (rem_0 = the input);  (2) s = rem_l 2^(m-1-l) over Z/2^64, + 2^62 on b (fhe_tlwe_lincomb): phase
 *   bit_l 2^63 + 2^62 + shifted noise;  (3) fhe_tfhe_mod_switch_many with nu;  (4) ONE fhe_tfhe_blind_rotate of fhe_tfhe_wop_table,
 *   P[c] = -h_{c mod 2^nu}: extraction j has phase -h_j for bit 0, +h_j for bit 1;  (5) fhe_tglwe_sample_extract(j) for j <= cb_d
 *   (j < cb_d in the last step) and h_j added to b: phase bit_l 2 h_j, that is bit_l g_j and bit_l 2^delta_l;  (6) except in the last
 *   step, fhe_tlwe_key_switch (ks_log_b, ks_d, ksk: n -> n_lwe) of row cb_d gives corr_l.
 * Then fhe_tlwe_pfks with group = cb_d over the batch m cb_d level rows in the order [c][l][j], under the circuit bootstrap's
 * two-function key: the TGGSW rows of batch m selectors in the order [c][l], l = 0 the least significant bit, which fhe_tfhe_lut_eval reads.
 * One blind rotation per bit serves every level of the selector AND the correction.
 *
 * The caller's conditions: the input noise times 2^(m-1) plus the mod-switch drift of 2^nu (n_lwe + 1) / 2 positions of the 2n stays
 * inside a quarter of the ring (n / 2 positions); cb_log_b cb_d <= 63, so that g_0 / 2 exists; m <= 16.  For cb_d a power of two nu is one
 * larger than fhe_tfhe_circuit_bootstrap's, and the drift twice as large.  (cb_d = 16 gives nu = 5, which fhe_tfhe_mod_switch_many itself does
 * not admit; these entries compute its formula.)
 *
 * The test polynomial of the step whose bit stands at log_delta, 1 <= log_delta <= 63; log_delta < 0: the last step's, without the
 * correction function.  out [n], host memory.  cb_d outside 1 .. 16, cb_log_b cb_d > 63, n/4 no multiple of 2^nu, log_delta = 0 or > 63:
 * FHE_ERR_INVALID; n outside 256 .. 2048: FHE_ERR_UNSUPPORTED. */
int fhe_tfhe_wop_table(int cb_log_b, int cb_d, size_t n, int log_delta, uint64_t *out);
/* Stream-ordered scratch of fhe_tfhe_wop_selectors in 64-bit words (fhe_tfhe_wop_pbs adds the selectors' rows, 4 batch m cb_d n words, and
 * then what fhe_tggsw_key_fill and fhe_tfhe_lut_eval take).  m < 1, n_lwe = 0, cb_d outside 1 .. 16, n/4 no multiple of 2^nu:
 * FHE_ERR_INVALID; m > 16, n outside 256 .. 2048: FHE_ERR_UNSUPPORTED. */
int fhe_tfhe_wop_workspace(size_t n, size_t n_lwe, int m, int cb_d, size_t batch, size_t *words);
/* The front of one step on its own, one pass over the batch (n_lwe + 1) words: rem = src - cor (cor_a, cor_b both NULL: rem = src),
 * s = rem 2^shift over Z/2^64 with 2^62 added to b, (at, bt) = fhe_tfhe_mod_switch_many(s) for the ring n with log_funcs = nu.  What
 * fhe_tlwe_lincomb {1, -1}, fhe_tlwe_lincomb {2^shift} + 2^62 and two fhe_tfhe_mod_switch_many calls compute, the same bits.  src, cor,
 * rem, at [batch][n_lwe] / [batch]; rem may be src (in place).  nu outside 0 .. 5 or above log2 n, shift outside 0 .. 63, cor_a without
 * cor_b, outputs equal to each other: FHE_ERR_INVALID. */
int fhe_tfhe_wop_front(const uint64_t *src_a, const uint64_t *src_b, const uint64_t *cor_a, const uint64_t *cor_b, size_t n_lwe, size_t batch,
                       size_t n, int nu, int shift, uint64_t *rem_a, uint64_t *rem_b, uint64_t *at, uint64_t *bt, fhe_mem mem, void *stream);
/* The bits as selectors.  lwe_a [batch][n_lwe], lwe_b [batch]; rows_a, rows_b [batch][m][2 cb_d][n]: the rows of batch m TGGSW
 * ciphertexts, ready for fhe_tggsw_key_fill / fhe_tggsw_prepare with count = batch m.  rem_a [batch][n_lwe], rem_b [batch]: both NULL,
 * or rem_{m-1}, the remainder after the last correction that exists, in which the top bit is still present.  ksk is read only for m > 1.
 * Bit-identical to the public entries named above chained, in every exact key form (fft64: on the same device).  Rejections as
 * fhe_tfhe_wop_table with m as fhe_tfhe_wop_workspace; outputs that are equal to each other, and FHE_MEM_DEVICE calls with an output
 * equal to lwe_a, lwe_b, ksk_a, ksk_b or pfksk: FHE_ERR_INVALID. */
int fhe_tfhe_wop_selectors(const fhe_torus_ctx *t, const fhe_tggsw_key *brk, int ks_log_b, int ks_d, const uint64_t *ksk_a, const uint64_t *ksk_b,
                           int cb_log_b, int cb_d, int pf_log_b, int pf_d, const uint64_t *pfksk, int m, const uint64_t *lwe_a, const uint64_t *lwe_b,
                           uint64_t *rows_a, uint64_t *rows_b, uint64_t *rem_a, uint64_t *rem_b, size_t batch, fhe_mem mem, void *stream);
/* T[message] in one call, all on `stream`: the selectors as above, fhe_tggsw_key_fill into sel_key at first_index (a key of
 * fhe_tggsw_key_reserve with the gadget (cb_log_b, cb_d), brk's ring and a capacity >= first_index + batch m), then fhe_tfhe_lut_eval of
 * polys (fhe_tfhe_lut_pack's) with its optional output key switch (out_ks_log_b, out_ks_d, out_ksk_a, out_ksk_b, n_lwe_out; both
 * pointers NULL: none).  Table words T[x] << (64 - m') give an output of the input's format, so calls compose.  Bit-identical to
 * fhe_tfhe_wop_selectors, fhe_tggsw_key_fill and fhe_tfhe_lut_eval chained.  Further rejections: a sel_key of another context, ring or
 * gadget, or sel_key == brk; those of fhe_tfhe_lut_eval. */
int fhe_tfhe_wop_pbs(const fhe_torus_ctx *t, const fhe_tggsw_key *brk, int ks_log_b, int ks_d, const uint64_t *ksk_a, const uint64_t *ksk_b, int cb_log_b,
                     int cb_d, int pf_log_b, int pf_d, const uint64_t *pfksk, int m, const uint64_t *lwe_a, const uint64_t *lwe_b, fhe_tggsw_key *sel_key,
                     size_t first_index, const uint64_t *polys, size_t n_out, int out_ks_log_b, int out_ks_d, const uint64_t *out_ksk_a,
                     const uint64_t *out_ksk_b, size_t n_lwe_out, uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem, void *stream);

/* ---- packing key switch (k = 1): many TLWE ciphertexts into one TGLWE ciphertext ----
 * The key is fhe_tlwe_pfksk_gen's with n_funcs = 1 and funcs = [1, 0, ..., 0] (the identity); gadget conventions as above.
 *
 * The prepared form: every row's a and b, once, in the evaluation domain of the context's two 60-bit primes -- an exact form for
 * every admitted gadget (R rows are summed before an inverse transform, R n 2^(64 + log_b) < 2^118; fhe_tlwe_pack cuts the rows into
 * such chunks itself), and keeps a device copy of the rows as they came: calls with count <= 16 run the scalar digits x key product of
 * fhe_tlwe_pfks on it and one rotate-and-add kernel, which is faster there (the key takes 3 x the words of pfksk on the device).
 * pfksk [d (n_in + 1)][1][2][n], read on `stream`; the entry returns when the prepared rows are complete, so
 * the key then serves calls on any stream.  log_b d > 64, n_in = 0, n not one of the context's rings (256 .. 2048):
 * FHE_ERR_INVALID; log_b > 31: FHE_ERR_UNSUPPORTED. */
typedef struct fhe_tlwe_pack_key fhe_tlwe_pack_key;
int  fhe_tlwe_pack_key_prepare(const fhe_torus_ctx *t, int log_b, int d, const uint64_t *pfksk, size_t n_in, size_t n, fhe_mem mem, void *stream,
                               fhe_tlwe_pack_key **out);
void fhe_tlwe_pack_key_destroy(fhe_tlwe_pack_key *key);
/* The packing key switch (tlwe.rs:144-153's digit x key product against rows that are TGLWE ciphertexts, tglwe.rs:91-103, each result
 * moved into place as tglwe.rs:61-66 rotates).  ct_a [packs][count][n_in], ct_b [packs][count]; out_a, out_b [packs][n].  With
 * c_{g,r,i} = ct_a[g][r][i] for i < n_in and c_{g,r,n_in} = ct_b[g][r], the TGLWE ciphertext out[g] is
 *   sum_{r < count} X^(r stride) * sum_j sum_{i <= n_in} digit_j(c_{g,r,i}) * pfksk[j (n_in + 1) + i]
 * over Z/2^64 on both halves, digits those of fhe_torus_decompose: its phase at coefficient r stride is the phase of input (g, r) plus
 * the rounding of the digits, elsewhere the phase is error only.  The same bits as fhe_tlwe_pfks (n_funcs = 1, group = 1) on the
 * packs count inputs, fhe_tglwe_rotate by r stride and the sum mod 2^64, in every schedule and on either route (lab switches
 * "PACK_SPLIT", "PACK_ROUTE", "PACK_SLAB").
 * count < 1, stride < 1, (count - 1) stride >= n, a key of another context: FHE_ERR_INVALID.  The outputs must not overlap the inputs:
 * FHE_MEM_DEVICE calls whose out_a or out_b equals ct_a or ct_b, and any call with out_a == out_b, return FHE_ERR_INVALID.  packs = 0:
 * FHE_OK, nothing touched.  Device-memory calls are stream ordered: no hipMalloc, no host wait; the digit polynomials (or the scalar route's rows)
 * are scratch from the library's stream-ordered pool. */
int fhe_tlwe_pack(const fhe_torus_ctx *t, const fhe_tlwe_pack_key *key, const uint64_t *ct_a, const uint64_t *ct_b, size_t count, size_t stride,
                  size_t packs, uint64_t *out_a, uint64_t *out_b, fhe_mem mem, void *stream);

/* ---- TGLWE ciphertext product (k = 1): tensor, exact division by 2^p, relinearisation ----
 * Ring Z[X]/(X^n + 1), n = 256 .. 2048.  s(w) is the word w read as a signed 64-bit integer (c64.rs:23-27, as fhe_torus_mul reads its
 * operands); the phase of (a, b) is b - a S (tglwe.rs:101, 110); rnd_p(x) = floor((x + 2^(p - 1)) / 2^p) per coefficient, 1 <= p <= 63.
 *   tensor : C2 = rnd_p(s(A1) s(A2)),  C1 = rnd_p(s(A1) s(B2) + s(B1) s(A2)),  C0 = rnd_p(s(B1) s(B2))   mod 2^64,
 *            the products and the sum over the INTEGERS (|coefficient| up to n 2^127); phase C0 - C1 S + C2 S^2
 *   key    : row j < d is a TGLWE encryption of h_j S^2, h_j = 2^(64 - log_b (d - j)) -- the weight of digit j of
 *            fhe_torus_decompose, least significant first, as in the rows of fhe_tggsw_encrypt --, S^2 the integer square of the binary
 *            key polynomial mod 2^64; rlk_a, rlk_b [d][n]
 *   relin  : out_a = C1 + sum_j digit_j(C2) RLK_j.a,  out_b = C0 + sum_j digit_j(C2) RLK_j.b   mod 2^64, digits those of
 *            fhe_torus_decompose(log_b, d); the same bits as fhe_tggsw_external_product of the pseudo-TGGSW [RLK rows; d zero rows]
 *            on (C2, 0), plus (C1, C0)
 *   mul    : relin(tensor(ct0, ct1, p)), those bits exactly
 * What the caller owns: with phases 2^p m_i + e_i (as integers, |phase| < 2^63) the product's phase is 2^p m1 m2 + m1 e2 + m2 e1 +
 * e1 e2 / 2^p, plus u e 2^(64 - p)-sized wrap terms whenever s(B) - s(A) S leaves [-2^63, 2^63) (|u| <= (n + 1) / 2), plus the
 * rounding of C0, C1 (1/2, ||S||_1 / 2), of C2 against S^2 (||S^2||_1 / 2), of the digits (n ||S^2||_inf 2^(63 - log_b d)) and the
 * key's noise times the digits; DESIGN.md 9.9 has the bound.  m1 m2 2^p must itself fit the torus.
 * Gadgets: log_b >= 1, d >= 1, log_b d <= 64, d n 2^(64 + log_b) < 2^118, else FHE_ERR_UNSUPPORTED.  Another n, p outside 1 .. 63, a
 * NULL pointer, a key of another context: FHE_ERR_INVALID.  Neither writes anything.  batch = 0: FHE_OK, nothing touched.
 * Device-memory calls are stream ordered: no hipMalloc, no host wait. */
typedef struct fhe_tglwe_relin_key fhe_tglwe_relin_key;
/* S^2 and the d plaintext rows h_j S^2 on the device, encrypted as fhe_tglwe_sk_encrypt encrypts `d` rows under (rng, stream_id): bit for
 * bit that entry's output on those plaintext rows.  sk [n] binary. */
int fhe_tglwe_rlk_gen(const fhe_torus_ctx *t, int log_b, int d, const uint64_t *sk, size_t n, double std_dev, const fhe_rng *rng, uint64_t stream_id,
                      uint64_t *rlk_a, uint64_t *rlk_b, fhe_mem mem, void *stream);
/* The rows in the evaluation domain of the context's two 60-bit primes.  Read on `stream`; the entry returns when the prepared rows are
 * complete, so the key then serves calls on any stream. */
int  fhe_tglwe_rlk_prepare(const fhe_torus_ctx *t, int log_b, int d, const uint64_t *rlk_a, const uint64_t *rlk_b, size_t n, fhe_mem mem, void *stream,
                           fhe_tglwe_relin_key **out);
void fhe_tglwe_rlk_destroy(fhe_tglwe_relin_key *key);
/* ct0, ct1 halves and c0, c1, c2: [batch][n].  Public so that several tensors can be added mod 2^64 and relinearised once.  The
 * [batch][n] ranges of the outputs must not overlap the inputs or each other: FHE_ERR_INVALID. */
int fhe_tglwe_tensor(const fhe_torus_ctx *t, const uint64_t *ct0_a, const uint64_t *ct0_b, const uint64_t *ct1_a, const uint64_t *ct1_b, size_t n,
                     int log_delta, uint64_t *c0, uint64_t *c1, uint64_t *c2, size_t batch, fhe_mem mem, void *stream);
/* (out_a, out_b) may be (c1, c0). */
int fhe_tglwe_relin(const fhe_torus_ctx *t, const fhe_tglwe_relin_key *key, const uint64_t *c0, const uint64_t *c1, const uint64_t *c2, uint64_t *out_a,
                    uint64_t *out_b, size_t batch, fhe_mem mem, void *stream);
/* One launch.  ct0 may be ct1 (a square); out may be either input: a team reads all it needs before it stores. */
int fhe_tglwe_mul(const fhe_torus_ctx *t, const fhe_tglwe_relin_key *key, const uint64_t *ct0_a, const uint64_t *ct0_b, const uint64_t *ct1_a,
                  const uint64_t *ct1_b, int log_delta, uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem, void *stream);

/* ---- TGLWE automorphism key switch, trace and ring packing (k = 1) ----
 * Ring Z[X]/(X^n + 1), n = 256 .. 2048, words mod 2^64, phase of (a, b) = b - a S; digit_j and h_j = 2^(64 - log_b (d - j)) those of
 * fhe_torus_decompose and of the relinearisation key above.
 *   sigma_g   : coefficient i of p goes to i g mod 2n; a position >= n means position - n with the sign flipped.  g odd, 1 <= g < 2n
 *   key       : AK_{g,j}, j < d: a TGLWE encryption of -h_j sigma_g(S) mod 2^64 under S; atk_a, atk_b [n_g][d][n] for the set gs [n_g]
 *   autks_g   : out_a = sum_j digit_j(sigma_g(a)) AK_{g,j}.a,  out_b = sigma_g(b) + sum_j digit_j(sigma_g(a)) AK_{g,j}.b   mod 2^64;
 *               phase = sigma_g(phase(a, b)) + the rounding of the digits + the key's noise times the digits
 *   trace     : for u = hi, hi - 1, ..., lo + 1: ct <- ct + autks_{2^u + 1}(ct), 0 <= lo < hi <= log2 n.  With hi = log2 n the
 *               coefficients at multiples of 2^(hi - lo) are kept, times 2^(hi - lo), and the others become zero; lo = 0 keeps
 *               coefficient 0 alone, times n
 *   embed     : the TLWE ciphertext (a'[n], b') under the coefficients of S -> the TGLWE ciphertext whose
 *               fhe_tglwe_sample_extract(index 0) it is: a[0] = a'[0], a[i] = -a'[n - i], b = b' at coefficient 0 and zero elsewhere
 *   merge_l   : (E, O) -> (E + X^(n/l) O) + autks_{l+1}(E - X^(n/l) O),  l = 2, 4, ..., count
 *   ring_pack : count = 2^c inputs, c <= log2 n: P(x) = embed(x) for one input, P(x_0 .. x_{m-1}) = merge_m(P(even-indexed),
 *               P(odd-indexed)); out = trace(P(all), lo = c, hi = log2 n) (count = n: P(all) itself).  n phase(x_r) sits at coefficient
 *               r (n / count) for every count, error only elsewhere.  It needs the keys g = 2^u + 1 for u = 1 .. log2 n
 * What the caller owns: every step doubles what it keeps, so phases leave multiplied by 2^(hi - lo), n for a pack: an input at scale
 * Delta decodes at n Delta and the top log2 n bits of its message space must be empty.  Noise: err <- 2 err + ks per step,
 * err_out <= n err_in + (n - 1) ks for a pack, ks = n 2^(63 - log_b d) (0 at log_b d = 64) + d n 2^(log_b - 1) |e_key|_inf; DESIGN.md
 * 9.10.  The packing key of fhe_tlwe_pack has d (n_in + 1) rows, this one d log2 n: a factor (n + 1) / log2 n, about 100 at n = 1024.
 * Gadgets: the rule of the relinearisation key (log_b >= 1, d >= 1, log_b d <= 64, d n 2^(64 + log_b) < 2^118), else
 * FHE_ERR_UNSUPPORTED.  Another n, an even g or g >= 2n, a g twice in a set or with no key in it, count not a power of two or > n,
 * lo >= hi or hi > log2 n, a NULL pointer, a key of another context: FHE_ERR_INVALID.  Rejected calls write nothing.  batch or
 * packs = 0: FHE_OK, nothing touched.  Device-memory calls are stream ordered: no hipMalloc, no host wait. */
typedef struct fhe_tglwe_auto_key fhe_tglwe_auto_key;
/* The n_g d plaintext rows -h_j sigma_g(S) on the device, encrypted as fhe_tglwe_sk_encrypt encrypts `n_g d` rows under (rng, stream_id):
 * bit for bit that entry's output on those plaintext rows.  sk [n] binary; gs [n_g] is a host array in both memory kinds, 1 <= n_g <= n. */
int fhe_tglwe_atk_gen(const fhe_torus_ctx *t, int log_b, int d, const uint64_t *sk, size_t n, const uint32_t *gs, size_t n_g, double std_dev,
                      const fhe_rng *rng, uint64_t stream_id, uint64_t *atk_a, uint64_t *atk_b, fhe_mem mem, void *stream);
/* The whole set in the evaluation domain of the context's two 60-bit primes (the layout and the transform of fhe_tglwe_rlk_prepare).
 * Read on `stream`; the entry returns when the prepared rows are complete, so the key then serves calls on any stream. */
int  fhe_tglwe_atk_prepare(const fhe_torus_ctx *t, int log_b, int d, const uint64_t *atk_a, const uint64_t *atk_b, size_t n, const uint32_t *gs, size_t n_g,
                           fhe_mem mem, void *stream, fhe_tglwe_auto_key **out);
void fhe_tglwe_atk_destroy(fhe_tglwe_auto_key *key);
/* autks_g on [batch][n] halves, one launch.  out may be the input (out_a == ct_a and out_b == ct_b: a team reads its ciphertext before
 * it stores); any other overlap among the four [batch][n] ranges: FHE_ERR_INVALID. */
int fhe_tglwe_automorphism(const fhe_torus_ctx *t, const fhe_tglwe_auto_key *key, uint32_t g, const uint64_t *ct_a, const uint64_t *ct_b, uint64_t *out_a,
                           uint64_t *out_b, size_t batch, fhe_mem mem, void *stream);
/* The hi - lo steps in ONE launch: the ciphertext stays in its team's registers, only the input and the result cross memory.  The same
 * bits as fhe_tglwe_automorphism and an addition mod 2^64 per step.  Aliasing as fhe_tglwe_automorphism. */
int fhe_tglwe_trace(const fhe_torus_ctx *t, const fhe_tglwe_auto_key *key, int lo, int hi, const uint64_t *ct_a, const uint64_t *ct_b, uint64_t *out_a,
                    uint64_t *out_b, size_t batch, fhe_mem mem, void *stream);
/* ct_a [packs][count][n], ct_b [packs][count] -> out_a, out_b [packs][n].  One launch per tree level over packs count / l teams (level
 * l = 2 reads the TLWE inputs: the embedding and the rotation by n / l are index arithmetic in the load), then the trace launch; count = 1
 * is embed + the full trace in one launch.  The inner levels are scratch from the library's stream-ordered pool; large `packs` run in
 * slabs (lab switch "PACK_SLAB").  The same bits as embed, fhe_tglwe_rotate, fhe_tglwe_automorphism and additions mod 2^64 composed.
 * The outputs must overlap neither the inputs nor each other: FHE_ERR_INVALID. */
int fhe_tlwe_ring_pack(const fhe_torus_ctx *t, const fhe_tglwe_auto_key *key, const uint64_t *ct_a, const uint64_t *ct_b, size_t count, size_t packs,
                       uint64_t *out_a, uint64_t *out_b, fhe_mem mem, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FHE_RING_H */
