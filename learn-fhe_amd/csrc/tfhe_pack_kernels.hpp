// Packing key switch: `count` TLWE ciphertexts into ONE TGLWE ciphertext (tlwe.rs:144-153's digit x key product over tglwe.rs:91-103's
// ciphertexts, each result times X^(r stride) as tglwe.rs:61-66 rotates, summed) as a sum of polynomial products:
//   out[g] = sum_{j, i} D_{g,j,i}(X) * key[j (n_in + 1) + i]  in Z_{2^64}[X]/(X^n + 1),   D_{g,j,i}(X) = sum_r digit_j(c_{g,r,i}) X^(r stride)
// Two kernels (a third, tlwe_pack_gather_kernel at the end, closes the scalar route that small counts take instead):
//   * tlwe_pack_digits_kernel, the front pass: transposes and decomposes.  A block owns 64 input coefficients i x 64 ciphertexts r of one
//     pack: it reads ct_a[g][r][i0 .. i0 + 63] (contiguous in i) into an LDS tile, then writes, for every digit j, digit_j at coefficient
//     r stride of polynomial (g, j (n_in + 1) + i) (contiguous in r at stride 1).  Digits are stored narrow (tfhe_pack.hpp:
//     pack_digit_bytes); the coefficients nobody writes are zero from a memset in front.
//   * tlwe_pack_kernel, the product: one team (fhew_kernels.hpp: WaveRing) owns (pack, chunk of key rows).  Per row it loads the digit
//     polynomial into registers, runs the forward transform and multiply-accumulates against the row's prepared a and b (one row ahead,
//     as the external product loads them); after the chunk two inverse transforms, for each of the two 60-bit primes in turn (the first
//     prime's residues wait in the team's LDS parking area), then the Chinese remainder to the signed integer mod 2^64.  One chunk per
//     pack: plain stores.  Several: 64-bit atomic adds into outputs that are ZERO before the launch -- additions mod 2^64 commute, so
//     every split gives the same bits.  No waits between workgroups.
// The front pass is a kernel of its own: fused, a team would fetch ct_a[g][r][i] for its one row i and every r -- a column walk of
// `count` 64-byte lines for 8 bytes each -- or keep an i-tile of all `count` ciphertexts in LDS (64 KiB at 8 x 1024), which the
// multi-wave teams of n >= 1024 have no room for beside their exchange image.
#pragma once
#include "dispatch.hpp"  // launch()
#include "torus_kernels.hpp"

namespace fhe {

constexpr int PACK_TILE = 64;

struct PackShape {
    unsigned n_in, n, count, stride, rows;  // rows = d (n_in + 1)
};

// grid (ceil((n_in + 1) / 64), ceil(count / 64), packs); 256 threads.  dig [packs][rows][n], zero where no digit lands
template <class D>
__global__ __launch_bounds__(256) void tlwe_pack_digits_kernel(const u64 *__restrict__ ct_a, const u64 *__restrict__ ct_b, D *__restrict__ dig, PackShape S,
                                                               TDecomp P) {
    __shared__ u64 tile[PACK_TILE][PACK_TILE + 1];  // [r][i], the rounded values the digits come from
    const unsigned rows_in = S.n_in + 1, g = blockIdx.z, i0 = blockIdx.x * PACK_TILE, r0 = blockIdx.y * PACK_TILE;
    const unsigned tx = threadIdx.x & (PACK_TILE - 1), ty = threadIdx.x / PACK_TILE;
    for (unsigned k = ty; k < PACK_TILE; k += 256 / PACK_TILE) {
        const unsigned r = r0 + k, i = i0 + tx;
        u64 v = 0;
        if (r < S.count && i < rows_in) {
            const size_t ct = size_t(g) * S.count + r;
            v = i < S.n_in ? ct_a[ct * S.n_in + i] : ct_b[ct];
        }
        tile[k][tx] = tdecomp_init(v, P);
    }
    __syncthreads();
    for (unsigned k = ty; k < PACK_TILE; k += 256 / PACK_TILE) {
        const unsigned i = i0 + k, r = r0 + tx;
        if (i >= rows_in || r >= S.count) continue;
        u64 st = tile[tx][k];
        D *dst = dig + (size_t(g) * S.rows + i) * S.n + size_t(r) * S.stride;  // (count - 1) stride < n
        for (int j = 0; j < P.d; ++j) {
            dst[size_t(j) * rows_in * S.n] = (D)(long long)tdecomp_next(st, P);
        }
    }
}

// a prepared packing key: evaluation-domain rows per prime, [rows][2][N] in key_perm layout (fhew_kernels.hpp)
struct PackKeyArg {
    const u64 *__restrict__ rows0, *__restrict__ rows1;
    TorusConsts T;
};

// in [polys][N] evaluation-domain residues (natural evaluation order) -> out [polys][N], key_perm layout, the pseudo-Mersenne packed
// operand form: key_permute_kernel for rows whose a and b halves alternate (a key row of fhe_tlwe_pfksk_gen is [2][n])
template <class W>
FHE_HEADER_KERNEL void pack_key_permute_kernel(const u64 *__restrict__ in, u64 *__restrict__ out, size_t polys, int pm_b) {
    constexpr int N = 1 << W::LOG_N;
    const size_t total = polys * N;
    const u64 lo_mask = (u64(1) << (pm_b - 31)) - 1;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const size_t poly = idx >> W::LOG_N;
        const u64 v = in[idx];
        out[poly * N + key_perm<W>(int(idx & (N - 1)))] = ((v >> (pm_b - 31)) << 32) | (v & lo_mask);
    }
}

template <class W, class D>
__device__ __forceinline__ void pack_load_digits(const D *__restrict__ row, int lane, int (&dg)[W::E]) {
#pragma unroll
    for (int e = 0; e < W::E; ++e) dg[e] = (int)row[coef_index<W>(lane, e)];
}

// One prime's pass over a chunk: the residues mod p of sum_rows D_row * key[row].a and ... .b, coefficient layout.  team_torus_gadget
// (torus_kernels.hpp) with the digits read from memory instead of decomposed from an accumulator.
template <class W, class D>
__device__ __forceinline__ void team_pack_pass(const D *__restrict__ dig, const u64 *__restrict__ rows, unsigned nrows, u64 p, int lane, u64 *lds,
                                               const Barrett &B, const typename ArithPM<60>::K &k, u64 (&sa)[W::E], u64 (&sb)[W::E]) {
    using A = ArithPM<60>;
    constexpr int E = W::E;
    RingConsts K;
    K.desc = nullptr;
    K.B = B;
    typename A::MacAcc ma[E], mb[E];
#pragma unroll
    for (int e = 0; e < E; ++e) ma[e] = mb[e] = A::mac_zero();
    KeyRow<W> kr;  // one row ahead
    load_row<W>(kr, rows, lane);
    int dg[E];
    pack_load_digits<W, D>(dig, lane, dg);
#pragma unroll 1
    for (unsigned j = 0; j < nrows; ++j) {
        u64 x[E];
#pragma unroll
        for (int e = 0; e < E; ++e) x[e] = dg[e] < 0 ? p - u64(-(long long)dg[e]) : u64(dg[e]);  // |digit| <= 2^30 < p
        if (j + 1 < nrows) pack_load_digits<W, D>(dig + size_t(j + 1) * W::N, lane, dg);
        fwd_run<A, typename W::C, W::LOG_N, W::LOG_E, 0, true, W::WAVE>(x, lane, nullptr, lds, true, k);
        mac_row<A, W>(x, ma, mb, kr, (int)j, K, k);
        if (j + 1 < nrows) load_row<W>(kr, rows + size_t(j + 1) * 2 * W::N, lane);
    }
#pragma unroll
    for (int e = 0; e < E; ++e) { sa[e] = A::mac_finish(ma[e], k); sb[e] = A::mac_finish(mb[e], k); }
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
        inv_run<A, typename W::C, W::LOG_N, W::LOG_E, W::LOG_N, true, W::WAVE>(sa, lane, nullptr, lds, true, k);
#pragma unroll
        for (int e = 0; e < E; ++e) { const u64 t = sa[e]; sa[e] = sb[e]; sb[e] = t; }
    }
}

// Workgroups are dealt round-robin over the chip's 8 dies, each with an L2 of its own, so workgroups b and b + 8 share one.  Team q of
// the workgroups b = x (mod 8) owns pack q % packs and chunk (q / packs) 8 + x: the teams that read the same key rows -- one per pack --
// run side by side behind the same L2, which fetches a row once for all of them (a placement for speed only: any other gives the
// same bits).  pack_team_blocks(chunks, packs) workgroups; teams whose chunk is past the last return at once.  dynamic LDS:
// W::TORUS_LDS_BYTES.  chunks > 1: out_a, out_b are zero before the launch.
constexpr unsigned PACK_DIES = 8;
template <class W>
inline size_t pack_team_blocks(size_t chunks, size_t packs) {
    const size_t per_die = (chunks + PACK_DIES - 1) / PACK_DIES * packs;
    return PACK_DIES * ((per_die + W::TEAMS - 1) / W::TEAMS);
}
template <class W, class D>
__global__ __launch_bounds__(W::THREADS, W::MIN_WAVES) void tlwe_pack_kernel(const D *__restrict__ dig, PackKeyArg key, unsigned rows, unsigned per_chunk,
                                                                             unsigned chunks, unsigned packs, u64 *__restrict__ out_a,
                                                                             u64 *__restrict__ out_b) {
    using A = ArithPM<60>;
    constexpr int E = W::E, N = W::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = W::lane(), team = W::team();
    const unsigned q = (blockIdx.x / PACK_DIES) * W::TEAMS + team, g = q % packs, chunk = (q / packs) * PACK_DIES + blockIdx.x % PACK_DIES;
    if (chunk >= chunks) return;  // team-uniform exit (a multi-wave team is a whole block: barriers stay matched)
    u64 *lds = reinterpret_cast<u64 *>(smem_raw) + team * W::TORUS_LDS_WORDS, *park = lds + W::PN;
    const unsigned row0 = chunk * per_chunk, nrows = min(per_chunk, rows - row0);
    const D *dg = dig + (size_t(g) * rows + row0) * N;
    const size_t koff = size_t(row0) * 2 * N;
    u64 xa[E], xb[E];
    {
        const typename A::K k0 = A::make(key.T.descs[0], W::LOG_N, 0, 0);
        team_pack_pass<W, D>(dg, key.rows0 + koff, nrows, key.T.p0, lane, lds, key.T.B0, k0, xa, xb);
#pragma unroll
        for (int e = 0; e < E; ++e) { park[e * W::TEAM + lane] = xa[e]; park[(E + e) * W::TEAM + lane] = xb[e]; }
    }
    {
        const typename A::K k1 = A::make(key.T.descs[1], W::LOG_N, 0, 0);
        team_pack_pass<W, D>(dg, key.rows1 + koff, nrows, key.T.p1, lane, lds, key.T.B1, k1, xa, xb);
    }
    u64 *ga = out_a + size_t(g) * N, *gb = out_b + size_t(g) * N;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const u64 va = crt2_mod64(park[e * W::TEAM + lane], xa[e], key.T), vb = crt2_mod64(park[(E + e) * W::TEAM + lane], xb[e], key.T);
        const int c = coef_index<W>(lane, e);
        if (chunks > 1) {
            atomicAdd(reinterpret_cast<unsigned long long *>(ga + c), (unsigned long long)va);
            atomicAdd(reinterpret_cast<unsigned long long *>(gb + c), (unsigned long long)vb);
        } else {
            ga[c] = va;
            gb[c] = vb;
        }
    }
}

// The closing step of the scalar route (small counts; tfhe_pack.hpp: pack_scalar_route): in_a, in_b [packs][count][n] are the outputs of
// fhe_tlwe_pfks on the inputs; out[g] = sum_r in[g][r] X^(r stride) (tglwe.rs:61-66 on each, r stride < n: one wrap at most), both halves.
// One thread per (half, pack, coefficient); lanes read consecutive words of one input at a time.
FHE_HEADER_KERNEL void tlwe_pack_gather_kernel(const u64 *__restrict__ in_a, const u64 *__restrict__ in_b, unsigned n, unsigned count, unsigned stride,
                                               size_t packs, u64 *__restrict__ out_a, u64 *__restrict__ out_b) {
    const size_t half_words = packs * n, total = 2 * half_words;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const bool is_b = idx >= half_words;
        const size_t w = is_b ? idx - half_words : idx, g = w / n;
        const unsigned k = unsigned(w - g * n);
        const u64 *src = (is_b ? in_b : in_a) + g * count * n;
        u64 acc = 0;
        for (unsigned r = 0; r < count; ++r) {
            const unsigned sh = r * stride;  // < n
            const u64 v = src[size_t(r) * n + (k >= sh ? k - sh : k + n - sh)];
            acc += k >= sh ? v : u64(0) - v;
        }
        (is_b ? out_b : out_a)[w] = acc;
    }
}

}  // namespace fhe
