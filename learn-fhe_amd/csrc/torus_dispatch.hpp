// The team shapes of the torus kernels per ring degree and the dispatcher that turns a key's log2 N into one of them: shared by the
// translation units that launch those kernels (torus_api.hip, tfhe_lut_api.hip).
#pragma once
#include "dispatch.hpp"
#include "fhew_kernels.hpp"

namespace {

// the team shape of the torus kernels per ring degree: 4 coefficients per lane from N = 1024 up (the state of a CMUX -- accumulator,
// difference, digit state, two unreduced sum pairs -- is heavier than FHEW's; measured at cfg5: 17.2-17.3 k gates/s against
// 16.6-16.9 k with 8 per lane, same session, and the better shape for small batches as well)
template <int LN>
using TorusRing = fhe::WaveRing<LN, (LN <= 9 ? LN - 6 : 2)>;
// the 30-bit path carries half the registers per coefficient: 8 per lane again (22.9 k against 21.8 k gates/s at cfg5)
template <int LN>
using TorusRing30 = fhe::WaveRing<LN, (LN <= 9 ? LN - 6 : 3)>;

// fft64 mode: a team over the N / 2 complex slots of a polynomial, 4 slots per lane from N = 1024 up (two waves per SIMD)
template <int LN>
using TorusRingF = fhe::WaveRing<LN - 1, (LN - 1 <= 8 ? LN - 1 - 6 : 2)>;
constexpr int TF_MIN_WAVES = 2;

// f(Type<Ring<LN>>{}) for the ring sizes of the torus kernels, N = 256 .. 2048; Ring: TorusRing, TorusRing30 or TorusRingF
template <template <int> class Ring, class F>
int with_torus(int log_n, F &&f) {
    return fhe::with_int<8, 9, 10, 11>(log_n, [&](auto ln) { return f(fhe::Type<Ring<decltype(ln)::value>>{}); });
}

}  // namespace
