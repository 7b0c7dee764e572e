// Which team kernel a prepared fhe_tggsw_key runs: the team shapes of the torus kernels per ring degree, and with_key_form, the ONE place
// that reads which form a key is in and turns it, with the key's log2 N, into a form policy of torus_forms.hpp and that policy's kernel
// argument.  Shared by the translation units that launch those kernels (torus_api.hip, tfhe_lut_api.hip).
#pragma once
#include "dispatch.hpp"
#include "torus_ctx.hpp"
#include "torus_forms.hpp"

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

// f(Type<Ring<LN>>{}) for the ring sizes of the torus kernels, N = 256 .. 2048; Ring: TorusRing, TorusRing30 or TorusRingF
template <template <int> class Ring, class F>
int with_torus(int log_n, F &&f) {
    return fhe::with_int<8, 9, 10, 11>(log_n, [&](auto ln) { return f(fhe::Type<Ring<decltype(ln)::value>>{}); });
}

// Whether a 30-bit key runs the CMUX whose digits are computed once, where the caller's kernels allow it (with_key_form<true>): base <= 2^7
// and at most 8 limbs (cfg5: base 2^7, d = 3): the digits are parked as bytes, the multiply-accumulate runs unreduced
// (torus30_kernels.hpp); a digit of base 2^8 ranges over [-128, 128]: one value too many for a byte.  The lab switch NO_PACKED_DIGITS
// keeps the older kernel (bit-identical); it is read here, at the launch.  The ONE statement of the rule: with_key_form and
// fhe_tggsw_key_form both ask it.
inline bool key_packs_digits(const fhe_tggsw_key *key) {
    return key->d_rows30 != nullptr && !key->d_rowsf && !key->d_rowsx3 && key->P.log_b <= 7 && 2 * key->d <= 8 && key->log_n >= 8 &&
           fhe::opt(fhe::OPT_NO_PACKED_DIGITS) == 0;
}

// The form as fhe_tggsw_key_form reports it (FHE_TGGSW_FORM_*): the pointers with_key_form reads, in its order
inline int key_form(const fhe_tggsw_key *key) {
    if (key->d_rowsx3) return FHE_TGGSW_FORM_X3;
    if (key->d_rowsf) return FHE_TGGSW_FORM_FFT64;
    return key->d_rows30 ? FHE_TGGSW_FORM_30 : FHE_TGGSW_FORM_60;
}

// f(Type<Form>{}, key_arg, lds_bytes) for the form `key` is in: Form the policy over the key's ring, key_arg its Form::Key with the rows
// offset to entry first_index, lds_bytes the dynamic LDS of a workgroup.  ALLOW_PACKED: a 30-bit key may run the CMUX whose digits are
// computed once; the callers whose kernels run the plain external product (and the key fill) pass false.
template <bool ALLOW_PACKED, class F>
int with_key_form(const fhe_torus_ctx *t, const fhe_tggsw_key *key, size_t first_index, F &&f) {
    const fhe::TDecomp &P = key->P;
    if (key->d_rowsf || key->d_rowsx3) {  // fft64 mode, or exact: three key pieces through f64 transforms
        return with_torus<TorusRingF>(key->log_n, [&](auto wr) {
            return fhe::with_bool(key->d_rowsx3 != nullptr, [&](auto x3) {
                using Form = fhe::FormF<typename decltype(wr)::type, decltype(x3)::value>;
                const double2 *rows = (x3 ? key->d_rowsx3 : key->d_rowsf) + first_index * Form::per(P);
                return f(fhe::Type<Form>{}, typename Form::Key{rows, P, t->d_twf}, Form::lds_bytes(key->d));
            });
        });
    }
    if (key->d_rows30) {  // three 30-bit primes
        const bool packed = ALLOW_PACKED && key_packs_digits(key);
        return with_torus<TorusRing30>(key->log_n, [&](auto wr) {
            auto run = [&](auto pk) {
                using Form = fhe::Form30<typename decltype(wr)::type, decltype(pk)::value>;
                const size_t per = Form::per(P);
                return f(fhe::Type<Form>{}, typename Form::Key{key->d_rows30 + first_index * per, key->count * per, P, t->T30}, Form::lds_bytes(key->d));
            };
            if constexpr (ALLOW_PACKED) {  // a caller that never packs compiles no packed kernel
                if (packed) return run(std::true_type{});
            }
            return run(std::false_type{});
        });
    }
    return with_torus<TorusRing>(key->log_n, [&](auto wr) {  // two 60-bit primes
        using Form = fhe::Form60<typename decltype(wr)::type>;
        const size_t off = first_index * Form::per(P);
        return f(fhe::Type<Form>{}, typename Form::Key{key->d_rows[0] + off, key->d_rows[1] + off, P, t->T}, Form::lds_bytes(key->d));
    });
}

// the blind-rotation kernel of a form: one name per form (torus_forms.hpp)
template <class W> constexpr auto blind_rotate_kernel(fhe::Type<fhe::Form60<W>>) { return &fhe::torus_blind_rotate_kernel<W>; }
template <class W> constexpr auto blind_rotate_kernel(fhe::Type<fhe::Form30<W, false>>) { return &fhe::torus30_blind_rotate_kernel<W>; }
template <class W> constexpr auto blind_rotate_kernel(fhe::Type<fhe::Form30<W, true>>) { return &fhe::torus30_blind_rotate_pk_kernel<W>; }
template <class W> constexpr auto blind_rotate_kernel(fhe::Type<fhe::FormF<W, false>>) { return &fhe::torusf_blind_rotate_kernel<W>; }
template <class W> constexpr auto blind_rotate_kernel(fhe::Type<fhe::FormF<W, true>>) { return &fhe::torusx3_blind_rotate_kernel<W>; }

}  // namespace
