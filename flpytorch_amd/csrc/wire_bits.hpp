// The encode -> bit-packed code pass of flc_pack_bits (wire_bits.hip), reached from ew_run
// (codecs.hip) with the codec functor it has set up: the functors that have a bit-packed form and
// the launch over them, instantiated in wire_bits.hip.
#pragma once
#include <type_traits>

#include "codec_ops.hpp"
#include "wire_codes.hpp"

namespace flc {

template <class Op> struct BitsOp : std::false_type {};
template <bool COMPAT> struct BitsOp<DitherOp<false, COMPAT>> : std::true_type {};
template <bool COMPAT> struct BitsOp<NaturalOp<COMPAT>> : std::true_type {};

template <class Op>
int launch_code_bits(const float* x, int64_t d, Op op, const float* levels, int s, const CodeArgs& ca, hipStream_t st);

// the same pass over a - b with the shift epilogues (flc_pack_shift_bits), instantiated in
// wire_shift_bits.hip
template <class Op>
int launch_shift_code_bits(const float* a, int64_t d, Op op, const float* levels, int s, const ShiftArgs& sh,
                           const CodeArgs& ca, hipStream_t st);

// one statement per width of the bit-packed forms: CASE(2) .. CASE(7), CASE(9)
#define FLC_BITS_SWITCH(b, CASE)                                                                   \
    switch (b) {                                                                                   \
        case 2: CASE(2) break; case 3: CASE(3) break; case 4: CASE(4) break; case 5: CASE(5) break; \
        case 6: CASE(6) break; case 7: CASE(7) break; default: CASE(9) break;                      \
    }

}  // namespace flc
