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

}  // namespace flc
