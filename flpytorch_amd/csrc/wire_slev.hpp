// The encode -> staged sparse level lists pass of flc_pack_slev (wire_slev.hip), reached from ew_run
// (codecs.hip) with the codec functor it has set up: the functors that have the sparse level form
// (standard dithering with a level table) and the launch over them, instantiated in wire_slev.hip.
#pragma once
#include <type_traits>

#include "codec_ops.hpp"
#include "wire_codes.hpp"

namespace flc {

template <class Op> struct SlevOp : std::false_type {};
template <bool COMPAT> struct SlevOp<DitherOp<false, COMPAT>> : std::true_type {};

template <class Op>
int launch_code_slev(const float* x, int64_t d, Op op, const float* levels, int s, const CodeArgs& ca, hipStream_t st);

}  // namespace flc
