// gg_pattern.hip - the pattern planes (gg_pattern.h) with their entry points (gg_pattern_planes, gg_batch_patterns,
// gg_batch_patterns_tracked) as a translation unit of their own, compiled with the default code-generation switches: the machine
// code of every kernel of the other units - and the hashes bench.py ties their PMC records to - does not depend on anything
// in here.  The launch path is plane_launch of gg_planes.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gymgo_amd_pattern.h"
#include "gg_pattern.h"

namespace {

using namespace gg;

struct PatternCall {
  const void *in;
  const int32_t *last, *orient;
  uint8_t *out;
  int64_t B;
  int32_t N;
  template <int R, bool TRACKED>
  void launch(unsigned grid, hipStream_t s, int esh, uint32_t one) const {
    k_patterns<R, TRACKED><<<grid, kWave, 0, s>>>(in, last, orient, out, esh, one, B, N);
  }
};

int32_t batch_patterns(bool tracked, const void *in, const int32_t *last, const int32_t *orient, void *out, int32_t dtype, int64_t B,
                       int32_t N, void *hip_stream) {
  return plane_launch(PatternCall{in, last, orient, static_cast<uint8_t *>(out), B, N}, tracked, in, out, out, 0, dtype, B, N, hip_stream);
}

}  // namespace

extern "C" {

int32_t gg_pattern_planes(void) { return gg::kPatternPlanes; }

int32_t gg_batch_patterns(const uint8_t *states, const int32_t *last, const int32_t *orient, void *out, int32_t out_dtype, int64_t B,
                          int32_t N, void *hip_stream) {
  return batch_patterns(false, states, last, orient, out, out_dtype, B, N, hip_stream);
}

int32_t gg_batch_patterns_tracked(const uint32_t *tracked, const int32_t *last, const int32_t *orient, void *out, int32_t out_dtype,
                                  int64_t B, int32_t N, void *hip_stream) {
  return batch_patterns(true, tracked, last, orient, out, out_dtype, B, N, hip_stream);
}

}  // extern "C"
