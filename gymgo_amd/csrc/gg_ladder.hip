// gg_ladder.hip - the ladder planes (gg_ladder.h) with their entry points (gg_batch_ladder, gg_batch_ladder_tracked) as a
// translation unit of their own, compiled with the default code-generation switches: the machine code of every kernel of the
// other units - and the hashes bench.py ties their PMC records to - does not depend on anything in here.  The launch path is
// plane_launch of gg_planes.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gymgo_amd.h"
#include "gg_ladder.h"

namespace {

using namespace gg;

struct LadderCall {
  const void *in;
  const int32_t *orient;
  uint8_t *out, *aborted;
  int64_t B;
  int32_t N;
  template <int R, bool TRACKED>
  void launch(unsigned grid, hipStream_t s, int esh, uint32_t one) const {
    k_ladder<R, TRACKED><<<grid, kWave, 0, s>>>(in, orient, out, aborted, esh, one, B, N);
  }
};

int32_t batch_ladder(bool tracked, const void *in, const int32_t *orient, void *out, uint8_t *aborted, int32_t dtype, int64_t B,
                     int32_t N, void *hip_stream) {
  return plane_launch(LadderCall{in, orient, static_cast<uint8_t *>(out), aborted, B, N}, tracked, in, out, out, 0, dtype, B, N,
                      hip_stream);
}

}  // namespace

extern "C" {

static_assert(gg::kLadderPlanes == GG_LADDER_PLANES && gg::Ladder<19>::kLevels == GG_LADDER_DEPTH(19), "the header's constants");

int32_t gg_batch_ladder(const uint8_t *states, const int32_t *orient, void *out, uint8_t *aborted, int32_t out_dtype, int64_t B,
                        int32_t N, void *hip_stream) {
  return batch_ladder(false, states, orient, out, aborted, out_dtype, B, N, hip_stream);
}

int32_t gg_batch_ladder_tracked(const uint32_t *tracked, const int32_t *orient, void *out, uint8_t *aborted, int32_t out_dtype,
                                int64_t B, int32_t N, void *hip_stream) {
  return batch_ladder(true, tracked, orient, out, aborted, out_dtype, B, N, hip_stream);
}

}  // extern "C"
