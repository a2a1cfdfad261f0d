// gg_tactics.hip - the tactical planes (gg_tactics.h) with their entry points (gg_tactics_planes, gg_batch_tactics,
// gg_batch_tactics_tracked) as a translation unit of their own, compiled with the default code-generation switches: the machine
// code of every kernel of the other units - and the hashes bench.py ties their PMC records to - does not depend on anything
// in here.  The launch path is plane_launch of gg_planes.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gymgo_amd_tactics.h"
#include "gg_tactics.h"

namespace {

using namespace gg;

struct TacticsCall {
  const void *in;
  const int32_t *orient;
  uint8_t *out;
  int64_t B;
  int32_t N;
  template <int R, bool TRACKED>
  void launch(unsigned grid, hipStream_t s, int esh, uint32_t one) const {
    k_tactics<R, TRACKED><<<grid, kWave, 0, s>>>(in, orient, out, esh, one, B, N);
  }
};

int32_t batch_tactics(bool tracked, const void *in, const int32_t *orient, void *out, int32_t dtype, int64_t B, int32_t N,
                      void *hip_stream) {
  return plane_launch(TacticsCall{in, orient, static_cast<uint8_t *>(out), B, N}, tracked, in, out, out, 0, dtype, B, N, hip_stream);
}

}  // namespace

extern "C" {

int32_t gg_tactics_planes(void) { return gg::kTacticsPlanes; }

int32_t gg_batch_tactics(const uint8_t *states, const int32_t *orient, void *out, int32_t out_dtype, int64_t B, int32_t N,
                         void *hip_stream) {
  return batch_tactics(false, states, orient, out, out_dtype, B, N, hip_stream);
}

int32_t gg_batch_tactics_tracked(const uint32_t *tracked, const int32_t *orient, void *out, int32_t out_dtype, int64_t B, int32_t N,
                                 void *hip_stream) {
  return batch_tactics(true, tracked, orient, out, out_dtype, B, N, hip_stream);
}

}  // extern "C"
