// gg_area.hip - the area ownership planes (gg_area.h) with their entry points (gg_area_planes, gg_batch_area,
// gg_batch_area_tracked) as a translation unit of their own, compiled with the default code-generation switches: the machine
// code of every kernel of the other units - and the hashes bench.py ties their PMC records to - does not depend on anything
// in here.  The launch path is plane_launch of gg_planes.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gymgo_amd_area.h"
#include "gg_area.h"

namespace {

using namespace gg;

struct AreaCall {
  const void *in;
  const int32_t *orient;
  const uint8_t *side;
  uint8_t *out;
  int32_t *counts;
  int64_t B;
  int32_t N;
  template <int R, bool TRACKED>
  void launch(unsigned grid, hipStream_t s, int esh, uint32_t one) const {
    k_area<R, TRACKED><<<grid, kWave, 0, s>>>(in, orient, side, out, counts, esh, one, B, N);
  }
};

int32_t batch_area(bool tracked, const void *in, const int32_t *orient, const uint8_t *side, void *out, int32_t *counts,
                   int32_t dtype, int64_t B, int32_t N, void *hip_stream) {
  return plane_launch(AreaCall{in, orient, side, static_cast<uint8_t *>(out), counts, B, N}, tracked, in, out, out, 0, dtype, B, N,
                      hip_stream);
}

}  // namespace

extern "C" {

int32_t gg_area_planes(void) { return gg::kAreaPlanes; }

int32_t gg_batch_area(const uint8_t *states, const int32_t *orient, const uint8_t *side, void *out, int32_t *counts,
                      int32_t out_dtype, int64_t B, int32_t N, void *hip_stream) {
  return batch_area(false, states, orient, side, out, counts, out_dtype, B, N, hip_stream);
}

int32_t gg_batch_area_tracked(const uint32_t *tracked, const int32_t *orient, const uint8_t *side, void *out, int32_t *counts,
                              int32_t out_dtype, int64_t B, int32_t N, void *hip_stream) {
  return batch_area(true, tracked, orient, side, out, counts, out_dtype, B, N, hip_stream);
}

}  // extern "C"
