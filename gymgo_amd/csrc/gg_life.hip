// gg_life.hip - the pass-alive life planes (gg_life.h) with their entry points (gg_life_planes, gg_batch_life,
// gg_batch_life_tracked) as a translation unit of their own, compiled with the default code-generation switches: the machine
// code of every kernel of the other units - and the hashes bench.py ties their PMC records to - does not depend on anything
// in here.  The launch path is plane_launch of gg_planes.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gymgo_amd.h"
#include "gg_life.h"

namespace {

using namespace gg;

struct LifeCall {
  const void *in;
  const int32_t *orient;
  uint8_t *out, *settled;
  int64_t B;
  int32_t N;
  template <int R, bool TRACKED>
  void launch(unsigned grid, hipStream_t s, int esh, uint32_t one) const {
    k_life<R, TRACKED><<<grid, kWave, 0, s>>>(in, orient, out, settled, esh, one, B, N);
  }
};

int32_t batch_life(bool tracked, const void *in, const int32_t *orient, void *out, uint8_t *settled, int32_t dtype, int64_t B,
                   int32_t N, void *hip_stream) {
  return plane_launch(LifeCall{in, orient, static_cast<uint8_t *>(out), settled, B, N}, tracked, in, out, out, 0, dtype, B, N,
                      hip_stream);
}

}  // namespace

extern "C" {

int32_t gg_life_planes(void) { return gg::kLifePlanes; }

int32_t gg_batch_life(const uint8_t *states, const int32_t *orient, void *out, uint8_t *settled, int32_t out_dtype, int64_t B,
                      int32_t N, void *hip_stream) {
  return batch_life(false, states, orient, out, settled, out_dtype, B, N, hip_stream);
}

int32_t gg_batch_life_tracked(const uint32_t *tracked, const int32_t *orient, void *out, uint8_t *settled, int32_t out_dtype,
                              int64_t B, int32_t N, void *hip_stream) {
  return batch_life(true, tracked, orient, out, settled, out_dtype, B, N, hip_stream);
}

}  // extern "C"
