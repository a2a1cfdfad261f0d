// gg_status.hip - stone status and the final score from playout ownership (gg_status.h) with their entry points
// (gg_status_planes, gg_batch_status, gg_batch_status_tracked) as a translation unit of their own, compiled with the default
// code-generation switches: the machine code of every kernel of the other units - and the hashes bench.py ties their PMC
// records to - does not depend on anything in here.  The launch path is plane_launch of gg_planes.h, with own as its `also`.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gymgo_amd_status.h"
#include "gg_status.h"

namespace {

using namespace gg;

struct StatusCall {
  const void *in;
  const int32_t *orient;
  const uint8_t *side;
  const uint32_t *own;
  uint32_t numK, den;
  uint8_t *out;
  int32_t *counts;
  int64_t B;
  int32_t N;
  template <int R, bool TRACKED>
  void launch(unsigned grid, hipStream_t s, int esh, uint32_t one) const {
    k_status<R, TRACKED><<<grid, kWave, 0, s>>>(in, orient, side, own, numK, den, out, counts, esh, one, B, N);
  }
};

// the checks in the order of include/gymgo_amd_status.h: the sizes, the scalars, B == 0, the 4-byte alignments, then
// plane_launch's (whose size checks have passed by then): the NULL pointers and the alignment of out
int32_t batch_status(bool tracked, const void *in, const int32_t *orient, const uint8_t *side, const int32_t *own, int32_t playouts,
                     int32_t num, int32_t den, void *out, int32_t *counts, int32_t dtype, int64_t B, int32_t N, void *hip_stream) {
  if (N < 2 || N > GG_MAX_BOARD || B < 0 || dtype < GG_W_F32 || dtype > GG_FEAT_U8) return GG_E_BADSIZE;
  if (playouts < 1 || playouts > GG_STATUS_MAX_PLAYOUTS || num < 1 || num > den || den > GG_STATUS_MAX_DEN || 2 * num <= den)
    return GG_E_BADARG;
  if (B == 0) return 0;
  if (((uintptr_t)own | (uintptr_t)counts) & 3u) return GG_E_BADARG;
  const StatusCall call{in, orient, side, reinterpret_cast<const uint32_t *>(own), (uint32_t)num * (uint32_t)playouts, (uint32_t)den,
                        static_cast<uint8_t *>(out), counts, B, N};   // (num K <= 2^30)
  return plane_launch(call, tracked, in, out, own, 0, dtype, B, N, hip_stream);
}

}  // namespace

extern "C" {

int32_t gg_status_planes(void) { return gg::kStatusPlanes; }

int32_t gg_batch_status(const uint8_t *states, const int32_t *orient, const uint8_t *side, const int32_t *own, int32_t playouts,
                        int32_t num, int32_t den, void *out, int32_t *counts, int32_t out_dtype, int64_t B, int32_t N,
                        void *hip_stream) {
  return batch_status(false, states, orient, side, own, playouts, num, den, out, counts, out_dtype, B, N, hip_stream);
}

int32_t gg_batch_status_tracked(const uint32_t *tracked, const int32_t *orient, const uint8_t *side, const int32_t *own,
                                int32_t playouts, int32_t num, int32_t den, void *out, int32_t *counts, int32_t out_dtype, int64_t B,
                                int32_t N, void *hip_stream) {
  return batch_status(true, tracked, orient, side, own, playouts, num, den, out, counts, out_dtype, B, N, hip_stream);
}

}  // extern "C"
