// gg_ladder.hip - the ladder planes (gg_ladder.h: gg_batch_ladder, gg_batch_ladder_tracked) as a translation
// unit of their own, entry points included, compiled with the default code-generation switches: the machine code of every
// kernel of the other six units - and the hashes bench.py ties their PMC records to - does not depend on anything in here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gymgo_amd.h"
#include "gg_common.h"
#include "gg_v2.h"
#include "gg_lat.h"
#include "gg_feat.h"
#include "gg_ladder.h"

namespace {

using namespace gg;

// the launch goes to the device that owns the buffers, whatever the calling thread's current device is (restored on return)
struct OnOwner {
  int prev = -1, dev = 0;
  bool switched = false;
  explicit OnOwner(const void *p) {
    (void)hipGetDevice(&prev);
    dev = prev < 0 ? 0 : prev;
    hipPointerAttribute_t at;
    if (p && hipPointerGetAttributes(&at, p) == hipSuccess) dev = at.device;
    else (void)hipGetLastError();   // a pointer HIP does not know: launch on the current device (and fail there)
    if (dev != prev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~OnOwner() {
    if (switched) (void)hipSetDevice(prev);
  }
};

template <int R>
void launch_ladder_r(bool tracked, const void *in, const int32_t *orient, uint8_t *out, uint8_t *aborted, int esh, uint32_t one,
                     int64_t B, int32_t N, int cus, hipStream_t s) {
  // one single-wave workgroup per four (N <= 13) / two boards, at most 64 per compute unit (the rest: grid-stride)
  const int64_t groups = (B + Ladder<R>::NBW - 1) / Ladder<R>::NBW, cap = (int64_t)cus * 64;
  const unsigned grid = (unsigned)(groups < cap ? groups : cap);
  if (tracked) k_ladder<R, true><<<grid, kWave, 0, s>>>(in, orient, out, aborted, esh, one, B, N);
  else k_ladder<R, false><<<grid, kWave, 0, s>>>(in, orient, out, aborted, esh, one, B, N);
}

int32_t batch_ladder(bool tracked, const void *in, const int32_t *orient, void *out, uint8_t *aborted, int32_t dtype, int64_t B,
                     int32_t N, void *hip_stream) {
  if (N < 2 || N > GG_MAX_BOARD || B < 0 || dtype < GG_W_F32 || dtype > GG_FEAT_U8) return GG_E_BADSIZE;
  if (B == 0) return 0;
  if (!in || !out) return GG_E_NULLPTR;
  const int esh = dtype == GG_FEAT_U8 ? 0 : (dtype == GG_W_F32 ? 2 : 1);   // log2 of the element size
  if ((uintptr_t)out & (uintptr_t)((1 << esh) - 1)) return GG_E_BADARG;
  const uint32_t one = dtype == GG_FEAT_U8 ? 1u : dtype == GG_W_F16 ? 0x3C00u : dtype == GG_W_BF16 ? 0x3F80u : 0x3F800000u;
  OnOwner on_dev(in);
  int cus = gg_device_cus();   // (of the device made current above; GYMGO_AMD_CUS honoured)
  if (cus <= 0) cus = 256;
  hipStream_t s = (hipStream_t)hip_stream;
  uint8_t *o = static_cast<uint8_t *>(out);
  if (N <= 9) launch_ladder_r<9>(tracked, in, orient, o, aborted, esh, one, B, N, cus, s);
  else if (N <= 13) launch_ladder_r<13>(tracked, in, orient, o, aborted, esh, one, B, N, cus, s);
  else launch_ladder_r<19>(tracked, in, orient, o, aborted, esh, one, B, N, cus, s);
  return (int32_t)hipGetLastError();
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
