// gg_feat.hip - the feature-plane kernels (gg_feat.h) with their entry points (gg_feature_planes, gg_batch_group_liberties,
// gg_batch_features, gg_batch_features_tracked and their oriented forms) as a translation unit of their own, compiled with
// the default code-generation switches: the machine code of every kernel of the other units - and the hashes bench.py ties
// their PMC records to - does not depend on anything in here.  The launch path is plane_launch of gg_planes.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gymgo_amd.h"
#include "gg_feat.h"

namespace {

using namespace gg;

// k_features / k_features_oriented (orient given) with the element size as a template argument
struct FeatureCall {
  const void *in;
  const int32_t *orient;
  uint8_t *out;
  int64_t B;
  int32_t N;
  template <int R, int ES, bool TRACKED>
  void launch_e(unsigned grid, hipStream_t s, uint32_t one) const {
    if (orient) k_features_oriented<R, ES, TRACKED><<<grid, kWave, 0, s>>>(in, orient, out, one, B, N);
    else k_features<R, ES, TRACKED><<<grid, kWave, 0, s>>>(in, out, one, B, N);
  }
  template <int R, bool TRACKED>
  void launch(unsigned grid, hipStream_t s, int esh, uint32_t one) const {
    if (esh == 0) launch_e<R, 1, TRACKED>(grid, s, one);
    else if (esh == 1) launch_e<R, 2, TRACKED>(grid, s, one);
    else launch_e<R, 4, TRACKED>(grid, s, one);
  }
};

// out: 16-byte aligned; oriented: orient must be given
int32_t batch_features(bool tracked, const void *in, const int32_t *orient, bool oriented, void *out, int32_t dtype, int64_t B,
                       int32_t N, void *hip_stream) {
  return plane_launch(FeatureCall{in, orient, static_cast<uint8_t *>(out), B, N}, tracked, in, out, oriented ? orient : out, 15, dtype,
                      B, N, hip_stream);
}

struct LibertiesCall {
  const uint8_t *states;
  uint8_t *libs;
  int64_t B;
  int32_t N;
  template <int R, bool TRACKED>
  void launch(unsigned grid, hipStream_t s, int, uint32_t) const {
    k_group_liberties<R><<<grid, kWave, 0, s>>>(states, libs, B, N);
  }
};

}  // namespace

extern "C" {

int32_t gg_feature_planes(void) { return gg::kFeatPlanes; }

int32_t gg_batch_group_liberties(const uint8_t *states, uint8_t *libs, int64_t B, int32_t N, void *hip_stream) {
  return plane_launch(LibertiesCall{states, libs, B, N}, false, states, libs, libs, 0, GG_FEAT_U8, B, N, hip_stream);
}

int32_t gg_batch_features(const uint8_t *states, void *out, int32_t out_dtype, int64_t B, int32_t N, void *hip_stream) {
  return batch_features(false, states, nullptr, false, out, out_dtype, B, N, hip_stream);
}

int32_t gg_batch_features_tracked(const uint32_t *tracked, void *out, int32_t out_dtype, int64_t B, int32_t N, void *hip_stream) {
  return batch_features(true, tracked, nullptr, false, out, out_dtype, B, N, hip_stream);
}

int32_t gg_batch_features_oriented(const uint8_t *states, const int32_t *orient, void *out, int32_t out_dtype, int64_t B, int32_t N,
                                   void *hip_stream) {
  return batch_features(false, states, orient, true, out, out_dtype, B, N, hip_stream);
}

int32_t gg_batch_features_tracked_oriented(const uint32_t *tracked, const int32_t *orient, void *out, int32_t out_dtype, int64_t B,
                                           int32_t N, void *hip_stream) {
  return batch_features(true, tracked, orient, true, out, out_dtype, B, N, hip_stream);
}

}  // extern "C"
