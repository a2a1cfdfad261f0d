// gg_feat.hip - the launches of the feature-plane kernels (gg_feat.h: gg_batch_features, gg_batch_features_tracked, their
// oriented forms, gg_batch_group_liberties) as a translation unit of their own, compiled with the default code-generation switches: the
// machine code of every kernel of the other four units - and the hashes bench.py ties their PMC records to - does not
// depend on anything in here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gg_common.h"
#include "gg_v2.h"
#include "gg_lat.h"
#include "gg_feat.h"

namespace gg {

namespace {
// one single-wave workgroup per four (N <= 13) / two boards, at most 64 per compute unit (the rest: grid-stride)
unsigned feat_grid(int cus, int64_t B, int nbw) {
  const int64_t groups = (B + nbw - 1) / nbw, cap = (int64_t)cus * 64;
  return (unsigned)(groups < cap ? groups : cap);
}
}  // namespace

// dtype: GG_W_F32 / GG_W_BF16 / GG_W_F16 / GG_FEAT_U8 (checked by the caller); `in`: byte planes, or tracked boards
#define GG_FEAT_E(R, ES, ONE)                                                                                          \
  do {                                                                                                                 \
    const unsigned grid_ = feat_grid(cus, B, Feat<R>::NBW);                                                            \
    if (tracked) k_features<R, ES, true><<<grid_, kWave, 0, s>>>(in, static_cast<uint8_t *>(out), ONE, B, N);          \
    else k_features<R, ES, false><<<grid_, kWave, 0, s>>>(in, static_cast<uint8_t *>(out), ONE, B, N);                 \
  } while (0)
#define GG_FEAT(R)                                                \
  do {                                                            \
    if (dtype == GG_FEAT_U8) GG_FEAT_E(R, 1, 1u);                 \
    else if (dtype == GG_W_F16) GG_FEAT_E(R, 2, 0x3C00u);         \
    else if (dtype == GG_W_BF16) GG_FEAT_E(R, 2, 0x3F80u);        \
    else GG_FEAT_E(R, 4, 0x3F800000u);                            \
  } while (0)
void launch_features(bool tracked, const void *in, void *out, int dtype, int64_t B, int32_t N, int cus, hipStream_t s) {
  if (N <= 9) GG_FEAT(9);
  else if (N <= 13) GG_FEAT(13);
  else GG_FEAT(19);
}
#undef GG_FEAT
#undef GG_FEAT_E

// ... and view orient[b] of them (k_features_oriented: the same grid, the boards turned in registers after the load)
#define GG_FEAT_E(R, ES, ONE)                                                                                                        \
  do {                                                                                                                               \
    const unsigned grid_ = feat_grid(cus, B, Feat<R>::NBW);                                                                          \
    if (tracked) k_features_oriented<R, ES, true><<<grid_, kWave, 0, s>>>(in, orient, static_cast<uint8_t *>(out), ONE, B, N);       \
    else k_features_oriented<R, ES, false><<<grid_, kWave, 0, s>>>(in, orient, static_cast<uint8_t *>(out), ONE, B, N);              \
  } while (0)
#define GG_FEAT(R)                                                \
  do {                                                            \
    if (dtype == GG_FEAT_U8) GG_FEAT_E(R, 1, 1u);                 \
    else if (dtype == GG_W_F16) GG_FEAT_E(R, 2, 0x3C00u);         \
    else if (dtype == GG_W_BF16) GG_FEAT_E(R, 2, 0x3F80u);        \
    else GG_FEAT_E(R, 4, 0x3F800000u);                            \
  } while (0)
void launch_features_oriented(bool tracked, const void *in, const int32_t *orient, void *out, int dtype, int64_t B, int32_t N, int cus,
                              hipStream_t s) {
  if (N <= 9) GG_FEAT(9);
  else if (N <= 13) GG_FEAT(13);
  else GG_FEAT(19);
}
#undef GG_FEAT
#undef GG_FEAT_E

void launch_group_liberties(const uint8_t *states, uint8_t *libs, int64_t B, int32_t N, int cus, hipStream_t s) {
  if (N <= 9) k_group_liberties<9><<<feat_grid(cus, B, Feat<9>::NBW), kWave, 0, s>>>(states, libs, B, N);
  else if (N <= 13) k_group_liberties<13><<<feat_grid(cus, B, Feat<13>::NBW), kWave, 0, s>>>(states, libs, B, N);
  else k_group_liberties<19><<<feat_grid(cus, B, Feat<19>::NBW), kWave, 0, s>>>(states, libs, B, N);
}

}  // namespace gg
