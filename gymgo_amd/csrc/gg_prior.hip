// gg_prior.hip - the move priors (gg_prior.h) with their entry points (gg_batch_move_priors, gg_batch_move_priors_tracked,
// gg_uct_prior_begin, gg_uct_prior_expand, gg_uct_prior_expand_leaves) as a translation unit of their own, compiled with the
// default code-generation switches: the machine code of every kernel of the other units - and the hashes bench.py ties their PMC records to - does not
// depend on anything in here.  A plane unit on gg_planes.h (frame and load); the pairs leave through prior_store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gymgo_amd_prior.h"
#include "gymgo_amd_uct_leaves.h"
#include "gg_prior.h"

namespace {

using namespace gg;

// One launch of k_move_priors on the device that owns `in`: one single-wave workgroup per four (N <= 13) / two boards, at most
// 64 per compute unit (the rest: grid-stride) - plane_launch_r's grid.  VL: the B = R L boards of a round, tree b / L.
template <bool TREE, bool VL = false>
int32_t prior_launch(bool tracked, const void *in, const int32_t *last, const int32_t *weights, int32_t *out, const int32_t *node,
                     int need_move, int32_t I, int64_t B, int32_t N, void *hip_stream, int32_t L = 1) {
  OnDeviceOf on_dev(in);
  const int64_t cap = (int64_t)on_dev.cus() * 64;
  hipStream_t s = (hipStream_t)hip_stream;
  uint32_t *o = reinterpret_cast<uint32_t *>(out);
  by_rows(N, [&](auto t) {
    constexpr int R = decltype(t)::R;
    const int64_t groups = (B + Planes<R>::NBW - 1) / Planes<R>::NBW;
    const unsigned grid = (unsigned)(groups < cap ? groups : cap);
    if (tracked) k_move_priors<R, true, TREE, VL><<<grid, kWave, 0, s>>>(in, last, weights, o, node, need_move, I, B, N, L);
    else if constexpr (!TREE) k_move_priors<R, false, false><<<grid, kWave, 0, s>>>(in, last, weights, o, node, need_move, I, B, N, L);
  });
  return (int32_t)hipGetLastError();
}

int32_t batch_move_priors(bool tracked, const void *in, const int32_t *last, const int32_t *weights, int32_t *out, int64_t B,
                          int32_t N, void *hip_stream) {
  if (N < 2 || N > GG_MAX_BOARD || B < 0) return GG_E_BADSIZE;
  if (B == 0) return 0;
  if (!in || !weights || !out) return GG_E_NULLPTR;
  if ((uintptr_t)out & 3u) return GG_E_BADARG;
  return prior_launch<false>(tracked, in, last, weights, out, nullptr, 0, 0, B, N, hip_stream);
}

// the sizes of a tree, as the RAVE calls check them (no playout count here: I + 1 nodes must be an int32); L slots a root: the
// R L rows are an int64
int32_t tree_sizes(int64_t R, int32_t N, int32_t I, int32_t L = 1) {
  if (N < 2 || N > GG_MAX_BOARD || R < 0) return GG_E_BADSIZE;
  if (I < 1 || I == 0x7FFFFFFF || L < 1) return GG_E_BADARG;
  if (R > INT64_MAX / L) return GG_E_BADSIZE;
  return 0;
}

}  // namespace

extern "C" {

int32_t gg_batch_move_priors(const uint8_t *states, const int32_t *last, const int32_t *weights, int32_t *out, int64_t B, int32_t N,
                             void *hip_stream) {
  return batch_move_priors(false, states, last, weights, out, B, N, hip_stream);
}

int32_t gg_batch_move_priors_tracked(const uint32_t *tracked, const int32_t *last, const int32_t *weights, int32_t *out, int64_t B,
                                     int32_t N, void *hip_stream) {
  return batch_move_priors(true, tracked, last, weights, out, B, N, hip_stream);
}

int32_t gg_uct_prior_begin(const uint32_t *roots, const int32_t *last_actions, int64_t R, int32_t N, int32_t I, const int32_t *weights,
                           int32_t *node_amaf, void *hip_stream) {
  if (int32_t e = tree_sizes(R, N, I)) return e;
  if (!roots || !weights || !node_amaf) return GG_E_NULLPTR;
  if (R == 0) return 0;
  if ((uintptr_t)node_amaf & 3u) return GG_E_BADARG;
  return prior_launch<true>(true, roots, last_actions, weights, node_amaf, nullptr, 0, I, R, N, hip_stream);
}

int32_t gg_uct_prior_expand(int64_t R, int32_t N, int32_t I, const int32_t *weights, const uint32_t *leaf, const int32_t *move,
                            const int32_t *leaf_id, int32_t *node_amaf, void *hip_stream) {
  if (int32_t e = tree_sizes(R, N, I)) return e;
  if (!weights || !leaf || !move || !leaf_id || !node_amaf) return GG_E_NULLPTR;
  if (R == 0) return 0;
  if ((uintptr_t)node_amaf & 3u) return GG_E_BADARG;
  return prior_launch<true>(true, leaf, move, weights, node_amaf, leaf_id, 1, I, R, N, hip_stream);
}

int32_t gg_uct_prior_expand_leaves(int64_t R, int32_t N, int32_t I, int32_t L, const int32_t *weights, const uint32_t *leaf,
                                   const int32_t *move, const int32_t *leaf_id, int32_t *node_amaf, void *hip_stream) {
  if (int32_t e = tree_sizes(R, N, I, L)) return e;
  if (!weights || !leaf || !move || !leaf_id || !node_amaf) return GG_E_NULLPTR;
  if (R == 0) return 0;
  if ((uintptr_t)node_amaf & 3u) return GG_E_BADARG;
  return prior_launch<true, true>(true, leaf, move, weights, node_amaf, leaf_id, 1, I, R * L, N, hip_stream, L);
}

}  // extern "C"
