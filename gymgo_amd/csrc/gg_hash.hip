// gg_hash.hip - the position and move hashes (gg_hash.h) with their entry points (gg_batch_hash, gg_batch_hash_tracked,
// gg_batch_move_hashes, gg_batch_move_hashes_tracked, gg_puct_superko) as a translation unit of their own, compiled with the default
// code-generation switches: the machine code of every kernel of the other units - and the hashes bench.py ties their PMC
// records to - does not depend on anything in here.  The launch path is plane_launch of gg_planes.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gymgo_amd.h"
#include "gg_hash.h"

namespace {

using namespace gg;

struct HashCall {
  const void *in;
  int64_t *out;
  int64_t B;
  int32_t N;
  template <int R, bool TRACKED>
  void launch(unsigned grid, hipStream_t s, int, uint32_t) const {
    k_hash<R, TRACKED><<<grid, kWave, 0, s>>>(in, out, B, N);
  }
};

struct MoveHashCall {
  const void *in;
  const int64_t *history;
  const int32_t *count;
  int32_t H;
  int64_t *hashes;
  uint8_t *repeat;
  uint32_t *rows;
  int64_t B;
  int32_t N;
  template <int R, bool TRACKED>
  void launch(unsigned grid, hipStream_t s, int, uint32_t) const {
    k_move_hashes<R, TRACKED><<<grid, kWave, 0, s>>>(in, history, count, H, hashes, repeat, rows, B, N);
  }
};

struct SuperkoCall {
  uint32_t *leaf;
  const int32_t *move, *leaf_id, *links;
  int64_t *node_hash;
  const int64_t *history;
  const int32_t *count;
  int32_t H, C, L;
  int64_t B;
  int32_t N;
  template <int R, bool TRACKED>
  void launch(unsigned grid, hipStream_t s, int, uint32_t) const {   // (tracked boards only)
    k_puct_superko<R><<<grid, kWave, 0, s>>>(leaf, move, leaf_id, links, node_hash, history, count, H, C, L, B, N);
  }
};

int32_t batch_hash(bool tracked, const void *in, int64_t *out, int64_t B, int32_t N, void *hip_stream) {
  return plane_launch(HashCall{in, out, B, N}, tracked, in, out, out, 7, GG_FEAT_U8, B, N, hip_stream);
}

// the checks in the order of include/gymgo_amd.h, all before any device work
int32_t batch_move_hashes(bool tracked, const void *in, const int64_t *history, const int32_t *count, int32_t H, int64_t *hashes,
                          uint8_t *repeat, uint32_t *rows, int64_t B, int32_t N, void *hip_stream) {
  if (N < 2 || N > GG_MAX_BOARD || B < 0) return GG_E_BADSIZE;
  if (H < 0) return GG_E_BADARG;
  if (B == 0) return 0;
  if (!in || (!hashes && !repeat && !rows)) return GG_E_NULLPTR;
  const bool masks = repeat || rows;
  if (masks && (!history || !count)) return GG_E_NULLPTR;
  if (((uintptr_t)hashes & 7u) || ((uintptr_t)rows & 3u)) return GG_E_BADARG;
  if (masks && (((uintptr_t)history & 7u) || ((uintptr_t)count & 3u))) return GG_E_BADARG;
  const void *out = hashes ? (const void *)hashes : repeat ? (const void *)repeat : (const void *)rows;
  return plane_launch(MoveHashCall{in, history, count, H, hashes, repeat, rows, B, N}, tracked, in, out, out, hashes ? 7 : 0,
                      GG_FEAT_U8, B, N, hip_stream);
}

}  // namespace

extern "C" {

static_assert(gg::kHashSeed == GG_HASH_SEED, "the header's constant");

int32_t gg_batch_hash(const uint8_t *states, int64_t *out, int64_t B, int32_t N, void *hip_stream) {
  return batch_hash(false, states, out, B, N, hip_stream);
}

int32_t gg_batch_hash_tracked(const uint32_t *tracked, int64_t *out, int64_t B, int32_t N, void *hip_stream) {
  return batch_hash(true, tracked, out, B, N, hip_stream);
}

int32_t gg_batch_move_hashes(const uint8_t *states, const int64_t *history, const int32_t *count, int32_t H, int64_t *hashes,
                             uint8_t *repeat, uint32_t *rows, int64_t B, int32_t N, void *hip_stream) {
  return batch_move_hashes(false, states, history, count, H, hashes, repeat, rows, B, N, hip_stream);
}

int32_t gg_batch_move_hashes_tracked(const uint32_t *tracked, const int64_t *history, const int32_t *count, int32_t H,
                                     int64_t *hashes, uint8_t *repeat, uint32_t *rows, int64_t B, int32_t N, void *hip_stream) {
  return batch_move_hashes(true, tracked, history, count, H, hashes, repeat, rows, B, N, hip_stream);
}

// the checks in the order of include/gymgo_amd.h, all before any device work
int32_t gg_puct_superko(int64_t R, int32_t N, int32_t C, int32_t L, const int32_t *links, int64_t *node_hash, const int64_t *history,
                        const int32_t *count, int32_t H, uint32_t *leaf, const int32_t *move, const int32_t *leaf_id,
                        void *hip_stream) {
  if (N < 2 || N > GG_MAX_BOARD || R < 0) return GG_E_BADSIZE;
  if (C < 1 || C == INT32_MAX || L < 1 || L > C || H < 0) return GG_E_BADARG;
  if (R == 0) return 0;
  if (!links || !node_hash || !leaf || !move || !leaf_id || (history == nullptr) != (count == nullptr)) return GG_E_NULLPTR;
  if (((uintptr_t)node_hash & 7u) || ((uintptr_t)history & 7u)) return GG_E_BADARG;
  if ((((uintptr_t)links | (uintptr_t)count | (uintptr_t)leaf | (uintptr_t)move | (uintptr_t)leaf_id) & 3u)) return GG_E_BADARG;
  const int64_t B = R * (int64_t)L;
  return plane_launch(SuperkoCall{leaf, move, leaf_id, links, node_hash, history, count, H, C, L, B, N}, true, leaf, leaf, leaf, 3,
                      GG_FEAT_U8, B, N, hip_stream);
}

}  // extern "C"
