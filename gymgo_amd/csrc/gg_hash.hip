// gg_hash.hip - the position and move hashes (gg_hash.h) with their entry points (gg_batch_hash, gg_batch_hash_tracked,
// gg_batch_move_hashes, gg_batch_move_hashes_tracked) as a translation unit of their own, compiled with the default
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

}  // extern "C"
