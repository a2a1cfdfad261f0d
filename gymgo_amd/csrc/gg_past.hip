// gg_past.hip - the history input planes (gg_past.h) with their entry points (gg_past_planes, gg_past_push,
// gg_past_push_tracked, gg_batch_past, gg_batch_past_tracked, gg_puct_past) as a translation unit of their own, compiled with
// the default code-generation switches: the machine code of every kernel of the other units - and the hashes bench.py ties
// their PMC records to - does not depend on anything in here.  The launch path is plane_launch of gg_planes.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gymgo_amd_past.h"
#include "gg_past.h"

namespace {

using namespace gg;

static_assert(kPastMaxT == GG_PAST_MAX_POSITIONS, "the header's constant");

struct PastPushCall {
  const void *in;
  const uint8_t *mask;
  uint32_t *rows;
  int32_t *count;
  int32_t H;
  int64_t B;
  int32_t N;
  template <int R, bool TRACKED>
  void launch(unsigned grid, hipStream_t s, int, uint32_t) const {
    k_past_push<R, TRACKED><<<grid, kWave, 0, s>>>(in, mask, rows, count, H, B, N);
  }
};

struct PastCall {
  const void *in;
  const uint32_t *rows;
  const int32_t *count;
  int32_t H, T, moves;
  const int32_t *orient;
  uint8_t *out;
  int64_t B;
  int32_t N;
  template <int R, bool TRACKED>
  void launch(unsigned grid, hipStream_t s, int esh, uint32_t one) const {
    k_past<R, TRACKED><<<grid, kWave, 0, s>>>(in, rows, count, H, T, moves, orient, out, esh, one, B, N);
  }
};

struct PuctPastCall {
  const uint32_t *leaf;
  const int32_t *leaf_id;
  const uint32_t *boards;
  const int32_t *links;
  const uint32_t *rows;
  const int32_t *count;
  int32_t H, T, moves;
  const int32_t *orient;
  uint8_t *out;
  int32_t C, L;
  int64_t B;
  int32_t N;
  template <int R, bool TRACKED>
  void launch(unsigned grid, hipStream_t s, int esh, uint32_t one) const {   // (tracked boards only)
    k_puct_past<R><<<grid, kWave, 0, s>>>(leaf, leaf_id, boards, links, rows, count, H, T, moves, orient, out, esh, one, C, L, B, N);
  }
};

bool sizes_ok(int32_t N, int64_t B) { return N >= 2 && N <= GG_MAX_BOARD && B >= 0; }
bool dtype_ok(int32_t dtype) { return dtype >= GG_W_F32 && dtype <= GG_FEAT_U8; }
bool shape_ok(int32_t T, int32_t moves, bool ring, int32_t H) {
  return T >= 1 && T <= GG_PAST_MAX_POSITIONS && (moves == 0 || moves == 1) && !(ring && H < 1);
}
bool aligned4(const void *a, const void *b = nullptr, const void *c = nullptr, const void *d = nullptr, const void *e = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 3u) == 0;
}

// the checks in the order of include/gymgo_amd_past.h, all before any device work
int32_t past_push(bool tracked, const void *in, const uint8_t *mask, uint32_t *rows, int32_t *count, int32_t H, int64_t B, int32_t N,
                  void *hip_stream) {
  if (!sizes_ok(N, B)) return GG_E_BADSIZE;
  if (H < 1) return GG_E_BADARG;
  if (B == 0) return 0;
  if (!in || !rows || !count) return GG_E_NULLPTR;
  if (!aligned4(rows, count, tracked ? in : nullptr)) return GG_E_BADARG;
  return plane_launch(PastPushCall{in, mask, rows, count, H, B, N}, tracked, in, rows, count, 3, GG_FEAT_U8, B, N, hip_stream);
}

int32_t batch_past(bool tracked, const void *in, const uint32_t *rows, const int32_t *count, int32_t H, int32_t T, int32_t moves,
                   const int32_t *orient, void *out, int32_t dtype, int64_t B, int32_t N, void *hip_stream) {
  if (!sizes_ok(N, B) || !dtype_ok(dtype)) return GG_E_BADSIZE;
  if (!shape_ok(T, moves, rows || count, H)) return GG_E_BADARG;
  if (B == 0) return 0;
  if (!in || !out || (rows == nullptr) != (count == nullptr)) return GG_E_NULLPTR;
  if (!aligned4(rows, count, orient, tracked ? in : nullptr)) return GG_E_BADARG;
  return plane_launch(PastCall{in, rows, count, H, T, moves, orient, static_cast<uint8_t *>(out), B, N}, tracked, in, out, out, 0, dtype,
                      B, N, hip_stream);
}

}  // namespace

extern "C" {

int32_t gg_past_planes(int32_t T, int32_t moves) {
  return shape_ok(T, moves, false, 0) ? gg::past_planes(T, moves) : -1;
}

int32_t gg_past_push(const uint8_t *states, const uint8_t *mask, uint32_t *rows, int32_t *count, int32_t H, int64_t B, int32_t N,
                     void *hip_stream) {
  return past_push(false, states, mask, rows, count, H, B, N, hip_stream);
}

int32_t gg_past_push_tracked(const uint32_t *tracked, const uint8_t *mask, uint32_t *rows, int32_t *count, int32_t H, int64_t B,
                             int32_t N, void *hip_stream) {
  return past_push(true, tracked, mask, rows, count, H, B, N, hip_stream);
}

int32_t gg_batch_past(const uint8_t *states, const uint32_t *rows, const int32_t *count, int32_t H, int32_t T, int32_t moves,
                      const int32_t *orient, void *out, int32_t out_dtype, int64_t B, int32_t N, void *hip_stream) {
  return batch_past(false, states, rows, count, H, T, moves, orient, out, out_dtype, B, N, hip_stream);
}

int32_t gg_batch_past_tracked(const uint32_t *tracked, const uint32_t *rows, const int32_t *count, int32_t H, int32_t T,
                              int32_t moves, const int32_t *orient, void *out, int32_t out_dtype, int64_t B, int32_t N,
                              void *hip_stream) {
  return batch_past(true, tracked, rows, count, H, T, moves, orient, out, out_dtype, B, N, hip_stream);
}

int32_t gg_puct_past(int64_t R, int32_t N, int32_t C, int32_t L, const uint32_t *boards, const int32_t *links, const uint32_t *rows,
                     const int32_t *count, int32_t H, int32_t T, int32_t moves, const uint32_t *leaf, const int32_t *leaf_id,
                     const int32_t *orient, void *out, int32_t out_dtype, void *hip_stream) {
  if (!sizes_ok(N, R) || !dtype_ok(out_dtype)) return GG_E_BADSIZE;
  if (C < 1 || C == INT32_MAX || L < 1 || L > C || !shape_ok(T, moves, rows || count, H)) return GG_E_BADARG;
  if (R == 0) return 0;
  if (!boards || !links || !leaf || !leaf_id || !out || (rows == nullptr) != (count == nullptr)) return GG_E_NULLPTR;
  if (!aligned4(boards, links, rows, count, leaf) || !aligned4(leaf_id, orient)) return GG_E_BADARG;
  const int64_t B = R * (int64_t)L;
  return plane_launch(PuctPastCall{leaf, leaf_id, boards, links, rows, count, H, T, moves, orient, static_cast<uint8_t *>(out), C, L, B,
                                   N},
                      true, leaf, out, out, 0, out_dtype, B, N, hip_stream);
}

}  // extern "C"
