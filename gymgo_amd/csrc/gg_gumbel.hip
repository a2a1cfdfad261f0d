// gg_gumbel.hip - the Gumbel root rule of the PUCT search (gg_gumbel.h) with its entry points (gg_gumbel_sequence,
// gg_gumbel_begin, gg_gumbel_select_leaves, gg_gumbel_root) as a translation unit of its own, compiled with the default
// code-generation switches: the machine code of every kernel of the other units - and the hashes bench.py ties their PMC
// records to - does not depend on anything in here.  The select kernel is the one walk of gg_puct.h, k_puct_select,
// instantiated with the root rule (k_puct_select<true, GumbelRoot>); this unit holds that instantiation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gymgo_amd_gumbel.h"
#include "gg_gumbel.h"
#include "gg_host.h"

namespace {

using namespace gg;

static_assert(sizeof(gg_puct_stat) == sizeof(PuctStat) && sizeof(PuctStat) == 16, "one 16-byte record per node");
static_assert(GG_MAX_BOARD * GG_MAX_BOARD + 1 <= kPuctStrides * kWave, "a lane holds every action of its strides");

bool finite_nonneg(double x) { return x >= 0.0 && x <= __DBL_MAX__; }

// the tree-search launch of gg_kernels.hip: four roots per four-wave workgroup, at most 32 workgroups per compute unit (the
// rest: grid-stride), on the device that owns `p`
template <typename... KArgs, typename... Args>
int32_t launch_roots(void (*kern)(KArgs...), const void *p, int64_t R, void *hip_stream, Args... args) {
  OnDeviceOf on_dev(p);
  const int64_t groups = (R + 3) / 4, cap = (int64_t)on_dev.cus() * 32;
  kern<<<(unsigned)(groups < cap ? groups : cap), 4 * kWave, 0, (hipStream_t)hip_stream>>>(args...);
  return (int32_t)hipGetLastError();
}

// sizes, then the tree's capacity (the conditions of gg_puct_select_leaves on C): the first two checks of every entry point
int32_t tree_ok(int64_t R, int32_t N, int32_t C) {
  if (N < 2 || N > GG_MAX_BOARD || R < 0) return GG_E_BADSIZE;
  if (C < 1 || C == 0x7FFFFFFF) return GG_E_BADARG;
  return 0;
}

PuctArgs tree_args(int64_t R, int32_t N, int32_t C, int32_t L, double c, const uint32_t *boards, const int32_t *child, const float *prior,
                   const int32_t *links, const gg_puct_stat *stats, const int32_t *nodes, uint32_t *leaf, int32_t *move,
                   int32_t *leaf_id) {
  return PuctArgs{const_cast<uint32_t *>(boards), const_cast<int32_t *>(child), const_cast<float *>(prior),
                  const_cast<int32_t *>(links), reinterpret_cast<PuctStat *>(const_cast<gg_puct_stat *>(stats)),
                  const_cast<int32_t *>(nodes), leaf, move, leaf_id, nullptr, nullptr, c, R, N, C, 0.f, L};
}

}  // namespace

extern "C" {

int32_t gg_gumbel_sequence(int32_t m, int32_t n, int32_t *seq) {
  if (m < 1 || n < 1) return GG_E_BADARG;
  if (!seq) return GG_E_NULLPTR;
  if (m == 1) {
    for (int32_t t = 0; t < n; ++t) seq[t] = t;
    return 0;
  }
  int32_t lg = 0;
  while (((int64_t)1 << lg) < m) ++lg;
  // v[i] for i < k is the number of passes so far (k never grows, so an action still considered was in every pass): one counter
  int64_t k = m, count = 0;
  int32_t pass = 0;
  while (count < n) {
    const int64_t q = (int64_t)n / ((int64_t)lg * k), e = q > 1 ? q : 1;
    for (int64_t i = 0; i < e && count < n; ++i, ++pass)
      for (int64_t j = 0; j < k && count < n; ++j) seq[count++] = pass;
    k = k / 2 > 2 ? k / 2 : 2;
  }
  return 0;
}

int32_t gg_gumbel_begin(int64_t R, int32_t N, int32_t C, const int32_t *child, const gg_puct_stat *stats, const int32_t *nodes,
                        int32_t *seen, int32_t *done, void *hip_stream) {
  if (int32_t e = tree_ok(R, N, C)) return e;
  if (R == 0) return 0;
  if (!child || !stats || !nodes || !seen || !done) return GG_E_NULLPTR;
  if ((uintptr_t)stats & 15u) return GG_E_BADARG;
  const PuctArgs u = tree_args(R, N, C, 1, 0.0, nullptr, child, nullptr, nullptr, stats, nodes, nullptr, nullptr, nullptr);
  return launch_roots(k_gumbel_begin, child, R, hip_stream, u, seen, done);
}

int32_t gg_gumbel_select_leaves(int64_t R, int32_t N, int32_t C, int32_t L, double c, const uint32_t *boards, int32_t *child,
                                const float *prior, int32_t *links, gg_puct_stat *stats, int32_t *nodes, const float *base,
                                const int32_t *seen, int32_t *done, const int32_t *seq, int32_t S, double c_visit, double c_scale,
                                uint32_t *leaf, int32_t *move, int32_t *leaf_id, void *hip_stream) {
  if (int32_t e = tree_ok(R, N, C)) return e;
  if (!finite_nonneg(c) || L < 1 || L > C || S < 1 || !finite_nonneg(c_visit) || !finite_nonneg(c_scale)) return GG_E_BADARG;
  if (R == 0) return 0;
  if (!boards || !child || !prior || !links || !stats || !nodes || !base || !seen || !done || !seq || !leaf || !move || !leaf_id)
    return GG_E_NULLPTR;
  if ((uintptr_t)stats & 15u) return GG_E_BADARG;
  GumbelSelectArgs u;
  static_cast<PuctArgs &>(u) = tree_args(R, N, C, L, c, boards, child, prior, links, stats, nodes, leaf, move, leaf_id);
  u.b = GumbelArgs{base, seen, done, seq, S, c_visit, c_scale, nullptr, nullptr, nullptr, nullptr};
  return launch_roots(k_puct_select<true, GumbelRoot>, leaf, R, hip_stream, u);
}

int32_t gg_gumbel_root(int64_t R, int32_t N, int32_t C, const uint32_t *boards, const int32_t *child, const gg_puct_stat *stats,
                       const int32_t *nodes, const float *base, const int32_t *seen, double c_visit, double c_scale,
                       int32_t *actions, float *q, int32_t *visits, float *value, void *hip_stream) {
  if (int32_t e = tree_ok(R, N, C)) return e;
  if (!finite_nonneg(c_visit) || !finite_nonneg(c_scale)) return GG_E_BADARG;
  if (R == 0) return 0;
  if (!boards || !child || !stats || !nodes || !base || !seen || !actions) return GG_E_NULLPTR;
  if ((uintptr_t)stats & 15u) return GG_E_BADARG;
  const PuctArgs u = tree_args(R, N, C, 1, 0.0, boards, child, nullptr, nullptr, stats, nodes, nullptr, nullptr, nullptr);
  const GumbelArgs b{base, seen, nullptr, nullptr, 0, c_visit, c_scale, actions, q, visits, value};   // (q, visits, value may be NULL)
  return launch_roots(k_gumbel_root, boards, R, hip_stream, u, b);
}

}  // extern "C"
