// gg_uct_leaves.hip - the UCT search with several leaves per root and round (gg_uct_leaves.h) with its entry points
// (gg_uct_select_leaves[_rave], gg_uct_backup_leaves[_rave], gg_uct_prior_expand_leaves) as a translation unit of its own, compiled
// with the default code-generation switches: the machine code of every kernel of the other units - and the hashes bench.py ties
// their PMC records to - does not depend on anything in here.  The kernels are the bodies of gg_uct.h and gg_prior.h instantiated
// with their slot loops; this unit holds those instantiations.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gymgo_amd_uct_leaves.h"
#include "gg_uct_leaves.h"
#include "gg_host.h"

namespace {

using namespace gg;

// the tree-search launch of gg_kernels.hip: four roots per four-wave workgroup, at most 32 workgroups per compute unit (the
// rest: grid-stride), on the device that owns `p`
template <typename... KArgs, typename... Args>
int32_t launch_roots(void (*kern)(KArgs...), const void *p, int64_t R, void *hip_stream, Args... args) {
  OnDeviceOf on_dev(p);
  const int64_t groups = (R + 3) / 4, cap = (int64_t)on_dev.cus() * 32;
  kern<<<(unsigned)(groups < cap ? groups : cap), 4 * kWave, 0, (hipStream_t)hip_stream>>>(args...);
  return (int32_t)hipGetLastError();
}

bool rows_ok(int64_t R, int32_t L) { return R <= INT64_MAX / L; }   // R L rows: an int64

// gg_uct_select's / gg_uct_backup's checks in their order with the capacity C where I stood, L beside the other arguments and the
// rows beside the other sizes; RAVE: what gg_uct_select_rave / gg_uct_backup_rave add (rave = false: k and fpu are not looked at)
int32_t leaves_args(UctArgs &u, bool rave, int64_t R, int32_t N, int32_t C, int32_t L, int32_t K, double c, double rave_equiv,
                    double fpu) {
  if (N < 2 || N > GG_MAX_BOARD || R < 0) return GG_E_BADSIZE;
  if (C < 1 || K < 1 || !(c >= 0.0 && c <= __DBL_MAX__) || L < 1) return GG_E_BADARG;
  if ((int64_t)C * K > 0x7FFFFFFF || !rows_ok(R, L)) return GG_E_BADSIZE;   // the root's n = C K is an int32
  if (rave) {
    if (2 * (int64_t)C * K > 0x7FFFFFFF) return GG_E_BADSIZE;   // s~ <= 2 C K is an int32
    if (!(rave_equiv > 0.0 && rave_equiv <= __DBL_MAX__) || !(fpu >= -__DBL_MAX__ && fpu <= __DBL_MAX__)) return GG_E_BADARG;
  }
  u = UctArgs{};
  u.c = c; u.R = R; u.N = N; u.I = C; u.K = K; u.k = rave_equiv; u.fpu = fpu;
  return 0;
}

template <bool RAVE>
int32_t select_leaves(int64_t R, int32_t N, int32_t C, int32_t L, int32_t K, double c, double rave_equiv, double fpu,
                      const double *log_table, const uint32_t *boards, int32_t *child, int32_t *links, int32_t *stats,
                      const int32_t *node_amaf, int32_t *nodes, int32_t *virt, uint32_t *leaf, int32_t *move, int32_t *leaf_id,
                      void *hip_stream) {
  UctArgs u;
  if (int32_t e = leaves_args(u, RAVE, R, N, C, L, K, c, rave_equiv, fpu)) return e;
  if (!log_table || !boards || !child || !links || !stats || (RAVE && !node_amaf) || !nodes || !virt || !leaf || !move || !leaf_id)
    return GG_E_NULLPTR;
  if (R == 0) return 0;
  u.boards = const_cast<uint32_t *>(boards); u.child = child; u.links = links; u.stats = stats; u.nodes = nodes;
  u.leaf = leaf; u.move = move; u.leaf_id = leaf_id; u.log_table = log_table; u.node_amaf = const_cast<int32_t *>(node_amaf);
  return launch_roots(k_uct_select_leaves<RAVE>, leaf, R, hip_stream, u, virt, L);
}

template <bool RAVE>
int32_t backup_leaves(int64_t R, int32_t N, int32_t C, int32_t L, int32_t K, const int32_t *counts, const int64_t *sums,
                      const int32_t *amaf, int64_t *totals, uint32_t *boards, const int32_t *links, int32_t *stats,
                      int32_t *node_amaf, int32_t *virt, const uint32_t *leaf, const int32_t *move, const int32_t *leaf_id,
                      void *hip_stream) {
  UctArgs u;
  if (int32_t e = leaves_args(u, RAVE, R, N, C, L, K, 0.0, 1.0, 0.0)) return e;
  if (!counts || !sums || (RAVE && (!amaf || !node_amaf)) || !boards || !links || !stats || !virt || !leaf || !move || !leaf_id)
    return GG_E_NULLPTR;
  if (R == 0) return 0;
  // (the backup only reads links, leaf, move and leaf_id: UctArgs serves the select too, where they are written)
  u.boards = boards; u.links = const_cast<int32_t *>(links); u.stats = stats; u.leaf = const_cast<uint32_t *>(leaf);
  u.move = const_cast<int32_t *>(move); u.leaf_id = const_cast<int32_t *>(leaf_id); u.counts = counts; u.sums = sums;
  u.totals = totals; u.node_amaf = node_amaf; u.amaf = amaf;
  return launch_roots(k_uct_backup_leaves<RAVE>, leaf, R, hip_stream, u, virt, L);
}

}  // namespace

extern "C" {

int32_t gg_uct_select_leaves(int64_t R, int32_t N, int32_t I, int32_t L, int32_t K, double c, const double *log_table,
                             const uint32_t *boards, int32_t *child, int32_t *links, int32_t *stats, int32_t *nodes, int32_t *virt,
                             uint32_t *leaf, int32_t *move, int32_t *leaf_id, void *hip_stream) {
  return select_leaves<false>(R, N, I, L, K, c, 1.0, 0.0, log_table, boards, child, links, stats, nullptr, nodes, virt, leaf, move,
                              leaf_id, hip_stream);
}

int32_t gg_uct_backup_leaves(int64_t R, int32_t N, int32_t I, int32_t L, int32_t K, const int32_t *counts, const int64_t *sums,
                             int64_t *totals, uint32_t *boards, const int32_t *links, int32_t *stats, int32_t *virt,
                             const uint32_t *leaf, const int32_t *move, const int32_t *leaf_id, void *hip_stream) {
  return backup_leaves<false>(R, N, I, L, K, counts, sums, nullptr, totals, boards, links, stats, nullptr, virt, leaf, move, leaf_id,
                              hip_stream);
}

int32_t gg_uct_select_leaves_rave(int64_t R, int32_t N, int32_t I, int32_t L, int32_t K, double c, double rave_equiv, double fpu,
                                  const double *log_table, const uint32_t *boards, int32_t *child, int32_t *links, int32_t *stats,
                                  const int32_t *node_amaf, int32_t *nodes, int32_t *virt, uint32_t *leaf, int32_t *move,
                                  int32_t *leaf_id, void *hip_stream) {
  return select_leaves<true>(R, N, I, L, K, c, rave_equiv, fpu, log_table, boards, child, links, stats, node_amaf, nodes, virt, leaf,
                             move, leaf_id, hip_stream);
}

int32_t gg_uct_backup_leaves_rave(int64_t R, int32_t N, int32_t I, int32_t L, int32_t K, const int32_t *counts, const int64_t *sums,
                                  const int32_t *amaf, int64_t *totals, uint32_t *boards, const int32_t *links, int32_t *stats,
                                  int32_t *node_amaf, int32_t *virt, const uint32_t *leaf, const int32_t *move,
                                  const int32_t *leaf_id, void *hip_stream) {
  return backup_leaves<true>(R, N, I, L, K, counts, sums, amaf, totals, boards, links, stats, node_amaf, virt, leaf, move, leaf_id,
                             hip_stream);
}

int32_t gg_uct_prior_expand_leaves(int64_t R, int32_t N, int32_t I, int32_t L, const int32_t *weights, const uint32_t *leaf,
                                   const int32_t *move, const int32_t *leaf_id, int32_t *node_amaf, void *hip_stream) {
  if (N < 2 || N > GG_MAX_BOARD || R < 0) return GG_E_BADSIZE;
  if (I < 1 || I == 0x7FFFFFFF || L < 1) return GG_E_BADARG;
  if (!rows_ok(R, L)) return GG_E_BADSIZE;
  if (!weights || !leaf || !move || !leaf_id || !node_amaf) return GG_E_NULLPTR;
  if (R == 0) return 0;
  if ((uintptr_t)node_amaf & 3u) return GG_E_BADARG;
  // gg_prior.hip's launch: one single-wave workgroup per four (N <= 13) / two boards, at most 64 per compute unit
  OnDeviceOf on_dev(leaf);
  const int64_t B = R * L, cap = (int64_t)on_dev.cus() * 64;
  by_rows(N, [&](auto t) {
    constexpr int RW = decltype(t)::R;
    const int64_t groups = (B + Planes<RW>::NBW - 1) / Planes<RW>::NBW;
    k_move_priors_leaves<RW><<<(unsigned)(groups < cap ? groups : cap), kWave, 0, (hipStream_t)hip_stream>>>(
        leaf, move, weights, reinterpret_cast<uint32_t *>(node_amaf), leaf_id, I, L, B, N);
  });
  return (int32_t)hipGetLastError();
}

}  // extern "C"
