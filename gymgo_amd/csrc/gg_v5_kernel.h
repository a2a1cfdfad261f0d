// gg_v5_kernel.h - the body of k_rollout5 (gg_v5.h), included once per playout policy: GG_R5_NAME = the kernel's name,
// GG_R5_POL = the policy of its draw (kPolUniform: k_rollout5; kPolNoEyeFill: k_rollout5_pol; kPolTactical: k_rollout5_tac, DESIGN 34;
// kPolPattern: k_rollout5_pat, DESIGN 36 - it READS last_actions, the previous action of every board, which must not be null).  Textual inclusion
// and not a shared inline body: k_rollout5 stays the kernel it was, instruction for instruction and by name (bench.py ties
// its PMC record to the machine code behind the mangled name).  No include guard.
// GG_R5_LOG (optional; defined: the move-log variants of gg_r5_log.hip): the kernel takes one more argument, mvlog uint16
// [B][plies], and the even lane of every live pair stores the ply's action there - entry [b][t] is the action board b played at ply t of
// the launch (a point, or N^2 for the pass); a board that is not live on a ply stores nothing.  Without it this file is what it was.
// ws (byte planes only, nullable: gg_batch_rollout_ws): the caller's workspace, uint32 [B][5 N + 1] in the layout of a tracked board.
// The load takes M of a board from there when its stones equal the workspace's rows EXACTLY (checked per pair of boards) and skips
// the from-scratch analysis; the store leaves the stones and M of every board it wrote, or analysed, behind.  Words 0 .. 2 N (the
// stones) and 3 N .. 5 N (M & black, M & white) of a board are used; the others are never touched.
#ifdef GG_R5_LOG
#define GG_R5_LOG_PARAM , uint16_t *__restrict__ mvlog
#else
#define GG_R5_LOG_PARAM
#endif
template <int R, int IO>
__global__ __launch_bounds__(kWave, 2) void GG_R5_NAME(uint8_t *__restrict__ states, uint64_t *__restrict__ rng,
                                                       int32_t *__restrict__ last_actions, int64_t *__restrict__ steps_done,
                                                       int64_t B, uint32_t inv, int plies, int auto_reset, int nb,
                                                       uint32_t *__restrict__ ws GG_R5_LOG_PARAM) {
  constexpr int POL = GG_R5_POL;
  static_assert(IO == 0 || IO == 2, "byte planes or tracked boards");
  constexpr int N = R;
  constexpr int RS = Lds5<R>::RS;
  constexpr int RV = (R + 3) / 4;
  constexpr int RPL = Lds5<R>::RPL;
  constexpr int PL = kNB5 * RS;   // words per plane of all boards
  constexpr int ZERO = Lds5<R>::kZero, DUMP = Lds5<R>::kDump;
  constexpr bool TRACKED = IO == 2;
  constexpr int P = N * N, S = 6 * P, W = 5 * N + 1;
  constexpr uint32_t FULLROW = (1u << N) - 1u;
  __shared__ __attribute__((aligned(16))) uint32_t lds[Lds5<R>::kTotal];
  uint32_t *st = lds + Lds5<R>::kState;     // st[colour * PL + board * RS + row]
  uint32_t *flagsv = lds + Lds5<R>::kMeta;  // bit 0 turn, 1 passed, 2 done, 3 on, 5 reset (dirty)
  int *lastv = reinterpret_cast<int *>(lds + Lds5<R>::kMeta + kNB5);
  int *playedv = reinterpret_cast<int *>(lds + Lds5<R>::kMeta + 2 * kNB5);
  uint32_t *rngv = lds + Lds5<R>::kMeta + 3 * kNB5;   // [2 * s], [2 * s + 1]
  uint32_t *tmp = lds + Lds5<R>::kTmp;      // tmp[(half * 2 + set) * RS + row], set 0 = invalid (GG_AB_VALID1, 19x19: valid), 1 = M
  uint32_t *clsv = lds + Lds5<R>::kCls;
  uint32_t *jobv = lds + Lds5<R>::kJob;
  uint32_t *gblk = lds + Lds5<R>::kG;
  uint32_t *sc = lds + Lds5<R>::kSc;
  constexpr bool MPLANE = Lds5<R>::kHasMpl;   // (19x19, -DGG_AB_MPLANE1=1) the rows of M stand in LDS for the job lanes
  static_assert(!MPLANE || (RPL % 2 == 0 && RS % 2 == 0 && Lds5<R>::kMpl % 2 == 0), "a lane's rows of the plane of M are 8-byte aligned pairs");
  uint32_t *mplv = lds + Lds5<R>::kMpl;       // mplv[board * RS + row]
  uint32_t *v2 = lds + Lds5<R>::kV2;
  uint32_t *park = lds + Lds5<R>::kUnion;   // tracked I/O: park[set * PL + board * RS + row], set 0 invalid, 1 mb, 2 mw
  const int64_t ngroups = (B + nb - 1) / nb;

  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t b_first = g * nb;
    int ln0;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln0));
    const Half hf = make_half(ln0, N, inv);
    const bool row = hf.hl < RS;
    const int s5 = hf.lane >> 1, t2 = hf.lane & 1, r05 = RPL * t2;   // board / lane of the pair / first row of this lane
    // the next mover's invalid-move mask and the stones of groups with >= 2 liberties, rows r05 .. r05 + RPL - 1 of board
    // s5: in registers from here to the write-back
    // (-DGG_AB_VALID1=1, 19x19: the rows carry the VALID points, full & ~invalid, under the name val_r - gg_v5.h; the load converts once,
    // the write-back converts back once, and an absent board's rows are zero either way: nothing is ever drawn from them)
    constexpr bool VAL = GG_AB_VALID1 != 0 && R == 19;
    uint32_t inv_r[RPL], M[RPL];
#define val_r inv_r   /* (the same registers under the name of what they hold with VAL) */
#pragma unroll
    for (int r = 0; r < RPL; ++r) inv_r[r] = M[r] = 0u;
    uint32_t wsmiss = 0;   // (workspace launches) bit s: board s was analysed from scratch at load - its workspace entry is rewritten
    GG_WSC_DECL;
    GG_LS_DECL;
    GG_PROF_DECL;
    // ---------------------------------------------------------------- load
    WAVE_SYNC();
    if (TRACKED) {
      // the group's boards are ONE contiguous block of nb x (5 N + 1) words: global -> LDS by LDS-DMA, all of it in flight
      // at once, sorted from the landing area (as k_rollout4 does)
      const int64_t nbrd = (B - b_first) < nb ? (B - b_first) : nb;
      const int nw = (int)nbrd * W;
      const uint32_t *gp = reinterpret_cast<const uint32_t *>(states) + b_first * (int64_t)W;
      constexpr int KD = Lds5<R>::kDmaWords / 256;   // DMA instructions per lane
      const uint8_t *gb = reinterpret_cast<const uint8_t *>(gp);
      const uint32_t mis = (uint32_t)((uintptr_t)gb & 15u);
      const int nvec = (int)((mis + (uint32_t)nw * 4u + 15u) >> 4);
      WAVE_SYNC();
      lds_drain();
      {
        const uint32_t stage_lds = lds_addr(park);
#pragma unroll
        for (int k = 0; k < KD; ++k) {
          const int v = hf.lane + kWave * k;
          if (v < nvec) dma16(gb - mis + 16 * v, stage_lds + 1024u * (uint32_t)k);
        }
      }
      uint64_t xg = 0;
      if (hf.lane < kNB5) xg = rng[(hf.lane < nb && b_first + hf.lane < B) ? b_first + hf.lane : B - 1];
      for (int i = hf.lane; i < 2 * PL; i += kWave) st[i] = 0;      // rows N .. RS-1 and absent boards read as zero
      if (hf.lane < Lds5<R>::kPad) lds[hf.lane] = 0;
      dma_wait();
      WAVE_SYNC();
      const uint32_t *stg = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(park) + mis);   // word i of the block
      for (int i = hf.lane; i < (int)nbrd * 2 * N; i += kWave) {
        const int sb = i / (2 * N), w = i - sb * (2 * N);
        const int pl = w >= N ? 1 : 0;
        st[pl * PL + sb * RS + (w - pl * N)] = stg[sb * W + w];
      }
      if (hf.lane < kNB5) {
        const int sb = hf.lane;
        const bool on = sb < nb && b_first + sb < B;
        flagsv[sb] = on ? ((stg[sb * W + 5 * N] & 7u) | 8u) : 0u;
        lastv[sb] = -1;
        playedv[sb] = 0;
        rngv[2 * sb] = (uint32_t)xg;
        rngv[2 * sb + 1] = (uint32_t)(xg >> 32);
      }
      {
        const bool have = s5 < (int)nbrd;
        const uint32_t *bq = stg + (have ? s5 : 0) * W;
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
          const int rw = r05 + r;
          const bool ok = have && rw < N;
          const int rc = ok ? rw : 0;
          const uint32_t iv = bq[2 * N + rc], mb = bq[3 * N + rc], mw = bq[4 * N + rc];
          if constexpr (VAL) val_r[r] = ok ? (FULLROW & ~iv) : 0u;
          else inv_r[r] = ok ? iv : 0u;
          M[r] = ok ? (mb | mw) : 0u;
        }
      }
      WAVE_SYNC();
    } else {
      if (hf.lane < kNB5) flagsv[hf.lane] = 0;                       // boards beyond nb: off
      for (int i = hf.lane; i < 2 * PL; i += kWave) st[i] = 0;
      if (hf.lane < Lds5<R>::kPad) lds[hf.lane] = 0;
      WAVE_SYNC();
      // Byte planes: pairs of boards, first classes by the per-ply analysis (analyze2); the global loads of pair i + 1 are
      // issued before pair i is converted
      constexpr int NVL = (4 * R * R + 15 + 15) / 512 + 1;   // 16-byte vectors per lane
      static_assert(NVL <= 3, "vectors per lane of a staged board");
      if (hf.lane < kNB5) {   // the generator states of the whole group: one coalesced load
        const uint64_t x = rng[(b_first + hf.lane < B) ? b_first + hf.lane : B - 1];
        rngv[2 * hf.lane] = (uint32_t)x;
        rngv[2 * hf.lane + 1] = (uint32_t)(x >> 32);
      }
      uint4 cv0 = make_uint4(0, 0, 0, 0), cv1 = cv0, cv2 = cv0, nv0 = cv0, nv1 = cv0, nv2 = cv0;
      uint32_t cfb = 0, nfb = 0;
      // the workspace rows of the lane's board (row lanes): black, white, M & black, M & white - fetched with the pair's bytes
      uint32_t cw0 = 0, cw1 = 0, cw2 = 0, cw3 = 0, nw0 = 0, nw1 = 0, nw2 = 0, nw3 = 0;
#define GG_ISSUE_WS5(I, A0, A1, A2, A3)                                                                                \
      do {                                                                                                             \
        const int s_ = 2 * (I) + hf.h;                                                                                 \
        const int64_t b_ = (b_first + s_ < B) ? b_first + s_ : B - 1;                                                  \
        if (hf.hl < N) {                                                                                               \
          const uint32_t *wp_ = ws + b_ * (int64_t)W + hf.hl;                                                          \
          A0 = wp_[0]; A1 = wp_[N]; A2 = wp_[3 * N]; A3 = wp_[4 * N];                                                  \
        }                                                                                                              \
      } while (0)
#define GG_ISSUE_PAIR5(I, V0, V1, V2, FB)                                                                              \
      do {                                                                                                             \
        const int s_ = 2 * (I) + hf.h;                                                                                 \
        const int64_t b_ = (b_first + s_ < B) ? b_first + s_ : B - 1;                                                  \
        const uint8_t *gs_ = states + b_ * (int64_t)S;                                                                 \
        FB = 0;                                                                                                        \
        if (hf.hl < 4) {                                                                                               \
          const int off_ = hf.hl == 0 ? 2 * P : hf.hl == 1 ? 3 * P : hf.hl == 2 ? 4 * P : 5 * P;                       \
          FB = gs_[off_];                                                                                              \
        }                                                                                                              \
        const uint32_t mis_ = (uint32_t)((uintptr_t)gs_ & 15u);                                                        \
        const uint4 *ga_ = reinterpret_cast<const uint4 *>(gs_ - mis_);                                                \
        const int nv_ = (int)(mis_ + 4 * P + 15) >> 4;                                                                 \
        if (hf.hl < nv_) V0 = ga_[hf.hl];                                                                              \
        if (NVL > 1 && hf.hl + 32 < nv_) V1 = ga_[hf.hl + 32];                                                         \
        if (NVL > 2 && hf.hl + 64 < nv_) V2 = ga_[hf.hl + 64];                                                         \
      } while (0)
      if (nb >= 2) GG_ISSUE_PAIR5(0, cv0, cv1, cv2, cfb);
      if (ws && nb >= 2) GG_ISSUE_WS5(0, cw0, cw1, cw2, cw3);
#pragma unroll 1
      for (int i = 0; i < nb / 2; ++i) {
        if (i + 1 < nb / 2) GG_ISSUE_PAIR5(i + 1, nv0, nv1, nv2, nfb);
        if (ws && i + 1 < nb / 2) GG_ISSUE_WS5(i + 1, nw0, nw1, nw2, nw3);
        const int s = 2 * i + hf.h;
        const bool on = b_first + s < B;
        const int64_t b = on ? b_first + s : B - 1;
        uint32_t black, white, invalid, mb = 0, mw = 0;
        const uint8_t *gs = states + b * (int64_t)S;
        uint8_t *io = reinterpret_cast<uint8_t *>(v2) + hf.h * Cfg<R>::kIoBytes;
        const uint32_t mi = (uint32_t)((uintptr_t)gs & 15u);
        const int nv = (int)(mi + 4 * P + 15) >> 4;
        GG_LS_START;
        const uint32_t flags = half_of(__ballot(cfb != 0), hf.h) & 0xFu;   // bit 0 turn, 1 (unused), 2 passed, 3 done
        WAVE_SYNC();
        uint4 *iov = reinterpret_cast<uint4 *>(io);
        if (hf.hl < nv) iov[hf.hl] = cv0;
        if (NVL > 1 && hf.hl + 32 < nv) iov[hf.hl + 32] = cv1;
        if (NVL > 2 && hf.hl + 64 < nv) iov[hf.hl + 64] = cv2;
        WAVE_SYNC();
        black = plane_to_row<R>(io + mi, N, hf.hl);
        white = plane_to_row<R>(io + mi + P, N, hf.hl);
        invalid = plane_to_row<R>(io + mi + 3 * P, N, hf.hl);
        const uint32_t turn = flags & 1u, passed = (flags >> 2) & 1u, done = (flags >> 3) & 1u;
        GG_LS(0);
        // both boards of the pair stand in the workspace stone for stone: their M comes from there, no analysis
        bool known = false;
        if (ws) {
          known = __ballot(hf.hl < N && (black != cw0 || white != cw1)) == 0;
          if (known) { mb = cw2; mw = cw3; }
          else wsmiss |= 3u << (2 * i);
          GG_WSC(known);
        }
        if (!known) {
          uint32_t ab;
          analyze2<R, false>(black, white, hf.full_l1 & ~(black | white), hf, v2, mb, ab, mw, nullptr, nullptr, true);
        }
        GG_LS(1);
        if (row) {
          st[0 * PL + s * RS + hf.hl] = black;
          st[1 * PL + s * RS + hf.hl] = white;
          tmp[(hf.h * 2 + 0) * RS + hf.hl] = VAL ? (hf.full_l1 & ~invalid) : invalid;   // (VAL: the row lane converts, zero for rows >= N)
          tmp[(hf.h * 2 + 1) * RS + hf.hl] = mb | mw;
        }
        if (hf.hl == 0) {
          flagsv[s] = turn | (passed << 1) | (done << 2) | (on ? 8u : 0u);
          lastv[s] = -1;
          playedv[s] = 0;
        }
        WAVE_SYNC();
        if ((hf.lane >> 2) == i) {   // the two pairs of lanes that own these boards pick their rows up
          const uint32_t *tp = tmp + ((s5 & 1) * 2) * RS + r05;
#pragma unroll
          for (int r = 0; r < RPL; ++r) {
            inv_r[r] = tp[r];
            M[r] = tp[RS + r];
          }
        }
        WAVE_SYNC();
        GG_LS(2);
        cv0 = nv0; cv1 = nv1; cv2 = nv2; cfb = nfb;
        if (ws) { cw0 = nw0; cw1 = nw1; cw2 = nw2; cw3 = nw3; }
      }
#undef GG_ISSUE_PAIR5
#undef GG_ISSUE_WS5
      GG_LS_FLUSH;
    }
    // the slot of an absent job: an all-zero block and class word (the loop area was the load's scratch)
    WAVE_SYNC();
    for (int i = hf.lane; i < kWave * RS; i += kWave) sc[i] = 0u;   // the seed blocks: all zero between two uses
    // (-DGG_AB_DESC1=1, 19x19: a lane without a job reads the descriptor of the absent job - board 0, row offset 0 - and not the dump
    // slot's, whose high bits hold whatever seed off the board was dumped last: its row offset must be one of a board)
    if (GG_AB_DESC1 != 0 && R == 19 && hf.lane == 0) jobv[ZERO] = 0u;
    if constexpr (MPLANE) {
      // the plane of M (gg_v5.h: GG_AB_MPLANE1): every pair of lanes stores the rows the load left it - from the tracked board, from the
      // workspace or from the from-scratch analysis, zero for an absent board - now that the load is done with the loop area
      uint2 *pm2 = reinterpret_cast<uint2 *>(mplv + s5 * RS + r05);
#pragma unroll
      for (int r = 0; r < RPL; r += 2) pm2[r / 2] = make_uint2(M[r], M[r + 1]);
    }
    WAVE_SYNC();

    // the flag word, the generator and the played plies of this lane's board travel in REGISTERS through the plies (the same
    // in both lanes of a pair): read back from LDS every ply they cost phase 1 a dependent round trip; LDS keeps the copies
    // the write-back reads (stores only)
    uint32_t flr = flagsv[s5];
    const uint64_t x0r = ((uint64_t)rngv[2 * s5 + 1] << 32) | rngv[2 * s5];
    int playedr = 0;
    // pattern: the board's previous action (the same in both lanes of the pair) - a point of the board, or -1 for anything else: the
    // caller's last_actions entry, whatever it holds, then the action of every live ply
    int prevr = -1;
    if constexpr (POL == kPolPattern) {
      const bool have = s5 < nb && b_first + s5 < B;
      const int la = last_actions[have ? b_first + s5 : B - 1];
      prevr = (have && (uint32_t)la < (uint32_t)P) ? la : -1;
    }
#ifdef GG_AB_P3
    uint32_t p3c_[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
#ifdef GG_LIVE_CHECK
    int drawsr = 0;        // plies on which this board was live (drew a move or passed)
    bool was_dead = false; // a ply on which it was not live has passed
#endif
    // ---------------------------------------------------------------- the plies
    GG_PROF(6);   // load
    FairShare fair(lds + Lds5<R>::kFair);
    const uint32_t fair_lag = plies >= 192 ? 24u : (plies >= 16 ? (uint32_t)plies >> 3 : 2u);
    bool lead = false;   // this wave is >= fair_lag plies ahead of its SIMD-mate
    uint32_t uq = 0;   // this lane's pre-mixed draw: lane j of a pair holds the one of ply (t & ~1) + j, swapped every ply
    // (-DGG_AB_DRAWADD1=1, 19x19) the draw's counter before the mix, x0 + (t + t5) c at the even ply t: a running value, advanced by 2 c
    // behind each mix, instead of a 32 x 64 multiply every second ply (gg_v5.h)
    constexpr bool DADD = GG_AB_DRAWADD1 != 0 && R == 19;
    // (-DGG_AB_DRAWC1=1 on top of it: the counter starts one c further on, x0 + (t + t5 + 1) c, which is what the mix takes in - no + c
    // on a copy every second ply)
    constexpr bool DRAWC = DADD && GG_AB_DRAWC1 != 0;
    uint64_t xdr = x0r + (uint64_t)(uint32_t)((ln0 & 1) + (DRAWC ? 1 : 0)) * 0x9E3779B97F4A7C15ull;   // (dead code without DADD)
#if GG_AB_LANE1
    // what depends on the lane number alone, formed ONCE and kept in registers through the plies (gg_v5.h: GG_AB_LANE1) - at 19x19,
    // where two waves per SIMD leave ~70 VGPRs free; 13x13 and 9x9 stand at 168 and 127 of the 170 and 128 VGPRs their three and four
    // waves allow and keep the fresh v_mbcnt (the constants below are dead code there)
    constexpr bool KEEP = R == 19;
    const int lnK = ln0;
    const int s4K = (lnK >> 1) & 31, t5K = lnK & 1, r0K = RPL * t5K;
    const bool blK = s4K < nb;
    const uint32_t fullK = (r0K + RPL - 1 < N) ? FULLROW : 0u;   // the one row of full[] that depends on the lane: the pair's last
    uint32_t *const stK = st + s4K * RS;        // the board's rows of the black plane; the white plane's lie PL words behind
    uint32_t *const gbK = gblk + 2 * s4K * RS;  // the board's G block, behind it its collection block
    uint32_t *const clsK = clsv + s4K;          // the board's info word
    uint32_t *const metaK = flagsv + s4K;       // the board's flag word; last action and played plies kNB5 and 2 kNB5 words behind
    uint32_t *const blkK = sc + lnK * RS;       // the seed block of this lane's job
#endif
    // (-DGG_AB_DESC1=1, 19x19) what the board's lanes put into every job descriptor they post: the board in bits 0-4 and its row offset
    // board * RS in bits 21-30, one kept word (gg_v5.h); the job lane takes the offset out by one shift
    constexpr bool DESC = GG_AB_DESC1 != 0 && R == 19;
    static_assert((kNB5 - 1) * RS < 1024, "the row offset of a board fits bits 21-30 of a job descriptor");
    uint32_t descK = (uint32_t)((ln0 >> 1) & 31) | ((uint32_t)(((ln0 >> 1) & 31) * RS) << 21);   // (dead code without DESC)
    if constexpr (DESC) asm volatile("" : "+v"(descK));   // (kept as it is: not put together again every ply)
#pragma unroll 1
    for (int t = 0; t < plies; ++t) {
      // Fair share of the SIMD (gg_common.h) every fourth ply - without it the older of a SIMD's two waves runs ahead and the
      // launch ends on one wave per SIMD: 1.51 -> 1.66 ms - combined with the PHASE of the ply: the flood of phase 2b is one
      // dependent chain per lane that needs the issue port every fifth cycle or so, the other phases have ten independent
      // rows per lane.  A wave in the flood therefore yields (priority 0 / 1: leader / straggler) and a wave in any other phase
      // issues first (2 / 3): 1.509 -> 1.488 ms per launch of 65 536 games x 256 plies; the other way round 1.561.
      if ((t & 3) == 0 && plies >= 8) {
        const uint32_t left = (uint32_t)(plies - t);
        lead = fair.behind((uint32_t)t, left < fair_lag ? (left > 2u ? left : 2u) : fair_lag) != 0u;
        if (lead) __builtin_amdgcn_s_setprio(2); else __builtin_amdgcn_s_setprio(3);
      }
#if GG_AB_LANE1
      int ln = lnK;
      if constexpr (!KEEP) asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
      const int s4 = KEEP ? s4K : (ln >> 1) & 31, t5 = KEEP ? t5K : ln & 1, r0 = KEEP ? r0K : RPL * t5;   // board, lane of the pair, first row of this lane
      const bool bl = KEEP ? blK : s4 < nb;
      uint32_t full[RPL];   // the N-bit row mask of the lane's rows that exist
#pragma unroll
      for (int r = 0; r < RPL; ++r) full[r] = (KEEP && RPL + r < N) ? FULLROW : (KEEP && r == RPL - 1 ? fullK : ((r0 + r < N) ? FULLROW : 0u));
#else
      int ln;
      asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
      const int s4 = (ln >> 1) & 31, t5 = ln & 1, r0 = RPL * t5;   // board, lane of the pair, first row of this lane
      const bool bl = s4 < nb;
      uint32_t full[RPL];   // the N-bit row mask of the lane's rows that exist
#pragma unroll
      for (int r = 0; r < RPL; ++r) full[r] = (r0 + r < N) ? FULLROW : 0u;
#endif
      // the board's rows of the mover's (GG_PM) and of the other (GG_PO) plane, `turn` 0 black / 1 white
#if GG_AB_LANE1
#define GG_PM(turn) (KEEP ? ((turn) ? stK + PL : stK) : st + (turn) * PL + s4 * RS)
#define GG_PO(turn) (KEEP ? ((turn) ? stK : stK + PL) : st + (1u - (turn)) * PL + s4 * RS)
#define GG_GB (KEEP ? gbK : gblk + 2 * s4 * RS)
#define GG_CLS (KEEP ? clsK : clsv + s4)
#else
#define GG_PM(turn) (st + (turn) * PL + s4 * RS)
#define GG_PO(turn) (st + (1u - (turn)) * PL + s4 * RS)
#define GG_GB (gblk + 2 * s4 * RS)
#define GG_CLS (clsv + s4)
#endif

      int a_q;
      uint32_t fl_q;
#if GG_AB_MOVE_RC
      uint32_t rc_q;               // the drawn point as (row << 5) | column; 0 on a pass, never off the board
#endif
      // phase 1 - two lanes per board, RPL rows each: liveness, the draw, the k-th valid point of the mask
      {
        const uint32_t fl = flr;
        // (-DGG_AB_BALLOT1=1 at 19x19 only, like the other cuts of round 27: 13x13 and 9x9 keep round 20's machine code)
        constexpr bool CMP1 = GG_AB_BALLOT1 != 0 && R == 19;
        bool live, reset;
        if constexpr (CMP1) {
          // bit 3 of the flag word is `on`, bit 2 `done`: live iff the board exists, is on and not (done without auto-reset), reset iff
          // it exists, is on and done with auto-reset - each ONE compare of the masked bits, and a compare is the form whose wave-wide
          // mask costs nothing more (a bool put together from several tests goes through v_cndmask 0 / 1 and a second compare)
          uint32_t flb = bl ? fl : 0u;
          asm volatile("" : "+v"(flb));   // (or the compiler turns the masked word back into the AND of two tests)
          live = (flb & (auto_reset ? 8u : 12u)) == 8u;
          reset = (flb & 12u) == (auto_reset ? 12u : ~0u);   // auto-reset: the board is init_state from now on
        } else {
          const bool on = bl && ((fl >> 3) & 1u);
          const bool done = (fl >> 2) & 1u;
          live = on && !(done && !auto_reset);
          reset = live && done;           // auto-reset: the board is init_state from now on
        }
        // Invariant: a board's live plies are a PREFIX of the launch (`on` never changes inside it; a done board stays done
        // unless auto_reset, and then it is live on every ply), and every live ply draws exactly once and moves (a_q >= 0:
        // phase 3 counts it) - so `played` equals the number of draws, which the write-back turns into the generator's advance.
#ifdef GG_LIVE_CHECK
        if (live && was_dead) atomicAdd(&gg_live_bad, 1ull);
        was_dead = was_dead || (bl && !live);
        drawsr += live ? 1 : 0;
#endif
        if constexpr (VAL) {
          // the reset path in front of the draw: it is wave-uniform and known from the flag word.  A board being reset draws over the
          // empty board - its valid rows are full[], its M is zero - and its planes are cleared HERE: DS instructions of a wave execute
          // in order, so the clears stand ahead of the policies' stone reads below and of phase 1's stone store (the policy sets keep
          // their & ~rm all the same).  The early exit moves with it: nothing below outlives the loop but what a live board writes.
          uint64_t resetm = CMP1 ? GG_BALLOT5(reset) & 0x5555555555555555ull : GG_BALLOT5(reset && t5 == 0);
          const bool none_live = GG_BALLOT5(live) == 0;
          if (none_live && resetm == 0) break;
          if (resetm) {   // rare
            if (reset) {
#pragma unroll
              for (int r = 0; r < RPL; ++r) { val_r[r] = full[r]; M[r] = 0u; }
            }
            while (resetm) {
              const int s = (__ffsll((unsigned long long)resetm) - 1) >> 1;   // lane 2 s -> board s
              resetm &= resetm - 1;
              for (int i = hf.lane; i < 2 * RS; i += kWave) st[(i / RS) * PL + s * RS + (i % RS)] = 0;
              if constexpr (MPLANE) { if (hf.lane < RS) mplv[s * RS + hf.lane] = 0; }   // (its jobs of THIS ply read M from the plane)
              if (hf.lane == 0) flagsv[s] = 8u | 32u;   // on, reset (written back even if nothing is played)
            }
            if (none_live) break;
            WAVE_SYNC();
          }
        }
        uint32_t v[RPL], p[RPL];
        const uint32_t rm = reset ? ~0u : 0u;   // a board being reset plays on the empty board
        uint32_t eye[RPL];
        uint32_t tl[RPL];            // pattern: the local-response points of the lane's rows
        uint32_t tc[RPL], te[RPL];   // tactical: the capture and the escape points of the lane's rows
        constexpr bool TAC = POL == kPolTactical || POL == kPolPattern;   // (the pattern policy is the tactical one with a tier more)
        constexpr uint32_t FB = kPolBits<POL>, FM = (1u << FB) - 1u;       // the fields of the packed counts
        // pattern: the matching points of the three rows around the previous move (columns pc - 1 .. pc + 1 without the
        // move itself), and the first of those rows (-4: no previous point - none given, a pass, or a board being reset)
        uint32_t pk[3] = {0u, 0u, 0u};
        int prw = -4;
        if constexpr (POL != kPolUniform) {
          // no_eye_fill: the mover's eyes leave the candidates.  The stone rows of the lane come out of LDS (the planes are as
          // phase 3 of the last ply - or the load - left them), the row beyond the pair's seam out of the partner lane by one
          // DPP swap per colour and side; off the board the mover's rows read as all ones and the opponent's as zero.
          const uint32_t turn = fl & 1u;
          const uint32_t *pm = GG_PM(turn) + r0, *po = GG_PO(turn) + r0;
          uint32_t me[RPL], op[RPL];
#pragma unroll
          for (int r = 0; r < RPL; ++r) { me[r] = pm[r]; op[r] = po[r]; }   // (rows >= N are zero)
          const uint32_t me_up = dpp0<QP_X1>(me[RPL - 1]), op_up = dpp0<QP_X1>(op[RPL - 1]);   // row RPL - 1, for the odd lane
          const uint32_t me_dn = dpp0<QP_X1>(me[0]), op_dn = dpp0<QP_X1>(op[0]);               // row RPL, for the even lane
          // tactical: M[] is in registers, its rows beyond the seam come by the same swaps; off the board M reads as all ones
          // like the mover's rows (the border is a mover's stone with liberties: never empty, never in atari)
          uint32_t m_up = 0u, m_dn = 0u;
          if constexpr (TAC) { m_up = dpp0<QP_X1>(M[RPL - 1]); m_dn = dpp0<QP_X1>(M[0]); }
#pragma unroll
          for (int r = 0; r < RPL; ++r) {
            const int rw = r0 + r;
            const uint32_t meU = r ? me[r - 1] : (t5 ? me_up : FULLROW), opU = r ? op[r - 1] : (t5 ? op_up : 0u);
            const uint32_t meDn = r + 1 < RPL ? me[r + 1] : (t5 ? 0u : me_dn), opD = r + 1 < RPL ? op[r + 1] : (t5 ? 0u : op_dn);
            const uint32_t meD = rw + 1 >= N ? FULLROW : meDn;
            const uint32_t edge = (rw == 0 || rw == N - 1) ? FULLROW : (1u | (1u << (N - 1)));
            eye[r] = eye_row(me[r], op[r], meU, meD, opU, opD, full[r], edge, N) & ~rm;
            if constexpr (TAC) {
              const uint32_t MU = r ? M[r - 1] : (t5 ? m_up : FULLROW);
              const uint32_t MDn = r + 1 < RPL ? M[r + 1] : (t5 ? 0u : m_dn);
              const uint32_t MD = rw + 1 >= N ? FULLROW : MDn;
              tactical_rows(me[r], op[r], M[r], meU, meD, opU, opD, MU, MD, full[r], tc[r], te[r]);
              tc[r] &= ~rm;   // (a board being reset: the planes and M still hold the finished game)
              te[r] &= ~rm;
            }
          }
          if constexpr (POL == kPolPattern) {
            // the five rows around the previous move come out of the board's planes in LDS at the move's own row - whichever lane
            // of the pair holds them, both lanes look at all eight points -, padded (pattern_pad), all ones off the board; eight
            // table bits (pattern_cols3).  Nothing is indexed without a previous point: row 0 is read for nothing.
            const bool hasp = prevr >= 0 && !reset;
            const int pv = hasp ? prevr : 0;
            const int pr = pv / N, pc = pv - pr * N;
            const uint32_t *bm = GG_PM(turn), *bo = GG_PO(turn);
            uint32_t wm[5], wo[5];
#pragma unroll
            for (int d = 0; d < 5; ++d) {
              const int rw = pr - 2 + d;
              const bool inb = (uint32_t)rw < (uint32_t)N;
              const uint32_t a = bm[inb ? rw : 0], b = bo[inb ? rw : 0];
              wm[d] = inb ? pattern_pad(a, N) : ~0u;
              wo[d] = inb ? pattern_pad(b, N) : ~0u;
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
              const bool inb = hasp && (uint32_t)(pr - 1 + a) < (uint32_t)N;
              const uint32_t m = pattern_cols3(wm[a], wo[a], wm[a + 1], wo[a + 1], wm[a + 2], wo[a + 2], pc, a != 1, N);
              pk[a] = inb ? m : 0u;
            }
            prw = hasp ? pr - 1 : -4;
          }
        }
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
          if constexpr (VAL) v[r] = val_r[r];   // (a board being reset: full[r], set in front of the draw)
          else v[r] = B3(full[r], rm, inv_r[r], TA & (TB | (~TC & 0xFF)));
          if constexpr (TAC) {
            // the three sets of the row and their counts in ONE word: F in bits 0-9, C in 10-19, E in 20-29 (<= 361 per board;
            // pattern: nine bits each, and L - at most eight points - from bit 27)
            tc[r] &= v[r];
            te[r] &= v[r];
            v[r] &= ~eye[r];
            uint32_t pw = (uint32_t)__popc(v[r]) | ((uint32_t)__popc(tc[r]) << FB) | ((uint32_t)__popc(te[r]) << (2 * FB));
            if constexpr (POL == kPolPattern) {
              const int d = r0 + r - prw;   // 0, 1, 2: the rows around the previous move
              tl[r] = v[r] & (d == 0 ? pk[0] : (d == 1 ? pk[1] : (d == 2 ? pk[2] : 0u)));
              pw |= (uint32_t)__popc(tl[r]) << (3 * FB);
            }
            p[r] = pw + (r ? p[r - 1] : 0u);
          } else {
            if constexpr (POL == kPolNoEyeFill) v[r] &= ~eye[r];
            p[r] = (uint32_t)__popc(v[r]) + (r ? p[r - 1] : 0u);
          }
        }
        uint32_t T = p[RPL - 1];
        // valid points of the board before this lane's rows (Pb) and on the whole board (n): one swap inside the pair
        const uint32_t oth = dpp0<QP_X1>(T);
        uint32_t Pb = t5 ? oth : 0u, n = T + oth;
        // The draws of a board, TWO plies at a time: the draw of ply t is mix(x0 + (t + 1) c) with x0 the generator the
        // launch found; lane j of the pair mixes the draw of ply t + j every second ply, a ply takes the even lane's and
        // the pair swaps
        if ((t & 1) == 0) {
          uint64_t xx = DADD ? xdr : x0r + (uint64_t)(uint32_t)(t + t5) * 0x9E3779B97F4A7C15ull;
          uq = (uint32_t)((DRAWC ? splitmix_mix(xx) : splitmix_next(xx)) >> 32);
          if constexpr (DADD) xdr += 2ull * 0x9E3779B97F4A7C15ull;
        }
        const uint32_t uh = dpp0<QP_L0>(uq);
        uq = dpp0<QP_X1>(uq);
        if constexpr (TAC) {
          // the tier: C, else E (pattern: else L), when the gate of this draw is open and the set is not empty, else F - the same in both lanes of
          // the pair (n holds the pair's three totals); the rows and the counts of the chosen set take the place of the valid ones
          const bool gate = (uh & 3u) != 0u;
          const bool useC = gate && ((n >> FB) & FM) != 0u, useE = gate && !useC && (POL == kPolPattern ? (n >> (2 * FB)) & FM : n >> (2 * FB)) != 0u;
          const bool useL = POL == kPolPattern && gate && !useC && !useE && (n >> (3 * FB)) != 0u;
          const uint32_t sh = useC ? FB : (useE ? 2 * FB : (useL ? 3 * FB : 0u));
          const uint32_t mc = useC ? ~0u : 0u, me_ = useE ? ~0u : 0u;
#pragma unroll
          for (int r = 0; r < RPL; ++r) {
            uint32_t vf = v[r];
            if constexpr (POL == kPolPattern) vf = B3(useL ? ~0u : 0u, tl[r], vf, T_SEL);
            v[r] = B3(mc, tc[r], B3(me_, te[r], vf, T_SEL), T_SEL);
            p[r] = (p[r] >> sh) & FM;
          }
          T = (T >> sh) & FM;
          Pb = (Pb >> sh) & FM;
          n = (n >> sh) & FM;
        }
        const uint32_t k = __umulhi(uh, POL != kPolUniform ? n : n + 1u);   // k == n: the pass (a policy: n == 0 alone)
        const bool hit = k >= Pb && k < Pb + T;       // this lane holds the k-th valid point
        int rr;
        uint32_t pos;
        if constexpr (RPL == 10) kth_set_bit10(v, p, (k - Pb) & 0x3FFu, rr, pos);
        else kth_set_bit<RPL>(v, p, (k - Pb) & 0x3FFu, rr, pos);
        const int rabs = r0 + rr;
        // (k < n: exactly one lane of the pair holds the point and hands it to the other; k, n and live are the same in both)
#if GG_AB_MOVE_RC
        // the point travels as (row, column) through the ply: phases 2a and 3 and the job lanes take it apart by shift and mask,
        // the flat index is formed once, for last_actions and the pass / idle tests.  (At most one lane of a pair hits, so the
        // pair's word is a point of the board or zero.)
        const uint32_t cand = hit ? ((uint32_t)rabs << 5) | pos : 0u;
        rc_q = cand | dpp0<QP_X1>(cand);
        const uint32_t pt = __umul24(rc_q >> 5, (uint32_t)N) + (rc_q & 31u);
#else
        const uint32_t cand = hit ? (uint32_t)(rabs * N + (int)pos) : 0u;
        const uint32_t pt = cand | dpp0<QP_X1>(cand);
#endif
        a_q = !live ? -1 : (k < n ? (int)pt : P);
        // pattern: the action of a live ply is the next ply's previous one (a pass: none)
        if constexpr (POL == kPolPattern) prevr = live ? (k < n ? (int)pt : -1) : prevr;
#ifdef GG_R5_LOG
        // the log: one predicated 2-byte store from the pair's even lane (live: the board exists, b_first + s4 < B, and t < plies).
        // A store and no load: nothing in the ply waits for it (vmcnt is next looked at by the write-back)
        if (a_q >= 0 && t5 == 0) mvlog[(b_first + s4) * (int64_t)plies + t] = (uint16_t)a_q;
#endif
        const bool place = live && hit;
        fl_q = reset ? 40u : fl;   // a board being reset: on, dirty, black to move
        // (CMP1: both lanes of a pair agree on `reset`, the even lanes by a scalar AND)
        // (VAL: the reset path stands in front of the draw; here it is dead code by two constants - a block scope around it moves 13x13's
        // and 9x9's instructions)
        uint64_t resetm = VAL ? 0ull : (CMP1 ? GG_BALLOT5(reset) & 0x5555555555555555ull : GG_BALLOT5(reset && t5 == 0));
        const bool none_live = VAL ? false : GG_BALLOT5(live) == 0;
        if (none_live && resetm == 0) break;
        if (resetm) {   // rare
          if (reset) {
#pragma unroll
            for (int r = 0; r < RPL; ++r) inv_r[r] = M[r] = 0u;
          }
          while (resetm) {
            const int s = (__ffsll((unsigned long long)resetm) - 1) >> 1;   // lane 2 s -> board s
            resetm &= resetm - 1;
            for (int i = hf.lane; i < 2 * RS; i += kWave) st[(i / RS) * PL + s * RS + (i % RS)] = 0;
            if constexpr (MPLANE) { if (hf.lane < RS) mplv[s * RS + hf.lane] = 0; }   // (its jobs of THIS ply read M from the plane)
            if (hf.lane == 0) flagsv[s] = 8u | 32u;   // on, reset (written back even if nothing is played)
          }
          if (none_live) break;
        }
        WAVE_SYNC();
        // the new stone goes into the mover's plane right away, and - as the group G it forms on its own - into the board's
        // G block (a job floods over it when q has a friendly neighbour)
        // (the lanes of EVERY board clear its G block and its collection block - a board that passes or idles leaves them
        // empty, phase 3 reads them unmasked -, then the lane that holds the point writes the stone: DS instructions of a wave
        // execute in order)
        uint32_t *gb = GG_GB;
        // (-DGG_AB_FLAT1=1 at 19x19 only: at 13x13 and 9x9 the flat stores cost the byte-plane kernels two VGPRs, and they stand at 168
        // and 127 of the 170 and 128 their three and four waves per SIMD allow)
        constexpr bool FLAT = GG_AB_FLAT1 != 0 && R == 19;
        if (FLAT || t5 == 0) *GG_CLS = 0u;   // the board's info word (FLAT: both lanes of the pair store the same zero, no exec region)
        {
          uint4 *pz = reinterpret_cast<uint4 *>(gb + t5 * RS);   // (lane 0 of the pair: the G block, lane 1: the collection block)
#pragma unroll
          for (int i = 0; i < RV; ++i) pz[i] = make_uint4(0u, 0u, 0u, 0u);
        }
        asm volatile("" ::: "memory");
        if constexpr (FLAT) {
          // no exec region: EVERY lane ORs - the lane that places the stone its bit, any other lane zero, into a row of its own board's
          // plane (nothing is written to a board that does not move) - and the G block takes the stone by an OR too: the pair's even
          // lane has just cleared it, and DS instructions of a wave execute in order
          const uint32_t turn = reset ? 0u : (fl & 1u);
          const uint32_t bit = place ? 1u << pos : 0u;
          const int rw = place ? rabs : r0;
          atomicOr(GG_PM(turn) + rw, bit);   // (ds_or without a return value: no round trip inside the phase)
          atomicOr(gb + rw, bit);
        } else if (place) {
          const int turn = reset ? 0 : (int)(fl & 1u);
          atomicOr(GG_PM(turn) + rabs, 1u << pos);   // (ds_or without a return value: no round trip inside the phase)
          gb[rabs] = 1u << pos;
        }
      }
      WAVE_SYNC();
      GG_PROF(0);

      // phase 2a - the board's lanes look at q's neighbours: lane 0 of the pair at the ones above / below, lane 1 at the ones
      // to the left / right; what the board-level tests need (empty neighbours of q, is any of them friendly, is q boxed
      // in) is one packed pair sum; the floods become jobs
      uint32_t qs;                 // bits 0-2 empty neighbours of q, 11 q has a friendly neighbour, 19 q is NOT boxed in
      int njobs;
      {
        const int a = a_q;
        const uint32_t turn = fl_q & 1u;
        const uint32_t mv1 = ((uint32_t)a < (uint32_t)P) ? 1u : 0u;   // a stone was placed
        int ar, ac;
#if GG_AB_MOVE_RC
        ar = (int)(rc_q >> 5);    // (a point of the board or zero whatever the board does: the bits are masked, not the address)
        ac = (int)(rc_q & 31u);
#else
        split_action(mv1 ? a : 0, N, inv, ar, ac);
#endif
        const uint32_t *pm = GG_PM(turn), *po = GG_PO(turn);
        uint32_t obit[2], packed = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int sg = 2 * j - 1;
          const int dr = t5 ? 0 : sg, dc = t5 ? sg : 0;
          const int nr = ar + dr, nc = ac + dc;   // row -1 .. N, column -1 .. N
          // (row -1 of a board is a zero row of the board before it or the pad, row N a zero row)
          const uint32_t rowm = pm[nr], rowo = po[nr];
          const uint32_t ncs = (uint32_t)nc & 31u;   // column -1 reads bit 31, column N bit N: never set in a row
          const uint32_t mbit = (rowm >> ncs) & mv1, ob = (rowo >> ncs) & mv1;
          const uint32_t onb = ((uint32_t)nr < (uint32_t)N && (uint32_t)nc < (uint32_t)N) ? mv1 : 0u;
          const uint32_t ex = mbit | ob;
          packed += (onb & ~ex) | (mbit << 8) | ((onb & ~ob) << 16);
          obit[j] = ob;
        }
        qs = packed + dpp0<QP_X1>(packed) + 0x70700u;
        const uint32_t friendly = (qs >> 11) & 1u;
        const uint32_t gf = t5 ? 0u : friendly;             // the pair's even lane posts the G job
        const uint32_t c = gf + obit[0] + obit[1];
        const uint64_t b0 = GG_BALLOT5((c & 1u) != 0u), b1 = GG_BALLOT5((c & 2u) != 0u);
        const uint32_t base = mbcnt64(b0) + 2u * mbcnt64(b1);
        njobs = (int)__popcll(b0) + 2 * (int)__popcll(b1);
        const uint32_t sG = base, s0 = base + gf, s1 = s0 + obit[0];
        const uint32_t dsb = DESC ? descK : (uint32_t)s4;   // the board (DESC: and its row offset in bits 21-30)
        const uint32_t common = dsb | (1u << 18) | ((turn ^ 1u) << 15);
#if GG_AB_MOVE_RC
        // (the seed travels as (row << 5) | column in bits 5-14: q itself for G, q -+ 32 / q -+ 1 for the opponent stone above / below /
        // left / right - a job that is posted has its seed on the board, the others go to the dump slot)
        const int step = t5 ? 1 : 32;
        const int sd = (int)rc_q;
#else
        // (the seed travels as a flat point index: q itself for G, q -+ N / q -+ 1 for the opponent stone above / below / left / right)
        const int step = t5 ? 1 : N;
        const int sd = a;
#endif
        jobv[gf ? sG : (uint32_t)DUMP] = (dsb | (1u << 18) | (turn << 15) | (1u << 16)) | ((uint32_t)sd << 5);
        const uint32_t dirs = (uint32_t)t5 << 20;   // bits 19-20: the direction of the job (0 up, 1 down, 2 left, 3 right)
        jobv[obit[0] ? s0 : (uint32_t)DUMP] = common | dirs | ((uint32_t)(sd - step) << 5);
        jobv[obit[1] ? s1 : (uint32_t)DUMP] = common | dirs | (1u << 19) | ((uint32_t)(sd + step) << 5);
      }
      WAVE_SYNC();

      // phase 2b - lane L runs job L: the flood (seed staged through the job's cleared block), then the liberties of the
      // group (dilate & empty, saturated at 2), all rows in registers; the class word: bits 0-1 liberties, 5 an opponent group
      // without a liberty (captured).  An opponent group that keeps >= 2 liberties zeroes
      // its block: phase 3 never sees it.
      if (!GG_AB_PRIO && plies >= 8) { if (lead) __builtin_amdgcn_s_setprio(0); else __builtin_amdgcn_s_setprio(1); }
#pragma unroll 1
      for (int jb = 0; jb < njobs; jb += kWave) {
        const int j = jb + ln;
        const bool have = j < njobs;
        const uint32_t d = jobv[have ? j : (DESC ? ZERO : DUMP)];
        const uint32_t ex = have ? 1u : 0u;
        const int sj = (int)(d & 31u);
#if GG_AB_DESC1
        // the row offset of the job's board: (DESC) bits 21-30 of the descriptor, bit 31 is never set in a posted one
        const int sjr = DESC ? (int)(d >> 21) : sj * RS;
#define GG_SJR sjr
#else
#define GG_SJR (sj * RS)
#endif
        int sr, scol;
#if GG_AB_MOVE_RC
        sr = (int)((d >> 10) & 31u);
        scol = (int)((d >> 5) & 31u);
#else
        split_action((int)((d >> 5) & 511u), N, inv, sr, scol);
#endif
        const uint32_t ownc = (d >> 15) & 1u;
        const uint32_t isG = have ? (d >> 16) & 1u : 0u;
#if GG_AB_LANE1
        uint32_t *blk = KEEP ? blkK : sc + ln * RS;   // this lane's seed block (all zero)
#else
        uint32_t *blk = sc + ln * RS;   // this lane's seed block (all zero)
#endif
        const uint4 *lds4 = reinterpret_cast<const uint4 *>(lds);
        // (DESC: word offsets, not a quotient - the row offset out of the descriptor is a multiple of four the compiler cannot see, and the
        // division costs a mask per address)
        const uint4 *pmv = DESC ? reinterpret_cast<const uint4 *>(lds + Lds5<R>::kState + (int)ownc * PL + GG_SJR)
                                : lds4 + (Lds5<R>::kState + (int)ownc * PL + sj * RS) / 4;
        const uint4 *pov = DESC ? reinterpret_cast<const uint4 *>(lds + Lds5<R>::kState + (int)(ownc ^ 1u) * PL + GG_SJR)
                                : lds4 + (Lds5<R>::kState + (int)(ownc ^ 1u) * PL + sj * RS) / 4;
        // the rows of M (the classes BEFORE this move) of the job's board, out of the registers of the two lanes that hold them
        // (-DGG_AB_MPLANE1=1, 19x19: out of the plane of M instead, below with the stone rows - the plane holds what the registers
        // hold, phase 3 of the last ply, the load or the reset path stored it, and M does not change between phase 1 and phase 3)
        const uint4 *pmmv = DESC ? reinterpret_cast<const uint4 *>(lds + Lds5<R>::kMpl + GG_SJR) : lds4 + (Lds5<R>::kMpl + sj * RS) / 4;
        uint32_t mm[R];
        if constexpr (!MPLANE) {
          const int src = 8 * sj;   // byte address of lane 2 sj for ds_bpermute
#pragma unroll
          for (int i = 0; i < RPL; ++i) {
            mm[i] = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)M[i]);
            if (RPL + i < R) mm[RPL + i] = (uint32_t)__builtin_amdgcn_ds_bpermute(src + 4, (int)M[i]);
          }
        }
        uint32_t cnt = 0;
        uint32_t res[R];   // the group (or the part of it that settles its class), normal bit order
        {
          uint32_t m[R], mrev[R], f[R], ot[R];
          {
            uint32_t mt[RV * 4], ft[RV * 4];
#pragma unroll
            for (int i = 0; i < RV; ++i) {
              const uint4 x = pmv[i], y = pov[i];
              mt[4 * i] = x.x; mt[4 * i + 1] = x.y; mt[4 * i + 2] = x.z; mt[4 * i + 3] = x.w;
              ot[4 * i] = y.x;
              if (4 * i + 1 < R) ot[4 * i + 1] = y.y;
              if (4 * i + 2 < R) ot[4 * i + 2] = y.z;
              if (4 * i + 3 < R) ot[4 * i + 3] = y.w;
              if constexpr (MPLANE) {
                const uint4 z = pmmv[i];
                mm[4 * i] = z.x;
                if (4 * i + 1 < R) mm[4 * i + 1] = z.y;
                if (4 * i + 2 < R) mm[4 * i + 2] = z.z;
                if (4 * i + 3 < R) mm[4 * i + 3] = z.w;
              }
            }
            // the seed is one bit of one row: written into the lane's zero block at its (dynamic) row and read back as the
            // flood's row set - two LDS instructions instead of a select per row (odd rows bit-reversed) -, then cleared again
            {
              const int srw = sr & (int)(0u - ex);
              asm volatile("" ::: "memory");
              blk[srw] = ex << (((uint32_t)scol ^ (0u - ((uint32_t)sr & 1u))) & 31u);   // odd rows: bit 31 - scol
              asm volatile("" ::: "memory");
              const uint4 *pf = reinterpret_cast<const uint4 *>(blk);
#pragma unroll
              for (int i = 0; i < RV; ++i) {
                const uint4 x = pf[i];
                ft[4 * i] = x.x; ft[4 * i + 1] = x.y; ft[4 * i + 2] = x.z; ft[4 * i + 3] = x.w;
              }
              asm volatile("" ::: "memory");
              blk[srw] = 0u;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
              m[r] = mt[r];
              mrev[r] = __brev(m[r]);
              f[r] = ft[r];
              res[r] = 0u;
              // (-DGG_AB_EMPTY1=1, 19x19: ot[] has no use inside flood_jobs but the liberties' empty rows - formed here, once per batch)
              if constexpr (GG_AB_EMPTY1 != 0 && R == 19) ot[r] = B3(ot[r], m[r], FULLROW, ~(TA | TB) & TC & 0xFF);
            }
          }
#ifdef GG_AB_MCHECK
          if constexpr (MPLANE) {   // (A/B builds only: the plane's rows against the registers', gg_v5.h: gg_mcheck)
            uint32_t bad_ = 0;
#pragma unroll
            for (int i = 0; i < R; ++i) {
              const uint32_t want_ = (uint32_t)__builtin_amdgcn_ds_bpermute(8 * sj + (i < RPL ? 0 : 4), (int)M[i < RPL ? i : i - RPL]);
              bad_ += (have && want_ != mm[i]) ? 1u : 0u;
            }
            if (bad_) atomicAdd(&gg_mcheck[0], (unsigned long long)bad_);
            if (have) atomicAdd(&gg_mcheck[1], (unsigned long long)R);
          }
#endif
          GG_PROF(1);
          // Which floods must reach their fixed point inside the batch's loop?  (Its length is the longest of its floods: 4.21
          // sweeps per batch when all 1.56 floods per board count, 3.87 when only G's 0.6 per board do, 3.00 with the weak
          // closure below and a first test after three sweeps, tools/exp/r5_sweeps.py: 1.445 -> 1.415 -> 1.349 ms per launch of
          // 65 536 games x 256 plies; flood_first_test<R>() in gg_v5.h says after which sweep the first test comes today.)
          //  * An OPPONENT group never: cut short, the part found so far either has two liberties - liberties of the whole
          //    group, which keeps its class: phase 3 never sees it - or fewer, and then the group may be captured or leave M
          //    and its full extent matters: the lane is unsettled and the loop goes on for it (groups with < 2 liberties are small).
          //  * The mover's group G only as far as its stones OUTSIDE M go: with two liberties found G joins M whole, and what the
          //    cut-short flood has not reached of it are stones of groups that were in M already (a group in atari that q
          //    connects hangs on q itself, stone by stone outside M: the weak closure holds it whole); with fewer, as above.
          // 19x19: while a lane is unsettled the loop goes on IN PLACE, one sweep and its test at a time (flood_jobs): no
          // restart from a re-encoded fill, the liberties taken once per test.
          // (the two-chain flood2_dual: 1.758 against 1.579 ms per launch - one more sweep-equivalent, as in k_rollout4)
          // the wave's priority falls HERE, in front of the dependent VALU chain it was introduced for, and not in front of the job loop:
          // the set-up above is LDS round trips (round 17: +1.2 % on the headline launch alone, and what makes the shorter flood pay; -DGG_AB_PRIO=0 in A/B builds for the old place)
          if (GG_AB_PRIO && plies >= 8) { if (lead) __builtin_amdgcn_s_setprio(0); else __builtin_amdgcn_s_setprio(1); }
          if constexpr (R == 19) {
            cnt = flood_jobs<R>(m, mrev, f, res, ot, mm, isG != 0u, have);
            GG_PROF(2);   // (with the liberties, which the loop takes after its tests)
          } else {
            // (9x9, 13x13: the restart form - first test after three sweeps, unsettled lanes flood on from the re-encoded fill)
            uint32_t open = 0;
            flood_jobs_restart<R, true>(m, mrev, f, res, isG != 0u, mm, open);
            GG_PROF(2);
            cnt = job_liberties<R>(res, ot, m);
            const bool unsettled = have && open != 0u && cnt < 2u;
            if (GG_BALLOT5(unsettled)) {
#pragma unroll
              for (int r = 0; r < R; ++r) f[r] = (r & 1) ? __brev(res[r]) : res[r];
              flood_jobs_restart<R, false>(m, mrev, f, res, unsettled, mm, open);
              cnt = job_liberties<R>(res, ot, m);
            }
          }
        }
        // (A/B builds with -DGG_AB_PRIO_HAND=1 raise the wave's priority HERE, behind the flood and its liberties, and not behind the
        // job loop: what follows is LDS traffic and a wave-wide wait, like the set-up.  Not shipped - docs/history/r19.md.)
        if (GG_AB_PRIO_HAND && plies >= 8) { if (lead) __builtin_amdgcn_s_setprio(2); else __builtin_amdgcn_s_setprio(3); }
        const uint32_t lib2 = cnt < 2u ? cnt : 2u;
        // G goes to its board's G block (over the stone phase 1 left there); an opponent group with no liberty left
        // (captured) or with one (it leaves M) is ORed into the board's collection block - one that keeps >= 2 is dropped
        uint32_t *gb = DESC ? gblk + 2 * GG_SJR : gblk + 2 * sj * RS;
#undef GG_SJR
#if GG_AB_HAND1
        // ONE path for both: a lane that hands a group over ORs its rows into the block its address chooses, gb for G, gb + RS for a
        // collected opponent group, and one word into the board's info word.  The OR is exact for G too: phase 1 cleared both blocks
        // of every board this ply and left only q in the G block, the flood of G starts at q (q is in res[]), a board has at most
        // one G job, and every job's fill stays inside the rows of its own colour - so the G block ends as res[], as the plain
        // store left it, and rows R .. RS - 1 stay zero.
        // (two rows per ds_or_b64: the blocks and RS are even, and for odd R the last pair ORs zero into row R, inside the block;
        // half the LDS instructions of nineteen ds_or_b32 - skipping empty rows by a per-row branch instead cost 4 %)
        static_assert(Lds5<R>::kG % 2 == 0 && RS % 2 == 0 && R + 1 <= RS, "8-byte aligned row pairs inside the block");
        // (-DGG_AB_FLAT1=1, 19x19: 13x13 and 9x9 stand two VGPRs below what their three and four waves per SIMD allow, and the words
        // formed in front of the region are live beside all of res[])
        constexpr bool HAND_FLAT = GG_AB_FLAT1 != 0 && R == 19;
        if constexpr (HAND_FLAT) {
          // the block's offset and the info word are formed by selects IN FRONT of the region (kept there by the empty asm), so that
          // the hand-over is the one exec region round 19 meant and not the halves of a branch on isG around it
          // G: its liberties; an opponent group: the direction in which it was captured (a zero word is ORed, not branched around)
          // (value and shift are selected, then shifted once: a select between the two shifted words compiles to a branch on isG)
          uint32_t off = isG ? 0u : (uint32_t)RS;
          const uint32_t wv = isG ? lib2 : (cnt == 0u ? 1u : 0u), wsh = isG ? 4u : ((d >> 19) & 3u);
          uint32_t word = wv << wsh;
          uint32_t sji = (uint32_t)sj;   // (the info word's index on its own: not re-derived from the block's address)
          asm volatile("" : "+v"(off), "+v"(word), "+v"(sji));
          if (isG || (have && cnt < 2u)) {
            uint32_t *dst = gb + off;
#pragma unroll
            for (int r = 0; r < R; r += 2) {
              const uint32_t hi = r + 1 < R ? res[r + 1] : 0u;
              atomicOr(reinterpret_cast<unsigned long long *>(dst + r), ((unsigned long long)hi << 32) | res[r]);
            }
            atomicOr(clsv + sji, word);
          }
        } else if (isG || (have && cnt < 2u)) {
          uint32_t *dst = gb + (isG ? 0 : RS);
#pragma unroll
          for (int r = 0; r < R; r += 2) {
            const uint32_t hi = r + 1 < R ? res[r + 1] : 0u;
            atomicOr(reinterpret_cast<unsigned long long *>(dst + r), ((unsigned long long)hi << 32) | res[r]);
          }
          // G: its liberties; an opponent group: the direction in which it was captured (a zero word is ORed, not branched around)
          const uint32_t word = isG ? lib2 << 4 : (cnt == 0u ? 1u << ((d >> 19) & 3u) : 0u);
          atomicOr(clsv + sj, word);
        }
#else
        if (isG) {
          uint4 *pz = reinterpret_cast<uint4 *>(gb);
#pragma unroll
          for (int i = 0; i < RV; ++i)
            pz[i] = make_uint4(res[4 * i], 4 * i + 1 < R ? res[4 * i + 1] : 0u, 4 * i + 2 < R ? res[4 * i + 2] : 0u, 4 * i + 3 < R ? res[4 * i + 3] : 0u);
          if (lib2) atomicOr(clsv + sj, lib2 << 4);
        } else if (have && cnt < 2u) {
          // (two rows per ds_or_b64: the blocks and RS are even, and for odd R the last pair ORs zero into row R, inside the
          // block; half the LDS instructions of nineteen ds_or_b32 - skipping empty rows by a per-row branch instead cost 4 %)
          static_assert(Lds5<R>::kG % 2 == 0 && RS % 2 == 0 && R + 1 <= RS, "8-byte aligned row pairs inside the block");
#pragma unroll
          for (int r = 0; r < R; r += 2) {
            const uint32_t hi = r + 1 < R ? res[r + 1] : 0u;
            atomicOr(reinterpret_cast<unsigned long long *>(gb + RS + r), ((unsigned long long)hi << 32) | res[r]);
          }
          if (cnt == 0u) atomicOr(clsv + sj, 1u << ((d >> 19) & 3u));
        }
#endif
      }
      // (-DGG_AB_PRIO_HAND=1: the priority is lowered and raised inside the loop body, a ply without a job never lowers it - nothing to raise)
      if (!(GG_AB_PRIO && GG_AB_PRIO_HAND) && plies >= 8) { if (lead) __builtin_amdgcn_s_setprio(2); else __builtin_amdgcn_s_setprio(3); }
      WAVE_SYNC();
      GG_PROF(3);

      // phase 3 - all thirty-two boards in ONE pass, RPL adjacent rows per lane: patch the classes, resolve captures and
      // ko, the next mover's mask (k_rollout4's phase 3 on pairs; A = this lane's two directions, B = its partner's)
      {
        const int a = a_q;
        const uint32_t fl = fl_q;
        const uint32_t info = *GG_CLS;
        const int turn0 = fl & 1u;
        uint32_t *pmine = GG_PM(turn0) + r0;
        uint32_t *popp = GG_PO(turn0) + r0;
        const uint32_t *gG = GG_GB + r0;   // the board's G block, behind it the collected opponent groups
        uint32_t mine1[RPL], opp0[RPL], all4[RPL], bg[RPL];
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
          mine1[r] = pmine[r];   // (rows >= N are zero)
          opp0[r] = popp[r];
          bg[r] = gG[r];
          all4[r] = gG[RS + r];
        }
        const bool moves_now = a >= 0;
        const bool is_pass = a == P;
        int ar, ac;
#if GG_AB_MOVE_RC
        ar = (int)(rc_q >> 5);
        ac = (int)(rc_q & 31u);                                // (zero for a pass, some point for an idle board: masked below)
#else
        split_action(a, N, inv, ar, ac);                       // (garbage for a pass / an idle board: masked below)
#endif
        const uint32_t capt_m = info & 15u;   // the directions in which an opponent group died (never set on a board that does not move)
        // The collection block holds the opponent groups next to q with NO liberty left (captured: q was their only liberty, so
        // they were never in M) or with exactly ONE (they had q and one more: they were in M).  So it splits by M alone:
        // captured = all4 & ~M, leaving M = all4 & M.  (all4 holds opponent stones only.)
#if GG_AB_MINPLACE1
        uint32_t fj[RPL];
#endif
        uint32_t g0[RPL], opp1[RPL];
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
#if GG_AB_MINPLACE1
          fj[r] = 0u;
#endif
          g0[r] = bg[r];   // the G block: the flood of G, the stone alone as phase 1 left it there, or nothing (pass / idle board)
          opp1[r] = B3(opp0[r], all4[r], M[r], TA & ~(TB & ~TC) & 0xFF);   // opp0 & ~cap: the opponent's stones after the captures
        }
        // liberties of G among the empty points (saturated at 2): G's own count, or the empty neighbours of q when the
        // stone stands alone
        const uint32_t ne = qs & 7u, ne2 = ne < 2u ? ne : 2u;
        uint32_t libsG = ((qs >> 11) & 1u) ? ((info >> 4) & 3u) : ne2;
        uint32_t ko_oh = 0, ko_bit = 0;   // the ko point: one-hot row of this lane / column bit (almost always none)
        GG_P3(0, 1u);
        GG_P3(8, (uint32_t)__popcll(GG_BALLOT5(capt_m != 0u && t5 == 0)));
        GG_P3(9, (uint32_t)__popcll(GG_BALLOT5(a >= 0 && t5 == 0)));
        // (-DGG_AB_MINPLACE1=1, 19x19) the atari-join does not touch M: its fill - the seeds when no trip is run, all zero on a wave-ply
        // without a capture - is a row set of its own that the mask rule ORs in, so that M is the same registers on every path to the rule
        constexpr bool MINPL = GG_AB_MINPLACE1 != 0 && R == 19;
        GG_MARK(10);
        if (GG_BALLOT5(capt_m != 0u)) {   // a capture on some board of the wave
          GG_MARK(11);
          GG_P3(1, 1u);
          uint32_t cap[RPL];   // the captured stones
#pragma unroll
          for (int r = 0; r < RPL; ++r) cap[r] = B3(all4[r], M[r], M[r], TA & ~TB & 0xFF);
          const uint32_t ncapn = (uint32_t)__popc(capt_m);        // captured neighbours of q
          constexpr bool CMP3 = GG_AB_BALLOT1 != 0 && R == 19;   // (ncapn == 1 && libsG == 0 as one compare)
          const bool one0 = CMP3 ? B3(ncapn, 1u, libsG, (TA ^ TB) | TC) == 0u : (ncapn == 1u && libsG == 0u);
          if (GG_BALLOT5(one0)) {
            GG_MARK(12);
            GG_P3(2, 1u);
            uint32_t dg[RPL];
            dilate_rows<RPL>(g0, dg);
            uint32_t cntc = 0;
#pragma unroll
            for (int r = 0; r < RPL; ++r) cntc += (uint32_t)__popc(dg[r] & cap[r]);
            const uint32_t c2 = cntc < 2u ? cntc : 2u;
            const uint32_t tot = c2 + dpp0<QP_X1>(c2);
            libsG += one0 ? (tot < 2u ? tot : 2u) : ncapn;
            GG_MARK(13);
          } else {
            libsG += ncapn;
          }
          // gogame.py:72-75: ko iff exactly one stone died and the new stone is boxed in (one captured NEIGHBOUR and a boxed-in
          // stone first: rare enough to keep the rest off the usual path)
          // (CMP3: ncapn == 1 && !(qs & CL_OPEN) as one compare)
          const bool ko1 = CMP3 ? B3(ncapn, 1u, qs & CL_OPEN, (TA ^ TB) | TC) == 0u : (ncapn == 1u && !(qs & CL_OPEN));
          if (GG_BALLOT5(ko1)) {
            GG_MARK(14);
            GG_P3(3, 1u);
            uint32_t died = 0;   // captured stones on this lane's rows (one captured neighbour: exactly one stone died iff its group is that stone)
#pragma unroll
            for (int r = 0; r < RPL; ++r) died += (uint32_t)__popc(cap[r]);
            const bool ko = ko1 && died + dpp0<QP_X1>(died) == 1u;
            // the one captured stone is q's neighbour in the direction of its job (bit 0 up, 1 down, 2 left, 3 right)
            const uint32_t kr = (uint32_t)ar - (capt_m & 1u) + ((capt_m >> 1) & 1u) - (uint32_t)r0;
            ko_oh = (ko && kr < (uint32_t)RPL) ? (1u << (kr & 31)) : 0u;
            ko_bit = 1u << (((uint32_t)ac - ((capt_m >> 2) & 1u) + (capt_m >> 3)) & 31u);
            GG_MARK(15);
          }
          GG_MARK(16);
          // the mover's groups in atari next to a captured stone (and not merged into G) now have >= 2 liberties: they join M
          // before the classes are patched.  The seeds are the stones of such groups next to a captured stone (zero on a board
          // without a capture: its cap is empty); the fill grows them inside `atari` by one-step dilation, Gauss-Seidel in
          // the lane (a row sees the row swept just before it as already grown; the partner lane's seam row as it was at the
          // start of the trip), down and up in turn, until a trip adds nothing.  The fixed point is the union of the atari
          // groups the seeds touch whatever the order.  The wave still runs as many trips as its slowest board needs, but
          // fewer than with the Jacobi dilation of round 7 (2.40 against 2.87 per wave-ply that enters the loop, 47 % of
          // them), at 6 instead of 7 VALU per row and trip (profiles/r08_p3_counts.txt).
          uint32_t atari[RPL], f[RPL], anyf = 0;
          constexpr bool SHL_FIRST = GG_AB_SHL1 != 0 && R == 19;
          {
            const uint32_t up = dpp0<0x138>(cap[RPL - 1]), dn = dpp0<0x130>(cap[0]);
            // (-DGG_AB_SHL1=1, 19x19: the adds of all rows first - an inline-asm add directly in front of the v_bitop3 that takes its
            // result is padded with an s_nop 0 by the compiler: by the listing none here, nine in each of the two trips below)
            uint32_t cl[RPL];
            if constexpr (SHL_FIRST) {
#pragma unroll
              for (int r = 0; r < RPL; ++r) cl[r] = shl1(cap[r]);
              __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int r = 0; r < RPL; ++r) {
              atari[r] = B3(mine1[r], M[r], g0[r], TA & ~(TB | TC) & 0xFF);   // mine & ~M & ~G
              const uint32_t above = r == 0 ? up : cap[r - 1], below = r == RPL - 1 ? dn : cap[r + 1];
              const uint32_t v = B3(cap[r] >> 1, above, below, T_OR3);
              f[r] = B3(SHL_FIRST ? cl[r] : shl1(cap[r]), v, atari[r], (TA | TB) & TC);           // dilate(cap) & atari
              anyf |= f[r];
            }
          }
          GG_MARK(17);
          if (GG_BALLOT5(anyf != 0u)) {
            GG_MARK(18);
            GG_P3(5, 1u);
#ifdef GG_AB_P3
            uint32_t trips_ = 0;
#define GG_TRIP ++trips_
#else
#define GG_TRIP do {} while (0)
#endif
            // one trip over the lane's rows in order R0, R0 + D, ..: a row grows from its (already grown) predecessor, its old
            // successor and itself; chg collects the bits a trip adds
#define GG_JOIN_TRIP(R0, D)                                                                                               \
            do {                                                                                                          \
              GG_TRIP;                                                                                                    \
              const uint32_t up_ = dpp0<0x138>(f[RPL - 1]), dn_ = dpp0<0x130>(f[0]);                                      \
              chg = 0;                                                                                                    \
              uint32_t fl_[RPL];   /* (SHL_FIRST: a row is shifted as the trip found it - its own visit is its first change) */ \
              if constexpr (SHL_FIRST) {                                                                                  \
                _Pragma("unroll") for (int i_ = 0; i_ < RPL; ++i_) fl_[i_] = shl1(f[i_]);                                 \
                __builtin_amdgcn_sched_barrier(0);                                                                        \
              }                                                                                                           \
              _Pragma("unroll") for (int i_ = 0; i_ < RPL; ++i_) {                                                        \
                const int r_ = (R0) + (D) * i_;                                                                           \
                const uint32_t above_ = r_ == 0 ? up_ : f[r_ == 0 ? 0 : r_ - 1];                                          \
                const uint32_t below_ = r_ == RPL - 1 ? dn_ : f[r_ == RPL - 1 ? 0 : r_ + 1];                              \
                const uint32_t v_ = B3(f[r_] >> 1, above_, below_, T_OR3);                                              \
                const uint32_t g_ = B3(SHL_FIRST ? fl_[r_] : shl1(f[r_]), v_, atari[r_], (TA | TB) & TC);                \
                chg = B3(g_, f[r_], chg, (TA & ~TB & 0xFF) | TC);                                                         \
                f[r_] |= g_;                                                                                              \
              }                                                                                                           \
            } while (0)
            uint32_t chg;
#pragma unroll 1
            for (int it = 0; it < R * R; ++it) {
              GG_JOIN_TRIP(0, 1);
              if (GG_BALLOT5(chg != 0u) == 0) break;
              GG_JOIN_TRIP(RPL - 1, -1);
              if (GG_BALLOT5(chg != 0u) == 0) break;
            }
#undef GG_JOIN_TRIP
#undef GG_TRIP
#ifdef GG_AB_P3
            GG_P3(6, trips_);
            p3c_[7] = trips_ > p3c_[7] ? trips_ : p3c_[7];
#endif
            if constexpr (!MINPL) {
#pragma unroll
              for (int r = 0; r < RPL; ++r) M[r] |= f[r];
            }
            GG_MARK(19);
          }
#if GG_AB_MINPLACE1
          if constexpr (MINPL) {   // (the fill as the join left it - the seeds when no trip was run - is what the mask rule ORs in)
#pragma unroll
            for (int r = 0; r < RPL; ++r) fj[r] = f[r];
          }
#endif
        }
        GG_MARK(20);
        // The mask rule.  The new M: the stones of M outside G and the collected groups (those left with one liberty leave M; a
        // captured group was never in it), and G if it has two liberties - (M & ~G & ~all4) | (gsel & G); it is the old rule's
        // (M & mine & ~G) | (gsel & G) | (M & opp & ~all4), as M holds stones only and all4 opponent stones only.  A point is
        // a legal move for the next player iff it is empty and has a neighbour in x: an empty point, a stone of the mover
        // outside the new M (in atari: placing there captures) or an opponent stone in it (a group it joins keeps a liberty):
        // x = full & ~(new M ? mine : opp).  Six v_bitop3 per row and the dilation (the old chain: nine).  Equal to the old
        // chain in every bit case these invariants admit (20 of 128), and they hold from ply to ply: M holds stones only (the load
        // takes it from the analysis' class planes, a reset clears it, each ply keeps a subset of M | G | the atari-join's mover
        // stones, and a captured stone was never in M); all4 holds opponent stones only and G mover stones only (phase 1 clears
        // both blocks, the jobs OR in fills inside their own colour's rows); every set lies inside `full` (rows and columns
        // >= N of the planes are zero).
        const uint32_t gsel = libsG >= 2u ? ~0u : 0u;
        uint32_t e[RPL], x[RPL], nbr[RPL];
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
          // (MINPL: (M | fill) & ~all4, then G | u or u & ~G by gsel - the fill lies inside the mover's stones outside M and G, so this is
          // the rule below with M | fill for M, in the same two v_bitop3)
#if GG_AB_MINPLACE1
          const uint32_t u = MINPL ? B3(M[r], fj[r], all4[r], (TA | TB) & ~TC & 0xFF)
                                   : B3(M[r], g0[r], all4[r], TA & ~(TB | TC) & 0xFF);   // M & ~G & ~all4
          M[r] = MINPL ? B3(gsel, g0[r], u, ((TA & TB) | (~TB & TC)) & 0xFF) : B3(gsel, g0[r], u, T_ANDOR);   // the new M
#else
          const uint32_t u = B3(M[r], g0[r], all4[r], TA & ~(TB | TC) & 0xFF);   // M & ~G & ~all4
          M[r] = B3(gsel, g0[r], u, T_ANDOR);                                      // the new M
#endif
          const uint32_t y = B3(M[r], mine1[r], opp1[r], T_SEL);
          x[r] = B3(full[r], y, y, TA & ~TB & 0xFF);
          e[r] = B3(full[r], opp1[r], mine1[r], TA & ~(TB | TC) & 0xFF);
        }
        // (-DGG_AB_VALID1=1, 19x19: the VALID rows, (h3 | dn) & e in two v_bitop3 a row - e lies inside full[] -, nbr[] holds them;
        //  -DGG_AB_ALLMOVE1=1, 19x19: every lane's board moves - any full wave of live games - and the new rows are assigned; absent slots
        //  of a short wave and frozen boards send the wave through the select)
        constexpr bool AMOVE = GG_AB_ALLMOVE1 != 0 && R == 19;
        if constexpr (VAL) {
          const uint32_t up = dpp0<0x138>(x[RPL - 1]), dn = dpp0<0x130>(x[0]);
#pragma unroll
          for (int r = 0; r < RPL; ++r) {
            const uint32_t above = r == 0 ? up : x[r - 1], below = r == RPL - 1 ? dn : x[r + 1];
            nbr[r] = B3(B3(shl1(x[r]), x[r] >> 1, above, T_OR3), below, e[r], (TA | TB) & TC);
          }
        } else {
          dilate_rows<RPL>(x, nbr);
        }
        const uint32_t mv_m = moves_now ? ~0u : 0u;
        if (AMOVE && GG_BALLOT5(!moves_now) == 0) {
#pragma unroll
          for (int r = 0; r < RPL; ++r) {
            if constexpr (VAL) val_r[r] = nbr[r];
            else inv_r[r] = B3(e[r], nbr[r], full[r], ~(TA & TB) & TC & 0xFF);
          }
        } else {
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
          const uint32_t invalid = VAL ? nbr[r] : B3(e[r], nbr[r], full[r], ~(TA & TB) & TC & 0xFF);
          inv_r[r] = B3(mv_m, invalid, inv_r[r], T_SEL);
        }
        }
        if (GG_BALLOT5(ko_oh != 0u)) {   // (only a board that moved has a ko point)
#pragma unroll
          for (int r = 0; r < RPL; ++r) {
            if constexpr (VAL) val_r[r] &= ~((uint32_t)__builtin_amdgcn_sbfe((int)ko_oh, r, 1) & ko_bit);
            else inv_r[r] |= (uint32_t)__builtin_amdgcn_sbfe((int)ko_oh, r, 1) & ko_bit;
          }
        }
        if (capt_m) {
#pragma unroll
          for (int r = 0; r < RPL; ++r) popp[r] = opp1[r];
        }
        if constexpr (MPLANE) {
          // the new M into its plane for the job lanes of the next ply: no exec region, every lane stores its rows (a board that does
          // not move rewrites what is there; the odd lane's last row is row N of the board and zero)
          uint2 *pm2 = reinterpret_cast<uint2 *>(mplv + s4 * RS + r0);
#pragma unroll
          for (int r = 0; r < RPL; r += 2) pm2[r / 2] = make_uint2(M[r], M[r + 1]);
        }
        // (a board being reset found fl_q = on | dirty | black to move in phase 1: the register copy follows even if it does not move)
        if constexpr (GG_AB_FLAT1 != 0 && R == 19) {
          // no exec region: the new flag word by a select, and BOTH lanes of the pair store the board's three meta words (they hold
          // the same values) - at the board's own words when it moves, else at the dump words nobody reads (Lds5::kDumpMeta)
          const uint32_t passed0 = (fl >> 1) & 1u, done0 = (fl >> 2) & 1u;
          const uint32_t passed = is_pass ? 1u : 0u, done = done0 | (passed & passed0);
          const uint32_t flm = (uint32_t)(turn0 ^ 1) | (passed << 1) | (done << 2) | 8u | (fl & 32u);
          flr = moves_now ? flm : fl;
          playedr += moves_now ? 1 : 0;
#if GG_AB_LANE1
          uint32_t *mp = KEEP ? (moves_now ? metaK : metaK + (Lds5<R>::kDumpMeta - Lds5<R>::kMeta))
                              : lds + (moves_now ? Lds5<R>::kMeta : Lds5<R>::kDumpMeta) + s4;
#else
          uint32_t *mp = lds + (moves_now ? Lds5<R>::kMeta : Lds5<R>::kDumpMeta) + s4;
#endif
          mp[0] = flr;
          mp[kNB5] = (uint32_t)a;
          mp[2 * kNB5] = (uint32_t)playedr;
        } else {
          flr = fl;
          if (moves_now) {
            const uint32_t passed0 = (fl >> 1) & 1u, done0 = (fl >> 2) & 1u;
            const uint32_t passed = is_pass ? 1u : 0u, done = done0 | (passed & passed0);
            flr = (uint32_t)(turn0 ^ 1) | (passed << 1) | (done << 2) | 8u | (fl & 32u);
            playedr += 1;
            if (t5 == 0) {
              flagsv[s4] = flr;
              lastv[s4] = a;
              playedv[s4] = playedr;
            }
          }
        }
      }
#undef GG_PM
#undef GG_PO
#undef GG_GB
#undef GG_CLS
      WAVE_SYNC();
      GG_PROF(4);
    }
    if (plies >= 8) fair.release();
    GG_PROF(5);
#ifdef GG_AB_P3
    if (ln0 == 0) {
#pragma unroll
      for (int k = 0; k < 10; ++k) {
        if (k == 7) atomicMax(&gg_p3[7], (unsigned long long)p3c_[7]);
        else atomicAdd(&gg_p3[k], (unsigned long long)p3c_[k]);
      }
    }
#endif
#ifdef GG_LIVE_CHECK
    if (playedr != drawsr) atomicAdd(&gg_live_bad, 1ull);
#endif

    // ---------------------------------------------------------------- store
    int lnS;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lnS));
    const int s5s = lnS >> 1, r05s = RPL * (lnS & 1);
    WAVE_SYNC();
    if (TRACKED) {
      // park the register rows, then one flat coalesced copy of the group's contiguous block
#pragma unroll
      for (int r = 0; r < RPL; ++r) {
        if (r05s + r < RS) {
          const uint32_t bk = st[0 * PL + s5s * RS + r05s + r], wh = st[1 * PL + s5s * RS + r05s + r];
          // (VAL: the invalid row again, full & ~valid; row N of the odd lane stays zero, an absent board's words never leave LDS)
          park[0 * PL + s5s * RS + r05s + r] = VAL ? (r05s + r < N ? FULLROW & ~val_r[r] : 0u) : inv_r[r];
          park[1 * PL + s5s * RS + r05s + r] = M[r] & bk;
          park[2 * PL + s5s * RS + r05s + r] = M[r] & wh;
        }
      }
      WAVE_SYNC();
      const int64_t nbrd = (B - b_first) < nb ? (B - b_first) : nb;
      const int nw = (int)nbrd * W;
      uint32_t *gp = reinterpret_cast<uint32_t *>(states) + b_first * (int64_t)W;
      // (untouched boards are not rewritten: one bit per board, read once; four words per lane and round with their LDS reads in
      // flight together - as k_rollout4's write-back: 48 rounds of flag read -> branch -> row read -> store were 10 us of a launch,
      // now 7.5)
      bool tch = false;
      if (lnS < (int)nbrd) tch = playedv[lnS] != 0 || (flagsv[lnS] & 32u);
      const uint64_t tmask = __ballot(tch);
#pragma unroll 1
      for (int i0 = lnS; i0 < nw; i0 += 4 * kWave) {
        uint32_t v[4];
        bool ok[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int i = i0 + k * kWave;
          const int ic = i < nw ? i : 0;
          const int sb = ic / W, w = ic - sb * W;
          ok[k] = i < nw && ((tmask >> sb) & 1ull);
          const int pl = w / N, rw = w - pl * N;   // (w == 5 N: pl == 5, rw == 0)
          const uint32_t *src = pl >= 5 ? flagsv + sb : (pl < 2 ? st + pl * PL + sb * RS + rw : park + (pl - 2) * PL + sb * RS + rw);
          const uint32_t x = *src;
          v[k] = pl >= 5 ? (x & 7u) : x;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (ok[k]) gp[i0 + k * kWave] = v[k];
      }
      if (lnS < nb && b_first + lnS < B) {
        const int sb = lnS;
        const int64_t b = b_first + sb;
        const int played = playedv[sb];
        rng[b] = (((uint64_t)rngv[2 * sb + 1] << 32) | rngv[2 * sb]) + (uint64_t)(uint32_t)played * 0x9E3779B97F4A7C15ull;
        if (last_actions) last_actions[b] = lastv[sb];
        if (steps_done && played) atomicAdd(reinterpret_cast<unsigned long long *>(steps_done) + b, (unsigned long long)played);
      }
      WAVE_SYNC();
    } else {
      // byte planes in place: the whole group in one contiguous write, then the per-game outputs
      const int nbrd = (int)((B - b_first) < nb ? (B - b_first) : nb);
      bool any_wr = false;
      if (lnS < nbrd) any_wr = playedv[lnS] != 0 || (flagsv[lnS] & 32u);
      // (the per-game words are read before the emitter takes the loop area over: the meta words live outside it)
      // (VAL: the emitter takes the invalid rows, full & ~valid, formed once here; it reads rows < N of boards < nbrd only)
      if constexpr (VAL) {
#pragma unroll
        for (int r = 0; r < RPL; ++r) inv_r[r] = FULLROW & ~val_r[r];
      }
      if (__ballot(any_wr))
        emit_group<R, RPL, 2>(states + b_first * (int64_t)S, nbrd, N, st, PL, RS, inv_r, flagsv, lds + Lds5<R>::kGrpBits,
                              reinterpret_cast<uint2 *>(lds + Lds5<R>::kGrpLut), lnS);
      if (lnS < nbrd) {
        const int sb = lnS;
        const int64_t b = b_first + sb;
        const int played = playedv[sb];
        rng[b] = (((uint64_t)rngv[2 * sb + 1] << 32) | rngv[2 * sb]) + (uint64_t)(uint32_t)played * 0x9E3779B97F4A7C15ull;
        if (last_actions) last_actions[b] = lastv[sb];
        if (steps_done && played) atomicAdd(reinterpret_cast<unsigned long long *>(steps_done) + b, (unsigned long long)played);
      }
      WAVE_SYNC();
      if (ws) {
        // the workspace entries of the boards whose bytes were written and of those analysed at load (any other board's entry
        // already holds exactly this): stones out of the planes, M & stones parked behind them (the emitter is done with the
        // loop area), then one flat coalesced copy of the four row sets as the tracked store above does it
        const uint64_t wmask = __ballot(lnS < nbrd && (any_wr || ((wsmiss >> (lnS & 31)) & 1u)));
        if (wmask) {
#pragma unroll
          for (int r = 0; r < RPL; ++r) {
            if (r05s + r < RS) {
              const uint32_t bk = st[0 * PL + s5s * RS + r05s + r], wh = st[1 * PL + s5s * RS + r05s + r];
              park[0 * PL + s5s * RS + r05s + r] = M[r] & bk;
              park[1 * PL + s5s * RS + r05s + r] = M[r] & wh;
            }
          }
          WAVE_SYNC();
          uint32_t *wg = ws + b_first * (int64_t)W;
          const int nw4 = nbrd * 4 * N;
#pragma unroll 1
          for (int i0 = lnS; i0 < nw4; i0 += 4 * kWave) {
            uint32_t v[4];
            int at[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int i = i0 + k * kWave;
              const int ic = i < nw4 ? i : 0;
              const int sb = ic / (4 * N), w = ic - sb * (4 * N);
              const int pl = w / N, rw = w - pl * N;
              v[k] = pl < 2 ? st[pl * PL + sb * RS + rw] : park[(pl - 2) * PL + sb * RS + rw];
              at[k] = (i < nw4 && ((wmask >> sb) & 1ull)) ? sb * W + (pl < 2 ? w : w + N) : -1;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (at[k] >= 0) wg[at[k]] = v[k];
          }
          WAVE_SYNC();
        }
      }
    }
    GG_WSC_FLUSH;
    GG_PROF(7);   // write-back
    GG_PROF_FLUSH;
  }
}
#undef GG_R5_LOG_PARAM
#undef val_r
