// bs_sweep.h -- what the clean outlines (bs_uncross.hip) and their sweep detection (bs_sweep.hip) share: the words of the
// detection that the host reads, the scratch of bs_ctx::sw, and the two host calls of one detection's sweep pass.
#pragma once

#include "bs_common.h"

namespace bs {

// the words of bs_ctx::uc[UC_MISC] (ints).  W_S_LENS .. W_S_CAND_HI are zeroed by every sweep_begin; W_S_MAXW lives as long as
// the count.
enum { W_ERR, W_MARKED, W_MAXCELL, W_CHANGED, W_S_MAXW, W_S_LENS, W_S_ITEMS_T, W_S_SWEEPING, W_S_ONLY, W_S_PAIRS, W_S_EXACT,
       W_S_WAVE, W_S_REJECT, W_S_CAND_LO, W_S_CAND_HI, W_COUNT };

// scratch of bs_ctx::sw
enum { SW_BITS, SW_SMARK, SW_ICNT, SW_IOFF, SW_ITEM, SW_CCNT, SW_COFF, SW_TMP, SW_COUNT };
static_assert(SW_COUNT <= (int)(sizeof(bs_ctx::sw) / sizeof(DevBuf)), "bs_ctx::sw is too short");

constexpr int SWEEP_WAVE_CAP = BS_SWEEP_WAVE_CAP;  // a path of more runs is tested by a wave, not by a thread
constexpr unsigned F_SWEEPING = 16;                // bit 4 of s_flag
constexpr uint8_t SM_SWEEPING = 1, SM_ONLY = 2;    // smark: sweeping; sweeping and not conflicting

struct SweepRun {  // one detection, as bs_uncross.hip has it
  hipStream_t st;
  const int2* segK;  // seg.x == -1: kept
  const int32_t *kscan, *klist;
  const int2* xy;
  const int32_t *ring, *noff;
  int32_t N, nr, width, height;
  int* d_words;
  int mode;
};

// Before the detection's first wait (after the kept scan and list): the corner bitmap, the items every node's run gives and
// their exclusive sum.  *h_items receives the item count with the stream's next synchronisation.
int sweep_begin(bs_ctx* ctx, const SweepRun& R, long long* h_items);
// After the pair tests: the items, the candidate corners and the exact tests.  smark [nseg] is written for every segment
// (SM_SWEEPING, SM_ONLY); in mode 2 the sweeping segments are also set in mark.  Counts go into d_words.
int sweep_detect(bs_ctx* ctx, const SweepRun& R, int32_t nseg, long long n_items, uint8_t* mark);
inline uint8_t* sweep_marks(bs_ctx* ctx) { return ctx->sw[SW_SMARK].as<uint8_t>(); }

}  // namespace bs
