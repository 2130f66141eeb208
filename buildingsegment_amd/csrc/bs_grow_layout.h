// bs_grow_layout.h -- sizes and scratch layout of the speculative grower's host loop (bs_grow_spec.hip).
// Host-only, plain C++17 without a HIP include: tests/cpp/grow_layout_check.cpp compiles it alone.
//
// GrowLayout walks one carver per carved slot of the context (rg_aux, rg_disp, rg_hout, rg_geo): the bytes to reserve and
// the pointers come from the same walk.  A buffer that serves a second purpose for a while is an *_in_* accessor.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/bs_api.h"

namespace bs {

constexpr int MAX_WAVES = 1 << 18;  // upper bound of plane attempts grown per round (the 50 M cloud has 158 k candidates in round 1)
constexpr int MAX_PENDING = 32768;  // finished planes waiting for earlier attempts
constexpr int TILE1 = 12, TILE2 = 16;  // tiles of the dispatch order, log2 positions (see tile_min_kernel)
constexpr int PULL_GROUP = 16;         // owner passes per host round trip (BS_OWNER_GROUP only lowers it)

struct GrowSizes {
  int64_t n, list_cap, planes_cap, pstore_cap, pstore_lim;
  int wave_cap, max_waves, pend_lim, KC, quads;
  unsigned long long pool_cap, pool_cap_eff;
  size_t nb256, nt1, nt2;
  // max_waves_req: MAX_WAVES, BS_MAX_WAVES or the limits hook's value (GrowConfig); lim: bs_selftest_grow_limits
  GrowSizes(int64_t n_, int K, int th_point_count, int64_t max_waves_req, const bs_grow_limits& lim) : n(n_)
  {
    list_cap = 2 * n + 64;
    planes_cap = n / std::max(1, th_point_count) + 64;
    // Plane attempts per round: ALL candidates.  A round is a barrier bounded by its longest plane, and the big
    // planes of a large scene are independent of each other -- but their seeds are spread over the whole index
    // range: with the lowest 32 768 candidates per round (round 1) the 50 M cloud grew its 136 k-, 131 k- and
    // 122 k-entry planes one round AFTER the 80 k-entry one although nothing connected them (39 k + 68 k + 35 k
    // sequential steps; a cap of 65 536 was worse still: 68 k + 66 k + 35 k).  The ~90 % of the attempts that fail
    // at depth 0 cost one step and 1.5 KB of pool each.  (Bounded at 2^18: with 655 k attempts on the 200 M scene the
    // round pool outgrew 16 GB and the FIRST call on a fresh context took 3 s longer; 2^18 keeps the pool at 12 GB.)
    wave_cap = (int)std::max<int64_t>(1, std::min<int64_t>(MAX_WAVES, n / 8 + 64));  // sizes the per-attempt arrays
    max_waves = (int)std::max<int64_t>(1, std::min<int64_t>(max_waves_req, wave_cap));
    // round pool: lists + stacks + logs of every concurrent attempt
    // (sized for wave_cap attempts, not for max_waves: the audit replays wave_cap attempts per batch whatever BS_MAX_WAVES
    // or bs_selftest_grow_limits say -- on a pool sized for the lowered number its replays ended ST_NOMEM and the audit
    // failed with "no progress" on a correct result; without a lowered max_waves the two are the same number)
    pool_cap = (unsigned long long)std::max<int64_t>(std::min<int64_t>(64 * n, (int64_t)3 << 30),
                                                     8 * n + (int64_t)(2 * 256 + 32 * 32) * 2 * wave_cap);
    // (a lowered pool: the buffer keeps its size, the attempts are told a smaller one)
    pool_cap_eff = lim.pool_cap > 0 ? std::min<unsigned long long>(pool_cap, (unsigned long long)lim.pool_cap) : pool_cap;
    // persistent store for planes that finished consistently but cannot be finalised yet (an earlier attempt is
    // still open): kept across rounds and re-validated instead of being re-grown
    pstore_cap = 6 * n + 65536;
    pstore_lim = lim.pstore_cap > 0 ? std::min<int64_t>(pstore_cap, lim.pstore_cap) : pstore_cap;
    pend_lim = lim.max_pending > 0 ? (int)std::min<int64_t>(MAX_PENDING, lim.max_pending) : MAX_PENDING;
    nb256 = (size_t)((n + 255) / 256);
    nt1 = (size_t)(n >> TILE1) + 2;
    nt2 = (size_t)(n >> TILE2) + 2;
    KC = K <= 16 ? 16 : 32;
    quads = 4 + KC / 4;
  }
};

// ---- small device and host scalars --------------------------------------------------------------------------
// A nested struct is a sub-block a kernel indexes from its first word: the static_asserts pin what the kernels use.
struct CandCount {  // cand_flag_kernel; the host reads both with one copy
  int32_t listed, lowest;
};
struct RefusalStats {  // validate1_kernel / validate3_kernel index it as rejects[0..11]; forge_kernel gets &forged_seed1
  int32_t refused, forged_seed1, forged_refused, unused[5];
  int32_t v1_robbed, v1_tag, v1_dup, v3_state;  // refusals by check
};
struct AuditStats {  // audit_compare_kernel: stats[0], stats[1]
  int32_t mismatches, committed_met;
};
static_assert(offsetof(CandCount, lowest) == 4 && offsetof(AuditStats, committed_met) == 4, "kernel indices");
static_assert(offsetof(RefusalStats, forged_seed1) == 4 && offsetof(RefusalStats, forged_refused) == 8 &&
                  offsetof(RefusalStats, v1_robbed) == 32 && offsetof(RefusalStats, v1_tag) == 36 &&
                  offsetof(RefusalStats, v1_dup) == 40 && offsetof(RefusalStats, v3_state) == 44 && sizeof(RefusalStats) == 48,
              "kernel indices");

struct MiscBlock {  // head of rg_aux
  CandCount cand;
  int32_t verify_bad;  // BS_VERIFY: verify_fixpoint_kernel / verify_records_kernel
  int32_t n_for_host;  // attempts of a big round that travel to the host (DeviceSelect)
  RefusalStats rej;    // zeroed once per call, read once at its end
  AuditStats audit;
  alignas(8) unsigned long long pool_top;      // Pool.top of the round pool
  alignas(128) int32_t flip[PULL_GROUP];       // flips of the passes of one group, one word per pass (decide passes too)
  alignas(128) int32_t wl_cnt[3];              // three worklist lengths, see wl_flush
  alignas(128) int32_t pstat[4 * PULL_GROUP];  // BS_DEBUG: four statistics per pass of a group, see pull_stats
};
struct HostFlags {  // page-locked tail of rg_hout: small scalars copied back per pass / round
  CandCount next_cand;  // after a round: the next round's list and the lowest candidate under the new owners
  int32_t refused, ncand;  // RefusalStats.refused so far; a candidate listing on its own
  AuditStats audit;
  int32_t n_for_host, decided_any;  // decided_any: last decide pass of a group
  int32_t flip[PULL_GROUP];
};

// ---- the carver and the four slots --------------------------------------------------------------------------
struct Carver {
  uintptr_t base;
  size_t top = 0;
  template <class T>
  T* take(size_t count, size_t align = alignof(T))
  {
    top = (top + align - 1) / align * align;
    T* const p = reinterpret_cast<T*>(base + top);
    top += sizeof(T) * count;
    return p;
  }
};

// PlaneOut, CopyDesc: the kernel parameter types of bs_grow_spec.hip (136 and 32 bytes; the test uses stand-ins).
// Walked from null bases: the bytes to reserve (the pointers are then offsets); from the slots' addresses: the pointers.
template <class PlaneOut, class CopyDesc>
struct GrowLayout {
  // rg_aux
  MiscBlock* misc;
  uint32_t* hmask;
  int32_t *omega, *base, *dead;
  int32_t* prio;     // original index of every position
  int32_t* rpos;     // n + 1 (+ pad): reverse-list counts / fill cursors during the setup
  int32_t* vmark;    // duplicate detection of validate1
  int32_t* d_seeds;  // committed seeds (planes_cap)
  uint8_t* ps;
  uint32_t* occ;  // bitmap, (n + 31) / 32 words + 2 the passes may touch
  uint8_t *dirty0, *dirty1;
  uint8_t *bdirty0, *bdirty1, *bcand;  // one flag per 256 points; bcand: can the group still hold a plane seed?
  int32_t* wl_list[2];                 // worklists of the owner passes (see wl_flush): two lists of groups and,
  uint32_t* wl_flag[2];                // for the dirty groups, two flag arrays (cleared as one range)
  PlaneOut *d_out, *d_pend;
  CopyDesc* d_copy;
  // rg_disp: dispatch order of big rounds
  unsigned long long *tmin1, *tmin2;  // tile minima (nt1, nt2), set to ~0 as one range
  uint32_t *dkeys_in, *dkeys_out;     // sort keys
  PlaneOut* d_outc;                   // finished attempts of a big round, compacted
  // rg_hout, page-locked: per-round results read by the host
  PlaneOut *h_out, *h_pend;
  HostFlags* hf;
  // rg_geo: the candidate lists, one (original index << 32 | position) key each
  unsigned long long *cand_raw, *d_cand;  // unsorted | sorted, n + 64 each
  size_t aux_bytes, disp_bytes, hout_bytes, geo_bytes;

  explicit GrowLayout(const GrowSizes& s, void* aux = nullptr, void* disp = nullptr, void* hout = nullptr, void* geo = nullptr)
  {
    const size_t n = (size_t)s.n, nb = s.nb256, wc = (size_t)s.wave_cap;
    Carver a{reinterpret_cast<uintptr_t>(aux)}, d{reinterpret_cast<uintptr_t>(disp)}, h{reinterpret_cast<uintptr_t>(hout)},
        g{reinterpret_cast<uintptr_t>(geo)};
    misc = a.take<MiscBlock>(1, 256);
    hmask = a.take<uint32_t>(n);
    omega = a.take<int32_t>(n);
    base = a.take<int32_t>(n);
    dead = a.take<int32_t>(n);
    prio = a.take<int32_t>(n);
    rpos = a.take<int32_t>(n + 64);
    vmark = a.take<int32_t>(n);
    d_seeds = a.take<int32_t>((size_t)s.planes_cap);
    ps = a.take<uint8_t>(n);
    occ = a.take<uint32_t>((n + 31) / 32 + 2, 16);
    dirty0 = a.take<uint8_t>(n);
    dirty1 = a.take<uint8_t>(n);
    bdirty0 = a.take<uint8_t>(nb);
    bdirty1 = a.take<uint8_t>(nb);
    bcand = a.take<uint8_t>(nb);
    wl_list[0] = a.take<int32_t>(nb, 16);
    wl_list[1] = a.take<int32_t>(nb);
    wl_flag[0] = a.take<uint32_t>(nb);
    wl_flag[1] = a.take<uint32_t>(nb);
    d_out = a.take<PlaneOut>(wc, 256);
    d_pend = a.take<PlaneOut>(MAX_PENDING);
    d_copy = a.take<CopyDesc>(wc + MAX_PENDING);
    tmin1 = d.take<unsigned long long>(s.nt1);
    tmin2 = d.take<unsigned long long>(s.nt2);
    dkeys_in = d.take<uint32_t>(wc);
    dkeys_out = d.take<uint32_t>(wc);
    d_outc = d.take<PlaneOut>(wc, 16);
    h_out = h.take<PlaneOut>(wc);
    h_pend = h.take<PlaneOut>(MAX_PENDING);
    hf = h.take<HostFlags>(1);
    cand_raw = g.take<unsigned long long>(n + 64);
    d_cand = g.take<unsigned long long>(n + 64);
    aux_bytes = a.top, disp_bytes = d.top, hout_bytes = h.top, geo_bytes = g.top;
  }
  // A buffer under a second meaning, and until when.  n words: the inverse of the spatial order (foreign input), until
  // build_records_kernel has run
  int32_t* pos_in_vmark() const { return vmark; }
  // n words: low-index bits of the static masks, from static_mask_kernel to rev_fill_kernel; vmark is cleared behind it
  uint32_t* lmask_in_vmark() const { return reinterpret_cast<uint32_t*>(vmark); }
  // n words: lowest reverse neighbour per position, from decide_finish_kernel to the end of the call
  int32_t* minr_in_rpos() const { return rpos; }
  // n and nb256 bytes: decided states of the first fixed point, until the dirty flags are cleared behind it
  uint8_t* state_in_dirty1() const { return dirty1; }
  uint8_t* bund_in_bdirty1() const { return bdirty1; }
  // wave_cap words: the audit's retry flags, one per attempt of a batch; outside the rounds only
  int32_t* retry_in_dkeys_in() const { return reinterpret_cast<int32_t*>(dkeys_in); }
  // n entries: the 64-bit fill cursors of the reverse lists, during the setup only
  unsigned long long* rcur_in_cand_raw() const { return cand_raw; }
};

}  // namespace bs
