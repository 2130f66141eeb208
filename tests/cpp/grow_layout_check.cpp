// Arithmetic check of bs_grow_layout.h (the scratch layout of the speculative grower's host loop): nothing is
// allocated, every layout is walked from a null base so that its pointers ARE the offsets.  See
// tests/test_grow_layout_cpu.py for what is asserted.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "bs_grow_layout.h"

using namespace bs;

struct PlaneOutS {  // stand-ins with the size and alignment of bs_grow_spec.hip's PlaneOut and CopyDesc
  alignas(8) unsigned char b[136];
};
struct CopyDescS {
  alignas(8) unsigned char b[32];
};

// the kernels' indices into the sub-blocks they are handed (validate1/3: rejects[0], [1], [2], [8..11]; forge_kernel:
// &rejects[1]; audit_compare_kernel: stats[0], stats[1]; cand_flag_kernel's count and minimum, copied back as a pair)
static_assert(offsetof(RefusalStats, refused) == 0 && offsetof(RefusalStats, forged_seed1) == 4 * 1 &&
                  offsetof(RefusalStats, forged_refused) == 4 * 2 && offsetof(RefusalStats, v1_robbed) == 4 * 8 &&
                  offsetof(RefusalStats, v1_tag) == 4 * 9 && offsetof(RefusalStats, v1_dup) == 4 * 10 &&
                  offsetof(RefusalStats, v3_state) == 4 * 11 && sizeof(RefusalStats) == 4 * 12,
              "validators");
static_assert(offsetof(AuditStats, mismatches) == 0 && offsetof(AuditStats, committed_met) == 4 && sizeof(AuditStats) == 8, "audit");
static_assert(offsetof(CandCount, listed) == 0 && offsetof(CandCount, lowest) == 4 && sizeof(CandCount) == 8, "candidates");
static_assert(offsetof(MiscBlock, pool_top) % 8 == 0 && sizeof(MiscBlock::pool_top) == 8, "pool top");
static_assert(offsetof(MiscBlock, flip) % 128 == 0 && offsetof(MiscBlock, wl_cnt) % 128 == 0 && offsetof(MiscBlock, pstat) % 128 == 0 &&
                  offsetof(MiscBlock, wl_cnt) - offsetof(MiscBlock, flip) >= 128 && sizeof(MiscBlock) <= 4096,
              "the words the passes' atomics hit keep 128-byte lines of their own, as when they sat at words 32, 64 and 128");
static_assert(sizeof(MiscBlock::flip) == 4 * PULL_GROUP && sizeof(HostFlags::flip) == 4 * PULL_GROUP &&
                  sizeof(MiscBlock::pstat) == 16 * PULL_GROUP && sizeof(MiscBlock::wl_cnt) == 12,
              "owner passes");
static_assert(offsetof(HostFlags, next_cand) + 8 <= offsetof(HostFlags, refused), "one copy-back of two words");

static long checks = 0, bad = 0;
#define CHECK(cond, ...)        \
  do {                          \
    checks++;                   \
    if (!(cond)) {              \
      if (bad++ < 20) {         \
        printf("FAIL %s: ", #cond); \
        printf(__VA_ARGS__);    \
        printf("\n");           \
      }                         \
    }                           \
  } while (0)

struct Reg {
  const char* name;
  uint64_t off, elem, count, align;
};
template <class T>
static Reg reg(const char* name, const T* p, uint64_t count, uint64_t align = alignof(T))
{
  return Reg{name, (uint64_t) reinterpret_cast<uintptr_t>(p), sizeof(T), count, align};
}
// an alias starts where its host region starts and is no longer than it
template <class T, class H>
static void alias(const char* name, const T* p, uint64_t count, const H* host, uint64_t host_count, int64_t n)
{
  CHECK((const void*)p == (const void*)host, "%s n=%" PRId64, name, n);
  CHECK(sizeof(T) * count <= sizeof(H) * host_count, "%s n=%" PRId64, name, n);
}

static void check_slot(const char* slot, const std::vector<Reg>& r, uint64_t total, uint64_t parent, int64_t n)
{
  uint64_t need = 0;  // bytes of everything in front, without padding: an offset cut to 32 bits falls below it
  for (size_t i = 0; i < r.size(); i++) {
    CHECK(r[i].off % r[i].align == 0, "%s.%s n=%" PRId64 " off=%" PRIu64, slot, r[i].name, n, r[i].off);
    CHECK(r[i].off >= need, "%s.%s n=%" PRId64 " off=%" PRIu64 " need=%" PRIu64, slot, r[i].name, n, r[i].off, need);
    CHECK(r[i].off + r[i].elem * r[i].count <= total, "%s.%s n=%" PRId64 " ends past %" PRIu64, slot, r[i].name, n, total);
    for (size_t j = 0; j < i; j++)
      CHECK(r[j].off + r[j].elem * r[j].count <= r[i].off || r[i].off + r[i].elem * r[i].count <= r[j].off,
            "%s.%s overlaps %s n=%" PRId64, slot, r[i].name, r[j].name, n);
    need += r[i].elem * r[i].count;
  }
  CHECK(total <= parent, "%s n=%" PRId64 " bytes %" PRIu64 " > before %" PRIu64, slot, n, total, parent);
}

static void check(int64_t n, int K, int th, const bs_grow_limits& lim)
{
  const int64_t req = lim.max_waves > 0 ? std::min<int64_t>(lim.max_waves, MAX_WAVES) : MAX_WAVES;
  const GrowSizes s(n, K, th, req, lim);
  // the sizes, written out again
  const uint64_t un = (uint64_t)n, MP = 32768, MW = 1u << 18;
  const uint64_t planes_cap = un / (uint64_t)(th < 1 ? 1 : th) + 64;
  const uint64_t wc = std::max<uint64_t>(1, std::min<uint64_t>(MW, un / 8 + 64));
  const uint64_t nb = (un + 255) / 256, nt1 = (un >> 12) + 2, nt2 = (un >> 16) + 2;
  const uint64_t pool = std::max<uint64_t>(std::min<uint64_t>(64 * un, (uint64_t)3 << 30), 8 * un + 3072 * wc);
  CHECK((uint64_t)s.list_cap == 2 * un + 64 && (uint64_t)s.planes_cap == planes_cap && (uint64_t)s.wave_cap == wc, "sizes n=%" PRId64, n);
  CHECK(s.nb256 == nb && s.nt1 == nt1 && s.nt2 == nt2 && s.pool_cap == pool && (uint64_t)s.pstore_cap == 6 * un + 65536, "sizes n=%" PRId64, n);
  CHECK(s.KC == (K <= 16 ? 16 : 32) && s.quads == 4 + s.KC / 4, "K=%d", K);
  CHECK(s.max_waves >= 1 && (uint64_t)s.max_waves <= wc && s.max_waves <= std::max<int64_t>(1, req), "max_waves n=%" PRId64, n);
  CHECK(s.pool_cap_eff <= pool && (lim.pool_cap <= 0 ? s.pool_cap_eff == pool : s.pool_cap_eff <= (uint64_t)lim.pool_cap), "pool n=%" PRId64, n);
  CHECK(s.pstore_lim <= s.pstore_cap && (lim.pstore_cap <= 0 ? s.pstore_lim == s.pstore_cap : s.pstore_lim <= lim.pstore_cap), "pstore n=%" PRId64, n);
  CHECK(s.pend_lim >= 1 && s.pend_lim <= (int)MP && (lim.max_pending <= 0 ? s.pend_lim == (int)MP : s.pend_lim <= lim.max_pending), "pending n=%" PRId64, n);

  const GrowLayout<PlaneOutS, CopyDescS> a(s);
  const GrowLayout<PlaneOutS, CopyDescS>&d = a, &h = a, &g = a;
  check_slot("rg_aux",
             {reg("misc", a.misc, 1, 256), reg("hmask", a.hmask, un), reg("omega", a.omega, un), reg("base", a.base, un),
              reg("dead", a.dead, un), reg("prio", a.prio, un), reg("rpos", a.rpos, un + 64), reg("vmark", a.vmark, un),
              reg("seeds", a.d_seeds, planes_cap), reg("ps", a.ps, un), reg("occ", a.occ, (un + 31) / 32 + 2, 16),
              reg("dirty0", a.dirty0, un), reg("dirty1", a.dirty1, un), reg("bdirty0", a.bdirty0, nb), reg("bdirty1", a.bdirty1, nb),
              reg("bcand", a.bcand, nb), reg("wl_list0", a.wl_list[0], nb, 16), reg("wl_list1", a.wl_list[1], nb),
              reg("wl_flag0", a.wl_flag[0], nb), reg("wl_flag1", a.wl_flag[1], nb), reg("d_out", a.d_out, wc, 256),
              reg("d_pend", a.d_pend, MP), reg("d_copy", a.d_copy, wc + MP)},
             a.aux_bytes,
             4 * (7 * un + planes_cap + 1024 + 128) + 5 * un + 3 * nb + 16 * nb + 8192 + 136 * (wc + MP) + 32 * (wc + MP), n);
  CHECK(a.wl_flag[1] == a.wl_flag[0] + nb, "the two flag arrays are cleared as one range, n=%" PRId64, n);
  alias("pos_in_vmark", a.pos_in_vmark(), un, a.vmark, un, n);
  alias("lmask_in_vmark", a.lmask_in_vmark(), un, a.vmark, un, n);
  alias("minr_in_rpos", a.minr_in_rpos(), un, a.rpos, un + 64, n);
  alias("state_in_dirty1", a.state_in_dirty1(), un, a.dirty1, un, n);
  alias("bund_in_bdirty1", a.bund_in_bdirty1(), nb, a.bdirty1, nb, n);

  check_slot("rg_disp",
             {reg("tmin1", d.tmin1, nt1), reg("tmin2", d.tmin2, nt2), reg("dkeys_in", d.dkeys_in, wc), reg("dkeys_out", d.dkeys_out, wc),
              reg("d_outc", d.d_outc, wc, 16)},
             d.disp_bytes, 8 * (nt1 + nt2) + 4 * 2 * wc + 64 + 136 * wc, n);
  CHECK(d.tmin2 == d.tmin1 + nt1, "the tile minima are set as one range, n=%" PRId64, n);
  alias("retry_in_dkeys_in", d.retry_in_dkeys_in(), wc, d.dkeys_in, wc, n);

  check_slot("rg_hout", {reg("h_out", h.h_out, wc), reg("h_pend", h.h_pend, MP), reg("flags", h.hf, 1)}, h.hout_bytes,
             136 * (wc + MP) + 256, n);

  check_slot("rg_geo", {reg("cand_raw", g.cand_raw, un + 64), reg("d_cand", g.d_cand, un + 64)}, g.geo_bytes, 8 * 2 * (un + 64), n);
  alias("rcur_in_cand_raw", g.rcur_in_cand_raw(), un, g.cand_raw, un + 64, n);

  if (n == ((int64_t)1 << 31) - 65) {  // offsets beyond 2^32, not cut to 32 bits
    CHECK((uint64_t) reinterpret_cast<uintptr_t>(a.omega) >= 4 * un, "omega");
    CHECK((uint64_t) reinterpret_cast<uintptr_t>(a.d_copy) >= 31 * un, "d_copy");
    CHECK((uint64_t) reinterpret_cast<uintptr_t>(g.d_cand) >= 8 * un, "d_cand");
    CHECK(a.aux_bytes > ((uint64_t)1 << 35), "aux");
  }
  // a lowered limit never changes a buffer: the layouts equal those without limits
  const bs_grow_limits none = {0, 0, 0, 0, -1, -1, 0, 0};
  const GrowSizes s0(n, K, th, MAX_WAVES, none);
  const GrowLayout<PlaneOutS, CopyDescS> a0(s0);
  CHECK((a0.aux_bytes == a.aux_bytes && a0.disp_bytes == d.disp_bytes && a0.hout_bytes == h.hout_bytes && a0.geo_bytes == g.geo_bytes &&
         s0.pool_cap == s.pool_cap && s0.pstore_cap == s.pstore_cap),
        "limits change a size, n=%" PRId64, n);
}

int main()
{
  const int64_t ns[] = {1, 2, 7, 8, 255, 256, 257, 511, 513, 4095, 65535, 65536, 65537, 2096632, 2096640, 2096648,
                        50000000, 200000000, ((int64_t)1 << 31) - 65};
  const int Ks[] = {2, 15, 16, 17, 32};
  const int ths[] = {0, 1, 50, 1000000000};
  const bs_grow_limits lims[] = {{0, 0, 0, 0, -1, -1, 0, 0}, {1, 0, 0, 0, -1, -1, 0, 0},    {4097, 0, 0, 0, -1, -1, 0, 0},
                                 {0, 1000, 0, 0, -1, -1, 0, 0}, {0, 0, 1, 0, -1, -1, 0, 0}, {0, 0, 0, 100, -1, -1, 0, 0},
                                 {0, 0, 0, 0, 0, 0, 1, 0}};
  for (const int64_t n : ns)
    for (const int K : Ks)
      for (const int th : ths)
        for (const bs_grow_limits& lim : lims)
          check(n, K, th, lim);
  printf("checks=%ld bad=%ld\n", checks, bad);
  return bad ? 1 : 0;
}
