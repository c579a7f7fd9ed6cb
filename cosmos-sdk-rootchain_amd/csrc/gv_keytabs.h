// gv_keytabs.h -- the pure parts of the runtime's secp256k1 key table sets:
// a set's layout (entries per group table, words per entry, groups per key),
// the bytes the arenas charge to the HBM budget, the one growth rule of the
// key arenas, the wide arena's layout list and the grouped route's promotion
// arithmetic.  Host-only (no HIP runtime call), so the CPU tests drive the
// same code (tests/keytabs), as gv_options.h and gv_kidx.h.  The owning type
// (KeyTabs) and its view (KeyView) are in gv_runtime.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "gv_kernels.h"
#include "gv_kidx.h"

namespace gvkt {

// A table set holds, per slot, ng group tables of nt entries of ew words
// (group 0 in one array, groups 1.. in another) and 8 Z words per group.
// nt = 2^(qw - 1) for a qw-bit window in every layout.
struct TabLayout {
  uint32_t nt = 0, ew = 0, ng = 0;
  size_t table_words() const { return (size_t)nt * ew; }   // one group table
  int qw() const { int w = 0; while (nt >> w) ++w; return w; }   // (no layout: 0)
  bool operator==(const TabLayout& o) const { return nt == o.nt && ew == o.ew && ng == o.ng; }
  bool operator!=(const TabLayout& o) const { return !(*this == o); }
};
inline TabLayout lay_k4() { return {GV_QTAB_N, GV_QENT_WORDS, GV_LGRP}; }
inline TabLayout lay_kn() { return {GV_K6_NT, GV_QENT_WORDS, GV_KN_ARENA_NG}; }   // the resident kn arena
inline TabLayout lay_k6() { return {GV_K6_NT, GV_QENT_WORDS, 4}; }                // the grouped k6 layout
inline TabLayout lay_kg(int ng) { return {GV_QTAB_N, GV_QENT_WORDS, (uint32_t)ng}; }   // ng: one of GV_KG_NGS
inline TabLayout lay_wide(int qw, int ng) {
  return qw && ng ? TabLayout{(uint32_t)gvk_kw_nt(qw), GV_KW_ENT_WORDS, (uint32_t)ng} : TabLayout{};
}

// Bytes of one slot's tables and Zs.
inline size_t slot_bytes(const TabLayout& l) { return (l.table_words() + 8) * l.ng * 4; }
// Bytes per slot of the resident arena: the k4 tables and the verdict word,
// with the kn arena its tables too.
inline size_t resident_slot_bytes(bool kn) { return slot_bytes(lay_k4()) + 4 + (kn ? slot_bytes(lay_kn()) : 0); }

// Table words of an open-addressing table (the pubkey index, a grouped
// arena's cache) over `cap` slots: a power of two, at least twice the capacity
// and 512.
inline size_t kidx_table_words(size_t cap) {
  size_t T = 512;
  while (T < 2 * cap) T <<= 1;
  return T;
}
// Bytes of a set's grouped arena of `cap` keys: the tables and verdicts and,
// per key, its raw row and its share of the cache's table.
inline size_t group_bytes(size_t cap, const TabLayout& l) {
  return cap * (slot_bytes(l) + 4) + (cap * GV_KIDX_ROW + kidx_table_words(cap)) * 4;
}

// The key arenas' growth rule: doubling, but not past cap_limit (the callers'
// reset point) -- past it the arena grows to exactly what is needed (a caller
// that never resets pays one copy per load, not a quadratic series of
// doublings); at least `floor`, in steps of 256.
inline size_t arena_grow_cap(size_t have, size_t need, size_t cap_limit, size_t floor) {
  const size_t grow = have >= cap_limit ? need : std::min<size_t>(2 * have, std::max<size_t>(need, cap_limit));
  return (std::max<size_t>({need, grow, floor}) + 255) / 256 * 256;
}

// opt_bytes with one holding replaced by another (an old arena by the new
// one; 0: none): never below zero.
inline size_t budget_replace(size_t opt_bytes, size_t old_b, size_t new_b) {
  return opt_bytes - std::min(opt_bytes, old_b) + new_b;
}

// The wide arena's layouts in order of falling memory per key: 768, 384, 240
// and 128 KiB of tables at 11 / 9 bits.  gv_keys_load starts an arena at the
// first one its options allow ("keys_wide" 2: any, 1: two windows per group;
// "keys_wide_qw": one width only) and moves the whole arena to the next
// allowed one when a growth is refused.
struct WideLayout {
  int qw, ng, wpg;                                // window width, groups, windows per group
};
const WideLayout kWideLayouts[] = {{GV_KW_QW, GV_KW_NG1, 1}, {GV_KW_QW, GV_KW_NG2, 2},
#if GV_KWN
                                   {GV_KWN_QW, GV_KWN_NG1, 1}, {GV_KWN_QW, GV_KWN_NG2, 2},
#endif
};
constexpr int kWideLayoutCount = (int)(sizeof kWideLayouts / sizeof kWideLayouts[0]);
inline TabLayout lay_wide(const WideLayout& w) { return lay_wide(w.qw, w.ng); }
// The first layout at or after index `from` of width only_qw (0: any) with at
// least min_wpg windows per group; kWideLayoutCount when there is none.
inline int wide_layout_next(int from, int only_qw, int min_wpg) {
  for (int i = from; i < kWideLayoutCount; ++i)
    if ((!only_qw || kWideLayouts[i].qw == only_qw) && kWideLayouts[i].wpg >= min_wpg) return i;
  return kWideLayoutCount;
}

// group_promote: a set whose keys recur moves from k4's
// layout to the option's kg layout (more groups: a dearer build per key, fewer
// doublings per item) and back.  The two constants, serialized on the C2 batch
// (profiles/r07/group_promote/consts_parent.jsonl): what a built key costs
// more than in k4's layout, what an item saves on the ladder, in picoseconds.
// Their ratio is the break-even in keys built per item: a promoted set demotes
// above it (T_down), a k4 set promotes after two warm calls (and on a third)
// that each built less than half of it (T_up).
struct PromoteCost {
  int ng;
  uint64_t key_ps, item_ps;
};
constexpr PromoteCost kPromoteCost[] = {{6, 5456, 307}, {7, 7170, 497}, {9, 11436, 621}};
inline const PromoteCost* promote_cost(int ng) {
  for (const PromoteCost& c : kPromoteCost)
    if (c.ng == ng) return &c;
  return nullptr;
}
// keys built over items against the break-even: below half of it / above it
inline bool promote_below_up(const PromoteCost& c, size_t built, size_t n) { return 2 * built * c.key_ps < n * c.item_ps; }
inline bool promote_above_down(const PromoteCost& c, size_t built, size_t n) { return built * c.key_ps > n * c.item_ps; }

// keys_index_split: a pub33 device batch the index looked
// up, `miss` of its items not resident.  It splits -- the resident items on the
// arena, the others as a dense sub-batch on the pub33 routes -- when the index
// is live, there is a miss, the option (`bound`: the most misses per call still
// split; 0 = never) covers them and the sub-batch's buffers are at hand.  Else
// no miss runs keyed and any miss falls through whole, as without the option.
inline bool kidx_split_ok(size_t bound, size_t miss, bool live, bool buffers) {
  return live && buffers && miss != 0 && miss <= bound;
}
// Rows of the sub-batch's buffers for `miss` items: the misses rounded up to
// 256, a growth at least doubling what is held (never sized by the option).
inline size_t kidx_split_rows(size_t have, size_t miss) {
  const size_t need = (miss + 255) / 256 * 256;
  return need <= have ? have : std::max(need, 2 * have);
}
// Their bytes, each part 256-byte aligned: the row counter, idx, pub33, sig64,
// dig32 (or u64 off + u32 len in its place), the accept bitmap.
struct SplitLayout {
  size_t idx, pub, sig, third, len, bits, total;
};
inline SplitLayout kidx_split_layout(size_t rows) {   // rows % 256 == 0
  SplitLayout L;
  L.idx = 256;
  L.pub = L.idx + rows * 4;
  L.sig = L.pub + (rows * 33 + 255) / 256 * 256;
  L.third = L.sig + rows * 64;
  L.len = L.third + rows * 8;
  L.bits = L.third + rows * 32;
  L.total = L.bits + (rows / 64 * 8 + 255) / 256 * 256;
  return L;
}

}  // namespace gvkt
