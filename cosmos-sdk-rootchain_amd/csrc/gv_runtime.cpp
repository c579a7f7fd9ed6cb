// gv_runtime.cpp -- the C-ABI runtime of libgpuverify.so (include/gpuverify.h).
//
// Per device: two pipeline "sets" (device scratch for one batch chunk, a HIP
// stream, pinned host staging), a persistent worker thread and a small pool of
// staging threads.  A host batch is split into contiguous slices, one per
// device (no collective -- SURVEY.md §8e); each slice is cut into chunks that
// alternate between the two sets, so the staging memcpy + H2D copy of chunk
// c+1 overlaps the kernels of chunk c (§8e "one host thread + 2 HIP streams
// per GPU, double-buffered pinned staging").  Only the packed accept bitmap
// comes back.  Fail-closed: any HIP error returns GV_EHIP and the caller
// re-verifies on the CPU.
//
// Ordering: every use of a set's device scratch, on whichever stream, first
// waits for the previous use of that set (its `last` event) and then records
// `last` again -- so a gv_dev_* call on a caller stream and a later host-path
// or gv_dev_* call on another stream can never overwrite the inputs of kernels
// still in flight.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <list>
#include <unordered_map>
#include <utility>
#include <future>
#include <mutex>
#include <random>
#include <memory>
#include <sched.h>
#include <thread>
#include <vector>

#include "../../include/gpuverify.h"
#include "gv_kernels.h"
#include "gv_kidx.h"
#include "gv_keytabs.h"
#include "gv_options.h"
#include "gv_stage.h"
#include "gv_async.h"

// The build facts gv_options.h's accept rules ask for: the grouped route's kg
// layouts (gv_kernels.h GV_KG_NGS), or 0 (off); the wide arena's widths.
bool gvopt::kg_layout_ok(int ng) {
  static const int kNGs[] = {GV_KG_NGS};
  if (ng == 0) return true;
  for (int v : kNGs)
    if (v == ng) return true;
  return false;
}
bool gvopt::kw_width_ok(int qw) { return gvk_kw_width_ok(qw); }

namespace {

#define CK(call)                                  \
  do {                                            \
    hipError_t e_ = (call);                       \
    if (e_ != hipSuccess) return GV_EHIP;         \
  } while (0)

using gvopt::kMaxItems;
constexpr size_t kLaneWords = 8 + 1 + 8 + 8 + 8 + GV_DIGIT_ROWS + 8 + 1 + GV_QTAB_WORDS;

size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

// The blob bytes [lo, hi) that the messages of items [lo_i, hi_i) span; no
// item: (0, 0).
std::pair<uint64_t, uint64_t> msg_range(const uint64_t* off, const uint32_t* len, size_t lo_i, size_t hi_i) {
  uint64_t lo = UINT64_MAX, hi = 0;
  for (size_t i = lo_i; i < hi_i; ++i) {
    lo = std::min<uint64_t>(lo, off[i]);
    hi = std::max<uint64_t>(hi, off[i] + len[i]);
  }
  if (lo > hi) lo = hi = 0;
  return {lo, hi};
}

// The key-ordered-lanes scratch (gv_sort.hip) of C lanes and nb buckets from
// word p on: 3 C + 2 round_up(nb, 64) + round_up(tb / 4 + 1, 64) words (tb =
// gvk_sort_temp_bytes(nb)).  No bits row: the secp256k1 pipeline adds its own.
gvk_sort carve_sort(uint32_t* p, size_t C, size_t nb, size_t tb) {
  gvk_sort so;
  so.pos = p; p += C;
  so.perm = p; p += C;
  so.kslot = p; p += C;
  so.bits = nullptr;
  so.cnt = p; p += round_up(nb, 64);
  so.off = p; p += round_up(nb, 64);
  so.temp = p;
  so.temp_bytes = tb;
  return so;
}
size_t sort_words(size_t C, size_t nb, size_t tb) { return 3 * C + 2 * round_up(nb, 64) + round_up(tb / 4 + 1, 64); }

// ------------------------------------------------------------ thread helpers
// Pool, Worker, par_copy*, host_cpus, run_sliced: gv_stage.h
using gvstage::CopySeg;
using gvstage::Pool;
using gvstage::Worker;
using gvstage::host_cpus;
using gvstage::par_copy;
using gvstage::par_copy_segs;
using gvstage::run_sliced;


// ------------------------------------------------------------ key table sets
// Layouts, bytes, the growth rule, the promotion arithmetic: gv_keytabs.h
using namespace gvkt;

// One secp256k1 key table set on the device, in the layout lay: per slot the
// group-0 table (qt) on the Z in zq (8 rows of stride cap), the tables of
// groups 1.. (qt2: lay.ng - 1 rows per slot) and the chain's parked Zs (zq2:
// (lay.ng - 1) x 8 rows of stride cap); ok: the verdict row of a set that owns
// one (the resident kn and wide sets share k4's).  Plain data: copied by
// assignment, freed by hand.  lay outlives free() (the wide arena's choice).
struct KeyTabs {
  uint32_t *qt = nullptr, *zq = nullptr, *ok = nullptr, *qt2 = nullptr, *zq2 = nullptr;
  size_t cap = 0;
  TabLayout lay;

  void free() {
    for (uint32_t** p : {&qt, &zq, &ok, &qt2, &zq2})
      if (*p) { (void)hipFree(*p); *p = nullptr; }
    cap = 0;
  }
  // An empty set becomes c slots of layout l; all or nothing.
  bool alloc(const TabLayout& l, size_t c, bool with_ok) {
    const size_t tb = l.table_words() * 4, g1 = (size_t)l.ng - 1;
    lay = l;
    if (hipMalloc(&qt, c * tb) != hipSuccess || hipMalloc(&zq, c * 8 * 4) != hipSuccess ||
        (with_ok && hipMalloc(&ok, c * 4) != hipSuccess) || hipMalloc(&qt2, c * g1 * tb) != hipSuccess ||
        hipMalloc(&zq2, c * g1 * 8 * 4) != hipSuccess) {
      free();
      (void)hipGetLastError();
      return false;
    }
    cap = c;
    return true;
  }
  // The first `used` slots of o (the same layout, any capacity) into this set
  // on st: the Z rows move from stride o.cap to stride cap.
  bool copy_from(const KeyTabs& o, size_t used, hipStream_t st) {
    const size_t tb = lay.table_words() * 4, g1 = (size_t)lay.ng - 1;
    bool good = hipMemcpyAsync(qt, o.qt, used * tb, hipMemcpyDeviceToDevice, st) == hipSuccess &&
                hipMemcpyAsync(qt2, o.qt2, used * g1 * tb, hipMemcpyDeviceToDevice, st) == hipSuccess;
    for (size_t r = 0; good && r < 8; ++r)
      good = hipMemcpyAsync(zq + r * cap, o.zq + r * o.cap, used * 4, hipMemcpyDeviceToDevice, st) == hipSuccess;
    for (size_t r = 0; good && r < g1 * 8; ++r)
      good = hipMemcpyAsync(zq2 + r * cap, o.zq2 + r * o.cap, used * 4, hipMemcpyDeviceToDevice, st) == hipSuccess;
    if (good && ok) good = hipMemcpyAsync(ok, o.ok, used * 4, hipMemcpyDeviceToDevice, st) == hipSuccess;
    return good;
  }
};

// A table set as a launch or a readback takes it: the resident arena's k4, kn
// or wide tables (arena_tabs) or a set's grouped keys (group_keys), with the
// selectors the kernels want (gvk_batch k6 / kqw / kwq, gvk_lat kn) and the
// G tables of its ladder.  The launch stream waits on `ready` first.
enum { kTabsK4 = 0, kTabsKn = 1, kTabsWide = 2 };   // gvk_lat's kn values
struct KeyView {
  const uint32_t *kqt = nullptr, *kzq = nullptr, *kok = nullptr, *kqt2 = nullptr, *kzq2 = nullptr;
  uint32_t kC = 0, kcount = 0;
  TabLayout lay;
  int k6 = 0, kqw = 0, kwq = 0, kn = kTabsK4;
  const uint32_t *gtab4 = nullptr, *gtab6 = nullptr;
  hipEvent_t ready = nullptr;

  KeyView() = default;
  // count slots of t; ok: the verdict row of a set that owns none
  KeyView(const KeyTabs& t, size_t count, const uint32_t* ok = nullptr)
      : kqt(t.qt), kzq(t.zq), kok(t.ok ? t.ok : ok), kqt2(t.qt2), kzq2(t.zq2), kC((uint32_t)t.cap),
        kcount((uint32_t)count), lay(t.lay) {}
  void to_batch(gvk_batch& b, const uint32_t* kslot) const {
    b.pub33 = nullptr;
    b.kslot = kslot; b.kqt = kqt; b.kzq = kzq; b.kok = kok;
    b.kC = kC; b.kcount = kcount;
    b.kqt2 = kqt2; b.gtab4 = gtab4;               // null gtab4: the 125-doubling keyed ladder
    b.k6 = k6; b.kqw = kqw; b.kwq = kwq; b.gtab6 = gtab6;
    b.keys_ready = ready;
  }
  // (k_verify_lat16_kn / _kw read no parked Zs; the k4 kernels no gtab6)
  void to_lat(gvk_lat& lb, const uint32_t* kslot) const {
    lb.pub33 = nullptr;
    lb.kslot = kslot; lb.kqt = kqt; lb.kzq = kzq; lb.kok = kok; lb.kC = kC; lb.kcount = kcount;
    lb.kqt2 = kqt2; lb.kzq2 = kn ? nullptr : kzq2;
    if (kn) { lb.gtab6 = gtab6; lb.kn = kn; }
  }
};

// ------------------------------------------------------------ device state
// Device scratch of one batch chunk of C lanes (C % 256 == 0): the staged
// inputs (one contiguous region so a host chunk is ONE H2D copy), the SoA
// working rows of the kernels, the accept bitmap.
struct Set {
  size_t cap = 0;
  uint8_t* scratch = nullptr;
  uint8_t* d_in = nullptr;                        // staged inputs, layout of in_layout()
  uint32_t *in_x = nullptr, *in_pfx = nullptr, *in_r = nullptr, *in_s = nullptr, *in_e = nullptr;
  uint32_t *digits = nullptr, *zq = nullptr, *flags = nullptr, *qtab = nullptr;
  uint64_t* bits = nullptr;
  uint8_t* d_blob = nullptr;                      // message path blob
  size_t blob_cap = 0;
  hipStream_t st = nullptr;                       // the set's own stream (host path; front priority)
  hipStream_t lad = nullptr;                      // host path: the chunk's ladder (ladder priority), so the
                                                  // next chunk's / batch's front kernels take CU slots first
  hipEvent_t lad_done = nullptr;
  hipEvent_t last = nullptr;                      // end of the last work using this set
  hipStream_t last_st = nullptr;
  hipEvent_t done = nullptr;                      // host path: chunk finished (bits on host)
  hipEvent_t h2d = nullptr;                       // host path: the chunk's H2D copies enqueued so far done
  hipEvent_t ecm_ready = nullptr;                 // pipelined device calls: front kernels done
  hipStream_t side = nullptr;                     // grouped keys: table builds beside k_scalar_inv
  hipEvent_t fork = nullptr, keys_done = nullptr;
  hipEvent_t grp_ready = nullptr;                 // slice grouping on this set: the keys' tables are built
  // in-batch key grouping: the per-batch key arena (tables of the batch's
  // distinct keys with their verdicts, for up to gk.cap keys in the layout gk.lay)
  KeyTabs gk;
  // the arena as a cache of key tables (option "group_reuse"; DESIGN section
  // 4.1k): rows [0, g_count) hold the tables of the keys whose raw rows
  // (GV_KIDX_ROW words, gv_kidx.h) are in g_rows, g_idx the open-addressing
  // table over them (g_T words, one block with g_rows).  g_live: the rows, the
  // table and g_count describe what the arena holds; g_route: the schedule the
  // tables were built for (GV_ROUTE_*) -- with gk's layout and the allocation
  // (ensure_group_arena clears g_live) the cache's validity tag
  uint32_t *g_rows = nullptr, *g_idx = nullptr;
  size_t g_T = 0, g_count = 0;
  bool g_live = false;
  int g_route = -1;
  int g_lng = 0;                                  // groups per key of the rows at hand (gk.lay.ng, or k4's 4 in a g_wide arena)
  uint64_t g_seed = 0;                            // the table's hash seed (ctx->opt.kidx_seed when it was filled)
  // layout promotion (option "group_promote").  g_hist: the
  // set's last two grouped calls on the k4 layout, newest in bit 0 -- set when
  // the call was warm (a lookup ran, nothing flushed) and built fewer keys
  // than items x T_up.  g_promoted: the set's key stream runs on the kg layout.
  // Both describe the stream, not the tables: they outlive a dropped cache and
  // are cleared by the options that choose the grouped schedule.
  // g_promo_refused: the promoted arena was refused (no retry until a
  // quiescing option).  g_wide: the arena was allocated for a promoted layout;
  // k4's rows index a prefix of it, so a demoted set keeps it
  unsigned g_hist = 0;
  bool g_promoted = false, g_promo_refused = false, g_wide = false;
  uint32_t* h_count = nullptr;                    // pinned: the distinct-key count read back
  // a routed pub33 device batch with a few keys that are not resident (option
  // "keys_index_split"): the dense sub-batch of those
  // items -- miss_buf, one block of kidx_split_layout(miss.cap).total bytes
  // charged to the HBM budget, carved into `miss` -- and the scratch set the pub33 routes
  // verify it on (miss_set: its scratch and `last` only).  They belong to the
  // set whose call split: the merge runs before that call's set_release, so
  // the set's next call (two pipelined calls alternate the sets) finds them free.
  // miss_done: the sub-batch's end on the front stream, which the ladder
  // stream's merge waits for
  uint32_t* miss_buf = nullptr;
  gvk_split miss = {};
  Set* miss_set = nullptr;
  hipEvent_t miss_done = nullptr;
  // pinned host staging
  uint8_t* h_in = nullptr;
  size_t h_in_cap = 0;
  uint8_t* h_blob = nullptr;
  size_t h_blob_cap = 0;
  uint64_t* h_bits = nullptr;
  size_t h_bits_cap = 0;
  uint8_t* h_out8 = nullptr;                      // zero-copy small batches: verdict bytes, written by the kernel
  size_t h_out8_cap = 0;
  // chunk waiting to be harvested
  bool busy = false;
  bool zc = false;                                // the chunk ran zero-copy (verdicts in h_out8)
  size_t c0 = 0, cn = 0;
};

// Input region layout of a chunk of C lanes: [pub33 (or u32 slot)] [sig64]
// [dig32 | u64 off + u32 len], each part 256-byte aligned.
struct InLayout {
  size_t sig, third, len, total;
};
InLayout in_layout(size_t C, bool keyed, bool msgs) {
  InLayout L;
  L.sig = round_up(C * (keyed ? 4 : 33), 256);
  L.third = L.sig + C * 64;
  L.len = L.third + C * 8;                        // msgs only
  L.total = msgs ? L.len + C * 4 : L.third + C * 32;
  return L;
}

// A key arena's pubkey index (options "keys_index" / "ed_keys_index";
// gv_kidx.h; DESIGN sections 4.1j and 4.3e).  Per context: device batches the
// index routed keyed / that fell through on a miss, and k_kidx_* launches
// since gv_open ("keys_index_hit", "_miss", "_launches"; the same behind "ed_").
struct KeyIndexStats {
  std::atomic<uint64_t> hit{0}, miss{0}, launches{0};
};
// ... and per device: the key rows of `row` words per slot (the bytes as
// loaded -- a rejected key's too), the table of T words (kidx_table_words of
// the arena's capacity: a power of two >= 2 cap, >= 512; a slot or
// GV_KIDX_EMPTY); `keys` leading slots went through k_kidx_put.  own_rows (the
// secp256k1 index): rows of capacity cap and the table are one block, the
// rows first; else (the ed25519 index) the rows are the arena's ekpub rows and
// only the table is the index's.  on: the running arena took the option at
// slot 0.  failed: an allocation was refused or a launch failed (no index
// until the arena's reset).  cnt (device): [0] keys k_kidx_put left out since
// the last refill (left_out: its last read-back), [16] the misses of the
// lookup in flight; h: its pinned copy.  seed, stat: the context's.
struct KeyIndex {
  const uint32_t row;
  const bool own_rows;
  const uint64_t* seed = nullptr;
  KeyIndexStats* stat = nullptr;
  uint32_t *rows = nullptr, *tab = nullptr, *cnt = nullptr, *h = nullptr;
  size_t cap = 0, T = 0, keys = 0;
  bool on = false, failed = false;
  uint64_t left_out = 0;
  size_t key_bytes() const {
    return row == GV_KIDX_ROW ? gv_kidx_key<GV_KIDX_ROW>::bytes : gv_kidx_key<GV_KIDX_ROW_ED>::bytes;
  }
  size_t bytes() const { return ((own_rows ? cap * row : 0) + T) * 4; }   // of the block it owns
  bool filled() const { return tab && keys && !failed; }                  // some slot's bytes are in the table
};

struct Dev {
  int id = 0;
  uint32_t* gtab = nullptr;
  Set set[2];
  Set gset[2];                                    // host slices: whole-slice key grouping (slice_group); the
                                                  // async lane alternates the two (a slice's grouping under the
                                                  // previous slice's chunks)
  hipEvent_t last_h2d = nullptr;                  // host slice: the previous chunk's H2D (h2d_serial)
  // key arena (gv_keys_load): the k4 table set (Q's table and the group tables
  // of 2^35 Q, 2^70 Q, 2^100 Q) and the verdicts of every slot
  KeyTabs k4;
  uint32_t* glat = nullptr;                       // group tables of G / lambda G (k_gen_glat)
  uint32_t* gtab4 = nullptr;                      // k_ecmult_k4's tables of 2^35 G, 2^70 G, 2^100 G (+ lambda)
  uint32_t* gtab6 = nullptr;                      // k_ecmult_k6's full-scalar 24-bit-window tables of 2^(36 t) G (3.5 GiB)
  bool gtab6_failed = false;                      // its allocation failed once: keyed / grouped batches stay on k4
  uint32_t* gtabf = nullptr;                      // k_ecmult_k4<true>'s full-scalar G tables (GV_GF_WORDS, 6 GiB)
  bool gtabf_failed = false;                      // its allocation failed once: k4 keeps the GLV G tables
  bool gtab4_failed = false;                      // gtab4's allocation failed: keyed batches on the 125-doubling ladder
  // the resident kn set (option "keys_k6"; lay_kn: 11 32-entry group tables of
  // 2^(12 g) Q), at k4's capacity, read by k_ecmult_kn and k_verify_lat16_kn
  KeyTabs kn;
  size_t keys6 = 0;                               // leading slots whose k6 tables are built
  // the resident arena's wide-window tables (option "keys_wide"), in an arena
  // of their own: the layout gv_keys_load picked (kWideLayouts, gv_keytabs.h;
  // kw.lay.ng 0: none yet), grown by doubling while the HBM budget holds it;
  // keysw leading slots built.  kw_full: the last layout's growth was refused
  // (no more wide-window builds until gv_keys_reset)
  KeyTabs kw;
  size_t keysw = 0;
  bool kw_full = false;
  // the arena's pubkey index (option "keys_index"): rows of its own, the prefix
  // and x as k_unpack forms them, capacity k4.cap
  KeyIndex kidx{GV_KIDX_ROW, true};
  hipEvent_t kidx_ev[2] = {nullptr, nullptr};     // time_kernels: around the last routed lookup's k_kidx_find
  hipEvent_t kidx_found = nullptr;                // the last gv_dev_keys_find on the context stream: the next pipelined
  bool kidx_found_used = false;                   // calls' FRONT streams wait for it (their sort / k_prep read its slots)
  // HBM held by the optional tables (G tables, key arenas) against ctx->opt.hbm_budget
  size_t opt_bytes = 0;
  // ring of per-launch stage events for gv_stage_stats
  static constexpr int kRing = 256;
  hipEvent_t ring[kRing][6] = {};                // start, after unpack / s^-1 / prep, ladder start, ladder end
  int ring_next = 0, ring_count = 0, last = -1;
  // ed25519: the resident comb table and one scratch set
  uint32_t* edtab = nullptr;
  uint32_t* edtab16 = nullptr;                    // the radix-2^16 comb table of B (k_ed_keyed), built on first use
  bool edtab16_failed = false;
  struct Ed {
    size_t cap = 0;                               // lanes
    uint8_t* d_in = nullptr;                      // pub32 | sig64 | off u64 | len u32 (ed_layout)
    uint32_t* atab = nullptr;                     // GV_ED_ROWS rows of cap words
    uint64_t* bits = nullptr;
    uint8_t* d_blob = nullptr;
    size_t blob_cap = 0;
    uint8_t* h_in = nullptr;
    size_t h_in_cap = 0;
    uint8_t* h_blob = nullptr;
    size_t h_blob_cap = 0;
    uint8_t* h_bits = nullptr;
    size_t h_bits_cap = 0;
    hipEvent_t last = nullptr;                    // end of the last work using the scratch
    hipStream_t last_st = nullptr;
  } ed;
  // ed25519 key arena (gv_ed_keys_load): per slot the comb table of -A
  // (GV_EDK_WORDS), the raw key words (8), the FromBytes verdict
  uint32_t *ektab = nullptr, *ekpub = nullptr, *ekok = nullptr;
  size_t ekcap = 0;
  // the wide ed25519 arena (option "ed_keys_wide"): per slot the radix-2^ekw_rb
  // comb of -A (ekw_rb 6: GV_EDK64_WORDS, 8: GV_EDK256_WORDS; the raw key and
  // the verdict stay in ekpub / ekok), capacity ekcapw, grown by doubling while
  // the HBM budget holds it; ekeysw leading slots built.  ekw_full: a growth or
  // a build failed (no more wide builds until gv_ed_keys_reset)
  uint32_t* ektabw = nullptr;
  size_t ekcapw = 0, ekeysw = 0;
  int ekw_rb = 0;
  bool ekw_full = false;
  // device-resident keyed ed25519 calls (gv_dev_verify_ed25519_msgs_keyed):
  // verdict bytes + slot-order sort scratch, and the event behind the last
  // kernel that reads it and the arena (the arena's writers wait for it)
  uint8_t* edkd_s = nullptr;
  size_t edkd_s_cap = 0;
  hipEvent_t edkd_last = nullptr;
  hipStream_t edkd_last_st = nullptr;
  // the ed25519 arena's pubkey index (option "ed_keys_index"): its rows are the
  // arena's ekpub rows (ensure_ed_keys keeps ed_kidx.rows == ekpub)
  KeyIndex ed_kidx{GV_KIDX_ROW_ED, false};
  uint8_t* edl_h = nullptr;                      // small keyed ed25519 batches: pinned inputs + verdicts (zero-copy)
  size_t edl_h_cap = 0;
  // ed25519 in-batch key grouping: per-batch key arena (comb tables of -A), pinned count, stats
  uint32_t *edg_ktab = nullptr, *edg_kpub = nullptr, *edg_kok = nullptr;
  size_t edg_cap = 0;
  size_t edg_words = 0;                           // table words per key of edg_ktab (the comb radix in use)
  uint32_t* ed_h_count = nullptr;
  uint64_t ed_grouped_batches = 0, ed_grouped_keys = 0;
  // large keyed ed25519 batches, two buffers (chunk i on set[i % 2]'s stream):
  // pinned staging, device copy, slot-order sort scratch (words)
  uint8_t *edk_h[2] = {nullptr, nullptr}, *edk_d[2] = {nullptr, nullptr};
  size_t edk_h_cap[2] = {0, 0}, edk_d_cap[2] = {0, 0};
  uint32_t* edk_s[2] = {nullptr, nullptr};
  size_t edk_s_cap[2] = {0, 0};
  std::mutex mu;
  Pool* pool = nullptr;                           // staging memcpy threads of this device (owned)
  Worker* worker = nullptr;                       // slice runner (devices 1..n-1 of a context)
  // pipelined device-resident calls on the context stream (gv_dev_verify_*,
  // stream NULL): the front kernels of call k+1 run under call k's ladder
  hipStream_t lo_st[2] = {nullptr, nullptr};
  hipStream_t hi_st[2] = {nullptr, nullptr};      // the ladders of set 0 / set 1 (two_ladders), else hi_st[0]
  hipEvent_t hi_done[2] = {nullptr, nullptr};     // the last ladder enqueued on hi_st[j]
  hipEvent_t bits_ev[2] = {nullptr, nullptr};     // the bitmap write of the last pipelined call of set j
  hipEvent_t bits_wait = nullptr, bits_rec = nullptr;   // the pipelined call being launched (dev_run -> launch)
  hipEvent_t plain_done = nullptr;                // the last non-pipelined call on the context stream
  bool hi_used[2] = {false, false}, plain_used = false, bits_used = false;
  uint64_t grouped_batches = 0, grouped_keys = 0;  // in-batch key grouping taken (gv_group_stats)
  int group_layout = 0;                           // groups per key of the last grouped call's tables ("group_layout")
  uint64_t routes[GV_ROUTES] = {};                // batches per schedule (gv_route_stats)
  int flip = 0;
  double last_slice_ms = 0;                       // host-buffer calls: this device's slice, wall time
  size_t last_slice_n = 0;
};

int ensure_cap(Set* s, size_t C) {
  if (C <= s->cap) return GV_OK;
  if (s->scratch) { (void)hipFree(s->scratch); s->scratch = nullptr; s->cap = 0; }
  const size_t in_bytes = in_layout(C, false, true).total + C * 32;
  const size_t bytes = in_bytes + C * kLaneWords * 4 + (C / 64) * 8 + 16 * 256;
  if (hipMalloc(&s->scratch, bytes) != hipSuccess) return GV_ENOMEM;
  uint8_t* p = s->scratch;
  auto take = [&](size_t nbytes) { uint8_t* r = p; p += round_up(nbytes, 256); return r; };
  s->d_in = take(in_bytes);
  s->in_x = (uint32_t*)take(C * 8 * 4);
  s->in_pfx = (uint32_t*)take(C * 4);
  s->in_r = (uint32_t*)take(C * 8 * 4);
  s->in_s = (uint32_t*)take(C * 8 * 4);
  s->in_e = (uint32_t*)take(C * 8 * 4);
  s->digits = (uint32_t*)take(C * GV_DIGIT_ROWS * 4);
  s->zq = (uint32_t*)take(C * 8 * 4);
  s->flags = (uint32_t*)take(C * 4);
  s->qtab = (uint32_t*)take(C * GV_QTAB_WORDS * 4);
  s->bits = (uint64_t*)take((C / 64) * 8);
  s->cap = C;
  return GV_OK;
}

int ensure_blob(Set* s, size_t bytes) {
  if (bytes <= s->blob_cap) return GV_OK;
  if (s->d_blob) (void)hipFree(s->d_blob);
  s->blob_cap = round_up(std::max<size_t>(bytes, 1), 1 << 20);
  if (hipMalloc(&s->d_blob, s->blob_cap) != hipSuccess) { s->blob_cap = 0; s->d_blob = nullptr; return GV_ENOMEM; }
  return GV_OK;
}

int ensure_pinned(uint8_t** p, size_t* cap, size_t bytes) {
  if (bytes <= *cap) return GV_OK;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t want = round_up(std::max<size_t>(bytes, 4096), 1 << 20);
  if (hipHostMalloc((void**)p, want, hipHostMallocDefault) != hipSuccess) { *p = nullptr; return GV_ENOMEM; }
  *cap = want;
  return GV_OK;
}

// Order work on stream st after the previous use of set s (any stream).
int set_acquire(Set* s, hipStream_t st) {
  if (s->last_st && s->last_st != st) CK(hipStreamWaitEvent(st, s->last, 0));
  return GV_OK;
}
int set_release(Set* s, hipStream_t st) {
  CK(hipEventRecord(s->last, st));
  s->last_st = st;
  return GV_OK;
}

// Grow the key arena to hold `need` slots, keeping the first `used` (the
// growth rule: arena_grow_cap, to key_cap -- GV_KEY_CAP or the "key_cap"
// option -- by doubling).
// k6: the arena also holds the kn group tables (allocated on the first k6
// load; *k6 is cleared when they do not fit the budget, the k4 tables stay).
// A failed copy leaves the arena as it was.
int ensure_keys(Dev* d, size_t need, size_t used, hipStream_t st, size_t key_cap, size_t budget, bool* k6) {
  const bool want6 = k6 && *k6, has6 = d->kn.qt != nullptr;
  if (need <= d->k4.cap && (!want6 || has6)) return GV_OK;
  const size_t cap = need > d->k4.cap ? arena_grow_cap(d->k4.cap, need, key_cap, 4096) : d->k4.cap;
  bool alloc6 = want6 || has6;
  // budget: the new arena beside the old one during the copy, plus the other
  // optional tables
  const size_t old_b = d->k4.cap * resident_slot_bytes(has6);
  const size_t base_b = budget_replace(d->opt_bytes, old_b, 0);
  if (base_b + old_b + cap * resident_slot_bytes(alloc6) > budget) {
    if (!alloc6 || has6 || base_b + old_b + cap * resident_slot_bytes(false) > budget) return GV_ENOMEM;
    alloc6 = false;                             // no room for the k6 tables: k4 only
    *k6 = false;
    if (need <= d->k4.cap) return GV_OK;
  }
  KeyTabs k4, kn;
  if (!k4.alloc(lay_k4(), cap, true)) return GV_ENOMEM;
  if (alloc6 && !kn.alloc(lay_kn(), cap, false)) { k4.free(); return GV_ENOMEM; }
  // the k6 tables of the slots below `used` exist only if the old arena had them
  if (used && (!k4.copy_from(d->k4, used, st) || (has6 && !kn.copy_from(d->kn, used, st)) ||
               hipStreamSynchronize(st) != hipSuccess)) {
    k4.free();
    kn.free();
    return GV_EHIP;
  }
  d->k4.free();
  d->kn.free();
  d->k4 = k4;
  d->kn = kn;
  d->opt_bytes = base_b + cap * resident_slot_bytes(alloc6);
  return GV_OK;
}

// Grow the wide-window arena (layout d->kw.lay) to `need` slots keeping the
// first `used`, as ensure_keys.  Returns false when the budget (the new arena
// beside the old one during the copy) does not hold it, when it would take
// device memory the k4 / k6 arena needs to grow to key_cap (plus 8 GiB of
// batch scratch: these tables are an optimisation and never make a later
// gv_keys_load or batch fail), or when an allocation fails: the arena is left
// as it was and batches keep the k6 tables.  Option "keys_wide1_cap" (a test
// hook) bounds the capacity of the GV_KW_QW-bit one-window layout,
// "keys_wide_mb" the new arena's bytes (0: no bound).  The ed25519 key
// arena's growth to ed_key_cap is reserved too (72 KB per key).
bool ensure_keys_wide(const gvopt::Options& opt, Dev* d, size_t need, size_t used, hipStream_t st) {
  KeyTabs& kw = d->kw;
  if (need <= kw.cap) return true;
  const size_t key_cap = opt.key_cap, limit = opt.keys_wide_bytes;
  const size_t cap = arena_grow_cap(kw.cap, need, key_cap, 4096);
  const size_t slot_b = slot_bytes(kw.lay);
  if (kw.lay == lay_wide(GV_KW_QW, GV_KW_NG1) && cap > opt.keys_wide1_cap) return false;
  if (limit && cap * slot_b > limit) return false;
  if (d->opt_bytes + cap * slot_b > opt.hbm_budget) return false;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
  const size_t reserve = (key_cap > d->k4.cap ? key_cap - d->k4.cap : 0) * resident_slot_bytes(true) +
                         (opt.ed_key_cap > d->ekcap ? opt.ed_key_cap - d->ekcap : 0) *
                             ((size_t)GV_EDK_WORDS + 8 + 1) * 4 +
                         (size_t(8) << 30);
  if (free_b < cap * slot_b + reserve) return false;
  KeyTabs grown;
  if (!grown.alloc(kw.lay, cap, false)) return false;
  used = std::min(used, d->keysw);                // the slots whose wide-window tables exist
  if (used && (!grown.copy_from(kw, used, st) || hipStreamSynchronize(st) != hipSuccess)) {
    grown.free();
    (void)hipGetLastError();
    return false;
  }
  d->opt_bytes = budget_replace(d->opt_bytes, kw.cap * slot_b, cap * slot_b);
  kw.free();
  kw = grown;
  return true;
}

// Drop the wide-window arena (its memory back to the device); the next one's layout is l.
void free_keys_wide(Dev* d, const TabLayout& l) {
  d->opt_bytes = budget_replace(d->opt_bytes, d->kw.cap * slot_bytes(d->kw.lay), 0);
  d->kw.free();
  d->kw.lay = l;
  d->keysw = 0;
}

// ---- ed25519 scratch
struct EdLayout {
  size_t sig, off, len, total;
};
EdLayout ed_layout(size_t C) {                    // C % 256 == 0: every part 256-aligned
  EdLayout L;
  L.sig = C * 32;
  L.off = L.sig + C * 64;
  L.len = L.off + C * 8;
  L.total = L.len + C * 4;
  return L;
}

int ed_ensure(Dev* d, size_t C, hipStream_t st) {
  if (!d->edtab) {                                // one-time: the comb table, built on the device
    if (hipMalloc(&d->edtab, (size_t)GV_ED_BTAB_WORDS * 4) != hipSuccess) { d->edtab = nullptr; return GV_ENOMEM; }
    CK(gvk_ed_btab(d->edtab, st));
    CK(hipStreamSynchronize(st));
  }
  if (!d->ed.last) CK(hipEventCreateWithFlags(&d->ed.last, hipEventDisableTiming));
  if (C <= d->ed.cap) return GV_OK;
  if (d->ed.last_st) CK(hipEventSynchronize(d->ed.last));
  if (d->ed.d_in) (void)hipFree(d->ed.d_in);
  if (d->ed.atab) (void)hipFree(d->ed.atab);
  if (d->ed.bits) (void)hipFree(d->ed.bits);
  d->ed.d_in = nullptr; d->ed.atab = nullptr; d->ed.bits = nullptr; d->ed.cap = 0;
  if (hipMalloc(&d->ed.d_in, ed_layout(C).total) != hipSuccess ||
      hipMalloc(&d->ed.atab, C * (size_t)GV_ED_ROWS * 4) != hipSuccess ||
      hipMalloc(&d->ed.bits, C / 8) != hipSuccess)
    return GV_ENOMEM;
  d->ed.cap = C;
  return GV_OK;
}

// One k_ed_verify launch over n items (device pointers) on stream st.
// ed25519 in-batch key grouping (option "ed_group"): batches of at least
// `min` items with at most items / `div` (and `cap`) distinct keys build each
// key's comb table once (k_ed_keys into a per-batch arena) and verify on
// k_ed_keyed; else the throughput kernels.
struct EdGroupCfg {
  bool on;
  size_t min;
  int div;
  size_t cap;
  bool sorted;
  bool split_keys;   // k_ed_keys_chain + k_ed_keys_tab (the table adds off the serial chain)
  bool btab16;       // k_ed_keyed takes [s]B from the radix-2^16 table
  bool r64;          // the per-batch key tables are radix-64 combs (43 windows of 32 entries)
};

// The radix-2^16 comb table of B, built on the device on first use (56.6 MB);
// null when the option is off or its allocation failed (k_ed_keyed then adds
// [s]B from the radix-256 table: same verdicts).
const uint32_t* ed_btab16(Dev* d, bool on, hipStream_t st) {
  if (!on) return nullptr;
  if (!d->edtab16 && !d->edtab16_failed) {
    uint32_t* t = nullptr;
    if (hipMalloc(&t, GV_ED_BTAB16_WORDS * 4) != hipSuccess) {
      (void)hipGetLastError();
      d->edtab16_failed = true;
    } else if (gvk_ed_btab16(t, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
      (void)hipFree(t);
      (void)hipGetLastError();
      d->edtab16_failed = true;
    } else {
      d->edtab16 = t;
    }
  }
  return d->edtab16;
}

// One small-batch ed25519 launch (k_ed_lat_sl / k_ed_lat_unc) of n items
// against d's radix-16 key arena of kcount slots.
gvk_edl fill_edl(const Dev* d, size_t n, size_t kcount, const uint32_t* slot, const uint8_t* sig, const uint8_t* blob,
                 const uint64_t* off, const uint32_t* len, uint8_t* out8) {
  gvk_edl b;
  memset(&b, 0, sizeof b);
  b.n = (uint32_t)n;
  b.slot = slot;
  b.sig64 = sig;
  b.msg_blob = blob;
  b.msg_off = off;
  b.msg_len = len;
  b.ktab = d->ektab;
  b.kpub = d->ekpub;
  b.kok = d->ekok;
  b.kcount = (uint32_t)kcount;
  b.btab = d->edtab;
  b.out8 = out8;
  return b;
}

int ensure_edg(Dev* d, size_t need, size_t words) {
  if (need <= d->edg_cap && words == d->edg_words) return GV_OK;
  for (uint32_t** q : {&d->edg_ktab, &d->edg_kpub, &d->edg_kok})
    if (*q) { (void)hipFree(*q); *q = nullptr; }
  d->edg_cap = 0;
  d->edg_words = words;
  const size_t cap = round_up(std::max<size_t>(need, 1024), 1024);
  if (hipMalloc(&d->edg_ktab, cap * words * 4) != hipSuccess ||
      hipMalloc(&d->edg_kpub, cap * 8 * 4) != hipSuccess || hipMalloc(&d->edg_kok, cap * 4) != hipSuccess)
    return GV_ENOMEM;
  d->edg_cap = cap;
  return GV_OK;
}

gvk_edk fill_edk(gv_ctx* ctx, const Dev* d, size_t n, size_t kcount, const uint32_t* perm, const uint32_t* slot,
                 const uint8_t* sig, const uint8_t* blob, const uint64_t* off, const uint32_t* len, uint8_t* out8,
                 const uint32_t* btab16);          // below gv_ctx

// The grouped route on the device (scratch: the per-lane table region, which
// the keyed kernel does not use).  *taken = false: the batch has too many
// distinct keys (or no room) and the caller runs the throughput kernels.
int ed_grouped(Dev* d, size_t n, const uint8_t* pub, const uint8_t* sig, const uint8_t* blob, const uint64_t* off,
               const uint32_t* len, uint64_t* bits, hipStream_t st, const EdGroupCfg& gc, bool* taken) {
  *taken = false;
  const size_t C = round_up(n, 256);
  size_t T = 512;
  while (T < 2 * n) T <<= 1;
  const size_t capU = std::min(gc.cap, std::max<size_t>(n / (size_t)gc.div, 1));
  const size_t nb = capU + 1, tb = gvk_sort_temp_bytes((uint32_t)nb);
  uint32_t* q = d->ed.atab;
  uint32_t *table = q, *rep = table + T, *uid = rep + C, *slot = uid + C, *count = slot + C;
  uint8_t* kpub32 = (uint8_t*)(count + 64);
  uint32_t* sp = count + 64 + round_up(capU * 8, 64);
  const gvk_sort so = carve_sort(sp, C, nb, tb);
  uint32_t* o8 = sp + sort_words(C, nb, tb);
  if ((size_t)(o8 + C / 4 - q) > C * (size_t)GV_ED_ROWS) return GV_OK;
  if (!d->ed_h_count && hipHostMalloc((void**)&d->ed_h_count, 64, hipHostMallocDefault) != hipSuccess) {
    d->ed_h_count = nullptr;
    return GV_ENOMEM;
  }
  CK(gvk_ed_group((uint32_t)n, pub, table, (uint32_t)T, rep, uid, count, (uint32_t)capU, kpub32, slot, st));
  CK(hipMemcpyAsync(d->ed_h_count, count, 4, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  const size_t U = *d->ed_h_count;
  if (U == 0 || U > capU || U * (size_t)gc.div > n) return GV_OK;
  uint32_t* wb = o8 + round_up(C / 4, 64);        // window-base scratch of the split key build
  if (!gc.split_keys || (size_t)(wb + U * 64 * 36 - q) > C * (size_t)GV_ED_ROWS) wb = nullptr;
  // radix-64 comb tables (43 additions per [h](-A) instead of 64) on the
  // split build; the one-lane build writes the radix-16 ones
  const int rb = gc.r64 && wb ? 6 : 4;
  int rc = ensure_edg(d, U, rb == 6 ? (size_t)GV_EDK64_WORDS : (size_t)GV_EDK_WORDS);
  if (rc) return rc == GV_ENOMEM ? GV_OK : rc;
  CK(gvk_ed_keys(kpub32, (uint32_t)U, 0u, nullptr, d->edg_ktab, d->edg_kpub, d->edg_kok, wb, rb, st));
  if (gc.sorted) CK(gvk_sort_slots(&so, (uint32_t)n, slot, (uint32_t)U, st));
  gvk_edk b = fill_edk(nullptr, d, n, U, gc.sorted ? so.perm : nullptr, slot, sig, blob, off, len, (uint8_t*)o8,
                       ed_btab16(d, gc.btab16, st));
  b.ktab = d->edg_ktab;                           // the per-batch arena
  b.kpub = d->edg_kpub;
  b.kok = d->edg_kok;
  b.rb = rb;
  CK(gvk_ed_keyed(&b, st));
  CK(gvk_ed_pack_bits((uint32_t)n, (const uint8_t*)o8, bits, st));
  d->ed_grouped_batches++;
  d->ed_grouped_keys += U;
  *taken = true;
  return GV_OK;
}

int ed_launch(bool timed, Dev* d, size_t n, const uint8_t* pub, const uint8_t* sig, const uint8_t* blob,
              const uint64_t* off, const uint32_t* len, uint64_t* bits, hipStream_t st, const EdGroupCfg& gc) {
  const size_t C = round_up(n, 256);
  int rc = ed_ensure(d, C, st);
  if (rc) return rc;
  if (d->ed.last_st && d->ed.last_st != st) CK(hipStreamWaitEvent(st, d->ed.last, 0));
  gvk_ed b;
  memset(&b, 0, sizeof b);
  b.n = (uint32_t)n;
  b.C = (uint32_t)C;
  b.pub32 = pub; b.sig64 = sig;
  b.msg_blob = blob; b.msg_off = off; b.msg_len = len;
  b.atab = d->ed.atab;
  b.btab = d->edtab;
  b.btab16 = ed_btab16(d, gc.btab16, st);
  b.bits = bits;
  hipEvent_t* rs = nullptr;
  if (timed) {                                    // stages: (none) x 3 | the ed25519 kernel
    rs = d->ring[d->ring_next];
    for (int i = 0; i < 6; ++i)
      if (!rs[i]) CK(hipEventCreate(&rs[i]));
    for (int i = 0; i < 5; ++i) CK(hipEventRecord(rs[i], st));
  }
  bool grouped = false;
  if (gc.on && n >= gc.min && (rc = ed_grouped(d, n, pub, sig, blob, off, len, bits, st, gc, &grouped))) return rc;
  if (!grouped) CK(gvk_ed_verify(&b, st));
  if (rs) {
    CK(hipEventRecord(rs[5], st));
    d->last = d->ring_next;
    d->ring_next = (d->ring_next + 1) % Dev::kRing;
    d->ring_count = std::min(d->ring_count + 1, Dev::kRing);
  }
  CK(hipEventRecord(d->ed.last, st));
  d->ed.last_st = st;
  return GV_OK;
}

}  // namespace

struct AsyncState;                               // gv_submit_* / gv_wait (below)

struct gv_ctx {
  std::vector<Dev*> devs;
  AsyncState* async = nullptr;                    // created by the first gv_submit_*
  gvopt::Options opt;                             // the tunables (gv_options.h)
  size_t keys = 0;              // key-arena slots in use (same on every device)
  std::atomic<uint64_t> keys_gen{0};  // gv_keys_reset calls
  std::atomic<uint64_t> keys_replaced{0};   // slots gv_keys_replace rewrote since gv_open ("keys_replaced")
  std::mutex keys_mu;
  KeyIndexStats kidx_stat;      // the arena's index: pub33 device batches (and the k_kidx_split / k_bits_merge launches)
  // ... routed with their non-resident items split off ("keys_index_split_calls"; they count in kidx_stat.hit
  // too), and those items ("keys_index_split_items")
  std::atomic<uint64_t> kidx_split_calls{0}, kidx_split_items{0};
  // the grouped route's key-table cache (option "group_reuse"): keys whose tables were reused / built by calls
  // with the option on, caches flushed, k_group_* launches ("group_reuse_hit", "_built", "_reset", "_launches")
  std::atomic<uint64_t> grp_hit{0}, grp_built{0}, grp_reset{0}, grp_launches{0};
  // ... and its layout promotion (option "group_promote"): sets moved to the kg layout / back to k4's
  std::atomic<uint64_t> grp_promoted{0}, grp_demoted{0};
  std::atomic<uint64_t> kidx_find_ns{0};             // time_kernels: the last routed lookup's k_kidx_find
  // ed25519 key arena (gv_ed_keys_load), same on every device
  size_t ed_keys = 0;
  std::atomic<uint64_t> ed_keys_gen{0};
  std::atomic<uint64_t> ed_keys_replaced{0};   // slots gv_ed_keys_replace rewrote since gv_open ("ed_keys_replaced")
  std::mutex ed_keys_mu;
  std::vector<uint8_t> ed_kpub;  // the raw keys per slot (large keyed batches run the throughput kernels on them)
  std::atomic<uint64_t> ed_keyed_wide{0};   // keyed batches / chunks that ran on wide tables since gv_open ("ed_keyed_wide")
  KeyIndexStats ed_kidx_stat;   // the ed25519 arena's index: pub32 device batches
};

namespace {

EdGroupCfg ed_group_cfg(const gv_ctx* ctx) {
  return EdGroupCfg{ctx->opt.ed_group, ctx->opt.ed_group_min, ctx->opt.ed_group_div, ctx->opt.ed_group_cap, ctx->opt.sort_keys,
                    ctx->opt.ed_keys_split, ctx->opt.ed_btab16, ctx->opt.ed_group_r64};
}

// k_ed_keyed reads d's wide tables when every slot of the arena has them
// (option "ed_keys_wide" still on), else the radix-16 ones.
bool ed_wide_serves(const gv_ctx* ctx, const Dev* d, size_t kcount) {
  return ctx->opt.ed_keys_wide && d->ektabw && d->ekw_rb && kcount && d->ekeysw >= kcount && d->ekcapw >= kcount;
}

// One k_ed_keyed batch of n items against d's ed25519 arena of kcount slots:
// its wide tables when they serve (counted in ed_keyed_wide), else the
// radix-16 ones.  ctx null (ed_grouped): the keys sit in the per-batch arena
// and the caller sets ktab / kpub / kok / rb.
gvk_edk fill_edk(gv_ctx* ctx, const Dev* d, size_t n, size_t kcount, const uint32_t* perm, const uint32_t* slot,
                 const uint8_t* sig, const uint8_t* blob, const uint64_t* off, const uint32_t* len, uint8_t* out8,
                 const uint32_t* btab16) {
  gvk_edk b;
  memset(&b, 0, sizeof b);
  b.n = (uint32_t)n;
  b.perm = perm;
  b.slot = slot;
  b.sig64 = sig;
  b.msg_blob = blob;
  b.msg_off = off;
  b.msg_len = len;
  b.kcount = (uint32_t)kcount;
  b.btab = d->edtab;
  b.btab16 = btab16;
  b.out8 = out8;
  if (!ctx) return b;
  const bool wide = ed_wide_serves(ctx, d, kcount);
  b.ktab = wide ? d->ektabw : d->ektab;
  b.rb = wide ? d->ekw_rb : 4;
  b.kpub = d->ekpub;
  b.kok = d->ekok;
  if (wide) ctx->ed_keyed_wide.fetch_add(1);
  return b;
}

// Optional device tables (the G tables past the 64 MiB GLV pair, the key
// arenas) are allocated against the context's HBM budget (gv_set_option
// "hbm_budget_mb", env GV_HBM_BUDGET_MB; default: whatever hipMalloc grants).
// A table that does not fit is remembered as failed and the batches take the
// schedule that needs less (k6 -> k4 -> the 125-doubling keyed ladder; the
// full-scalar G tables -> the GLV G windows) with the same verdicts.
uint32_t* opt_alloc(gv_ctx* ctx, Dev* d, size_t bytes) {
  if (d->opt_bytes + bytes > ctx->opt.hbm_budget) return nullptr;
  uint32_t* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  d->opt_bytes += bytes;
  return p;
}
void opt_free(Dev* d, uint32_t*& p, size_t bytes) {
  if (!p) return;
  (void)hipFree(p);
  p = nullptr;
  d->opt_bytes = budget_replace(d->opt_bytes, bytes, 0);
}
constexpr size_t kGtab4Bytes = (size_t)GV_KEY2_TABLES * 2 * GV_GTAB_N * 16 * 4;

// Build one G table set on stream st (set s is a scratch set with capacity >=
// 256: its flags rows hold the base points).  Enqueued only; the caller syncs.
template <class GEN>
int gen_table(Set* s, hipStream_t st, GEN&& gen) {
  int rc;
  if ((rc = ensure_cap(s, 256))) return rc;
  if ((rc = set_acquire(s, st))) return rc;
  if (gen(s->flags) != hipSuccess) return GV_EHIP;
  return set_release(s, st);
}

// The full-scalar G tables (GV_GF_WORDS, 6 GiB: k_ecmult_k4<true> and the
// per-item route's k_ecmult<false, true>), the 20-bit-window tables of 2^35 G,
// 2^70 G, 2^100 G and their lambda images (k_ecmult_k4, 192 MiB) and the k6
// ladder's full-scalar 24-bit-window tables (GV_K6_GTAB_WORDS, 3.5 GiB):
// built at gv_open on every device at once (gv_open: enqueue on each device,
// then one sync each; ~0.5 s), or on first use after an option switched a
// schedule on.  sync = false: enqueue only.
int ensure_gtabf(gv_ctx* ctx, Dev* d, Set* s, hipStream_t st, bool sync = true) {
  if (d->gtabf || !ctx->opt.gfull || d->gtabf_failed) return GV_OK;
  uint32_t* tf = opt_alloc(ctx, d, GV_GF_WORDS * 4);
  if (!tf) { d->gtabf_failed = true; return GV_OK; }
  int rc = gen_table(s, st, [&](uint32_t* sc) { return gvk_gen_gtablef(tf, sc, st); });
  if (!rc && sync && hipStreamSynchronize(st) != hipSuccess) rc = GV_EHIP;
  if (rc) { opt_free(d, tf, GV_GF_WORDS * 4); return rc; }
  d->gtabf = tf;
  return GV_OK;
}

int ensure_gtab4(gv_ctx* ctx, Dev* d, Set* s, hipStream_t st, bool sync = true) {
  if (!ctx->opt.keyed_k4) return GV_OK;
  if (!d->gtab4 && !d->gtab4_failed) {
    uint32_t* t4 = opt_alloc(ctx, d, kGtab4Bytes);
    if (!t4) {
      d->gtab4_failed = true;                   // keyed batches keep k_ecmult<true>
      return GV_OK;
    }
    int rc = gen_table(s, st, [&](uint32_t* sc) { return gvk_gen_gtable4(t4, sc, st); });
    if (!rc && sync && hipStreamSynchronize(st) != hipSuccess) rc = GV_EHIP;
    if (rc) { opt_free(d, t4, kGtab4Bytes); return rc; }
    d->gtab4 = t4;
  }
  return ensure_gtabf(ctx, d, s, st, sync);
}

// k_ecmult_k6's G tables.  A failure is remembered and keyed / grouped batches
// stay on k4.  `want`: the schedule is on (ctx->opt.k6 for the grouped route,
// ctx->opt.keys_k6 for the resident arena).
int ensure_gtab6(gv_ctx* ctx, Dev* d, Set* s, hipStream_t st, bool want, bool sync = true) {
  if (d->gtab6 || !want || d->gtab6_failed) return GV_OK;
  uint32_t* t6 = opt_alloc(ctx, d, GV_K6_GTAB_WORDS * 4);
  if (!t6) { d->gtab6_failed = true; return GV_OK; }
  int rc = gen_table(s, st, [&](uint32_t* sc) { return gvk_gen_gtable6(t6, sc, st); });
  if (!rc && sync && hipStreamSynchronize(st) != hipSuccess) rc = GV_EHIP;
  if (rc) { opt_free(d, t6, GV_K6_GTAB_WORDS * 4); return rc; }
  d->gtab6 = t6;
  return GV_OK;
}

// The set's per-batch key arena for in-batch grouping (cap keys in layout l:
// k4's, the grouped k6 one or a kg one), charged to the HBM budget like the
// other optional tables -- and, per key, its raw row and its share of the
// cache's table (group_bytes).
size_t group_held(const Set* s) { return s->gk.cap ? group_bytes(s->gk.cap, s->gk.lay) : 0; }
// The arena at hand serves this layout: the one it was allocated for, or --
// an arena allocated by a layout promotion (g_wide) -- k4's four groups, whose
// rows (qi * 3 + grp - 1; Z rows (grp - 1) * 8 * kC) index a prefix of the
// larger allocation: a demoted set frees and allocates nothing.
bool group_arena_fits(const Set* s, size_t cap, const TabLayout& l) {
  const TabLayout& h = s->gk.lay;
  return cap <= s->gk.cap && l.table_words() == h.table_words() &&
         (l.ng == h.ng || (s->g_wide && l.ng == GV_LGRP && l.ng < h.ng));
}
int ensure_group_arena(gv_ctx* ctx, Dev* d, Set* s, size_t cap, const TabLayout& l) {
  if (group_arena_fits(s, cap, l)) return GV_OK;
  d->opt_bytes = budget_replace(d->opt_bytes, group_held(s), 0);
  s->gk.free();
  if (s->g_rows) { (void)hipFree(s->g_rows); s->g_rows = nullptr; }
  s->g_idx = nullptr;
  s->g_live = false;                              // a new allocation holds no tables
  s->g_count = 0;
  s->g_wide = false;                              // (group_keys marks a promotion's allocation)
  s->gk.lay = l;
  const size_t T = kidx_table_words(cap);
  if (d->opt_bytes + group_bytes(cap, l) > ctx->opt.hbm_budget) return GV_ENOMEM;
  if (!s->gk.alloc(l, cap, true)) return GV_ENOMEM;
  if (hipMalloc(&s->g_rows, (cap * GV_KIDX_ROW + T) * 4) != hipSuccess) {
    (void)hipGetLastError();
    s->gk.free();
    s->g_rows = nullptr;
    return GV_ENOMEM;
  }
  s->g_T = T;
  s->g_idx = s->g_rows + cap * GV_KIDX_ROW;
  d->opt_bytes += group_bytes(cap, l);
  return GV_OK;
}

// group_keys' rows at the head of the set's per-lane Q-table region q (unused
// by the keyed pipeline; the pub33 pipeline rewrites it) for a batch of n
// items, C lanes, at most capU distinct keys: the dedupe's rows and table (T
// words), the distinct keys' (x, prefix) -- with group_reuse each key's cache
// row, the keys missed and their (x, prefix) gathered dense for the build --
// then the key-table build's scratch rows (gvk_keys_scratch_words): room words.
struct GroupScratch {
  size_t T, room;
  uint32_t *rep, *uid, *kslot, *count, *table, *kx, *kpfx, *krow, *miss, *mx, *mpfx, *sc;
};
GroupScratch carve_group(uint32_t* q, size_t C, size_t n, size_t capU, bool reuse) {
  GroupScratch g;
  g.T = kidx_table_words(n);
  g.rep = q; g.uid = q + C; g.kslot = q + 2 * C; g.count = q + 3 * C; g.table = q + 3 * C + 256;
  g.kx = g.table + g.T; g.kpfx = g.kx + 8 * capU;
  g.krow = g.kpfx + capU; g.miss = g.krow + capU; g.mx = g.miss + capU; g.mpfx = g.mx + 8 * capU;
  g.sc = reuse ? g.mpfx + capU : g.kpfx + capU;
  const size_t used = (size_t)(g.sc - q), total = (size_t)GV_QTAB_WORDS * C;
  g.room = used < total ? total - used : 0;
  return g;
}

// The layout of a grouped call's tables: kg (5-bit windows over kgng groups) >
// k6 (6-bit, 4 groups) > k4, each needing gtab6 (kg, k6) and its arena within
// the HBM budget -- or, the caller having chosen none, the set's own
// (group_promote; pc: its constants, null: off): a promoted set stays on the
// kg layout unless this call's lookup (looked) missed more keys than the
// break-even (a cold call rebuilds in the kg layout: the flag describes the
// key stream); a k4 set promotes on a large enough warm call behind two warm
// calls, all three below half the break-even.  The set's arena then holds
// capU keys of c->lay for the schedule c->route -- or, route -1, no arena (it
// was freed first: the cache is dropped): the batch takes the pub33 pipeline.
struct GroupChoice {
  TabLayout lay;
  int route = -1;
};
int choose_group_layout(gv_ctx* ctx, Dev* d, Set* s, hipStream_t st, size_t n, size_t capU, size_t room,
                        const PromoteCost* pc, bool looked, size_t missed, GroupChoice* c) {
  int rc = GV_OK;
  const bool k6_room = gvk_keys_scratch_words((uint32_t)capU, 4, GV_K6_NT, 0) <= room;
  const int kgng = ctx->opt.kg, png = ctx->opt.group_promote;   // 0 or one of GV_KG_NGS
  const bool kg_room = kgng && gvk_keys_scratch_words((uint32_t)capU, kgng, GV_QTAB_N, 0) <= room;
  bool promo = false;                             // the kg layout by promotion
  if (s->g_promoted)
    promo = pc && !(looked && promote_above_down(*pc, missed, n));
  else if (pc && !s->g_promo_refused && !d->gtab6_failed)
    promo = n >= ctx->opt.group_promote_min && (s->g_hist & 3) == 3 && looked && promote_below_up(*pc, missed, n);
  const int kgsel = promo ? png : kg_room ? kgng : 0;   // the kg layout this call tries (0: none)
  if (((ctx->opt.k6 && k6_room) || kgsel) && (rc = ensure_gtab6(ctx, d, s, st, true))) return rc;
  // the arena for the set's whole capacity when the budget holds it: a later,
  // larger chunk on this set does not regrow it (hipFree waits for the device)
  const size_t capA = round_up(std::max<size_t>(s->cap / ctx->opt.group_div, 256), 256);
  auto arena = [&](const TabLayout& l) {
    if (capA > capU && !group_arena_fits(s, capA, l)) {
      const int r = ensure_group_arena(ctx, d, s, capA, l);
      if (r != GV_ENOMEM) return r;
    }
    return ensure_group_arena(ctx, d, s, capU, l);
  };
  bool kg = kgsel && d->gtab6;
  // a promotion's arena is asked of the budget before the k4 arena is given
  // up: a refusal leaves the set, its tables and the route as they were
  if (kg && promo && !group_arena_fits(s, capU, lay_kg(png)) &&
      budget_replace(d->opt_bytes, group_held(s), group_bytes(capU, lay_kg(png))) > ctx->opt.hbm_budget)
    kg = false;
  if (kg && (rc = arena(lay_kg(kgsel)))) {
    if (rc != GV_ENOMEM) return rc;
    kg = false;                                 // no room for kgsel groups
  }
  if (promo) {
    if (kg) s->g_wide = true;                   // (k4's rows fit the allocation: a demotion keeps it)
    if (kg && !s->g_promoted) {
      s->g_promoted = true;
      ctx->grp_promoted++;
    } else if (!kg && !s->g_promoted) {
      s->g_promo_refused = true;                // no gtab6 or no memory: k4, and no retry until a quiescing option
    }
  }
  if (s->g_promoted && !(promo && kg)) {        // back to k4: flushed by the caller (another schedule's tables)
    s->g_promoted = false;
    s->g_hist = 0;
    ctx->grp_demoted++;
  }
  bool k6 = !kg && ctx->opt.k6 && k6_room && d->gtab6;
  if (k6 && (rc = arena(lay_k6()))) {
    if (rc != GV_ENOMEM) return rc;
    k6 = false;                                 // no room for the 32-entry tables: k4
  }
  if (!kg && !k6 && (rc = ensure_gtab4(ctx, d, s, st))) return rc;
  // a k4 arena that has to be allocated anyway, for a batch that could promote
  // its set later, is sized for the promoted layout when the budget holds it
  // (k4's rows take a prefix): the promotion then frees and allocates nothing
  // (hipFree drains the device, and 2.5 GB of arena per 1M-item set took up
  // to ~0.1 s to map: profiles/r07/group_promote/session_b_shapes/)
  if (!kg && !k6 && pc && !s->g_promoted && !s->g_promo_refused && !d->gtab6_failed &&
      n >= ctx->opt.group_promote_min && !group_arena_fits(s, capU, lay_k4())) {
    rc = arena(lay_kg(png));
    if (!rc) s->g_wide = true;
    else if (rc != GV_ENOMEM) return rc;
  }
  if (!kg && !k6 && (rc = arena(lay_k4()))) return rc == GV_ENOMEM ? GV_OK : rc;
  c->lay = kg ? lay_kg(kgsel) : k6 ? lay_k6() : lay_k4();
  c->route = kg ? GV_ROUTE_KG : k6 ? GV_ROUTE_K6 : GV_ROUTE_K4;
  return GV_OK;
}

// In-batch key grouping for a pub33 throughput batch of n items (b prepared
// for the pub33 pipeline, inputs on the device): the SoA rows are unpacked,
// the items grouped by key (k_dedupe*), and when the batch has at most
// n / group_div distinct keys their tables are built once into the set's
// batch arena and b is switched to the keyed pipeline with the key's arena
// row as slot (*view: the tables as b got them).  Scratch: carve_group.  One
// read-back (the distinct-key count and, with it, the count of keys the set's
// cache does not hold) decides the route and what is built.
//
// group_reuse: the arena's rows [0, g_count) keep the
// tables of the keys of earlier batches on this set.  k_group_find looks the
// batch's distinct keys up before the read-back; the keys it missed are built
// into rows [g_count, g_count + M) and entered (k_group_put), and the items'
// slots are the rows (k_group_map).  When the rows do not fit, or the tables
// at hand are another schedule's, the cache is flushed: this call builds all
// its keys into rows [0, U) as a call without the option does, and enters
// them.  g_count is committed once every launch is enqueued; an error on the
// way leaves the cache dropped (the next call starts cold).
//
// group_promote: choose_group_layout, gv_keytabs.h.
int group_keys(gv_ctx* ctx, Dev* d, Set* s, gvk_batch& b, size_t n, hipStream_t st, uint32_t** used_end = nullptr,
               KeyView* view = nullptr) {
  const size_t C = b.C;
  const size_t capU = round_up(std::max<size_t>(C / ctx->opt.group_div, 256), 256);
  const bool reuse = ctx->opt.group_reuse;
  const uint64_t seed = ctx->opt.kidx_seed;
  const GroupScratch g = carve_group(s->qtab, C, n, capU, reuse);
  if (gvk_keys_scratch_words((uint32_t)capU, GV_LGRP, GV_QTAB_N, 0) > g.room) return GV_OK;   // no room: pub33
  // layout promotion: the caller chose no layout ("kg", "k6"), the cache is on
  // and the promoted layout's build fits the scratch
  const int png = ctx->opt.group_promote;
  const PromoteCost* pc = png && !ctx->opt.kg && !ctx->opt.k6 && reuse ? promote_cost(png) : nullptr;
  if (pc && gvk_keys_scratch_words((uint32_t)capU, png, GV_QTAB_N, 0) > g.room) pc = nullptr;
  if (!s->h_count && hipHostMalloc((void**)&s->h_count, 64, hipHostMallocDefault) != hipSuccess) {
    s->h_count = nullptr;
    return GV_ENOMEM;
  }
  int rc = GV_OK;
  // the key rows only: the signature / digest rows follow in gvk_verify, in
  // item order or (keyed, key-ordered lanes) in slot order
  CK(gvk_unpack(b.pub33, nullptr, nullptr, (uint32_t)n, (uint32_t)C, b.in_x, b.in_pfx, b.in_r, b.in_s, b.in_e, st));
  b.unpacked = 2;
  if (!reuse) s->g_live = false;                  // this call overwrites rows [0, U)
  const bool looked = reuse && s->g_live && s->g_seed == seed;
  // (a lookup in flight: the items' slots follow the decision, in one pass -- k_group_map)
  CK(gvk_dedupe((uint32_t)n, (uint32_t)C, b.in_x, b.in_pfx, g.table, (uint32_t)g.T, g.rep, g.uid, g.count,
                looked ? nullptr : g.kslot, (uint32_t)capU, (uint32_t)capU, g.kx, g.kpfx, st));
  // a failure from here on drops the cache, unless the batch leaves for the
  // pub33 pipeline with the arena untouched (keep) or all is enqueued (commit)
  struct Drop {
    Set* s;
    bool armed;
    ~Drop() { if (armed) s->g_live = false; }
  } drop{s, false};
  if (looked) {
    drop.armed = true;                            // (count[1], the misses: cleared by gvk_dedupe)
    CK(gvk_group_find(s->g_idx, (uint32_t)s->g_T, s->g_rows, (uint32_t)s->g_count, seed, g.kx, g.kpfx,
                      (uint32_t)capU, g.count, (uint32_t)capU, g.krow, g.miss, g.count + 1, st));
    ctx->grp_launches++;
  }
  CK(hipMemcpyAsync(s->h_count, g.count, looked ? 8 : 4, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  const size_t U = *s->h_count;
  auto keep = [&] { drop.armed = false; return GV_OK; };
  if (U == 0 || U * ctx->opt.group_div > n || U > capU) return keep();   // many distinct keys: the pub33 pipeline
  GroupChoice ch;
  if ((rc = choose_group_layout(ctx, d, s, st, n, capU, g.room, pc, looked, looked ? s->h_count[1] : U, &ch))) return rc;
  const int route = ch.route;
  if (route < 0) return GV_OK;
  const bool kg = route == GV_ROUTE_KG, k6 = route == GV_ROUTE_K6;
  const KeyTabs& gk = s->gk;
  // what is built, and where: the keys the lookup missed behind the rows in
  // use, or -- a cold, flushed or switched-off cache -- every key from row 0
  const uint32_t kC = (uint32_t)(reuse ? gk.cap : capU);
  bool append = looked && s->g_live && s->g_route == route;   // (g_live: the arena was not reallocated above)
  if (append && s->g_count + s->h_count[1] > gk.cap) append = false;
  const size_t M = append ? s->h_count[1] : U, base = append ? s->g_count : 0;
  const uint32_t *bx = append ? g.mx : g.kx, *bpfx = append ? g.mpfx : g.kpfx;
  if (reuse) {
    drop.armed = true;
    if (!append) {
      if (s->g_live && s->g_count) ctx->grp_reset++;
      s->g_live = false;
      CK(hipMemsetAsync(s->g_idx, 0xFF, s->g_T * 4, st));
    }
    CK(gvk_group_put(s->g_idx, (uint32_t)s->g_T, s->g_rows, seed, g.kx, g.kpfx, (uint32_t)capU,
                     append ? g.miss : nullptr, (uint32_t)M, (uint32_t)base, append ? g.mx : nullptr,
                     append ? g.mpfx : nullptr, st));
    if (M) ctx->grp_launches += 2;
    if (looked) {
      CK(gvk_group_map((uint32_t)n, g.rep, g.uid, append ? g.krow : nullptr, g.kslot, st));
      ctx->grp_launches++;
    }
  }
  const int nt = (int)ch.lay.nt, ng = (int)ch.lay.ng;
  int with_qe = 0;
  KeyView v(gk, base + M);
  v.kC = kC;
  v.lay = ch.lay;
  if (M) {
    // the tables are built on the set's side stream while k_scalar_inv (which
    // does not read keys) runs on st: both are one wave per SIMD or so
    CK(hipEventRecord(s->fork, st));
    CK(hipStreamWaitEvent(s->side, s->fork, 0));
    // the forward pass's entries in coalesced scratch rows after the ratio and
    // E rows, when they fit (else through the tables themselves)
    with_qe = ctx->opt.keys_scratch && gvk_keys_scratch_words((uint32_t)M, ng, nt, 1) <= g.room ? 1 : 0;
    if (kg)
      CK(gvk_keys_build_rows_kg((uint32_t)M, (uint32_t)capU, bx, bpfx, g.sc, with_qe, (uint32_t)base, gk.qt, gk.zq, kC,
                                gk.ok, gk.qt2, gk.zq2, ng, s->side));
    else
      CK((k6 ? gvk_keys_build_rows6 : gvk_keys_build_rows)((uint32_t)M, (uint32_t)capU, bx, bpfx, g.sc, with_qe,
                                                          (uint32_t)base, gk.qt, gk.zq, kC, gk.ok, gk.qt2, gk.zq2, s->side));
    CK(hipEventRecord(s->keys_done, s->side));
    v.ready = s->keys_done;
  } else {
    // nothing to build: the rows were built on the side stream by earlier
    // calls on this set, whose ladders waited for them -- and so does this one,
    // should such a call have failed before its ladder was enqueued
    CK(hipStreamWaitEvent(st, s->keys_done, 0));
  }
  if (used_end) *used_end = g.sc + (M ? gvk_keys_scratch_words((uint32_t)M, ng, nt, with_qe) : 0);
  v.gtab4 = d->gtab4;
  v.gtab6 = d->gtab6;
  v.k6 = kg ? ng : k6 ? 4 : 0;
  v.kqw = kg ? 2 : 0;
  v.to_batch(b, g.kslot);
  b.gtabf = ctx->opt.gfull ? d->gtabf : nullptr;    // built by ensure_gtab4 above on first use
  if (view) *view = v;
  if (reuse) {                                  // everything is enqueued: the cache now holds these rows
    s->g_count = base + M;
    s->g_route = route;
    s->g_lng = ng;
    s->g_seed = seed;
    s->g_live = true;
    ctx->grp_hit += U - M;
    ctx->grp_built += M;
  }
  // the promotion rule's history: this call on the k4 layout, warm and below T_up
  s->g_hist = pc && route == GV_ROUTE_K4 ? (s->g_hist << 1 | (append && promote_below_up(*pc, M, n) ? 1u : 0u)) & 3u : 0u;
  d->group_layout = ng;
  drop.armed = false;
  d->grouped_batches++;
  d->grouped_keys += M;
  return GV_OK;
}

// Key-ordered lanes (gv_sort.hip) for a keyed k4 batch: scratch from word
// `base` of the set's Q-table region (unused by the keyed pipeline past the
// grouping rows); no room or the option off: item order.
void plan_sort(gv_ctx* ctx, Set* s, gvk_batch& b, uint32_t* base) {
  if (!ctx->opt.sort_keys || !b.kslot || !(b.gtab4 || (b.k6 && b.gtab6))) return;
  const size_t C = b.C, nb = (size_t)b.kcount + 1;
  const size_t tb = gvk_sort_temp_bytes((uint32_t)nb);
  uint32_t* p = s->qtab + round_up((size_t)(base - s->qtab), 64);
  gvk_sort so = carve_sort(p, C, nb, tb);
  p += sort_words(C, nb, tb);
  so.bits = (uint64_t*)p; p += C / 32;            // the slot-ordered accept bits, behind the scan scratch
  if ((size_t)(p - s->qtab) > (size_t)GV_QTAB_WORDS * C) return;
  b.srt = so;
}

// ---- the key arenas' pubkey index (KeyIndex above; gv_kidx.h;
// kidx_table_words: gv_keytabs.h).  One set of functions serves d->kidx and
// d->ed_kidx; the callers hold the arena's locks (d->mu; the ed25519 arena's
// ed_keys_mu before it, and they have waited for edkd_last).
constexpr size_t kKidxCntBytes = 256;

void kidx_free(Dev* d, KeyIndex& ix) {
  opt_free(d, ix.own_rows ? ix.rows : ix.tab, ix.bytes());   // (own rows: one block, the table behind them)
  ix.tab = nullptr;
  ix.cap = ix.T = 0;
}
// No index on this device until the arena's reset: every call takes the routes
// it takes without one.
void kidx_stop(Dev* d, KeyIndex& ix) {
  (void)hipGetLastError();
  kidx_free(d, ix);
  ix.failed = true;
  ix.keys = 0;
  ix.left_out = 0;
}
// The arena is empty again (its reset, or a load from slot 0): so is the
// index -- the next load from slot 0 clears the table -- and a stopped one may
// start again.
void kidx_reset(KeyIndex& ix) {
  ix.keys = 0;
  ix.left_out = 0;
  ix.failed = false;
}
// The index covers its arena of `count` slots as it stands (an empty arena:
// every key misses).  enabled: the arena's option now.
bool kidx_live(const KeyIndex& ix, bool enabled, size_t count) {
  if (!enabled || ix.failed || ix.keys != count) return false;
  return count == 0 || (ix.on && ix.tab);
}
bool kidx_live(const gv_ctx* ctx, const Dev* d) { return kidx_live(d->kidx, ctx->opt.keys_index, ctx->keys); }
bool ed_kidx_live(const gv_ctx* ctx, const Dev* d) {
  return kidx_live(d->ed_kidx, ctx->opt.ed_keys_index, ctx->ed_keys);
}

// The counters and the pinned word, once per device.
int kidx_setup(gv_ctx* ctx, Dev* d, KeyIndex& ix, hipStream_t st) {
  if (!ix.cnt) {
    if (!(ix.cnt = opt_alloc(ctx, d, kKidxCntBytes))) return GV_ENOMEM;
    CK(hipMemsetAsync(ix.cnt, 0, kKidxCntBytes, st));
  }
  if (!ix.h && hipHostMalloc((void**)&ix.h, 64, hipHostMallocDefault) != hipSuccess) {
    ix.h = nullptr;
    return GV_ENOMEM;
  }
  return GV_OK;
}

// Slots base.. (or d_slots[g]) enter the table from their rows; a launch counts.
hipError_t kidx_put(KeyIndex& ix, size_t n, size_t base, const uint32_t* d_slots, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const hipError_t e = gvk_kidx_put(ix.row, ix.tab, (uint32_t)ix.T, ix.rows, (uint32_t)n, (uint32_t)base, d_slots,
                                    *ix.seed, ix.cnt, st);
  if (e == hipSuccess) ix.stat->launches++;
  return e;
}
// k_kidx_find over the arena's first `count` slots (the caller counts the launch).
hipError_t kidx_find(const KeyIndex& ix, size_t count, const uint8_t* d_keys, size_t n, uint32_t* d_out,
                     uint32_t* d_miss, hipStream_t st) {
  return gvk_kidx_find(ix.row, ix.tab, (uint32_t)ix.T, ix.rows, (uint32_t)count, *ix.seed, d_keys, (uint32_t)n, d_out,
                       d_miss, st);
}

// Empty the table and enter slots [0, count) from their rows.
int kidx_refill(KeyIndex& ix, size_t count, hipStream_t st) {
  CK(hipMemsetAsync(ix.tab, 0xFF, ix.T * 4, st));
  CK(hipMemsetAsync(ix.cnt, 0, 4, st));
  CK(kidx_put(ix, count, 0, nullptr, st));
  return GV_OK;
}
// The keys the table's last fill and the appends since left out.
int kidx_read_left_out(KeyIndex& ix, hipStream_t st) {
  CK(hipMemcpyAsync(ix.h + 8, ix.cnt, 4, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  ix.left_out = ix.h[8];
  return GV_OK;
}
// After a replacement rewrote rows: the table again from the first `count`
// rows -- the old bytes leave it, and the order of replacements does not
// matter -- or no index.
void kidx_refilled(Dev* d, KeyIndex& ix, size_t count, hipStream_t st) {
  if (kidx_refill(ix, count, st) != GV_OK || kidx_read_left_out(ix, st) != GV_OK) kidx_stop(d, ix);
}
// A load that wrote the slots [base, base + n) also enters them into the
// index while every earlier slot is in it (enabled: the arena's option now);
// the arena's own load then decides kidx_stop or keys = base + n: a refused
// allocation or a failed launch only stops the index on this device.
bool kidx_appendable(const KeyIndex& ix, bool enabled, size_t base) {
  return enabled && ix.on && !ix.failed && ix.keys == base;
}

// The secp256k1 index's rows and table for the arena's capacity (d->k4.cap),
// charged to the HBM budget like the other optional tables.  On growth the
// rows of the first `used` slots are copied and the table refilled from them.
int kidx_ensure(gv_ctx* ctx, Dev* d, size_t used, hipStream_t st) {
  KeyIndex& ix = d->kidx;
  int rc;
  if ((rc = kidx_setup(ctx, d, ix, st))) return rc;
  if (ix.rows && ix.cap >= d->k4.cap) return GV_OK;
  const size_t cap = d->k4.cap, T = kidx_table_words(cap), bytes = (cap * ix.row + T) * 4;
  if (T > (size_t(1) << 31)) return GV_ENOMEM;
  uint32_t* rows = opt_alloc(ctx, d, bytes);                  // one block: the rows, then the table
  if (!rows) return GV_ENOMEM;
  used = ix.rows ? std::min(used, ix.keys) : 0;
  if (used && (hipMemcpyAsync(rows, ix.rows, used * ix.row * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
               hipStreamSynchronize(st) != hipSuccess)) {
    opt_free(d, rows, bytes);
    return GV_EHIP;
  }
  kidx_free(d, ix);
  ix.rows = rows; ix.tab = rows + cap * ix.row; ix.cap = cap; ix.T = T;
  return kidx_refill(ix, used, st);
}

// The slots of a device batch of keys (n items, device AoS) into `out` (n
// words): k_kidx_find on st, then one 4-byte read-back of the miss count and
// a sync -- what group_keys pays for its key count.  *nmiss: the items whose
// key was not found (their word of `out` is GV_KIDX_EMPTY).  ev (may be null):
// two events recorded around the kernel.
int kidx_lookup(KeyIndex& ix, size_t count, size_t n, const uint8_t* pub, uint32_t* out, hipStream_t st, size_t* nmiss,
                hipEvent_t* ev) {
  uint32_t* miss = ix.cnt + 16;
  CK(hipMemsetAsync(miss, 0, 4, st));
  if (ev) CK(hipEventRecord(ev[0], st));
  CK(kidx_find(ix, count, pub, n, out, miss, st));
  ix.stat->launches++;
  if (ev) CK(hipEventRecord(ev[1], st));
  CK(hipMemcpyAsync(ix.h, miss, 4, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  *nmiss = *ix.h;
  return GV_OK;
}
// ... of a pub33 batch, timed with "time_kernels" on ("keys_index_find_ns").
int kidx_lookup33(gv_ctx* ctx, Dev* d, size_t n, const uint8_t* pub, uint32_t* out, hipStream_t st, size_t* nmiss) {
  const bool timed = ctx->opt.time_kernels;
  if (timed)
    for (hipEvent_t& e : d->kidx_ev)
      if (!e) CK(hipEventCreate(&e));
  int rc;
  if ((rc = kidx_lookup(d->kidx, ctx->keys, n, pub, out, st, nmiss, timed ? d->kidx_ev : nullptr))) return rc;
  if (timed) {
    float ms = 0;
    CK(hipEventElapsedTime(&ms, d->kidx_ev[0], d->kidx_ev[1]));
    ctx->kidx_find_ns = (uint64_t)(ms * 1e6f);
  }
  return GV_OK;
}

// gv_keys_find / gv_ed_keys_find on a live index of `count` slots: the n host
// keys staged, looked up and the slots read back, in scratch of the call's
// own.  The launch counts even when the call fails.
int kidx_find_host(Dev* d, KeyIndex& ix, size_t count, size_t n, const uint8_t* pub, uint32_t* slot_out) {
  if (count == 0) {
    memset(slot_out, 0xFF, n * 4);
    return GV_OK;
  }
  CK(hipSetDevice(d->id));
  hipStream_t st = d->set[0].st;
  uint8_t* buf = nullptr;
  const size_t kb = ix.key_bytes(), pb = round_up(n * kb, 256);
  if (hipMalloc(&buf, pb + n * 4) != hipSuccess) return GV_ENOMEM;
  int rc = GV_OK;
  if (hipMemcpyAsync(buf, pub, n * kb, hipMemcpyHostToDevice, st) != hipSuccess ||
      kidx_find(ix, count, buf, n, (uint32_t*)(buf + pb), nullptr, st) != hipSuccess ||
      hipMemcpyAsync(slot_out, buf + pb, n * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    rc = GV_EHIP;
  ix.stat->launches++;
  (void)hipFree(buf);
  return rc;
}

// The sub-batch buffers and the scratch set of a call on set s that splits
// `miss` non-resident items off (option "keys_index_split"): false when the
// HBM budget or hipMalloc refuses them -- the call then falls through whole.
// The buffers grow by kidx_split_rows; the scratch set as launch() will ask.
size_t grow_items(const gv_ctx* ctx, size_t C);
bool miss_ensure(gv_ctx* ctx, Dev* d, Set* s, size_t miss) {
  if (!s->miss_done && hipEventCreateWithFlags(&s->miss_done, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    s->miss_done = nullptr;
    return false;
  }
  if (!s->miss_set) {
    Set* m = new Set;
    if (hipEventCreateWithFlags(&m->last, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      delete m;
      return false;
    }
    s->miss_set = m;
  }
  const size_t rows = kidx_split_rows(s->miss.cap, miss);
  if (rows != s->miss.cap) {
    opt_free(d, s->miss_buf, kidx_split_layout(s->miss.cap).total);
    s->miss = gvk_split{};
    const SplitLayout L = kidx_split_layout(rows);
    if (rows > kMaxItems || !(s->miss_buf = opt_alloc(ctx, d, L.total))) return false;
    uint8_t* p = (uint8_t*)s->miss_buf;
    gvk_split& m = s->miss;
    m.cap = (uint32_t)rows;
    m.count = (uint32_t*)p;
    m.idx = (uint32_t*)(p + L.idx);
    m.pub33 = p + L.pub; m.sig64 = p + L.sig; m.dig32 = p + L.third;
    m.off = (uint64_t*)(p + L.third); m.len = (uint32_t*)(p + L.len);
    m.bits = (uint64_t*)(p + L.bits);
  }
  if (ensure_cap(s->miss_set, grow_items(ctx, round_up(miss, 256))) != GV_OK) {
    (void)hipGetLastError();
    return false;
  }
  return true;
}

// A chunk past the ramp's first size grows its set straight to a whole
// max_batch chunk (device scratch, pinned staging, the grouping arena): a
// regrowth costs tens of ms (hipFree waits for the device, pinning pages), so
// it happens once -- not again when a larger chunk, a queued whole slice or a
// host-buffer call follows device-resident calls of another size.
size_t grow_items(const gv_ctx* ctx, size_t C) {
  return ctx->opt.pipe_chunk && C > ctx->opt.pipe_chunk ? std::max(C, round_up(ctx->opt.max_batch, 256)) : C;
}

// The tables of the resident arena (gv_keys_load) that serve a keyed batch:
// the wide-window ones when every slot in use has them (their own arena: Z
// rows of stride kw.cap) and the caller's schedule reads their layout
// (wide_ok), else the kn ones when every slot has those (kn_ok), else k4's.
KeyView arena_tabs(const gv_ctx* ctx, const Dev* d, bool wide_ok, bool kn_ok = true) {
  KeyView v(d->k4, ctx->keys);
  if (wide_ok && ctx->opt.keys_wide && d->kw.qt && d->kw.lay.ng && d->gtab6 && d->keysw >= ctx->keys) {
    v = KeyView(d->kw, ctx->keys, d->k4.ok);
    v.kn = kTabsWide; v.k6 = (int)v.lay.ng; v.kqw = 1; v.kwq = v.lay.qw(); v.gtab6 = d->gtab6;
  } else if (kn_ok && ctx->opt.keys_k6 && d->kn.qt && d->gtab6 && d->keys6 >= ctx->keys) {
    v = KeyView(d->kn, ctx->keys, d->k4.ok);
    v.kn = kTabsKn; v.k6 = GV_KN_ARENA_NG; v.gtab6 = d->gtab6;
  }
  v.gtab4 = d->gtab4;
  return v;
}

// What launch() verifies: n items by key bytes (pub33) or by slot (kslot) of
// the resident arena or of `ka`, digests (dig32) or messages (blob, off, len).
struct Items {
  size_t n = 0;
  const uint8_t* pub33 = nullptr;
  const uint32_t* kslot = nullptr;
  const uint8_t *sig64 = nullptr, *dig32 = nullptr, *blob = nullptr;
  const uint64_t* off = nullptr;
  const uint32_t* len = nullptr;
  const KeyView* ka = nullptr;                    // a host slice's grouped keys, which kslot then indexes
  bool no_group = false;                          // the per-item pub33 pipeline whatever the keys repeat
  bool index = false;                             // pub33 throughput batches may route through the pubkey index
  bool quiet = false;                             // no stage events (a split call's sub-batch: the ring describes the main batch)
};
// Where the verdicts go: the accept bitmap (device) or, on the sliced
// small-batch kernels, one byte per item (out8).  st_ecm (pipelined
// device-resident calls): the ladder runs there, after the front kernels on
// st; the set's scratch is released on st_ecm.
struct LaunchOut {
  uint64_t* bits = nullptr;
  uint8_t* out8 = nullptr;
  hipStream_t st_ecm = nullptr;
};

// Launch the pipeline for the items, whose inputs already sit on the device
// (or in pinned host memory), on set s's scratch, stream st.  The caller
// holds d->mu.
int launch(gv_ctx* ctx, Dev* d, Set* s, const Items& it, const LaunchOut& out, hipStream_t st) {
  const size_t n = it.n;
  const uint32_t* kslot = it.kslot;             // (or the index's slots, below)
  const KeyView* ka = it.ka;
  if (n == 0 || n > kMaxItems) return GV_EINVAL;
  const size_t C = round_up(n, 256);
  int rc = ensure_cap(s, grow_items(ctx, C));
  if (rc) return rc;
  if (kslot && !ka) {                           // the arena always exists for a keyed batch
    rc = ensure_keys(d, 1, ctx->keys, st, ctx->opt.key_cap, ctx->opt.hbm_budget, nullptr);
    if (rc) return rc;
  }
  rc = set_acquire(s, st);
  if (rc) return rc;
  gvk_batch b;
  memset(&b, 0, sizeof b);
  b.n = (uint32_t)n; b.C = (uint32_t)C;
  b.pub33 = it.pub33; b.sig64 = it.sig64; b.dig32 = it.dig32;
  b.msg_blob = it.blob; b.msg_off = it.off; b.msg_len = it.len;
  b.gtab = d->gtab;
  b.gtabf = ctx->opt.gfull ? d->gtabf : nullptr;
  b.in_x = s->in_x; b.in_pfx = s->in_pfx; b.in_r = s->in_r; b.in_s = s->in_s; b.in_e = s->in_e;
  b.digits = s->digits; b.zq = s->zq; b.flags = s->flags; b.qtab = s->qtab;
  b.bits = out.bits;
  b.inv_m = ctx->opt.inv_small ? 0u : (uint32_t)GV_INV_M;
  // index (gv_dev_verify_digests / _msgs, option "keys_index"): a throughput
  // batch whose keys are all resident runs as the keyed call with those slots
  // would -- the slots looked up into the head of the set's Q-table region
  // (free on the keyed pipeline; plan_sort starts past them).  A few misses
  // (option "keys_index_split", kidx_split_ok): the batch still runs keyed,
  // its miss lanes (slot GV_KIDX_EMPTY: out of range, answered 0) compacted
  // into a sub-batch that is verified below and merged in.  Any other miss:
  // the batch goes on as without the index.
  bool via_index = false;
  size_t split = 0;                             // the items split off
  if (it.index && it.pub33 && !kslot && n > ctx->opt.lat_max && ctx->keys && kidx_live(ctx, d)) {
    size_t nmiss = 0;
    if ((rc = kidx_lookup33(ctx, d, n, it.pub33, s->qtab, st, &nmiss))) return rc;
    const size_t bound = ctx->opt.keys_index_split;
    const bool wanted = kidx_split_ok(bound, nmiss, true, true);   // (the buffers are asked for only then)
    if (kidx_split_ok(bound, nmiss, true, wanted && miss_ensure(ctx, d, s, nmiss))) split = nmiss;
    via_index = nmiss == 0 || split;
    if (via_index) kslot = s->qtab;
    (via_index ? ctx->kidx_stat.hit : ctx->kidx_stat.miss)++;
    if (split) {
      CK(gvk_kidx_split(&s->miss, s->qtab, (uint32_t)n, it.pub33, it.sig64, it.dig32, it.off, it.len, st));
      ctx->kidx_stat.launches++;
      ctx->kidx_split_calls++;
      ctx->kidx_split_items += split;
    }
  }
  // a host slice's grouped keys (the slots are on the device already:
  // slice_group read the key count back after k_dedupe_map; only k_prep on
  // reads the tables, so the chunk's unpack / sort / s^-1 overlap the slice's
  // table build: ka->ready), or the resident arena's k4 tables
  const KeyView kv = !kslot ? KeyView() : ka ? *ka : arena_tabs(ctx, d, false, false);
  if (kslot) kv.to_batch(b, kslot);
  hipEvent_t* rs = nullptr;
  if (ctx->opt.time_kernels && !it.quiet) {
    rs = d->ring[d->ring_next];
    for (int i = 0; i < 6; ++i)
      if (!rs[i]) CK(hipEventCreate(&rs[i]));
    CK(hipEventRecord(rs[0], st));
    for (int i = 0; i < 3; ++i) b.ev[i] = rs[i + 1];
    b.ev_ecm_start = rs[4];
    b.ev[3] = rs[5];
  }
  // k6 group tables (a grouped slice's chunks) are read by k_ecmult_k6 only:
  // such a chunk takes the pipeline whatever its size
  const bool small = n <= (kslot ? ctx->opt.lat_max_keyed : ctx->opt.lat_max) && !b.k6 && !via_index;
  const bool pipelined = out.st_ecm != nullptr && !small;
  // the resident arena's wide or kn tables: throughput batches on
  // k_ecmult_kn / k_ecmult_k6 (the small-batch kernels choose below)
  if (kslot && !ka && !small) arena_tabs(ctx, d, true).to_batch(b, kslot);
  if (pipelined) {
    b.st_ecm = out.st_ecm;
    b.ecm_ready = s->ecm_ready;
    b.bits_wait = d->bits_wait;
    b.bits_done = split ? nullptr : d->bits_rec;   // (a split call: recorded behind the merge, below)
  }
  if (small) {
    // small batch: one fused kernel, several lanes per signature (gv_lat.hip)
    if (b.keys_ready) CK(hipStreamWaitEvent(st, b.keys_ready, 0));   // a host slice's tables
    gvk_lat lb;
    memset(&lb, 0, sizeof lb);
    lb.n = (uint32_t)n; lb.C = (uint32_t)C;
    lb.pub33 = it.pub33; lb.sig64 = it.sig64; lb.dig32 = it.dig32;
    lb.msg_blob = it.blob; lb.msg_off = it.off; lb.msg_len = it.len;
    lb.gtab = d->gtab; lb.e_soa = s->in_e; lb.bits = out.bits;
    lb.ev[0] = b.ev[0];
    if (!kslot && n <= ctx->opt.lat_rows_max) lb.gtab6 = d->gtab6;   // k_verify_lat_sl4 (null: not built)
    const bool sliced = ctx->opt.lat_sliced && n <= (kslot ? ctx->opt.lat_sl_max_keyed : ctx->opt.lat_sl_max);
    if (out.out8 && !sliced) return GV_EINVAL;  // byte verdicts: the sliced kernels only
    lb.out8 = out.out8;
    d->routes[kslot ? GV_ROUTE_LAT_KEYED : GV_ROUTE_LAT]++;
    if (kslot) {                                // keyed: 16 lanes per signature (group tables)
      // every slot has its GV_KW_QW-bit one-window wide tables:
      // k_verify_lat16_kw (no doublings); an arena of another layout, or
      // lat_kw off, takes the kn tables: k_verify_lat16_kn (6 doublings, G
      // from the 24-bit tables); else, or not sliced, k4's
      const bool kw1 = ctx->opt.lat_kw && d->kw.lay == lay_wide(GV_KW_QW, GV_KW_NG1);
      (sliced && !ka ? arena_tabs(ctx, d, kw1) : kv).to_lat(lb, kslot);
      lb.glat = d->glat;
      if (sliced) CK(gvk_verify_lat16_sl(&lb, st));
      else CK(gvk_verify_lat16(&lb, st));
    } else if (sliced) {
      CK(gvk_verify_lat_sl(&lb, st));
    } else {
      CK(gvk_verify_lat(&lb, st));
    }
    if (rs) {                                   // stages: SHA | fused kernel | (none) | (none)
      CK(hipEventRecord(rs[2], st));
      CK(hipEventRecord(rs[3], st));
      CK(hipEventRecord(rs[4], st));
      CK(hipEventRecord(rs[5], st));
    }
  } else {
    uint32_t* sort_base = s->qtab + (via_index ? C : 0);   // keyed: the Q-table region is free (past the looked-up slots)
    if (!kslot && it.pub33 && ctx->opt.group_keys && !it.no_group && n >= ctx->opt.group_min) {
      rc = group_keys(ctx, d, s, b, n, st, &sort_base);
      if (rc) return rc;
    }
    if (!b.kslot) {                               // the per-item route: G on the unsplit u1 (gfull_item)
      if (ctx->opt.gfull && ctx->opt.gfull_item && (rc = ensure_gtabf(ctx, d, s, st))) return rc;
      b.gtabf = ctx->opt.gfull && ctx->opt.gfull_item ? d->gtabf : nullptr;
    }
    plan_sort(ctx, s, b, sort_base);
    d->routes[b.kqw == 2 && b.gtab6               ? GV_ROUTE_KG
              : b.kqw && b.gtab6 && b.k6 == gvk_kw_ng(b.kwq, 2) ? GV_ROUTE_KW2
              : b.kqw && b.gtab6                ? GV_ROUTE_KW
              : b.k6 == GV_KN_ARENA_NG && b.gtab6 ? GV_ROUTE_KN
              : b.k6 && b.gtab6                ? GV_ROUTE_K6
              : b.kslot && b.gtab4 && b.gtabf ? GV_ROUTE_K4F
              : b.kslot && b.gtab4            ? GV_ROUTE_K4
              : b.kslot                       ? GV_ROUTE_KEYED125
              : b.gtabf                       ? GV_ROUTE_ITEMF
                                              : GV_ROUTE_PUB33]++;
    CK(gvk_verify(&b, st));
    if (split) {
      // the front stream is free again (the ladder runs on st_ecm): the
      // sub-batch goes under the main ladder as the next call's front kernels
      // would -- by its 33 key bytes, never grouped (no host sync), the call's
      // thresholds picking its kernel -- and the ladder stream ORs its accept
      // bits in behind its own bitmap write, before the event later calls'
      // bitmap writes wait for and before the set is released
      const gvk_split& m = s->miss;
      Items sub;
      sub.n = split;
      sub.pub33 = m.pub33; sub.sig64 = m.sig64;
      if (it.dig32) sub.dig32 = m.dig32;
      else { sub.blob = it.blob; sub.off = m.off; sub.len = m.len; }
      sub.no_group = true;
      sub.quiet = true;
      LaunchOut so;
      so.bits = m.bits;
      if ((rc = launch(ctx, d, s->miss_set, sub, so, st))) return rc;
      hipStream_t se = pipelined ? out.st_ecm : st;
      if (se != st) {
        CK(hipEventRecord(s->miss_done, st));
        CK(hipStreamWaitEvent(se, s->miss_done, 0));
      }
      CK(gvk_bits_merge(&m, (uint32_t)split, (uint32_t)n, out.bits, se));
      ctx->kidx_stat.launches++;
      if (pipelined && d->bits_rec) CK(hipEventRecord(d->bits_rec, se));
    }
  }
  if (rs) {
    d->last = d->ring_next;
    d->ring_next = (d->ring_next + 1) % Dev::kRing;
    d->ring_count = std::min(d->ring_count + 1, Dev::kRing);
  }
  return set_release(s, pipelined ? out.st_ecm : st);
}

// Device-resident calls.  A caller stream: everything on it, in order.  The
// context stream (stream NULL): batches past the small-batch bound are
// PIPELINED -- consecutive calls alternate the two scratch sets, their front
// kernels (unpack, s^-1, prep) go to the set's low-priority stream and every
// ladder to ONE high-priority stream, so call k+1's front kernels fill call
// k's ladder tail (the last ~1 ms of a 7 ms ladder runs below full occupancy)
// while the ladders stay in call order (their d_bits writes too).  Small
// batches and the other calls on the context stream are ordered after every
// pipelined ladder (hi_done) and the next ladder after them (plain_done).
void order_after_pipeline(Dev* d, hipStream_t st) {
  for (int j = 0; j < 2; ++j)
    if (d->hi_used[j]) (void)hipStreamWaitEvent(st, d->hi_done[j], 0);
}
template <class F>
int dev_run(gv_ctx* ctx, Dev* d, void* stream, size_t n, bool keyed, F&& fn) {
  if (stream) {
    order_after_pipeline(d, (hipStream_t)stream);
    return fn(&d->set[0], (hipStream_t)stream, (hipStream_t) nullptr);
  }
  if (!ctx->opt.pipeline_dev || n <= (keyed ? ctx->opt.lat_max_keyed : ctx->opt.lat_max)) {
    hipStream_t st = d->set[0].st;
    order_after_pipeline(d, st);
    const int rc = fn(&d->set[0], st, (hipStream_t) nullptr);
    if (rc) return rc;
    CK(hipEventRecord(d->plain_done, st));
    d->plain_used = true;
    return GV_OK;
  }
  const int j = d->flip;
  d->flip ^= 1;
  // two_ladders: set j's ladder on hi_st[j], so call k+1's ladder starts in
  // call k's tail (its front ran under call k's ladder); the bitmap writes
  // stay in call order through bits_ev.  Else one ladder stream.
  hipStream_t hs = d->hi_st[ctx->opt.two_ladders ? j : 0];
  hipEvent_t& hd = d->hi_done[ctx->opt.two_ladders ? j : 0];
  if (d->plain_used) CK(hipStreamWaitEvent(hs, d->plain_done, 0));
  // a gv_dev_keys_find enqueued on the context stream before this call: its
  // slots may be this call's d_slot, which the front kernels read
  if (d->kidx_found_used) CK(hipStreamWaitEvent(d->lo_st[j], d->kidx_found, 0));
  d->bits_wait = (ctx->opt.two_ladders && d->bits_used) ? d->bits_ev[j ^ 1] : nullptr;
  d->bits_rec = ctx->opt.two_ladders ? d->bits_ev[j] : nullptr;
  const int rc = fn(&d->set[j], d->lo_st[j], hs);
  d->bits_wait = d->bits_rec = nullptr;
  if (rc) return rc;
  CK(hipEventRecord(hd, hs));
  d->hi_used[ctx->opt.two_ladders ? j : 0] = true;
  d->bits_used = ctx->opt.two_ladders;
  return GV_OK;
}
// A device-resident secp256k1 batch: the items' verdicts into the bitmap d_bits.
int dev_launch(gv_ctx* ctx, Dev* d, void* stream, const Items& it, void* d_bits) {
  return dev_run(ctx, d, stream, it.n, it.kslot != nullptr, [&](Set* s, hipStream_t st, hipStream_t se) {
    LaunchOut out;
    out.bits = (uint64_t*)d_bits;
    out.st_ecm = se;
    return launch(ctx, d, s, it, out, st);
  });
}

struct HostBatch {
  const uint8_t *pub33, *sig64, *dig32, *blob;
  const uint64_t* off;
  const uint32_t* len;
  const uint32_t* slots;
  uint8_t* out_ok;
  uint64_t* out_bits;
  bool pinned = false;          // digest inputs in pinned host memory (gv_host_alloc): no staging copy
  const uint32_t* d_slots = nullptr;   // slice grouping: per-item key ids on the device (offset lo)
  const KeyView* ka = nullptr;         // ... and the arena they index
  size_t d_slots_lo = 0;
  bool plain = false;                  // the per-item pub33 pipeline, no in-batch grouping (a grouped
                                       // slice's first chunk, run while the slice's key tables build)
};

// Host memory the device can read directly (hipHostMalloc / gv_host_alloc /
// hipHostRegister), as opposed to pageable memory that must be staged.
bool is_pinned(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

// Harvest a finished chunk of set s into the caller's outputs.
int harvest(Dev* d, Set* s, const HostBatch& hb) {
  CK(hipEventSynchronize(s->done));
  const size_t c0 = s->c0, cn = s->cn, words = (cn + 63) / 64;
  if (s->zc) {                                  // zero-copy small batch: verdict bytes in h_out8
    if (hb.out_ok) {
      memcpy(hb.out_ok + c0, s->h_out8, cn);
    } else {                                    // c0 % 64 == 0
      for (size_t w = 0; w < words; ++w) {
        uint64_t v = 0;
        const size_t lim = std::min<size_t>(64, cn - 64 * w);
        for (size_t i = 0; i < lim; ++i) v |= (uint64_t)(s->h_out8[64 * w + i] & 1u) << i;
        hb.out_bits[c0 / 64 + w] = v;
      }
    }
    s->busy = false;
    return GV_OK;
  }
  if (hb.out_ok) {
    uint8_t* o = hb.out_ok + c0;
    const uint64_t* w = s->h_bits;
    // 8 verdict bytes per bitmap byte through a 256-entry table (lo % 64 == 0)
    static const std::array<uint64_t, 256> spread = [] {
      std::array<uint64_t, 256> t{};
      for (int v = 0; v < 256; ++v)
        for (int b = 0; b < 8; ++b) t[v] |= (uint64_t)((v >> b) & 1) << (8 * b);
      return t;
    }();
    auto unpack = [&](size_t lo, size_t hi) {
      const uint8_t* wb = (const uint8_t*)w;
      size_t i = lo;
      for (; i + 8 <= hi; i += 8) {
        const uint64_t v = spread[wb[i >> 3]];
        memcpy(o + i, &v, 8);
      }
      for (; i < hi; ++i) o[i] = (uint8_t)((w[i >> 6] >> (i & 63)) & 1u);
    };
    if (cn < (size_t(1) << 18)) unpack(0, cn);
    else {
      const int parts = d->pool->size();
      const size_t per = round_up((cn + parts - 1) / parts, 64);
      d->pool->run(parts, [&](int p) { unpack(std::min(cn, p * per), std::min(cn, (p + 1) * per)); });
    }
  } else {
    memcpy(hb.out_bits + c0 / 64, s->h_bits, words * 8);   // c0 % 64 == 0 (chunks are 256-aligned)
  }
  s->busy = false;
  return GV_OK;
}

// A host chunk's ladder runs on the set's ladder stream (below the front
// priority of the set streams), so the next chunk's front kernels -- and an
// asynchronously submitted batch's grouping and key tables -- take CU slots
// as this ladder's workgroups retire instead of queueing behind it (the
// device-resident pipeline's stream priorities, dev_run).  Small batches run
// one fused kernel on the set stream.
hipStream_t chunk_ladder(const gv_ctx* ctx, Set* s, size_t cn, bool keyed) {
  const size_t lmax = keyed ? ctx->opt.lat_max_keyed : ctx->opt.lat_max;
  return ctx->opt.host_ladder_stream && cn > lmax ? s->lad : nullptr;
}
// The set stream continues after the chunk's ladder (the bitmap's D2H).
int ladder_join(Set* s) {
  if (s->last_st != s->lad) return GV_OK;       // the ladder ran on the set stream
  CK(hipEventRecord(s->lad_done, s->lad));
  CK(hipStreamWaitEvent(s->st, s->lad_done, 0));
  return GV_OK;
}

// Stage chunk [c0, c0 + cn) of a host batch into set s and enqueue H2D ->
// kernels -> D2H of the bitmap on the set's stream.
int submit(gv_ctx* ctx, Dev* d, Set* s, size_t c0, size_t cn, const HostBatch& hb) {
  const size_t C = round_up(cn, 256);
  const bool dslots = hb.d_slots != nullptr;    // slice grouping: slots already on the device
  const bool keyed = hb.slots != nullptr || dslots, msgs = hb.dig32 == nullptr;
  const uint32_t* dsl = dslots ? hb.d_slots + (c0 - hb.d_slots_lo) : nullptr;
  const size_t grow_c = grow_items(ctx, C);   // (device scratch and pinned staging)
  int rc = ensure_cap(s, grow_c);
  if (rc) return rc;
  const InLayout L = in_layout(C, keyed, msgs);
  size_t hb_bytes = 0;
  if ((rc = ensure_pinned((uint8_t**)&s->h_bits, &s->h_bits_cap, (C / 64) * 8))) return rc;
  uint8_t* h = nullptr;                           // the staging buffer (not for the caller's pinned buffers)
  uint64_t bmin = 0;
  // h2d_serial: this chunk's copies start after the previous chunk's
  auto h2d_begin = [&]() -> int {
    if (ctx->opt.h2d_serial && d->last_h2d) CK(hipStreamWaitEvent(s->st, d->last_h2d, 0));
    return GV_OK;
  };
  auto h2d_end = [&]() -> int {
    CK(hipEventRecord(s->h2d, s->st));
    d->last_h2d = s->h2d;
    return GV_OK;
  };
  // zero-copy small batch: the sliced kernel reads pinned host memory (the
  // caller's buffers or the staging buffer; messages too: its scalar wave
  // hashes them) and writes one verdict byte per item to pinned memory (no
  // H2D / memset / D2H)
  const size_t lmax = keyed ? ctx->opt.lat_max_keyed : ctx->opt.lat_max;
  const size_t slmax = keyed ? ctx->opt.lat_sl_max_keyed : ctx->opt.lat_sl_max;
  const bool zc = ctx->opt.lat_zero_copy && ctx->opt.lat_sliced && cn <= slmax && cn <= lmax && !dslots;
  auto mark_busy = [&]() { s->busy = true; s->zc = zc; s->c0 = c0; s->cn = cn; return GV_OK; };
  // the chunk's items: keys or slots, signatures, and at `third` the digests
  // or (messages) the offsets with the lengths behind them as in_layout puts them
  auto items_at = [&](const uint8_t* key, const uint8_t* sig, const uint8_t* third, const uint8_t* blob) {
    Items it;
    it.n = cn;
    if (keyed) it.kslot = (const uint32_t*)key;
    else it.pub33 = key;
    it.sig64 = sig;
    if (msgs) {
      it.blob = blob;
      it.off = (const uint64_t*)third;
      it.len = (const uint32_t*)(third + (L.len - L.third));
    } else {
      it.dig32 = third;
    }
    return it;
  };
  auto run_zero_copy = [&](const Items& it) -> int {
    if ((rc = ensure_pinned(&s->h_out8, &s->h_out8_cap, cn))) return rc;
    LaunchOut out;
    out.out8 = s->h_out8;
    if ((rc = launch(ctx, d, s, it, out, s->st))) return rc;
    CK(hipEventRecord(s->done, s->st));
    return mark_busy();
  };
  // the inputs are in d_in (H2D enqueued): kernels, then the bitmap's D2H
  auto run_staged = [&]() -> int {
    const uint8_t* din = s->d_in;
    Items it = items_at(din, din + L.sig, din + L.third, s->d_blob);
    if (dslots) it.kslot = dsl;
    it.ka = hb.ka;
    it.no_group = hb.plain;
    LaunchOut out;
    out.bits = s->bits;
    out.st_ecm = chunk_ladder(ctx, s, cn, keyed);
    if ((rc = launch(ctx, d, s, it, out, s->st)) || (rc = ladder_join(s))) return rc;
    CK(hipMemcpyAsync(s->h_bits, s->bits, ((cn + 63) / 64) * 8, hipMemcpyDeviceToHost, s->st));
    CK(hipEventRecord(s->done, s->st));
    if ((rc = set_release(s, s->st))) return rc;
    return mark_busy();
  };
  if (hb.pinned && !msgs) {                 // the caller's pinned buffers: read in place, no staging
    const uint8_t* kp = keyed ? (const uint8_t*)(hb.slots + c0) : hb.pub33 + c0 * 33;
    const uint8_t* sp = hb.sig64 + c0 * 64;
    const uint8_t* dp = hb.dig32 + c0 * 32;
    if (zc) return run_zero_copy(items_at(kp, sp, dp, nullptr));
    if ((rc = set_acquire(s, s->st)) || (rc = h2d_begin())) return rc;
    if (!dslots) CK(hipMemcpyAsync(s->d_in, kp, cn * (keyed ? 4 : 33), hipMemcpyHostToDevice, s->st));
    CK(hipMemcpyAsync(s->d_in + L.sig, sp, cn * 64, hipMemcpyHostToDevice, s->st));
    CK(hipMemcpyAsync(s->d_in + L.third, dp, cn * 32, hipMemcpyHostToDevice, s->st));
    if ((rc = h2d_end())) return rc;
    return run_staged();
  }
  // (grown: room for the largest layout, pub33 + digests, so a plain chunk
  // after keyed ones does not regrow it either)
  const size_t stage_bytes = grow_c > C ? in_layout(grow_c, false, false).total : L.total;
  if ((rc = ensure_pinned(&s->h_in, &s->h_in_cap, stage_bytes))) return rc;
  h = s->h_in;
  bool sent = false;
  if (!msgs && !zc && ctx->opt.stage_pieces > 1 && cn >= 65536) {
    // large pageable chunk: staged in pieces, each piece's H2D right behind
    // its copy, so the transfer of piece i overlaps the staging of piece i+1
    if ((rc = set_acquire(s, s->st)) || (rc = h2d_begin())) return rc;
    const size_t per = round_up((cn + ctx->opt.stage_pieces - 1) / ctx->opt.stage_pieces, 256);
    const size_t kb = keyed ? 4 : 33;
    for (size_t a = 0; a < cn; a += per) {
      const size_t m = std::min(per, cn - a);
      const CopySeg segs[3] = {CopySeg{h + L.sig + a * 64, hb.sig64 + (c0 + a) * 64, m * 64},
                               CopySeg{h + L.third + a * 32, hb.dig32 + (c0 + a) * 32, m * 32},
                               keyed ? CopySeg{h + a * 4, (const uint8_t*)(hb.slots + c0 + a), m * 4}
                                     : CopySeg{h + a * 33, hb.pub33 + (c0 + a) * 33, m * 33}};
      par_copy_segs(d->pool, segs, dslots ? 2 : 3);
      if (!dslots) CK(hipMemcpyAsync(s->d_in + a * kb, h + a * kb, m * kb, hipMemcpyHostToDevice, s->st));
      CK(hipMemcpyAsync(s->d_in + L.sig + a * 64, h + L.sig + a * 64, m * 64, hipMemcpyHostToDevice, s->st));
      CK(hipMemcpyAsync(s->d_in + L.third + a * 32, h + L.third + a * 32, m * 32, hipMemcpyHostToDevice, s->st));
    }
    if ((rc = h2d_end())) return rc;
    sent = true;
  } else if (!msgs) {                       // keys/slots, signatures, digests: one pool pass
    const CopySeg segs[3] = {CopySeg{h + L.sig, hb.sig64 + c0 * 64, cn * 64},
                             CopySeg{h + L.third, hb.dig32 + c0 * 32, cn * 32},
                             keyed ? CopySeg{h, (const uint8_t*)(hb.slots + c0), cn * 4}
                                   : CopySeg{h, hb.pub33 + c0 * 33, cn * 33}};
    par_copy_segs(d->pool, segs, dslots ? 2 : 3);
  } else {
    if (dslots) {
    } else if (keyed) par_copy(d->pool, h, hb.slots + c0, cn * 4);
    else par_copy(d->pool, h, hb.pub33 + c0 * 33, cn * 33);
    par_copy(d->pool, h + L.sig, hb.sig64 + c0 * 64, cn * 64);
    const auto [lo, hi] = msg_range(hb.off, hb.len, c0, c0 + cn);
    bmin = lo;
    hb_bytes = hi - lo;
    uint64_t* ro = (uint64_t*)(h + L.third);
    for (size_t i = 0; i < cn; ++i) ro[i] = hb.off[c0 + i] - bmin;
    memcpy(h + L.len, hb.len + c0, cn * 4);
    if ((rc = ensure_pinned(&s->h_blob, &s->h_blob_cap, std::max<size_t>(hb_bytes, 1)))) return rc;
    if ((rc = ensure_blob(s, hb_bytes))) return rc;
    par_copy(d->pool, s->h_blob, hb.blob + bmin, hb_bytes);
  }
  if (zc) return run_zero_copy(items_at(h, h + L.sig, h + L.third, s->h_blob));
  if (!sent) {
    if ((rc = set_acquire(s, s->st)) || (rc = h2d_begin())) return rc;
    const size_t from = dslots ? L.sig : 0;   // device slots: no key region to send
    CK(hipMemcpyAsync(s->d_in + from, h + from, (msgs ? L.total : L.third + cn * 32) - from, hipMemcpyHostToDevice,
                      s->st));
    if (msgs && hb_bytes) CK(hipMemcpyAsync(s->d_blob, s->h_blob, hb_bytes, hipMemcpyHostToDevice, s->st));
    if ((rc = h2d_end())) return rc;
  } else if (msgs && hb_bytes) {
    CK(hipMemcpyAsync(s->d_blob, s->h_blob, hb_bytes, hipMemcpyHostToDevice, s->st));
  }
  return run_staged();
}

// Does a host slice repeat its keys enough for grouping?  Birthday count on a
// pseudo-random sample of m keys: at average multiplicity k the sample holds
// about m^2 (k - 1) / 2n repeated keys; take the route when a quarter of the
// count expected at k = group_div is there (a strided sample would miss
// round-robin key orders).
bool worth_grouping(const uint8_t* pub33, size_t n, int div) {
  const size_t m = std::min<size_t>(n, 4096);
  std::vector<uint64_t> h(m);
  uint64_t r = 0x9E3779B97F4A7C15ull;
  for (size_t i = 0; i < m; ++i) {
    r ^= r << 13; r ^= r >> 7; r ^= r << 17;
    const uint8_t* p = pub33 + (r % n) * 33;
    uint64_t v;
    memcpy(&v, p + 1, 8);
    h[i] = v ^ ((uint64_t)p[0] * 0xFF51AFD7ED558CCDull) ^ ((uint64_t)p[25] << 32 | p[32]);
  }
  std::sort(h.begin(), h.end());
  size_t dups = 0;
  for (size_t i = 1; i < m; ++i) dups += h[i] == h[i - 1];
  const double expect = (double)m * (double)m * (double)(div - 1) / (2.0 * (double)n);
  return (double)dups >= std::max(1.0, expect / 4);
}

// Whole-slice key grouping for a pub33 host slice [lo, lo + n): the slice's
// keys are sent once (pageable input staged in pieces, each piece's H2D right
// behind its copy), unpacked and grouped over the WHOLE slice -- so the key
// tables are built once per slice, not once per pipeline chunk -- and when
// the slice has few enough distinct keys the chunks then run keyed: only
// signatures and digests (or messages) travel per chunk, the slots stay on
// the device.  *ka is filled and *d_slots set when the route is taken.
int slice_group(gv_ctx* ctx, Dev* d, size_t lo, size_t n, const HostBatch& hb, KeyView* ka,
                const uint32_t** d_slots, Set* g) {
  *d_slots = nullptr;
  if (!worth_grouping(hb.pub33 + lo * 33, n, ctx->opt.group_div)) return GV_OK;
  const size_t C = round_up(n, 256);
  int rc = ensure_cap(g, grow_items(ctx, C));
  if (rc) return rc;
  if ((rc = set_acquire(g, g->st))) return rc;
  const uint8_t* src = hb.pub33 + lo * 33;
  if (hb.pinned) {
    CK(hipMemcpyAsync(g->d_in, src, n * 33, hipMemcpyHostToDevice, g->st));
  } else {
    if ((rc = ensure_pinned(&g->h_in, &g->h_in_cap, n * 33))) return rc;
    const size_t piece = round_up((n + 3) / 4, 256) * 33;
    for (size_t o = 0; o < n * 33; o += piece) {
      const size_t b = std::min(piece, n * 33 - o);
      par_copy(d->pool, g->h_in + o, src + o, b);
      CK(hipMemcpyAsync(g->d_in + o, g->h_in + o, b, hipMemcpyHostToDevice, g->st));
    }
  }
  gvk_batch b;
  memset(&b, 0, sizeof b);
  b.n = (uint32_t)n; b.C = (uint32_t)C;
  b.pub33 = g->d_in;
  b.in_x = g->in_x; b.in_pfx = g->in_pfx; b.in_r = g->in_r; b.in_s = g->in_s; b.in_e = g->in_e;
  if ((rc = group_keys(ctx, d, g, b, n, g->st, nullptr, ka))) return rc;
  if (!b.kslot) return set_release(g, g->st);   // many distinct keys after all: per-chunk pipeline
  if (b.keys_ready) CK(hipStreamWaitEvent(g->st, b.keys_ready, 0));   // (null: every key's tables were at hand)
  CK(hipEventRecord(g->grp_ready, g->st));
  ka->ready = g->grp_ready;                     // (the chunks wait for this, not for the build's own event)
  *d_slots = b.kslot;
  return GV_OK;   // the set stays acquired until run_slice releases it after the last chunk
}

std::vector<Worker*> workers(const gv_ctx* ctx) {
  std::vector<Worker*> w;
  for (Dev* d : ctx->devs) w.push_back(d->worker);
  return w;
}

// Chunk sizes of a host slice of `count` items.  Pipelined (past lat_max): a
// ramp -- pipe_chunk first, each later chunk at most pipe_growth times the one
// before -- so the first kernels start after a short staging copy and every
// later chunk is staged (pageable -> pinned copy, H2D) while the one before it
// computes.  Else equal chunks of at most max_batch.  Every chunk but the last
// is a multiple of 256 (harvest copies bitmap words).
std::vector<size_t> chunk_ramp(const gv_ctx* ctx, size_t count, bool pipelined, bool async = false) {
  std::vector<size_t> sz;
  if (pipelined) {
    const size_t first = async ? ctx->opt.async_chunk : ctx->opt.pipe_chunk;
    const size_t growth = async ? (size_t)ctx->opt.async_growth : (size_t)ctx->opt.pipe_growth;
    size_t c = std::min(first, ctx->opt.max_batch), left = count;
    while (left) {
      const size_t take = std::min(left, c);
      sz.push_back(take);
      left -= take;
      c = std::min(ctx->opt.max_batch, c * growth);
    }
    const size_t m = sz.size();             // a runt tail joins the chunk before it
    if (m >= 2 && 2 * sz[m - 1] < sz[m - 2] && sz[m - 1] + sz[m - 2] <= ctx->opt.max_batch) {
      sz[m - 2] += sz[m - 1];
      sz.pop_back();
    }
  } else {
    const size_t nch = (count + ctx->opt.max_batch - 1) / ctx->opt.max_batch;
    const size_t chunk = std::min(ctx->opt.max_batch, round_up((count + nch - 1) / nch, 256));
    for (size_t c0 = 0; c0 < count; c0 += chunk) sz.push_back(std::min(chunk, count - c0));
  }
  return sz;
}

// Verify items [lo, hi) of a host batch on one device: chunks alternate
// between the two sets so staging + H2D of one overlaps the kernels of the other.
int run_slice(gv_ctx* ctx, Dev* d, size_t lo, size_t hi, const HostBatch& hb) {
  std::lock_guard<std::mutex> lk(d->mu);
  CK(hipSetDevice(d->id));
  const size_t n = hi - lo;
  const auto t_begin = std::chrono::steady_clock::now();
  struct SliceTimer {
    Dev* d;
    size_t n;
    std::chrono::steady_clock::time_point t0;
    ~SliceTimer() {
      d->last_slice_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      d->last_slice_n = n;
    }
  } timer{d, n, t_begin};
  d->last_h2d = nullptr;                          // no earlier chunk of this slice
  const bool pipelined = n > (hb.slots ? ctx->opt.lat_max_keyed : ctx->opt.lat_max) && ctx->opt.pipe_chunk;
  auto chunk_sizes = [&](size_t count) { return chunk_ramp(ctx, count, pipelined); };
  std::vector<size_t> sizes = chunk_sizes(n);
  int rc = GV_OK;
  // a pub33 slice big enough for the pipeline: group its keys once for all chunks
  const bool try_group = hb.pub33 && !hb.slots && ctx->opt.group_keys && n >= ctx->opt.group_min && sizes.size() > 1;
  // ... and with slice_plain_first, its first items run the per-item pub33
  // pipeline (their own key parse and Q tables), submitted BEFORE the
  // grouping: their H2D and kernels run while the rest of the slice's keys
  // are sent, grouped and tabulated, so the GPU has ladder work from the
  // start instead of waiting for the key tables
  HostBatch hp = hb;
  hp.plain = true;
  const size_t np = try_group && pipelined && ctx->opt.slice_plain_first
                        ? std::min(round_up(ctx->opt.slice_plain_first, 256), round_up(n / 4, 256)) : 0;
  int k = 0;
  if (np) {
    if ((rc = submit(ctx, d, &d->set[0], lo, np, hp))) return rc;
    k = 1;
  }
  HostBatch hg = hb;
  KeyView ka;
  bool grouped = false;
  if (try_group) {
    const uint32_t* dsl = nullptr;
    rc = slice_group(ctx, d, lo + np, n - np, hb, &ka, &dsl, &d->gset[0]);
    if (rc == GV_OK && dsl) {
      grouped = true;
      hg.d_slots = dsl;
      hg.d_slots_lo = lo + np;
      hg.ka = &ka;
    }
  }
  const HostBatch& hr = grouped ? hg : hb;
  if (np) sizes = chunk_sizes(n - np);
  size_t c0 = lo + np;
  for (size_t i = 0; i < sizes.size() && rc == GV_OK; c0 += sizes[i], ++i, k ^= 1) {
    Set* s = &d->set[k];
    if (s->busy && (rc = harvest(d, s, hr))) break;
    rc = submit(ctx, d, s, c0, sizes[i], hr);
  }
  for (Set& s : d->set)                          // drain (also after an error)
    if (s.busy) {
      const int r2 = harvest(d, &s, hr);
      if (rc == GV_OK) rc = r2;
      s.busy = false;
    }
  if (grouped) {                                  // every chunk done: the slice's arena is free
    const int r2 = set_release(&d->gset[0], d->gset[0].st);
    if (rc == GV_OK) rc = r2;
  }
  return rc;
}

// ---- ed25519 host-buffer batches: chunks of at most ed_chunk items, staged
// through pinned memory on the device's first stream.
struct EdHost {
  const uint8_t* pub32;
  const uint8_t* sig64;
  const uint8_t* blob;
  const uint64_t* off;
  const uint32_t* len;
  uint8_t* out_ok;
};

int ed_slice(gv_ctx* ctx, Dev* d, size_t lo, size_t hi, const EdHost& hb) {
  std::lock_guard<std::mutex> lk(d->mu);
  CK(hipSetDevice(d->id));
  hipStream_t st = d->set[0].st;
  const size_t chunk = std::min<size_t>(ctx->opt.max_batch, 262144);
  for (size_t c0 = lo; c0 < hi; c0 += chunk) {
    const size_t cn = std::min(chunk, hi - c0), C = round_up(cn, 256);
    int rc = ed_ensure(d, C, st);
    if (rc) return rc;
    const EdLayout L = ed_layout(C);
    if ((rc = ensure_pinned(&d->ed.h_in, &d->ed.h_in_cap, L.total))) return rc;
    if ((rc = ensure_pinned(&d->ed.h_bits, &d->ed.h_bits_cap, C / 8))) return rc;
    if (d->ed.last_st) CK(hipEventSynchronize(d->ed.last));      // the staging buffers are free
    uint8_t* h = d->ed.h_in;
    const auto [lo_b, hi_b] = msg_range(hb.off, hb.len, c0, c0 + cn);
    const size_t nb = hi_b - lo_b;
    if ((rc = ensure_pinned(&d->ed.h_blob, &d->ed.h_blob_cap, nb))) return rc;
    if (nb > d->ed.blob_cap) {
      if (d->ed.d_blob) (void)hipFree(d->ed.d_blob);
      d->ed.blob_cap = round_up(nb, 1 << 20);
      if (hipMalloc(&d->ed.d_blob, d->ed.blob_cap) != hipSuccess) { d->ed.d_blob = nullptr; d->ed.blob_cap = 0; return GV_ENOMEM; }
    }
    if (!d->ed.d_blob) {
      d->ed.blob_cap = 1 << 20;
      if (hipMalloc(&d->ed.d_blob, d->ed.blob_cap) != hipSuccess) { d->ed.d_blob = nullptr; d->ed.blob_cap = 0; return GV_ENOMEM; }
    }
    const CopySeg segs[2] = {CopySeg{h, hb.pub32 + c0 * 32, cn * 32}, CopySeg{h + L.sig, hb.sig64 + c0 * 64, cn * 64}};
    par_copy_segs(d->pool, segs, 2);
    uint64_t* ro = (uint64_t*)(h + L.off);
    for (size_t i = 0; i < cn; ++i) ro[i] = hb.off[c0 + i] - lo_b;
    memcpy(h + L.len, hb.len + c0, cn * 4);
    if (nb) par_copy(d->pool, d->ed.h_blob, hb.blob + lo_b, nb);
    CK(hipMemcpyAsync(d->ed.d_in, h, L.total, hipMemcpyHostToDevice, st));
    if (nb) CK(hipMemcpyAsync(d->ed.d_blob, d->ed.h_blob, nb, hipMemcpyHostToDevice, st));
    const uint8_t* din = d->ed.d_in;
    rc = ed_launch(ctx->opt.time_kernels, d, cn, din, din + L.sig, d->ed.d_blob, (const uint64_t*)(din + L.off),
                   (const uint32_t*)(din + L.len), d->ed.bits, st, ed_group_cfg(ctx));
    if (rc) return rc;
    CK(hipMemcpyAsync(d->ed.h_bits, d->ed.bits, ((cn + 63) / 64) * 8, hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    const uint64_t* w = (const uint64_t*)d->ed.h_bits;
    for (size_t i = 0; i < cn; ++i) hb.out_ok[c0 + i] = (uint8_t)((w[i >> 6] >> (i & 63)) & 1u);
  }
  return GV_OK;
}

int run_ed_host(gv_ctx* ctx, size_t n, const EdHost& hb) {
  if (!ctx) return GV_EINVAL;
  if (ctx->opt.fault_inject) return GV_EFAULT;
  if (n == 0) return GV_OK;
  if (!hb.pub32 || !hb.sig64 || !hb.off || !hb.len || !hb.out_ok) return GV_EINVAL;
  for (size_t i = 0; i < n; ++i)
    if (hb.len[i] && !hb.blob) return GV_EINVAL;
  return run_sliced(workers(ctx), n, 256,
                    [&](size_t k, size_t lo, size_t hi) { return ed_slice(ctx, ctx->devs[k], lo, hi, hb); });
}

int run_host(gv_ctx* ctx, size_t n, const HostBatch& hb_in) {
  if (!ctx) return GV_EINVAL;
  if (ctx->opt.fault_inject) return GV_EFAULT;
  if (n == 0) return GV_OK;
  if ((!hb_in.pub33 && !hb_in.slots) || !hb_in.sig64 || (!hb_in.out_ok && !hb_in.out_bits)) return GV_EINVAL;
  if (!hb_in.dig32 && (!hb_in.blob || !hb_in.off || !hb_in.len)) return GV_EINVAL;
  HostBatch hb = hb_in;
  hb.pinned = hb.dig32 && is_pinned(hb.slots ? (const void*)hb.slots : hb.pub33) && is_pinned(hb.sig64) &&
              is_pinned(hb.dig32);
  // device 0's slice on the caller, devices 1.. on their persistent workers
  return run_sliced(workers(ctx), n, 256,
                    [&](size_t k, size_t lo, size_t hi) { return run_slice(ctx, ctx->devs[k], lo, hi, hb); });
}


}  // namespace

// ---- asynchronous host batches (gv_submit_* / gv_wait)
//
// One lane thread per device takes the device's slices of submitted batches
// in submission order and runs them as ONE stream of chunks over the two
// scratch sets: the next slice's staging, key grouping and key tables (on the
// other grouping set) are enqueued while the previous slice's last chunks
// still compute, so consecutive batches overlap the way pipelined
// device-resident calls do -- the synchronous entry points drain every slice
// before they return.  A batch is done when every device's slice has been
// harvested; gv_wait returns its result.  The lane holds the device lock from
// its first queued slice until its queue is empty and every chunk harvested.
// The queue, tickets and quiesce are gv_async.h (also driven by the CPU
// harness with fake devices); the lane body is lane_stream below.
struct AsyncState : gvasync::Lanes<HostBatch> {
  using gvasync::Lanes<HostBatch>::Lanes;
};
using AsyncSlice = gvasync::Slice<HostBatch>;

namespace {

struct ActiveSlice {
  AsyncSlice sl;
  HostBatch hr;                                   // what the chunks run (a grouped slice: device slots)
  KeyView ka;
  Set* g = nullptr;                               // its grouping set (released after its last chunk)
  int inflight = 0;
  bool submitted = false;
  int rc = GV_OK;
};

void finish_slice(AsyncState* as, ActiveSlice& a) {
  if (a.g) {
    const int rc = set_release(a.g, a.g->st);
    if (rc && !a.rc) a.rc = rc;
  }
  as->finish(a.sl, a.rc);
}

// Runs device k's queued slices (d->mu held) until the queue is empty or
// lane_burst slices have run, then drains.
void lane_stream(gv_ctx* ctx, AsyncState* as, size_t k, Dev* d) {
  std::list<ActiveSlice> act;
  ActiveSlice* owner[2] = {nullptr, nullptr};
  int sk = 0, gflip = 0;
  d->last_h2d = nullptr;
  auto retire = [&](ActiveSlice* a) {
    finish_slice(as, *a);
    for (auto it = act.begin(); it != act.end(); ++it)
      if (&*it == a) { act.erase(it); break; }
  };
  auto harvest_set = [&](int j) {                 // the chunk in flight on set j
    Set* s = &d->set[j];
    if (!s->busy) return;
    ActiveSlice* a = owner[j];
    const int rc = harvest(d, s, a->hr);
    if (rc && !a->rc) a->rc = rc;
    owner[j] = nullptr;
    if (--a->inflight == 0 && a->submitted) retire(a);
  };
  auto drain = [&]() {                            // the older chunk first
    harvest_set(sk);
    harvest_set(sk ^ 1);
  };
  for (size_t taken = 0;; ++taken) {
    AsyncSlice sl;
    // after lane_burst slices the lane drains and lets go of d->mu (the
    // Lanes loop calls it again while the queue holds slices): a caller that
    // keeps the queue full cannot starve synchronous calls on this device
    if (taken >= ctx->opt.lane_burst || !as->pop(k, sl)) break;
    const bool behind = !act.empty();             // an earlier slice's chunks still in flight
    act.emplace_back();
    ActiveSlice& a = act.back();
    a.sl = sl;
    a.hr = sl.job->hb;
    const size_t lo = sl.lo, n = sl.hi - sl.lo;
    const HostBatch& hb = sl.job->hb;
    const bool pipelined = n > (hb.slots ? ctx->opt.lat_max_keyed : ctx->opt.lat_max) && ctx->opt.pipe_chunk;
    const bool in_place = hb.pinned;               // read from the caller's pinned buffers, no staging
    const std::vector<size_t> sizes = ctx->opt.async_whole && in_place ? chunk_ramp(ctx, n, pipelined && !behind)
                                                                   : chunk_ramp(ctx, n, pipelined, true);
    const bool try_group = hb.pub33 && !hb.slots && ctx->opt.group_keys && n >= ctx->opt.group_min && sizes.size() > 1;
    if (try_group) {
      Set* g = &d->gset[gflip];
      gflip ^= 1;
      for (const ActiveSlice& o : act)            // an older slice still on this grouping set: drain it
        if (&o != &a && o.g == g) { drain(); break; }
      const uint32_t* dsl = nullptr;
      const int rc = slice_group(ctx, d, lo, n, hb, &a.ka, &dsl, g);
      if (rc) a.rc = rc;
      else if (dsl) {
        a.g = g;
        a.hr.d_slots = dsl;
        a.hr.d_slots_lo = lo;
        a.hr.ka = &a.ka;
      }
    }
    size_t c0 = lo;
    for (size_t i = 0; i < sizes.size() && a.rc == GV_OK; c0 += sizes[i], ++i) {
      harvest_set(sk);
      const int rc = submit(ctx, d, &d->set[sk], c0, sizes[i], a.hr);
      if (rc) { a.rc = rc; break; }
      owner[sk] = &a;
      ++a.inflight;
      sk ^= 1;
    }
    a.submitted = true;
    if (a.inflight == 0) retire(&a);
  }
  drain();
}

// Device k's lane body (gvasync::Lanes calls it when k's queue holds a slice).
void lane_run(gv_ctx* ctx, AsyncState* as, size_t k) {
  Dev* d = ctx->devs[k];
  std::lock_guard<std::mutex> dl(d->mu);
  if (hipSetDevice(d->id) != hipSuccess) {        // fail every queued slice of this device
    as->fail_queued(k, GV_EHIP);
    return;
  }
  lane_stream(ctx, as, k, d);
}

AsyncState* async_state(gv_ctx* ctx) {
  static std::mutex create_mu;
  std::lock_guard<std::mutex> lk(create_mu);
  if (!ctx->async) {
    // (a lane runs only for a submitted slice, i.e. after ctx->async is set)
    ctx->async = new AsyncState(ctx->devs.size(), [ctx](size_t k) { lane_run(ctx, ctx->async, k); });
  }
  return ctx->async;
}

// Held by gv_keys_load / gv_keys_reset (gvasync::Lanes::Quiesce): no
// submitted keyed batch reads a slot that moves, and no submission slips in.
struct AsyncQuiesce : gvasync::Lanes<HostBatch>::Quiesce {
  explicit AsyncQuiesce(gv_ctx* ctx) : Quiesce(ctx->async) {}
};

int submit_host(gv_ctx* ctx, size_t n, const HostBatch& hb_in, uint64_t* ticket) {
  if (!ctx || !ticket) return GV_EINVAL;
  *ticket = 0;
  if (ctx->opt.fault_inject) return GV_EFAULT;
  if (n > 0) {
    if ((!hb_in.pub33 && !hb_in.slots) || !hb_in.sig64 || (!hb_in.out_ok && !hb_in.out_bits)) return GV_EINVAL;
    if (!hb_in.dig32 && (!hb_in.blob || !hb_in.off || !hb_in.len)) return GV_EINVAL;
  }
  HostBatch hb = hb_in;
  hb.pinned = hb_in.dig32 && is_pinned(hb_in.slots ? (const void*)hb_in.slots : hb_in.pub33) &&
              is_pinned(hb_in.sig64) && is_pinned(hb_in.dig32);
  *ticket = async_state(ctx)->submit(hb, n);
  return GV_OK;
}

}  // namespace

namespace {

void free_set(Set& s) {
  if (s.st) (void)hipStreamSynchronize(s.st);
  if (s.scratch) (void)hipFree(s.scratch);
  if (s.d_blob) (void)hipFree(s.d_blob);
  if (s.h_in) (void)hipHostFree(s.h_in);
  if (s.h_blob) (void)hipHostFree(s.h_blob);
  if (s.h_bits) (void)hipHostFree(s.h_bits);
  if (s.h_out8) (void)hipHostFree(s.h_out8);
  if (s.last) (void)hipEventDestroy(s.last);
  if (s.done) (void)hipEventDestroy(s.done);
  if (s.ecm_ready) (void)hipEventDestroy(s.ecm_ready);
  if (s.fork) (void)hipEventDestroy(s.fork);
  if (s.keys_done) (void)hipEventDestroy(s.keys_done);
  if (s.grp_ready) (void)hipEventDestroy(s.grp_ready);
  if (s.side) { (void)hipStreamSynchronize(s.side); (void)hipStreamDestroy(s.side); }
  s.gk.free();
  if (s.g_rows) (void)hipFree(s.g_rows);
  if (s.h_count) (void)hipHostFree(s.h_count);
  if (s.miss_buf) (void)hipFree(s.miss_buf);
  if (s.miss_done) (void)hipEventDestroy(s.miss_done);
  if (s.miss_set) { free_set(*s.miss_set); delete s.miss_set; }
  if (s.lad) { (void)hipStreamSynchronize(s.lad); (void)hipStreamDestroy(s.lad); }
  if (s.lad_done) (void)hipEventDestroy(s.lad_done);
  if (s.st) (void)hipStreamDestroy(s.st);
}

}  // namespace

extern "C" {


// gv_open's pre-sizing (GV_PRESIZE=1, off by default): both scratch sets of
// every device at a whole max_batch chunk, and their grouping arenas when the
// HBM budget holds them, allocated and written once, so a node's first large
// calls neither allocate nor first-touch them.  First 1M call 1.30 -> 1.26x
// steady (profiles/r06/first_call/presize_ab.jsonl): the rest is the first
// ladders themselves (4.51, 4.30, 4.17 then 4.0 ms), not allocation; off by
// default because the ~6 GB it holds per device would come out of the HBM
// budget that the resident key arena sizes itself from.
static int presize_devices(gv_ctx* ctx) {
  const size_t C = round_up(ctx->opt.max_batch, 256);
  const size_t capU = round_up(std::max<size_t>(C / ctx->opt.group_div, 256), 256);
  for (Dev* d : ctx->devs) {
    if (hipSetDevice(d->id) != hipSuccess) return GV_EHIP;
    for (Set& s : d->set) {
      int rc = ensure_cap(&s, C);
      if (rc) return rc;
      if (hipMemsetAsync(s.scratch, 0, s.d_in ? (size_t)((uint8_t*)(s.bits + C / 64) - s.scratch) : 0, s.st) !=
          hipSuccess)
        return GV_EHIP;
      rc = ensure_group_arena(ctx, d, &s, capU, lay_k4());
      if (rc == GV_OK) {
        for (uint32_t* p : {s.gk.qt, s.gk.qt2})
          if (hipMemsetAsync(p, 0, (size_t)capU * GV_KEY_WORDS * 4 * (p == s.gk.qt ? 1 : GV_LGRP - 1), s.st) !=
              hipSuccess)
            return GV_EHIP;
      } else if (rc != GV_ENOMEM) {
        return rc;
      }
    }
    for (Set& s : d->set)
      if (hipStreamSynchronize(s.st) != hipSuccess) return GV_EHIP;
  }
  return GV_OK;
}

int gv_open(const int* dev_ids, int n_dev, gv_ctx** out) {
  if (!out || n_dev < 0 || (n_dev > 0 && !dev_ids)) return GV_EINVAL;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return GV_ENODEV;
  std::vector<int> ids;
  if (n_dev == 0) for (int i = 0; i < count; ++i) ids.push_back(i);
  else for (int i = 0; i < n_dev; ++i) {
    if (dev_ids[i] < 0 || dev_ids[i] >= count) return GV_ENODEV;
    ids.push_back(dev_ids[i]);
  }
  for (int id : ids) {                          // the kernels are written for wave64
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, id) != hipSuccess || prop.warpSize != 64) return GV_ENODEV;
  }
  gv_ctx* ctx = new gv_ctx();
  gvopt::opt_from_env(ctx->opt, getenv);          // every GV_* option variable, by its row's rule
  {                                             // the index hash's seed: not computable from outside the process
    std::random_device rd;
    ctx->opt.kidx_seed = ((uint64_t)rd() << 32) ^ (uint64_t)rd() ^
                     (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count() * 0x9E3779B97F4A7C15ull ^
                     (uint64_t)(uintptr_t)ctx;
    ctx->opt.ed_kidx_seed = ctx->opt.kidx_seed;     // (the ed25519 index: another table, the same secret)
  }
  ctx->opt.stage_threads = gvstage::stage_pool_threads(host_cpus(), (int)ids.size());
  for (size_t k = 0; k < ids.size(); ++k) {
    Dev* d = new Dev();
    d->id = ids[k];
    d->kidx.seed = &ctx->opt.kidx_seed;
    d->kidx.stat = &ctx->kidx_stat;
    d->ed_kidx.seed = &ctx->opt.ed_kidx_seed;
    d->ed_kidx.stat = &ctx->ed_kidx_stat;
    ctx->devs.push_back(d);
    d->pool = new Pool(ctx->opt.stage_threads - 1);
    if (k > 0) d->worker = new Worker();
    bool ok = hipSetDevice(d->id) == hipSuccess;
    // Stream priorities of the pipelined device-resident calls (env
    // GV_LADDER_PRIO): "front" (default) -- the front kernels (unpack, key
    // grouping, the key-table build on the side stream, s^-1, prep) above the
    // ladders, so a slot a ladder workgroup frees goes to the next call's
    // front first and it is done before the current ladder drains; "ladder" --
    // the ladders above (the round-3 order: the front then runs in the ladder's
    // tail); "equal".
    int lo_prio = 0, hi_prio = 0;
    ok = ok && hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio) == hipSuccess;
    int front_prio = hi_prio, ladder_prio = lo_prio;
    if (const char* lp = getenv("GV_LADDER_PRIO")) {
      if (!strcmp(lp, "ladder")) { front_prio = lo_prio; ladder_prio = hi_prio; }
      else if (!strcmp(lp, "equal")) front_prio = ladder_prio = lo_prio;
    }
    for (Set* sp : {&d->set[0], &d->set[1], &d->gset[0], &d->gset[1]})
      ok = ok && hipStreamCreateWithPriority(&sp->st, hipStreamNonBlocking, front_prio) == hipSuccess &&
           hipStreamCreateWithPriority(&sp->lad, hipStreamNonBlocking, ladder_prio) == hipSuccess &&
           hipEventCreateWithFlags(&sp->lad_done, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&sp->last, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&sp->done, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&sp->h2d, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&sp->ecm_ready, hipEventDisableTiming) == hipSuccess &&
           hipStreamCreateWithPriority(&sp->side, hipStreamNonBlocking, front_prio) == hipSuccess &&
           hipEventCreateWithFlags(&sp->fork, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&sp->keys_done, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&sp->grp_ready, hipEventDisableTiming) == hipSuccess;
    // pipelined device-resident calls: front kernels on two streams
    // (alternating sets), the ladders on two more (two_ladders)
    for (int j = 0; j < 2; ++j)
      ok = ok && hipStreamCreateWithPriority(&d->lo_st[j], hipStreamNonBlocking, front_prio) == hipSuccess;
    for (int j = 0; j < 2; ++j)
      ok = ok && hipStreamCreateWithPriority(&d->hi_st[j], hipStreamNonBlocking, ladder_prio) == hipSuccess &&
           hipEventCreateWithFlags(&d->hi_done[j], hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&d->bits_ev[j], hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&d->plain_done, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipMalloc(&d->gtab, (size_t)2 * GV_GTAB_N * 16 * 4) == hipSuccess &&
         gvk_gen_gtable(d->gtab, d->set[0].st) == hipSuccess && hipStreamSynchronize(d->set[0].st) == hipSuccess;
    ok = ok && hipMalloc(&d->glat, (size_t)GV_GLAT_WORDS * 4) == hipSuccess &&
         gvk_gen_glat(d->glat, d->set[0].st) == hipSuccess && hipStreamSynchronize(d->set[0].st) == hipSuccess;
    if (!ok) { gv_close(ctx); return GV_EHIP; }
  }
  // The large G tables of the default schedules (full-scalar k4 / per-item,
  // k4's group tables, k6), enqueued on every device before waiting on any, so
  // a node's first block does not build them (~0.5 s per device, concurrent
  // across devices).  GV_EAGER_TABLES=0: built on first use instead.
  const char* eager = getenv("GV_EAGER_TABLES");
  if (!eager || strcmp(eager, "0") != 0) {
    for (Dev* d : ctx->devs) {
      if (hipSetDevice(d->id) != hipSuccess) { gv_close(ctx); return GV_EHIP; }
      Set* s = &d->set[0];
      int rc = ensure_gtab4(ctx, d, s, s->st, false);
      if (!rc) rc = ensure_gtab6(ctx, d, s, s->st, ctx->opt.k6 || ctx->opt.keys_k6, false);
      if (rc) { gv_close(ctx); return rc; }
    }
    for (Dev* d : ctx->devs)
      if (hipSetDevice(d->id) != hipSuccess || hipStreamSynchronize(d->set[0].st) != hipSuccess) {
        gv_close(ctx);
        return GV_EHIP;
      }
  }
  const char* presize = getenv("GV_PRESIZE");
  if (presize && strcmp(presize, "0") != 0) {
    const int rc = presize_devices(ctx);
    if (rc) { gv_close(ctx); return rc; }
  }
  *out = ctx;
  return GV_OK;
}

void gv_close(gv_ctx* ctx) {
  if (!ctx) return;
  if (AsyncState* as = ctx->async) {              // the lanes finish what is queued, then quit
    as->close();
    delete as;
    ctx->async = nullptr;
  }
  for (Dev* d : ctx->devs) {
    delete d->worker;
    (void)hipSetDevice(d->id);
    for (Set& s : d->set) free_set(s);
    for (Set& g : d->gset) free_set(g);
    if (d->gtab) (void)hipFree(d->gtab);
    if (d->glat) (void)hipFree(d->glat);
    if (d->gtab4) (void)hipFree(d->gtab4);
    if (d->gtab6) (void)hipFree(d->gtab6);
    if (d->gtabf) (void)hipFree(d->gtabf);
    for (KeyTabs* t : {&d->k4, &d->kn, &d->kw}) t->free();
    if (d->edtab) (void)hipFree(d->edtab);
    if (d->edtab16) (void)hipFree(d->edtab16);
    if (d->ed.d_in) (void)hipFree(d->ed.d_in);
    if (d->ed.atab) (void)hipFree(d->ed.atab);
    if (d->ed.bits) (void)hipFree(d->ed.bits);
    if (d->ed.d_blob) (void)hipFree(d->ed.d_blob);
    if (d->ed.h_in) (void)hipHostFree(d->ed.h_in);
    if (d->ed.h_blob) (void)hipHostFree(d->ed.h_blob);
    if (d->ed.h_bits) (void)hipHostFree(d->ed.h_bits);
    if (d->ed.last) (void)hipEventDestroy(d->ed.last);
    for (uint32_t* p : {d->ektab, d->ekpub, d->ekok, d->ektabw}) if (p) (void)hipFree(p);
    if (d->edkd_s) (void)hipFree(d->edkd_s);
    if (d->edkd_last) (void)hipEventDestroy(d->edkd_last);
    for (KeyIndex* ix : {&d->kidx, &d->ed_kidx}) {
      kidx_free(d, *ix);
      if (ix->cnt) (void)hipFree(ix->cnt);
      if (ix->h) (void)hipHostFree(ix->h);
    }
    for (hipEvent_t e : d->kidx_ev) if (e) (void)hipEventDestroy(e);
    if (d->kidx_found) (void)hipEventDestroy(d->kidx_found);
    if (d->edl_h) (void)hipHostFree(d->edl_h);
    for (uint32_t* q : {d->edg_ktab, d->edg_kpub, d->edg_kok}) if (q) (void)hipFree(q);
    if (d->ed_h_count) (void)hipHostFree(d->ed_h_count);
    for (int k = 0; k < 2; ++k) {
      if (d->edk_h[k]) (void)hipHostFree(d->edk_h[k]);
      if (d->edk_d[k]) (void)hipFree(d->edk_d[k]);
      if (d->edk_s[k]) (void)hipFree(d->edk_s[k]);
    }
    for (auto& rs : d->ring)
      for (auto e : rs) if (e) (void)hipEventDestroy(e);
    for (hipStream_t t : {d->lo_st[0], d->lo_st[1], d->hi_st[0], d->hi_st[1]})
      if (t) { (void)hipStreamSynchronize(t); (void)hipStreamDestroy(t); }
    for (hipEvent_t e : {d->hi_done[0], d->hi_done[1], d->bits_ev[0], d->bits_ev[1]})
      if (e) (void)hipEventDestroy(e);
    if (d->plain_done) (void)hipEventDestroy(d->plain_done);
    delete d->pool;
    delete d;
  }
  delete ctx;
}

int gv_num_devices(const gv_ctx* ctx) { return ctx ? (int)ctx->devs.size() : 0; }

int gv_verify_msgs(gv_ctx* ctx, size_t n, const uint8_t* pub33, const uint8_t* sig64,
                   const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len,
                   uint8_t* out_ok) {
  return run_host(ctx, n, HostBatch{pub33, sig64, nullptr, msg_blob, msg_off, msg_len, nullptr, out_ok, nullptr});
}

int gv_verify_digests(gv_ctx* ctx, size_t n, const uint8_t* pub33, const uint8_t* sig64,
                      const uint8_t* dig32, uint8_t* out_ok) {
  if (!dig32 && n) return GV_EINVAL;
  return run_host(ctx, n, HostBatch{pub33, sig64, dig32, nullptr, nullptr, nullptr, nullptr, out_ok, nullptr});
}

int gv_verify_digests_bits(gv_ctx* ctx, size_t n, const uint8_t* pub33, const uint8_t* sig64,
                           const uint8_t* dig32, uint64_t* out_bits) {
  if (!dig32 && n) return GV_EINVAL;
  return run_host(ctx, n, HostBatch{pub33, sig64, dig32, nullptr, nullptr, nullptr, nullptr, nullptr, out_bits});
}

int gv_verify_msgs_bits(gv_ctx* ctx, size_t n, const uint8_t* pub33, const uint8_t* sig64,
                        const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len,
                        uint64_t* out_bits) {
  return run_host(ctx, n, HostBatch{pub33, sig64, nullptr, msg_blob, msg_off, msg_len, nullptr, nullptr, out_bits});
}

static int dev_common(gv_ctx* ctx, int slot, size_t n, const void* pub, const void* sig, void* bits,
                      Dev** dout) {
  if (!ctx) return GV_EINVAL;
  if (ctx->opt.fault_inject) return GV_EFAULT;
  if (slot < 0 || slot >= (int)ctx->devs.size()) return GV_ENODEV;
  if (n == 0) return GV_OK;
  if (!pub || !sig || !bits) return GV_EINVAL;
  if (((uintptr_t)pub & 3) || ((uintptr_t)sig & 3)) return GV_EINVAL;
  if (n > kMaxItems) return GV_EINVAL;
  *dout = ctx->devs[slot];
  return GV_OK;
}

int gv_submit_digests(gv_ctx* ctx, size_t n, const uint8_t* pub33, const uint8_t* sig64, const uint8_t* dig32,
                      uint8_t* out_ok, uint64_t* ticket) {
  if (n && !dig32) return GV_EINVAL;
  return submit_host(ctx, n, HostBatch{pub33, sig64, dig32, nullptr, nullptr, nullptr, nullptr, out_ok, nullptr},
                     ticket);
}

int gv_submit_digests_keyed(gv_ctx* ctx, size_t n, const uint32_t* slot, const uint8_t* sig64, const uint8_t* dig32,
                            uint8_t* out_ok, uint64_t* ticket) {
  if (n && (!slot || !dig32)) return GV_EINVAL;
  return submit_host(ctx, n, HostBatch{nullptr, sig64, dig32, nullptr, nullptr, nullptr, slot, out_ok, nullptr},
                     ticket);
}

int gv_submit_msgs(gv_ctx* ctx, size_t n, const uint8_t* pub33, const uint8_t* sig64, const uint8_t* msg_blob,
                   const uint64_t* msg_off, const uint32_t* msg_len, uint8_t* out_ok, uint64_t* ticket) {
  return submit_host(ctx, n, HostBatch{pub33, sig64, nullptr, msg_blob, msg_off, msg_len, nullptr, out_ok, nullptr},
                     ticket);
}

int gv_submit_msgs_keyed(gv_ctx* ctx, size_t n, const uint32_t* slot, const uint8_t* sig64, const uint8_t* msg_blob,
                         const uint64_t* msg_off, const uint32_t* msg_len, uint8_t* out_ok, uint64_t* ticket) {
  if (n && !slot) return GV_EINVAL;
  return submit_host(ctx, n, HostBatch{nullptr, sig64, nullptr, msg_blob, msg_off, msg_len, slot, out_ok, nullptr},
                     ticket);
}

int gv_wait(gv_ctx* ctx, uint64_t ticket) {
  if (!ctx || !ctx->async) return GV_EINVAL;
  return ctx->async->wait(ticket, GV_EINVAL);
}

int gv_dev_verify_digests(gv_ctx* ctx, int dev_slot, size_t n, const void* d_pub33,
                          const void* d_sig64, const void* d_dig32, void* d_bits, void* stream) {
  Dev* d = nullptr;
  int rc = dev_common(ctx, dev_slot, n, d_pub33, d_sig64, d_bits, &d);
  if (rc || n == 0) return rc;
  if (!d_dig32 || ((uintptr_t)d_dig32 & 3)) return GV_EINVAL;
  std::lock_guard<std::mutex> lk(d->mu);
  CK(hipSetDevice(d->id));
  Items it;
  it.n = n; it.pub33 = (const uint8_t*)d_pub33; it.sig64 = (const uint8_t*)d_sig64; it.dig32 = (const uint8_t*)d_dig32;
  it.index = true;
  return dev_launch(ctx, d, stream, it, d_bits);
}

int gv_dev_verify_msgs(gv_ctx* ctx, int dev_slot, size_t n, const void* d_pub33, const void* d_sig64,
                       const void* d_msg_blob, const void* d_msg_off, const void* d_msg_len, void* d_bits,
                       void* stream) {
  Dev* d = nullptr;
  int rc = dev_common(ctx, dev_slot, n, d_pub33, d_sig64, d_bits, &d);
  if (rc || n == 0) return rc;
  if (!d_msg_blob || !d_msg_off || !d_msg_len) return GV_EINVAL;
  std::lock_guard<std::mutex> lk(d->mu);
  CK(hipSetDevice(d->id));
  Items it;
  it.n = n; it.pub33 = (const uint8_t*)d_pub33; it.sig64 = (const uint8_t*)d_sig64;
  it.blob = (const uint8_t*)d_msg_blob; it.off = (const uint64_t*)d_msg_off; it.len = (const uint32_t*)d_msg_len;
  it.index = true;
  return dev_launch(ctx, d, stream, it, d_bits);
}

// ---- ed25519
namespace {
// Small uncached ed25519 batches on one device (k_ed_lat_unc, one signature
// per block): the kernel reads keys, signatures and messages from the pinned
// staging buffer and writes verdict bytes there (no H2D / D2H copies).
int ed_unc_small(gv_ctx* ctx, size_t n, const EdHost& hb) {
  Dev* d = ctx->devs[0];
  std::lock_guard<std::mutex> lk(d->mu);
  CK(hipSetDevice(d->id));
  hipStream_t st = d->set[0].st;
  int rc = ed_ensure(d, 256, st);                 // the resident comb table of B
  if (rc) return rc;
  const auto [lo, hi] = msg_range(hb.off, hb.len, 0, n);
  const size_t o_sig = round_up(n * 32, 64), o_off = o_sig + n * 64, o_len = o_off + n * 8, o_out = o_len + n * 4,
               o_blob = round_up(o_out + n, 64), total = o_blob + (hi - lo);
  if ((rc = ensure_pinned(&d->edl_h, &d->edl_h_cap, total))) return rc;
  uint8_t* h = d->edl_h;
  memcpy(h, hb.pub32, n * 32);
  memcpy(h + o_sig, hb.sig64, n * 64);
  uint64_t* ro = (uint64_t*)(h + o_off);
  for (size_t i = 0; i < n; ++i) ro[i] = hb.off[i] - lo;
  memcpy(h + o_len, hb.len, n * 4);
  if (hi > lo) memcpy(h + o_blob, hb.blob + lo, hi - lo);
  gvk_edl b = fill_edl(d, n, 0, nullptr, h + o_sig, h + o_blob, (const uint64_t*)(h + o_off),
                       (const uint32_t*)(h + o_len), h + o_out);
  b.pub32 = h;                                    // uncached: the keys themselves (k_ed_lat_unc reads no arena)
  d->routes[GV_ROUTE_ED_LAT]++;
  CK(gvk_ed_lat_unc(&b, st));
  CK(hipStreamSynchronize(st));
  memcpy(hb.out_ok, h + o_out, n);
  return GV_OK;
}
}  // namespace

int gv_verify_ed25519_msgs(gv_ctx* ctx, size_t n, const uint8_t* pub32, const uint8_t* sig64,
                           const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len,
                           uint8_t* out_ok) {
  const EdHost hb{pub32, sig64, msg_blob, msg_off, msg_len, out_ok};
  if (ctx && !ctx->opt.fault_inject && n && n <= ctx->opt.ed_unc_lat_max && pub32 && sig64 && msg_off && msg_len && out_ok) {
    for (size_t i = 0; i < n; ++i)
      if (msg_len[i] && !msg_blob) return GV_EINVAL;
    return ed_unc_small(ctx, n, hb);
  }
  return run_ed_host(ctx, n, hb);
}

// gv_dev_verify_ed25519_msgs: below, behind the keyed call whose body it shares (ed_dev_keyed).

// ---- key arena
namespace {
// A replace chunk's slot list (host, cn entries) to the device: behind the
// chunk's pub33 in the set's staged-input region (the signature part of
// in_layout, which a key-table build leaves unused).
hipError_t stage_slots(Set* s, size_t C, const uint32_t* slots, size_t cn, hipStream_t st, const uint32_t** d_slots) {
  uint8_t* p = s->d_in + in_layout(C, false, false).sig;
  *d_slots = (const uint32_t*)p;
  return hipMemcpyAsync(p, slots, cn * 4, hipMemcpyHostToDevice, st);
}

// The n keys pub33 (host) through set s in chunks of `step`: the set grown to
// the chunk's lanes C (256-aligned), or those whose Q-table region holds the
// words(cn) words of a key-table build's scratch if more, the chunk's bytes
// uploaded -- slots (host, n entries; null: none): the chunk's part of the list
// behind them (stage_slots) -- body(c0, cn, C, d_slots) enqueued, and a sync
// (the caller's pub33 chunk is read by then).  The caller holds d->mu.
int key_chunks(Set* s, hipStream_t st, const uint8_t* pub33, size_t n, const uint32_t* slots, size_t step,
               const std::function<size_t(size_t)>& words,
               const std::function<hipError_t(size_t, uint32_t, uint32_t, const uint32_t*)>& body) {
  int rc;
  for (size_t c0 = 0; c0 < n; c0 += step) {
    const size_t cn = std::min(step, n - c0), C = round_up(cn, 256);
    if ((rc = ensure_cap(s, words ? std::max(C, round_up(words(cn) / GV_QTAB_WORDS + 1, 256)) : C))) return rc;
    if ((rc = set_acquire(s, st))) return rc;
    CK(hipMemcpyAsync(s->d_in, pub33 + c0 * 33, cn * 33, hipMemcpyHostToDevice, st));
    const uint32_t* d_slots = nullptr;
    if (slots) CK(stage_slots(s, C, slots + c0, cn, st, &d_slots));
    CK(body(c0, (uint32_t)cn, (uint32_t)C, d_slots));
    if ((rc = set_release(s, st))) return rc;
    CK(hipStreamSynchronize(st));
  }
  return GV_OK;
}

// The k4 and / or the resident k6 tables of the n keys pub33 (host) into slots
// base.., or -- slots given (gv_keys_replace) -- key i into slot slots[i]; one
// pub33 upload per chunk for both builds.  The k4 build takes max_batch keys
// at a time; the k6 tables' scratch rows per key are ~12x its (GV_KN_ARENA_NG
// groups of 32 entries): smaller chunks.
int build_k4k6(gv_ctx* ctx, Dev* d, Set* s, hipStream_t st, const uint8_t* pub33, size_t n, size_t base,
               const uint32_t* slots, bool k4, bool k6) {
  const size_t step = k6 ? std::min<size_t>(ctx->opt.max_batch, 32768) : ctx->opt.max_batch;
  auto words = [&](size_t cn) {                   // (ratios, E, and when they fit the forward-pass entries)
    return std::max<size_t>(k4 ? gvk_keys_scratch_words((uint32_t)cn, GV_LGRP, GV_QTAB_N, 0) : 0,
                            k6 ? gvk_keys_scratch_words((uint32_t)cn, GV_KN_ARENA_NG, GV_K6_NT, 1) : 0);
  };
  return key_chunks(s, st, pub33, n, slots, step, words, [&](size_t c0, uint32_t cn, uint32_t C, const uint32_t* d_slots) {
    const uint32_t b0 = slots ? 0u : (uint32_t)(base + c0);
    hipError_t e = hipSuccess;
    if (k4) {
      const size_t room = (size_t)GV_QTAB_WORDS * s->cap;
      const int qe4 = ctx->opt.keys_scratch && gvk_keys_scratch_words(cn, GV_LGRP, GV_QTAB_N, 1) <= room;
      e = gvk_keys_build(s->d_in, cn, C, s->in_x, s->in_pfx, s->in_r, s->in_s, s->in_e, s->qtab, qe4, b0, d_slots,
                         d->k4.qt, d->k4.zq, (uint32_t)d->k4.cap, d->k4.ok, d->k4.qt2, d->k4.zq2, st);
    }
    if (k6 && e == hipSuccess)
      e = gvk_keys_build6(s->d_in, cn, C, s->in_x, s->in_pfx, s->in_r, s->in_s, s->in_e, s->qtab,
                          ctx->opt.keys_scratch ? 1 : 0, b0, d_slots, d->kn.qt, d->kn.zq, (uint32_t)d->kn.cap, d->k4.ok,
                          d->kn.qt2, d->kn.zq2, st);
    return e;
  });
}

// The wide-window tables (layout d->kw.lay) of the n keys pub33 (host) into
// slots base.. of the wide arena (slots: as build_k4k6's), in chunks whose
// build scratch stays within what the k6 build's chunks take.
int build_wide(gv_ctx* ctx, Dev* d, Set* s, hipStream_t st, const uint8_t* pub33, size_t n, size_t base,
               const uint32_t* slots = nullptr) {
  const KeyTabs& kw = d->kw;
  const int qw = kw.lay.qw(), nt = (int)kw.lay.nt, ng = (int)kw.lay.ng, qew = ctx->opt.keys_scratch ? 1 : 0;
  const size_t stepw = std::min<size_t>(ctx->opt.max_batch, std::max<size_t>(256, 32768 / (size_t)ng / 256 * 256));
  auto words = [&](size_t cn) { return (size_t)gvk_keys_scratch_words((uint32_t)cn, ng, nt, qew); };
  return key_chunks(s, st, pub33, n, slots, stepw, words, [&](size_t c0, uint32_t cn, uint32_t C, const uint32_t* d_slots) {
    return gvk_keys_build_wide(s->d_in, cn, C, s->in_x, s->in_pfx, s->in_r, s->in_s, s->in_e, s->qtab, qew,
                               (uint32_t)(base + c0), d_slots, kw.qt, kw.zq, (uint32_t)kw.cap, d->k4.ok, kw.qt2, kw.zq2,
                               qw, ng, st);
  });
}

// The index rows of the n keys pub33 (host) for slots base.. (slots: as
// build_k4k6's), in the build chunks' staging; put: the chunk's slots also
// enter the table (an append; a replacement refills it afterwards).  The rows
// come from the bytes as given: read_back_pub33 below cannot stand in, it
// turns a rejected key's prefix into 00.
int kidx_write(gv_ctx* ctx, Dev* d, Set* s, hipStream_t st, const uint8_t* pub33, size_t n, size_t base,
               const uint32_t* slots, bool put) {
  KeyIndex& ix = d->kidx;
  return key_chunks(s, st, pub33, n, slots, ctx->opt.max_batch, nullptr,
                    [&](size_t c0, uint32_t cn, uint32_t, const uint32_t* d_slots) {
    const uint32_t b0 = slots ? 0u : (uint32_t)(base + c0);
    hipError_t e = gvk_kidx_rows(s->d_in, cn, b0, d_slots, ix.rows, st);
    if (e == hipSuccess) ix.stat->launches++;
    if (e == hipSuccess && put) e = kidx_put(ix, cn, b0, d_slots, st);
    return e;
  });
}
// gv_keys_load's part: rows and table entries of the new slots base.., after
// their tables.
int kidx_load(gv_ctx* ctx, Dev* d, Set* s, hipStream_t st, const uint8_t* pub33, size_t n, size_t base) {
  int rc;
  KeyIndex& ix = d->kidx;
  const bool had = ix.rows && ix.cap >= d->k4.cap;
  if ((rc = kidx_ensure(ctx, d, base, st))) return rc;
  if (base == 0 && had && (rc = kidx_refill(ix, 0, st))) return rc;   // an arena restarted: the table is cleared
  if ((rc = kidx_write(ctx, d, s, st, pub33, n, base, nullptr, true))) return rc;
  return kidx_read_left_out(ix, st);
}

// Affine 1*Q (64 bytes) and the verdict of the n slots `slots` (host) of the
// k4 tables, kcount slots in use; scratch of the call's own.
int keys_point_read(Dev* d, hipStream_t st, size_t n, const uint32_t* slots, size_t kcount, uint8_t* xy, uint8_t* ok) {
  uint8_t* buf = nullptr;
  const size_t sb = round_up(n * 4, 256), xb = round_up(n * 64, 256);
  if (hipMalloc(&buf, sb + xb + n) != hipSuccess) return GV_ENOMEM;
  int rc = GV_OK;
  if (hipMemcpyAsync(buf, slots, n * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
      gvk_keys_point((uint32_t)n, (const uint32_t*)buf, d->k4.qt, d->k4.zq, (uint32_t)d->k4.cap, d->k4.ok,
                     (uint32_t)kcount, buf + sb, buf + sb + xb, st) != hipSuccess ||
      hipMemcpyAsync(xy, buf + sb, n * 64, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(ok, buf + sb + xb, n, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    rc = GV_EHIP;
  (void)hipFree(buf);
  return rc;
}

// The compressed keys of slots 0..n-1 read back from the k4 tables (affine
// 1*Q of each slot); a slot whose key ParsePubKey rejected gets a prefix
// byte it rejects again (0x00), so a rebuild keeps its verdict.
int read_back_pub33(Dev* d, hipStream_t st, size_t n, std::vector<uint8_t>& pub) {
  std::vector<uint32_t> slots(n);
  for (size_t i = 0; i < n; ++i) slots[i] = (uint32_t)i;
  std::vector<uint8_t> xy(n * 64), ok(n);
  const int rc = keys_point_read(d, st, n, slots.data(), n, xy.data(), ok.data());
  if (rc) return rc;
  pub.assign(n * 33, 0);
  for (size_t i = 0; i < n; ++i) {
    uint8_t* p = &pub[i * 33];
    memcpy(p + 1, &xy[i * 64], 32);
    p[0] = ok[i] ? (uint8_t)(0x02 | (xy[i * 64 + 63] & 1)) : 0x00;
  }
  return GV_OK;
}

// A replacement's slot list against an arena of `count` slots: each slot
// loaded, none twice (two lanes would write one row).
bool check_slots(size_t count, size_t n, const uint32_t* slots) {
  if (n > count) return false;
  std::vector<uint64_t> seen((count + 63) / 64, 0);
  for (size_t i = 0; i < n; ++i) {
    const size_t sl = slots[i];
    if (sl >= count || (seen[sl >> 6] >> (sl & 63) & 1)) return false;
    seen[sl >> 6] |= (uint64_t)1 << (sl & 63);
  }
  return true;
}
}  // namespace

int gv_keys_load(gv_ctx* ctx, size_t n, const uint8_t* pub33, uint32_t* slot_out) {
  if (!ctx) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (!pub33 || !slot_out) return GV_EINVAL;
  AsyncQuiesce q(ctx);                          // no submitted keyed batch reads slots that move
  std::lock_guard<std::mutex> kl(ctx->keys_mu);
  const size_t base = ctx->keys;
  if (base + n > kMaxItems) return GV_EINVAL;
  for (Dev* d : ctx->devs) {                    // every device holds every key
    std::lock_guard<std::mutex> lk(d->mu);
    CK(hipSetDevice(d->id));
    Set* s = &d->set[0];
    hipStream_t st = s->st;
    for (hipStream_t t : d->hi_st) CK(hipStreamSynchronize(t));   // no pipelined ladder reads an arena being grown
    if (base == 0) {                            // after gv_keys_reset the slots are rewritten from 0
      d->keys6 = d->keysw = 0;
      d->kw_full = false;
      kidx_reset(d->kidx);
      d->kidx.on = ctx->opt.keys_index;             // the arena takes the option here
    }
    // an earlier load that failed on a later device left this one's index ahead
    // of the arena (rows of keys no slot holds): no index until gv_keys_reset
    if (d->kidx.keys > base) kidx_stop(d, d->kidx);
    // the k6 tables too when their G tables exist (or can be built) and the
    // arena has room for them (else k4 only: the k4 route serves the slots)
    int rc = ensure_gtab4(ctx, d, s, st);
    if (!rc) rc = ensure_gtab6(ctx, d, s, st, ctx->opt.keys_k6 || ctx->opt.keys_wide);
    if (rc) return rc;
    bool k6 = ctx->opt.keys_k6 && d->gtab6 && d->keys6 == base;
    if ((rc = ensure_keys(d, base + n, base, st, ctx->opt.key_cap, ctx->opt.hbm_budget, &k6))) return rc;
    if ((rc = build_k4k6(ctx, d, s, st, pub33, n, base, nullptr, true, k6))) return rc;
    if (k6) d->keys6 = base + n;
    // the wide-window tables: while every earlier slot has them and memory
    // holds the grown arena (a refusal of the last layout stops them until
    // gv_keys_reset: batches then take the k6 tables).  An arena started from
    // slot 0 takes the first layout the options allow (kWideLayouts); when a
    // growth is refused the whole arena moves to the next allowed layout --
    // one 11-bit window per group (12 tables of 64 KiB per key), two (6), one
    // 9-bit window per group (15 tables of 16 KiB), two (8): the loaded slots'
    // keys are read back from the k4 tables and rebuilt from slot 0.
    if (ctx->opt.keys_wide && d->gtab6 && d->keysw == base && !d->kw_full) {
      const int only_qw = ctx->opt.keys_wide_qw;
      int li = wide_layout_next(0, only_qw, ctx->opt.keys_wide == 2 ? 1 : 2);
      if (base != 0 && d->kw.lay.ng) {            // a running arena keeps its layout
        li = kWideLayoutCount;
        for (int i = 0; i < kWideLayoutCount; ++i)
          if (lay_wide(kWideLayouts[i]) == d->kw.lay) li = i;
      } else if (li < kWideLayoutCount && d->kw.lay != lay_wide(kWideLayouts[li])) {
        free_keys_wide(d, lay_wide(kWideLayouts[li]));
      }
      bool ok = li < kWideLayoutCount && ensure_keys_wide(ctx->opt, d, base + n, base, st);
      // (a failed read-back only stops the wide tables: the k6 ones serve)
      std::vector<uint8_t> old_pub;
      bool moved = false;
      while (!ok && (li = wide_layout_next(li + 1, only_qw, 1)) < kWideLayoutCount) {
        const bool back = moved || !base || read_back_pub33(d, st, base, old_pub) == GV_OK;
        moved = true;
        free_keys_wide(d, lay_wide(kWideLayouts[li]));
        if (!back) break;
        ok = ensure_keys_wide(ctx->opt, d, base + n, 0, st);   // (never the one-window 11-bit layout: keys_wide1_cap is moot)
      }
      // a failed rebuild only stops the wide tables (the k6 / k4 ones serve
      // every slot): never a gv_keys_load error
      if (ok && moved && base && build_wide(ctx, d, s, st, old_pub.data(), base, 0) != GV_OK) ok = false;
      if (ok && build_wide(ctx, d, s, st, pub33, n, base) != GV_OK) ok = false;
      if (!ok) {
        (void)hipGetLastError();
        d->keysw = 0;                             // no slot's wide tables are trusted past a failed build
        d->kw_full = true;
      } else {
        d->keysw = base + n;
      }
    }
    // the pubkey index, while every earlier slot is in it: a refused
    // allocation or a failed launch only stops it on this device
    if (kidx_appendable(d->kidx, ctx->opt.keys_index, base)) {
      if (kidx_load(ctx, d, s, st, pub33, n, base) != GV_OK) kidx_stop(d, d->kidx);
      else d->kidx.keys = base + n;
    }
  }
  ctx->keys = base + n;
  for (size_t i = 0; i < n; ++i) slot_out[i] = (uint32_t)(base + i);
  return GV_OK;
}

int gv_keys_replace(gv_ctx* ctx, size_t n, const uint32_t* slots, const uint8_t* pub33) {
  if (!ctx) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (!slots || !pub33) return GV_EINVAL;
  AsyncQuiesce q(ctx);                          // a batch already submitted runs against the old keys
  std::lock_guard<std::mutex> kl(ctx->keys_mu);
  // every check before the first device write (k_keys_tables reads a kzq
  // column before lane 0 overwrites it)
  const size_t count = ctx->keys;
  if (!check_slots(count, n, slots)) return GV_EINVAL;
  std::vector<uint32_t> fs;                    // the slots (and their keys) below a table set's built prefix
  std::vector<uint8_t> fp;
  auto below = [&](size_t lim) {
    fs.clear();
    fp.clear();
    for (size_t i = 0; i < n; ++i)
      if (slots[i] < lim) {
        fs.push_back(slots[i]);
        fp.insert(fp.end(), pub33 + i * 33, pub33 + (i + 1) * 33);
      }
  };
  for (Dev* d : ctx->devs) {                    // every device holds every key
    std::lock_guard<std::mutex> lk(d->mu);
    CK(hipSetDevice(d->id));
    Set* s = &d->set[0];
    hipStream_t st = s->st;
    for (hipStream_t t : d->hi_st) CK(hipStreamSynchronize(t));   // no pipelined ladder reads a row being rewritten
    if (count > d->k4.cap || d->keys6 > d->k4.cap || d->keysw > d->kw.cap) return GV_EINVAL;   // (never: the arenas hold their slots)
    int rc;
    // which: 0 the k4 tables (every slot), 1 the k6 tables (slots below keys6),
    // 2 the wide tables in the arena's layout (slots below keysw); one pass of
    // gv_keys_load's chunks per table set
    for (int which = 0; which < 3; ++which) {
      const size_t lim = which == 0 ? count : which == 1 ? (d->kn.qt ? d->keys6 : 0) : (d->kw.qt ? d->keysw : 0);
      if (lim == 0) continue;
      const uint32_t* sl = slots;
      const uint8_t* pb = pub33;
      size_t m = n;
      if (lim < count) {
        below(lim);
        sl = fs.data();
        pb = fp.data();
        m = fs.size();
      }
      rc = which == 2 ? build_wide(ctx, d, s, st, pb, m, 0, sl)
                      : build_k4k6(ctx, d, s, st, pb, m, 0, sl, which == 0, which == 1);
      if (rc) return rc;
    }
    // the index (whatever the option says now: its rows must not go stale):
    // the named slots' rows, then the table refilled from every row -- the
    // old bytes leave it, and the order of replacements does not matter
    if (d->kidx.filled()) {
      below(d->kidx.keys);
      if (!fs.empty() && kidx_write(ctx, d, s, st, fp.data(), fs.size(), 0, fs.data(), false) != GV_OK)
        kidx_stop(d, d->kidx);
      else
        kidx_refilled(d, d->kidx, d->kidx.keys, st);
    }
  }
  ctx->keys_replaced.fetch_add(n);
  return GV_OK;
}

int gv_keys_reset(gv_ctx* ctx) {
  if (!ctx) return GV_EINVAL;
  AsyncQuiesce q(ctx);
  std::lock_guard<std::mutex> kl(ctx->keys_mu);
  ctx->keys = 0;
  ctx->keys_gen.fetch_add(1);
  for (Dev* d : ctx->devs) {                    // the index is empty with the arena; a stopped one may start again
    std::lock_guard<std::mutex> lk(d->mu);
    kidx_reset(d->kidx);
  }
  return GV_OK;
}

size_t gv_keys_count(const gv_ctx* ctx) { return ctx ? ctx->keys : 0; }

// ---- ed25519 key arena + small keyed batches (k_ed_keys, k_ed_lat_sl)
namespace {
// Growth doubles the arena but stops at the callers' reset point (ed_key_cap:
// GV_ED_KEY_CAP or the option) and past it grows to exactly what is needed:
// the transient peak of a growth -- old and new arena both allocated, 72 KB
// per key each -- stays within cap + the old arena.
int ensure_ed_keys(Dev* d, size_t need, size_t used, hipStream_t st, size_t cap_limit) {
  if (need <= d->ekcap) return GV_OK;
  const size_t cap = arena_grow_cap(d->ekcap, need, cap_limit, 256);
  uint32_t *t = nullptr, *p = nullptr, *o = nullptr;
  auto fail = [&]() {
    for (uint32_t* q : {t, p, o}) if (q) (void)hipFree(q);
    return GV_ENOMEM;
  };
  if (hipMalloc(&t, cap * (size_t)GV_EDK_WORDS * 4) != hipSuccess) return fail();
  if (hipMalloc(&p, cap * 8 * 4) != hipSuccess) return fail();
  if (hipMalloc(&o, cap * 4) != hipSuccess) return fail();
  if (used) {
    CK(hipMemcpyAsync(t, d->ektab, used * (size_t)GV_EDK_WORDS * 4, hipMemcpyDeviceToDevice, st));
    CK(hipMemcpyAsync(p, d->ekpub, used * 8 * 4, hipMemcpyDeviceToDevice, st));
    CK(hipMemcpyAsync(o, d->ekok, used * 4, hipMemcpyDeviceToDevice, st));
    CK(hipStreamSynchronize(st));
  }
  for (uint32_t* q : {d->ektab, d->ekpub, d->ekok}) if (q) (void)hipFree(q);
  d->ektab = t; d->ekpub = p; d->ekok = o; d->ekcap = cap;
  d->ed_kidx.rows = p;                          // (the index reads the arena's rows)
  return GV_OK;
}

// The tables of the n keys pub32 (host) into slots base.. of d's arena, or
// into slots[i] (host, n entries; null: append) -- nothing else in the arena
// moves.  Scratch: the keys, the slot list when there is one, then the window
// bases of the split build.
int ed_build(gv_ctx* ctx, Dev* d, hipStream_t st, const uint8_t* pub32, size_t n, size_t base, const uint32_t* slots) {
  uint8_t* dp = nullptr;
  const size_t o_sl = round_up(n * 32, 256), o_wb = o_sl + (slots ? round_up(n * 4, 256) : 0);
  const size_t wb_bytes = n * 64 * 36 * 4;
  const bool split = ctx->opt.ed_keys_split && wb_bytes <= ((size_t)1 << 30);
  if (hipMalloc(&dp, o_wb + (split ? wb_bytes : 0)) != hipSuccess) return GV_ENOMEM;
  const bool ok = hipMemcpyAsync(dp, pub32, n * 32, hipMemcpyHostToDevice, st) == hipSuccess &&
                  (!slots || hipMemcpyAsync(dp + o_sl, slots, n * 4, hipMemcpyHostToDevice, st) == hipSuccess) &&
                  gvk_ed_keys(dp, (uint32_t)n, slots ? 0u : (uint32_t)base, slots ? (const uint32_t*)(dp + o_sl) : nullptr,
                              d->ektab, d->ekpub, d->ekok, split ? (uint32_t*)(dp + o_wb) : nullptr, 4,
                              st) == hipSuccess &&
                  hipStreamSynchronize(st) == hipSuccess;
  (void)hipFree(dp);
  return ok ? GV_OK : GV_EHIP;
}

// ---- the wide ed25519 arena (option "ed_keys_wide"; ektabw beside ektab)
inline size_t ed_wide_slot_bytes(int rb) {
  return rb == 8 ? (size_t)GV_EDK256_WORDS * 4 : rb == 6 ? (size_t)GV_EDK64_WORDS * 4 : 0;
}
inline size_t ed_wide_windows(int rb) { return rb == 8 ? 32 : 43; }

// Drop the wide ed25519 arena (its memory back to the device).
void free_ed_keys_wide(Dev* d) {
  if (d->ektabw) { (void)hipFree(d->ektabw); d->ektabw = nullptr; }
  d->opt_bytes = budget_replace(d->opt_bytes, d->ekcapw * ed_wide_slot_bytes(d->ekw_rb), 0);
  d->ekcapw = d->ekeysw = 0;
}

// Grow the wide ed25519 arena (radix d->ekw_rb) to `need` slots keeping the
// first `used` -- doubling, not past ed_key_cap, then exact, as
// ensure_ed_keys.  False, and the arena as it was, when `limit` (option
// "ed_keys_wide_mb"; 0: none) or the HBM budget does not hold the new arena,
// when it would take device memory the secp256k1 wide arena keeps free too
// (the k4 / k6 arena's growth to key_cap, the radix-16 ed25519 arena's to
// ed_key_cap, 8 GiB of batch scratch), or when an allocation fails.
bool ensure_ed_keys_wide(gv_ctx* ctx, Dev* d, size_t need, size_t used, hipStream_t st) {
  if (need <= d->ekcapw) return true;
  const size_t cap = arena_grow_cap(d->ekcapw, need, ctx->opt.ed_key_cap, 256);
  const size_t slot_b = ed_wide_slot_bytes(d->ekw_rb);
  if (!slot_b) return false;
  if (ctx->opt.ed_keys_wide_bytes && cap * slot_b > ctx->opt.ed_keys_wide_bytes) return false;
  if (d->opt_bytes + cap * slot_b > ctx->opt.hbm_budget) return false;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
  const size_t reserve = (ctx->opt.key_cap > d->k4.cap ? ctx->opt.key_cap - d->k4.cap : 0) * resident_slot_bytes(true) +
                         (ctx->opt.ed_key_cap > d->ekcap ? ctx->opt.ed_key_cap - d->ekcap : 0) *
                             ((size_t)GV_EDK_WORDS + 8 + 1) * 4 +
                         (size_t(8) << 30);
  if (free_b < cap * slot_b + reserve) return false;
  uint32_t* t = nullptr;
  if (hipMalloc(&t, cap * slot_b) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  used = std::min(used, d->ekeysw);
  if (used && (hipMemcpyAsync(t, d->ektabw, used * slot_b, hipMemcpyDeviceToDevice, st) != hipSuccess ||
               hipStreamSynchronize(st) != hipSuccess)) {
    (void)hipFree(t);
    (void)hipGetLastError();
    return false;
  }
  if (d->ektabw) (void)hipFree(d->ektabw);
  d->opt_bytes = budget_replace(d->opt_bytes, d->ekcapw * slot_b, cap * slot_b);
  d->ektabw = t;
  d->ekcapw = cap;
  return true;
}

// The wide tables of the n keys pub32 (host) into slots base.. of d's wide
// arena, or into slots[i] (host; null: append), by the split build
// (k_ed_keys_chain / k_ed_keys_tab at the arena's radix; the chain rewrites
// the slots' raw key words and verdicts with the values ed_build left), in
// chunks whose window-base scratch stays within ed_build's 1 GiB.
int ed_build_wide(Dev* d, hipStream_t st, const uint8_t* pub32, size_t n, size_t base, const uint32_t* slots) {
  const size_t wb_key = ed_wide_windows(d->ekw_rb) * 36 * 4;
  const size_t step = std::min<size_t>(n, std::min<size_t>(65536, ((size_t)1 << 30) / wb_key));
  const size_t o_sl = round_up(step * 32, 256), o_wb = o_sl + round_up(step * 4, 256);
  uint8_t* dp = nullptr;
  if (hipMalloc(&dp, o_wb + step * wb_key) != hipSuccess) {
    (void)hipGetLastError();
    return GV_ENOMEM;
  }
  bool ok = true;
  for (size_t c0 = 0; ok && c0 < n; c0 += step) {
    const size_t cn = std::min(step, n - c0);
    ok = hipMemcpyAsync(dp, pub32 + c0 * 32, cn * 32, hipMemcpyHostToDevice, st) == hipSuccess &&
         (!slots || hipMemcpyAsync(dp + o_sl, slots + c0, cn * 4, hipMemcpyHostToDevice, st) == hipSuccess) &&
         gvk_ed_keys(dp, (uint32_t)cn, slots ? 0u : (uint32_t)(base + c0), slots ? (const uint32_t*)(dp + o_sl) : nullptr,
                     d->ektabw, d->ekpub, d->ekok, (uint32_t*)(dp + o_wb), d->ekw_rb, st) == hipSuccess &&
         hipStreamSynchronize(st) == hipSuccess;
  }
  (void)hipFree(dp);
  return ok ? GV_OK : GV_EHIP;
}

// A device-resident keyed batch still queued reads the arena: its writers
// (load, replace, a load after reset) wait for it before they write, move or
// free arena memory.  The caller holds ed_keys_mu and d->mu.
int ed_arena_quiesce(Dev* d) {
  if (d->edkd_last_st) CK(hipEventSynchronize(d->edkd_last));
  return GV_OK;
}

// gv_ed_keys_load's part of the pubkey index (option "ed_keys_index"; DESIGN
// section 4.3e), after the load has written the ekpub rows of slots [base,
// base + n): the table for the arena's capacity (d->ekcap), charged to the HBM
// budget like the other optional tables, and the new slots into it.  A table
// that had to grow, and one of an arena restarted from slot 0, is filled from
// every row.
int ed_kidx_load(gv_ctx* ctx, Dev* d, hipStream_t st, size_t n, size_t base) {
  KeyIndex& ix = d->ed_kidx;
  int rc;
  if ((rc = kidx_setup(ctx, d, ix, st))) return rc;
  const size_t T = kidx_table_words(d->ekcap);
  if (T > (size_t(1) << 31)) return GV_ENOMEM;
  if (!ix.tab || ix.T < T) {
    uint32_t* tab = opt_alloc(ctx, d, T * 4);
    if (!tab) return GV_ENOMEM;
    kidx_free(d, ix);
    ix.tab = tab;
    ix.T = T;
    if ((rc = kidx_refill(ix, base + n, st))) return rc;
  } else if (base == 0) {
    if ((rc = kidx_refill(ix, n, st))) return rc;
  } else {
    CK(kidx_put(ix, n, base, nullptr, st));
  }
  return kidx_read_left_out(ix, st);
}
}  // namespace

int gv_ed_keys_load(gv_ctx* ctx, size_t n, const uint8_t* pub32, uint32_t* slot_out) {
  if (!ctx) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (!pub32 || !slot_out) return GV_EINVAL;
  std::lock_guard<std::mutex> kl(ctx->ed_keys_mu);
  const size_t base = ctx->ed_keys;
  if (base + n > kMaxItems) return GV_EINVAL;
  for (Dev* d : ctx->devs) {                    // every device holds every key
    std::lock_guard<std::mutex> lk(d->mu);
    CK(hipSetDevice(d->id));
    hipStream_t st = d->set[0].st;
    int rc = ed_arena_quiesce(d);
    if (rc) return rc;
    if (base == 0) {                            // after gv_ed_keys_reset the slots are rewritten from 0
      d->ekeysw = 0;
      d->ekw_full = false;
      if (d->ekw_rb != ctx->opt.ed_keys_wide) {     // the option is read again: another radix, or none
        free_ed_keys_wide(d);
        d->ekw_rb = ctx->opt.ed_keys_wide;
      }
      kidx_reset(d->ed_kidx);
      d->ed_kidx.on = ctx->opt.ed_keys_index;       // the arena takes the option here
    }
    // an earlier load that failed on a later device left this one's index ahead
    // of the arena (slots the count does not cover): no index until gv_ed_keys_reset
    if (d->ed_kidx.keys > base) kidx_stop(d, d->ed_kidx);
    rc = ensure_ed_keys(d, base + n, base, st, ctx->opt.ed_key_cap);
    if (!rc) rc = ed_build(ctx, d, st, pub32, n, base, nullptr);
    if (rc) return rc;
    // the wide tables while every earlier slot has them and memory holds the
    // grown arena; a refusal or a failed build frees them and stops them until
    // gv_ed_keys_reset (every slot keeps its radix-16 table): never an error
    if (ctx->opt.ed_keys_wide && d->ekw_rb && d->ekeysw == base && !d->ekw_full) {
      if (ensure_ed_keys_wide(ctx, d, base + n, base, st) && ed_build_wide(d, st, pub32, n, base, nullptr) == GV_OK) {
        d->ekeysw = base + n;
      } else {
        (void)hipGetLastError();
        free_ed_keys_wide(d);
        d->ekw_full = true;
      }
    }
    // the index, behind the builds that wrote the slots' ekpub rows (the wide
    // chain rewrites them with the same words); a refusal or a failure stops
    // it until gv_ed_keys_reset: never an error
    if (kidx_appendable(d->ed_kidx, ctx->opt.ed_keys_index, base)) {
      if (ed_kidx_load(ctx, d, st, n, base) != GV_OK) kidx_stop(d, d->ed_kidx);
      else d->ed_kidx.keys = base + n;
    }
  }
  ctx->ed_kpub.insert(ctx->ed_kpub.end(), pub32, pub32 + n * 32);
  ctx->ed_keys = base + n;
  for (size_t i = 0; i < n; ++i) slot_out[i] = (uint32_t)(base + i);
  return GV_OK;
}

int gv_ed_keys_replace(gv_ctx* ctx, size_t n, const uint32_t* slots, const uint8_t* pub32) {
  if (!ctx) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (!slots || !pub32) return GV_EINVAL;
  // keyed verifies hold ed_keys_mu for the whole call: none runs under a replacement
  std::lock_guard<std::mutex> kl(ctx->ed_keys_mu);
  // every check before the first device write
  const size_t count = ctx->ed_keys;
  if (!check_slots(count, n, slots)) return GV_EINVAL;
  std::vector<uint32_t> ws;                     // the slots (and their keys) below the wide tables' built prefix
  std::vector<uint8_t> wp;
  for (Dev* d : ctx->devs) {                    // every device holds every key
    std::lock_guard<std::mutex> lk(d->mu);
    CK(hipSetDevice(d->id));
    if (count > d->ekcap || d->ekeysw > d->ekcapw) return GV_EINVAL;   // (never: the arenas hold their slots)
    int rc = ed_arena_quiesce(d);               // a batch already enqueued runs against the old keys
    if (!rc) rc = ed_build(ctx, d, d->set[0].st, pub32, n, 0, slots);
    // the index names bytes: once rows may have changed it is refilled from
    // every row or stopped, whatever "ed_keys_index" says now
    const bool indexed = d->ed_kidx.filled();
    if (rc) {
      if (indexed) kidx_stop(d, d->ed_kidx);
      return rc;
    }
    if (indexed) kidx_refilled(d, d->ed_kidx, std::min(d->ed_kidx.keys, count), d->set[0].st);
    if (d->ektabw && d->ekeysw) {               // the wide tables of the named slots that have them
      const uint32_t* sl = slots;
      const uint8_t* pb = pub32;
      size_t m = n;
      if (d->ekeysw < count) {
        ws.clear();
        wp.clear();
        for (size_t i = 0; i < n; ++i)
          if (slots[i] < d->ekeysw) {
            ws.push_back(slots[i]);
            wp.insert(wp.end(), pub32 + i * 32, pub32 + (i + 1) * 32);
          }
        sl = ws.data();
        pb = wp.data();
        m = ws.size();
      }
      if (m && (rc = ed_build_wide(d, d->set[0].st, pb, m, 0, sl))) return rc;
    }
  }
  // the host copy (large batches with ed_keyed 0 read it) only after every device has succeeded
  for (size_t i = 0; i < n; ++i) memcpy(&ctx->ed_kpub[(size_t)slots[i] * 32], pub32 + i * 32, 32);
  ctx->ed_keys_replaced.fetch_add(n);
  return GV_OK;
}

int gv_ed_keys_point(gv_ctx* ctx, size_t n, const uint32_t* slots, uint32_t w, uint32_t j, uint8_t* out_enc32,
                     uint8_t* out_pub32, uint8_t* out_ok) {
  if (!ctx) return GV_EINVAL;
  if (w >= 64 || j < 1 || j > 8) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (!slots || !out_enc32 || !out_pub32 || !out_ok || n > kMaxItems) return GV_EINVAL;
  std::lock_guard<std::mutex> kl(ctx->ed_keys_mu);
  Dev* d = ctx->devs[0];
  std::lock_guard<std::mutex> lk(d->mu);
  CK(hipSetDevice(d->id));
  hipStream_t st = d->set[0].st;
  // an arena never allocated (or smaller than the count: never) reads as empty
  const size_t kcount = std::min(ctx->ed_keys, d->ekcap);
  uint8_t* buf = nullptr;
  const size_t sb = round_up(n * 4, 256), eb = round_up(n * 32, 256);
  if (hipMalloc(&buf, sb + 2 * eb + n) != hipSuccess) return GV_ENOMEM;
  int rc = GV_OK;
  if (hipMemcpyAsync(buf, slots, n * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
      gvk_ed_keys_point((uint32_t)n, (const uint32_t*)buf, w, j, d->ektab, d->ekpub, d->ekok, (uint32_t)kcount,
                        buf + sb, buf + sb + eb, buf + sb + 2 * eb, st) != hipSuccess ||
      hipMemcpyAsync(out_enc32, buf + sb, n * 32, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(out_pub32, buf + sb + eb, n * 32, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(out_ok, buf + sb + 2 * eb, n, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    rc = GV_EHIP;
  (void)hipFree(buf);
  return rc;
}

int gv_ed_keys_reset(gv_ctx* ctx) {
  if (!ctx) return GV_EINVAL;
  std::lock_guard<std::mutex> kl(ctx->ed_keys_mu);
  ctx->ed_keys = 0;
  ctx->ed_kpub.clear();
  for (Dev* d : ctx->devs) {                    // the wide tables start over with the arena (memory kept for the next load)
    std::lock_guard<std::mutex> lk(d->mu);
    d->ekeysw = 0;
    d->ekw_full = false;
    kidx_reset(d->ed_kidx);                       // the index too
  }
  ctx->ed_keys_gen.fetch_add(1);
  return GV_OK;
}
size_t gv_ed_keys_count(const gv_ctx* ctx) { return ctx ? ctx->ed_keys : 0; }
uint64_t gv_ed_keys_generation(const gv_ctx* ctx) { return ctx ? ctx->ed_keys_gen.load() : 0; }

namespace {
struct EdKeyedHost {
  const uint32_t* slot;
  const uint8_t* sig64;
  const uint8_t* blob;
  const uint64_t* off;
  const uint32_t* len;
  uint8_t* out_ok;
};

int ensure_dev(uint8_t** p, size_t* cap, size_t bytes) {
  if (bytes <= *cap) return GV_OK;
  if (*p) (void)hipFree(*p);
  *cap = 0;
  const size_t c = round_up(bytes, (size_t)1 << 20);
  if (hipMalloc((void**)p, c) != hipSuccess) { *p = nullptr; return GV_ENOMEM; }
  *cap = c;
  return GV_OK;
}

// Items [lo, hi) of a large keyed ed25519 batch on one device (k_ed_keyed):
// chunks alternate between two buffers / streams, so the host staging of
// chunk i + 1 (slots, signatures, offsets, messages into pinned memory) runs
// while chunk i copies and computes; lanes sorted by slot on the device.
int ed_keyed_slice(gv_ctx* ctx, Dev* d, size_t lo, size_t hi, const EdKeyedHost& hb, size_t kcount) {
  std::lock_guard<std::mutex> lk(d->mu);
  CK(hipSetDevice(d->id));
  int rc = ed_ensure(d, 256, d->set[0].st);       // the resident comb table of B
  if (rc) return rc;
  const size_t n = hi - lo;
  const size_t chunk = std::min<size_t>(ctx->opt.max_batch, n > 131072 ? round_up((n + 3) / 4, 256) : n);
  const size_t nb = kcount + 1, tb = gvk_sort_temp_bytes((uint32_t)nb);
  struct Pending { size_t c0 = 0, cn = 0, o_out = 0; bool busy = false; } pend[2];
  auto finish = [&](int k) -> int {                // chunk on buffer k: wait, copy the verdicts out
    if (!pend[k].busy) return GV_OK;
    pend[k].busy = false;
    CK(hipStreamSynchronize(d->set[k].st));
    memcpy(hb.out_ok + pend[k].c0, d->edk_h[k] + pend[k].o_out, pend[k].cn);
    return GV_OK;
  };
  auto submit = [&](int k, size_t c0) -> int {
    int rc = finish(k);
    if (rc) return rc;
    hipStream_t st = d->set[k].st;
    const size_t cn = std::min(chunk, hi - c0);
    const auto [lo_b, hi_b] = msg_range(hb.off, hb.len, c0, c0 + cn);
    const size_t o_sig = round_up(cn * 4, 256), o_off = o_sig + cn * 64, o_len = o_off + cn * 8,
                 o_out = o_len + cn * 4, o_blob = round_up(o_out + cn, 256), total = o_blob + (hi_b - lo_b);
    const size_t C = round_up(cn, 256), sw = sort_words(C, nb, tb);
    if ((rc = ensure_pinned(&d->edk_h[k], &d->edk_h_cap[k], total))) return rc;
    if ((rc = ensure_dev(&d->edk_d[k], &d->edk_d_cap[k], total))) return rc;
    if ((rc = ensure_dev((uint8_t**)&d->edk_s[k], &d->edk_s_cap[k], sw * 4))) return rc;
    uint8_t* h = d->edk_h[k];
    const CopySeg segs[2] = {CopySeg{h, (const uint8_t*)(hb.slot + c0), cn * 4},
                             CopySeg{h + o_sig, hb.sig64 + c0 * 64, cn * 64}};
    par_copy_segs(d->pool, segs, 2);
    uint64_t* ro = (uint64_t*)(h + o_off);
    for (size_t i = 0; i < cn; ++i) ro[i] = hb.off[c0 + i] - lo_b;
    memcpy(h + o_len, hb.len + c0, cn * 4);
    if (hi_b > lo_b) par_copy(d->pool, h + o_blob, hb.blob + lo_b, hi_b - lo_b);
    uint8_t* dd = d->edk_d[k];
    CK(hipMemcpyAsync(dd, h, total, hipMemcpyHostToDevice, st));
    const gvk_sort so = carve_sort(d->edk_s[k], C, nb, tb);
    if (ctx->opt.sort_keys) CK(gvk_sort_slots(&so, (uint32_t)cn, (const uint32_t*)dd, (uint32_t)kcount, st));
    const gvk_edk b = fill_edk(ctx, d, cn, kcount, ctx->opt.sort_keys ? so.perm : nullptr, (const uint32_t*)dd, dd + o_sig,
                               dd + o_blob, (const uint64_t*)(dd + o_off), (const uint32_t*)(dd + o_len), dd + o_out,
                               ed_btab16(d, ctx->opt.ed_btab16, st));
    CK(gvk_ed_keyed(&b, st));
    CK(hipMemcpyAsync(h + o_out, dd + o_out, cn, hipMemcpyDeviceToHost, st));
    pend[k] = Pending{c0, cn, o_out, true};
    return GV_OK;
  };
  int k = 0;
  for (size_t c0 = lo; c0 < hi && rc == GV_OK; c0 += chunk, k ^= 1) rc = submit(k, c0);
  for (int j = 0; j < 2; ++j) {                   // drain, the older chunk first (also after an error)
    const int r2 = finish(k ^ j);
    if (rc == GV_OK) rc = r2;
  }
  if (rc) {
    (void)hipStreamSynchronize(d->set[0].st);
    (void)hipStreamSynchronize(d->set[1].st);
  }
  return rc;
}
}  // namespace

int gv_verify_ed25519_msgs_keyed(gv_ctx* ctx, size_t n, const uint32_t* slot, const uint8_t* sig64,
                                 const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len,
                                 uint8_t* out_ok) {
  if (!ctx) return GV_EINVAL;
  if (ctx->opt.fault_inject) return GV_EFAULT;
  if (n == 0) return GV_OK;
  if (!slot || !sig64 || !msg_off || !msg_len || !out_ok) return GV_EINVAL;
  for (size_t i = 0; i < n; ++i)
    if (msg_len[i] && !msg_blob) return GV_EINVAL;
  // ed_keys_mu is held for the whole call, small batches included: a
  // concurrent gv_ed_keys_reset + load cannot move a slot between the lookup
  // of kcount and the kernel (the large-batch path always held it; lock order
  // ed_keys_mu -> d->mu, as in gv_ed_keys_load)
  std::lock_guard<std::mutex> kl(ctx->ed_keys_mu);
  const size_t kcount = ctx->ed_keys;
  {
    if (n > ctx->opt.ed_lat_max && kcount && ctx->opt.ed_keyed) {
      // large batches: one signature per lane against the key tables
      // (k_ed_keyed), split over the devices like run_ed_host
      const EdKeyedHost hb{slot, sig64, msg_blob, msg_off, msg_len, out_ok};
      return run_sliced(workers(ctx), n, 256, [&](size_t k, size_t lo, size_t hi) {
        return ed_keyed_slice(ctx, ctx->devs[k], lo, hi, hb, kcount);
      });
    }
    if (n > ctx->opt.ed_lat_max || kcount == 0) {
      // large batches (ed_keyed 0): the throughput kernels over the slots' raw keys
      std::vector<uint8_t> pub(n * 32, 0);
      for (size_t i = 0; i < n; ++i)
        if (slot[i] < kcount) memcpy(&pub[i * 32], &ctx->ed_kpub[(size_t)slot[i] * 32], 32);
      int rc = kcount ? run_ed_host(ctx, n, EdHost{pub.data(), sig64, msg_blob, msg_off, msg_len, out_ok}) : GV_OK;
      if (rc) return rc;
      for (size_t i = 0; i < n; ++i)
        if (slot[i] >= kcount) out_ok[i] = 0;              // no key in that slot: never a valid signature
      return GV_OK;
    }
  }
  Dev* d = ctx->devs[0];
  std::lock_guard<std::mutex> lk(d->mu);
  CK(hipSetDevice(d->id));
  hipStream_t st = d->set[0].st;
  int rc = ed_ensure(d, 256, st);                 // the resident comb table of B
  if (rc) return rc;
  const auto [lo, hi] = msg_range(msg_off, msg_len, 0, n);
  // zero-copy: the kernel reads the pinned inputs and writes verdict bytes
  const size_t o_sig = round_up(n * 4, 64), o_off = o_sig + n * 64, o_len = o_off + n * 8, o_out = o_len + n * 4,
               o_blob = round_up(o_out + n, 64), total = o_blob + (hi - lo);
  if ((rc = ensure_pinned(&d->edl_h, &d->edl_h_cap, total))) return rc;
  uint8_t* h = d->edl_h;
  memcpy(h, slot, n * 4);
  memcpy(h + o_sig, sig64, n * 64);
  uint64_t* ro = (uint64_t*)(h + o_off);
  for (size_t i = 0; i < n; ++i) ro[i] = msg_off[i] - lo;
  memcpy(h + o_len, msg_len, n * 4);
  if (hi > lo) memcpy(h + o_blob, msg_blob + lo, hi - lo);
  const gvk_edl b = fill_edl(d, n, kcount, (const uint32_t*)h, h + o_sig, h + o_blob, (const uint64_t*)(h + o_off),
                             (const uint32_t*)(h + o_len), h + o_out);
  CK(gvk_ed_lat(&b, st));
  CK(hipStreamSynchronize(st));
  memcpy(out_ok, h + o_out, n);
  return GV_OK;
}

// Device-resident keyed ed25519: batches up to "ed_lat_max" on k_ed_lat_sl
// (the radix-16 tables), larger ones on k_ed_keyed in slot order -- the wide
// tables when every slot has them --, whatever "ed_keyed" says (no host copy
// of the items exists for the throughput kernels).  Either kernel writes a
// verdict byte per item into the device's scratch; k_ed_pack_bits makes the
// bitmap.  ed_keys_mu is held while the batch is enqueued and edkd_last is
// recorded behind its last kernel: the arena's writers wait for it.
//
// ed_dev_keyed is that batch for both of its callers, which hold ed_keys_mu
// and d->mu: gv_dev_verify_ed25519_msgs_keyed with the caller's d_slot, and
// gv_dev_verify_ed25519_msgs (option "ed_keys_index") with d_slot null and the
// batch's d_pub32 -- the slots are then looked up into the same scratch, n
// words behind the sort's, by one k_kidx_find ordered behind edkd_last like
// every other user of it, and the host waits for the miss count.  Any miss:
// *missed is set and nothing else was enqueued (the caller takes the pub32
// route).  kcount > 0.
namespace {
int ed_dev_keyed(gv_ctx* ctx, Dev* d, size_t n, size_t kcount, const uint32_t* d_slot, const uint8_t* d_pub32,
                 const void* d_sig64, const void* d_msg_blob, const void* d_msg_off, const void* d_msg_len, void* d_bits,
                 hipStream_t st, bool* missed) {
  int rc;
  if ((rc = ed_ensure(d, 256, st))) return rc;    // the resident comb table of B
  if (!d->edkd_last) CK(hipEventCreateWithFlags(&d->edkd_last, hipEventDisableTiming));
  const bool small = n <= ctx->opt.ed_lat_max;
  const bool sorted = !small && ctx->opt.sort_keys;
  const size_t C = round_up(n, 256), nb = kcount + 1, tb = gvk_sort_temp_bytes((uint32_t)nb);
  const size_t sw = sorted ? sort_words(C, nb, tb) : 0;
  const size_t need = C + sw * 4 + (d_slot ? 0 : n * 4);
  if (need > d->edkd_s_cap) {                     // the scratch grows: the last batch on it first
    if (d->edkd_last_st) CK(hipEventSynchronize(d->edkd_last));
    if ((rc = ensure_dev(&d->edkd_s, &d->edkd_s_cap, need))) return rc;
  }
  if (d->edkd_last_st && d->edkd_last_st != st) CK(hipStreamWaitEvent(st, d->edkd_last, 0));
  if (!d_slot) {
    uint32_t* found = (uint32_t*)(d->edkd_s + C + sw * 4);
    size_t nmiss = 0;
    if ((rc = kidx_lookup(d->ed_kidx, ctx->ed_keys, n, d_pub32, found, st, &nmiss, nullptr))) return rc;
    if (nmiss) {
      *missed = true;
      return GV_OK;
    }
    d_slot = found;
  }
  uint8_t* out8 = d->edkd_s;
  if (small) {
    const gvk_edl b = fill_edl(d, n, kcount, d_slot, (const uint8_t*)d_sig64, (const uint8_t*)d_msg_blob,
                               (const uint64_t*)d_msg_off, (const uint32_t*)d_msg_len, out8);
    CK(gvk_ed_lat(&b, st));
  } else {
    const uint32_t* btab16 = ed_btab16(d, ctx->opt.ed_btab16, st);
    const uint32_t* perm = nullptr;
    if (sorted) {
      const gvk_sort so = carve_sort((uint32_t*)(d->edkd_s + C), C, nb, tb);
      CK(gvk_sort_slots(&so, (uint32_t)n, d_slot, (uint32_t)kcount, st));
      perm = so.perm;
    }
    const gvk_edk b = fill_edk(ctx, d, n, kcount, perm, d_slot, (const uint8_t*)d_sig64, (const uint8_t*)d_msg_blob,
                               (const uint64_t*)d_msg_off, (const uint32_t*)d_msg_len, out8, btab16);
    CK(gvk_ed_keyed(&b, st));
  }
  CK(gvk_ed_pack_bits((uint32_t)n, out8, (uint64_t*)d_bits, st));
  CK(hipEventRecord(d->edkd_last, st));
  d->edkd_last_st = st;
  return GV_OK;
}
}  // namespace

int gv_dev_verify_ed25519_msgs_keyed(gv_ctx* ctx, int dev_slot, size_t n, const void* d_slot, const void* d_sig64,
                                     const void* d_msg_blob, const void* d_msg_off, const void* d_msg_len,
                                     void* d_bits, void* stream) {
  Dev* d = nullptr;
  int rc = dev_common(ctx, dev_slot, n, d_slot, d_sig64, d_bits, &d);
  if (rc || n == 0) return rc;
  if (!d_msg_off || !d_msg_len || ((uintptr_t)d_sig64 & 15)) return GV_EINVAL;
  std::lock_guard<std::mutex> kl(ctx->ed_keys_mu);
  std::lock_guard<std::mutex> lk(d->mu);
  CK(hipSetDevice(d->id));
  hipStream_t st = stream ? (hipStream_t)stream : d->set[0].st;
  order_after_pipeline(d, st);
  // an arena never allocated (or smaller than the count: never) reads as empty
  const size_t kcount = std::min(ctx->ed_keys, d->ekcap);
  if (kcount == 0) {                              // no key in any slot: no launch reads the arena
    CK(hipMemsetAsync(d_bits, 0, (n + 63) / 64 * 8, st));
    return GV_OK;
  }
  return ed_dev_keyed(ctx, d, n, kcount, (const uint32_t*)d_slot, nullptr, d_sig64, d_msg_blob, d_msg_off, d_msg_len,
                      d_bits, st, nullptr);
}

// gv_dev_verify_ed25519_msgs: device-resident pub32 items.  With
// "ed_keys_index" on it takes ed_keys_mu, then d->mu, and a batch whose keys
// the live index all names runs as gv_dev_verify_ed25519_msgs_keyed would with
// those slots (one hit); any miss (one miss) and every other case run
// ed_launch as before.  Off: d->mu alone, as ever.
int gv_dev_verify_ed25519_msgs(gv_ctx* ctx, int dev_slot, size_t n, const void* d_pub32, const void* d_sig64,
                               const void* d_msg_blob, const void* d_msg_off, const void* d_msg_len, void* d_bits,
                               void* stream) {
  Dev* d = nullptr;
  int rc = dev_common(ctx, dev_slot, n, d_pub32, d_sig64, d_bits, &d);
  if (rc || n == 0) return rc;
  if (!d_msg_off || !d_msg_len || ((uintptr_t)d_pub32 & 15) || ((uintptr_t)d_sig64 & 15)) return GV_EINVAL;
  std::unique_lock<std::mutex> kl;
  if (ctx->opt.ed_keys_index) kl = std::unique_lock<std::mutex>(ctx->ed_keys_mu);
  std::lock_guard<std::mutex> lk(d->mu);
  CK(hipSetDevice(d->id));
  hipStream_t st = stream ? (hipStream_t)stream : d->set[0].st;
  order_after_pipeline(d, st);
  if (kl.owns_lock() && ctx->opt.ed_keys_index && ctx->ed_keys && ctx->ed_keys <= d->ekcap && ed_kidx_live(ctx, d)) {
    bool missed = false;
    if ((rc = ed_dev_keyed(ctx, d, n, ctx->ed_keys, nullptr, (const uint8_t*)d_pub32, d_sig64, d_msg_blob, d_msg_off,
                           d_msg_len, d_bits, st, &missed)))
      return rc;
    (missed ? ctx->ed_kidx_stat.miss : ctx->ed_kidx_stat.hit)++;
    if (!missed) return GV_OK;
  }
  return ed_launch(ctx->opt.time_kernels, d, n, (const uint8_t*)d_pub32, (const uint8_t*)d_sig64, (const uint8_t*)d_msg_blob,
                   (const uint64_t*)d_msg_off, (const uint32_t*)d_msg_len, (uint64_t*)d_bits, st, ed_group_cfg(ctx));
}

int gv_ed_keys_find(gv_ctx* ctx, size_t n, const uint8_t* pub32, uint32_t* slot_out) {
  if (!ctx) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (!pub32 || !slot_out || n > kMaxItems) return GV_EINVAL;
  std::lock_guard<std::mutex> kl(ctx->ed_keys_mu);
  Dev* d = ctx->devs[0];
  std::lock_guard<std::mutex> lk(d->mu);
  if (!ed_kidx_live(ctx, d)) return GV_EINVAL;   // cannot tell (not: not resident)
  return kidx_find_host(d, d->ed_kidx, ctx->ed_keys, n, pub32, slot_out);
}

// Asynchronous on `stream`: the lookup reads the table and the arena's rows,
// so it is ordered behind edkd_last and recorded as the last reader of the
// arena, like a keyed batch (gv_ed_keys_load / _replace wait for it).
int gv_dev_ed_keys_find(gv_ctx* ctx, int dev_slot, size_t n, const void* d_pub32, void* d_slot_out, void* stream) {
  if (!ctx) return GV_EINVAL;
  if (dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return GV_ENODEV;
  if (n == 0) return GV_OK;
  if (!d_pub32 || !d_slot_out || ((uintptr_t)d_slot_out & 3) || n > kMaxItems) return GV_EINVAL;
  Dev* d = ctx->devs[dev_slot];
  std::lock_guard<std::mutex> kl(ctx->ed_keys_mu);
  std::lock_guard<std::mutex> lk(d->mu);
  if (!ed_kidx_live(ctx, d)) return GV_EINVAL;
  CK(hipSetDevice(d->id));
  hipStream_t st = stream ? (hipStream_t)stream : d->set[0].st;
  order_after_pipeline(d, st);
  if (ctx->ed_keys == 0) {
    CK(hipMemsetAsync(d_slot_out, 0xFF, n * 4, st));
    return GV_OK;
  }
  if (!d->edkd_last) CK(hipEventCreateWithFlags(&d->edkd_last, hipEventDisableTiming));
  if (d->edkd_last_st && d->edkd_last_st != st) CK(hipStreamWaitEvent(st, d->edkd_last, 0));
  CK(kidx_find(d->ed_kidx, ctx->ed_keys, (const uint8_t*)d_pub32, n, (uint32_t*)d_slot_out, nullptr, st));
  ctx->ed_kidx_stat.launches++;
  CK(hipEventRecord(d->edkd_last, st));
  d->edkd_last_st = st;
  return GV_OK;
}

int gv_ed_keys_wide_point(gv_ctx* ctx, size_t n, const uint32_t* slots, uint32_t w, uint32_t j, uint8_t* out_enc32,
                          uint8_t* out_ok) {
  if (!ctx) return GV_EINVAL;
  std::lock_guard<std::mutex> kl(ctx->ed_keys_mu);
  Dev* d = ctx->devs[0];
  std::lock_guard<std::mutex> lk(d->mu);
  const size_t kcount = d->ektabw ? std::min(std::min(d->ekeysw, d->ekcapw), ctx->ed_keys) : 0;
  const int rb = kcount ? d->ekw_rb : 0;
  if (rb != 6 && rb != 8) return GV_EINVAL;       // no wide arena
  if (w >= ed_wide_windows(rb) || j < 1 || j > (1u << (rb - 1))) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (!slots || !out_enc32 || !out_ok || n > kMaxItems) return GV_EINVAL;
  CK(hipSetDevice(d->id));
  hipStream_t st = d->set[0].st;
  uint8_t* buf = nullptr;
  const size_t sb = round_up(n * 4, 256), eb = round_up(n * 32, 256);
  if (hipMalloc(&buf, sb + eb + n) != hipSuccess) return GV_ENOMEM;
  int rc = GV_OK;
  if (hipMemcpyAsync(buf, slots, n * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
      gvk_ed_keys_wide_point((uint32_t)n, (const uint32_t*)buf, w, j, rb, d->ektabw, d->ekok, (uint32_t)kcount, buf + sb,
                             buf + sb + eb, st) != hipSuccess ||
      hipMemcpyAsync(out_enc32, buf + sb, n * 32, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(out_ok, buf + sb + eb, n, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    rc = GV_EHIP;
  (void)hipFree(buf);
  return rc;
}

int gv_host_alloc(gv_ctx* ctx, size_t bytes, void** out) {
  if (!ctx || !out || bytes == 0) return GV_EINVAL;
  *out = nullptr;
  if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) { *out = nullptr; return GV_ENOMEM; }
  return GV_OK;
}
int gv_host_free(gv_ctx* ctx, void* p) {
  if (!ctx) return GV_EINVAL;
  if (p && hipHostFree(p) != hipSuccess) return GV_EHIP;
  return GV_OK;
}

int gv_route_stats(gv_ctx* ctx, int dev_slot, uint64_t out[GV_ROUTES]) {
  if (!ctx || !out || dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return GV_EINVAL;
  Dev* d = ctx->devs[dev_slot];
  std::lock_guard<std::mutex> lk(d->mu);
  for (int i = 0; i < GV_ROUTES; ++i) out[i] = d->routes[i];
  return GV_OK;
}

int gv_group_stats(gv_ctx* ctx, int dev_slot, uint64_t* batches, uint64_t* keys) {
  if (!ctx || dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return GV_EINVAL;
  Dev* d = ctx->devs[dev_slot];
  std::lock_guard<std::mutex> lk(d->mu);
  if (batches) *batches = d->grouped_batches + d->ed_grouped_batches;
  if (keys) *keys = d->grouped_keys + d->ed_grouped_keys;
  return GV_OK;
}

int gv_last_slices(gv_ctx* ctx, double* ms_out, size_t* n_out, int cap) {
  if (!ctx || cap < 0 || (cap > 0 && (!ms_out || !n_out))) return GV_EINVAL;
  const int m = std::min<int>(cap, (int)ctx->devs.size());
  for (int k = 0; k < m; ++k) {
    Dev* d = ctx->devs[k];
    std::lock_guard<std::mutex> lk(d->mu);
    ms_out[k] = d->last_slice_ms;
    n_out[k] = d->last_slice_n;
  }
  return m;
}
uint64_t gv_keys_generation(const gv_ctx* ctx) { return ctx ? ctx->keys_gen.load() : 0; }

int gv_keys_point(gv_ctx* ctx, size_t n, const uint32_t* slots, uint8_t* out_xy64, uint8_t* out_ok) {
  if (!ctx) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (!slots || !out_xy64 || !out_ok || n > kMaxItems) return GV_EINVAL;
  Dev* d = ctx->devs[0];
  std::lock_guard<std::mutex> lk(d->mu);
  CK(hipSetDevice(d->id));
  hipStream_t st = d->set[0].st;
  int rc = ensure_keys(d, 1, ctx->keys, st, ctx->opt.key_cap, ctx->opt.hbm_budget, nullptr);
  return rc ? rc : keys_point_read(d, st, n, slots, ctx->keys, out_xy64, out_ok);
}

namespace {
// Every group below the layout's NG, every entry in 1..NT.
bool entry_args_ok(const KeyView& t, size_t n, const uint32_t* groups, const uint32_t* js) {
  for (size_t i = 0; i < n; ++i)
    if (groups[i] >= t.lay.ng || js[i] < 1 || js[i] > t.lay.nt) return false;
  return true;
}
// The triples up, k_keys_entry, the points and verdicts down; scratch of the
// call's own (nothing of the context is written).  An arena with no slot to
// read answers zeros without a launch.
int entry_read(const KeyView& t, hipStream_t st, size_t n, const uint32_t* slots, const uint32_t* groups,
               const uint32_t* js, uint8_t* out_xy64, uint8_t* out_ok) {
  if (t.kcount == 0 || !t.kqt || !t.kqt2 || !t.kzq || !t.kok) {
    memset(out_xy64, 0, n * 64);
    memset(out_ok, 0, n);
    return hipStreamSynchronize(st) == hipSuccess ? GV_OK : GV_EHIP;
  }
  uint8_t* buf = nullptr;
  const size_t sb = round_up(n * 4, 256), xb = round_up(n * 64, 256);
  if (hipMalloc(&buf, 3 * sb + xb + n) != hipSuccess) return GV_ENOMEM;
  int rc = GV_OK;
  uint8_t *d_xy = buf + 3 * sb, *d_ok = d_xy + xb;
  if (hipMemcpyAsync(buf, slots, n * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(buf + sb, groups, n * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(buf + 2 * sb, js, n * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
      gvk_keys_entry((uint32_t)n, (const uint32_t*)buf, (const uint32_t*)(buf + sb), (const uint32_t*)(buf + 2 * sb),
                     t.kqt, t.kqt2, t.kzq, t.kC, t.kok, t.kcount, t.lay.nt, t.lay.ew, t.lay.ng, d_xy, d_ok,
                     st) != hipSuccess ||
      hipMemcpyAsync(out_xy64, d_xy, n * 64, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(out_ok, d_ok, n, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    rc = GV_EHIP;
  (void)hipFree(buf);
  return rc;
}
}  // namespace

int gv_keys_entry(gv_ctx* ctx, int dev_slot, int tabs, size_t n, const uint32_t* slots, const uint32_t* groups,
                  const uint32_t* js, uint8_t* out_xy64, uint8_t* out_ok) {
  if (!ctx || dev_slot < 0 || dev_slot >= (int)ctx->devs.size() || tabs < 0 || tabs > 2) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (!slots || !groups || !js || !out_xy64 || !out_ok || n > kMaxItems) return GV_EINVAL;
  Dev* d = ctx->devs[dev_slot];
  std::lock_guard<std::mutex> lk(d->mu);
  // the slots that have the set's tables: all (k4), below keys6 (kn), below keysw (wide)
  const KeyTabs& tb = tabs == 0 ? d->k4 : tabs == 1 ? d->kn : d->kw;
  if (tabs && (!tb.qt || !tb.lay.ng)) return GV_EINVAL;
  KeyView t(tb, std::min({ctx->keys, tabs == 0 ? ctx->keys : tabs == 1 ? d->keys6 : d->keysw, tb.cap}), d->k4.ok);
  if (tabs == 0) t.lay = lay_k4();              // (an arena never loaded answers zeros, not an error)
  if (!entry_args_ok(t, n, groups, js)) return GV_EINVAL;
  CK(hipSetDevice(d->id));
  return entry_read(t, d->set[0].st, n, slots, groups, js, out_xy64, out_ok);
}

int gv_group_entry(gv_ctx* ctx, int dev_slot, int set, size_t n, const uint32_t* rows, const uint32_t* groups,
                   const uint32_t* js, uint8_t* out_key33, uint8_t* out_xy64, uint8_t* out_ok) {
  if (!ctx || dev_slot < 0 || dev_slot >= (int)ctx->devs.size() || set < 0 || set > 3) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (!rows || !groups || !js || !out_key33 || !out_xy64 || !out_ok || n > kMaxItems) return GV_EINVAL;
  Dev* d = ctx->devs[dev_slot];
  std::lock_guard<std::mutex> lk(d->mu);
  const Set* s = set < 2 ? &d->set[set] : &d->gset[set - 2];
  if (!s->g_live || !s->gk.qt || !s->g_rows || !s->gk.lay.nt || s->g_lng < 2 || s->g_lng > (int)s->gk.lay.ng)
    return GV_EINVAL;
  const size_t count = std::min(s->g_count, s->gk.cap);
  KeyView t(s->gk, count);
  t.lay.ng = (uint32_t)s->g_lng;                  // (k4's four groups in a promotion's arena)
  if (!entry_args_ok(t, n, groups, js)) return GV_EINVAL;
  CK(hipSetDevice(d->id));
  // after the set's last work (an asynchronous gv_dev_verify_* call) and the
  // table build on its side stream
  hipStream_t st = d->set[0].st;
  if (s->last && s->last_st && s->last_st != st) CK(hipStreamWaitEvent(st, s->last, 0));
  if (s->keys_done) CK(hipStreamWaitEvent(st, s->keys_done, 0));
  std::vector<uint32_t> krows(count * GV_KIDX_ROW);
  if (count) CK(hipMemcpyAsync(krows.data(), s->g_rows, count * GV_KIDX_ROW * 4, hipMemcpyDeviceToHost, st));
  std::vector<uint8_t> xy(n * 64), ok(n);
  const int rc = entry_read(t, st, n, rows, groups, js, xy.data(), ok.data());   // (synchronizes st)
  if (rc) return rc;
  memcpy(out_xy64, xy.data(), n * 64);
  memcpy(out_ok, ok.data(), n);
  for (size_t i = 0; i < n; ++i) {
    uint8_t* p = out_key33 + i * 33;
    memset(p, 0, 33);
    if (rows[i] >= count) continue;
    const uint32_t* r = &krows[(size_t)rows[i] * GV_KIDX_ROW];
    p[0] = (uint8_t)r[0];
    for (int w = 0; w < 8; ++w)
      for (int b = 0; b < 4; ++b) p[1 + 4 * (7 - w) + b] = (uint8_t)(r[1 + w] >> (24 - 8 * b));
  }
  return GV_OK;
}

int gv_keys_find(gv_ctx* ctx, size_t n, const uint8_t* pub33, uint32_t* slot_out) {
  if (!ctx) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (!pub33 || !slot_out || n > kMaxItems) return GV_EINVAL;
  Dev* d = ctx->devs[0];
  std::lock_guard<std::mutex> lk(d->mu);
  if (!kidx_live(ctx, d)) return GV_EINVAL;     // cannot tell (not: not resident)
  return kidx_find_host(d, d->kidx, ctx->keys, n, pub33, slot_out);
}

int gv_dev_keys_find(gv_ctx* ctx, int dev_slot, size_t n, const void* d_pub33, void* d_slot_out, void* stream) {
  if (!ctx) return GV_EINVAL;
  if (dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return GV_ENODEV;
  if (n == 0) return GV_OK;
  if (!d_pub33 || !d_slot_out || ((uintptr_t)d_slot_out & 3) || n > kMaxItems) return GV_EINVAL;
  Dev* d = ctx->devs[dev_slot];
  std::lock_guard<std::mutex> lk(d->mu);
  if (!kidx_live(ctx, d)) return GV_EINVAL;
  CK(hipSetDevice(d->id));
  if (!stream && !d->kidx_found) CK(hipEventCreateWithFlags(&d->kidx_found, hipEventDisableTiming));
  // n = 0 to dev_run: on the context stream the lookup is ordered like a small
  // batch -- after every pipelined ladder, and the next ladder after it; the
  // front kernels of the pipelined calls that follow (which read d_slot_out
  // when it is their d_slot) wait for kidx_found
  return dev_run(ctx, d, stream, 0, false, [&](Set*, hipStream_t st, hipStream_t) -> int {
    if (ctx->keys == 0) {
      CK(hipMemsetAsync(d_slot_out, 0xFF, n * 4, st));
      if (!stream) {
        CK(hipEventRecord(d->kidx_found, st));
        d->kidx_found_used = true;
      }
      return GV_OK;
    }
    CK(kidx_find(d->kidx, ctx->keys, (const uint8_t*)d_pub33, n, (uint32_t*)d_slot_out, nullptr, st));
    ctx->kidx_stat.launches++;
    if (!stream) {
      CK(hipEventRecord(d->kidx_found, st));
      d->kidx_found_used = true;
    }
    return GV_OK;
  });
}

int gv_verify_digests_keyed(gv_ctx* ctx, size_t n, const uint32_t* slot, const uint8_t* sig64,
                            const uint8_t* dig32, uint8_t* out_ok) {
  if (n && (!slot || !dig32)) return GV_EINVAL;
  return run_host(ctx, n, HostBatch{nullptr, sig64, dig32, nullptr, nullptr, nullptr, slot, out_ok, nullptr});
}

int gv_verify_msgs_keyed(gv_ctx* ctx, size_t n, const uint32_t* slot, const uint8_t* sig64,
                         const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len,
                         uint8_t* out_ok) {
  if (n && !slot) return GV_EINVAL;
  return run_host(ctx, n, HostBatch{nullptr, sig64, nullptr, msg_blob, msg_off, msg_len, slot, out_ok, nullptr});
}

int gv_dev_verify_digests_keyed(gv_ctx* ctx, int dev_slot, size_t n, const void* d_slot, const void* d_sig64,
                                const void* d_dig32, void* d_bits, void* stream) {
  Dev* d = nullptr;
  int rc = dev_common(ctx, dev_slot, n, d_slot, d_sig64, d_bits, &d);
  if (rc || n == 0) return rc;
  if (!d_dig32 || ((uintptr_t)d_dig32 & 3)) return GV_EINVAL;
  std::lock_guard<std::mutex> lk(d->mu);
  CK(hipSetDevice(d->id));
  Items it;
  it.n = n; it.kslot = (const uint32_t*)d_slot; it.sig64 = (const uint8_t*)d_sig64; it.dig32 = (const uint8_t*)d_dig32;
  return dev_launch(ctx, d, stream, it, d_bits);
}

namespace {
// gv_get_option's rows of a pubkey index, by the name behind "keys_index_" /
// "ed_keys_index_".  Of the context: batches routed keyed, batches that fell
// through on a miss, k_kidx_* launches so far (false: not one of the three).
bool kidx_stat_option(const KeyIndexStats& st, const char* name, long long* val) {
  const std::atomic<uint64_t>* c = !strcmp(name, "hit") ? &st.hit : !strcmp(name, "miss") ? &st.miss
                                   : !strcmp(name, "launches") ? &st.launches : nullptr;
  if (c) *val = (long long)c->load();
  return c != nullptr;
}
// Of the first device, under the arena's locks: whether the index covers the
// arena (`live`), the slots in it, the keys its probe bound left out, its table
// words -- 0 each without a table or after a stop.
const char* const kKidxDevOptions[] = {"live", "keys", "left_out", "words"};
long long kidx_dev_option(const KeyIndex& ix, bool live, const char* name) {
  if (!strcmp(name, "live")) return live;
  if (!ix.tab || ix.failed) return 0;
  return (long long)(!strcmp(name, "keys") ? ix.keys : !strcmp(name, "left_out") ? ix.left_out : ix.T);
}
}  // namespace

int gv_get_option(gv_ctx* ctx, const char* key, long long* val) {
  if (!ctx || !key || !val) return GV_EINVAL;
  if (const gvopt::Row* r = gvopt::opt_find(key)) {   // the tunables (gv_options.h)
    if (!r->readable) return GV_EINVAL;
    *val = gvopt::opt_read(ctx->opt, *r);
    return GV_OK;
  }
  // read-only live values: an index's, under the same names for both arenas
  const bool edi = !strncmp(key, "ed_keys_index_", 14);
  const char* const iname = edi ? key + 14 : !strncmp(key, "keys_index_", 11) ? key + 11 : nullptr;
  if (iname && kidx_stat_option(edi ? ctx->ed_kidx_stat : ctx->kidx_stat, iname, val)) return GV_OK;
  const struct {
    const char* k;
    long long v;
  } live[] = {{"keys_replaced", (long long)ctx->keys_replaced.load()},   // gv_keys_replace's slots so far
              {"ed_keys_replaced", (long long)ctx->ed_keys_replaced.load()},   // the same for gv_ed_keys_replace
              {"ed_keyed_wide", (long long)ctx->ed_keyed_wide.load()},   // keyed batches / chunks on wide tables
              // routed batches whose non-resident items were split off ("keys_index_split"), and those items
              {"keys_index_split_calls", (long long)ctx->kidx_split_calls.load()},
              {"keys_index_split_items", (long long)ctx->kidx_split_items.load()},
              {"group_reuse_hit", (long long)ctx->grp_hit.load()},       // grouped keys whose tables were at hand
              {"group_reuse_built", (long long)ctx->grp_built.load()},   // ... and built, by calls with group_reuse on
              {"group_reuse_reset", (long long)ctx->grp_reset.load()},   // caches flushed (full, or another schedule's)
              {"group_reuse_launches", (long long)ctx->grp_launches.load()},   // k_group_* launches so far
              {"group_promoted", (long long)ctx->grp_promoted.load()},   // sets moved to the "group_promote" layout
              {"group_demoted", (long long)ctx->grp_demoted.load()},     // ... and back to k4's
              {"keys_index_find_ns", (long long)ctx->kidx_find_ns.load()},     // the last routed lookup's kernel
                                                                               // ("time_kernels" on)
              {"kw_qw", GV_KW_QW},                   // the wide arena's window width (build)
              {"kwn_qw", GV_KWN ? GV_KWN_QW : 0}};   // its narrow width (build; 0: not compiled)
  for (const auto& o : live)
    if (!strcmp(key, o.k)) {
      *val = o.v;
      return GV_OK;
    }
  // the first device's wide arena as gv_keys_load left it -- its window width
  // (0: no slot has wide tables) and its groups; its pubkey indexes
  // (kidx_dev_option); its wide ed25519 arena as gv_ed_keys_load left it -- its
  // radix bits (0: no slot has wide tables) and the slots that have them;
  // whether it holds a built radix-2^16 comb table of B ("ed_btab16_live":
  // 0 also when the build failed and k_ed_keyed adds [s]B from the radix-256
  // table; reading it never builds the table)
  const bool idx = iname && std::any_of(std::begin(kKidxDevOptions), std::end(kKidxDevOptions),
                                        [&](const char* k) { return !strcmp(iname, k); });
  const bool ed = !strcmp(key, "ed_kw_rb") || !strcmp(key, "ed_kw_keys") || edi;
  static const char* const kDev[] = {"kw_arena_qw", "kw_arena_ng", "group_reuse_rows", "group_layout",
                                     "hbm_optional_bytes", "ed_btab16_live"};
  if (edi && !idx) return GV_EINVAL;
  if (!ed && !idx && std::none_of(std::begin(kDev), std::end(kDev), [&](const char* k) { return !strcmp(key, k); }))
    return GV_EINVAL;
  if (ctx->devs.empty()) return GV_EINVAL;
  std::unique_lock<std::mutex> kl;
  if (ed) kl = std::unique_lock<std::mutex>(ctx->ed_keys_mu);
  Dev* d = ctx->devs[0];
  std::lock_guard<std::mutex> lk(d->mu);
  const bool kw = d->kw.qt && d->keysw, ekw = d->ektabw && d->ekeysw;
  // (the row capacity of the first scratch set's grouping arena; 0: none yet)
  *val = idx                                   ? kidx_dev_option(edi ? d->ed_kidx : d->kidx,
                                                                 edi ? ed_kidx_live(ctx, d) : kidx_live(ctx, d), iname)
         : !strcmp(key, "group_reuse_rows")    ? (long long)d->set[0].gk.cap
         // groups per key of the device's last grouped call (4: k4's and k6's layouts; 0: none yet); the
         // bytes of optional tables the HBM budget counts on the device
         : !strcmp(key, "group_layout")        ? (long long)d->group_layout
         : !strcmp(key, "hbm_optional_bytes")  ? (long long)d->opt_bytes
         : !strcmp(key, "ed_btab16_live")      ? (long long)(d->edtab16 ? 1 : 0)
         : !strcmp(key, "kw_arena_qw")         ? (kw ? d->kw.lay.qw() : 0)
         : !strcmp(key, "kw_arena_ng")         ? (kw ? (int)d->kw.lay.ng : 0)
         : !strcmp(key, "ed_kw_rb")            ? (ekw ? d->ekw_rb : 0)
                                               : (long long)(ekw ? d->ekeysw : 0);
  return GV_OK;
}

// Every device lock, taken in device order (returned held); drain: the
// pipelined ladders of every device have finished and the next pipelined call
// waits for no earlier bitmap, so no call launches on a mix of old and new
// option state.
static int quiesce_all(gv_ctx* ctx, bool drain, std::vector<std::unique_lock<std::mutex>>* held) {
  for (Dev* d : ctx->devs) held->emplace_back(d->mu);
  if (!drain) return GV_OK;
  for (Dev* d : ctx->devs) {
    CK(hipSetDevice(d->id));
    for (hipStream_t t : d->hi_st) CK(hipStreamSynchronize(t));
    d->bits_used = false;
  }
  return GV_OK;
}

int gv_set_option(gv_ctx* ctx, const char* key, long long val) {
  if (!ctx || !key) return GV_EINVAL;
  const gvopt::Row* r = gvopt::opt_find(key);
  if (!r || !gvopt::opt_check(*r, val)) return GV_EINVAL;
  // the row's effect, held until the value is stored
  std::vector<std::unique_lock<std::mutex>> held;
  std::unique_lock<std::mutex> kl;
  switch (r->fx) {
    case gvopt::FX_NONE: break;
    case gvopt::FX_QUIESCE:
    case gvopt::FX_POOLS:                         // (no drain: no device stages while its pool is replaced)
      if (int rc = quiesce_all(ctx, r->fx == gvopt::FX_QUIESCE, &held)) return rc;
      break;
    case gvopt::FX_ED_KEYS_MU: kl = std::unique_lock<std::mutex>(ctx->ed_keys_mu); break;
    case gvopt::FX_KEYS_EMPTY:
      kl = std::unique_lock<std::mutex>(ctx->keys_mu);
      if (ctx->keys != 0) return GV_EINVAL;
      break;
    case gvopt::FX_ED_KEYS_EMPTY:
      kl = std::unique_lock<std::mutex>(ctx->ed_keys_mu);
      if (ctx->ed_keys != 0) return GV_EINVAL;
      break;
  }
  // a quiescing option may pick the grouped route's table layout, and a fault
  // injected mid-call leaves a set's rows unknown: every set's key-table cache
  // starts cold (group_keys)
  const bool faults = !strcmp(key, "fault_inject");
  if (faults && quiesce_all(ctx, false, &held)) return GV_EHIP;
  if (r->fx == gvopt::FX_QUIESCE || faults)
    for (Dev* d : ctx->devs)
      for (Set* s : {&d->set[0], &d->set[1], &d->gset[0], &d->gset[1]}) {
        s->g_live = false;
        if (!faults) s->g_promo_refused = false;  // a refused promotion may be tried again
        // the options that choose the grouped schedule also end a set's promotion and its
        // history (any other leaves them: they describe the key stream, not the tables)
        if (!faults && (r->f.i == &gvopt::Options::kg || r->f.b == &gvopt::Options::k6 ||
                        r->f.b == &gvopt::Options::gfull || r->f.b == &gvopt::Options::group_reuse ||
                        r->f.i == &gvopt::Options::group_promote)) {
          s->g_promoted = false;
          s->g_hist = 0;
        }
      }
  gvopt::opt_store(ctx->opt, *r, val);
  if (r->fx == gvopt::FX_POOLS)
    for (Dev* d : ctx->devs) {
      delete d->pool;
      d->pool = new Pool((int)val - 1);
    }
  return GV_OK;
}

// [unpack/sha, s^-1, prep, ladder] ms of one launch (ladder: its own start to end)
static int stage_ms(hipEvent_t* e, float ms[4]) {
  CK(hipEventSynchronize(e[5]));
  for (int i = 0; i < 3; ++i) CK(hipEventElapsedTime(&ms[i], e[i], e[i + 1]));
  CK(hipEventElapsedTime(&ms[3], e[4], e[5]));
  return GV_OK;
}

int gv_last_stage_ms(gv_ctx* ctx, int dev_slot, float* unpack_ms, float* prep_ms, float* ecmult_ms) {
  if (!ctx || dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return GV_EINVAL;
  if (!ctx->opt.time_kernels) return GV_EINVAL;
  Dev* d = ctx->devs[dev_slot];
  if (d->last < 0) return GV_EINVAL;
  CK(hipSetDevice(d->id));
  float ms[4];
  int rc = stage_ms(d->ring[d->last], ms);
  if (rc) return rc;
  if (unpack_ms) *unpack_ms = ms[0];
  if (prep_ms) *prep_ms = ms[1] + ms[2];
  if (ecmult_ms) *ecmult_ms = ms[3];
  return GV_OK;
}

int gv_stage_stats4(gv_ctx* ctx, int dev_slot, int* count, double ms_out[4]) {
  if (!ctx || dev_slot < 0 || dev_slot >= (int)ctx->devs.size() || !ms_out) return GV_EINVAL;
  Dev* d = ctx->devs[dev_slot];
  std::lock_guard<std::mutex> lk(d->mu);
  CK(hipSetDevice(d->id));
  double sum[4] = {0, 0, 0, 0};
  const int cnt = d->ring_count;
  for (int k = 0; k < cnt; ++k) {
    float ms[4];
    int rc = stage_ms(d->ring[(d->ring_next - 1 - k + Dev::kRing) % Dev::kRing], ms);
    if (rc) return rc;
    for (int i = 0; i < 4; ++i) sum[i] += ms[i];
  }
  d->ring_count = 0;
  if (count) *count = cnt;
  for (int i = 0; i < 4; ++i) ms_out[i] = cnt ? sum[i] / cnt : 0.0;
  return GV_OK;
}

int gv_stage_stats(gv_ctx* ctx, int dev_slot, int* count, double* unpack_ms, double* prep_ms,
                   double* ecmult_ms) {
  double ms[4];
  int rc = gv_stage_stats4(ctx, dev_slot, count, ms);
  if (rc) return rc;
  if (unpack_ms) *unpack_ms = ms[0];
  if (prep_ms) *prep_ms = ms[1] + ms[2];
  if (ecmult_ms) *ecmult_ms = ms[3];
  return GV_OK;
}

int gv_dev_alloc(gv_ctx* ctx, int dev_slot, size_t bytes, void** d_ptr) {
  if (!ctx || !d_ptr || dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return GV_EINVAL;
  *d_ptr = nullptr;
  CK(hipSetDevice(ctx->devs[dev_slot]->id));
  if (hipMalloc(d_ptr, std::max<size_t>(bytes, 1)) != hipSuccess) return GV_ENOMEM;
  return GV_OK;
}

int gv_dev_free(gv_ctx* ctx, int dev_slot, void* d_ptr) {
  if (!ctx || dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return GV_EINVAL;
  CK(hipSetDevice(ctx->devs[dev_slot]->id));
  if (d_ptr) CK(hipFree(d_ptr));
  return GV_OK;
}

int gv_dev_copy(gv_ctx* ctx, int dev_slot, void* dst, const void* src, size_t bytes, int kind) {
  if (!ctx || dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return GV_EINVAL;
  if (bytes == 0) return GV_OK;
  if (!dst || !src) return GV_EINVAL;
  hipMemcpyKind k;
  switch (kind) {
    case 1: k = hipMemcpyHostToDevice; break;
    case 2: k = hipMemcpyDeviceToHost; break;
    case 3: k = hipMemcpyDeviceToDevice; break;
    default: return GV_EINVAL;
  }
  Dev* d = ctx->devs[dev_slot];
  CK(hipSetDevice(d->id));
  for (hipStream_t t : {d->lo_st[0], d->lo_st[1], d->hi_st[0], d->hi_st[1]})   // after every pipelined call (synchronous copy)
    CK(hipStreamSynchronize(t));
  hipStream_t st = d->set[0].st;
  CK(hipMemcpyAsync(dst, src, bytes, k, st));
  CK(hipStreamSynchronize(st));
  return GV_OK;
}

int gv_dev_stream_create(gv_ctx* ctx, int dev_slot, void** stream_out) {
  if (!ctx || !stream_out || dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return GV_EINVAL;
  *stream_out = nullptr;
  CK(hipSetDevice(ctx->devs[dev_slot]->id));
  hipStream_t st = nullptr;
  CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  *stream_out = (void*)st;
  return GV_OK;
}

int gv_dev_stream_sync(gv_ctx* ctx, int dev_slot, void* stream) {
  if (!ctx || !stream || dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return GV_EINVAL;
  CK(hipSetDevice(ctx->devs[dev_slot]->id));
  CK(hipStreamSynchronize((hipStream_t)stream));
  return GV_OK;
}

int gv_dev_stream_destroy(gv_ctx* ctx, int dev_slot, void* stream) {
  if (!ctx || !stream || dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return GV_EINVAL;
  CK(hipSetDevice(ctx->devs[dev_slot]->id));
  CK(hipStreamDestroy((hipStream_t)stream));
  return GV_OK;
}

int gv_dev_sync(gv_ctx* ctx, int dev_slot) {
  if (!ctx || dev_slot < 0 || dev_slot >= (int)ctx->devs.size()) return GV_EINVAL;
  Dev* d = ctx->devs[dev_slot];
  CK(hipSetDevice(d->id));
  for (Set& s : d->set) CK(hipStreamSynchronize(s.st));
  for (hipStream_t t : {d->lo_st[0], d->lo_st[1], d->hi_st[0], d->hi_st[1]}) CK(hipStreamSynchronize(t));
  return GV_OK;
}

const char* gv_strerror(int code) {
  switch (code) {
    case GV_OK: return "ok";
    case GV_EINVAL: return "invalid argument";
    case GV_ENODEV: return "no usable HIP device";
    case GV_EHIP: return "HIP runtime error";
    case GV_ENOMEM: return "out of memory";
    case GV_EFAULT: return "injected fault";
    default: return "unknown error";
  }
}

#if GV_STAMP
// Diagnostic builds only (not in gpuverify.h): the k_ecmult wave stamps of
// the last launches on dev_slot (tools/ecmult_stamps.py).
int gv_diag_stamps(gv_ctx* ctx, int dev_slot, uint64_t* out, size_t n_u64) {
  if (!ctx || dev_slot < 0 || dev_slot >= (int)ctx->devs.size() || !out) return GV_EINVAL;
  Dev* d = ctx->devs[dev_slot];
  std::lock_guard<std::mutex> lk(d->mu);
  CK(hipSetDevice(d->id));
  CK(hipDeviceSynchronize());
  CK(gvk_stamps_read(out, n_u64));
  return GV_OK;
}
#endif

int gv_debug_op(gv_ctx* ctx, int dev_slot, int op, size_t n, const uint32_t* in, uint32_t* out) {
  if (!ctx || dev_slot < 0 || dev_slot >= (int)ctx->devs.size() || !in || !out) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (n > kMaxItems) return GV_EINVAL;
  Dev* d = ctx->devs[dev_slot];
  std::lock_guard<std::mutex> lk(d->mu);
  CK(hipSetDevice(d->id));
  hipStream_t st = d->set[0].st;
  const size_t npad = round_up(n, 256);
  uint32_t *din = nullptr, *dout = nullptr;
  CK(hipMalloc(&din, npad * 64));
  if (hipMalloc(&dout, npad * 64) != hipSuccess) { (void)hipFree(din); return GV_ENOMEM; }
  int rc = GV_OK;
  if (hipMemsetAsync(din, 0, npad * 64, st) != hipSuccess ||
      hipMemcpyAsync(din, in, n * 64, hipMemcpyHostToDevice, st) != hipSuccess ||
      gvk_debug(op, (uint32_t)n, din, dout, st) != hipSuccess ||
      hipMemcpyAsync(out, dout, n * 64, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    rc = GV_EHIP;
  (void)hipFree(din);
  (void)hipFree(dout);
  return rc;
}

int gv_debug_sl_op(gv_ctx* ctx, int dev_slot, int op, size_t n, const uint32_t* in, uint32_t* out) {
  if (!ctx || dev_slot < 0 || dev_slot >= (int)ctx->devs.size() || !in || !out) return GV_EINVAL;
  const bool secp = op >= 0 && op < GV_SLOP_SECP_END, ed = op >= GV_SLOP_ED_MUL && op < GV_SLOP_ED_END;
  if (!secp && !ed) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (n > kMaxItems) return GV_EINVAL;
  Dev* d = ctx->devs[dev_slot];
  std::lock_guard<std::mutex> lk(d->mu);
  CK(hipSetDevice(d->id));
  hipStream_t st = d->set[0].st;
  const size_t bin = n * GV_SL_IN * 4, bout = n * GV_SL_OUT * 4;
  uint32_t *din = nullptr, *dout = nullptr;
  CK(hipMalloc(&din, bin));
  if (hipMalloc(&dout, bout) != hipSuccess) { (void)hipFree(din); return GV_ENOMEM; }
  int rc = GV_OK;
  if (hipMemcpyAsync(din, in, bin, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(dout, 0, bout, st) != hipSuccess ||
      (secp ? gvk_debug_sl : gvk_debug_esl)(op, (uint32_t)n, din, dout, st) != hipSuccess ||
      hipMemcpyAsync(out, dout, bout, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    rc = GV_EHIP;
  (void)hipFree(din);
  (void)hipFree(dout);
  return rc;
}

int gv_debug_lane_op(gv_ctx* ctx, int dev_slot, int op, size_t n, const uint32_t* in, uint32_t* out) {
  if (!ctx || dev_slot < 0 || dev_slot >= (int)ctx->devs.size() || !in || !out) return GV_EINVAL;
  const bool secp = op >= 0 && op < GV_LNOP_SECP_END;                                  // gv_kernels.hip: one chain
  const bool lat = op >= GV_LNOP_LAT && op < GV_LNOP_LAT + GV_LNOP_SECP_END;           // gv_lat.hip: two chains
  const bool ed = op >= GV_LNOP_ED_MUL && op < GV_LNOP_ED_END;
  if (!secp && !lat && !ed) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (n > kMaxItems) return GV_EINVAL;
  Dev* d = ctx->devs[dev_slot];
  std::lock_guard<std::mutex> lk(d->mu);
  CK(hipSetDevice(d->id));
  hipStream_t st = d->set[0].st;
  const size_t bin = n * GV_LN_IN * 4, bout = n * GV_LN_OUT * 4;
  uint32_t *din = nullptr, *dout = nullptr, *atab = nullptr;
  CK(hipMalloc(&din, bin));
  if (hipMalloc(&dout, bout) != hipSuccess) { (void)hipFree(din); return GV_ENOMEM; }
  if (op == GV_LNOP_GE_ADD_TAB && hipMalloc(&atab, n * GV_LN_ATAB_WORDS * 4) != hipSuccess) {
    (void)hipFree(din);
    (void)hipFree(dout);
    return GV_ENOMEM;
  }
  int rc = GV_OK;
  if (hipMemcpyAsync(din, in, bin, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(dout, 0, bout, st) != hipSuccess ||
      (secp  ? gvk_debug_lane(op, (uint32_t)n, din, dout, st)
       : lat ? gvk_debug_lane_lat(op - GV_LNOP_LAT, (uint32_t)n, din, dout, st)
             : gvk_debug_elane(op, (uint32_t)n, din, dout, atab, st)) != hipSuccess ||
      hipMemcpyAsync(out, dout, bout, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    rc = GV_EHIP;
  (void)hipFree(din);
  (void)hipFree(dout);
  if (atab) (void)hipFree(atab);
  return rc;
}

}  // extern "C"
