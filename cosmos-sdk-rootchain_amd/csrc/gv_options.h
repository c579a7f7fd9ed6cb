// gv_options.h -- the runtime's tunables, once: the Options struct (every
// field gv_set_option, gv_get_option or a GV_* environment variable touches,
// with the measurements behind its default) and ONE table with a row per
// option name: what gv_set_option accepts, how the value is stored, what the
// runtime must do before the store becomes visible, whether gv_get_option
// reads the key, and the environment variable with its own rule.  Host-only
// (no HIP), so the CPU tests drive the same table (tests/options), as
// gv_kidx.h, gv_stage.h and gv_async.h.
//
// The setter's and the environment's rules differ in places (async_growth
// rejects 65 as an option and clamps it as GV_ASYNC_GROWTH; GV_KEYS_INDEX is
// on for exactly "1", every other flag for anything but "0";
// GV_LAT_ROWS_MAX has no bound).  The table states them as they are.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gpuverify.h"

namespace gvopt {

constexpr size_t kMaxItems = 0xFFFFFF00ull;       // per launch (u32 lane indices)

// Build facts two accept rules need (gv_kernels.h: the kg layouts GV_KG_NGS
// or 0, the wide arena's window widths), defined by the including file.
static bool kg_layout_ok(int ng);
static bool kw_width_ok(int qw);

struct Options {
  size_t max_batch = size_t(1) << 20;
  size_t lat_max = 8192;        // batches up to this size take a fused small-batch kernel (gv_lat.hip), larger ones the pipeline
  size_t lat_sl_max = 2048;     // ... and up to this size the limb-sliced one (one signature per block); between the two the
                                // four-lanes-per-signature kernel (0.50 ms flat to 8192): profiles/r02/lat_sliced/batch_curve*.json
  // keyed batches (the key arena): the sliced keyed kernel takes 4 waves per
  // signature and the 16-lanes-per-signature kernel beats the k4 pipeline to
  // ~14k (profiles/r02/lat_sliced/keyed_curve.json).  Setting lat_max /
  // lat_sl_max sets these too; lat_max_keyed / lat_sl_max_keyed only these.
  size_t lat_max_keyed = 14336;
  size_t lat_sl_max_keyed = 1536;
  size_t pipe_chunk = 262144;   // host path: first chunk of the two-set copy/compute pipeline (0 = max_batch;
                                // profiles/r03/hostpath_sweep.jsonl: 262144 x 4 steadiest on pageable input)
  int pipe_growth = 4;          // host path: each later chunk at most this times the one before
  int stage_pieces = 2;         // host path, pageable chunks of >= 65,536 items: staged in this many pieces, each
                                // piece's H2D behind its copy (1 = one copy then one H2D; GV_STAGE_PIECES):
                                // 121.4 / 129.4 / 126.2 / 126.8M/s at 1 / 2 / 4 / 8 (profiles/r04/hostpath/stage_pieces_ab.jsonl)
  size_t async_chunk = 262144;  // submitted batches staged through the library (pageable, messages): fixed chunks
  int async_growth = 1;         // of this size growing by async_growth (GV_ASYNC_CHUNK, GV_ASYNC_GROWTH;
                                // "async_chunk" / "async_growth"): the copy of one chunk overlaps the others
  bool async_whole = true;      // submitted batches read in place (the caller's pinned buffers): a slice behind
                                // one still in flight is ONE chunk (its H2D and front run under the previous
                                // ladder), a slice on an idle device takes the synchronous ramp (GV_ASYNC_WHOLE,
                                // "async_whole").  1M pinned batches: 4.6 ms each steady vs 5.2 ms in 262,144-item
                                // chunks (a 262,144-item ladder is 1,024 blocks = 1.33 rounds of the chip's 768
                                // resident ones, and the next one only starts as it drains); pageable batches in
                                // one chunk lose the copy overlap (143 vs 177M/s): profiles/r06/async/
  bool host_ladder_stream = false;  // host chunks' ladders on the set's low-priority ladder stream (chunk_ladder;
                                    // GV_HOST_LADDER_STREAM=1).  Measured off: async pinned 185 vs 157-167M/s,
                                    // sync pinned 158-160 vs 150-152M/s (profiles/r05/async_ab.jsonl)
  size_t lane_burst = 16;       // submitted batches: slices an async lane runs before it drains and releases the
                                // device lock (GV_LANE_BURST)
  bool lat_kw = true;           // keyed small batches on the wide arena's one-window tables (k_verify_lat16_kw)
                                // when every slot has them, else the kn tables (GV_LAT_KW, "lat_kw")
  bool h2d_serial = true;       // host slices: a chunk's H2D waits for the previous chunk's, so concurrent
                                // transfers do not share the link and delay the chunk the GPU needs first
                                // (GV_H2D_SERIAL)
  bool gfull_item = true;       // the per-item (pub33, ungrouped) route takes G on the unsplit u1 too: 11 G
                                // additions from the full-scalar tables instead of 14 (GV_GFULL_ITEM)
  bool inv_small = true;        // k_scalar_inv folds fewer signatures per lane below 2^19 items (gvk_inv_m);
                                // 0: GV_INV_M always (GV_INV_SMALL)
  size_t slice_plain_first = 0; // host path, slices to be grouped: this many items first on the per-item pipeline,
                                // submitted before the rest's keys are sent, grouped and tabulated (0 = off;
                                // GV_SLICE_PLAIN_FIRST)
  int stage_threads = 8;        // host path: staging threads per device, its slice's thread included (gv_open:
                                // gvstage::stage_pool_threads -- half the process's CPUs, affinity capped by
                                // the cgroup quota, split over the devices, 1..8 each)
  bool time_kernels = false;
  bool fault_inject = false;
  bool lat_zero_copy = true;    // host-buffer batches on the sliced kernels read the pinned staging buffer and write
                                // verdict bytes to pinned memory directly: no H2D, memset or D2H (GV_LAT_ZC=0: A/B)
  bool lat_sliced = true;       // small batches on k_verify_lat_sl / k_verify_lat16_sl (GV_LAT_SLICED=0: the one-lane-field kernels, A/B)
  size_t lat_rows_max = 512;     // pub33 small batches of at most this many: k_verify_lat_sl4 (rows of a wave on one accumulator, G from gtab6); 0: k_verify_lat_sl
  bool keyed_k4 = true;         // keyed batches on k_ecmult_k4 (GV_KEYED_K4=0: the 125-doubling ladder, A/B)
  bool gfull = true;            // k4 batches take G on the unsplit scalar: 11 25-bit windows instead of 14 20-bit
                                // GLV windows (k_ecmult_k4<true>, 6 GiB of tables; GV_GFULL=0: A/B)
  bool k6 = false;              // grouped batches on k_ecmult_k6: 6-bit Q windows on 32-entry key tables, the lambda
                                // frame, G on the unsplit u1 in 24-bit windows (GV_K6=1)
  int kg = 0;                   // grouped batches on k_ecmult_kn<5, kg>: k4's 16-entry 5-bit tables over kg groups
                                // (one of GV_KG_NGS; 0 = k_ecmult_k4), G after the last doubling from the 24-bit
                                // tables on the real curve (GV_KG, "kg"; takes precedence over k6).  Off: with
                                // the unsplit key chain k4 stays ahead -- 223 vs 215-218M/s for kg 4 (its
                                // ladder 2-3 % shorter, but at 126 VGPRs x 4 waves the next call's front kernels
                                // no longer co-reside), 7 / 9 groups cut the ladder 10-17 % and cost more in the
                                // front (217 / 210M/s; profiles/r06/ab/ab3, ab4)
  int keys_wide = 2;            // ... and wide-window tables while device memory holds them (GV_KEYS_WIDE): 2 = one
                                // GV_KW_QW-bit window per group (11: 12 groups of 1,024 entries, no doublings, 24 Q
                                // additions), moving to two per group (6 groups, 11 doublings) when that no longer fits,
                                // then to the GV_KWN_QW-bit layouts (keys_wide_qw); 1 = two per group; 0 = none
  size_t keys_wide1_cap = SIZE_MAX;   // test hook: the one-window layout's slot capacity ("keys_wide1_cap")
  int keys_wide_qw = 0;         // the wide arena's window width ("keys_wide_qw", GV_KEYS_WIDE_QW): 0 = the GV_KW_QW-bit
                                // layouts, then the GV_KWN_QW-bit ones when those no longer fit (kWideLayouts);
                                // GV_KW_QW / GV_KWN_QW = that width's two layouts only
  size_t keys_wide_bytes = 0;   // the wide arena is never allocated larger than this ("keys_wide_mb", GV_KEYS_WIDE_MB;
                                // 0 = no limit): past it the arena moves down the layouts, then to the k6 tables
  bool keys_k6 = true;          // the resident arena (gv_keys_load) also holds k6 tables and its throughput batches
                                // run k_ecmult_k6: the table build is paid once per key, not per batch (GV_KEYS_K6)
  size_t key_cap = GV_KEY_CAP;  // the callers' key-arena reset point: growth doubles up to here ("key_cap", GV_KEY_CAP)
  size_t ed_key_cap = GV_ED_KEY_CAP;   // the same for the ed25519 arena ("ed_key_cap", GV_ED_KEY_CAP)
  size_t hbm_budget = SIZE_MAX; // bytes of optional device tables per device (G tables, key arenas; "hbm_budget_mb",
                                // GV_HBM_BUDGET_MB): a table past it is not built and batches take the schedule
                                // that needs less, with the same verdicts
  bool pipeline_dev = true;     // pipelined device-resident calls on the context stream (dev_run; GV_PIPELINE=0: A/B)
  bool two_ladders = true;      // ... whose ladders alternate two high-priority streams, so the next ladder starts in
                                // the current one's tail (bitmap writes kept in call order; GV_TWO_LADDERS=0: A/B)
  bool group_keys = true;       // pub33 throughput batches parse each distinct key once (group_keys; GV_GROUP_KEYS=0: A/B)
  bool group_reuse = true;      // ... and a set keeps the tables of the keys it has built: a later batch on the set
                                // builds only the keys it has not seen (the set's arena as a cache, filled then
                                // flushed; "group_reuse", GV_GROUP_REUSE=0: every call rebuilds)
  int group_promote = 9;        // ... and a set whose keys recur moves its tables to the kg layout of this many groups
                                // (6, 7, 9; 0 = never: k4's layout): after two warm calls and on a third, each
                                // building fewer keys per item than half the break-even, the set rebuilds its keys
                                // once in the kg layout and its calls run k_ecmult_kn<5, NG> -- 10 doublings
                                // instead of 30 at 9 groups; it goes back when a call misses more keys than the
                                // break-even ("group_promote", GV_GROUP_PROMOTE).  Inert when
                                // "kg" or "k6" names a layout
  size_t group_promote_min = 262144;   // ... on a batch of at least this many items (one full residency of the ladder:
                                       // 256 CUs x 4 SIMDs x 4 waves x 64 lanes; "group_promote_min")
  bool keys_scratch = true;     // key tables: forward entries through coalesced scratch rows (GV_KEYS_SCRATCH=0: A/B)
  bool sort_keys = true;        // keyed k4 batches run their lanes in slot order (gv_sort.hip; GV_SORT_KEYS=0: A/B)
  size_t group_min = 16384;     // ... batches of at least this many items
  int group_div = 5;            // ... taking the keyed pipeline when distinct keys <= items / group_div (break-even ~4:
                                // a key build ~18 ns vs ~4 ns saved per item, profiles/r03/group_ab)
  bool keys_index = false;      // gv_keys_load also keeps a device index of the arena, 33 key bytes -> slot (gv_kidx.h),
                                // and gv_dev_verify_digests / _msgs route a throughput batch whose keys are all
                                // resident onto the keyed pipeline ("keys_index", GV_KEYS_INDEX): taken by an arena
                                // started from slot 0; 0 stops its use at once
  uint64_t kidx_seed = 0;       // the index hash's seed, drawn at gv_open ("keys_index_seed": a test hook)
  size_t keys_index_split = 0;  // ... and a routed batch with at most this many items whose keys are NOT resident still
                                // runs keyed: those items are compacted into a sub-batch for the pub33 routes, under
                                // the main ladder, and their accept bits merged in ("keys_index_split"; 0 = any miss
                                // sends the whole batch to the pub33 routes)
  bool ed_group = true;          // ed25519 throughput batches: in-batch key grouping + k_ed_keyed (GV_ED_GROUP=0: A/B)
  size_t ed_group_min = 196608;  // ... from this many items (the key build's chain is ~1 ms of one-lane chains whatever
                                 // the key count up to ~65k keys; the keyed kernel saves ~6.4 ns per item; host
                                 // chunks of 262,144 qualify)
  int ed_group_div = 16;         // ... with at most items / ed_group_div distinct keys
  size_t ed_group_cap = 16384;   // ... and at most this many (72 KB of comb table per key)
  bool ed_keys_split = true;     // ed25519 key tables: serial chain and table adds in two launches (GV_ED_KEYS_SPLIT=0: A/B)
  bool ed_btab16 = true;         // k_ed_keyed's [s]B from the radix-2^16 table: 16 additions instead of 32 (GV_ED_BTAB16)
  bool ed_group_r64 = true;      // grouped ed25519 key tables as radix-64 combs: 43 [h](-A) additions, not 64 (GV_ED_GROUP_R64)
  bool ed_keyed = true;          // keyed ed25519 batches past ed_lat_max on k_ed_keyed (GV_ED_KEYED=0: the throughput kernels)
  size_t ed_lat_max = 2048;      // keyed ed25519 batches up to this size take k_ed_lat_sl (one signature per block)
  int ed_keys_wide = 0;          // the ed25519 arena also holds radix-2^6 or radix-2^8 combs of -A for k_ed_keyed
                                 // (0 = none, 6, 8; "ed_keys_wide", GV_ED_KEYS_WIDE): taken by an arena started from
                                 // slot 0; 0 stops their use at once
  size_t ed_keys_wide_bytes = 0; // the wide ed25519 arena is never allocated larger than this ("ed_keys_wide_mb",
                                 // GV_ED_KEYS_WIDE_MB; 0 = no limit)
  bool ed_keys_index = false;    // gv_ed_keys_load also keeps a device index of the ed25519 arena, 32 key bytes -> slot
                                 // (gv_kidx.h at 8-word rows: the arena's own ekpub rows), and
                                 // gv_dev_verify_ed25519_msgs runs a batch whose keys are all resident as the keyed
                                 // call would ("ed_keys_index", GV_ED_KEYS_INDEX): taken by an
                                 // arena started from slot 0; 0 stops its use at once
  uint64_t ed_kidx_seed = 0;     // its hash seed, drawn at gv_open ("ed_keys_index_seed": a test hook)
  size_t ed_unc_lat_max = 2048;  // uncached ed25519 host batches up to this size take k_ed_lat_unc (one signature per block)
};

// What gv_set_option accepts (lo, hi: the rule's bounds).
enum Accept {
  A_BOOL,      // 0 or 1
  A_RANGE,     // [lo, hi]
  A_ZERO_OR,   // 0 or [256, kMaxItems]
  A_SET,       // a value below 64 whose bit is set in lo ({0, 6, 8})
  A_KG,        // kg_layout_ok((int)val)
  A_KW_WIDTH,  // 0 or a width within [0, 32] that kw_width_ok takes
  A_MIN0,      // >= 0
  A_ANY        // no check
};
// How a size_t member is stored (flags); a bool stores val != 0, an int (int)val.
enum Xform { X_ASIS = 0, X_ROUND256 = 1, X_SHL20 = 2, X_ZERO_MAX = 4 };
// What the runtime does between the check and the store.
enum Effect {
  FX_NONE,
  FX_QUIESCE,      // every device lock, drain the pipelined ladders: no call launches on a mix of old and new state
  FX_ED_KEYS_MU,   // hold ed_keys_mu
  FX_KEYS_EMPTY,   // hold keys_mu; rejected unless the resident arena is empty
  FX_POOLS,        // every device lock; replace the staging pools after the store
  FX_ED_KEYS_EMPTY // hold ed_keys_mu; rejected unless the ed25519 arena is empty
};
// How gv_open reads the row's environment variable.
enum EnvRule {
  E_NONE,
  E_NOT0,        // on unless "0"
  E_IS1,         // on for exactly "1"
  E_SETTER,      // parsed (an int member as atoi does, else atoll), checked and stored as the setter would; a reject is ignored
  E_CLAMP_1_64,  // atoi, clamped to [1, 64]
  E_MIN1,        // max(1, atoi)
  E_RAW_U,       // strtoull, unchecked
  E_SIZE         // atoll within [256, kMaxItems], rounded up to 256; else ignored
};

struct Field {
  bool Options::*b = nullptr;
  int Options::*i = nullptr;
  size_t Options::*z = nullptr;
  constexpr Field(bool Options::*p) : b(p) {}
  constexpr Field(int Options::*p) : i(p) {}
  constexpr Field(size_t Options::*p) : z(p) {}
};

struct Row {
  const char* name;          // the option key; null: the environment variable only
  Field f;                   // the member it writes
  Accept accept;
  long long lo, hi;
  int xform;
  Effect fx;
  bool readable;             // gv_get_option reads the key
  const char* env = nullptr;
  EnvRule env_rule = E_NONE;
  size_t Options::*also = nullptr;   // a coupled member written too (lat_max sets lat_max_keyed)
};

constexpr long long kMaxMb = (long long)(SIZE_MAX >> 20);
#define GVO(m) &Options::m
constexpr Row kRows[] = {
    // name, member, accept, lo, hi, stored, effect, readable[, environment, its rule[, coupled member]]
    {"lat_max", GVO(lat_max), A_RANGE, 0, kMaxItems, X_ASIS, FX_NONE, false, nullptr, E_NONE, GVO(lat_max_keyed)},
    {"lat_max_keyed", GVO(lat_max_keyed), A_RANGE, 0, kMaxItems, X_ASIS, FX_NONE, false},
    {"lat_sl_max", GVO(lat_sl_max), A_RANGE, 0, kMaxItems, X_ASIS, FX_NONE, false, nullptr, E_NONE,
     GVO(lat_sl_max_keyed)},
    {"lat_sl_max_keyed", GVO(lat_sl_max_keyed), A_RANGE, 0, kMaxItems, X_ASIS, FX_NONE, false},
    {"ed_unc_lat_max", GVO(ed_unc_lat_max), A_RANGE, 0, kMaxItems, X_ASIS, FX_NONE, false},
    {"ed_lat_max", GVO(ed_lat_max), A_RANGE, 0, kMaxItems, X_ASIS, FX_NONE, false},
    {"lat_zero_copy", GVO(lat_zero_copy), A_BOOL, 0, 1, X_ASIS, FX_NONE, false, "GV_LAT_ZC", E_NOT0},
    {"lat_sliced", GVO(lat_sliced), A_BOOL, 0, 1, X_ASIS, FX_NONE, false, "GV_LAT_SLICED", E_NOT0},
    {"lat_rows_max", GVO(lat_rows_max), A_RANGE, 0, kMaxItems, X_ASIS, FX_NONE, false, "GV_LAT_ROWS_MAX", E_RAW_U},
    {"max_batch", GVO(max_batch), A_RANGE, 256, kMaxItems, X_ROUND256, FX_NONE, true, "GV_MAX_BATCH", E_SIZE},
    {"pipe_chunk", GVO(pipe_chunk), A_ZERO_OR, 256, kMaxItems, X_ROUND256, FX_NONE, false},
    {"pipe_growth", GVO(pipe_growth), A_RANGE, 1, 64, X_ASIS, FX_NONE, false},
    {"stage_threads", GVO(stage_threads), A_RANGE, 1, 64, X_ASIS, FX_POOLS, false},
    {"stage_pieces", GVO(stage_pieces), A_RANGE, 1, 64, X_ASIS, FX_NONE, false, "GV_STAGE_PIECES", E_MIN1},
    {"h2d_serial", GVO(h2d_serial), A_BOOL, 0, 1, X_ASIS, FX_NONE, false, "GV_H2D_SERIAL", E_NOT0},
    {"gfull_item", GVO(gfull_item), A_BOOL, 0, 1, X_ASIS, FX_NONE, false, "GV_GFULL_ITEM", E_NOT0},
    {"inv_small", GVO(inv_small), A_BOOL, 0, 1, X_ASIS, FX_NONE, false, "GV_INV_SMALL", E_NOT0},
    {"slice_plain_first", GVO(slice_plain_first), A_RANGE, 0, kMaxItems, X_ASIS, FX_NONE, false,
     "GV_SLICE_PLAIN_FIRST", E_RAW_U},
    {"group_keys", GVO(group_keys), A_BOOL, 0, 1, X_ASIS, FX_NONE, true, "GV_GROUP_KEYS", E_NOT0},
    {"group_min", GVO(group_min), A_RANGE, 256, kMaxItems, X_ASIS, FX_NONE, false},
    {"group_div", GVO(group_div), A_RANGE, 2, 1024, X_ASIS, FX_NONE, false},
    {"ed_btab16", GVO(ed_btab16), A_BOOL, 0, 1, X_ASIS, FX_NONE, false, "GV_ED_BTAB16", E_NOT0},
    {"ed_group_r64", GVO(ed_group_r64), A_BOOL, 0, 1, X_ASIS, FX_NONE, false, "GV_ED_GROUP_R64", E_NOT0},
    {"ed_keys_split", GVO(ed_keys_split), A_BOOL, 0, 1, X_ASIS, FX_NONE, false, "GV_ED_KEYS_SPLIT", E_NOT0},
    {"ed_group", GVO(ed_group), A_BOOL, 0, 1, X_ASIS, FX_NONE, false, "GV_ED_GROUP", E_NOT0},
    {"ed_group_min", GVO(ed_group_min), A_RANGE, 256, kMaxItems, X_ASIS, FX_NONE, false},
    {"ed_keyed", GVO(ed_keyed), A_BOOL, 0, 1, X_ASIS, FX_NONE, false, "GV_ED_KEYED", E_NOT0},
    // the radix of an arena started from slot 0 from now on (a running arena
    // keeps its tables until gv_ed_keys_reset); 0 stops their use at once
    {"ed_keys_wide", GVO(ed_keys_wide), A_SET, 1 | 1 << 6 | 1 << 8, 0, X_ASIS, FX_ED_KEYS_MU, true,
     "GV_ED_KEYS_WIDE", E_SETTER},
    {"ed_keys_wide_mb", GVO(ed_keys_wide_bytes), A_RANGE, 0, kMaxMb, X_SHL20, FX_ED_KEYS_MU, true,
     "GV_ED_KEYS_WIDE_MB", E_SETTER},
    // the layout of an arena started from slot 0 from now on (a running arena
    // keeps its layout until gv_keys_reset); 0 stops its use at once
    {"keys_wide", GVO(keys_wide), A_RANGE, 0, 2, X_ASIS, FX_QUIESCE, true, "GV_KEYS_WIDE", E_SETTER},
    // taken by an arena started from slot 0 from now on (a running arena keeps
    // what it has until gv_keys_reset); 0 stops the use of the index at once
    {"keys_index", GVO(keys_index), A_BOOL, 0, 1, X_ASIS, FX_QUIESCE, true, "GV_KEYS_INDEX", E_IS1},
    // test hook: the index hash's seed, while no key is in the arena
    {"keys_index_seed", GVO(kidx_seed), A_ANY, 0, 0, X_ASIS, FX_KEYS_EMPTY, false},
    {"kg", GVO(kg), A_KG, 0, 0, X_ASIS, FX_QUIESCE, true, "GV_KG", E_SETTER},
    // the widths an arena started from slot 0 may take from now on
    {"keys_wide_qw", GVO(keys_wide_qw), A_KW_WIDTH, 0, 32, X_ASIS, FX_NONE, true, "GV_KEYS_WIDE_QW", E_SETTER},
    {"keys_wide_mb", GVO(keys_wide_bytes), A_RANGE, 0, kMaxMb, X_SHL20, FX_NONE, true, "GV_KEYS_WIDE_MB", E_SETTER},
    {"keys_wide1_cap", GVO(keys_wide1_cap), A_MIN0, 0, 0, X_ZERO_MAX, FX_NONE, false},
    // schedule switches
    {"two_ladders", GVO(two_ladders), A_BOOL, 0, 1, X_ASIS, FX_QUIESCE, true, "GV_TWO_LADDERS", E_NOT0},
    {"gfull", GVO(gfull), A_BOOL, 0, 1, X_ASIS, FX_QUIESCE, true, "GV_GFULL", E_NOT0},
    {"k6", GVO(k6), A_BOOL, 0, 1, X_ASIS, FX_QUIESCE, true, "GV_K6", E_NOT0},
    {"keys_k6", GVO(keys_k6), A_BOOL, 0, 1, X_ASIS, FX_QUIESCE, true, "GV_KEYS_K6", E_NOT0},
    {"async_chunk", GVO(async_chunk), A_RANGE, 256, kMaxItems, X_ROUND256, FX_NONE, true, "GV_ASYNC_CHUNK", E_SIZE},
    {"lat_kw", GVO(lat_kw), A_BOOL, 0, 1, X_ASIS, FX_NONE, true, "GV_LAT_KW", E_NOT0},
    {"async_whole", GVO(async_whole), A_BOOL, 0, 1, X_ASIS, FX_NONE, true, "GV_ASYNC_WHOLE", E_NOT0},
    {"async_growth", GVO(async_growth), A_RANGE, 1, 64, X_ASIS, FX_NONE, true, "GV_ASYNC_GROWTH", E_CLAMP_1_64},
    {"host_ladder_stream", GVO(host_ladder_stream), A_BOOL, 0, 1, X_ASIS, FX_NONE, false, "GV_HOST_LADDER_STREAM",
     E_NOT0},
    {"key_cap", GVO(key_cap), A_RANGE, 256, kMaxItems, X_ASIS, FX_NONE, true, "GV_KEY_CAP", E_SETTER},
    {"ed_key_cap", GVO(ed_key_cap), A_RANGE, 256, kMaxItems, X_ASIS, FX_NONE, false, "GV_ED_KEY_CAP", E_SETTER},
    // (0: no budget, the default gv_open starts from -- GV_HBM_BUDGET_MB=0 leaves it)
    {"hbm_budget_mb", GVO(hbm_budget), A_MIN0, 0, 0, X_SHL20 | X_ZERO_MAX, FX_NONE, false, "GV_HBM_BUDGET_MB",
     E_SETTER},
    {"sort_keys", GVO(sort_keys), A_BOOL, 0, 1, X_ASIS, FX_NONE, true, "GV_SORT_KEYS", E_NOT0},
    {"pipeline_dev", GVO(pipeline_dev), A_BOOL, 0, 1, X_ASIS, FX_NONE, true, "GV_PIPELINE", E_NOT0},
    {"time_kernels", GVO(time_kernels), A_ANY, 0, 0, X_ASIS, FX_NONE, false},
    {"fault_inject", GVO(fault_inject), A_ANY, 0, 0, X_ASIS, FX_NONE, false},
    // the environment only
    {nullptr, GVO(keyed_k4), A_BOOL, 0, 1, X_ASIS, FX_NONE, false, "GV_KEYED_K4", E_NOT0},
    {nullptr, GVO(keys_scratch), A_BOOL, 0, 1, X_ASIS, FX_NONE, false, "GV_KEYS_SCRATCH", E_NOT0},
    {nullptr, GVO(lane_burst), A_RANGE, 1, kMaxItems, X_ASIS, FX_NONE, false, "GV_LANE_BURST", E_MIN1},
};
// Rows added after the table was recorded: tests/golden/options_parent.json
// pins kRows' keys and variables one to one (tests/test_options_host.py), so a
// later option stands here.  Same columns, same rules: opt_find and
// opt_from_env read both.
constexpr Row kRowsLater[] = {
    {"group_reuse", GVO(group_reuse), A_BOOL, 0, 1, X_ASIS, FX_QUIESCE, true, "GV_GROUP_REUSE", E_NOT0},
    // 0 or one of the kg layouts above k4's four groups (gv_kernels.h GV_KG_NGS)
    {"group_promote", GVO(group_promote), A_SET, 1 | 1 << 6 | 1 << 7 | 1 << 9, 0, X_ASIS, FX_QUIESCE, true,
     "GV_GROUP_PROMOTE", E_SETTER},
    {"group_promote_min", GVO(group_promote_min), A_RANGE, 0, kMaxItems, X_ASIS, FX_NONE, true},
    // the most non-resident items of a routed batch that are still split off (0: none; no variable)
    {"keys_index_split", GVO(keys_index_split), A_RANGE, 0, kMaxItems, X_ASIS, FX_NONE, true},
    // taken by an ed25519 arena started from slot 0 from now on (a running arena
    // keeps what it has until gv_ed_keys_reset); 0 stops the use of the index at once
    {"ed_keys_index", GVO(ed_keys_index), A_BOOL, 0, 1, X_ASIS, FX_ED_KEYS_MU, true, "GV_ED_KEYS_INDEX", E_IS1},
    // test hook: that index hash's seed, while no key is in the ed25519 arena
    {"ed_keys_index_seed", GVO(ed_kidx_seed), A_ANY, 0, 0, X_ASIS, FX_ED_KEYS_EMPTY, false},
};
#undef GVO

static inline const Row* opt_find(const char* key) {
  for (const Row& r : kRows)
    if (r.name && !strcmp(key, r.name)) return &r;
  for (const Row& r : kRowsLater)
    if (r.name && !strcmp(key, r.name)) return &r;
  return nullptr;
}

// The setter's accept rule.
static inline bool opt_check(const Row& r, long long val) {
  switch (r.accept) {
    case A_BOOL: return val == 0 || val == 1;
    case A_RANGE: return val >= r.lo && val <= r.hi;
    case A_ZERO_OR: return val == 0 || (val >= r.lo && val <= r.hi);
    case A_SET: return val >= 0 && val < 64 && ((r.lo >> val) & 1);
    case A_KG: return kg_layout_ok((int)val);
    case A_KW_WIDTH: return val == 0 || (val >= r.lo && val <= r.hi && kw_width_ok((int)val));
    case A_MIN0: return val >= 0;
    case A_ANY: return true;
  }
  return false;
}

// Store an accepted value in the row's stored form.
static inline void opt_store(Options& o, const Row& r, long long val) {
  if (r.f.b) o.*r.f.b = val != 0;
  if (r.f.i) o.*r.f.i = (int)val;
  if (r.f.z) {
    size_t v = (size_t)val;
    if (r.xform & X_ROUND256) v = (v + 255) / 256 * 256;
    if (r.xform & X_SHL20) v <<= 20;
    if ((r.xform & X_ZERO_MAX) && val == 0) v = SIZE_MAX;
    o.*r.f.z = v;
    if (r.also) o.*r.also = v;
  }
}

// Check, then store.  Returns the effect the caller must apply before the
// store becomes visible to other threads (gv_set_option checks, applies the
// effect and stores in three steps; this form serves an Options nobody else
// sees yet) or -1: rejected, nothing stored.
static inline int opt_check_and_store(Options& o, const Row& r, long long val) {
  if (!opt_check(r, val)) return -1;
  opt_store(o, r, val);
  return r.fx;
}

// The value gv_get_option reports for a readable row.
static inline long long opt_read(const Options& o, const Row& r) {
  if (r.f.b) return o.*r.f.b;
  if (r.f.i) return o.*r.f.i;
  return (long long)((r.xform & X_SHL20) ? o.*r.f.z >> 20 : o.*r.f.z);
}

// Every row's environment variable into o, by the row's rule.  getenv_fn:
// getenv, or a test's stand-in.
template <class G>
static inline void opt_from_env(Options& o, G&& getenv_fn) {
  auto one = [&](const Row& r) {
    const char* s = r.env ? getenv_fn(r.env) : nullptr;
    if (!s) return;
    const int iv = atoi(s);
    switch (r.env_rule) {
      case E_NONE: break;
      case E_NOT0: o.*r.f.b = strcmp(s, "0") != 0; break;
      case E_IS1: o.*r.f.b = !strcmp(s, "1"); break;
      case E_SIZE:                                // (its rows' setter rule is the same [256, kMaxItems], rounded up)
      case E_SETTER: (void)opt_check_and_store(o, r, r.f.i ? (long long)iv : atoll(s)); break;
      case E_CLAMP_1_64: o.*r.f.i = iv < 1 ? 1 : iv > 64 ? 64 : iv; break;
      case E_MIN1: opt_store(o, r, iv < 1 ? 1 : iv); break;
      case E_RAW_U: o.*r.f.z = (size_t)strtoull(s, nullptr, 10); break;
    }
  };
  for (const Row& r : kRows) one(r);
  for (const Row& r : kRowsLater) one(r);
}

}  // namespace gvopt
