// gv_kidx.hip -- kernels of the resident key arenas' pubkey index (options
// "keys_index" and "ed_keys_index": one put and one find kernel, templates over
// the row length; gv_kidx.h holds the row loader, the hash, the probe sequence,
// insert and lookup), of a routed batch's split into resident and non-resident items
// (option "keys_index_split"), and of the grouped route's per-set key-table
// cache over the same routines (option "group_reuse").  All are one lane per
// key or item, memory-bound and tiny beside a table build or a ladder.
#include <hip/hip_runtime.h>
#include "gv_kernels.h"
#include "gv_kidx.h"

namespace gv {
typedef uint32_t u32;

// One atomicAdd per wave of the lanes with `hit` set (as k_dedupe_assign).
__device__ inline void wave_count(bool hit, u32* counter) {
  const uint64_t m = __ballot(hit);
  if (m == 0 || !counter) return;                      // wave-uniform
  if ((threadIdx.x & 63u) == (u32)__builtin_ctzll(m)) atomicAdd(counter, (u32)__builtin_popcountll(m));
}

// Key g of a load or replace chunk (device pub33, stride 33) -> the raw key
// row of its slot: base + g, or slots[g] (bounded and distinct, by the caller).
__global__ __launch_bounds__(256) void k_kidx_rows(const uint8_t* pub33, u32 n, u32 base, const u32* slots,
                                                    u32* rows) {
  const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  u32 row[GV_KIDX_ROW];
  gv_kidx_row_n<GV_KIDX_ROW>(pub33 + (size_t)g * 33u, row);
  u32* out = rows + (size_t)(slots ? slots[g] : base + g) * GV_KIDX_ROW;
#pragma unroll
  for (int i = 0; i < GV_KIDX_ROW; ++i) out[i] = row[i];
}

// Slot base + g (or slots[g]) of an arena of R-word rows enters the table.
// The rows were written by an earlier launch (k_kidx_rows, k_group_put; the
// ed25519 arena's table builds); the lanes share table words only (atomicCAS /
// atomicMin, gv_kidx.h).
template <int R>
__global__ __launch_bounds__(256) void k_kidx_put(u32* table, u32 tmask, const u32* rows, u32 n, u32 base,
                                                   const u32* slots, uint64_t seed, u32* left_out) {
  const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
  bool out = false;
  if (g < n) out = !gv_kidx_put_n<R>(table, tmask, rows, slots ? slots[g] : base + g, seed);
  wave_count(out, left_out);
}

// Item g's key bytes (KB of them, by the row length; the caller's AoS, any alignment) -> slot_out[g]: the
// lowest slot below `count` holding exactly those bytes, or GV_KIDX_EMPTY.
// miss (may be null) counts the items not found.
template <int R>
__global__ __launch_bounds__(256) void k_kidx_find(const u32* table, u32 tmask, const u32* rows, u32 count,
                                                    uint64_t seed, const uint8_t* keys, u32 n, u32* slot_out,
                                                    u32* miss) {
  constexpr int KB = gv_kidx_key<R>::bytes;
  const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
  u32 slot = 0;
  if (g < n) {
    u32 row[R];
    const uint8_t* p = keys + (size_t)g * KB;
    if (KB % 4 == 0 && ((uintptr_t)keys & 3u) == 0) {   // kernel-uniform: a pub32 batch as whole words
#pragma unroll
      for (int i = 0; i < R; ++i) row[i] = ((const u32*)p)[i];
    } else {
      gv_kidx_row_n<R>(p, row);
    }
    slot = gv_kidx_find_n<R>(table, tmask, rows, count, row, seed);
    slot_out[g] = slot;
  }
  wave_count(g < n && slot == GV_KIDX_EMPTY, miss);
}

// ---- a routed batch with a few keys that are not resident (option
// "keys_index_split").
//
// k_kidx_split: one lane per item of the batch.  An item whose looked-up slot
// is GV_KIDX_EMPTY takes the next row j of the dense sub-batch (one atomicAdd
// per wave on *count, as k_group_find; the order of rows across waves is
// unspecified): idx[j] = the item, its 33 key bytes (the caller's AoS,
// unaligned), its 64 signature bytes and its digest (dig32) or its message's
// offset and length (dig32 null; the blob is shared) into row j of the
// sub-batch's arrays.  A row at or past cap is never written (the host
// launches only when the misses fit).  sig64 / dig32 are 4-byte aligned (the
// device calls check); a 16-byte aligned sig64 is copied as 16-byte vectors.
__global__ __launch_bounds__(256) void k_kidx_split(const u32* slot, u32 n, const uint8_t* pub33, const uint8_t* sig64,
                                                     const uint8_t* dig32, const uint64_t* off, const u32* len,
                                                     u32 cap, u32* count, u32* idx, uint8_t* mpub, uint8_t* msig,
                                                     uint8_t* mdig, uint64_t* moff, u32* mlen) {
  const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
  const bool missed = g < n && slot[g] == GV_KIDX_EMPTY;
  const uint64_t m = __ballot(missed);
  if (m == 0) return;                                    // wave-uniform
  const u32 lane = threadIdx.x & 63u, leader = (u32)__builtin_ctzll(m);
  u32 b0 = 0;
  if (lane == leader) b0 = atomicAdd(count, (u32)__builtin_popcountll(m));
  b0 = (u32)__shfl((int)b0, (int)leader);
  if (!missed) return;
  const u32 j = b0 + (u32)__builtin_popcountll(m & ((1ull << lane) - 1ull));
  if (j >= cap) return;
  idx[j] = g;
  const uint8_t* p = pub33 + (size_t)g * 33u;
  uint8_t* q = mpub + (size_t)j * 33u;
#pragma unroll
  for (int i = 0; i < 33; ++i) q[i] = p[i];
  if (((uintptr_t)sig64 & 15u) == 0) {                   // kernel-uniform
    const uint4* s = (const uint4*)(sig64 + (size_t)g * 64u);
    uint4* t = (uint4*)(msig + (size_t)j * 64u);
    const uint4 a = s[0], b = s[1], c = s[2], d = s[3];
    t[0] = a; t[1] = b; t[2] = c; t[3] = d;
  } else {
    const u32* s = (const u32*)(sig64 + (size_t)g * 64u);
    u32* t = (u32*)(msig + (size_t)j * 64u);
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = s[i];
  }
  if (dig32) {
    const u32* s = (const u32*)(dig32 + (size_t)g * 32u);
    u32* t = (u32*)(mdig + (size_t)j * 32u);
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = s[i];
  } else {
    moff[j] = off[g];
    mlen[j] = len[g];
  }
}

// k_bits_merge: one lane per sub-batch row j < m.  An accepted row (bit j of
// sub) sets bit idx[j] of the batch's bitmap -- an atomic OR: two rows may
// share a word.
__global__ __launch_bounds__(256) void k_bits_merge(const uint64_t* sub, const u32* idx, u32 m, u32 n,
                                                     unsigned long long* bits) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m || !((sub[j >> 6] >> (j & 63u)) & 1ull)) return;
  const u32 i = idx[j];
  if (i < n) atomicOr(bits + (i >> 6), 1ull << (i & 63u));
}

// ---- the grouped route's per-set key-table cache (option "group_reuse";
// DESIGN section 4.1k): the same rows, table and routines over the set's
// per-batch arena, whose row r holds the tables of the key in rows[r].
//
// k_group_find: one lane per distinct key u of the batch (kx / kpfx of stride
// CU as k_dedupe_assign left them; *ucount keys, the lanes past it and past
// capU do nothing).  A key whose 9 words are in the cache's first `count` rows
// gets row[u] = that row; every other key takes the next miss number m (one
// atomic per wave, as k_dedupe_assign): miss[m] = u, row[u] = count + m, the
// row its tables are built into when the host appends (count + m may lie past
// the arena: the host then flushes and reads neither list).
__global__ __launch_bounds__(256) void k_group_find(const u32* table, u32 tmask, const u32* rows, u32 count,
                                                     uint64_t seed, const u32* kx, const u32* kpfx, u32 CU,
                                                     const u32* ucount, u32 capU, u32* row, u32* miss, u32* mcount) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 U = min(*ucount, capU);
  const bool live = u < U;
  u32 r = 0;
  if (live) {
    u32 key[GV_KIDX_ROW];
    key[0] = kpfx[u];
#pragma unroll
    for (int i = 0; i < 8; ++i) key[1 + i] = kx[(size_t)i * CU + u];
    r = gv_kidx_find_n<GV_KIDX_ROW>(table, tmask, rows, count, key, seed);
  }
  const bool missed = live && r == GV_KIDX_EMPTY;
  const uint64_t m = __ballot(missed);
  if (m != 0) {                                          // wave-uniform
    const u32 lane = threadIdx.x & 63u, leader = (u32)__builtin_ctzll(m);
    u32 b0 = 0;
    if (lane == leader) b0 = atomicAdd(mcount, (u32)__builtin_popcountll(m));
    b0 = (u32)__shfl((int)b0, (int)leader);
    if (missed) {
      const u32 mi = b0 + (u32)__builtin_popcountll(m & ((1ull << lane) - 1ull));
      miss[mi] = u;
      r = count + mi;
    }
  }
  if (live) row[u] = r;
}

// k_group_put: new key m (batch key list[m], or m itself with a null list) ->
// cache row base + m, and, with mx, key column m of the build's input rows mx
// / mpfx (stride CU): the missed keys gathered dense.  The rows enter the table
// in a launch of their own (k_kidx_put reads other lanes' rows).
__global__ __launch_bounds__(256) void k_group_put(const u32* kx, const u32* kpfx, u32 CU, const u32* list, u32 n,
                                                    u32 base, u32* rows, u32* mx, u32* mpfx) {
  const u32 m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  const u32 u = list ? list[m] : m;
  u32* out = rows + (size_t)(base + m) * GV_KIDX_ROW;
  const u32 pre = kpfx[u];
  out[0] = pre;
  if (mx) mpfx[m] = pre;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const u32 w = kx[(size_t)i * CU + u];
    out[1 + i] = w;
    if (mx) mx[(size_t)i * CU + m] = w;
  }
}

// k_dedupe_map through the cache: item g's slot is the cache row of its key
// (null row: the key's id, the row a flushed cache builds it into).
__global__ __launch_bounds__(256) void k_group_map(u32 n, const u32* rep, const u32* uid, const u32* row, u32* kslot) {
  const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const u32 r = rep[g];
  kslot[g] = r == 0xFFFFFFFFu ? 0xFFFFFFFFu : row ? row[uid[r]] : uid[r];
}
}  // namespace gv

extern "C" {
hipError_t gvk_kidx_rows(const uint8_t* pub33, uint32_t n, uint32_t base, const uint32_t* slots, uint32_t* rows,
                         hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(gv::k_kidx_rows, dim3((n + 255) / 256), dim3(256), 0, st, pub33, n, base, slots, rows);
  return hipGetLastError();
}

// row_words picks the instantiation: GV_KIDX_ROW or GV_KIDX_ROW_ED, nothing else.
hipError_t gvk_kidx_put(uint32_t row_words, uint32_t* table, uint32_t tslots, const uint32_t* rows, uint32_t n,
                        uint32_t base, const uint32_t* slots, uint64_t seed, uint32_t* left_out, hipStream_t st) {
  if (row_words != GV_KIDX_ROW && row_words != GV_KIDX_ROW_ED) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (tslots == 0 || (tslots & (tslots - 1))) return hipErrorInvalidValue;
  const auto k = row_words == GV_KIDX_ROW ? gv::k_kidx_put<GV_KIDX_ROW> : gv::k_kidx_put<GV_KIDX_ROW_ED>;
  hipLaunchKernelGGL(k, dim3((n + 255) / 256), dim3(256), 0, st, table, tslots - 1, rows, n, base, slots, seed,
                     left_out);
  return hipGetLastError();
}

hipError_t gvk_kidx_find(uint32_t row_words, const uint32_t* table, uint32_t tslots, const uint32_t* rows,
                         uint32_t count, uint64_t seed, const uint8_t* keys, uint32_t n, uint32_t* slot_out,
                         uint32_t* miss, hipStream_t st) {
  if (row_words != GV_KIDX_ROW && row_words != GV_KIDX_ROW_ED) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (tslots == 0 || (tslots & (tslots - 1))) return hipErrorInvalidValue;
  const auto k = row_words == GV_KIDX_ROW ? gv::k_kidx_find<GV_KIDX_ROW> : gv::k_kidx_find<GV_KIDX_ROW_ED>;
  hipLaunchKernelGGL(k, dim3((n + 255) / 256), dim3(256), 0, st, table, tslots - 1, rows, count, seed, keys, n,
                     slot_out, miss);
  return hipGetLastError();
}

hipError_t gvk_kidx_split(const gvk_split* s,const uint32_t* slot, uint32_t n, const uint8_t* pub33,
                          const uint8_t* sig64, const uint8_t* dig32, const uint64_t* off, const uint32_t* len,
                          hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (!s->cap || (!dig32 && (!off || !len))) return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(s->count, 0, 4, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gv::k_kidx_split, dim3((n + 255) / 256), dim3(256), 0, st, slot, n, pub33, sig64, dig32, off, len,
                     s->cap, s->count, s->idx, s->pub33, s->sig64, s->dig32, s->off, s->len);
  return hipGetLastError();
}

hipError_t gvk_bits_merge(const gvk_split* s, uint32_t m, uint32_t n, uint64_t* bits, hipStream_t st) {
  if (m == 0) return hipSuccess;
  if (m > s->cap) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gv::k_bits_merge, dim3((m + 255) / 256), dim3(256), 0, st, (const uint64_t*)s->bits,
                     (const uint32_t*)s->idx, m, n, (unsigned long long*)bits);
  return hipGetLastError();
}

hipError_t gvk_group_find(const uint32_t* table, uint32_t tslots, const uint32_t* rows, uint32_t count, uint64_t seed,
                          const uint32_t* kx, const uint32_t* kpfx, uint32_t CU, const uint32_t* ucount, uint32_t capU,
                          uint32_t* row, uint32_t* miss, uint32_t* mcount, hipStream_t st) {
  if (tslots == 0 || (tslots & (tslots - 1)) || capU == 0 || capU % 256 || capU > CU) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gv::k_group_find, dim3(capU / 256), dim3(256), 0, st, table, tslots - 1, rows, count, seed, kx,
                     kpfx, CU, ucount, capU, row, miss, mcount);
  return hipGetLastError();
}

hipError_t gvk_group_put(uint32_t* table, uint32_t tslots, uint32_t* rows, uint64_t seed, const uint32_t* kx,
                         const uint32_t* kpfx, uint32_t CU, const uint32_t* list, uint32_t n, uint32_t base,
                         uint32_t* mx, uint32_t* mpfx, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (tslots == 0 || (tslots & (tslots - 1)) || n > CU) return hipErrorInvalidValue;
  const dim3 blk(256), grd((n + 255) / 256);
  hipLaunchKernelGGL(gv::k_group_put, grd, blk, 0, st, kx, kpfx, CU, list, n, base, rows, mx, mpfx);
  hipLaunchKernelGGL(gv::k_kidx_put<GV_KIDX_ROW>, grd, blk, 0, st, table, tslots - 1, (const uint32_t*)rows, n, base,
                     (const uint32_t*)nullptr, seed, (uint32_t*)nullptr);
  return hipGetLastError();
}

hipError_t gvk_group_map(uint32_t n, const uint32_t* rep, const uint32_t* uid, const uint32_t* row, uint32_t* kslot,
                         hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(gv::k_group_map, dim3((n + 255) / 256), dim3(256), 0, st, n, rep, uid, row, kslot);
  return hipGetLastError();
}
}
