// gv_kidx.hip -- kernels of the resident key arena's pubkey index (option
// "keys_index"; gv_kidx.h holds the hash, the probe sequence, insert and
// lookup).  All three are one lane per key or item, memory-bound and tiny
// beside a table build or a ladder.
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
  gv_kidx_row(pub33 + (size_t)g * 33u, row);
  u32* out = rows + (size_t)(slots ? slots[g] : base + g) * GV_KIDX_ROW;
#pragma unroll
  for (int i = 0; i < GV_KIDX_ROW; ++i) out[i] = row[i];
}

// Slot base + g (or slots[g]) enters the table.  The rows were written by an
// earlier launch; the lanes share table words only.
__global__ __launch_bounds__(256) void k_kidx_put(u32* table, u32 tmask, const u32* rows, u32 n, u32 base,
                                                   const u32* slots, uint64_t seed, u32* left_out) {
  const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
  bool out = false;
  if (g < n) out = !gv_kidx_put(table, tmask, rows, slots ? slots[g] : base + g, seed);
  wave_count(out, left_out);
}

// Item g's 33 bytes (the caller's AoS pub33, unaligned) -> slot_out[g]: the
// lowest slot holding exactly those bytes, or GV_KIDX_EMPTY.  miss (may be
// null) counts the items not found.
__global__ __launch_bounds__(256) void k_kidx_find(const u32* table, u32 tmask, const u32* rows, u32 count,
                                                    uint64_t seed, const uint8_t* pub33, u32 n, u32* slot_out,
                                                    u32* miss) {
  const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
  u32 slot = 0;
  if (g < n) {
    u32 row[GV_KIDX_ROW];
    gv_kidx_row(pub33 + (size_t)g * 33u, row);
    slot = gv_kidx_find(table, tmask, rows, count, row, seed);
    slot_out[g] = slot;
  }
  wave_count(g < n && slot == GV_KIDX_EMPTY, miss);
}
}  // namespace gv

extern "C" {
hipError_t gvk_kidx_rows(const uint8_t* pub33, uint32_t n, uint32_t base, const uint32_t* slots, uint32_t* rows,
                         hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(gv::k_kidx_rows, dim3((n + 255) / 256), dim3(256), 0, st, pub33, n, base, slots, rows);
  return hipGetLastError();
}

hipError_t gvk_kidx_put(uint32_t* table, uint32_t tslots, const uint32_t* rows, uint32_t n, uint32_t base,
                        const uint32_t* slots, uint64_t seed, uint32_t* left_out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (tslots == 0 || (tslots & (tslots - 1))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gv::k_kidx_put, dim3((n + 255) / 256), dim3(256), 0, st, table, tslots - 1, rows, n, base, slots,
                     seed, left_out);
  return hipGetLastError();
}

hipError_t gvk_kidx_find(const uint32_t* table, uint32_t tslots, const uint32_t* rows, uint32_t count, uint64_t seed,
                         const uint8_t* pub33, uint32_t n, uint32_t* slot_out, uint32_t* miss, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (tslots == 0 || (tslots & (tslots - 1))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gv::k_kidx_find, dim3((n + 255) / 256), dim3(256), 0, st, table, tslots - 1, rows, count, seed,
                     pub33, n, slot_out, miss);
  return hipGetLastError();
}
}
