// evict_fake.cpp -- the CPU stand-in of tests/sanitize (fake_gpuverify.cpp,
// included as text) with gv_keys_replace and gv_ed_keys_replace over its key
// stores, for the eviction harnesses (evict_harness.cpp,
// evict_ed_harness.cpp).  Test infrastructure only.
#include "../sanitize/fake_gpuverify.cpp"

#include <set>

namespace {
// rows of K bytes: each slot loaded, none twice, then the keys into their slots
template <size_t K>
int replace_rows(std::vector<uint8_t>& store, size_t n, const uint32_t* slots, const uint8_t* pub) {
  const size_t cnt = store.size() / K;
  std::set<uint32_t> seen;
  for (size_t i = 0; i < n; ++i)
    if (slots[i] >= cnt || !seen.insert(slots[i]).second) return GV_EINVAL;
  for (size_t i = 0; i < n; ++i) memcpy(&store[K * (size_t)slots[i]], pub + K * i, K);
  return GV_OK;
}
// the key a store holds for a slot (the harness' invariant checks)
template <size_t K>
int row(const std::vector<uint8_t>& store, uint32_t slot, uint8_t* out) {
  if ((size_t)slot >= store.size() / K) return 0;
  memcpy(out, &store[K * (size_t)slot], K);
  return 1;
}
}  // namespace

extern "C" {

int gv_keys_replace(gv_ctx* ctx, size_t n, const uint32_t* slots, const uint8_t* pub33) {
  if (!ctx) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (!slots || !pub33) return GV_EINVAL;
  quiesce(ctx);
  std::lock_guard<std::mutex> g(ctx->mu);
  return replace_rows<33>(ctx->keys, n, slots, pub33);
}

int gv_ed_keys_replace(gv_ctx* ctx, size_t n, const uint32_t* slots, const uint8_t* pub32) {
  if (!ctx) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (!slots || !pub32) return GV_EINVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  return replace_rows<32>(ctx->ed_keys, n, slots, pub32);
}

int gvfake_key(gv_ctx* ctx, uint32_t slot, uint8_t out33[33]) {
  std::lock_guard<std::mutex> g(ctx->mu);
  return row<33>(ctx->keys, slot, out33);
}

int gvfake_ed_key(gv_ctx* ctx, uint32_t slot, uint8_t out32[32]) {
  std::lock_guard<std::mutex> g(ctx->mu);
  return row<32>(ctx->ed_keys, slot, out32);
}

}  // extern "C"
