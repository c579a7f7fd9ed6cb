// evict_ed_fake.cpp -- the CPU stand-in of tests/sanitize (fake_gpuverify.cpp,
// included as text) with gv_ed_keys_replace over its ed25519 byte store, for
// the ed25519 eviction harness (evict_ed_harness.cpp).  Test infrastructure
// only.
#include "../sanitize/fake_gpuverify.cpp"

#include <set>

extern "C" {

int gv_ed_keys_replace(gv_ctx* ctx, size_t n, const uint32_t* slots, const uint8_t* pub32) {
  if (!ctx) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (!slots || !pub32) return GV_EINVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  const size_t cnt = ctx->ed_keys.size() / 32;
  std::set<uint32_t> seen;
  for (size_t i = 0; i < n; ++i)
    if (slots[i] >= cnt || !seen.insert(slots[i]).second) return GV_EINVAL;
  for (size_t i = 0; i < n; ++i) memcpy(&ctx->ed_keys[32 * (size_t)slots[i]], pub32 + 32 * i, 32);
  return GV_OK;
}

// the key the store holds for an ed25519 slot (the harness' invariant checks)
int gvfake_ed_key(gv_ctx* ctx, uint32_t slot, uint8_t out32[32]) {
  std::lock_guard<std::mutex> g(ctx->mu);
  if ((size_t)slot >= ctx->ed_keys.size() / 32) return 0;
  memcpy(out32, &ctx->ed_keys[32 * (size_t)slot], 32);
  return 1;
}

}  // extern "C"
