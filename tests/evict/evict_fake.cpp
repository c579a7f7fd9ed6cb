// evict_fake.cpp -- the CPU stand-in of tests/sanitize (fake_gpuverify.cpp,
// included as text) with gv_keys_replace over its key store, for the eviction
// harness (evict_harness.cpp).  Test infrastructure only.
#include "../sanitize/fake_gpuverify.cpp"

#include <set>

extern "C" {

int gv_keys_replace(gv_ctx* ctx, size_t n, const uint32_t* slots, const uint8_t* pub33) {
  if (!ctx) return GV_EINVAL;
  if (n == 0) return GV_OK;
  if (!slots || !pub33) return GV_EINVAL;
  quiesce(ctx);
  std::lock_guard<std::mutex> g(ctx->mu);
  const size_t cnt = ctx->keys.size() / 33;
  std::set<uint32_t> seen;
  for (size_t i = 0; i < n; ++i)
    if (slots[i] >= cnt || !seen.insert(slots[i]).second) return GV_EINVAL;
  for (size_t i = 0; i < n; ++i) memcpy(&ctx->keys[33 * (size_t)slots[i]], pub33 + 33 * i, 33);
  return GV_OK;
}

// the key the store holds for a slot (the harness' invariant checks)
int gvfake_key(gv_ctx* ctx, uint32_t slot, uint8_t out33[33]) {
  std::lock_guard<std::mutex> g(ctx->mu);
  if ((size_t)slot >= ctx->keys.size() / 33) return 0;
  memcpy(out33, &ctx->keys[33 * (size_t)slot], 33);
  return 1;
}

}  // extern "C"
