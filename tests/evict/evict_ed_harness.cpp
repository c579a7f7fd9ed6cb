// evict_ed_harness.cpp -- the host mirror's clock eviction over the ed25519
// key arena (gvh_set_ed_key_resident) under ASan + UBSan or TSan
// (tests/test_ed_key_evict_host.py), over the CPU fake with
// gv_ed_keys_replace (evict_fake.cpp).  host/gvhost.cpp is compiled into
// this file so that the checks below can read the app's ed25519 key-slot
// bookkeeping.
//   1. SETS validator sets of VALS keys each (OpenSSL keys from fixed seeds)
//      sign commits; some commits carry a signature with a flipped bit, some
//      calls carry two commits.  THREADS threads drive gvh_verify_commits
//      (keys_trusted = 1) over the sets round-robin on one app with a resident
//      size of `resident`.  After every call: the arena never passes the
//      resident size, every slot's stored key is the key the clock's reverse
//      array names, the map sends that key to that slot and holds nothing else
//      (GVH_EVICT_AUDIT: admit_keys aborts if a slot named by the batch in
//      hand is among the victims).
//   2. The same calls, serially, on an app with resident 0: every result must
//      be equal, and the arena must have grown past the resident size.
// Prints {"codes": [...], "replaced": n, "resets": n, "count": n} and exits 0,
// or exits 1 with the first difference.
#define GVH_EVICT_AUDIT 1
#include "../../cosmos-sdk-rootchain_amd/host/gvhost.cpp"

#include <openssl/evp.h>
#include <stdio.h>

extern "C" gv_ctx* gvfake_open(void);
extern "C" void gvfake_close(gv_ctx*);
extern "C" int gvfake_ed_key(gv_ctx*, uint32_t slot, uint8_t out32[32]);

namespace {
constexpr int SETS = 12, VALS = 40, THREADS = 4, ROUNDS = 18;

int fail(const char* what) {
  fprintf(stderr, "evict_ed_harness: %s\n", what);
  return 1;
}

struct ValSet {
  std::vector<EVP_PKEY*> priv;
  std::vector<uint8_t> pub;          // VALS x 32
  std::vector<int64_t> power;
};

// One signed commit (VerifyCommit form: signature i <-> validator i).
struct Commit {
  std::vector<uint8_t> flag, sig, blob;
  std::vector<uint32_t> sig_len, msg_len;
  std::vector<uint64_t> msg_off;
  gvh_commit c{};
};

void sign_commit(Commit& k, const ValSet& vs, int set, int round, int bad) {
  k.flag.assign(VALS, GVH_COMMIT_FLAG_COMMIT);
  k.sig.assign(64 * VALS, 0);
  k.sig_len.assign(VALS, 64);
  for (int i = 0; i < VALS; ++i) {
    char msg[64];
    const int ml = snprintf(msg, sizeof msg, "vote set %d round %d validator %d", set, round, i);
    k.msg_off.push_back(k.blob.size());
    k.msg_len.push_back((uint32_t)ml);
    k.blob.insert(k.blob.end(), msg, msg + ml);
    EVP_MD_CTX* m = EVP_MD_CTX_new();
    size_t sl = 64;
    if (!m || EVP_DigestSignInit(m, nullptr, nullptr, nullptr, vs.priv[i]) != 1 ||
        EVP_DigestSign(m, &k.sig[64 * i], &sl, (const uint8_t*)msg, (size_t)ml) != 1 || sl != 64)
      abort();
    EVP_MD_CTX_free(m);
  }
  if (bad >= 0) k.sig[64 * bad + 5] ^= 0x10;
  k.c.trusting = 0;
  k.c.basic_ok = 1;
  k.c.n_vals = VALS;
  k.c.val_pub32 = vs.pub.data();
  k.c.val_power = vs.power.data();
  k.c.n_sigs = VALS;
  k.c.flag = k.flag.data();
  k.c.sig64 = k.sig.data();
  k.c.sig_len = k.sig_len.data();
  k.c.msg_blob = k.blob.data();
  k.c.msg_off = k.msg_off.data();
  k.c.msg_len = k.msg_len.data();
  k.c.keys_trusted = 1;
}

// The ed25519 bookkeeping of app against the fake's store; nullptr when consistent.
const char* audit(gvh_app* app, gv_ctx* ctx, size_t resident) {
  std::lock_guard<std::mutex> g(app->gpu_mu);
  const size_t count = gv_ed_keys_count(ctx);
  if (count > resident) return "arena past the resident size";
  const auto& clk = app->ed.clock;
  if (clk.key.size() != count) return "reverse array and arena differ in size";
  if (clk.ref.size() != count || clk.stamp.size() != count) return "clock arrays differ in size";
  if (app->ed.map.size() != count) return "map holds a key no slot holds";
  for (size_t s = 0; s < count; ++s) {
    uint8_t k[32];
    if (!gvfake_ed_key(ctx, (uint32_t)s, k)) return "slot not in the store";
    if (memcmp(k, clk.key[s].data(), 32)) return "reverse array names another key than the store holds";
    const uint32_t* v = app->ed.map.find(k);
    if (!v || *v != s) return "map does not send a slot's key to that slot";
  }
  return nullptr;
}

struct Res {
  int32_t code, idx;
  int64_t got;
  bool operator==(const Res& o) const { return code == o.code && idx == o.idx && got == o.got; }
};
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return fail("usage: evict_ed_harness resident");
  const size_t resident = (size_t)atol(argv[1]);
  std::vector<ValSet> sets(SETS);
  for (int s = 0; s < SETS; ++s)
    for (int v = 0; v < VALS; ++v) {
      uint8_t seed[32];
      for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(s * 41 + v * 7 + i * 3 + 1);
      seed[0] = (uint8_t)s;
      seed[1] = (uint8_t)v;
      EVP_PKEY* k = EVP_PKEY_new_raw_private_key(EVP_PKEY_ED25519, nullptr, seed, 32);
      uint8_t pub[32];
      size_t pl = 32;
      if (!k || EVP_PKEY_get_raw_public_key(k, pub, &pl) != 1 || pl != 32) return fail("OpenSSL ed25519 key");
      sets[s].priv.push_back(k);
      sets[s].pub.insert(sets[s].pub.end(), pub, pub + 32);
      sets[s].power.push_back(1);
    }
  // the calls of thread t: ROUNDS calls, set (3 t + 5 r) mod SETS, every third
  // call a second commit of the next set; every fourth commit has a bad signature
  struct Call { std::vector<Commit> cm; std::vector<gvh_commit> raw; };
  std::vector<std::vector<Call>> calls(THREADS);
  for (int t = 0; t < THREADS; ++t) {
    calls[t].resize(ROUNDS);
    for (int r = 0; r < ROUNDS; ++r) {
      Call& c = calls[t][r];
      const int nc = r % 3 == 2 ? 2 : 1;
      c.cm.resize(nc);
      for (int q = 0; q < nc; ++q) {
        const int set = (3 * t + 5 * r + q) % SETS;
        sign_commit(c.cm[q], sets[set], set, r * 8 + t, (r + t + q) % 4 == 0 ? (r * 7 + t) % VALS : -1);
      }
      for (auto& k : c.cm) c.raw.push_back(k.c);
    }
  }

  // 1. concurrent, eviction on
  gv_ctx* c1 = gvfake_open();
  gvh_app* a1 = gvh_app_new(c1);
  gvh_set_ed_key_resident(a1, resident);
  {
    size_t got = 0;
    gvh_get_ed_key_stats(a1, &got, nullptr, nullptr);
    if (got != resident) return fail("gvh_set_ed_key_resident did not take (gv_ed_keys_replace not linked?)");
  }
  std::vector<std::vector<Res>> got(THREADS);
  std::vector<const char*> err(THREADS, nullptr);
  std::vector<std::thread> th;
  for (int t = 0; t < THREADS; ++t)
    th.emplace_back([&, t]() {
      for (Call& c : calls[t]) {
        std::vector<gvh_commit_result> out(c.raw.size());
        if (gvh_verify_commits(a1, c.raw.size(), c.raw.data(), out.data()) != GVH_OK) {
          err[t] = "gvh_verify_commits";
          return;
        }
        for (auto& o : out) got[t].push_back(Res{o.code, o.idx, o.got});
        if (const char* e = audit(a1, c1, resident)) {
          err[t] = e;
          return;
        }
      }
    });
  for (auto& x : th) x.join();
  for (const char* e : err)
    if (e) return fail(e);
  uint64_t replaced = 0, resets = 0;
  gvh_get_ed_key_stats(a1, nullptr, &replaced, &resets);
  const size_t count = gv_ed_keys_count(c1);

  // 2. serial, eviction off
  gv_ctx* c2 = gvfake_open();
  gvh_app* a2 = gvh_app_new(c2);
  std::vector<std::vector<Res>> ref(THREADS);
  for (int t = 0; t < THREADS; ++t)
    for (Call& c : calls[t]) {
      std::vector<gvh_commit_result> out(c.raw.size());
      if (gvh_verify_commits(a2, c.raw.size(), c.raw.data(), out.data()) != GVH_OK)
        return fail("gvh_verify_commits (resident 0)");
      for (auto& o : out) ref[t].push_back(Res{o.code, o.idx, o.got});
    }
  if (gv_ed_keys_count(c2) != (size_t)SETS * VALS) return fail("resident 0: the arena does not hold every set");
  if (gv_ed_keys_count(c2) <= resident) return fail("the workload does not pass the resident size");
  {
    uint64_t rep0 = 1;
    gvh_get_ed_key_stats(a2, nullptr, &rep0, nullptr);
    if (rep0 != 0) return fail("resident 0 replaced slots");
  }
  if (!(got == ref)) return fail("results with eviction != resident 0");
  for (gvh_app* a : {a1, a2}) gvh_app_free(a);
  printf("{\"codes\": [");
  bool first = true;
  for (auto& v : ref)
    for (auto& r : v) {
      printf("%s%d", first ? "" : ", ", r.code);
      first = false;
    }
  printf("], \"replaced\": %llu, \"resets\": %llu, \"count\": %zu}\n", (unsigned long long)replaced,
         (unsigned long long)resets, count);
  for (gv_ctx* c : {c1, c2}) gvfake_close(c);
  for (auto& s : sets)
    for (EVP_PKEY* k : s.priv) EVP_PKEY_free(k);
  return 0;
}
