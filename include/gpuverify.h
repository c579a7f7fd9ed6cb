/*
 * gpuverify.h -- C ABI of libgpuverify.so, the MI355X (gfx950) batched
 * secp256k1 transaction-signature verifier.
 *
 * Drop-in boundary.  Every entry point below replaces, for a
 * whole batch at once, the reference's per-signature call
 *
 *     pubKey.VerifyBytes(signBytes, sig)            x/auth/ante/sigverify.go:210
 *
 * i.e. tendermint v0.33.4 crypto/secp256k1 PubKeySecp256k1.VerifyBytes
 * (secp256k1_nocgo.go), reached through SigVerificationDecorator.AnteHandle
 * (x/auth/ante/sigverify.go:170-216) and, for multisig leaves, through
 * multisig.PubKeyMultisigThreshold.VerifyBytes (the type switch at
 * x/auth/ante/sigverify.go:303-321 names both key types).  out_ok[i] is
 * exactly VerifyBytes(msg_i, sig_i) for pubkey pub33_i: 1 = true, 0 = false.
 * Cryptographic rejection is never an error code.
 *
 * Plain pointers and sizes only (cgo / ctypes / JNI friendly).  The caller owns
 * every buffer; the library copies inputs into its own device memory and keeps
 * no caller pointer after a call returns (the gv_submit_* calls excepted: they
 * keep theirs until gv_wait).  Host-buffer gv_verify_* calls are synchronous
 * and a gv_ctx may be shared by concurrent threads (calls on one device
 * serialise; every use of a device's scratch, on any stream, is ordered after
 * the previous one, so gv_dev_* calls on different caller streams never
 * overwrite each other's in-flight inputs).
 * INTEGRATION.md shows the Go (cgo) binding a maintainer adds as
 * crypto/gpuverify and the BatchSigVerificationDecorator built on it.
 */
#ifndef GPUVERIFY_H
#define GPUVERIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Return codes: 0 = OK, negative = infrastructure error.  On any nonzero
 * return the caller must not use out_ok and should re-verify on the CPU
 * (fail-closed; SURVEY.md §5 "Failure detection"). */
#define GV_OK        0
#define GV_EINVAL   -1   /* bad argument (null pointer, misaligned device ptr, ...) */
#define GV_ENODEV   -2   /* no usable HIP device / bad device id */
#define GV_EHIP     -3   /* HIP runtime or kernel error */
#define GV_ENOMEM   -4   /* device or host allocation failed */
#define GV_EFAULT   -5   /* injected fault (option "fault_inject") */

typedef struct gv_ctx gv_ctx;

/* Open a context on dev_ids[0..n_dev) (HIP ordinals); n_dev == 0 -> every
 * visible device.  Builds the per-device G table.  Replaces nothing in the
 * reference (which has no device state); the Go shim calls it once at app
 * construction (simapp/app.go:335-339 wiring site). */
int gv_open(const int* dev_ids, int n_dev, gv_ctx** out);
void gv_close(gv_ctx* ctx);
int gv_num_devices(const gv_ctx* ctx);

/* Batch VerifyBytes over messages.  Item i: pubkey pub33 + 33*i (SEC1
 * compressed, as stored by secp256k1.PubKeySecp256k1 [33]byte), signature
 * sig64 + 64*i (R||S big-endian, tendermint's 64-byte format), message
 * msg_blob[msg_off[i] .. msg_off[i] + msg_len[i]) (StdSignBytes,
 * x/auth/types/stdtx.go:248-259).  Signatures whose length is not 64 are
 * decided (false) by the caller before the call, exactly like VerifyBytes'
 * first check.  Replaces the loop body at x/auth/ante/sigverify.go:194-213. */
int gv_verify_msgs(gv_ctx* ctx, size_t n, const uint8_t* pub33, const uint8_t* sig64,
                   const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len,
                   uint8_t* out_ok);

/* Same with the messages already hashed: dig32 + 32*i = SHA256(msg_i)
 * (tendermint crypto.Sha256).  This is VerifyBytes minus its hashing step
 * (btcec Signature.Verify(hash, pub) preceded by the tendermint checks). */
int gv_verify_digests(gv_ctx* ctx, size_t n, const uint8_t* pub33, const uint8_t* sig64,
                      const uint8_t* dig32, uint8_t* out_ok);

/* Packed-bitmap variants: bit (i % 64) of out_bits[i / 64] is item i's
 * verdict; ceil(n/64) words are written (unused high bits 0). */
int gv_verify_digests_bits(gv_ctx* ctx, size_t n, const uint8_t* pub33, const uint8_t* sig64,
                           const uint8_t* dig32, uint64_t* out_bits);
int gv_verify_msgs_bits(gv_ctx* ctx, size_t n, const uint8_t* pub33, const uint8_t* sig64,
                        const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len,
                        uint64_t* out_bits);

/* Device-resident entry points for callers whose batch already lives in HBM
 * (benchmarks, a node that stages blocks on the GPU).  dev_slot indexes the
 * context's devices; d_* are device pointers on that device (4-byte aligned);
 * d_bits receives ceil(n/64) words; stream is a hipStream_t (NULL = the
 * context's stream).  Asynchronous: results are ready when the stream is. */
int gv_dev_verify_digests(gv_ctx* ctx, int dev_slot, size_t n, const void* d_pub33,
                          const void* d_sig64, const void* d_dig32, void* d_bits, void* stream);
int gv_dev_verify_msgs(gv_ctx* ctx, int dev_slot, size_t n, const void* d_pub33,
                       const void* d_sig64, const void* d_msg_blob, const void* d_msg_off,
                       const void* d_msg_len, void* d_bits, void* stream);

/* Device memory and stream helpers for callers of the gv_dev_* entry points
 * that have no HIP runtime of their own (bench.py, tests).  kind: 1 = host to
 * device, 2 = device to host, 3 = device to device; copies are ordered on the
 * context stream of dev_slot and synchronous. */
int gv_dev_alloc(gv_ctx* ctx, int dev_slot, size_t bytes, void** d_ptr);
int gv_dev_free(gv_ctx* ctx, int dev_slot, void* d_ptr);
int gv_dev_copy(gv_ctx* ctx, int dev_slot, void* dst, const void* src, size_t bytes, int kind);
int gv_dev_sync(gv_ctx* ctx, int dev_slot);
/* A non-blocking HIP stream on dev_slot for the gv_dev_* calls' `stream`
 * argument (callers without a HIP runtime of their own), its synchronisation
 * and destruction. */
int gv_dev_stream_create(gv_ctx* ctx, int dev_slot, void** stream_out);
int gv_dev_stream_sync(gv_ctx* ctx, int dev_slot, void* stream);
int gv_dev_stream_destroy(gv_ctx* ctx, int dev_slot, void* stream);

/* Account pubkey cache.  The reference amino-decodes and
 * btcec-parses an account's pubkey on every VerifyBytes
 * (x/auth/types/account.go:65-72 -> secp256k1_nocgo.go ParsePubKey), and a
 * node verifies the same accounts block after block.  gv_keys_load parses n
 * SEC1 keys once (prefix, x < p, square root) and keeps each key's table of
 * 16 multiples resident in HBM on every device of the context (1,280 B per
 * key, plus the tables of 2^35 Q, 2^70 Q, 2^100 Q for the small-batch keyed
 * kernels: 5.4 KB per key) and, with option "keys_k6" (default), the
 * throughput ladder's 11 tables of 32 multiples of 2^(12 k) Q on one Z (28 KB
 * per key: 1M accounts = 34 GB of the 288 GB); slot_out[i] receives key i's
 * slot.
 * A key that ParsePubKey rejects gets a slot too, and every verify against it
 * is false.  Slots are assigned in load order and name their key until
 * gv_keys_reset, or until gv_keys_replace puts another key into them.
 * Loading must not race keyed verifies of the same context. */
int gv_keys_load(gv_ctx* ctx, size_t n, const uint8_t* pub33, uint32_t* slot_out);
int gv_keys_reset(gv_ctx* ctx);
size_t gv_keys_count(const gv_ctx* ctx);
/* Replacement: after GV_OK slot slots[i] behaves in every respect -- every
 * keyed entry point on every schedule, the gv_submit_*_keyed lanes,
 * gv_keys_point -- as if pub33 + 33*i had been loaded into it (a key
 * ParsePubKey rejects gives a false slot; a key equal to one resident in
 * another slot is fine, the two slots are independent).  Every table set the
 * slot already has is rebuilt on every device of the context: the k4 tables,
 * the k6 tables, the wide tables in the arena's current layout.  Nothing is
 * allocated, grown or moved: gv_keys_count, gv_keys_generation and the
 * arena's layout ("kw_arena_qw" / "kw_arena_ng") do not change, so a caller
 * that replaces a slot keeps its own pubkey -> slot map right (drop the old
 * key's entry; the generation does not tell).  Like gv_keys_load it waits
 * for every submitted batch first: a batch submitted before the call runs
 * against the old keys.
 * GV_EINVAL, and nothing changed, when a slot is >= gv_keys_count() or
 * appears twice (ctx, slots or pub33 NULL with n > 0 too); n == 0 is GV_OK.
 * On GV_EHIP no slot named in the call is trusted: the caller must
 * gv_keys_reset.  Option "keys_replaced" (read-only) counts the slots
 * replaced since gv_open. */
int gv_keys_replace(gv_ctx* ctx, size_t n, const uint32_t* slots, const uint8_t* pub33);
/* Number of gv_keys_reset calls on ctx so far: a caller that keeps a
 * pubkey -> slot map drops it when the generation moved (slots of an older
 * generation may name other keys). */
uint64_t gv_keys_generation(const gv_ctx* ctx);

/* Routing policy shared by the callers above this ABI (the Go shim
 * go/crypto/gpuverify reads these through cgo; the C++ mirror host/gvhost.cpp
 * uses them as its defaults), so the two cannot drift apart:
 *   GV_CPU_CROSSOVER  batches smaller than this go to the reference CPU
 *                     VerifyBytes (one host core answers a
 *                     single signature in ~0.20 ms, the sliced small-batch
 *                     kernels ~0.21 ms at any size up to 256);
 *   GV_KEY_LOAD_MIN   only batches of at least this many leaves (a block)
 *                     load keys that are not resident yet; a smaller batch
 *                     (CheckTx) goes keyed only when all its keys are
 *                     resident, else pub33 (loading per
 *                     CheckTx window cost 35.8k -> 5.1k tx/s);
 *   GV_KEY_CAP        arena size at which the caller resets the arena
 *                     (5.4 KB of HBM per key), unless it keeps the arena
 *                     at a resident size below this by replacing slots
 *                     (gv_keys_replace; gvh_set_key_resident, the shim's
 *                     KeyResident). */
#define GV_CPU_CROSSOVER 4
#define GV_KEY_LOAD_MIN 4096
#define GV_KEY_CAP (1u << 22)
/* ... and the ed25519 key arena's (gv_ed_keys_load: 72 KB of HBM per key),
 * unless the caller keeps it at a resident size below this by replacing
 * slots (gv_ed_keys_replace; gvh_set_ed_key_resident, the shim's
 * EdKeyResident). */
#define GV_ED_KEY_CAP (1u << 16)

/* Key-arena readback (tests, tools): for each slot, the affine point the
 * arena holds for it, out_xy64 + 64*i = x || y (32 bytes each, big-endian),
 * and out_ok[i] = its ParsePubKey verdict (a slot >= gv_keys_count(): zeros
 * and 0).  Reads the first device's arena. */
int gv_keys_point(gv_ctx* ctx, size_t n, const uint32_t* slots, uint8_t* out_xy64, uint8_t* out_ok);
/* Key-table readback (tests, tools): every entry of every table set of the
 * resident arena of device dev_slot.  tabs picks the set: 0 the k4 / keyed
 * latency tables (5-bit windows: 4 groups of 16 entries, every loaded slot),
 * 1 the kn tables ("keys_k6": 6-bit windows, 11 groups of 32 entries), 2 the
 * wide tables in the arena's layout ("kw_arena_qw" = QW 11 or 9 bits,
 * "kw_arena_ng" groups of 2^(QW-1) entries).  Item i names slot slots[i],
 * group groups[i] < NG and entry js[i] in 1..NT = 2^(QW-1); out_xy64 + 64*i
 * = x || y (32 bytes each, big-endian) of the affine point the table holds
 * there, which is js[i] * 2^(QW * w0(groups[i])) * Q for the slot's key Q
 * -- group k starts at window w0(k) = k P - max(0, k - R), P = ceil(QWIN /
 * NG), R = QWIN - (P - 1) NG, QWIN = 26 / 22 / 12 / 15 windows per 128-bit
 * half for QW = 5 / 6 / 11 / 9 -- and out_ok[i] = the slot's ParsePubKey
 * verdict.  A slot at or past the slots that have the table set (at most
 * gv_keys_count()): zeros and 0; a rejected key: zeros and 0.
 * GV_EINVAL, and the outputs untouched, for a NULL ctx (or pointer with n >
 * 0), a bad dev_slot, a tabs the context holds no tables of (no kn or wide
 * arena), any groups[i] >= NG or js[i] outside 1..NT; n == 0 is GV_OK.  Reads
 * only: nothing is allocated in an arena, no counter or option moves; under
 * gv_keys_point's locks. */
int gv_keys_entry(gv_ctx* ctx, int dev_slot, int tabs, size_t n, const uint32_t* slots, const uint32_t* groups,
                  const uint32_t* js, uint8_t* out_xy64, uint8_t* out_ok);
/* Grouped-set readback (tests, tools): the key tables a scratch set of device
 * dev_slot keeps across calls (option "group_reuse"): set 0 / 1 the sets of
 * the device-resident calls, 2 / 3 those of the host slices.  Item i names
 * cache row rows[i], group groups[i] and entry js[i] in the layout of the
 * set's last grouped call ("group_layout" groups; 16 entries of 5-bit
 * windows, or with "k6" 4 groups of 32 entries of 6-bit windows; w0 as for
 * gv_keys_entry); out_key33 + 33*i = the 33 key bytes the row was built
 * from, as sent, out_xy64 / out_ok as gv_keys_entry's.  A row at or past the
 * rows in use: zeros and 0 in all three; a rejected key: its bytes, zeros
 * and 0.  Waits for the set's last call, so it may follow an asynchronous
 * gv_dev_verify_*.  GV_EINVAL, and the outputs untouched, for a NULL ctx (or
 * pointer with n > 0), a bad dev_slot or set, a set that holds no live cache
 * (never used, dropped, "group_reuse" 0), a group or entry outside the
 * layout; n == 0 is GV_OK.  Reads only, as gv_keys_entry. */
int gv_group_entry(gv_ctx* ctx, int dev_slot, int set, size_t n, const uint32_t* rows, const uint32_t* groups,
                   const uint32_t* js, uint8_t* out_key33, uint8_t* out_xy64, uint8_t* out_ok);

/* The arena's pubkey index (option "keys_index", below): which slot holds a
 * key.  With the option on, gv_keys_load and gv_keys_replace keep on every
 * device, beside the tables, each slot's 33 bytes as they were given (a key
 * ParsePubKey rejects too) and a hash table over them; a lookup returns a
 * slot only after comparing all 33 bytes with that slot's, so verifying by
 * the slot it returns gives exactly the pub33 verdict.  The index may be
 * incomplete -- a key whose probe finds no free word within 64 steps is left
 * out ("keys_index_left_out") and answers as not resident -- but it never
 * names a slot with other bytes.
 * gv_keys_find: slot_out[i] = the lowest slot holding exactly the bytes
 * pub33 + 33*i, or 0xFFFFFFFF.  Host buffers, the first device's index, under
 * gv_keys_point's locks.  GV_OK with every entry 0xFFFFFFFF on an empty arena;
 * n == 0 is GV_OK; GV_EINVAL when ctx, pub33 or slot_out is NULL or the
 * context has no live index ("keys_index" 0, an arena started without it, an
 * index its device's HBM budget refused): "cannot tell", which a caller must
 * not take for "not resident". */
int gv_keys_find(gv_ctx* ctx, size_t n, const uint8_t* pub33, uint32_t* slot_out);
/* The device-resident form, on dev_slot's index: d_pub33 = n x 33 key bytes
 * (any alignment), d_slot_out = n u32 words (4-byte aligned; NULL or
 * misaligned: GV_EINVAL and nothing is written).  Asynchronous on `stream`
 * (NULL: the context stream, ordered with the other calls on it -- after
 * every call enqueued before it, and the calls enqueued after it, the front
 * kernels of pipelined ones included, after it); its output can be passed
 * straight to gv_dev_verify_digests_keyed on the same stream (both NULL, or
 * the same caller stream; across two streams the caller orders them).
 * Same results and errors as gv_keys_find; GV_ENODEV for a bad dev_slot.
 *
 * A routed batch with a few keys that are not resident (option
 * "keys_index_split", below; default 0 = off).  gv_dev_verify_digests /
 * gv_dev_verify_msgs, on a caller stream or the context stream, read back how
 * many items M of a batch past "lat_max" the index did not find.  With
 * 0 < M <= "keys_index_split" the call splits instead of falling through:
 *  - all n lanes run the keyed throughput pipeline with the looked-up slots;
 *    a miss lane carries slot 0xFFFFFFFF, which every keyed kernel answers
 *    false, so this pass writes 0 at the miss positions;
 *  - the M items are compacted into a dense sub-batch (their 33 key bytes, 64
 *    signature bytes, digest or message offset and length; the message blob is
 *    shared) and verified by key bytes on the pub33 routes, never grouped (no
 *    host sync), the call's own thresholds choosing the kernel: a fused
 *    small-batch kernel up to "lat_max" / "lat_sl_max", the per-item pipeline
 *    past them.  It is enqueued behind the main batch's front kernels and runs
 *    under the main ladder;
 *  - its accept bits are ORed into d_bits at the items' positions as part of
 *    the call's bitmap write: behind the ladder's (or the unsort's) write,
 *    before any later call's bitmap write and before the call's scratch is
 *    released.  Calls into the same d_bits leave the last call's bits.
 * The verdicts are bit for bit those of the fall-through.  M == 0 runs the
 * keyed route, M past the option falls through whole, and so does a call
 * whose miss buffers or scratch the HBM budget or hipMalloc refuses: an index
 * that is incomplete or cannot split is never an error (only HIP failures are
 * GV_EHIP).  The miss buffers (133 B per row and a bitmap) belong to the
 * call's scratch set, are charged to "hbm_budget_mb", grow by doubling to the
 * M actually seen rounded up to 256 -- never to the option's value -- and are
 * freed by gv_close.  Stage times (gv_last_stage_ms, gv_stage_stats*) keep
 * describing the main batch; gv_route_stats counts both passes: one arena
 * route and one pub33-side route.  The calls read the arena exactly as routed
 * calls do (the rule about loads racing keyed verifies covers them). */
int gv_dev_keys_find(gv_ctx* ctx, int dev_slot, size_t n, const void* d_pub33, void* d_slot_out, void* stream);

/* VerifyBytes with the key given by slot: out_ok[i] is exactly what
 * gv_verify_digests / gv_verify_msgs return with pub33 = the key loaded into
 * slot[i]; a slot >= gv_keys_count() gives false.  Same batching, errors and
 * multi-device split as the pub33 entry points; batches up to "lat_max" take
 * the fused small-batch kernel with the key's table read from the arena. */
int gv_verify_digests_keyed(gv_ctx* ctx, size_t n, const uint32_t* slot, const uint8_t* sig64,
                            const uint8_t* dig32, uint8_t* out_ok);
int gv_verify_msgs_keyed(gv_ctx* ctx, size_t n, const uint32_t* slot, const uint8_t* sig64,
                         const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len,
                         uint8_t* out_ok);
/* Device-resident keyed digests: d_slot = n u32 slots on dev_slot. */
int gv_dev_verify_digests_keyed(gv_ctx* ctx, int dev_slot, size_t n, const void* d_slot, const void* d_sig64,
                                const void* d_dig32, void* d_bits, void* stream);

/* ---- ed25519 ------------------------------------------
 * out_ok[i] = tendermint v0.33.4 PubKeyEd25519(pub32[i]).VerifyBytes(msg_i,
 * sig64[i]) for a 64-byte signature, i.e. go1.14 crypto/ed25519 Verify:
 * sig[63] & 224 == 0, S < L (ScMinimal), A = FromBytes(pub) (non-canonical y
 * accepted, no small-order check), encode([S]B - [SHA-512(R||A||M) mod L]A)
 * == R as bytes.  Replaces, for a batch, the per-leaf call reached through
 * multisig.PubKeyMultisigThreshold.VerifyBytes for ed25519 sub-keys
 * (x/auth/ante/sigverify.go:210 via :303-306 / :325-338).  Signatures of any
 * other length are false without a call (VerifyBytes' first check), as for
 * secp256k1.  msg_blob may be NULL when every length is 0. */
int gv_verify_ed25519_msgs(gv_ctx* ctx, size_t n, const uint8_t* pub32, const uint8_t* sig64,
                           const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len,
                           uint8_t* out_ok);
/* Device-resident: d_pub32 (n x 32) and d_sig64 (n x 64) 16-byte aligned,
 * d_msg_off u64 / d_msg_len u32 per item; accept bitmap into d_bits
 * (ceil(n/64) u64 words).  Asynchronous on `stream` (NULL: the library's).
 * With option "ed_keys_index" on, a non-empty ed25519 arena and a live index
 * (gv_ed_keys_find, below) the call, at every n >= 1, first looks the batch's
 * keys up on the device: one small kernel, then a 4-byte read-back of the
 * miss count, for which the HOST WAITS -- the call blocks until everything
 * enqueued on `stream` before it and the lookup have finished, as the routed
 * secp256k1 calls do.  When every key is resident the batch then runs exactly
 * as gv_dev_verify_ed25519_msgs_keyed would with those slots (same kernels by
 * size, the wide tables when every slot has them, same bitmap write) and is
 * asynchronous from there on; one or more keys not found sends the whole batch
 * down the route it takes without the index.  Same verdicts either way; an
 * index that cannot answer is never an error (only HIP failures are GV_EHIP).
 * With the option on the call takes the arena's lock, then the device's, as
 * the keyed call; off, the device's alone. */
int gv_dev_verify_ed25519_msgs(gv_ctx* ctx, int dev_slot, size_t n, const void* d_pub32, const void* d_sig64,
                               const void* d_msg_blob, const void* d_msg_off, const void* d_msg_len, void* d_bits,
                               void* stream);
/* Cached ed25519 keys: the IBC 07-tendermint light client verifies a
 * validator set's commit signatures block after block
 * (x/ibc/07-tendermint/update.go:88 lite.Verify, misbehaviour.go:88-97
 * VerifyCommitTrusting), and multisig accounts keep their ed25519 sub-keys.
 * gv_ed_keys_load runs FromBytes once per key and keeps the comb table of -A
 * (j * 16^w * (-A), w < 64, j <= 8: 72 KB per key) and the raw key bytes
 * resident on every device; slot_out[i] receives key i's slot (a key
 * FromBytes rejects gets one too, and every verify against it is false).
 * gv_verify_ed25519_msgs_keyed gives exactly gv_verify_ed25519_msgs's verdict
 * with pub32 = the key loaded into slot[i] (a slot >= gv_ed_keys_count()
 * gives false).  Batches up to "ed_lat_max" (default 2048) take k_ed_lat_sl
 * (one signature per block, no doublings: ~0.1 ms end to end), larger ones the
 * throughput kernels.  Loading must not race keyed verifies of the same
 * context; gv_ed_keys_generation counts gv_ed_keys_reset calls. */
int gv_ed_keys_load(gv_ctx* ctx, size_t n, const uint8_t* pub32, uint32_t* slot_out);
int gv_ed_keys_reset(gv_ctx* ctx);
size_t gv_ed_keys_count(const gv_ctx* ctx);
uint64_t gv_ed_keys_generation(const gv_ctx* ctx);
/* Replacement: after GV_OK slot slots[i] behaves on every ed25519 keyed
 * route -- k_ed_lat_sl up to "ed_lat_max", k_ed_keyed past it, with
 * "ed_keyed" 0 the throughput kernels over the slot's raw key -- and in
 * gv_ed_keys_point as if pub32 + 32*i had been loaded into it (a key
 * FromBytes rejects gives a false slot; a key equal to one resident in
 * another slot is fine, the two slots are independent).  The table, the raw
 * bytes and the verdict are rebuilt on every device of the context, by the
 * kernels of gv_ed_keys_load ("ed_keys_split" picks the same pair), and the
 * host copy of the raw bytes follows once every device has succeeded.
 * Nothing is allocated in the arena, grown or moved: gv_ed_keys_count and
 * gv_ed_keys_generation do not change, so a caller that replaces a slot keeps
 * its own pubkey -> slot map right (drop the old key's entry; the generation
 * does not tell).  It takes the locks of gv_ed_keys_load (the arena's, then
 * each device's); keyed verifies hold the arena's lock for the whole call,
 * so a replacement never runs under one.
 * GV_EINVAL, and nothing changed, when a slot is >= gv_ed_keys_count() or
 * appears twice (ctx, slots or pub32 NULL with n > 0 too); n == 0 is GV_OK.
 * On GV_EHIP, or GV_ENOMEM from the scratch allocation, no slot named in the
 * call is trusted: the caller must gv_ed_keys_reset.  Option
 * "ed_keys_replaced" (read-only) counts the slots replaced since gv_open. */
int gv_ed_keys_replace(gv_ctx* ctx, size_t n, const uint32_t* slots, const uint8_t* pub32);
/* ed25519 key-arena readback (tests, tools): for each slot, out_enc32 + 32*i
 * = the canonical encoding of entry (w, j) of its table, j * 16^w * (-A)
 * (w < 64, 1 <= j <= 8, else GV_EINVAL); out_pub32 + 32*i = the raw key bytes
 * Verify hashes; out_ok[i] = its FromBytes verdict.  A slot >=
 * gv_ed_keys_count(): zeros and 0; a rejected key: its bytes, 0 and a zero
 * encoding.  Reads the first device's arena under gv_ed_keys_load's locks. */
int gv_ed_keys_point(gv_ctx* ctx, size_t n, const uint32_t* slots, uint32_t w, uint32_t j, uint8_t* out_enc32,
                     uint8_t* out_pub32, uint8_t* out_ok);
int gv_verify_ed25519_msgs_keyed(gv_ctx* ctx, size_t n, const uint32_t* slot, const uint8_t* sig64,
                                 const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len,
                                 uint8_t* out_ok);
/* Device-resident keyed ed25519: bit i of d_bits (ceil(n/64) u64 words, the
 * unused high bits of the last word 0) is exactly
 * gv_verify_ed25519_msgs_keyed's verdict for item i -- d_slot (n x u32, 4-byte
 * aligned), d_sig64 (n x 64, 16-byte aligned), d_msg_off u64 / d_msg_len u32
 * per item, d_msg_blob (may be NULL when every length is 0), all device
 * memory of dev_slot; GV_EINVAL, and d_bits untouched, for a NULL or
 * misaligned one.  A slot >= gv_ed_keys_count() gives 0; an empty arena gives
 * all zeros without a launch that reads the arena.  Every n >= 1 is answered:
 * up to "ed_lat_max" items on k_ed_lat_sl (one signature per block, the
 * radix-16 tables), more on k_ed_keyed with the lanes in slot order
 * ("sort_keys"), on the wide tables (option "ed_keys_wide") when every slot
 * has them -- "ed_keyed" does not apply: the items never reach the host.
 * Asynchronous on `stream` (NULL: the library's); its scratch use is ordered
 * after the previous call's, as for the other gv_dev_* calls.
 * Arena safety: the call holds the arena's lock while it enqueues and leaves
 * an event per device behind its last kernel.  gv_ed_keys_load,
 * gv_ed_keys_replace and a load after gv_ed_keys_reset wait for that event
 * before they write, move or free arena memory (a growth frees the old arena,
 * and so does a wide arena that stops): a batch enqueued before a replacement
 * sees the old keys, one enqueued after it the new ones. */
int gv_dev_verify_ed25519_msgs_keyed(gv_ctx* ctx, int dev_slot, size_t n, const void* d_slot, const void* d_sig64,
                                     const void* d_msg_blob, const void* d_msg_off, const void* d_msg_len,
                                     void* d_bits, void* stream);
/* Wide ed25519 arena readback (tests, tools): out_enc32 + 32*i = the
 * canonical encoding of entry (w, j) = j * 2^(rb w) * (-A) of slot slots[i]'s
 * wide table, rb = "ed_kw_rb" (6: w < 43, j = 1..32; 8: w < 32, j = 1..128);
 * out_ok[i] = the key's FromBytes verdict.  GV_EINVAL when there is no wide
 * arena ("ed_kw_rb" 0) or w / j is out of range.  A slot >= "ed_kw_keys":
 * zeros and 0; a rejected key: a zero encoding and 0.  Reads the first
 * device's wide arena under gv_ed_keys_point's locks. */
int gv_ed_keys_wide_point(gv_ctx* ctx, size_t n, const uint32_t* slots, uint32_t w, uint32_t j, uint8_t* out_enc32,
                          uint8_t* out_ok);
/* The ed25519 arena's pubkey index (option "ed_keys_index", below): which slot
 * holds a key.  The arena already keeps each slot's 32 bytes as they were
 * given (a key FromBytes rejects too); with the option on, gv_ed_keys_load and
 * gv_ed_keys_replace also keep on every device a hash table over them.  The
 * byte string is the identity, not the point: a non-canonical encoding and
 * its canonical twin are different keys, as they are to the hash inside
 * Verify.  A lookup returns a slot only after comparing all 32 bytes with
 * that slot's, so verifying by the slot it returns gives exactly the pub32
 * verdict.  The index may be incomplete -- a key whose probe finds no free
 * word within 64 steps is left out ("ed_keys_index_left_out") and answers as
 * not resident -- but it never names a slot with other bytes.
 * gv_ed_keys_find: slot_out[i] = the lowest slot holding exactly the bytes
 * pub32 + 32*i, or 0xFFFFFFFF.  Host buffers, the first device's index, under
 * gv_ed_keys_point's locks.  GV_OK with every entry 0xFFFFFFFF on an empty
 * arena (no launch); n == 0 is GV_OK; GV_EINVAL when ctx, pub32 or slot_out
 * is NULL or the context has no live index ("ed_keys_index" 0, an arena
 * started without it, an index its device's HBM budget refused): "cannot
 * tell", which a caller must not take for "not resident". */
int gv_ed_keys_find(gv_ctx* ctx, size_t n, const uint8_t* pub32, uint32_t* slot_out);
/* The device-resident form, on dev_slot's index: d_pub32 = n x 32 key bytes
 * (any alignment), d_slot_out = n u32 words (4-byte aligned; NULL or
 * misaligned: GV_EINVAL and nothing is written).  Asynchronous on `stream`
 * (NULL: the library's); its output can be passed straight to
 * gv_dev_verify_ed25519_msgs_keyed on the same stream (across two streams the
 * caller orders them).  It reads the arena as a keyed batch does and leaves
 * the same event behind, so loads and replacements wait for it.  Same results
 * and errors as gv_ed_keys_find; GV_ENODEV for a bad dev_slot. */
int gv_dev_ed_keys_find(gv_ctx* ctx, int dev_slot, size_t n, const void* d_pub32, void* d_slot_out, void* stream);

/* Options: "max_batch" (lanes per device launch, default 1<<20, at most
 * 0xFFFFFF00),
 * "lat_max" (batches of at most this many items -- per device slice -- take
 * a fused small-batch kernel, default 8192; 0 = never),
 * "lat_sl_max" (batches of at most this many items take the limb-sliced
 * small-batch kernels k_verify_lat_sl / k_verify_lat16_sl, one signature per
 * block; larger ones up to lat_max the four-lanes-per-signature
 * k_verify_lat / k_verify_lat16; default 2048),
 * "lat_max_keyed" / "lat_sl_max_keyed" (the same two bounds for keyed
 * batches, defaults 14336 / 1536: the sliced keyed kernel takes four waves
 * per signature, and the 16-lanes-per-signature keyed kernel beats the keyed
 * pipeline to ~14k; setting "lat_max" / "lat_sl_max" sets these too),
 * "lat_sliced" (0/1: 0 never takes the sliced kernels; default 1),
 * "ed_unc_lat_max" (uncached ed25519 host batches of at most this many
 * items take k_ed_lat_unc: one signature per block, FromBytes(A) in the
 * kernel; default 2048, 0 = never),
 * "lat_rows_max" (pub33 sliced batches of at most this many items take
 * k_verify_lat_sl4: five waves per signature, each ladder wave's four rows on
 * one accumulator, G from the k6 tables after the ladder; default 512, 0 =
 * never, env GV_LAT_ROWS_MAX),
 * "lat_zero_copy" (0/1: host-buffer digest batches on the sliced kernels
 * are read by the kernel straight from the pinned staging buffer and answered
 * as verdict bytes in pinned memory -- no H2D, memset or D2H; default 1),
 * "pipe_chunk" (host-buffer calls past lat_max: first chunk of the two-stream
 * copy/compute pipeline per device, default 262144; 0 = one chunk per
 * max_batch), "pipe_growth" (each later chunk at most this many times the one
 * before, default 4: the staging of chunk i+1 hides under the kernels of
 * chunk i), "stage_threads" (pageable -> pinned staging copy threads PER
 * DEVICE, the slice's own thread included: each device stages through its own
 * pool; default half the process's CPUs -- affinity capped by the cgroup
 * quota -- split over the devices, 1..8 each),
 * "stage_pieces" (pageable host chunks of at least 65,536 items are staged
 * into pinned memory in this many pieces, each piece's H2D right behind its
 * copy; default 2, env GV_STAGE_PIECES),
 * "lat_kw" (0/1: keyed sliced small batches whose slots all have the
 * resident arena's one-window wide tables take k_verify_lat16_kw -- no
 * doublings -- instead of the kn tables' k_verify_lat16_kn; default 1, env
 * GV_LAT_KW),
 * "async_chunk" / "async_growth" (submitted batches staged through the
 * library -- pageable buffers, messages: fixed chunks of async_chunk items,
 * each later one at most async_growth times the one before; default 262144
 * and 1, env GV_ASYNC_CHUNK / GV_ASYNC_GROWTH), "async_whole" (0/1:
 * submitted digest batches read in place from gv_host_alloc memory run as
 * ONE chunk when they queue behind a batch still in flight -- their copies
 * and front kernels then run under the previous batch's ladder -- and take
 * the pipe_chunk ramp on an idle device; default 1, env GV_ASYNC_WHOLE),
 * "h2d_serial" (0/1: a host slice's chunks send their inputs one after the
 * other -- each chunk's H2D waits for the previous chunk's -- so the chunk
 * the GPU needs first is not slowed by the next one's transfer; default 1,
 * env GV_H2D_SERIAL),
 * "gfull_item" (0/1: the per-item pub33 route -- batches not grouped by
 * key -- also adds G on the unsplit u1 from the "gfull" tables: 11 G
 * additions instead of 14; default 1, env GV_GFULL_ITEM),
 * "inv_small" (0/1: batches under 2^19 items fold fewer signatures per lane
 * in the s^-1 batch inversion, so it stays short where it precedes the first
 * ladder -- a host slice's first chunk; default 1, env GV_INV_SMALL),
 * "slice_plain_first" (host-buffer pub33 slices grouped by key: this many
 * items first on the per-item pipeline while the slice's key tables build;
 * 0 = off, the default; env GV_SLICE_PLAIN_FIRST),
 * "group_keys" (0/1: a pub33 batch past the small-batch bound with at least
 * "group_min" items (default 16384) whose distinct keys number at most
 * items / "group_div" (default 5) parses each distinct key once -- grouped
 * on the device, tables built into a per-batch arena, the items verified by
 * the keyed pipeline; same verdicts; default 1, env GV_GROUP_KEYS),
 * "group_reuse" (0/1: that arena is kept as a cache -- each of a device's
 * scratch sets remembers the keys whose tables it has built, all 33 bytes
 * compared, and a later batch on the set builds only the keys it has not
 * seen; rows are appended until the arena is full, then the cache is flushed
 * and the batch builds all its keys; any option that drains the pipeline
 * starts every cache cold; 0: every batch rebuilds every key, no k_group_*
 * kernel runs; same verdicts; default 1, env GV_GROUP_REUSE),
 * "group_promote" (0, 6, 7 or 9: a scratch set whose keys recur moves its
 * cache from k4's four groups per key to the kg layout of this many -- the
 * layouts of "kg", a dearer build per key and a ladder of 20 / 15 / 10
 * doublings instead of 30, k_ecmult_kn<5, NG>.  A set promotes on a batch of
 * at least "group_promote_min" items (default 262144; not quiescing) whose
 * lookup, like those of the set's two calls before it, missed fewer keys per
 * item than half the measured break-even: it flushes and rebuilds that
 * batch's keys once in the kg layout.  It goes back to k4's layout, the same
 * way, on a batch whose lookup misses more than the break-even.  The first
 * promotion allocates the larger arena within "hbm_budget_mb" -- refused:
 * the set stays on k4, no error, no retry until a quiescing option -- and
 * later promotions and demotions neither free nor allocate.  The flag
 * outlives whatever drops the cache (a promoted set rebuilds cold in the kg
 * layout); "kg", "k6", "gfull", "group_reuse" and the option itself clear
 * it.  Inert while "kg" or "k6" names a layout or "group_reuse" is 0; same
 * verdicts; 0 = never; default 9, env GV_GROUP_PROMOTE; quiescing).  A set's
 * first arena, allocated for a batch that could promote it, is sized for the
 * promoted layout when the budget holds it, so that a promotion allocates
 * nothing,
 * "ed_group" (0/1: ed25519 throughput batches -- gv_verify_ed25519_msgs and
 * the device-resident variant -- of at least "ed_group_min" items (default
 * 196608; host chunks of 262,144 qualify) with at most items / 16 (and 16384) distinct keys build each key's
 * comb table once (k_ed_keys into a per-batch arena) and verify on k_ed_keyed,
 * lanes in slot order; same verdicts; default 1, env GV_ED_GROUP),
 * "ed_keyed" (0/1: gv_verify_ed25519_msgs_keyed batches past "ed_lat_max"
 * run one signature per lane against the cached comb tables of -A -- 64
 * table adds for [h](-A), no doublings, lanes in slot order; 0 = the
 * throughput kernels over the slots' raw keys; same verdicts; default 1, env
 * GV_ED_KEYED),
 * "ed_group_r64" (0/1: the grouped route's per-batch ed25519 key tables are
 * radix-64 combs -- 43 windows of 32 entries, 43 additions per [h](-A)
 * instead of 64; same verdicts; default 1, env GV_ED_GROUP_R64),
 * "ed_keys_wide" (0, 6 or 8, else GV_EINVAL; default 0, env
 * GV_ED_KEYS_WIDE: gv_ed_keys_load also builds, in an arena of its own beside
 * the radix-16 one, each key's radix-2^6 comb of -A -- 43 windows of 32
 * entries, 198,144 B per key -- or radix-2^8 comb -- 32 windows of 128
 * entries, 576 KiB per key --, and k_ed_keyed batches, host and
 * device-resident, read them while every slot has them: 43 / 32 additions
 * per [h](-A) instead of 64; same verdicts.  Taken by an arena started from
 * slot 0; 0 stops their use at once.  The wide arena doubles up to
 * "ed_key_cap", is charged to "hbm_budget_mb" and is admitted only while the
 * device keeps the room the secp256k1 wide arena reserves; a refused growth,
 * a failed allocation or build frees it and stops it until gv_ed_keys_reset
 * -- never a gv_ed_keys_load error, every slot keeps its radix-16 table;
 * gv_ed_keys_replace rebuilds the wide tables of the slots that have them),
 * "ed_keys_wide_mb" (MiB, 0 = no limit, the default; env GV_ED_KEYS_WIDE_MB:
 * the wide ed25519 arena is never allocated larger),
 * "ed_keys_index" (0/1, else GV_EINVAL; default 0, env GV_ED_KEYS_INDEX: on for
 * exactly "1": gv_ed_keys_load and gv_ed_keys_replace also keep the ed25519
 * arena's pubkey index on every device -- a table of 4 B x T, T the power of
 * two >= 2 x the arena's capacity and >= 512, over the key bytes the arena
 * holds anyway; charged to "hbm_budget_mb"; a refused or failed allocation or
 * a failed launch stops the index on that device until gv_ed_keys_reset and is
 * never a gv_ed_keys_load / gv_ed_keys_replace error -- gv_ed_keys_find /
 * gv_dev_ed_keys_find answer from it, and gv_dev_verify_ed25519_msgs runs a
 * batch whose keys are all resident as the keyed call would, see there.  Taken
 * by an arena started from slot 0: a running arena keeps what it has until
 * gv_ed_keys_reset; 0 stops the use of the index at once),
 * "ed_keys_index_seed" (test hook: the 64-bit seed of that index's hash, drawn
 * per context at gv_open; GV_EINVAL unless the ed25519 arena is empty),
 * "ed_btab16" (0/1: k_ed_keyed -- cached keys past "ed_lat_max" and grouped
 * keys -- and the per-item throughput kernels add [s]B from a radix-2^16 comb table of B, j * 65536^w * B for
 * w < 16 and j <= 2^15 (56.6 MB per device, built on first use): 16
 * additions instead of 32; same verdicts; default 1, env GV_ED_BTAB16; when
 * the table's allocation or build fails the same kernels add [s]B from the
 * radix-256 table, and gv_get_option "ed_btab16_live" (read only) tells:
 * 1 when the first device holds a built table, else 0 -- reading it never
 * builds the table),
 * "sort_keys" (0/1: keyed throughput batches on the 4-group ladder -- cached
 * slots, grouped keys -- run their lanes in slot order: a counting sort by
 * slot, the signature rows read in that order, the accept bits gathered back
 * to item order; same verdicts; default 1, env GV_SORT_KEYS),
 * "pipeline_dev" (0/1: device-resident calls on the context stream past the
 * small-batch bound are pipelined -- consecutive calls alternate scratch sets,
 * their unpack / s^-1 / prep kernels run under the previous call's ladder on
 * a stream above the ladders' priority (env GV_LADDER_PRIO "front", the
 * default; "ladder" / "equal" for A/B); a caller stream is never pipelined;
 * default 1, env GV_PIPELINE),
 * "two_ladders" (0/1: pipelined calls' ladders alternate two streams, so the
 * next ladder fills the current one's tail; bitmap writes stay in call order;
 * default 1, env GV_TWO_LADDERS),
 * "gfull" (0/1: keyed batches on the 4-group ladder add G from the unsplit
 * u1 = e/s -- 11 signed 25-bit windows from tables of 2^o G (6 GiB per device,
 * built by gv_open) -- instead of 14 GLV windows; same verdicts;
 * default 1, env GV_GFULL; route counter GV_ROUTE_K4F),
 * "k6" (0/1: in-batch grouped keys on the 6-bit-window ladder -- 4 groups of
 * 32-entry key tables, 30 doublings, G from 11 24-bit windows of the unsplit
 * u1 (5.5 GiB of tables, built by gv_open); same verdicts; default 0, env
 * GV_K6; route counter GV_ROUTE_K6),
 * "kg" (0 or 6 / 7 / 9: in-batch grouped keys on the many-group 5-bit
 * ladder -- k4's 16-entry tables of 5-bit windows split over kg groups
 * instead of 4, so the ladder runs ceil(26 / kg) positions (kg 7: 15
 * doublings, 9: 10) for kg x 16 table entries per key; G from 11 24-bit
 * windows of the unsplit u1 after the last doubling, on the real curve; same
 * verdicts; takes precedence over "k6"; env GV_KG; route counter
 * GV_ROUTE_KG),
 * "keys_k6" (0/1: gv_keys_load also builds each key's 6-bit-window tables --
 * 11 groups of 32 entries on one Z, 28 KB per key beside the 5.4 KB of k4
 * tables -- and keyed throughput batches whose slots all have them run the
 * 6-doubling ladder; small keyed batches keep the k4 tables; same verdicts;
 * default 1, env GV_KEYS_K6; route counter GV_ROUTE_KN),
 * "keys_wide" (0/1/2: gv_keys_load also builds each key's wide-window tables
 * on one Z, in an arena of their own that grows by doubling while the HBM
 * budget holds it and the device keeps room for the k4 / k6 arena to reach
 * key_cap.  The arena has one of four layouts, in order of falling memory per
 * key:
 *   A  11-bit windows, one per group: 12 tables of 1,024 entries, 768 KiB per
 *      key, no doublings and 24 Q additions per verify;
 *   B  11-bit, two per group: 6 tables, 384 KiB, 11 doublings;
 *   C  9-bit, one per group: 15 tables of 256 entries, 240 KiB, no doublings
 *      and 30 Q additions;
 *   D  9-bit, two per group: 8 tables, 128 KiB, 9 doublings.
 * 2 (default) starts an arena at A, 1 at B; an arena whose growth is refused
 * moves as a whole to the next layout of the list (the loaded keys are read
 * back from the k4 tables and rebuilt from slot 0), and only a refusal of D
 * stops the wide tables until gv_keys_reset; an arena started from slot 0
 * after gv_keys_reset starts at the top again.  Keyed throughput batches
 * whose slots all have wide tables run that ladder (else the k6 one); same
 * verdicts; the option takes effect for an arena started from slot 0, 0 at
 * once; env GV_KEYS_WIDE; route counters GV_ROUTE_KW (one window per group,
 * either width) / GV_ROUTE_KW2 (two)),
 * "keys_wide_qw" (0/9/11: the widths the wide arena may take -- 0 (default):
 * all four layouts; 11: A and B only, past B the k6 tables; 9: C and D only,
 * "keys_wide" 2 starting at C and 1 at D; anything else is GV_EINVAL; takes
 * effect for an arena started from slot 0; env GV_KEYS_WIDE_QW; the widths
 * are the build's "kw_qw" / "kwn_qw"),
 * "keys_wide_mb" (MiB: the wide arena is never allocated larger than this --
 * a growth whose new arena would pass it is refused and the arena moves down
 * the layouts as above; 0 = no limit, the default; env GV_KEYS_WIDE_MB),
 * "keys_index" (0/1: gv_keys_load and gv_keys_replace also keep the arena's
 * pubkey index on every device -- 36 B of key bytes per slot of capacity and
 * a table of at least two 4-byte words per slot, charged to "hbm_budget_mb";
 * a refused or failed allocation stops the index on that device until
 * gv_keys_reset and is never a gv_keys_load error -- gv_keys_find /
 * gv_dev_keys_find answer from it, and gv_dev_verify_digests /
 * gv_dev_verify_msgs look a batch past "lat_max" up in it (one kernel and a
 * 4-byte read-back): when every key of the batch is resident the batch runs
 * on the keyed throughput pipeline as gv_dev_verify_digests_keyed would with
 * those slots -- the same arena tables, sort and ladder, no per-call key
 * parsing or table build; one exception: a routed batch always takes the
 * throughput pipeline, also in the band "lat_max" < n <= "lat_max_keyed"
 * (8193..14336 by default) where the keyed call itself takes the keyed
 * small-batch kernel -- and on any miss exactly as without the option; same
 * verdicts either way.
 * With it on, those two calls read the arena: the rule of the keyed calls,
 * "loading must not race keyed verifies of the same context", then covers
 * them too (gv_keys_load and gv_keys_replace drain the pipelined ladders
 * before they write).  Taken by an arena started from slot 0, a running
 * arena keeps what it has until gv_keys_reset; 0 stops the use of the index
 * at once; default 0, env GV_KEYS_INDEX=1),
 * "keys_index_seed" (test hook: the 64-bit seed of the index hash, drawn per
 * context at gv_open; GV_EINVAL unless the arena is empty),
 * "keys_index_split" (0 .. 0xFFFFFF00: the most non-resident items per call
 * with which a batch the index routes is still split -- the resident items on
 * the arena, the others as a sub-batch on the pub33 routes, see "a routed
 * batch with a few keys that are not resident" above; past it, and with 0,
 * any miss sends the whole batch to the pub33 routes as before; default 0, no
 * environment variable.  Recommended: the most first-seen keys a batch is
 * expected to carry -- on 1M-item batches over 65,536 resident keys the split
 * beat the fall-through by more than the +-3 % box spread at every count
 * measured, 1.74x at 1 miss down to 1.18x at 65,536, the largest measured, so
 * the break-even lies past 65,536 per 1M items; a single miss costs 0.9 %
 * of the all-resident rate),
 * "key_cap" / "ed_key_cap" (the callers' reset points of the secp256k1 /
 * ed25519 key arenas: an arena grows by doubling up to it and exactly past it;
 * defaults GV_KEY_CAP / GV_ED_KEY_CAP, env of the same names; the Go shim sets
 * both to its KeyCap / EdKeyCap at Open),
 * "hbm_budget_mb" (MiB of optional device tables per device -- the G tables
 * past the GLV pair, the key arenas, the grouping arenas; a table past the
 * budget is not built and batches take the schedule that needs less, with the
 * same verdicts: k6 -> k4 -> the 125-doubling keyed ladder, full-scalar G ->
 * GLV G; keys_load returns GV_ENOMEM when not even the k4 arena fits; 0 = no
 * limit, the default; env GV_HBM_BUDGET_MB; the large G tables are built by
 * gv_open unless env GV_EAGER_TABLES=0),
 * "time_kernels" (0/1: record HIP events around each kernel stage; the
 * ladder's time is its own start to end),
 * "fault_inject" (0/1: every verify call fails with GV_EFAULT; test hook). */
int gv_set_option(gv_ctx* ctx, const char* key, long long val);
/* The current value of a schedule option set by gv_set_option or its
 * environment variable: "kg", "k6", "gfull", "keys_k6", "keys_wide",
 * "keys_wide_qw", "keys_wide_mb", "group_keys", "sort_keys", "pipeline_dev",
 * "two_ladders", "key_cap", "max_batch", "async_chunk", "async_growth",
 * "async_whole", "lat_kw", and (read only) "kw_qw" / "kwn_qw", the wide and
 * the narrow window width of the resident arena's wide tables this library
 * was built with (11 / 9; "kwn_qw" 0: one width only), and "kw_arena_qw" /
 * "kw_arena_ng", the window width and the group count of the first device's
 * wide arena as the last gv_keys_load left it (both 0: no slot has wide
 * tables), and "keys_replaced" / "ed_keys_replaced", the slots
 * gv_keys_replace / gv_ed_keys_replace have rewritten since gv_open, and
 * "ed_keys_wide" / "ed_keys_wide_mb" with (read only) "ed_kw_rb", the radix
 * bits of the first device's wide ed25519 arena (0: no slot has wide tables),
 * "ed_kw_keys", the slots that have them, and "ed_keyed_wide", the keyed
 * ed25519 batches (host calls: chunks) that ran on wide tables since gv_open,
 * and (read only) "ed_btab16_live" (1: the first device holds a built
 * radix-2^16 comb table of B, see "ed_btab16"; 0: not built yet, or its
 * allocation or build failed and [s]B comes from the radix-256 table),
 * and "keys_index" with (read only) "keys_index_live" (1: the first device's
 * index covers the arena as it stands), "keys_index_keys" (the slots in it),
 * "keys_index_left_out" (keys the probe bound kept out of the table),
 * "keys_index_words" (its table's words), "keys_index_hit" /
 * "keys_index_miss" (pub33 device batches routed onto the keyed pipeline /
 * that fell through on a miss, since gv_open), "keys_index_launches" (index
 * kernels launched since gv_open: 0 while the option has never been on) and
 * "keys_index_find_ns" (the last routed lookup's kernel, HIP events, with
 * "time_kernels" on), and "ed_keys_index" with (read only)
 * "ed_keys_index_live", "ed_keys_index_keys", "ed_keys_index_left_out",
 * "ed_keys_index_words" (the first device's ed25519 index) and
 * "ed_keys_index_hit" / "ed_keys_index_miss" / "ed_keys_index_launches" (pub32
 * device batches run keyed / that fell through on a miss, and k_edkidx_*
 * launches, since gv_open), each meaning what its "keys_index_*" counterpart
 * means, and "keys_index_split" with (read only)
 * "keys_index_split_calls" / "keys_index_split_items" (routed batches whose
 * non-resident items were split off, and the sum of those items, since
 * gv_open: a split call counts in "keys_index_hit", not in "keys_index_miss"
 * -- which keeps meaning that the whole batch fell through -- and adds 3 to
 * "keys_index_launches": its find, split and merge kernels), and "group_reuse" with (read only) "group_reuse_hit" /
 * "group_reuse_built" (distinct keys of grouped batches whose tables were at
 * hand / were built, by calls with the option on, since gv_open),
 * "group_reuse_reset" (caches flushed: full, or holding another schedule's
 * tables), "group_reuse_launches" (k_group_* launches since gv_open: 0 while
 * the option has never been on) and "group_reuse_rows" (the row capacity of
 * the first device's first scratch set's grouping arena; 0: none yet),
 * "group_promote" and "group_promote_min" with (read only) "group_layout"
 * (groups per key of the tables the first device's last grouped call ran on:
 * 4 for k4's and k6's layouts, the kg layout's NG otherwise; 0: none yet),
 * "group_promoted" / "group_demoted" (sets moved to the "group_promote"
 * layout / back to k4's, since gv_open) and "hbm_optional_bytes" (the bytes
 * of optional tables "hbm_budget_mb" counts on the first device).
 * GV_EINVAL for any other key.  Instrumentation (bench route
 * attribution). */
int gv_get_option(gv_ctx* ctx, const char* key, long long* val);

/* Asynchronous host batches.  gv_submit_* queue a batch with the arguments
 * of the matching gv_verify_* entry point and return at once with a ticket;
 * gv_wait(ticket) blocks until that batch's verdicts are in out_ok and
 * returns its result (the gv_verify_* codes; a ticket is waited for once).
 * Batches run in submission order per context, each device's slices as one
 * stream of chunks: the next batch's staging, key grouping and key tables run
 * while the previous batch's last chunks compute, so a caller that keeps a
 * batch queued ahead (the next block's PreVerifyTxs, a replay) gets the
 * device-resident pipeline's overlap from host buffers.  Unlike gv_verify_*,
 * the library keeps the caller's pointers until gv_wait returns: the buffers
 * (ideally gv_host_alloc memory, read in place) must stay valid and unchanged
 * until then.  gv_wait is also a ticket's release: a caller that abandons a
 * batch (an error of its own between submit and wait) still waits for it,
 * since the library reads and writes its buffers until the batch is done; a
 * ticket never waited keeps a few hundred bytes of bookkeeping until gv_close,
 * which finishes the queued batches and frees it.  gv_keys_load /
 * gv_keys_reset wait for every submitted batch first, and submissions made
 * while one of them runs wait until it returns.  Replaces nothing in the
 * reference (its ante handler verifies synchronously, x/auth/ante/
 * sigverify.go:210); it is how baseapp's pre-verification hook keeps the
 * GPU busy across blocks (baseapp/abci.go:203-221). */
int gv_submit_digests(gv_ctx* ctx, size_t n, const uint8_t* pub33, const uint8_t* sig64, const uint8_t* dig32,
                      uint8_t* out_ok, uint64_t* ticket);
int gv_submit_digests_keyed(gv_ctx* ctx, size_t n, const uint32_t* slot, const uint8_t* sig64, const uint8_t* dig32,
                            uint8_t* out_ok, uint64_t* ticket);
int gv_submit_msgs(gv_ctx* ctx, size_t n, const uint8_t* pub33, const uint8_t* sig64, const uint8_t* msg_blob,
                   const uint64_t* msg_off, const uint32_t* msg_len, uint8_t* out_ok, uint64_t* ticket);
int gv_submit_msgs_keyed(gv_ctx* ctx, size_t n, const uint32_t* slot, const uint8_t* sig64, const uint8_t* msg_blob,
                         const uint64_t* msg_off, const uint32_t* msg_len, uint8_t* out_ok, uint64_t* ticket);
int gv_wait(gv_ctx* ctx, uint64_t ticket);

/* With "time_kernels" on: milliseconds of the last launch's stages on dev_slot
 * (unpack+sha, prep, ecmult), measured with HIP events on the launch stream. */
int gv_last_stage_ms(gv_ctx* ctx, int dev_slot, float* unpack_ms, float* prep_ms, float* ecmult_ms);

/* With "time_kernels" on: average stage milliseconds over every launch on
 * dev_slot since the previous call (at most the last 256 launches); *count
 * receives the number of launches averaged.  Synchronises dev_slot. */
int gv_stage_stats(gv_ctx* ctx, int dev_slot, int* count, double* unpack_ms, double* prep_ms,
                   double* ecmult_ms);

/* Same, per stage: ms[0] unpack (+ SHA-256 on the message path), ms[1]
 * k_scalar_inv, ms[2] k_prep, ms[3] k_ecmult (fused latency kernel: ms[3]). */
int gv_stage_stats4(gv_ctx* ctx, int dev_slot, int* count, double ms[4]);
/* Host-buffer calls on a multi-device context: per device slot, the wall time
 * (ms) and item count of that device's slice in the last gv_verify_* call
 * (bench.py --inproc: per-device rates).  Returns the number of slots written. */
int gv_last_slices(gv_ctx* ctx, double* ms_out, size_t* n_out, int cap);
/* Pinned host memory for a caller's input buffers: a host-buffer digest call
 * (gv_verify_digests[_bits|_keyed]) whose pub33 / slot, sig64 and dig32
 * arrays lie in such memory skips the library's pageable -> pinned staging
 * copy (the device reads them in place: DMA, or zero-copy for small batches).
 * The Go shim packs its batches into these buffers. */
int gv_host_alloc(gv_ctx* ctx, size_t bytes, void** out);
int gv_host_free(gv_ctx* ctx, void* p);
/* In-batch key grouping (options "group_keys", "ed_group"): on dev_slot, the
 * number of batches -- secp256k1 and ed25519 -- that took the grouped (keyed)
 * pipeline and the keys whose tables they built (with "group_reuse" the
 * keys the sets' caches did not hold; every distinct key without it). */
int gv_group_stats(gv_ctx* ctx, int dev_slot, uint64_t* batches, uint64_t* keys);
/* Batches per secp256k1 schedule on dev_slot since gv_open, out[GV_ROUTES]:
 * GV_ROUTE_PUB33 (per-item pipeline: k_prep + k_ecmult), GV_ROUTE_KEYED125
 * (keyed, 125-doubling ladder), GV_ROUTE_K4 (keyed 4-group ladder over the
 * key arena), GV_ROUTE_K6 (in-batch key grouping on the 6-bit-window ladder),
 * GV_ROUTE_LAT (small pub33 batches: gv_lat.hip kernels), GV_ROUTE_LAT_KEYED
 * (small keyed batches), GV_ROUTE_K4F (the 4-group ladder with the G half on
 * the unsplit scalar, 25-bit windows), GV_ROUTE_ITEMF (the per-item pipeline
 * with the G half on the unsplit scalar, "gfull_item"), GV_ROUTE_KN (keyed
 * batches on the resident arena's k6 tables: 11 groups of 6-bit windows, 6
 * doublings, option "keys_k6"), GV_ROUTE_ED_LAT (small uncached ed25519
 * host batches on k_ed_lat_unc, option "ed_unc_lat_max"), GV_ROUTE_KW (keyed
 * batches on the resident arena's wide-window tables, one window per group:
 * 12 groups at 11 bits or 15 at 9, no doublings, option "keys_wide"),
 * GV_ROUTE_KW2 (the same with two windows per group: 6 groups and 11
 * doublings, or 8 and 9), GV_ROUTE_KG (in-batch
 * key grouping on the many-group 5-bit ladder, option "kg").  Instrumentation only (bench route
 * attribution, node metrics). */
#define GV_ROUTE_PUB33 0
#define GV_ROUTE_KEYED125 1
#define GV_ROUTE_K4 2
#define GV_ROUTE_K6 3
#define GV_ROUTE_LAT 4
#define GV_ROUTE_LAT_KEYED 5
#define GV_ROUTE_K4F 6
#define GV_ROUTE_ITEMF 7
#define GV_ROUTE_KN 8
#define GV_ROUTE_ED_LAT 9
#define GV_ROUTE_KW 10
#define GV_ROUTE_KW2 11
#define GV_ROUTE_KG 12
#define GV_ROUTES 13
int gv_route_stats(gv_ctx* ctx, int dev_slot, uint64_t out[GV_ROUTES]);

const char* gv_strerror(int code);

/* Test hook: run one arithmetic building block per item on dev_slot
 * (op codes in gv_kernels.hip k_debug; in/out = n x 16 little-endian u32
 * host arrays).  Used by the GPU unit tests only. */
int gv_debug_op(gv_ctx* ctx, int dev_slot, int op, size_t n, const uint32_t* in, uint32_t* out);

/* Test hook for the limb-sliced layers of the small-batch kernels
 * (secp_fsl.cuh, ed_fsl.cuh, the row-parallel rounds): one item per 64-lane
 * wave, operands replicated in its four 16-lane rows.  in = n x 80 words:
 * operand j's nine raw limbs (unreduced) at words 9j..9j+8, j < 8 (the
 * cached-point additions take eight field elements), word 79 = flags (1 neg,
 * 2 pre, 4 / 8 first / second input at infinity, 16 words, not limbs: the op
 * reads canonical words from word 0 on).  out = n x 80 words: four result
 * slots of 16 words (all sixteen lanes of row 0), then 16 status words
 * (0 boolean result, 1 infinity out, 2 the four rows agree, 3 op known).
 * Op codes: GV_SLOP_* in csrc/gv_kernels.h.  GV_EINVAL for an unknown op.
 * Used by the GPU unit tests only. */
int gv_debug_sl_op(gv_ctx* ctx, int dev_slot, int op, size_t n, const uint32_t* in, uint32_t* out);

/* Test hook for the one-lane 9 x 29 layers (secp_fe29.cuh, secp_fe29x.cuh,
 * secp_group29.cuh, secp_group29x.cuh, ed_fe29.cuh, ed_group.cuh,
 * ed_scalar.cuh): one item per lane, one function per item, in the item
 * layout of gv_debug_sl_op.  in = n x 80 words: operand j's nine raw limbs at
 * 9j..9j+8, j < 8, word 79 = flags (1 neg, 2 no T out, 4 / 8 first / second
 * input at infinity, 16 words, not limbs, bits 8..11 the table entry of
 * ge_add_tab).  out = n x 80 words: four result slots of 16 words, then 16
 * status words (0 boolean result, 1 infinity out, 3 op known and run).
 * Op codes: GV_LNOP_* in csrc/gv_lane.h; a secp256k1 op c runs in the
 * one-chain unit, c + 64 in the two-chain unit of the small-batch kernels.
 * GV_EINVAL for an unknown op.  Used by the GPU unit tests only. */
int gv_debug_lane_op(gv_ctx* ctx, int dev_slot, int op, size_t n, const uint32_t* in, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* GPUVERIFY_H */
