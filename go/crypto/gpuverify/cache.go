package gpuverify

import (
	"container/list"
	"crypto/sha256"
	"sync"

	"github.com/tendermint/tendermint/crypto/ed25519"
	"github.com/tendermint/tendermint/crypto/secp256k1"
)

// Leaf kinds in a verdict-cache key.
const (
	KindSecp256k1 byte = 0
	KindEd25519   byte = 1
)

// LeafKey is the verdict-cache key of one VerifyBytes(msg, sig) leaf:
// SHA256(kind || pub || sig || SHA256(msg)).  A secp256k1 verdict depends on
// msg only through SHA256(msg) (tendermint crypto.Sha256 -> ecdsa.Verify), an
// ed25519 verdict on msg itself -- which SHA256(msg) identifies (collision
// resistance) -- so a cached verdict is exactly the reference's answer.
func LeafKey(kind byte, pub, sig, msg []byte) [32]byte {
	h := sha256.Sum256(msg)
	b := make([]byte, 0, 1+len(pub)+len(sig)+32)
	b = append(b, kind)
	b = append(b, pub...)
	b = append(b, sig...)
	b = append(b, h[:]...)
	return sha256.Sum256(b)
}

// VerdictCache is a bounded LRU map LeafKey -> verdict, safe for concurrent
// use.  PreVerifyTxs fills it; BatchSigVerificationDecorator reads it.
type VerdictCache struct {
	mu  sync.Mutex
	cap int
	m   map[[32]byte]*list.Element
	ll  *list.List
}

type cacheEntry struct {
	key [32]byte
	ok  bool
}

// NewVerdictCache returns a cache holding at most capacity verdicts.
func NewVerdictCache(capacity int) *VerdictCache {
	if capacity < 1 {
		capacity = 1
	}
	return &VerdictCache{cap: capacity, m: make(map[[32]byte]*list.Element, capacity), ll: list.New()}
}

// Get returns (verdict, true) on a hit.
func (c *VerdictCache) Get(k [32]byte) (bool, bool) {
	c.mu.Lock()
	defer c.mu.Unlock()
	if e, ok := c.m[k]; ok {
		c.ll.MoveToFront(e)
		return e.Value.(*cacheEntry).ok, true
	}
	return false, false
}

// Put records a verdict, evicting the least recently used entry when full.
func (c *VerdictCache) Put(k [32]byte, ok bool) {
	c.mu.Lock()
	defer c.mu.Unlock()
	if e, hit := c.m[k]; hit {
		e.Value.(*cacheEntry).ok = ok
		c.ll.MoveToFront(e)
		return
	}
	if c.ll.Len() >= c.cap {
		old := c.ll.Back()
		c.ll.Remove(old)
		delete(c.m, old.Value.(*cacheEntry).key)
	}
	c.m[k] = c.ll.PushFront(&cacheEntry{k, ok})
}

// Len is the number of cached verdicts.
func (c *VerdictCache) Len() int {
	c.mu.Lock()
	defer c.mu.Unlock()
	return c.ll.Len()
}

// slotClock is the second-chance clock over the key arena's slots (GPU
// KeyResident; the C++ mirror's rule, host/gvhost.cpp verify_secp): per slot
// the key it holds (the slot map's reverse), a reference bit set by every
// batch that names the slot, and the stamp of the last such batch.  The hand
// persists across batches.  Guarded by GPU.mu.
type slotClock struct {
	keys  []secp256k1.PubKeySecp256k1
	ref   []bool
	stamp []uint64
	hand  int
	batch uint64
}

func (c *slotClock) reset() { c.keys, c.ref, c.stamp, c.hand = nil, nil, nil, 0 }

// begin starts a batch: the slots it touches are never its victims.
func (c *slotClock) begin() { c.batch++ }

func (c *slotClock) touch(slot uint32) {
	if int(slot) < len(c.ref) {
		c.ref[slot], c.stamp[slot] = true, c.batch
	}
}

// hold records that slot now holds key, named by the batch in hand.
func (c *slotClock) hold(slot uint32, key secp256k1.PubKeySecp256k1) {
	for int(slot) >= len(c.keys) {
		c.keys = append(c.keys, secp256k1.PubKeySecp256k1{})
		c.ref = append(c.ref, false)
		c.stamp = append(c.stamp, 0)
	}
	c.keys[slot] = key
	c.touch(slot)
}

// victims sweeps from the hand over the first count slots -- two turns at
// most: the first clears reference bits, the second takes -- for need slots
// the batch in hand does not name.  nil when there are too few (nothing
// changed); undo puts the sweep back when the caller cannot use the victims.
func (c *slotClock) victims(count, need int) (v []uint32, undo func()) {
	if need == 0 {
		return nil, func() {}
	}
	span := count
	if span > len(c.keys) {
		span = len(c.keys)
	}
	hand0, h := c.hand, 0
	if span > 0 {
		h = c.hand % span
	}
	var cleared []uint32
	for step := 0; step < 2*span && len(v) < need; step, h = step+1, (h+1)%span {
		switch {
		case c.stamp[h] == c.batch:
		case c.ref[h]:
			c.ref[h] = false
			cleared = append(cleared, uint32(h))
		default:
			v = append(v, uint32(h))
			c.stamp[h] = c.batch
		}
	}
	undo = func() {
		for _, s := range v {
			c.stamp[s] = 0
		}
		for _, s := range cleared {
			c.ref[s] = true
		}
		c.hand = hand0
	}
	if len(v) < need {
		undo()
		return nil, func() {}
	}
	c.hand = h
	return v, undo
}

// edSlotClock is the same clock over the ed25519 key arena's slots (GPU
// EdKeyResident; host/gvhost.cpp verify_ed).  The reference bits, stamps and
// the hand are slotClock's; its key array only counts the slots here, and the
// ed25519 keys the slots hold stand beside it.
type edSlotClock struct {
	slotClock
	edKeys []ed25519.PubKeyEd25519
}

func (c *edSlotClock) reset() { c.slotClock.reset(); c.edKeys = nil }

// hold records that slot now holds key, named by the batch in hand.
func (c *edSlotClock) hold(slot uint32, key ed25519.PubKeyEd25519) {
	c.slotClock.hold(slot, secp256k1.PubKeySecp256k1{})
	for int(slot) >= len(c.edKeys) {
		c.edKeys = append(c.edKeys, ed25519.PubKeyEd25519{})
	}
	c.edKeys[slot] = key
}
