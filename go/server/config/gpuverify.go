package config

// Node configuration of the GPU signature verifier (SURVEY.md §5): app.toml
// keys under [gpu-verify], next to the BaseConfig of server/config/config.go.
//
// Patch (two lines): add the field to Config (config.go:44-47)
//
//	GPUVerify GPUVerifyConfig `mapstructure:"gpu-verify"`
//
// and DefaultGPUVerifyConfig() to DefaultConfig (config.go:78-88); append
// GPUVerifyTemplate to the app.toml template (server/config/toml.go).  The
// start command binds the matching flags (server/gpuverify_flags.go).

import (
	"fmt"
	"strconv"
	"strings"
	"time"
)

// GPUVerifyConfig: every knob of the verifier a node operator sets.
type GPUVerifyConfig struct {
	// Enable routes signature checks to the GPU; false keeps the reference
	// CPU path (the decorator then verifies with gpuverify.CPU).
	Enable bool `mapstructure:"enable"`
	// Devices: comma-separated HIP device ids ("" = every visible device).
	Devices string `mapstructure:"devices"`
	// MaxBatch: largest batch one device call takes (gv_set_option max_batch).
	MaxBatch int `mapstructure:"max-batch"`
	// CPUBelow: batches with fewer leaves run the reference VerifyBytes.
	CPUBelow int `mapstructure:"cpu-below"`
	// Keyed: verify through the HBM account-key arena (SURVEY.md §8f-2).
	Keyed bool `mapstructure:"keyed"`
	// KeyLoadMin: smallest batch that loads keys into the arena.
	KeyLoadMin int `mapstructure:"key-load-min"`
	// KeyCap, EdKeyCap: arena sizes at which the arenas are reset.
	KeyCap   int `mapstructure:"key-cap"`
	EdKeyCap int `mapstructure:"ed-key-cap"`
	// KeyResident: keep the secp256k1 arena at this many slots by replacing
	// the least recently used keys (gv_keys_replace); 0 = off.
	KeyResident int `mapstructure:"key-resident"`
	// EdKeyResident: the same for the ed25519 arena (gv_ed_keys_replace);
	// 0 = off, at most EdKeyCap.
	EdKeyResident int `mapstructure:"ed-key-resident"`
	// KeysWideQW: window widths of the key arena's wide tables (gv_set_option
	// keys_wide_qw): 0 = 11-bit, then 9-bit when those no longer fit; 11 or 9
	// = that width only.
	KeysWideQW int `mapstructure:"keys-wide-qw"`
	// EdKeysWide: the ed25519 arena also keeps radix-2^6 (6) or radix-2^8 (8)
	// comb tables for large keyed batches (gv_set_option ed_keys_wide); 0 =
	// the radix-16 tables only.
	EdKeysWide int `mapstructure:"ed-keys-wide"`
	// KeysIndex: the library keeps a device-side pubkey -> slot index of the
	// key arena (gv_set_option keys_index; gv_keys_find): device-resident
	// pub33 batches whose keys are all resident run on the arena's tables.
	KeysIndex bool `mapstructure:"keys-index"`
	// KeysIndexSplit: such a batch may hold up to this many items whose keys
	// are not resident and still run on the arena's tables, those items
	// verified by key bytes beside it (gv_set_option keys_index_split; 0 =
	// any such item sends the whole batch to the pub33 routes).
	KeysIndexSplit int `mapstructure:"keys-index-split"`
	// EdKeysIndex: the same index for the ed25519 key arena (gv_set_option
	// ed_keys_index; gv_ed_keys_find): device-resident pub32 batches whose keys
	// are all resident run on the arena's tables.
	EdKeysIndex bool `mapstructure:"ed-keys-index"`
	// CacheEntries: the verdict cache (0 = no cache).
	CacheEntries int `mapstructure:"cache-entries"`
	// CheckTxWindowTxs / CheckTxWindow: the concurrent-CheckTx accumulation
	// window (baseapp.CheckTxWindow; a lone request never waits).
	CheckTxWindowTxs int           `mapstructure:"checktx-window-txs"`
	CheckTxWindow    time.Duration `mapstructure:"checktx-window"`
	// PreVerifyBlocks: pre-verify each block before its DeliverTx loop
	// (baseapp.PreVerifyTxs) and, where blocks are known ahead, the next one
	// beside it (PreVerifyAhead).
	PreVerifyBlocks bool `mapstructure:"preverify-blocks"`
}

// DefaultGPUVerifyConfig: off by default (a node opts in), the library's own
// defaults otherwise (include/gpuverify.h: GV_CPU_CROSSOVER, GV_KEY_LOAD_MIN,
// GV_KEY_CAP, GV_ED_KEY_CAP; the CheckTx window of the C++ mirror).
func DefaultGPUVerifyConfig() GPUVerifyConfig {
	return GPUVerifyConfig{
		Enable: false, Devices: "", MaxBatch: 1 << 20, CPUBelow: 4, Keyed: true, KeyLoadMin: 4096,
		KeyCap: 1 << 22, EdKeyCap: 1 << 16, KeyResident: 0, EdKeyResident: 0, KeysWideQW: 0, EdKeysWide: 0, KeysIndex: false, KeysIndexSplit: 0, EdKeysIndex: false, CacheEntries: 1 << 20,
		CheckTxWindowTxs: 64, CheckTxWindow: 200 * time.Microsecond, PreVerifyBlocks: true,
	}
}

// DeviceIDs parses Devices (nil = every visible device).
func (c GPUVerifyConfig) DeviceIDs() ([]int, error) {
	if strings.TrimSpace(c.Devices) == "" {
		return nil, nil
	}
	var ids []int
	for _, f := range strings.Split(c.Devices, ",") {
		id, err := strconv.Atoi(strings.TrimSpace(f))
		if err != nil || id < 0 {
			return nil, fmt.Errorf("gpu-verify.devices: bad device id %q", f)
		}
		ids = append(ids, id)
	}
	return ids, nil
}

// Validate rejects values the library would refuse.
func (c GPUVerifyConfig) Validate() error {
	if _, err := c.DeviceIDs(); err != nil {
		return err
	}
	switch {
	case c.MaxBatch < 256:
		return fmt.Errorf("gpu-verify.max-batch must be >= 256, got %d", c.MaxBatch)
	case c.CPUBelow < 0, c.KeyLoadMin < 1, c.KeyCap < 1, c.EdKeyCap < 1, c.CacheEntries < 0:
		return fmt.Errorf("gpu-verify: negative or zero size in %+v", c)
	case c.KeyResident < 0 || c.KeyResident > c.KeyCap:
		return fmt.Errorf("gpu-verify.key-resident must be 0 (off) or at most key-cap, got %d", c.KeyResident)
	case c.EdKeyResident < 0 || c.EdKeyResident > c.EdKeyCap:
		return fmt.Errorf("gpu-verify.ed-key-resident must be 0 (off) or at most ed-key-cap, got %d", c.EdKeyResident)
	case c.KeysWideQW != 0 && c.KeysWideQW != 9 && c.KeysWideQW != 11:
		return fmt.Errorf("gpu-verify.keys-wide-qw must be 0, 9 or 11, got %d", c.KeysWideQW)
	case c.EdKeysWide != 0 && c.EdKeysWide != 6 && c.EdKeysWide != 8:
		return fmt.Errorf("gpu-verify.ed-keys-wide must be 0, 6 or 8, got %d", c.EdKeysWide)
	case c.KeysIndexSplit < 0:
		return fmt.Errorf("gpu-verify.keys-index-split must be >= 0, got %d", c.KeysIndexSplit)
	case c.CheckTxWindowTxs < 1 || c.CheckTxWindow < 0:
		return fmt.Errorf("gpu-verify: bad CheckTx window (%d txs, %v)", c.CheckTxWindowTxs, c.CheckTxWindow)
	}
	return nil
}

// GPUVerifyTemplate is the app.toml section (text/template over Config).
const GPUVerifyTemplate = `
###############################################################################
###                       GPU signature verification                        ###
###############################################################################

[gpu-verify]

# Route tx signature checks (x/auth ante, IBC commits) to the GPU verifier.
enable = {{ .GPUVerify.Enable }}

# HIP device ids, comma separated ("" = every visible device).
devices = "{{ .GPUVerify.Devices }}"

# Largest batch of one device call.
max-batch = {{ .GPUVerify.MaxBatch }}

# Batches with fewer signatures run on the CPU.
cpu-below = {{ .GPUVerify.CPUBelow }}

# Keep account keys parsed in GPU memory; loads only from key-load-min leaves.
keyed = {{ .GPUVerify.Keyed }}
key-load-min = {{ .GPUVerify.KeyLoadMin }}
key-cap = {{ .GPUVerify.KeyCap }}
ed-key-cap = {{ .GPUVerify.EdKeyCap }}

# Keep the account-key arena at this many keys, replacing the least recently
# used ones (0 = off: the arena grows to key-cap and is reset there).  65536
# keeps the fastest wide-table layout whatever the number of accounts seen.
key-resident = {{ .GPUVerify.KeyResident }}

# The same for the ed25519 arena (IBC validator sets, multisig ed25519
# sub-keys; 72 KiB of GPU memory per key): 0 = off, the arena grows to
# ed-key-cap and starts over there with every chain's keys dropped together.
ed-key-resident = {{ .GPUVerify.EdKeyResident }}

# Window width of the key arena's wide tables: 0 = 11-bit tables (768 / 384 KiB
# per key), then 9-bit ones (240 / 128 KiB) when those no longer fit; 11 or 9 =
# that width only.
keys-wide-qw = {{ .GPUVerify.KeysWideQW }}

# Wider comb tables of the ed25519 arena for large keyed batches: 0 = off (72 KiB
# per key), 6 = radix-64 tables beside them (194 KiB more per key), 8 = radix-256
# ones (576 KiB more).  Taken when the arena next starts from slot 0.
ed-keys-wide = {{ .GPUVerify.EdKeysWide }}

# Device-side index of the account-key arena (key bytes -> slot, 44 bytes of GPU
# memory per slot of capacity): pub33 batches staged on the GPU run on the
# resident tables when all their keys are resident.  Taken when the arena next
# starts from slot 0.
keys-index = {{ .GPUVerify.KeysIndex }}

# With keys-index: a batch with at most this many signatures whose keys are not
# resident still runs on the resident tables; those signatures are verified by
# their key bytes beside it (0 = one such signature sends the whole batch to
# the per-key route).  Same verdicts either way.
keys-index-split = {{ .GPUVerify.KeysIndexSplit }}

# Device-side index of the ed25519 key arena (32 key bytes -> slot, 8 bytes of
# GPU memory per slot of capacity): ed25519 batches staged on the GPU run on the
# resident tables when all their keys are resident.  Taken when the arena next
# starts from slot 0.
ed-keys-index = {{ .GPUVerify.EdKeysIndex }}

# Verdict cache entries (0 disables it).
cache-entries = {{ .GPUVerify.CacheEntries }}

# Concurrent CheckTx requests are pre-verified together: up to this many
# txs or this long after the first (a lone request never waits).
checktx-window-txs = {{ .GPUVerify.CheckTxWindowTxs }}
checktx-window = "{{ .GPUVerify.CheckTxWindow }}"

# Pre-verify each block before its DeliverTx loop.
preverify-blocks = {{ .GPUVerify.PreVerifyBlocks }}
`
