"""gpuverify.py -- ctypes binding of libgpuverify.so (include/gpuverify.h).

Host-side mirror of the reference's verification interface for tests and the
benchmark (the reference's own host language, Go, has no toolchain in this
image; INTEGRATION.md carries the cgo binding).  Names follow the reference:

  PubKeySecp256k1(pub33).verify_bytes(msg, sig)   tendermint VerifyBytes
                                                  (x/auth/ante/sigverify.go:210)
  Verifier.verify_batch_msgs / verify_batch_digests   batched VerifyBytes
                                                  (crypto/gpuverify in INTEGRATION.md)

This module never falls back to a CPU implementation: if libgpuverify.so is
missing or no HIP device is present it raises GpuVerifyError.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# GV_LIB overrides the library path (A/B runs of alternative builds); the default
# is the in-tree build.
# defaults of the "lat_max" / "lat_sl_max" options (gv_runtime.cpp): the small-batch / pipeline
# crossover and the sliced / four-lanes-per-signature small-batch crossover
LAT_MAX_DEFAULT = 8192
LAT_SL_MAX_DEFAULT = 2048
LAT_ROWS_MAX_DEFAULT = 512        # pub33 batches up to this many: k_verify_lat_sl4 ("lat_rows_max")
# keyed batches: their own defaults (setting "lat_max" / "lat_sl_max" sets the keyed ones too)
LAT_MAX_KEYED_DEFAULT = 14336
LAT_SL_MAX_KEYED_DEFAULT = 1536
LIB_PATH = os.environ.get("GV_LIB") or os.path.join(HERE, "lib", "libgpuverify.so")

GV_OK, GV_EINVAL, GV_ENODEV, GV_EHIP, GV_ENOMEM, GV_EFAULT = 0, -1, -2, -3, -4, -5

# every symbol include/gpuverify.h declares
EXPORTED_SYMBOLS = (
    "gv_open", "gv_close", "gv_num_devices", "gv_verify_msgs", "gv_verify_digests",
    "gv_verify_digests_bits", "gv_verify_msgs_bits", "gv_dev_verify_digests", "gv_dev_verify_msgs",
    "gv_set_option", "gv_get_option", "gv_last_stage_ms", "gv_strerror", "gv_debug_op", "gv_dev_alloc", "gv_dev_free",
    "gv_dev_copy", "gv_dev_sync", "gv_stage_stats", "gv_keys_load", "gv_keys_reset", "gv_keys_count", "gv_keys_generation",
    "gv_verify_digests_keyed", "gv_verify_msgs_keyed", "gv_dev_verify_digests_keyed", "gv_stage_stats4",
    "gv_keys_point", "gv_keys_replace", "gv_dev_stream_create", "gv_dev_stream_sync", "gv_dev_stream_destroy",
    "gv_verify_ed25519_msgs", "gv_dev_verify_ed25519_msgs", "gv_last_slices", "gv_group_stats", "gv_route_stats", "gv_host_alloc", "gv_host_free",
    "gv_ed_keys_load", "gv_ed_keys_reset", "gv_ed_keys_count", "gv_ed_keys_generation", "gv_verify_ed25519_msgs_keyed",
    "gv_ed_keys_replace", "gv_ed_keys_point", "gv_dev_verify_ed25519_msgs_keyed", "gv_ed_keys_wide_point",
    "gv_submit_digests", "gv_submit_digests_keyed", "gv_submit_msgs", "gv_submit_msgs_keyed", "gv_wait",
    "gv_keys_find", "gv_dev_keys_find", "gv_debug_sl_op", "gv_keys_entry", "gv_group_entry",
    "gv_ed_keys_find", "gv_dev_ed_keys_find", "gv_debug_lane_op",
)

# gv_debug_sl_op (csrc/gv_kernels.h): words per item, flags, status words, op codes
SL_IN, SL_OUT = 80, 80
SLF_NEG, SLF_PRE, SLF_INF_A, SLF_INF_B, SLF_WORDS = 1, 2, 4, 8, 16
SLS_FLAG, SLS_INF, SLS_ROWS, SLS_KNOWN = 0, 1, 2, 3
SLOP = {name: i for i, name in enumerate((
    "mul", "sqr", "mul_plus8", "mul_plusb", "mul2", "norm", "sub", "neg", "is_zero", "from_words", "load_words",
    "to_words", "sqrt", "rows_all", "gjsl_double", "gjsl_add_scaled", "gjsl_add_gej", "gj4_double", "gj4_add",
    "gj4_add_gej", "gj4_add_affine", "modinv"))}
SLOP.update({name: 64 + i for i, name in enumerate((
    "ed_mul", "ed_sqr", "ed_norm", "ed_sub", "ed_is_zero", "ed_to_words", "ed_from_words", "ed_pow22523",
    "ed_decode_strict", "ed_decode_lenient", "gesl_add_cached", "gesl_add_pre", "gesl_add", "ge4_double",
    "ge4_add_cached", "ge4_add", "ed_digits"))})

# gv_debug_lane_op (csrc/gv_lane.h): the item layout of gv_debug_sl_op; secp256k1 op c runs in the
# one-chain unit, c + LNOP_LAT in the two-chain unit
LN_IN, LN_OUT = 80, 80
LNF_NEG, LNF_NOT, LNF_INF_A, LNF_INF_B, LNF_WORDS, LNF_ENTRY_SHIFT = 1, 2, 4, 8, 16, 8
LNS_FLAG, LNS_INF, LNS_KNOWN = 0, 1, 3
LNOP_LAT = 64
LNOP = {name: i for i, name in enumerate((
    "mul", "sqr", "multi_ss", "multi_mmm", "multi_mm", "multi_ssm", "sub1", "neg1", "sub_norm1", "sub_norm2",
    "sub_norm3", "shl_norm1", "shl_norm2", "shl_norm3", "mul3_norm", "norm", "to_words", "from_words", "is_zero",
    "is_zero_fast", "equal", "inv", "sqrt", "x_mul", "x_mul_p1", "x_mul_p8", "x_mul2", "x_sqr", "x_sqrd_p1",
    "x_sqrd_p8", "x_sqr3", "x_sqrt", "gej_double", "gej_add_ge", "gej_add_gej", "gejx_double", "gejx_add_scaled"))}
LNOP_SECP_END = len(LNOP)
LNOP.update({name: 128 + i for i, name in enumerate((
    "ed_mul", "ed_sqr", "ed_sub1", "ed_neg1", "ed_sub_norm1", "ed_sub_norm2", "ed_sub_norm3", "ed_add_norm", "ed_norm",
    "ed_to_words", "ed_from_words", "ed_is_zero", "ed_is_negative", "ed_inv", "ed_pow22523", "ge_dbl_t", "ge_dbl_nt",
    "ge_add_cached", "ge_add_pre", "ge_to_cached", "ge_to_pre", "ge_neg", "ge_frombytes", "ge_tobytes", "ge_add_tab",
    "sc_reduce512", "sc_minimal", "ed_radix16", "ed_comb4", "ed_comb6", "ed_comb8"))})
LNOP_ED_END = 128 + len(LNOP) - LNOP_SECP_END


class GpuVerifyError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        msg = _strerror(code) if _lib is not None else str(code)
        super().__init__(f"{what}: {msg} ({code})" if what else f"{msg} ({code})")


_lib = None


def build() -> str:
    subprocess.run(["make", "-s", "-C", HERE], check=True)
    return LIB_PATH


def load(path: str = LIB_PATH):
    """Load libgpuverify.so and declare argtypes.  Does not touch the GPU."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise GpuVerifyError(GV_ENODEV, f"{path} not built (run make -C {HERE})")
    L = ctypes.CDLL(path)
    vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.gv_open.argtypes = [ctypes.POINTER(i32), i32, ctypes.POINTER(vp)]
    L.gv_open.restype = i32
    L.gv_close.argtypes = [vp]
    L.gv_close.restype = None
    L.gv_num_devices.argtypes = [vp]
    L.gv_num_devices.restype = i32
    L.gv_verify_msgs.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    L.gv_verify_msgs.restype = i32
    L.gv_verify_digests.argtypes = [vp, sz, vp, vp, vp, vp]
    L.gv_verify_digests.restype = i32
    L.gv_verify_digests_bits.argtypes = [vp, sz, vp, vp, vp, vp]
    L.gv_verify_digests_bits.restype = i32
    L.gv_verify_msgs_bits.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    L.gv_verify_msgs_bits.restype = i32
    L.gv_dev_verify_digests.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp]
    L.gv_dev_verify_digests.restype = i32
    L.gv_dev_verify_msgs.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp, vp, vp]
    L.gv_dev_verify_msgs.restype = i32
    L.gv_verify_ed25519_msgs.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    L.gv_verify_ed25519_msgs.restype = i32
    L.gv_dev_verify_ed25519_msgs.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp, vp, vp]
    L.gv_dev_verify_ed25519_msgs.restype = i32
    L.gv_ed_keys_load.argtypes = [vp, sz, vp, vp]
    L.gv_ed_keys_load.restype = i32
    L.gv_ed_keys_reset.argtypes = [vp]
    L.gv_ed_keys_reset.restype = i32
    L.gv_ed_keys_count.argtypes = [vp]
    L.gv_ed_keys_count.restype = sz
    L.gv_ed_keys_generation.argtypes = [vp]
    L.gv_ed_keys_generation.restype = ctypes.c_uint64
    L.gv_ed_keys_replace.argtypes = [vp, sz, vp, vp]
    L.gv_ed_keys_replace.restype = i32
    L.gv_ed_keys_point.argtypes = [vp, sz, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp]
    L.gv_ed_keys_point.restype = i32
    L.gv_verify_ed25519_msgs_keyed.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    L.gv_verify_ed25519_msgs_keyed.restype = i32
    L.gv_dev_verify_ed25519_msgs_keyed.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp, vp, vp]
    L.gv_dev_verify_ed25519_msgs_keyed.restype = i32
    L.gv_ed_keys_wide_point.argtypes = [vp, sz, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    L.gv_ed_keys_wide_point.restype = i32
    L.gv_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_longlong]
    L.gv_set_option.restype = i32
    L.gv_get_option.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_longlong)]
    L.gv_get_option.restype = i32
    L.gv_last_stage_ms.argtypes = [vp, i32] + [ctypes.POINTER(ctypes.c_float)] * 3
    L.gv_last_stage_ms.restype = i32
    L.gv_strerror.argtypes = [i32]
    L.gv_strerror.restype = ctypes.c_char_p
    L.gv_debug_op.argtypes = [vp, i32, i32, sz, vp, vp]
    L.gv_debug_op.restype = i32
    L.gv_debug_sl_op.argtypes = [vp, i32, i32, sz, vp, vp]
    L.gv_debug_sl_op.restype = i32
    L.gv_debug_lane_op.argtypes = [vp, i32, i32, sz, vp, vp]
    L.gv_debug_lane_op.restype = i32
    L.gv_dev_alloc.argtypes = [vp, i32, sz, ctypes.POINTER(vp)]
    L.gv_dev_alloc.restype = i32
    L.gv_dev_free.argtypes = [vp, i32, vp]
    L.gv_dev_free.restype = i32
    L.gv_dev_copy.argtypes = [vp, i32, vp, vp, sz, i32]
    L.gv_dev_copy.restype = i32
    L.gv_dev_sync.argtypes = [vp, i32]
    L.gv_dev_sync.restype = i32
    L.gv_dev_stream_create.argtypes = [vp, i32, ctypes.POINTER(vp)]
    L.gv_dev_stream_create.restype = i32
    L.gv_dev_stream_sync.argtypes = [vp, i32, vp]
    L.gv_dev_stream_sync.restype = i32
    L.gv_dev_stream_destroy.argtypes = [vp, i32, vp]
    L.gv_dev_stream_destroy.restype = i32
    L.gv_stage_stats.argtypes = [vp, i32, ctypes.POINTER(i32)] + [ctypes.POINTER(ctypes.c_double)] * 3
    L.gv_stage_stats.restype = i32
    L.gv_stage_stats4.argtypes = [vp, i32, ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_double)]
    L.gv_stage_stats4.restype = i32
    L.gv_last_slices.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_size_t), i32]
    L.gv_last_slices.restype = i32
    L.gv_group_stats.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.gv_group_stats.restype = i32
    L.gv_route_stats.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_uint64)]
    L.gv_route_stats.restype = i32
    L.gv_host_alloc.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
    L.gv_host_alloc.restype = i32
    L.gv_host_free.argtypes = [vp, vp]
    L.gv_host_free.restype = i32
    L.gv_keys_load.argtypes = [vp, sz, vp, vp]
    L.gv_keys_load.restype = i32
    L.gv_keys_reset.argtypes = [vp]
    L.gv_keys_reset.restype = i32
    L.gv_keys_count.argtypes = [vp]
    L.gv_keys_count.restype = sz
    L.gv_keys_generation.argtypes = [vp]
    L.gv_keys_generation.restype = ctypes.c_uint64
    L.gv_keys_point.argtypes = [vp, sz, vp, vp, vp]
    L.gv_keys_point.restype = i32
    L.gv_keys_replace.argtypes = [vp, sz, vp, vp]
    L.gv_keys_replace.restype = i32
    # (as the pubkey index below: a library from before the entry readback lacks them)
    for name, args in (("gv_keys_entry", [vp, i32, i32, sz, vp, vp, vp, vp, vp]),
                       ("gv_group_entry", [vp, i32, i32, sz, vp, vp, vp, vp, vp, vp])):
        if hasattr(L, name):
            getattr(L, name).argtypes = args
            getattr(L, name).restype = i32
    # (a library from before the pubkey index, loaded through GV_LIB for an A/B
    # run, lacks these two: the wrappers then raise AttributeError when called)
    for name, args in (("gv_keys_find", [vp, sz, vp, vp]), ("gv_dev_keys_find", [vp, i32, sz, vp, vp, vp]),
                       ("gv_ed_keys_find", [vp, sz, vp, vp]), ("gv_dev_ed_keys_find", [vp, i32, sz, vp, vp, vp])):
        if hasattr(L, name):
            getattr(L, name).argtypes = args
            getattr(L, name).restype = i32
    L.gv_verify_digests_keyed.argtypes = [vp, sz, vp, vp, vp, vp]
    L.gv_verify_digests_keyed.restype = i32
    L.gv_verify_msgs_keyed.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    L.gv_verify_msgs_keyed.restype = i32
    L.gv_dev_verify_digests_keyed.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp]
    L.gv_dev_verify_digests_keyed.restype = i32
    u64p = ctypes.POINTER(ctypes.c_uint64)
    for name, nargs in (("gv_submit_digests", 4), ("gv_submit_digests_keyed", 4), ("gv_submit_msgs", 6),
                        ("gv_submit_msgs_keyed", 6)):
        getattr(L, name).argtypes = [vp, sz] + [vp] * nargs + [u64p]
        getattr(L, name).restype = i32
    L.gv_wait.argtypes = [vp, ctypes.c_uint64]
    L.gv_wait.restype = i32
    _lib = L
    return L


def _strerror(code: int) -> str:
    return _lib.gv_strerror(code).decode()


def _ptr(a: np.ndarray):
    assert a.flags["C_CONTIGUOUS"]
    return ctypes.c_void_p(a.ctypes.data)


def _check(rc: int, what: str):
    if rc != GV_OK:
        raise GpuVerifyError(rc, what)


def pack_msgs(msgs):
    """list[bytes] -> (blob u8, off u64, len u32)"""
    lens = np.fromiter((len(m) for m in msgs), dtype=np.uint32, count=len(msgs))
    off = np.zeros(len(msgs), dtype=np.uint64)
    if len(msgs) > 1:
        off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    blob = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy()
    return blob, off, lens


class Verifier:
    """Batched VerifyBytes on one or more MI355X devices (gv_ctx)."""

    def __init__(self, devices=None):
        L = load()
        ctx = ctypes.c_void_p()
        if devices:
            ids = (ctypes.c_int * len(devices))(*devices)
            rc = L.gv_open(ids, len(devices), ctypes.byref(ctx))
        else:
            rc = L.gv_open(None, 0, ctypes.byref(ctx))
        _check(rc, "gv_open")
        self._ctx = ctx
        self._L = L
        # submitted batches not yet waited for: ticket -> (input arrays, verdicts).
        # The library reads the inputs and writes the verdicts until gv_wait, so
        # they live here, not only in the Pending the caller may drop.
        self._inflight = {}

    def close(self):
        if self._ctx:
            for t in list(self._inflight):        # the lanes use these buffers until each batch is done
                self._release(t)
            self._L.gv_close(self._ctx)
            self._ctx = None

    def _release(self, ticket) -> int:
        """gv_wait on a ticket still in flight (a dropped Pending, close()); 0 if already waited."""
        if ticket not in self._inflight or not self._ctx:
            return 0
        rc = self._L.gv_wait(self._ctx, ticket)
        self._inflight.pop(ticket, None)
        return rc

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def num_devices(self) -> int:
        return self._L.gv_num_devices(self._ctx)

    def reset_schedule(self):
        """The small-batch schedule options back to their defaults."""
        self.set_option("lat_max", LAT_MAX_DEFAULT)
        self.set_option("lat_sl_max", LAT_SL_MAX_DEFAULT)
        self.set_option("lat_max_keyed", LAT_MAX_KEYED_DEFAULT)
        self.set_option("lat_sl_max_keyed", LAT_SL_MAX_KEYED_DEFAULT)
        self.set_option("lat_rows_max", LAT_ROWS_MAX_DEFAULT)

    def set_option(self, key: str, val: int):
        _check(self._L.gv_set_option(self._ctx, key.encode(), int(val)), f"gv_set_option({key})")

    def get_option(self, key: str) -> int:
        """gv_get_option: a readable tunable or a read-only live value (include/gpuverify.h lists
        them), e.g. "ed_kw_rb" (the wide ed25519 arena's radix bits), "ed_keyed_wide" (keyed
        ed25519 batches on wide tables) or "ed_btab16_live" (1 when the first device holds a
        built radix-2^16 comb table of B; 0 before the first call that uses it, or when its
        allocation or build failed and [s]B comes from the radix-256 table; never builds it)."""
        v = ctypes.c_longlong(0)
        _check(self._L.gv_get_option(self._ctx, key.encode(), ctypes.byref(v)), f"gv_get_option({key})")
        return int(v.value)

    def verify_batch_digests(self, pub33: np.ndarray, sig64: np.ndarray, dig32: np.ndarray) -> np.ndarray:
        pub33, sig64, dig32 = (np.ascontiguousarray(a, dtype=np.uint8) for a in (pub33, sig64, dig32))
        n = pub33.shape[0]
        assert pub33.shape == (n, 33) and sig64.shape == (n, 64) and dig32.shape == (n, 32)
        out = np.zeros(n, dtype=np.uint8)
        if n:
            _check(self._L.gv_verify_digests(self._ctx, n, _ptr(pub33), _ptr(sig64), _ptr(dig32), _ptr(out)),
                   "gv_verify_digests")
        return out

    def verify_batch_digests_bits(self, pub33, sig64, dig32) -> np.ndarray:
        n = pub33.shape[0]
        out = np.zeros((n + 63) // 64, dtype=np.uint64)
        if n:
            _check(self._L.gv_verify_digests_bits(self._ctx, n, _ptr(pub33), _ptr(sig64), _ptr(dig32),
                                                  _ptr(out)), "gv_verify_digests_bits")
        return out

    def verify_batch_msgs(self, pub33: np.ndarray, sig64: np.ndarray, msgs) -> np.ndarray:
        """msgs: list[bytes] or a (blob, off, len) triple."""
        pub33, sig64 = (np.ascontiguousarray(a, dtype=np.uint8) for a in (pub33, sig64))
        blob, off, ln = pack_msgs(msgs) if isinstance(msgs, (list, tuple)) and (
            len(msgs) == 0 or isinstance(msgs[0], (bytes, bytearray))) else msgs
        n = pub33.shape[0]
        out = np.zeros(n, dtype=np.uint8)
        if n:
            _check(self._L.gv_verify_msgs(self._ctx, n, _ptr(pub33), _ptr(sig64), _ptr(blob), _ptr(off),
                                          _ptr(ln), _ptr(out)), "gv_verify_msgs")
        return out

    # ---- asynchronous host batches (gv_submit_* / gv_wait)
    class Pending:
        """A submitted batch: its ticket and verdict array.  The Verifier keeps
        the input arrays (and the verdicts) alive until the batch is waited for;
        a Pending dropped without wait() is waited for when it is collected, so
        the library never touches freed memory."""
        def __init__(self, ticket, out):
            self.ticket, self.out = ticket, out

    def _submit(self, fn, name, n, args, keep):
        out = np.zeros(n, dtype=np.uint8)
        t = ctypes.c_uint64(0)
        _check(fn(self._ctx, n, *[_ptr(a) for a in args], _ptr(out), ctypes.byref(t)), name)
        self._inflight[t.value] = (keep, out)
        p = Verifier.Pending(t.value, out)
        weakref.finalize(p, self._release, t.value)
        return p

    def submit_digests(self, pub33, sig64, dig32) -> "Verifier.Pending":
        a = [np.ascontiguousarray(x, dtype=np.uint8) for x in (pub33, sig64, dig32)]
        return self._submit(self._L.gv_submit_digests, "gv_submit_digests", a[0].shape[0], a, a)

    def submit_digests_keyed(self, slots, sig64, dig32) -> "Verifier.Pending":
        a = [np.ascontiguousarray(slots, dtype=np.uint32)] + [np.ascontiguousarray(x, dtype=np.uint8)
                                                             for x in (sig64, dig32)]
        return self._submit(self._L.gv_submit_digests_keyed, "gv_submit_digests_keyed", a[0].shape[0], a, a)

    def submit_msgs(self, pub33, sig64, msgs, slots=None) -> "Verifier.Pending":
        blob, off, ln = pack_msgs(msgs) if isinstance(msgs, (list, tuple)) and (
            len(msgs) == 0 or isinstance(msgs[0], (bytes, bytearray))) else msgs
        sig64 = np.ascontiguousarray(sig64, dtype=np.uint8)
        if slots is not None:
            k = np.ascontiguousarray(slots, dtype=np.uint32)
            a = [k, sig64, blob, off, ln]
            return self._submit(self._L.gv_submit_msgs_keyed, "gv_submit_msgs_keyed", k.shape[0], a, a)
        p = np.ascontiguousarray(pub33, dtype=np.uint8)
        a = [p, sig64, blob, off, ln]
        return self._submit(self._L.gv_submit_msgs, "gv_submit_msgs", p.shape[0], a, a)

    def wait(self, pending: "Verifier.Pending") -> np.ndarray:
        if pending.ticket not in self._inflight:
            raise GpuVerifyError(GV_EINVAL, "gv_wait: ticket already waited for")
        rc = self._L.gv_wait(self._ctx, pending.ticket)
        self._inflight.pop(pending.ticket, None)
        _check(rc, "gv_wait")
        return pending.out

    # ---- account pubkey cache (gv_keys_*)
    def keys_load(self, pub33: np.ndarray) -> np.ndarray:
        """Parse and keep n keys resident; returns their slots (u32)."""
        pub33 = np.ascontiguousarray(pub33, dtype=np.uint8)
        n = pub33.shape[0]
        assert pub33.shape == (n, 33)
        slots = np.zeros(n, dtype=np.uint32)
        if n:
            _check(self._L.gv_keys_load(self._ctx, n, _ptr(pub33), _ptr(slots)), "gv_keys_load")
        return slots

    def keys_point(self, slots: np.ndarray):
        """Affine points (n x 64 bytes x||y) and ParsePubKey verdicts the key arena holds for `slots`."""
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        n = slots.shape[0]
        xy = np.zeros((n, 64), dtype=np.uint8)
        ok = np.zeros(n, dtype=np.uint8)
        if n:
            _check(self._L.gv_keys_point(self._ctx, n, _ptr(slots), _ptr(xy), _ptr(ok)), "gv_keys_point")
        return xy, ok

    @staticmethod
    def _entry_triples(what: str, slots, groups, js):
        """The (slot, group, j) triples of an entry readback as three equal-length 1-d u32 arrays."""
        out = []
        for name, a in (("slots", slots), ("groups", groups), ("js", js)):
            a = np.asarray(a)
            if a.ndim != 1 or a.dtype.kind not in "ui" or (a.size and (a.min() < 0 or a.max() >= 2 ** 32)):
                raise ValueError(f"{what}: {name} must be a 1-d array of u32")
            out.append(a)
        if not out[0].shape == out[1].shape == out[2].shape:
            raise ValueError(f"{what}: {out[0].shape[0]} slots, {out[1].shape[0]} groups, {out[2].shape[0]} entries")
        return [np.ascontiguousarray(a, dtype=np.uint32) for a in out]

    def keys_entry(self, tabs: int, slots, groups, js, dev_slot: int = 0):
        """Key-table readback (gv_keys_entry): for each triple (slots[i], groups[i], js[i]) the affine
        point (n x 64 bytes x||y) entry js[i] of group groups[i] of the slot's table holds, and the
        slot's ParsePubKey verdict.  tabs: 0 the k4 tables, 1 the kn tables, 2 the wide tables in the
        arena's layout ("kw_arena_qw" / "kw_arena_ng"); dev_slot: whose arena."""
        for name, a in (("tabs", tabs), ("dev_slot", dev_slot)):
            if isinstance(a, bool) or not isinstance(a, (int, np.integer)):
                raise ValueError(f"keys_entry: {name} must be an integer")
        slots, groups, js = self._entry_triples("keys_entry", slots, groups, js)
        n = slots.shape[0]
        xy = np.zeros((n, 64), dtype=np.uint8)
        ok = np.zeros(n, dtype=np.uint8)
        if n:
            _check(self._L.gv_keys_entry(self._ctx, int(dev_slot), int(tabs), n, _ptr(slots), _ptr(groups), _ptr(js),
                                         _ptr(xy), _ptr(ok)), "gv_keys_entry")
        return xy, ok

    def group_entry(self, set_index: int, rows, groups, js, dev_slot: int = 0):
        """Grouped-set readback (gv_group_entry): for each triple (rows[i], groups[i], js[i]) of the
        key tables scratch set set_index keeps across calls (0 / 1: device-resident calls, 2 / 3:
        host slices) the 33 key bytes the row was built from (n x 33), the entry's affine point
        (n x 64) and the key's ParsePubKey verdict."""
        for name, a in (("set_index", set_index), ("dev_slot", dev_slot)):
            if isinstance(a, bool) or not isinstance(a, (int, np.integer)):
                raise ValueError(f"group_entry: {name} must be an integer")
        rows, groups, js = self._entry_triples("group_entry", rows, groups, js)
        n = rows.shape[0]
        key = np.zeros((n, 33), dtype=np.uint8)
        xy = np.zeros((n, 64), dtype=np.uint8)
        ok = np.zeros(n, dtype=np.uint8)
        if n:
            _check(self._L.gv_group_entry(self._ctx, int(dev_slot), int(set_index), n, _ptr(rows), _ptr(groups),
                                          _ptr(js), _ptr(key), _ptr(xy), _ptr(ok)), "gv_group_entry")
        return key, xy, ok

    def keys_replace(self, slots: np.ndarray, pub33: np.ndarray):
        """Rebuild loaded slots in place: slot slots[i] then holds key pub33[i] as if it had been
        loaded there (keys_count, keys_generation and the arena's layout do not move: the caller
        keeps its own pubkey -> slot map right).  Slots must be loaded and distinct."""
        slots = np.ascontiguousarray(slots)
        pub33 = np.ascontiguousarray(pub33)
        if slots.ndim != 1 or slots.dtype.kind not in "ui" or (slots.size and (slots.min() < 0 or slots.max() >= 2 ** 32)):
            raise ValueError("keys_replace: slots must be a 1-d array of u32 slot numbers")
        if pub33.dtype != np.uint8 or pub33.ndim != 2 or pub33.shape[1] != 33:
            raise ValueError("keys_replace: pub33 must be an (n, 33) uint8 array")
        if pub33.shape[0] != slots.shape[0]:
            raise ValueError(f"keys_replace: {slots.shape[0]} slots for {pub33.shape[0]} keys")
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        n = slots.shape[0]
        if n:
            _check(self._L.gv_keys_replace(self._ctx, n, _ptr(slots), _ptr(pub33)), "gv_keys_replace")

    KEY_NOT_FOUND = 0xFFFFFFFF

    def keys_find(self, pub33: np.ndarray) -> np.ndarray:
        """The arena's pubkey index (option "keys_index"): for each (33,) key the lowest slot
        holding exactly those bytes, or KEY_NOT_FOUND.  GpuVerifyError(GV_EINVAL) when the
        context has no live index -- "cannot tell", not "not resident"."""
        pub33 = np.asarray(pub33)
        if pub33.dtype != np.uint8 or pub33.ndim != 2 or pub33.shape[1] != 33:
            raise ValueError("keys_find: pub33 must be an (n, 33) uint8 array")
        pub33 = np.ascontiguousarray(pub33)
        n = pub33.shape[0]
        slots = np.full(n, self.KEY_NOT_FOUND, dtype=np.uint32)
        if n:
            _check(self._L.gv_keys_find(self._ctx, n, _ptr(pub33), _ptr(slots)), "gv_keys_find")
        return slots

    def dev_keys_find(self, slot: int, n: int, d_pub, d_slots_out, stream=None):
        """Device-resident keys_find on device slot `slot`: d_pub = n x 33 key bytes, d_slots_out =
        n u32 words (4-byte aligned) -- device addresses (ints); asynchronous on stream (a
        hipStream_t int; None: the library's).  The output feeds dev_verify_digests_keyed."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
            raise ValueError("dev_keys_find: n must be a non-negative integer")
        if isinstance(slot, bool) or not isinstance(slot, (int, np.integer)):
            raise ValueError("dev_keys_find: slot must be a device slot number")
        for name, a in (("d_pub", d_pub), ("d_slots_out", d_slots_out), ("stream", stream)):
            if a is not None and (isinstance(a, bool) or not isinstance(a, (int, np.integer)) or a < 0):
                raise ValueError(f"dev_keys_find: {name} must be a device address (int)")
        if n == 0:
            return
        if not d_pub or not d_slots_out:
            raise ValueError("dev_keys_find: d_pub and d_slots_out must not be null")
        if d_slots_out & 3:
            raise ValueError("dev_keys_find: d_slots_out must be 4-byte aligned")
        _check(self._L.gv_dev_keys_find(self._ctx, int(slot), int(n), ctypes.c_void_p(d_pub),
                                        ctypes.c_void_p(d_slots_out), ctypes.c_void_p(stream or 0)),
               "gv_dev_keys_find")

    def keys_reset(self):
        _check(self._L.gv_keys_reset(self._ctx), "gv_keys_reset")

    @property
    def keys_count(self) -> int:
        return self._L.gv_keys_count(self._ctx)

    def keys_generation(self) -> int:
        return self._L.gv_keys_generation(self._ctx)

    def verify_batch_digests_keyed(self, slots: np.ndarray, sig64: np.ndarray, dig32: np.ndarray) -> np.ndarray:
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        sig64, dig32 = (np.ascontiguousarray(a, dtype=np.uint8) for a in (sig64, dig32))
        n = slots.shape[0]
        assert sig64.shape == (n, 64) and dig32.shape == (n, 32)
        out = np.zeros(n, dtype=np.uint8)
        if n:
            _check(self._L.gv_verify_digests_keyed(self._ctx, n, _ptr(slots), _ptr(sig64), _ptr(dig32), _ptr(out)),
                   "gv_verify_digests_keyed")
        return out

    def verify_batch_msgs_keyed(self, slots: np.ndarray, sig64: np.ndarray, msgs) -> np.ndarray:
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        sig64 = np.ascontiguousarray(sig64, dtype=np.uint8)
        blob, off, ln = pack_msgs(msgs) if isinstance(msgs, (list, tuple)) and (
            len(msgs) == 0 or isinstance(msgs[0], (bytes, bytearray))) else msgs
        n = slots.shape[0]
        out = np.zeros(n, dtype=np.uint8)
        if n:
            _check(self._L.gv_verify_msgs_keyed(self._ctx, n, _ptr(slots), _ptr(sig64), _ptr(blob), _ptr(off),
                                                _ptr(ln), _ptr(out)), "gv_verify_msgs_keyed")
        return out

    def dev_verify_digests_keyed(self, slot: int, n: int, d_slots, d_sig, d_dig, d_bits, stream=None):
        _check(self._L.gv_dev_verify_digests_keyed(self._ctx, slot, n, ctypes.c_void_p(d_slots),
                                                   ctypes.c_void_p(d_sig), ctypes.c_void_p(d_dig),
                                                   ctypes.c_void_p(d_bits), ctypes.c_void_p(stream or 0)),
               "gv_dev_verify_digests_keyed")

    def dev_verify_digests(self, slot: int, n: int, d_pub, d_sig, d_dig, d_bits, stream=None):
        """Device-resident path: d_* are device addresses (ints); stream a hipStream_t int."""
        _check(self._L.gv_dev_verify_digests(self._ctx, slot, n, ctypes.c_void_p(d_pub), ctypes.c_void_p(d_sig),
                                             ctypes.c_void_p(d_dig), ctypes.c_void_p(d_bits),
                                             ctypes.c_void_p(stream or 0)), "gv_dev_verify_digests")

    def dev_verify_msgs(self, slot: int, n: int, d_pub, d_sig, d_blob, d_off, d_len, d_bits, stream=None):
        _check(self._L.gv_dev_verify_msgs(self._ctx, slot, n, ctypes.c_void_p(d_pub), ctypes.c_void_p(d_sig),
                                          ctypes.c_void_p(d_blob), ctypes.c_void_p(d_off), ctypes.c_void_p(d_len),
                                          ctypes.c_void_p(d_bits), ctypes.c_void_p(stream or 0)),
               "gv_dev_verify_msgs")

    # ---- ed25519
    def verify_batch_ed25519(self, pub32: np.ndarray, sig64: np.ndarray, msgs) -> np.ndarray:
        """out[i] = PubKeyEd25519(pub32[i]).VerifyBytes(msg_i, sig64[i]); msgs: list[bytes] or
        a (blob, off, len) triple."""
        pub32, sig64 = (np.ascontiguousarray(a, dtype=np.uint8) for a in (pub32, sig64))
        blob, off, ln = pack_msgs(msgs) if isinstance(msgs, (list, tuple)) and (
            len(msgs) == 0 or isinstance(msgs[0], (bytes, bytearray))) else msgs
        n = pub32.shape[0]
        assert pub32.shape == (n, 32) and sig64.shape == (n, 64) and len(off) == n and len(ln) == n
        out = np.zeros(n, dtype=np.uint8)
        if n:
            _check(self._L.gv_verify_ed25519_msgs(self._ctx, n, _ptr(pub32), _ptr(sig64), _ptr(blob),
                                                  _ptr(np.ascontiguousarray(off, dtype=np.uint64)),
                                                  _ptr(np.ascontiguousarray(ln, dtype=np.uint32)), _ptr(out)),
                   "gv_verify_ed25519_msgs")
        return out

    def ed_keys_load(self, pub32: np.ndarray) -> np.ndarray:
        """FromBytes + the comb table of -A, kept resident per key; returns the slots (u32)."""
        pub32 = np.ascontiguousarray(pub32, dtype=np.uint8)
        n = pub32.shape[0]
        assert pub32.shape == (n, 32)
        slots = np.zeros(n, dtype=np.uint32)
        if n:
            _check(self._L.gv_ed_keys_load(self._ctx, n, _ptr(pub32), _ptr(slots)), "gv_ed_keys_load")
        return slots

    def ed_keys_replace(self, slots: np.ndarray, pub32: np.ndarray):
        """Rebuild loaded ed25519 slots in place: slot slots[i] then holds key pub32[i] as if it had
        been loaded there (ed_keys_count and ed_keys_generation do not move: the caller keeps its
        own pubkey -> slot map right).  Slots must be loaded and distinct."""
        slots = np.ascontiguousarray(slots)
        pub32 = np.ascontiguousarray(pub32)
        if slots.ndim != 1 or slots.dtype.kind not in "ui" or (slots.size and (slots.min() < 0 or slots.max() >= 2 ** 32)):
            raise ValueError("ed_keys_replace: slots must be a 1-d array of u32 slot numbers")
        if pub32.dtype != np.uint8 or pub32.ndim != 2 or pub32.shape[1] != 32:
            raise ValueError("ed_keys_replace: pub32 must be an (n, 32) uint8 array")
        if pub32.shape[0] != slots.shape[0]:
            raise ValueError(f"ed_keys_replace: {slots.shape[0]} slots for {pub32.shape[0]} keys")
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        n = slots.shape[0]
        if n:
            _check(self._L.gv_ed_keys_replace(self._ctx, n, _ptr(slots), _ptr(pub32)), "gv_ed_keys_replace")

    def ed_keys_point(self, slots: np.ndarray, w: int = 0, j: int = 1):
        """For `slots` of the ed25519 key arena: the encoding of table entry j * 16^w * (-A)
        (n x 32 bytes), the raw key bytes (n x 32) and the FromBytes verdicts."""
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        n = slots.shape[0]
        enc = np.zeros((n, 32), dtype=np.uint8)
        pub = np.zeros((n, 32), dtype=np.uint8)
        ok = np.zeros(n, dtype=np.uint8)
        if n:
            _check(self._L.gv_ed_keys_point(self._ctx, n, _ptr(slots), w, j, _ptr(enc), _ptr(pub), _ptr(ok)),
                   "gv_ed_keys_point")
        return enc, pub, ok

    def ed_keys_find(self, pub32: np.ndarray) -> np.ndarray:
        """The ed25519 arena's pubkey index (option "ed_keys_index"): for each (32,) key the
        lowest slot holding exactly those bytes, or KEY_NOT_FOUND.  GpuVerifyError(GV_EINVAL)
        when the context has no live index -- "cannot tell", not "not resident"."""
        pub32 = np.asarray(pub32)
        if pub32.dtype != np.uint8 or pub32.ndim != 2 or pub32.shape[1] != 32:
            raise ValueError("ed_keys_find: pub32 must be an (n, 32) uint8 array")
        pub32 = np.ascontiguousarray(pub32)
        n = pub32.shape[0]
        slots = np.full(n, self.KEY_NOT_FOUND, dtype=np.uint32)
        if n:
            _check(self._L.gv_ed_keys_find(self._ctx, n, _ptr(pub32), _ptr(slots)), "gv_ed_keys_find")
        return slots

    def dev_ed_keys_find(self, slot: int, n: int, d_pub, d_slots_out, stream=None):
        """Device-resident ed_keys_find on device slot `slot`: d_pub = n x 32 key bytes (any
        alignment), d_slots_out = n u32 words (4-byte aligned) -- device addresses (ints);
        asynchronous on stream (a hipStream_t int; None: the library's).  The output feeds
        dev_verify_ed25519_keyed."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
            raise ValueError("dev_ed_keys_find: n must be a non-negative integer")
        if isinstance(slot, bool) or not isinstance(slot, (int, np.integer)):
            raise ValueError("dev_ed_keys_find: slot must be a device slot number")
        for name, a in (("d_pub", d_pub), ("d_slots_out", d_slots_out), ("stream", stream)):
            if a is not None and (isinstance(a, bool) or not isinstance(a, (int, np.integer)) or a < 0):
                raise ValueError(f"dev_ed_keys_find: {name} must be a device address (int)")
        if n == 0:
            return
        if not d_pub or not d_slots_out:
            raise ValueError("dev_ed_keys_find: d_pub and d_slots_out must not be null")
        if d_slots_out & 3:
            raise ValueError("dev_ed_keys_find: d_slots_out must be 4-byte aligned")
        _check(self._L.gv_dev_ed_keys_find(self._ctx, int(slot), int(n), ctypes.c_void_p(d_pub),
                                           ctypes.c_void_p(d_slots_out), ctypes.c_void_p(stream or 0)),
               "gv_dev_ed_keys_find")

    def ed_keys_reset(self):
        _check(self._L.gv_ed_keys_reset(self._ctx), "gv_ed_keys_reset")

    @property
    def ed_keys_count(self) -> int:
        return self._L.gv_ed_keys_count(self._ctx)

    @property
    def ed_keys_generation(self) -> int:
        return self._L.gv_ed_keys_generation(self._ctx)

    def verify_batch_ed25519_keyed(self, slots: np.ndarray, sig64: np.ndarray, msgs) -> np.ndarray:
        """verify_batch_ed25519 with the key of each item given by its ed25519 key-arena slot."""
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        sig64 = np.ascontiguousarray(sig64, dtype=np.uint8)
        blob, off, ln = pack_msgs(msgs) if isinstance(msgs, (list, tuple)) and (
            len(msgs) == 0 or isinstance(msgs[0], (bytes, bytearray))) else msgs
        n = slots.shape[0]
        assert sig64.shape == (n, 64) and len(off) == n and len(ln) == n
        out = np.zeros(n, dtype=np.uint8)
        if n:
            _check(self._L.gv_verify_ed25519_msgs_keyed(self._ctx, n, _ptr(slots), _ptr(sig64), _ptr(blob),
                                                        _ptr(np.ascontiguousarray(off, dtype=np.uint64)),
                                                        _ptr(np.ascontiguousarray(ln, dtype=np.uint32)), _ptr(out)),
                   "gv_verify_ed25519_msgs_keyed")
        return out

    def dev_verify_ed25519(self, slot: int, n: int, d_pub, d_sig, d_blob, d_off, d_len, d_bits, stream=None):
        _check(self._L.gv_dev_verify_ed25519_msgs(self._ctx, slot, n, ctypes.c_void_p(d_pub), ctypes.c_void_p(d_sig),
                                                  ctypes.c_void_p(d_blob), ctypes.c_void_p(d_off),
                                                  ctypes.c_void_p(d_len), ctypes.c_void_p(d_bits),
                                                  ctypes.c_void_p(stream or 0)), "gv_dev_verify_ed25519_msgs")

    def dev_verify_ed25519_keyed(self, slot: int, n: int, d_slots, d_sig, d_blob, d_off, d_len, d_bits, stream=None):
        """Device-resident verify_batch_ed25519_keyed: d_* are device addresses (ints) on device
        slot `slot` -- d_slots n x u32, d_sig n x 64 (16-byte aligned), d_off u64 / d_len u32 per
        item, d_blob (0 when every length is 0) --, accept bits into d_bits ((n + 63) // 64 u64
        words); stream a hipStream_t int (None: the library's)."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
            raise ValueError("dev_verify_ed25519_keyed: n must be a non-negative integer")
        if isinstance(slot, bool) or not isinstance(slot, (int, np.integer)):
            raise ValueError("dev_verify_ed25519_keyed: slot must be a device slot number")
        for name, a in (("d_slots", d_slots), ("d_sig", d_sig), ("d_blob", d_blob), ("d_off", d_off),
                        ("d_len", d_len), ("d_bits", d_bits), ("stream", stream)):
            if a is not None and (isinstance(a, bool) or not isinstance(a, (int, np.integer)) or a < 0):
                raise ValueError(f"dev_verify_ed25519_keyed: {name} must be a device address (int)")
        if n == 0:
            return
        _check(self._L.gv_dev_verify_ed25519_msgs_keyed(self._ctx, int(slot), int(n), ctypes.c_void_p(d_slots or 0),
                                                        ctypes.c_void_p(d_sig or 0), ctypes.c_void_p(d_blob or 0),
                                                        ctypes.c_void_p(d_off or 0), ctypes.c_void_p(d_len or 0),
                                                        ctypes.c_void_p(d_bits or 0), ctypes.c_void_p(stream or 0)),
               "gv_dev_verify_ed25519_msgs_keyed")

    def ed_keys_wide_point(self, slots: np.ndarray, w: int = 0, j: int = 1):
        """For `slots` of the wide ed25519 arena (option "ed_keys_wide" 6 or 8): the encoding of
        table entry j * 2^(rb w) * (-A) (n x 32 bytes) and the FromBytes verdicts; rb, the
        windows and the entries per window are the arena's ("ed_kw_rb": 43 x 32 or 32 x 128)."""
        slots = np.ascontiguousarray(slots)
        if slots.ndim != 1 or slots.dtype.kind not in "ui" or (slots.size and (slots.min() < 0 or slots.max() >= 2 ** 32)):
            raise ValueError("ed_keys_wide_point: slots must be a 1-d array of u32 slot numbers")
        for name, a, lo, hi in (("w", w, 0, 42), ("j", j, 1, 128)):      # the widest ranges either radix has
            if isinstance(a, bool) or not isinstance(a, (int, np.integer)) or not lo <= a <= hi:
                raise ValueError(f"ed_keys_wide_point: {name} must be an integer in [{lo}, {hi}]")
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        n = slots.shape[0]
        enc = np.zeros((n, 32), dtype=np.uint8)
        ok = np.zeros(n, dtype=np.uint8)
        if n:
            _check(self._L.gv_ed_keys_wide_point(self._ctx, n, _ptr(slots), int(w), int(j), _ptr(enc), _ptr(ok)),
                   "gv_ed_keys_wide_point")
        return enc, ok

    def last_stage_ms(self, slot: int = 0):
        a, b, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        _check(self._L.gv_last_stage_ms(self._ctx, slot, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
               "gv_last_stage_ms")
        return a.value, b.value, c.value

    # ---- device memory helpers (no torch/HIP runtime needed on the caller side)
    def dev_alloc(self, nbytes: int, slot: int = 0) -> int:
        p = ctypes.c_void_p()
        _check(self._L.gv_dev_alloc(self._ctx, slot, nbytes, ctypes.byref(p)), "gv_dev_alloc")
        return p.value

    def dev_free(self, ptr: int, slot: int = 0):
        _check(self._L.gv_dev_free(self._ctx, slot, ctypes.c_void_p(ptr)), "gv_dev_free")

    def dev_upload(self, ptr: int, arr: np.ndarray, slot: int = 0):
        arr = np.ascontiguousarray(arr)
        _check(self._L.gv_dev_copy(self._ctx, slot, ctypes.c_void_p(ptr), _ptr(arr), arr.nbytes, 1), "gv_dev_copy")

    def dev_download(self, arr: np.ndarray, ptr: int, slot: int = 0):
        assert arr.flags["C_CONTIGUOUS"]
        _check(self._L.gv_dev_copy(self._ctx, slot, _ptr(arr), ctypes.c_void_p(ptr), arr.nbytes, 2), "gv_dev_copy")

    def dev_sync(self, slot: int = 0):
        _check(self._L.gv_dev_sync(self._ctx, slot), "gv_dev_sync")

    def stream_create(self, slot: int = 0) -> int:
        p = ctypes.c_void_p()
        _check(self._L.gv_dev_stream_create(self._ctx, slot, ctypes.byref(p)), "gv_dev_stream_create")
        return p.value

    def stream_sync(self, stream: int, slot: int = 0):
        _check(self._L.gv_dev_stream_sync(self._ctx, slot, ctypes.c_void_p(stream)), "gv_dev_stream_sync")

    def stream_destroy(self, stream: int, slot: int = 0):
        _check(self._L.gv_dev_stream_destroy(self._ctx, slot, ctypes.c_void_p(stream)), "gv_dev_stream_destroy")

    def stage_stats(self, slot: int = 0):
        c = ctypes.c_int()
        a, b, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _check(self._L.gv_stage_stats(self._ctx, slot, ctypes.byref(c), ctypes.byref(a), ctypes.byref(b),
                                      ctypes.byref(d)), "gv_stage_stats")
        return c.value, a.value, b.value, d.value

    def stage_stats4(self, slot: int = 0):
        """(count, [unpack/sha, scalar_inv, prep, ecmult] ms averaged over the launches since the last call)."""
        c = ctypes.c_int()
        ms = (ctypes.c_double * 4)()
        _check(self._L.gv_stage_stats4(self._ctx, slot, ctypes.byref(c), ms), "gv_stage_stats4")
        return c.value, list(ms)

    def host_array(self, shape, dtype=np.uint8):
        """A numpy array in pinned host memory (gv_host_alloc): host-buffer digest
        calls on such arrays skip the staging copy.  Freed with host_free(arr)."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = ctypes.c_void_p()
        _check(self._L.gv_host_alloc(self._ctx, max(1, nbytes), ctypes.byref(p)), "gv_host_alloc")
        buf = (ctypes.c_uint8 * max(1, nbytes)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=np.uint8, count=nbytes).view(dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def host_free(self, arr):
        p = self._pinned.pop(arr.ctypes.data)
        _check(self._L.gv_host_free(self._ctx, p), "gv_host_free")

    def group_stats(self, slot: int = 0):
        """(batches that took the in-batch key grouping, keys whose tables were built) on device slot;
        with "group_reuse" on, a key whose tables the scratch set still holds is not built again."""
        b, k = ctypes.c_uint64(), ctypes.c_uint64()
        _check(self._L.gv_group_stats(self._ctx, slot, ctypes.byref(b), ctypes.byref(k)), "gv_group_stats")
        return b.value, k.value

    KG_DEFAULT = 0         # gv_runtime.cpp gv_ctx::kg (the grouped route's default layout)
    ROUTES = ("pub33", "keyed125", "k4", "k6", "lat", "lat_keyed", "k4f", "item_f", "kn", "ed_lat", "kw", "kw2", "kg")

    def route_stats(self, slot: int = 0) -> dict:
        """Batches per secp256k1 schedule on device slot since open (gv_route_stats)."""
        out = (ctypes.c_uint64 * len(self.ROUTES))()
        _check(self._L.gv_route_stats(self._ctx, slot, out), "gv_route_stats")
        return dict(zip(self.ROUTES, (int(v) for v in out)))

    def last_slices(self):
        """[(ms, items)] per device slot: each device's slice of the last host-buffer call."""
        nd = self.num_devices
        ms = (ctypes.c_double * max(1, nd))()
        nn = (ctypes.c_size_t * max(1, nd))()
        m = self._L.gv_last_slices(self._ctx, ms, nn, nd)
        if m < 0:
            raise GpuVerifyError(m, "gv_last_slices")
        return [(ms[k], nn[k]) for k in range(m)]

    def debug_op(self, op: int, words: np.ndarray, slot: int = 0) -> np.ndarray:
        words = np.ascontiguousarray(words, dtype=np.uint32)
        n = words.shape[0]
        assert words.shape == (n, 16)
        out = np.zeros((n, 16), dtype=np.uint32)
        _check(self._L.gv_debug_op(self._ctx, slot, op, n, _ptr(words), _ptr(out)), "gv_debug_op")
        return out

    def debug_sl_op(self, op, words: np.ndarray, slot: int = 0) -> np.ndarray:
        """One row-sliced operation (SLOP name or code) per item: words n x SL_IN
        (operand j's raw limbs at 9j..9j+8, flags last) -> n x SL_OUT (four
        slots of row 0's sixteen lanes, then the status words)."""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        n = words.shape[0]
        assert words.shape == (n, SL_IN)
        out = np.zeros((n, SL_OUT), dtype=np.uint32)
        code = SLOP[op] if isinstance(op, str) else int(op)
        _check(self._L.gv_debug_sl_op(self._ctx, slot, code, n, _ptr(words), _ptr(out)), "gv_debug_sl_op")
        return out

    def debug_lane_op(self, op, words: np.ndarray, chains: int = 1, slot: int = 0) -> np.ndarray:
        """One function of the one-lane 9 x 29 layers (LNOP name or code) per
        item, one item per lane: words n x LN_IN -> n x LN_OUT, the layout of
        debug_sl_op.  chains = 2 runs a secp256k1 op (given by name) in the
        two-chain unit of the small-batch kernels."""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        n = words.shape[0]
        assert words.shape == (n, LN_IN) and chains in (1, 2)
        out = np.zeros((n, LN_OUT), dtype=np.uint32)
        code = LNOP[op] if isinstance(op, str) else int(op)
        if chains == 2:
            assert isinstance(op, str) and code < LNOP_SECP_END
            code += LNOP_LAT
        _check(self._L.gv_debug_lane_op(self._ctx, slot, code, n, _ptr(words), _ptr(out)), "gv_debug_lane_op")
        return out


class PubKeySecp256k1:
    """Mirror of tendermint crypto/secp256k1.PubKeySecp256k1 ([33]byte) whose
    VerifyBytes runs on the GPU (batch of one).  Same argument meaning and
    result: bool, never an exception for a cryptographic rejection."""

    _shared = None

    def __init__(self, pub33: bytes):
        assert len(pub33) == 33
        self.key = bytes(pub33)

    @classmethod
    def _verifier(cls):
        if cls._shared is None:
            cls._shared = Verifier()
        return cls._shared

    def verify_bytes(self, msg: bytes, sig: bytes) -> bool:
        if len(sig) != 64:          # VerifyBytes' first check, decided on the host
            return False
        pub = np.frombuffer(self.key, dtype=np.uint8).reshape(1, 33)
        s = np.frombuffer(bytes(sig), dtype=np.uint8).reshape(1, 64)
        return bool(self._verifier().verify_batch_msgs(pub, s, [bytes(msg)])[0])
