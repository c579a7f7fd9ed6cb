"""Which kernel schedule every entry point takes, against the record of the
commit before launch() took a descriptor and submit() one predicate
(tests/golden/route_matrix_parent.json): per case the delta of the 13
gv_route_stats counters and of "ed_keyed_wide", "keys_index_hit",
"keys_index_miss" and "keys_index_launches"; the verdicts of every case must
equal the oracle's.

The small-batch bounds are lowered (lat_max 256, lat_sl_max 64, lat_rows_max
32, ed_lat_max / ed_unc_lat_max 64, group_min / ed_group_min 256) so that n in
{1, 32, 33, 64, 65, 256, 257, 1000} crosses every threshold.  The items tile a
base set of 16 (16 distinct keys) whose first four are an invalid signature,
a high-S one, a key off the curve and -- keyed -- a slot nothing was loaded
into (a set of n >= 4 holds all four); per-item routes also run a set of one
item per distinct golden key (at n = 257 too many keys for in-batch grouping,
and not all of them resident: the index misses).  Axes: the entry points
(host digests / messages, pinned digests with lat_zero_copy 0 / 1, host
keyed, gv_submit_* + gv_wait, the device-resident calls with and without
keys_index and on a caller stream, the four ed25519 calls), the arena states (none, k4 only, kn, wide 1, wide 2,
lat_kw, ed_keys_wide 0 / 6 / 8, ed_keyed) and one schedule switch at a time.
GV_ROUTE_KEYED125 needs GV_KEYED_K4=0: a fresh child process.

GV_ROUTE_MATRIX_RECORD=path makes the module write the record instead of
comparing against it (run once on the parent commit's library)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (REPO, os.path.join(REPO, "cosmos-sdk-rootchain_amd"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gpuverify as gvm                     # noqa: E402
from golden_io import load_digest_vectors, load_msg_vectors   # noqa: E402
from oracle import ed25519_ref as ED        # noqa: E402
from oracle import oracle as O              # noqa: E402
from oracle import secp_ref as R            # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(HERE, "golden", "route_matrix_parent.json")
SIZES = (1, 32, 33, 64, 65, 256, 257, 1000)
BOUNDS = {"lat_max": 256, "lat_sl_max": 64, "lat_rows_max": 32, "ed_lat_max": 64, "ed_unc_lat_max": 64,
          "group_min": 256, "ed_group_min": 256}      # (lat_max / lat_sl_max set the keyed bounds too)
SWITCHES = {"gfull": 0, "gfull_item": 0, "k6": 1, "kg": 4, "group_keys": 0, "sort_keys": 0, "lat_sliced": 0,
            "pipeline_dev": 0, "two_ladders": 0}
EXTRA = ("ed_keyed_wide", "keys_index_hit", "keys_index_miss", "keys_index_launches")
UNLOADED = 5                                 # (past the arena's count) a slot nothing was loaded into


# ---------------------------------------------------------------- the inputs
def _secp_base():
    """16 items over 16 distinct keys, as messages (the digest is SHA-256 of
    the message): invalid signature, high-S, key off the curve, then valid."""
    pub, sig, msgs, ok, cats = load_msg_vectors()
    dpub, _, _, _, dcats = load_digest_vectors()
    seen, pick = set(), []
    for i in range(len(ok)):
        if cats[i] == "valid_msg" and pub[i].tobytes() not in seen:
            seen.add(pub[i].tobytes())
            pick.append(i)
    pick = pick[:16]
    assert len(pick) == 16
    p, s, m = pub[pick].copy(), sig[pick].copy(), [msgs[i] for i in pick]
    s[0, 40] ^= 1                                                    # an invalid signature
    hs = R.N - int.from_bytes(s[1, 32:].tobytes(), "big")             # the same signature with s' = n - s
    s[1, 32:] = np.frombuffer(hs.to_bytes(32, "big"), np.uint8)
    p[2] = dpub[dcats.index("x_nonresidue")]                         # no point has this x
    return p, s, m


def _ed_base():
    g = json.load(open(os.path.join(HERE, "golden", "ed25519_vectors.json")))["categories"]
    items = [g["wrong_msg"][0], g["s_ge_l"][0], g["pub_not_on_curve"][0]] + g["valid"][:13]
    pub = np.array([np.frombuffer(bytes.fromhex(v["pub"]), np.uint8) for v in items])
    sig = np.array([np.frombuffer(bytes.fromhex(v["sig"]), np.uint8) for v in items])
    return pub, sig, [bytes.fromhex(v["msg"]) for v in items]


class Data:
    """The base sets and their oracle verdicts, computed once."""

    def __init__(self):
        self.pub, self.sig, self.msgs = _secp_base()
        self.dig = np.array([np.frombuffer(hashlib.sha256(m).digest(), np.uint8) for m in self.msgs])
        blob, off, ln = gvm.pack_msgs(self.msgs)
        self.ok = O.verify_msgs(self.pub, self.sig, blob, off, ln)
        assert np.array_equal(self.ok, O.verify_digests(self.pub, self.sig, self.dig))
        assert not self.ok[:3].any() and self.ok[3:].all()
        self.okk = self.ok.copy()
        self.okk[3] = 0                                              # keyed: item 3 names an unloaded slot
        mp, ms, md, _, cats = load_digest_vectors()                  # one item per distinct key, the specials first
        pick, seen = [], set()

        def take(i):
            if mp[i].tobytes() in seen:
                return False
            seen.add(mp[i].tobytes())
            pick.append(i)
            return True
        for c in ("wrong_msg", "high_s", "x_nonresidue"):
            next(i for i in range(len(cats)) if cats[i] == c and take(i))
        for i in range(len(cats)):
            take(i)
        assert len(pick) > 100
        mp, ms, md = mp[pick], ms[pick], md[pick]
        self.many = (mp, ms, md, O.verify_digests(mp, ms, md, threads=4))
        assert not self.many[3][:3].any()
        self.epub, self.esig, self.emsgs = _ed_base()
        self.eok = np.array([ED.verify(bytes(p), m, bytes(s)) for p, s, m in zip(self.epub, self.esig, self.emsgs)],
                            np.uint8)
        assert not self.eok[:3].any() and self.eok[3:].all()
        self.eokk = self.eok.copy()
        self.eokk[3] = 0

    @staticmethod
    def tile(a, n):
        idx = np.arange(n) % len(a)
        return [a[i] for i in idx] if isinstance(a, list) else np.ascontiguousarray(a[idx])


# ---------------------------------------------------------------- the entry points
def _bits(v, d_bits, n):
    w = np.zeros((n + 63) // 64, np.uint64)
    v.dev_download(w, d_bits)
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n]


def _on_device(v, arrays, n, call, stream=False):
    """Upload, run call(ptrs..., d_bits, stream) and read the bitmap back."""
    ptrs = [v.dev_alloc(max(a.nbytes, 16)) for a in arrays] + [v.dev_alloc(((n + 63) // 64) * 8)]
    st = v.stream_create() if stream else None
    try:
        for p, a in zip(ptrs, arrays):
            if a.nbytes:
                v.dev_upload(p, a)
        call(*ptrs, st)
        if st:
            v.stream_sync(st)
        v.dev_sync()
        return _bits(v, ptrs[-1], n)
    finally:
        if st:
            v.stream_destroy(st)
        for p in ptrs:
            v.dev_free(p)


def _pinned(v, arrays, call):
    pin = [v.host_array(a.shape, a.dtype) for a in arrays]
    try:
        for p, a in zip(pin, arrays):
            p[...] = a
        return call(*pin)
    finally:
        for p in pin:
            v.host_free(p)


def run_entry(v, D, entry, n, slots=None, eslots=None):
    """One call of `entry` over n tiled items: (verdicts, expected)."""
    t = D.tile
    if entry.endswith("_many"):
        pub, sig, dig, ok = (t(a, n) for a in D.many)
        if entry == "host_dig_many":
            return v.verify_batch_digests(pub, sig, dig), ok
        return _on_device(v, [pub, sig, dig], n, lambda a, b, c, o, st: v.dev_verify_digests(0, n, a, b, c, o)), ok
    if entry.startswith("ed_"):
        pub, sig, msgs = t(D.epub, n), t(D.esig, n), t(D.emsgs, n)
        blob, off, ln = gvm.pack_msgs(msgs)
        sl = t(eslots, n) if eslots is not None else None
        if entry == "ed_host":
            return v.verify_batch_ed25519(pub, sig, msgs), t(D.eok, n)
        if entry == "ed_host_keyed":
            return v.verify_batch_ed25519_keyed(sl, sig, msgs), t(D.eokk, n)
        if entry == "ed_dev":
            return _on_device(v, [pub, sig, blob, off, ln], n,
                              lambda a, b, c, d, e, o, st: v.dev_verify_ed25519(0, n, a, b, c, d, e, o)), t(D.eok, n)
        assert entry == "ed_dev_keyed"
        return _on_device(v, [sl, sig, blob, off, ln], n,
                          lambda a, b, c, d, e, o, st: v.dev_verify_ed25519_keyed(0, n, a, b, c, d, e, o)), t(D.eokk, n)
    pub, sig, dig, msgs = t(D.pub, n), t(D.sig, n), t(D.dig, n), t(D.msgs, n)
    sl = t(slots, n) if slots is not None else None
    ok, okk = t(D.ok, n), t(D.okk, n)
    if entry == "host_dig":
        return v.verify_batch_digests(pub, sig, dig), ok
    if entry == "host_msg":
        return v.verify_batch_msgs(pub, sig, msgs), ok
    if entry == "pinned_dig":
        return _pinned(v, [pub, sig, dig], v.verify_batch_digests), ok
    if entry == "pinned_keyed":
        return _pinned(v, [sl, sig, dig], v.verify_batch_digests_keyed), okk
    if entry == "host_keyed":
        return v.verify_batch_digests_keyed(sl, sig, dig), okk
    if entry == "host_keyed_msg":
        return v.verify_batch_msgs_keyed(sl, sig, msgs), okk
    if entry == "submit_dig":
        return v.wait(v.submit_digests(pub, sig, dig)), ok
    if entry == "submit_msg":
        return v.wait(v.submit_msgs(pub, sig, msgs)), ok
    if entry == "submit_keyed":
        return v.wait(v.submit_digests_keyed(sl, sig, dig)), okk
    if entry == "submit_keyed_msg":
        return v.wait(v.submit_msgs(None, sig, msgs, slots=sl)), okk
    if entry == "dev_dig":
        return _on_device(v, [pub, sig, dig], n, lambda a, b, c, o, st: v.dev_verify_digests(0, n, a, b, c, o)), ok
    if entry == "dev_msg":
        blob, off, ln = gvm.pack_msgs(msgs)
        return _on_device(v, [pub, sig, blob, off, ln], n,
                          lambda a, b, c, d, e, o, st: v.dev_verify_msgs(0, n, a, b, c, d, e, o)), ok
    assert entry in ("dev_keyed", "dev_keyed_stream")
    return _on_device(v, [sl, sig, dig], n, lambda a, b, c, o, st: v.dev_verify_digests_keyed(0, n, a, b, c, o, st),
                      stream=entry == "dev_keyed_stream"), okk


# ---------------------------------------------------------------- the cases
def _counters(v):
    r = v.route_stats()
    return [r[k] for k in gvm.Verifier.ROUTES] + [v.get_option(k) for k in EXTRA]


class Matrix:
    def __init__(self, v, D):
        self.v, self.D, self.deltas, self.wrong = v, D, {}, []
        self.slots = self.eslots = None

    def case(self, name, entry, n, **opts):
        """Run one case under `opts` (put back afterwards); record its deltas."""
        assert name not in self.deltas, name
        old = {}
        for k, val in opts.items():
            old[k] = SETTABLE_DEFAULT[k] if k in SETTABLE_DEFAULT else self.v.get_option(k)
            self.v.set_option(k, val)
        try:
            c0 = _counters(self.v)
            got, want = run_entry(self.v, self.D, entry, n, self.slots, self.eslots)
            self.deltas[name] = [b - a for a, b in zip(c0, _counters(self.v))]
            if not np.array_equal(np.asarray(got, np.uint8), np.asarray(want, np.uint8)):
                self.wrong.append(name)
        finally:
            for k, val in old.items():
                self.v.set_option(k, val)

    def arena(self, **opts):
        """A fresh resident arena under `opts` holding the base set's keys
        (the off-curve key too: a slot with verdict 0), with its index."""
        v = self.v
        v.keys_reset()
        for k, val in dict({"keys_wide": 2, "keys_k6": 1, "keys_index": 1}, **opts).items():
            v.set_option(k, val)
        self.slots = v.keys_load(self.D.pub).astype(np.uint32)
        self.slots[3] = v.keys_count + UNLOADED

    def ed_arena(self, wide):
        v = self.v
        v.ed_keys_reset()
        v.set_option("ed_keys_wide", wide)
        self.eslots = v.ed_keys_load(self.D.epub).astype(np.uint32)
        self.eslots[3] = v.ed_keys_count + UNLOADED


# options a case may set that gv_get_option does not read: their defaults
SETTABLE_DEFAULT = {"lat_zero_copy": 1, "lat_sliced": 1, "gfull_item": 1, "ed_keyed": 1}


def run_matrix(v, D, keyed125=False):
    m = Matrix(v, D)
    for k, val in BOUNDS.items():
        v.set_option(k, val)
    if keyed125:                              # (the child: GV_KEYED_K4=0) the 125-doubling keyed ladder
        m.arena(keys_wide=0, keys_k6=0)
        for n in (257, 1000):
            m.case(f"keyed125/dev_keyed/{n}", "dev_keyed", n)
            m.case(f"keyed125/host_keyed/{n}", "host_keyed", n)
            m.case(f"keyed125/grouped/dev_dig/{n}", "dev_dig", n)
        return m
    # no arena: the pub33 entry points at every size, then one switch at a time
    for entry in ("host_dig", "host_msg", "pinned_dig", "submit_dig", "submit_msg", "dev_dig", "dev_msg"):
        for n in SIZES:
            m.case(f"none/{entry}/{n}", entry, n)
    for n in SIZES:
        m.case(f"none/pinned_dig/zc0/{n}", "pinned_dig", n, lat_zero_copy=0)
    for n in (64, 257, 1000):
        m.case(f"none/host_dig/zc0/{n}", "host_dig", n, lat_zero_copy=0)
        for entry in ("host_dig_many", "dev_dig_many"):
            m.case(f"none/{entry}/{n}", entry, n)
            for sw in ("gfull", "gfull_item", "group_keys"):
                m.case(f"none/{entry}/{sw}/{n}", entry, n, **{sw: SWITCHES[sw]})
        for sw, val in SWITCHES.items():
            for entry in ("host_dig", "dev_dig", "dev_msg"):
                m.case(f"none/{entry}/{sw}/{n}", entry, n, **{sw: val})
    # the resident arena's states: every keyed entry point, and the pub33 device calls through the index
    keyed = ("host_keyed", "host_keyed_msg", "submit_keyed", "submit_keyed_msg", "dev_keyed", "dev_keyed_stream")
    for state, opts in (("k4", {"keys_wide": 0, "keys_k6": 0}), ("kn", {"keys_wide": 0}), ("wide1", {"keys_wide": 1}),
                        ("wide2", {})):
        m.arena(**opts)
        for n in SIZES:
            for entry in keyed:
                m.case(f"{state}/{entry}/{n}", entry, n)
            for entry in ("dev_dig", "dev_msg"):
                m.case(f"{state}/{entry}/index/{n}", entry, n)
                m.case(f"{state}/{entry}/noindex/{n}", entry, n, keys_index=0)
        for n in (32, 64, 65, 256):
            for entry in ("host_keyed", "dev_keyed"):
                m.case(f"{state}/{entry}/lat_kw0/{n}", entry, n, lat_kw=0)
        m.case(f"{state}/dev_dig_many/index/257", "dev_dig_many", 257)      # keys the arena does not hold
        if state in ("k4", "wide2"):
            for n in SIZES:
                m.case(f"{state}/pinned_keyed/{n}", "pinned_keyed", n)
                m.case(f"{state}/pinned_keyed/zc0/{n}", "pinned_keyed", n, lat_zero_copy=0)
            for n in (64, 257, 1000):
                for sw in ("gfull", "sort_keys", "lat_sliced", "pipeline_dev", "two_ladders"):
                    for entry in ("host_keyed", "dev_keyed"):
                        m.case(f"{state}/{entry}/{sw}/{n}", entry, n, **{sw: SWITCHES[sw]})
    v.keys_reset()
    # ed25519: the unkeyed calls, then the keyed ones per arena state
    for n in SIZES:
        for entry in ("ed_host", "ed_dev"):
            m.case(f"ed/{entry}/{n}", entry, n)
    for wide in (0, 6, 8):
        m.ed_arena(wide)
        for n in SIZES:
            for ed_keyed in (1, 0):
                for entry in ("ed_host_keyed", "ed_dev_keyed"):
                    m.case(f"edw{wide}/{entry}/ed_keyed{ed_keyed}/{n}", entry, n, ed_keyed=ed_keyed)
        for n in (65, 1000):
            for entry in ("ed_host_keyed", "ed_dev_keyed"):
                m.case(f"edw{wide}/{entry}/sort_keys/{n}", entry, n, sort_keys=0)
    v.ed_keys_reset()
    v.set_option("ed_keys_wide", 0)
    return m


def _child():
    """GV_KEYED_K4=0 (set by the parent process): the keyed125 cases as JSON."""
    with gvm.Verifier([0]) as v:
        m = run_matrix(v, Data(), keyed125=True)
    print(json.dumps({"deltas": m.deltas, "wrong": m.wrong}))


@pytest.fixture(scope="module")
def matrix():
    D = Data()
    with gvm.Verifier([0]) as v:
        m = run_matrix(v, D)
    env = dict(os.environ, GV_KEYED_K4="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True,
                       stdout=subprocess.PIPE, timeout=120)
    child = json.loads(r.stdout.decode().strip().splitlines()[-1])
    m.deltas.update(child["deltas"])
    m.wrong += child["wrong"]
    record = os.environ.get("GV_ROUTE_MATRIX_RECORD")
    if record:
        with open(record, "w") as f:
            json.dump({"counters": list(gvm.Verifier.ROUTES) + list(EXTRA), "cases": m.deltas}, f,
                      separators=(",", ":"))
            f.write("\n")
    return m


@pytest.fixture(scope="module")
def parent():
    with open(os.environ.get("GV_ROUTE_MATRIX_RECORD") or FIXTURE) as f:
        return json.load(f)


def test_every_verdict_equals_the_oracle(matrix):
    assert not matrix.wrong, matrix.wrong[:20]


def test_every_case_takes_the_parent_route(matrix, parent):
    assert parent["counters"] == list(gvm.Verifier.ROUTES) + list(EXTRA)
    assert sorted(matrix.deltas) == sorted(parent["cases"])
    diff = {k: (matrix.deltas[k], parent["cases"][k]) for k in parent["cases"] if matrix.deltas[k] != parent["cases"][k]}
    assert not diff, list(diff.items())[:10]


def test_the_parent_record_covers_every_route(parent):
    for i, route in enumerate(gvm.Verifier.ROUTES):
        assert any(d[i] for d in parent["cases"].values()), route


if __name__ == "__main__" and sys.argv[1:] == ["--child"]:
    _child()
