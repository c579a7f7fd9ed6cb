"""Multisig keys whose sub-keys are multisigs, through every ante path of the
host mirror (libgvhost), judged by the restatement of the reference's
recursion in tests/ante_ref.py:

  x/auth/types/stdtx.go:125-137     CountSubKeys, used by ValidateSigCountDecorator (sigverify.go:275-291)
  x/auth/ante/sigverify.go:299-338  DefaultSigVerificationGasConsumer <-> ConsumeMultisignatureVerificationGas
                                    (nested errors dropped, nested panics not)
  tendermint crypto/multisig        PubKeyMultisigThreshold.VerifyBytes calling each sub-key's VerifyBytes
  x/auth/ante/ante_test.go:627-659  TestCountSubkeys: 1, 5 and 11 ("multi level multikey") leaves

The unmarked tests stop before signature verification (ReCheck context) or
use HostApp.consume_sig_gas, so they need no verifier; the rest are marked gpu
and run the verification, block, verdict-cache and CheckTx-window paths.
"""
import hashlib
import random
import threading

import pytest

import gpuverify as gvm
import gvhost
import txkit as T
from ante_ref import AnteRef, Meter, count_subkeys, decode_pubkey

CHAIN = "gv-nest"
FEE = T.Fee([(0, "stake")], 1000000)
UNAUTH = "signature verification failed; verify correct account sequence and chain-id: unauthorized"
INDEX_PANIC = "runtime error: index out of range: panic"
JUNK = b"\x01" * 64                      # a signature nobody verifies (gas stage, ReCheck)


# ------------------------------------------------------------------ key trees
class SecpKey:
    ed = False

    def __init__(self, tag: bytes):
        self.priv = T.privkey_from_secret(b"nest-" + tag)
        self.amino = T.amino_secp(T.secp_pubkey(self.priv))

    def sign(self, msg):
        return T.secp_sign(self.priv, msg)


class EdKey:
    ed = True

    def __init__(self, tag: bytes):
        self.seed, pub32 = T.ed25519_keypair(hashlib.sha256(b"nest-ed-" + tag).digest())
        self.amino = T.amino_ed25519(pub32)

    def sign(self, msg):
        return T.ed25519_sign(self.seed, msg)


class Multi:
    """PubKeyMultisigThreshold{K, PubKeys}; a sub-key is a leaf key or a Multi."""

    def __init__(self, k, subs):
        self.k, self.subs = k, list(subs)

    @property
    def amino(self):
        return T.amino_multisig(self.k, [s.amino for s in self.subs])

    def n_leaves(self):
        return sum(s.n_leaves() if isinstance(s, Multi) else 1 for s in self.subs)

    def depth(self):
        return 1 + max([s.depth() for s in self.subs if isinstance(s, Multi)] or [0])


def keys(tag, n):
    return [SecpKey(b"%s-%d" % (tag, i)) for i in range(n)]


def msig(node, parts):
    """Multisignature of `node`: parts = {sub-key index: that sub-key's signature bytes}."""
    idx = sorted(parts)
    return T.multisignature([i in parts for i in range(len(node.subs))], [parts[i] for i in idx])


def rand_tree(rng, tag, max_depth=3, max_leaves=12, ed_prob=0.0):
    """A seeded key tree: 2..4 sub-keys per multisig, at least one nested
    multisig under the root, at most max_depth multisig levels and max_leaves leaves."""
    ctr = [0]

    def leaf():
        ctr[0] += 1
        cls = EdKey if rng.random() < ed_prob else SecpKey
        return cls(b"%s-%d" % (tag, ctr[0]))

    def build(depth, cap, force):
        n = rng.randint(2, min(4, cap))
        subs, used = [], 0
        nested_at = rng.randrange(n) if force else -1
        for j in range(n):
            room = cap - used - (n - j - 1)              # every later sub-key keeps at least one leaf
            if depth < max_depth and room >= 2 and (j == nested_at or rng.random() < 0.3):
                sub = build(depth + 1, min(room, 5), False)
                used += sub.n_leaves()
            else:
                sub = leaf()
                used += 1
            subs.append(sub)
        return Multi(rng.randint(1, n), subs)

    while True:
        t = build(1, max_leaves, True)
        if t.depth() >= 2:
            return t


# ------------------------------------------------------------ signature trees
def sign_tree(node, rng, sign):
    """A signature for `node` as a tree that can still be mutated: K..N sub-keys
    chosen at random, a nested multisig among them wherever the node has one.
    sign(leaf key) -> that leaf's signature bytes."""
    if not isinstance(node, Multi):
        return {"key": node, "sig": sign(node)}
    n = len(node.subs)
    chosen = sorted(rng.sample(range(n), rng.randint(node.k, n)))
    nested = [i for i, s in enumerate(node.subs) if isinstance(s, Multi)]
    if nested and not set(nested) & set(chosen):
        chosen[rng.randrange(len(chosen))] = rng.choice(nested)
        chosen.sort()
    return {"node": node, "chosen": chosen, "bits": [i in chosen for i in range(n)],
            "kids": [sign_tree(node.subs[i], rng, sign) for i in chosen], "extra": None, "raw": None}


def encode(st) -> bytes:
    if "sig" in st:
        return st["sig"]
    if st["raw"] is not None:
        return st["raw"]
    if st["extra"] is None:
        ba = T.compact_bit_array(st["bits"])
    else:                                               # extra_bits_stored chosen freely
        elems = bytearray((len(st["bits"]) + 7) // 8)
        for i, b in enumerate(st["bits"]):
            if b:
                elems[i >> 3] |= 1 << (7 - i % 8)
        ba = T.uvarint(1 << 3) + T.uvarint(st["extra"]) + T.amino_bytes_field(2, bytes(elems))
    return T.amino_bytes_field(1, ba) + b"".join(T.amino_bytes_field(2, encode(k)) for k in st["kids"])


def multis(st, depth=0):
    """[(multisig node of the signature tree, depth)] in pre-order"""
    if "sig" in st:
        return []
    return [(st, depth)] + [x for k in st["kids"] for x in multis(k, depth + 1)]


LEAF_KINDS = ("bad_leaf", "corrupt", "short_sig")              # test_block_paths.build_block's kinds ...
FALSE_KINDS = ("too_few", "short_bits")                         # ... verification false, no panic
PANIC_KINDS = ("malformed", "long_bits", "more_bits", "extra_past")


def mutate(st, kind, level, rng, msg=None):
    """Apply one mutation at a node of the signature tree: level 'outer' = the
    top-level Multisignature (or a leaf directly under it), 'inner' = a nested
    one (or a leaf under a nested one).  Returns the multisig node touched."""
    nodes = multis(st)
    cand = [m for m, d in nodes if (d == 0) == (level == "outer")]
    if kind in LEAF_KINDS or kind == "ed_leaf":
        with_leaf = [(m, d) for m, d in nodes if any("sig" in k for k in m["kids"])]
        at_level = [m for m, d in with_leaf if (d == 0) == (level == "outer")]
        m = rng.choice(at_level or [m for m, _ in with_leaf])               # no leaf at that level: any level
        j = rng.choice([j for j, k in enumerate(m["kids"]) if "sig" in k])
        leaf = m["kids"][j]
        if kind == "bad_leaf":                           # signed by another key of the same type
            leaf["sig"] = (EdKey if leaf["key"].ed else SecpKey)(b"intruder").sign(msg)
        elif kind == "corrupt":
            s = leaf["sig"]
            leaf["sig"] = s[:10] + bytes([s[10] ^ 1]) + s[11:]
        elif kind == "short_sig":                        # VerifyBytes' length check
            leaf["sig"] = leaf["sig"][:63]
        else:                                            # ed_leaf: the key tree gets an ed25519 key there
            ek = EdKey(b"swap-%d" % rng.randrange(1 << 30))
            m["node"].subs[m["chosen"][j]] = ek
            leaf["key"] = ek
        return m
    m = rng.choice(cand)
    if kind == "too_few":                                # K-1 bits and signatures
        keep = m["node"].k - 1
        for i in m["chosen"][keep:]:
            m["bits"][i] = False
        m["chosen"], m["kids"] = m["chosen"][:keep], m["kids"][:keep]
    elif kind == "short_bits":                           # bit array shorter than the key list
        m["bits"] = m["bits"][:-1]
        m["kids"] = m["kids"][:sum(m["bits"])]
    elif kind == "malformed":                            # bytes amino cannot decode
        m["raw"] = encode(m)[:-1] if rng.random() < 0.5 else b"\xff\xff"
    elif kind == "long_bits":                            # a set bit past the key list, with a signature
        m["bits"] = m["bits"] + [True]
        m["kids"] = m["kids"] + [{"key": None, "sig": JUNK}]
    elif kind == "more_bits":                            # more set bits than signatures
        m["kids"] = m["kids"][:-1]
    elif kind == "extra_past":                           # Size() = extra > 8 * len(Elems): bit 8 indexes Elems[1]
        m["extra"] = rng.randint(9, 15)
    else:
        raise ValueError(kind)
    return m


def ante3(r):
    return r["code"], r["log"], r["gas_used"]


# ================================================================= CPU tests
def recheck_pair(sig_limit=7):
    app = gvhost.HostApp(None, chain_id=CHAIN, height=1)
    app.set_context(CHAIN, 1, recheck=True)
    app.set_params(tx_sig_limit=sig_limit)
    return app, AnteRef(CHAIN, height=1, recheck=True, sig_limit=sig_limit)


def recheck_tx(app, ref, key, with_pub=True, preset=False, number=7):
    """One MsgSend signed (with junk: ReCheck verifies nothing) by `key`, every
    bit set at every level, through both judges: (mirror result, restatement)."""
    addr = T.address(key.amino)
    pub = key.amino if preset else b""
    app.set_account(addr, number, 0, pub)
    ref.set_account(addr, number, 0, pub)
    msgs = [T.MsgSend(addr, b"\x09" * 20, [(1, "stake")])]
    sigs = [(key.amino if with_pub else b"", encode(full_tree(key)))]     # the gas stage walks the whole tree
    tx = T.std_tx(msgs, FEE, "", sigs)
    rc, r = app.ante(tx)
    assert rc == 0
    return r, ref.ante(msgs, FEE, "", sigs, len(tx))


def full_tree(node):
    """the signature tree of `node` with every bit set at every level, junk leaf signatures"""
    if not isinstance(node, Multi):
        return {"key": node, "sig": JUNK}
    n = len(node.subs)
    return {"node": node, "chosen": list(range(n)), "bits": [True] * n, "kids": [full_tree(s) for s in node.subs],
            "extra": None, "raw": None}


def count_shapes():
    """TestCountSubkeys' three keys (ante_test.go:635-640)"""
    single = SecpKey(b"cs-single")
    one_level = Multi(4, keys(b"cs-one", 5))
    multi_level = Multi(2, [Multi(4, keys(b"cs-sub1", 5)), Multi(4, keys(b"cs-sub2", 5)), SecpKey(b"cs-top")])
    return single, one_level, multi_level


def test_count_subkeys_shapes_in_the_sig_limit_log():
    """CountSubKeys = 1, 5, 11, read off the mirror's ErrTooManySignatures log
    with the limit one below, and accepted (ReCheck: code 0) with the limit at
    the count; (code, log, gas) equal the restatement either way."""
    for key, want in zip(count_shapes(), (1, 5, 11)):
        assert count_subkeys(decode_pubkey(key.amino)) == want
        app, ref = recheck_pair(sig_limit=want - 1)
        r, exp = recheck_tx(app, ref, key)
        assert ante3(r) == exp
        assert (r["code"], r["log"]) == (14, f"signatures: {want}, limit: {want - 1}: maximum number of signatures "
                                              "exceeded")
        app.close()
        app, ref = recheck_pair(sig_limit=want)
        r, exp = recheck_tx(app, ref, key)
        assert ante3(r) == exp and r["code"] == 0, r
        app.close()


def test_multi_level_key_at_the_default_limit():
    """ante_test.go:651 at TxSigLimit 7: 11 signatures; the same account with
    the key on the account and none in the tx counts 1 (the count is over the
    tx's pubkeys) and passes."""
    multi_level = count_shapes()[2]
    app, ref = recheck_pair()
    r, exp = recheck_tx(app, ref, multi_level)
    assert ante3(r) == exp
    assert (r["code"], r["log"]) == (14, "signatures: 11, limit: 7: maximum number of signatures exceeded")
    r, exp = recheck_tx(app, ref, multi_level, with_pub=False, preset=True)
    assert ante3(r) == exp and r["code"] == 0, r
    # the gas stage charged all 11 leaves of the account's key
    lone = SecpKey(b"cs-lone")
    r1, exp1 = recheck_tx(app, ref, lone, with_pub=False, preset=True, number=8)
    assert ante3(r1) == exp1 and r1["code"] == 0
    assert r["gas_used"] - r1["gas_used"] > 10 * 1000
    app.close()


def test_sig_limit_boundary_on_a_nested_tree():
    """2-of-3 {2-of-3, 1-of-3, key}: exactly 7 leaves pass TxSigLimit 7; one
    more leaf in the inner key (8) does not."""
    seven = Multi(2, [Multi(2, keys(b"b7-a", 3)), Multi(1, keys(b"b7-b", 3)), SecpKey(b"b7-c")])
    eight = Multi(2, [Multi(2, keys(b"b8-a", 3)), Multi(1, keys(b"b8-b", 4)), SecpKey(b"b8-c")])
    assert (seven.n_leaves(), eight.n_leaves()) == (7, 8)
    app, ref = recheck_pair()
    r, exp = recheck_tx(app, ref, seven)
    assert ante3(r) == exp and r["code"] == 0, r
    r, exp = recheck_tx(app, ref, eight, number=9)
    assert ante3(r) == exp
    assert (r["code"], r["log"]) == (14, "signatures: 8, limit: 7: maximum number of signatures exceeded")
    app.close()


def test_two_signers_counts_add_up():
    """The count runs over the signers in order: a plain key (1) then a 7-leaf
    nested key reaches 8 at the second signer."""
    plain = SecpKey(b"two-plain")
    nested = Multi(1, [Multi(2, keys(b"two-a", 4)), Multi(1, keys(b"two-b", 3))])
    app, ref = recheck_pair()
    pa, na = T.address(plain.amino), T.address(nested.amino)
    for x in (app, ref):
        x.set_account(pa, 1, 0)
        x.set_account(na, 2, 0)
    msgs = [T.MsgSend(pa, b"\x09" * 20, [(1, "stake")]), T.MsgSend(na, b"\x09" * 20, [(1, "stake")])]
    sigs = [(plain.amino, JUNK), (nested.amino, encode(full_tree(nested)))]
    tx = T.std_tx(msgs, FEE, "", sigs)
    rc, r = app.ante(tx)
    assert rc == 0 and ante3(r) == ref.ante(msgs, FEE, "", sigs, len(tx))
    assert (r["code"], r["log"]) == (14, "signatures: 8, limit: 7: maximum number of signatures exceeded")
    app.close()


def test_nested_key_canonical_bytes_and_address():
    """Multisig Address() = SHA256(amino bytes)[:20] of the canonical encoding:
    the mirror decodes and re-encodes the tree (decode_pubkey_body /
    encode_pubkey); depths 1-4, mixed leaf types, K = 0, 1 and a two-byte uvarint."""
    def expect(amino):
        return hashlib.sha256(amino).digest()[:20]

    def leaf(i):
        return (EdKey if i % 3 == 1 else SecpKey)(b"addr-%d" % i)

    seen = set()
    for depth in (1, 2, 3, 4):
        for k in (0, 1, 300):
            node = Multi(k, [leaf(0), leaf(1)])
            for d in range(1, depth):                    # wrap: the nested key first, in the middle, last
                subs = [leaf(10 * d), leaf(10 * d + 1)]
                subs.insert(d % 3, node)
                node = Multi(k if d % 2 else 2, subs)
            assert node.depth() == depth
            amino = node.amino
            if k == 300:
                assert T.uvarint(300) == b"\xac\x02" and b"\x08\xac\x02" in amino
            got = gvhost.pubkey_address(amino)
            assert got == expect(amino) == T.address(amino)
            seen.add(got)
    assert len(seen) == 12


def chain_of(levels, leaf):
    node = leaf
    for _ in range(levels):
        node = Multi(1, [node])
    return node


def test_mirror_depth_bound():
    """The mirror's own bound, a defensive deviation: the reference has no
    nesting limit (amino recurses as deep as the bytes go), so the bound is
    not part of tests/ante_ref.py.  16 multisig levels around a key decode and
    are charged like the reference; 17 are ErrPanic 'multisig nesting too deep'."""
    app = gvhost.HostApp(None, chain_id=CHAIN, height=1)
    ref = AnteRef(CHAIN)
    leaf = SecpKey(b"deep")
    ok, deep = chain_of(16, leaf), chain_of(17, leaf)
    sig16, sig17 = encode(full_tree(ok)), encode(full_tree(deep))
    r = app.consume_sig_gas(sig16, ok.amino)
    assert ante3(r) == ref.consume_sig_gas(sig16, ok.amino) == (0, "", 1000)
    assert gvhost.pubkey_address(ok.amino) == hashlib.sha256(ok.amino).digest()[:20]
    r = app.consume_sig_gas(sig17, deep.amino)
    assert ante3(r) == (111222, "multisig nesting too deep: panic", 0) and r["codespace"] == "undefined"
    assert ref.consume_sig_gas(sig17, deep.amino) == (0, "", 1000)          # the reference's own answer
    with pytest.raises(ValueError):
        gvhost.pubkey_address(deep.amino)
    app.close()
    # the same through the ante chain (ReCheck): 16 levels equal the restatement
    app, ref = recheck_pair()
    r, exp = recheck_tx(app, ref, ok)
    assert ante3(r) == exp and r["code"] == 0, r
    app.close()


def test_gas_runs_out_between_two_inner_leaves():
    """2-of-3 {key, 2-of-2 {key, ed25519}, key}, all bits: charges 1000, then
    1000 + 590 inside, then 1000.  The meter's limit decides where the
    reference's ConsumeGas panics; the location is that leaf's descriptor."""
    a, c, e, b = SecpKey(b"og-a"), SecpKey(b"og-c"), EdKey(b"og-e"), SecpKey(b"og-b")
    key = Multi(2, [a, Multi(2, [c, e]), b])
    sig = encode(full_tree(key))
    app = gvhost.HostApp(None, chain_id=CHAIN, height=1)
    ref = AnteRef(CHAIN)
    for limit, want in ((0, (0, "", 3590)),
                        (3590, (0, "", 3590)),
                        (1500, (11, "out of gas in location: ante verify: secp256k1: out of gas", 2000)),
                        (2300, (11, "out of gas in location: ante verify: ed25519: out of gas", 2590)),
                        (2590, (11, "out of gas in location: ante verify: secp256k1: out of gas", 3590))):
        assert ante3(app.consume_sig_gas(sig, key.amino, limit)) == ref.consume_sig_gas(sig, key.amino, limit) == want
    app.close()


GAS_KINDS = ("none", "malformed", "long_bits", "short_bits", "more_bits", "extra_past", "ed_leaf", "gas_limit")


class Tape(Meter):
    """an infinite meter that keeps the total after every charge"""

    def __init__(self):
        super().__init__(None)
        self.totals = []

    def consume(self, amount, desc):
        super().consume(amount, desc)
        self.totals.append(self.used)


def leaf_depths(st, depth=0):
    """depth of the multisig holding each leaf signature, in the order the gas walk charges them"""
    if "sig" in st:
        return [depth - 1]
    return [d for k in st["kids"] for d in leaf_depths(k, depth + 1)]


def gas_cases(n=400, seed=0x6A5):
    """[(kind, level, pub amino, sig bytes, gas limit, between)]: kinds and
    levels round-robin, the rest seeded.  gas_limit cases: the limit lies
    between the totals after two consecutive leaves -- for level 'inner', two
    leaves of nested multisigs where the signature has such a pair (between =
    True), else before any nested leaf."""
    rng = random.Random(seed)
    ref = AnteRef(CHAIN)
    out = []
    for c in range(n):
        kind, level = GAS_KINDS[c % len(GAS_KINDS)], ("outer", "inner")[c // len(GAS_KINDS) % 2]
        tree = rand_tree(rng, b"gas-%d" % c, ed_prob=0.15)
        st = sign_tree(tree, rng, lambda k: JUNK)
        limit, between = 0, False
        if kind not in ("none", "gas_limit"):
            mutate(st, kind, level, rng)
        sig = encode(st)
        if kind == "gas_limit":
            tape = Tape()
            ref._sig_gas(tape, sig, decode_pubkey(tree.amino), True)
            totals, depths = [0] + tape.totals, leaf_depths(st)
            assert len(depths) == len(tape.totals)
            # the walk runs out at leaf i (0-based) for a limit in [totals[i], totals[i + 1] - 1]
            if level == "inner":
                cand = [i for i in range(1, len(depths)) if depths[i] >= 1 and depths[i - 1] >= 1]
                between = bool(cand)
                cand = cand or [i for i in range(len(depths)) if depths[i] >= 1]
            else:
                cand = [i for i in range(len(depths)) if depths[i] == 0] or list(range(len(depths)))
            i = rng.choice(cand)
            limit = rng.randint(max(1, totals[i]), totals[i + 1] - 1)
        out.append((kind, level, tree.amino, sig, limit, between))
    return out


def test_gas_consumer_differential():
    """~400 seeded trees (depth <= 3, <= 12 leaves, secp256k1 and ed25519
    leaves) with random Multisignatures, well-formed and mutated at the outer
    or an inner level: HostApp.consume_sig_gas == the restatement's gas
    recursion on (code, log, gas_used) -- the log carries the panic text and
    the out-of-gas location."""
    cases = gas_cases()
    app = gvhost.HostApp(None, chain_id=CHAIN, height=1)
    ref = AnteRef(CHAIN)
    kinds, codes, n_between = {}, {}, 0
    for kind, level, pub, sig, limit, between in cases:
        want = ref.consume_sig_gas(sig, pub, limit)
        n_between += between
        kinds[kind, level] = kinds.get((kind, level), 0) + 1
        codes[want[0]] = codes.get(want[0], 0) + 1
        if kind in ("malformed", "long_bits", "more_bits", "extra_past"):
            assert want[0] == 111222, (kind, level, want)
        if kind == "gas_limit":
            assert want[0] == 11, (kind, level, want)
        got = app.consume_sig_gas(sig, pub, limit)
        assert ante3(got) == want, (kind, level, limit, sig.hex(), pub.hex())
    app.close()
    print("gas differential: kinds", sorted(kinds.items()), "codes", sorted(codes.items()),
          "out of gas between two inner leaves", n_between)
    # conditions, on the restatement's results alone
    assert set(kinds) == {(k, lv) for k in GAS_KINDS for lv in ("outer", "inner")}
    assert min(kinds.values()) >= 10, kinds
    assert all(codes.get(c, 0) >= 10 for c in (0, 11, 111222)), codes
    assert n_between >= 10


# ================================================================= GPU tests
@pytest.fixture(scope="module")
def ver():
    v = gvm.Verifier([0])
    yield v
    v.close()


class Pair:
    """The mirror (with a verifier) and the restatement over the same accounts."""

    def __init__(self, ver, sig_limit=7, height=3):
        self.app = gvhost.HostApp(ver, chain_id=CHAIN, height=height)
        self.app.set_params(tx_sig_limit=sig_limit)
        self.ref = AnteRef(CHAIN, height=height, sig_limit=sig_limit)
        self.numbers = {}

    def add(self, key, number, preset=False):
        addr = T.address(key.amino)
        pub = key.amino if preset else b""
        self.app.set_account(addr, number, 0, pub)
        self.ref.set_account(addr, number, 0, pub)
        self.numbers[addr] = number
        return addr

    def seq(self, addr):
        return self.ref.accounts[addr].sequence

    def sign_bytes(self, addr, msgs, seq=None):
        return T.std_sign_bytes(CHAIN, self.numbers[addr], self.seq(addr) if seq is None else seq, FEE, msgs, "")

    def check(self, msgs, sigs, code, leaves, log=None, gpu=None):
        """ante on both; the mirror equals the restatement on (code, log, gas)
        and on every signer's sequence afterwards.  leaves: the leaves the
        mirror had to decide (one per set bit with a 64-byte signature, every
        signer's), each by the GPU batch or the verdict cache; gpu: how many of
        them by the GPU, where the test's signatures make that certain (a leaf
        whose exact bytes an earlier tx of the app carried is a cache hit).
        Returns the mirror's result."""
        tx = T.std_tx(msgs, FEE, "", sigs)
        rc, r = self.app.ante(tx)
        want = self.ref.ante(msgs, FEE, "", sigs, len(tx))
        assert rc == 0 and ante3(r) == want, (r, want)
        assert r["code"] == code and r["gpu_leaves"] + r["cache_hits"] == leaves, r
        if gpu is not None:
            assert r["gpu_leaves"] == gpu, r
        if log is not None:
            assert r["log"] == log
        for a in T.tx_signers(msgs):
            assert self.app.get_account(a)["sequence"] == self.seq(a)
        return r

    def close(self):
        self.app.close()


SINK = b"\x09" * 20


def send(addr, amount=1):
    return [T.MsgSend(addr, SINK, [(amount, "stake")])]


@pytest.mark.gpu
def test_two_level_key_valid_and_bad_leaves(ver):
    """2-of-3 {a, b, 2-of-2 {c, d}}: the GPU batch holds the leaves of both
    levels (one per set bit with a 64-byte signature)."""
    a, b, c, d = keys(b"n1", 4)
    inner = Multi(2, [c, d])
    key = Multi(2, [a, b, inner])
    p = Pair(ver)
    addr = p.add(key, 11)
    msgs = send(addr)
    sb = p.sign_bytes(addr, msgs)
    sig = msig(key, {0: a.sign(sb), 2: msig(inner, {0: c.sign(sb), 1: d.sign(sb)})})
    p.check(msgs, [(key.amino, sig)], 0, 3, gpu=3)                         # the set-bit leaves, a fresh cache
    assert p.seq(addr) == 1
    sb = p.sign_bytes(addr, msgs)
    sig = msig(key, {0: a.sign(sb), 1: b.sign(sb), 2: msig(inner, {0: c.sign(sb), 1: d.sign(sb)})})
    p.check(msgs, [(b"", sig)], 0, 4)                                      # all three outer bits
    sb = p.sign_bytes(addr, msgs)
    good = {0: a.sign(sb), 1: b.sign(sb), 2: msig(inner, {0: c.sign(sb), 1: d.sign(sb)})}
    for bad in ({**good, 2: msig(inner, {0: c.sign(sb), 1: c.sign(sb)})},                  # bad inner leaf
                {**good, 1: a.sign(sb)},                                                    # bad outer leaf
                {**good, 0: SecpKey(b"n1-x").sign(sb)}):
        p.check(msgs, [(b"", msig(key, bad))], 4, 4, UNAUTH)
    short = {**good, 2: msig(inner, {0: c.sign(sb), 1: d.sign(sb)[:63]})}                 # 63-byte inner signature
    p.check(msgs, [(b"", msig(key, short))], 4, 3, UNAUTH)
    assert p.seq(addr) == 2
    p.check(msgs, [(b"", msig(key, good))], 0, 4)
    p.close()


@pytest.mark.gpu
def test_ed25519_leaf_at_depth_two(ver):
    a, c = keys(b"n2", 2)
    e = EdKey(b"n2-e")
    inner = Multi(2, [e, c])
    key = Multi(2, [a, inner])
    p = Pair(ver)
    addr = p.add(key, 12)
    msgs = send(addr)
    sb = p.sign_bytes(addr, msgs)
    ok = msig(key, {0: a.sign(sb), 1: msig(inner, {0: e.sign(sb), 1: c.sign(sb)})})
    bad = msig(key, {0: a.sign(sb), 1: msig(inner, {0: e.sign(sb + b"x"), 1: c.sign(sb)})})
    p.check(msgs, [(key.amino, bad)], 4, 3, UNAUTH)
    p.check(msgs, [(key.amino, ok)], 0, 3)
    assert p.seq(addr) == 1
    # the nested ed25519 leaf was charged 590 and its 'unsupported' error dropped
    assert ante3(p.app.consume_sig_gas(ok, key.amino)) == p.ref.consume_sig_gas(ok, key.amino) == (0, "", 2590)
    p.close()


@pytest.mark.gpu
def test_same_key_at_both_levels_duplicate_leaves(ver):
    """2-of-2 {a, 1-of-2 {a, c}} with a's one signature in both places: two
    identical leaves in one batch; the next tx meets a non-empty verdict
    cache; after PreVerifyTxs both leaves are answered from it."""
    a, c = keys(b"n3", 2)
    inner = Multi(1, [a, c])
    key = Multi(2, [a, inner])
    p = Pair(ver)
    addr = p.add(key, 13)
    msgs = send(addr)
    for with_pub in (True, False):
        sb = p.sign_bytes(addr, msgs)
        s = a.sign(sb)
        r = p.check(msgs, [(key.amino if with_pub else b"", msig(key, {0: s, 1: msig(inner, {0: s})}))], 0, 2,
                    gpu=2)
        assert r["cache_hits"] == 0
    assert p.app.cache_size() > 0
    sb = p.sign_bytes(addr, msgs)
    s = a.sign(sb)
    sigs = [(b"", msig(key, {0: s, 1: msig(inner, {0: s})}))]
    rc, n = p.app.preverify([T.std_tx(msgs, FEE, "", sigs)])
    assert rc == 0
    r = p.check(msgs, sigs, 0, 2, gpu=0)
    assert r["cache_hits"] == 2
    # the duplicate is as bad as its twin: a's signature over other bytes, twice
    sb = p.sign_bytes(addr, msgs)
    s = a.sign(sb + b"x")
    p.check(msgs, [(b"", msig(key, {0: s, 1: msig(inner, {0: s})}))], 4, 2, UNAUTH)
    p.close()


@pytest.mark.gpu
def test_inner_structure_fails_with_good_outer_leaves(ver):
    """Inner threshold not met / inner bit-array size mismatch: the inner
    VerifyBytes is false, so the outer AND is false (code 4), with every outer
    leaf good."""
    a, b, c, d, e = keys(b"n4", 5)
    inner = Multi(2, [c, d, e])
    key = Multi(2, [a, b, inner])
    p = Pair(ver)
    addr = p.add(key, 14, preset=True)
    msgs = send(addr)
    sb = p.sign_bytes(addr, msgs)
    below = msig(inner, {1: d.sign(sb)})                                    # 1 < K = 2
    p.check(msgs, [(b"", msig(key, {0: a.sign(sb), 1: b.sign(sb), 2: below}))], 4, 2, UNAUTH)
    four = T.multisignature([True, True, False, False], [c.sign(sb), d.sign(sb)])    # 4 bits, 3 keys
    p.check(msgs, [(b"", msig(key, {0: a.sign(sb), 1: b.sign(sb), 2: four}))], 4, 2, UNAUTH)
    two = T.multisignature([True, True], [c.sign(sb), d.sign(sb)])                   # 2 bits, 3 keys
    p.check(msgs, [(b"", msig(key, {0: a.sign(sb), 1: b.sign(sb), 2: two}))], 4, 2, UNAUTH)
    ok = msig(inner, {0: c.sign(sb), 2: e.sign(sb)})
    p.check(msgs, [(b"", msig(key, {0: a.sign(sb), 1: b.sign(sb), 2: ok}))], 0, 4)
    p.close()


@pytest.mark.gpu
def test_malformed_inner_multisignature_panics_in_the_gas_stage(ver):
    """MustUnmarshalBinaryBare at depth 2 panics after the outer leaf before it
    was charged; ErrPanic, no sequence increment, nothing verified."""
    a, b, c, d = keys(b"n5", 4)
    inner = Multi(2, [c, d])
    key = Multi(2, [a, inner, b])
    p = Pair(ver)
    addr = p.add(key, 15)
    msgs = send(addr)
    sb = p.sign_bytes(addr, msgs)
    good = msig(inner, {0: c.sign(sb), 1: d.sign(sb)})
    r = p.check(msgs, [(key.amino, msig(key, {0: a.sign(sb), 1: good[:-1], 2: b.sign(sb)}))], 111222, 0,
                "insufficient bytes decoding byteslice: panic")
    assert r["codespace"] == "undefined" and p.seq(addr) == 0
    assert p.app.get_account(addr)["pub"] == b""                            # SetPubKey rolled back
    # a set inner bit with no signature for it: Sigs[sigIndex] panics after c's charge
    lone = T.multisignature([True, True], [c.sign(sb)])
    r2 = p.check(msgs, [(key.amino, msig(key, {0: a.sign(sb), 1: lone, 2: b.sign(sb)}))], 111222, 0, INDEX_PANIC)
    assert r2["gas_used"] > r["gas_used"] - 10 * len(good) + 1000           # c's charge, a shorter tx
    p.check(msgs, [(key.amino, msig(key, {0: a.sign(sb), 1: good, 2: b.sign(sb)}))], 0, 4)
    p.close()


@pytest.mark.gpu
def test_depth_three_chain_around_two_of_three(ver):
    a, b, c = keys(b"n6", 3)
    core = Multi(2, [a, b, c])
    mid = Multi(1, [core])
    key = Multi(1, [mid])
    p = Pair(ver)
    addr = p.add(key, 16)
    msgs = send(addr)
    sb = p.sign_bytes(addr, msgs)
    wrap = lambda s: msig(key, {0: msig(mid, {0: s})})
    p.check(msgs, [(key.amino, wrap(msig(core, {0: a.sign(sb), 2: b.sign(sb)})))], 4, 2, UNAUTH)
    p.check(msgs, [(key.amino, wrap(msig(core, {0: a.sign(sb), 2: c.sign(sb)})))], 0, 2)
    sb = p.sign_bytes(addr, msgs)
    p.check(msgs, [(b"", wrap(msig(core, {1: b.sign(sb)})))], 4, 0, UNAUTH)            # 1 < K at depth 3
    p.check(msgs, [(b"", wrap(msig(core, {0: a.sign(sb), 1: b.sign(sb), 2: c.sign(sb)})))], 0, 3)
    p.close()


@pytest.mark.gpu
def test_eight_leaf_tree_needs_a_higher_sig_limit(ver):
    key = Multi(2, [Multi(2, keys(b"n7-a", 3)), Multi(3, keys(b"n7-b", 4)), SecpKey(b"n7-c")])
    assert key.n_leaves() == 8
    m1, m2, top = key.subs

    def sigs_for(p, addr):
        sb = p.sign_bytes(addr, send(addr))
        return [(key.amino, msig(key, {0: msig(m1, {0: m1.subs[0].sign(sb), 2: m1.subs[2].sign(sb)}),
                                       1: msig(m2, {i: m2.subs[i].sign(sb) for i in (0, 1, 3)}),
                                       2: top.sign(sb)}))]

    p = Pair(ver)
    addr = p.add(key, 17)
    p.check(send(addr), sigs_for(p, addr), 14, 0, "signatures: 8, limit: 7: maximum number of signatures exceeded")
    assert p.seq(addr) == 0
    p.close()
    p = Pair(ver, sig_limit=12)
    addr = p.add(key, 17)
    p.check(send(addr), sigs_for(p, addr), 0, 6)
    assert p.seq(addr) == 1
    p.close()


@pytest.mark.gpu
def test_two_signers_first_failure_in_either(ver):
    """A nested multisig signer and a plain key in one tx: one batch holds
    both signers' leaves; the first failing signer decides, nobody's sequence
    moves, and the gas stops at that signer's account read."""
    a, b, c = keys(b"n8", 3)
    inner = Multi(1, [b, c])
    nested = Multi(2, [a, inner])
    plain = SecpKey(b"n8-plain")
    p = Pair(ver)
    na, pa = p.add(nested, 18), p.add(plain, 19)
    msgs = [T.MsgSend(na, SINK, [(1, "stake")]), T.MsgSend(pa, SINK, [(2, "stake")])]
    sbn, sbp = p.sign_bytes(na, msgs), p.sign_bytes(pa, msgs)
    sa, sp = a.sign(sbn), plain.sign(sbp)
    good_n = msig(nested, {0: sa, 1: msig(inner, {1: c.sign(sbn)})})
    bad_n = msig(nested, {0: sa, 1: msig(inner, {1: b.sign(sbn)})})
    r1 = p.check(msgs, [(nested.amino, bad_n), (plain.amino, sp)], 4, 3, UNAUTH, gpu=3)
    r2 = p.check(msgs, [(nested.amino, good_n), (plain.amino, a.sign(sbp))], 4, 3, UNAUTH, gpu=2)   # sa: cached
    assert r2["gas_used"] > r1["gas_used"]                                  # the walk got one account read further
    assert p.seq(na) == p.seq(pa) == 0
    p.check(msgs, [(nested.amino, good_n), (plain.amino, sp)], 0, 3, gpu=0)
    assert p.seq(na) == p.seq(pa) == 1
    p.close()


# ------------------------------------------------------- seeded differential
DIFF_KINDS = LEAF_KINDS + FALSE_KINDS + PANIC_KINDS + ("wrong_seq",)
N_ACCTS, N_TXS, PER_KIND = 10, 150, 6


class Workload:
    """150 txs over 10 nested accounts and the restatement's verdict for each,
    computed once for every run of the differential."""

    def __init__(self):
        rng = random.Random(0x4E57)
        self.accts = []
        for i in range(N_ACCTS):
            tree = rand_tree(rng, b"acct-%d" % i, ed_prob=0.08)
            self.accts.append((tree, T.address(tree.amino), 100 + i, i % 2 == 1))       # odd: key preset, not in txs
        kinds = ["none"] * (N_TXS - PER_KIND * len(DIFF_KINDS)) + [k for k in DIFF_KINDS for _ in range(PER_KIND)]
        rng.shuffle(kinds)
        self.ref = self.new_ref()
        self.kinds, self.txs, self.want, self.ed_leaves = kinds, [], [], 0
        for t, kind in enumerate(kinds):
            tree, addr, number, preset = self.accts[rng.randrange(N_ACCTS)]
            seq = self.ref.accounts[addr].sequence
            msgs = send(addr, 1 + t % 7)
            sb = T.std_sign_bytes(CHAIN, number, seq + (3 if kind == "wrong_seq" else 0), FEE, msgs, "")
            st = sign_tree(tree, rng, lambda k: k.sign(sb))
            if kind not in ("none", "wrong_seq"):
                mutate(st, kind, rng.choice(("outer", "inner")), rng, sb)
            self.ed_leaves += sum(k["key"] is not None and k["key"].ed for m, _ in multis(st) for k in m["kids"]
                                  if "sig" in k)
            sigs = [(b"" if preset else tree.amino, encode(st))]
            tx = T.std_tx(msgs, FEE, "", sigs)
            self.txs.append(tx)
            self.want.append(self.ref.ante(msgs, FEE, "", sigs, len(tx)))
        self.final = {addr: self.ref.accounts[addr].sequence for _, addr, _, _ in self.accts}

    def new_ref(self):
        ref = AnteRef(CHAIN, height=4, sig_limit=12)
        for tree, addr, number, preset in self.accts:
            ref.set_account(addr, number, 0, tree.amino if preset else b"")
        return ref

    def new_app(self, ver, gpu_hash):
        app = gvhost.HostApp(ver, chain_id=CHAIN, height=4)
        app.set_params(tx_sig_limit=12)
        app.set_gpu_hash(gpu_hash)
        for tree, addr, number, preset in self.accts:
            app.set_account(addr, number, 0, tree.amino if preset else b"")
        return app

    def run(self, ver, mode, gpu_hash):
        """[(code, log, gas_used, gas_wanted)] per tx, and the final sequences"""
        app = self.new_app(ver, gpu_hash)
        if mode == "ante" or mode == "preverify_ante":
            if mode == "preverify_ante":
                rc, _ = app.preverify(self.txs)
                assert rc == 0
            res = []
            for tx in self.txs:
                rc, r = app.ante(tx)
                assert rc == 0
                res.append(r)
        elif mode == "deliver_block":
            rc, res = app.deliver_block(self.txs)
            assert rc == 0
        else:
            third = N_TXS // 3
            rc, blocks = app.deliver_blocks_results([self.txs[:third], self.txs[third:2 * third], self.txs[2 * third:]])
            assert rc == 0
            res = [r for blk in blocks for r in blk]
        final = {addr: app.get_account(addr)["sequence"] for _, addr, _, _ in self.accts}
        app.close()
        return [ante3(r) + (r["gas_wanted"],) for r in res], final


@pytest.fixture(scope="module")
def workload():
    return Workload()


@pytest.fixture(scope="module")
def runs():
    return {}


def run_of(runs, workload, ver, mode, gpu_hash):
    if (mode, gpu_hash) not in runs:
        runs[mode, gpu_hash] = workload.run(ver, mode, gpu_hash)
    return runs[mode, gpu_hash]


def test_differential_workload_conditions(workload):
    """On the restatement's verdicts alone: >= 40 % accepted, every mutation
    kind at least 4 times, codes 0, 4 and 111222 all there, about 60 ed25519 leaves."""
    codes = [w[0] for w in workload.want]
    count = {k: workload.kinds.count(k) for k in ("none",) + DIFF_KINDS}
    by_code = {c: codes.count(c) for c in sorted(set(codes))}
    print("nested differential: kinds", count, "codes", by_code, "ed25519 leaves", workload.ed_leaves,
          "leaves per account", [t.n_leaves() for t, _, _, _ in workload.accts])
    assert codes.count(0) >= 0.4 * N_TXS, by_code
    assert all(count[k] >= 4 for k in DIFF_KINDS), count
    assert {0, 4, 111222} <= set(codes), by_code
    for kind, w in zip(workload.kinds, workload.want):
        assert w[0] == {"none": 0}.get(kind, 111222 if kind in PANIC_KINDS else 4), (kind, w)
    assert 20 <= workload.ed_leaves <= 120


MODES = ("ante", "deliver_block", "deliver_blocks", "preverify_ante")


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_hash", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_nested_differential(ver, workload, runs, mode, gpu_hash):
    """The same 150 txs through the per-tx ante, DeliverBlock, the pipelined
    replay in 3 blocks, and the per-tx ante after PreVerifyTxs (memoised
    plans; the gas shortcut falls back to the consumer on the panic cases):
    each equals the restatement tx by tx on (code, log, gas_used) and ends in
    its account sequences."""
    res, final = run_of(runs, workload, ver, mode, gpu_hash)
    for t, (got, want) in enumerate(zip(res, workload.want)):
        assert got[:3] == want, (t, workload.kinds[t], got, want)
    assert len(res) == N_TXS and final == workload.final


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_hash", [False, True])
def test_nested_differential_paths_agree(ver, workload, runs, gpu_hash):
    """... and the four equal each other, gas_wanted included."""
    base = run_of(runs, workload, ver, MODES[0], gpu_hash)
    for mode in MODES[1:]:
        assert run_of(runs, workload, ver, mode, gpu_hash) == base, mode
    assert all(r[3] == FEE.gas for r in base[0])


@pytest.mark.gpu
def test_checktx_window_with_nested_accounts(ver):
    """32 txs of 32 nested accounts through CheckTx at once (a window set):
    the results of the serial ante on a fresh app."""
    rng = random.Random(0xC7)
    accts, txs = [], []
    for i in range(32):
        tree = rand_tree(rng, b"ctx-%d" % i)
        addr = T.address(tree.amino)
        accts.append((addr, 300 + i))
        msgs = send(addr, 1 + i % 5)
        sb = T.std_sign_bytes(CHAIN, 300 + i, 0, FEE, msgs, "")
        st = sign_tree(tree, rng, lambda k: k.sign(sb))
        if i % 5 == 4:
            mutate(st, ("bad_leaf", "too_few", "more_bits")[i // 5 % 3], ("outer", "inner")[i % 2], rng, sb)
        txs.append(T.std_tx(msgs, FEE, "", [(tree.amino, encode(st))]))

    def fresh():
        app = gvhost.HostApp(ver, chain_id=CHAIN, height=6)
        app.set_params(tx_sig_limit=12)
        for addr, number in accts:
            app.set_account(addr, number, 0)
        return app

    app = fresh()
    app.set_window(32, 20000)
    out = [None] * len(txs)
    start = threading.Barrier(len(txs))

    def worker(i):
        start.wait()
        out[i] = app.checktx(txs[i])

    th = [threading.Thread(target=worker, args=(i,)) for i in range(len(txs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    seqs = [app.get_account(a)["sequence"] for a, _ in accts]
    app.close()
    plain = fresh()
    serial = [plain.ante(tx) for tx in txs]
    assert [(rc, ante3(r)) for rc, r in out] == [(rc, ante3(r)) for rc, r in serial]
    assert all(rc == 0 for rc, _ in serial)
    codes = [r["code"] for _, r in serial]
    assert (codes.count(0), codes.count(4), codes.count(111222)) == (26, 4, 2), codes
    assert seqs == [plain.get_account(a)["sequence"] for a, _ in accts]
    plain.close()
