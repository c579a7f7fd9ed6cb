"""ed25519 signatures with a chosen S -- test infrastructure shared by
test_ed_chosen_s_host.py and test_ed_chosen_s_gpu.py, built from
oracle/ed25519_ref.py alone (no file is committed for them).

Every verdict is encode([h](-A) + [S]B) == R.  go1.14 accepts keys of small
order, so a VALID signature exists for any S < L:
  * A = the identity (01 00 .. 00): [h](-A) is the identity whatever the hash,
    so R = encode([S]B) verifies for every message;
  * A = a torsion point T: R = encode([S]B + t) verifies when t = -[h]T; the
    eight t and a message counter are tried until one does (torsion_items).
That puts S at the edges of the kernels' signed-digit recodings of S (edges)
and on every entry of the comb tables of B a valid S can name (sweeps), each
with a rejected twin (twins), so an always-accept kernel fails too.

recode() is the balanced digit expansion written from its definition; it is
the independent statement the kernels' five recodings are held against."""
import functools
import hashlib
from dataclasses import dataclass, field

import numpy as np

from oracle import ed25519_ref as E

P, L = E.P, E.L
IDENT_KEY = E.encode_point(E.IDENT)


# ------------------------------------------------------------------ digits
def recode(s, bits):
    """The balanced radix-2^bits digits of s, least significant first, over
    256 / bits windows: the unique d_w in (-2^(bits-1), 2^(bits-1)] with
    sum d_w 2^(bits w) = s."""
    assert bits in (8, 16) and 0 <= s < 1 << 256
    nw, half, full = 256 // bits, 1 << (bits - 1), 1 << bits
    d, r = [], s
    for _ in range(nw):
        x = r % full                      # d_w = r mod 2^bits, taken from (-half, half]
        if x > half:
            x -= full
        d.append(x)
        r = (r - x) // full
    assert r == 0, "a carry leaves the top window"
    assert sum(x << (bits * w) for w, x in enumerate(d)) == s
    return d


def geometry(bits):
    return 256 // bits, 1 << (bits - 1), 1 << bits          # nw, half, full


# ------------------------------------------------------------------- [S]B
@functools.lru_cache(maxsize=None)
def _pow2_b():
    """2^i B, i < 253, extended coordinates"""
    out, q = [], E._ext(E.B)
    for _ in range(253):
        out.append(q)
        q = E._add(q, q)
    return out


def mul_b_ext(s):
    """[s]B in extended coordinates, 0 <= s < 2^253"""
    r, tab, i = E._ext(E.IDENT), _pow2_b(), 0
    while s:
        if s & 1:
            r = E._add(r, tab[i])
        s >>= 1
        i += 1
    return r


def _neg_ext(p):
    x, y, z, t = p
    return ((-x) % P, y, z, (-t) % P)


def encode_batch(pts):
    """canonical encodings of extended points, one inversion for all of them"""
    n = len(pts)
    pre, acc = [0] * n, 1
    for i, p in enumerate(pts):
        pre[i] = acc
        acc = acc * p[2] % P
    inv = pow(acc, P - 2, P)
    out = [None] * n
    for i in range(n - 1, -1, -1):
        x, y, z, _ = pts[i]
        zi = inv * pre[i] % P
        inv = inv * z % P
        out[i] = E.encode_point((x * zi % P, y * zi % P))
    return out


# ------------------------------------------------------------------- items
@dataclass
class Items:
    """A batch: pub n x 32, sig n x 64 (R || S), msgs (None: every message is
    empty), the expected verdicts, and per item its S and a label."""
    name: str
    pub: np.ndarray
    sig: np.ndarray
    want: np.ndarray
    S: list
    label: list
    msgs: list = field(default=None)

    def __len__(self):
        return len(self.S)

    def msg_arg(self):
        """what verify_batch_ed25519* take: the list, or for empty messages one
        (blob, off, len) triple of zeros"""
        if self.msgs is not None:
            return self.msgs
        z = np.zeros(len(self), np.uint64)
        return (np.zeros(1, np.uint8), z, z.astype(np.uint32))

    def msg(self, i):
        return b"" if self.msgs is None else self.msgs[i]

    def describe(self, i, bits=16):
        return (f"{self.name}[{i}] {self.label[i]} want={int(self.want[i])} S={self.S[i]:#x} "
                f"digits{bits}={recode(self.S[i], bits)}")


def _rows(chunks, width):
    return np.frombuffer(b"".join(chunks), np.uint8).reshape(-1, width).copy()


def identity_items(name, svals, labels, encs=None):
    """valid items of the identity key with empty messages: R = encode([S]B)"""
    svals = list(svals)
    assert all(0 <= s < L for s in svals)
    if encs is None:
        encs = encode_batch([mul_b_ext(s) for s in svals])
    n = len(svals)
    sig = _rows([r + s.to_bytes(32, "little") for r, s in zip(encs, svals)], 64)
    return Items(name, np.tile(np.frombuffer(IDENT_KEY, np.uint8), (n, 1)), sig, np.ones(n, np.uint8), svals,
                 list(labels))


def twins(items):
    """The same S with the next item's R (cyclically): every one is rejected,
    as the S of a set are distinct and below L, so the R are distinct points."""
    assert len(items) > 1 and len(set(items.S)) == len(items)
    sig = items.sig.copy()
    sig[:, :32] = np.roll(items.sig[:, :32], -1, axis=0)
    assert (sig[:, :32] != items.sig[:, :32]).any(axis=1).all()
    return Items(items.name + "/twin", items.pub, sig, np.zeros(len(items), np.uint8), items.S,
                 [lb + " with the next R" for lb in items.label], items.msgs)


def concat(name, parts):
    msgs = None
    if any(p.msgs is not None for p in parts):
        msgs = [p.msg(i) for p in parts for i in range(len(p))]
    return Items(name, np.concatenate([p.pub for p in parts]), np.concatenate([p.sig for p in parts]),
                 np.concatenate([p.want for p in parts]), [s for p in parts for s in p.S],
                 [f"{p.name}: {lb}" for p in parts for lb in p.label], msgs)


def take(items, idx):
    idx = [int(i) for i in idx]
    return Items(items.name, items.pub[idx], items.sig[idx], items.want[idx], [items.S[i] for i in idx],
                 [items.label[i] for i in idx], None if items.msgs is None else [items.msgs[i] for i in idx])


# ------------------------------------------------------------------- edges
@functools.lru_cache(maxsize=None)
def edges_labelled():
    """((label, S), ...): the edge values of S, distinct, all 0 <= S < L"""
    vals = [("0", 0), ("1", 1), ("2", 2), ("L-1", L - 1), ("L-2", L - 2), ("L-2^125", L - 2**125),
            ("2^252-1", 2**252 - 1), ("2^252", 2**252), ("2^252+1", 2**252 + 1)]
    for bits in (16, 8):
        nw, half, full = geometry(bits)
        four = (("half-1", half - 1), ("half", half), ("half+1", half + 1), ("full-1", full - 1))
        for w in range(nw - 1):                               # one window alone
            vals += [(f"r{bits} window {w} = {n}", v << (bits * w)) for n, v in four]
        for n, v in four:                                     # every window below the top at once
            vals.append((f"r{bits} all windows = {n}", sum(v << (bits * w) for w in range(nw - 1)) % 2**252))
        for k in range(1, nw):                                # 0xFF.. runs below a window boundary
            vals += [(f"r{bits} 2^({bits}*{k}) - {n}", (1 << (bits * k)) - d)
                     for n, d in (("1", 1), ("(half-1)", half - 1), ("half", half), ("(half+1)", half + 1))]
        for st in (0, 1, nw // 2, nw - 2):                    # ripples started at window st
            for n, lo, hi in (("half+1 under full-1", half + 1, full - 1), ("half under half-1", half, half - 1)):
                v = (lo << (bits * st)) + sum(hi << (bits * w) for w in range(st + 1, nw))
                vals.append((f"r{bits} ripple from window {st}: {n}", v % 2**252))
    seen, out = set(), []
    for lb, v in vals:
        assert 0 <= v < L, lb
        if v not in seen:
            seen.add(v)
            out.append((lb, v))
    return tuple(out)


def edges():
    return [v for _, v in edges_labelled()]


@functools.lru_cache(maxsize=None)
def edge_items():
    lab = edges_labelled()
    return identity_items("edges", [v for _, v in lab], [lb for lb, _ in lab])


# ------------------------------------------------------------------ sweeps
SWEEPS = ("plus", "even_minus", "odd_minus", "top")


def sweep_digits(kind, bits, j):
    """the digit vector item j of a sweep claims (before any borrow at j = half)"""
    nw = 256 // bits
    if kind == "top":
        return [0] * (nw - 1) + [j]
    if kind == "plus":
        return [j] * (nw - 1) + [0]
    par = 0 if kind == "even_minus" else 1
    return [-j if w % 2 == par else j for w in range(nw - 1)] + [1]


def sweep_len(kind, bits):
    nw, half, _ = geometry(bits)
    return ((0x1000 if bits == 16 else 16) if kind == "top" else half) + 1


def _check_sweep_digits(kind, bits, j, s):
    nw, half, _ = geometry(bits)
    claim, got = sweep_digits(kind, bits, j), recode(s, bits)
    if kind in ("even_minus", "odd_minus") and j == half:
        # -half is no balanced digit: it is +half with a borrow from the neighbour above
        for w in range(nw - 1):
            if claim[w] < 0:
                claim[w] += 1 << bits
                claim[w + 1] -= 1
    assert got == claim, (kind, bits, j)
    if kind != "top" and j < half:
        assert all(abs(d) == j for d in got[:nw - 1])


@functools.lru_cache(maxsize=None)
def sweeps(bits):
    """{kind: Items}: every entry (w, j) of the radix-2^bits comb table of B a
    valid S can reach -- j = 0 .. half in every window below the top with each
    sign (plus; even_minus / odd_minus put -j in the even / odd windows), and
    every top-window entry an S < L can name (top)."""
    nw, half, _ = geometry(bits)
    out = {}
    for kind in SWEEPS:
        n = sweep_len(kind, bits)
        s0 = sum(d << (bits * w) for w, d in enumerate(sweep_digits(kind, bits, 0)))
        delta = sum(d << (bits * w) for w, d in enumerate(sweep_digits(kind, bits, 1))) - s0
        step = mul_b_ext(abs(delta))
        if delta < 0:
            step = _neg_ext(step)
        svals, pts, p = [], [], mul_b_ext(s0)
        for j in range(n):                                    # S_j = S_0 + j delta, R_j = R_(j-1) + [delta]B
            svals.append(s0 + j * delta)
            pts.append(p)
            p = E._add(p, step)
        assert all(0 <= s < L for s in svals)
        probe = sorted({0, 1, n - 2, n - 1, *range(0, n, 1024)})
        for j, s in enumerate(svals):                         # item j has the digits it claims
            _check_sweep_digits(kind, bits, j, s)
        it = identity_items(f"r{bits} {kind}", svals, [f"j={j}" for j in range(n)], encode_batch(pts))
        for j in probe:                                       # the incremental R against the oracle
            assert E.verify(IDENT_KEY, b"", bytes(it.sig[j])), (kind, bits, j)
        out[kind] = it
    return out


def single_digit_probes(j):
    """For the first failing j of a 16-bit sweep: per window w below the top the
    values j 2^(16 w) (digit +j alone) and 2^(16 (w+1)) - j 2^(16 w) (digit -j
    under a 1), as identity-key items with their (w, sign j) labels."""
    svals, labels = [], []
    for w in range(15):
        svals.append(j << (16 * w))
        labels.append((w, +j))
        if 0 < j < 32768:
            svals.append((1 << (16 * (w + 1))) - (j << (16 * w)))
            labels.append((w, -j))
    if j <= 0x1000:
        svals.append(j << 240)
        labels.append((15, +j))
    return identity_items(f"single digit {j}", svals, [f"(w, digit) = {lb}" for lb in labels]), labels


# ----------------------------------------------------------- torsion keys
def torsion_edge_values():
    """about 32 of the edge values: L - 1, the ripples of both radices, every
    window at once, and a carry run below a window boundary"""
    pick = [(lb, v) for lb, v in edges_labelled()
            if lb in ("0", "1", "L-1", "L-2^125", "2^252-1", "2^252") or "ripple" in lb
            or "all windows = half" in lb or "all windows = full-1" in lb
            or lb in ("r16 2^(16*8) - half", "r16 2^(16*15) - (half+1)", "r8 2^(8*16) - half", "r8 2^(8*31) - 1",
                      "r16 window 14 = half", "r8 window 30 = half+1")]
    assert 28 <= len(pick) <= 36, len(pick)
    return pick


def _craft(pub, a_point, s, r_encs, tors, tag):
    """(msg, R) with encode([s]B + t) = R valid for key bytes pub (a torsion
    point a_point): t = -[h]A for h = H(R || pub || msg), over the eight t and
    at most 200 message counters"""
    neg = [E.point_mul(k, E.point_neg(a_point)) for k in range(8)]      # [h](-A) depends on h mod 8 only
    for c in range(200):
        msg = b"chosen S %s #%d" % (tag, c)
        for t, enc in zip(tors, r_encs):
            if enc == bytes(32):
                continue                                      # the one R a zeroed table entry would also produce
            h = E.sc_reduce(hashlib.sha512(enc + pub + msg).digest())
            if neg[h % 8] == t:
                return msg, enc
    raise AssertionError(f"no valid signature within 200 counters: {tag.decode()}")


@functools.lru_cache(maxsize=None)
def torsion_items():
    """Items whose [h](-A) is not the identity: every non-identity torsion key
    with each of torsion_edge_values(), the non-canonical encodings y + p of
    small-order keys with eight of them, all valid (E.verify), and per item a
    sibling with the message changed (verdict from E.verify)."""
    tors = E.small_order_points()
    keys = [(E.encode_point(t), t) for t in tors if t != E.IDENT]
    assert len(keys) == 7
    nonc = []
    for y0 in range(19):
        for sgn in (0, 1):
            enc = ((y0 + P) | (sgn << 255)).to_bytes(32, "little")
            a = E.decode_point(enc)
            if a is not None and E.point_mul(8, a) == E.IDENT:
                nonc.append((enc, a))
    assert len(nonc) >= 3
    picked = torsion_edge_values()
    pubs, sigs, msgs, want, svals, labels = [], [], [], [], [], []
    for si, (lb, s) in enumerate(picked):
        sb = E._affine(mul_b_ext(s))
        r_encs = [E.encode_point(E.point_add(sb, t)) for t in tors]
        for ki, (pub, a) in enumerate(keys + (nonc if si % 4 == 0 else [])):
            msg, enc = _craft(pub, a, s, r_encs, tors, b"%d/%d" % (si, ki))
            sig = enc + s.to_bytes(32, "little")
            for m in (msg, msg + b"!"):
                ok = E.verify(pub, m, sig)
                assert ok or m is not msg, (lb, ki)
                pubs.append(pub)
                sigs.append(sig)
                msgs.append(m)
                want.append(ok)
                svals.append(s)
                labels.append(f"key {pub.hex()[:8]}.. {'sibling ' if m is not msg else ''}{lb}")
    want = np.array(want, np.uint8)
    assert want[0::2].all()
    assert 3 * int((want[1::2] == 0).sum()) >= len(want) // 2, "too few rejected siblings"
    return Items("torsion", _rows(pubs, 32), _rows(sigs, 64), want, svals, labels, msgs)
