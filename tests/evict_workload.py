"""The churn workload of the key-eviction tests (tests/test_key_evict_host.py,
tests/test_key_evict_gpu.py): blocks of single-signer MsgSend txs whose signers
rotate over far more accounts than the resident size, a third of each block
repeating signers of the block before, some signatures bad; then one block
whose fresh signers outnumber every slot of the arena.  Reference codes from
tests/ante_ref.py."""
import random
import struct

import txkit as T
from ante_ref import AnteRef

CHAIN = "gv-evict"
HEIGHT = 7
FEE = T.Fee([(0, "stake")], 1000000)
RESIDENT = 512
ACCOUNTS, BLOCKS, BLOCK_TXS, REPEAT = 2000, 8, 300, 100
OVERFLOW = 600                                    # fresh signers of the last block: more than RESIDENT slots


class Key:
    def __init__(self, tag: bytes):
        self.priv = T.privkey_from_secret(b"evict-" + tag)
        self.amino = T.amino_secp(T.secp_pubkey(self.priv))
        self.addr = T.address(self.amino)

    def sign(self, msg):
        return T.secp_sign(self.priv, msg)


def workload(check_threads=0):
    """(accounts, blocks, parts, check): accounts as (addr, number, seq, stored
    pub); parts[i] = (msgs, sigs) of flat tx i for ante_ref; check: per-thread
    CheckTx txs on accounts of their own (check_threads lists)."""
    rng = random.Random(0xE71C7)
    keys = [Key(b"a%d" % i) for i in range(ACCOUNTS + OVERFLOW)]
    sink = Key(b"sink").addr
    accts = [(k.addr, 10 + i, 0, k.amino) for i, k in enumerate(keys)]
    seq = [0] * len(keys)
    blocks, parts = [], []

    def tx_of(i, t):
        k = keys[i]
        msgs = [T.MsgSend(k.addr, sink, [(1 + t % 5, "s")])]
        wrong = rng.random() < 0.03
        sb = T.std_sign_bytes(CHAIN, 10 + i, seq[i] + (2 if wrong else 0), FEE, msgs, "")
        bad = rng.random() < 0.04
        sg = [(b"", keys[(i + 1) % len(keys)].sign(sb) if bad else k.sign(sb))]
        if not (wrong or bad):
            seq[i] += 1
        parts.append((msgs, sg))
        return T.std_tx(msgs, FEE, "", sg)

    nxt, prev = 0, []
    for b in range(BLOCKS):
        signers = rng.sample(prev, REPEAT) if prev else []
        while len(signers) < BLOCK_TXS:
            signers.append(nxt % ACCOUNTS)
            nxt += 1
        rng.shuffle(signers)
        blocks.append([tx_of(i, t) for t, i in enumerate(signers)])
        prev = signers
    blocks.append([tx_of(ACCOUNTS + j, j) for j in range(OVERFLOW)])
    check = []
    for th in range(check_threads):
        ks = [Key(b"c%d-%d" % (th, j)) for j in range(4)]
        cseq, txs = [0] * 4, []
        for t in range(40):
            j = t % 4
            k = ks[j]
            msgs = [T.MsgSend(k.addr, sink, [(1, "c")])]
            sb = T.std_sign_bytes(CHAIN, 5000 + 4 * th + j, cseq[j], FEE, msgs, "")
            bad = t % 13 == 7
            txs.append(T.std_tx(msgs, FEE, "", [(k.amino, ks[(j + 1) % 4].sign(sb) if bad else k.sign(sb))]))
            cseq[j] += 0 if bad else 1
        check.append(txs)
        accts += [(k.addr, 5000 + 4 * th + j, 0, b"") for j, k in enumerate(ks)]
    return accts, blocks, parts, check


def reference_codes(accts, blocks, parts):
    ref = AnteRef(CHAIN, height=HEIGHT)
    for addr, num, sq, pub in accts:
        ref.set_account(addr, num, sq, pub)
    txs = [tx for b in blocks for tx in b]
    return [ref.ante(msgs, FEE, "", sigs, len(tx))[0] for tx, (msgs, sigs) in zip(txs, parts)], ref


def write_fixture(path, accts, blocks, check):
    """The fixture format of tests/sanitize/harness.cpp."""
    out = bytearray(b"GVSAN1")
    out += struct.pack("<I", len(CHAIN)) + CHAIN.encode() + struct.pack("<q", HEIGHT)
    out += struct.pack("<I", len(accts))
    for addr, num, sq, pub in accts:
        out += addr + struct.pack("<QQI", num, sq, len(pub)) + pub
    for group in (blocks, check):
        out += struct.pack("<I", len(group))
        for txs in group:
            out += struct.pack("<I", len(txs))
            for tx in txs:
                out += struct.pack("<I", len(tx)) + tx
    with open(path, "wb") as f:
        f.write(out)
