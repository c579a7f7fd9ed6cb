"""ed25519 items at every SHA-512 block count the kernels can see -- test
infrastructure shared by test_ed_gpu.py and test_ed_keyed_gpu.py.

SHA-512(R || A || M) pads 64 + len + 17 bytes up to a multiple of 128, so a
message of 128 j - 81 bytes is the last that fits j blocks and 128 j - 80 the
first that needs j + 1.  LENGTHS brackets that boundary for j = 1..17 (j = 16:
1967 / 1968, where edl_hash_digits in csrc/ed_lat.hip leaves the LDS-staged
sha512_wave for the byte-stream path), plus 0, 1 and 2500.

Every length gives three items of one key: the valid OpenSSL signature, the
last message byte flipped, and byte 0 flipped (the empty message has no byte
to flip: a one-byte message stands in for both).  The expected verdict is 1,
0, 0 by construction, confirmed by OpenSSL for every item and by
oracle/ed25519_ref.py on a sample of 20."""
import functools
import random

import numpy as np

import ed_openssl as OSSL
from oracle import ed25519_ref as E

LENGTHS = sorted({0, 1, 2500} | {128 * j - d for j in range(1, 18) for d in (82, 81, 80, 79)})
NKEYS = 3


@functools.lru_cache(maxsize=None)
def items():
    """(pubs, key index per item, messages, sig array n x 64, expected uint8 n)"""
    assert len(LENGTHS) == 71 and 47 in LENGTHS and 48 in LENGTHS and 1967 in LENGTHS and 1968 in LENGTHS
    rng = random.Random(0x512)
    seeds = [rng.randbytes(32) for _ in range(NKEYS)]
    pubs = [OSSL.public_key(s) for s in seeds]
    key, msgs, sigs, want = [], [], [], []
    for i, n in enumerate(LENGTHS):
        k = i % NKEYS
        m = rng.randbytes(n)
        sg = OSSL.sign(seeds[k], m)
        if n:
            last = m[:-1] + bytes([m[-1] ^ 0x80])
            first = bytes([m[0] ^ 0x01]) + m[1:]
        else:
            last, first = b"\x80", b"\x01"
        for mm, w in ((m, 1), (last, 0), (first, 0)):
            assert OSSL.verify(pubs[k], mm, sg) == bool(w), (n, w)
            key.append(k)
            msgs.append(mm)
            sigs.append(np.frombuffer(sg, np.uint8))
            want.append(w)
    for i in random.Random(20).sample(range(len(msgs)), 20):
        assert E.verify(pubs[key[i]], msgs[i], bytes(sigs[i])) == bool(want[i]), i
    return pubs, np.array(key), msgs, np.array(sigs).reshape(-1, 64), np.array(want, np.uint8)
