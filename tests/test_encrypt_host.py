"""Host side of SymmSHE encrypt / genSK (include/lolhip.h): no GPU needed.

 - lolhip_chacha20_block, the block function the sampling kernels run, against RFC 8439 (§2.3.2 and A.1) and the numpy
   restatement of tests/enc_ref.py on random inputs;
 - a host-only plan refuses both sampling entries (no CPU fallback);
 - the new declarations are exported (the header-driven export test sees them as well).
"""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import enc_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lolhip_encrypt_work_len", "lolhip_encrypt_batch", "lolhip_error_rounded_batch", "lolhip_chacha20_block")


def _serial(words):
    """the serialized block as the RFC prints it: little-endian bytes, grouped by word"""
    return [struct.pack("<I", int(w)).hex() for w in words]


def _nonce(hexwords):
    return [int.from_bytes(bytes.fromhex(h), "little") for h in hexwords]


def test_chacha20_block_rfc8439_2_3_2(lolhip):
    key = bytes(range(32))
    got = lolhip.chacha20_block(key, 1, _nonce(["00000009", "0000004a", "00000000"]))
    want = ("10f1e7e4 d13b5915 500fdd1f a32071c4 c7d1f4c7 33c06803 0422aa9a c3d46c4e "
            "d2826446 079faa09 14c2d705 d98b02a2 b5129cd1 de164eb9 cbd083e8 a2503c4e").split()
    assert _serial(got) == want


def test_chacha20_block_rfc8439_a1_vector1(lolhip):
    got = lolhip.chacha20_block(bytes(32), 0, [0, 0, 0])
    want = ("76b8e0ad a0f13d90 405d6ae5 5386bd28 bdd219b8 a08ded1a a836efcc 8b770dc7 "
            "da41597c 5157488d 7724e03f b8d84a37 6a43b8f4 1518a11c c387b669 b2ee6586").split()
    assert _serial(got) == want


def test_chacha20_block_matches_restatement(lolhip):
    rng = np.random.default_rng(8439)
    for _ in range(64):
        key = rng.bytes(32)
        ctr = int(rng.integers(0, 2 ** 32))
        nonce = [int(v) for v in rng.integers(0, 2 ** 32, size=3)]
        got = lolhip.chacha20_block(key, ctr, nonce)
        want = er.chacha20_blocks(key, ctr, *nonce)[0]
        assert np.array_equal(got, want)


def test_restated_stream_layout_is_the_block_function(lolhip):
    """tests/enc_ref.stream: item b of offset ctr = nonce (domain, lo32(ctr + b), hi32(ctr + b)), counter = block"""
    key = bytes(range(100, 132))
    ctr = 2 ** 32 - 2                                     # the item number carries into the high nonce word
    w = er.stream(key, er.DOM_UNIFORM, ctr, 4, 3)
    for b in range(4):
        nb = ctr + b
        for k in range(3):
            got = lolhip.chacha20_block(key, k, [er.DOM_UNIFORM, nb & 0xFFFFFFFF, nb >> 32])
            assert np.array_equal(w[b, k], got)


def test_host_only_plan_refuses_encrypt_and_error_rounded(lolhip):
    pq = lolhip.Plan([(2, 4)], [17, 97], host_only=True)
    pp = lolhip.Plan([(2, 4)], [16], host_only=True)
    pt = np.zeros((1, pq.n), dtype=np.int64)
    s_crt = np.zeros((pq.n, 2), dtype=np.int64)
    with pytest.raises(lolhip.NoDeviceError):
        pq.encrypt(pt, s_crt, pp, 1.0, key=bytes(32))
    with pytest.raises(lolhip.NoDeviceError):
        pq.encrypt(pt, s_crt, pp, 1.0, out_crt=True)
    with pytest.raises(lolhip.NoDeviceError):
        pq.errorRounded(1.0, B=2, key=bytes(32))


def test_encrypt_entries_are_exported_and_declared(lolhip):
    hdr = open(os.path.join(ROOT, "include", "lolhip.h")).read()
    names = set(re.findall(r"LOLHIP_API\s+[\w\s\*]+?\b(\w+)\s*\(", hdr))
    raw = C.CDLL(lolhip.lib_path())
    for nm in NEW:
        assert nm in names, f"include/lolhip.h does not declare {nm}"
        assert hasattr(raw, nm), f"liblolhip.so does not export {nm}"


def test_encrypt_work_len(lolhip):
    L = lolhip.lib()
    p16 = lolhip.Plan([(2, 4)], [17, 97], host_only=True)           # 2-power: the rep slab only
    assert L.lolhip_encrypt_work_len(p16._h, 3) == 3 * p16.n
    p45 = lolhip.Plan([(3, 2), (5, 1)], [181, 271, 541], host_only=True)
    assert L.lolhip_encrypt_work_len(p45._h, 5) == 5 * p45.n * (2 + 3)
    assert L.lolhip_encrypt_work_len(p16._h, -1) == -1               # LOLHIP_ERR_INVALID
