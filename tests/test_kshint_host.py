"""Host side of the key-switch and tunnel hints (include/lolhip.h lolhip_kshint_batch, lolhip_tunnel_hint_batch): no
GPU needed.

 - the new declarations are exported (the header-driven export test sees them as well);
 - the work lengths follow the formula of the header;
 - a host-only plan (or extension) refuses both entries with LOLHIP_ERR_NO_DEVICE and writes nothing;
 - the restated domain-3 / domain-4 streams of tests/kshint_ref.py are the block function at chosen (item, block) pairs.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import enc_ref as er
import kshint_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lolhip_kshint_work_len", "lolhip_kshint_batch", "lolhip_tunnel_hint_work_len", "lolhip_tunnel_hint_batch")
SENT = 0x5A5A5A5A


def test_kshint_entries_are_exported_and_declared(lolhip):
    hdr = open(os.path.join(ROOT, "include", "lolhip.h")).read()
    names = set(re.findall(r"LOLHIP_API\s+[\w\s\*]+?\b(\w+)\s*\(", hdr))
    raw = C.CDLL(lolhip.lib_path())
    for nm in NEW:
        assert nm in names, f"include/lolhip.h does not declare {nm}"
        assert hasattr(raw, nm), f"liblolhip.so does not export {nm}"


def test_kshint_work_len(lolhip):
    L = lolhip.lib()
    p16 = lolhip.Plan([(2, 4)], [17, 97], host_only=True)           # 2-power: the residue slab only
    for base in (0, 2, 5):
        nL = p16.decomposeLen(base)
        assert L.lolhip_kshint_work_len(p16._h, base, 3) == 3 * nL * p16.n * 2
    p45 = lolhip.Plan([(3, 2), (5, 1)], [181, 271, 541], host_only=True)
    nL = p45.decomposeLen(16)
    assert L.lolhip_kshint_work_len(p45._h, 16, 5) == 5 * nL * p45.n * (3 + 1)     # + the double slab of the map
    assert L.lolhip_kshint_work_len(p16._h, 0, -1) == -1               # LOLHIP_ERR_INVALID
    assert L.lolhip_kshint_work_len(p16._h, 1, 1) == -1                # base 1


def test_tunnel_hint_work_len(lolhip):
    L = lolhip.lib()
    qs = [1021, 1201]                                                    # primes = 1 mod lcm(12, 20)
    PE, PR, PS = (lolhip.Plan.for_index(m, qs, host_only=True) for m in (4, 12, 20))
    XR, XS = lolhip.Ext(PE, PR), lolhip.Ext(PE, PS)
    rel, T = PR.n // PE.n, 2
    for base in (0, 16):
        nL = PS.decomposeLen(base)
        lin = rel * PR.n * T + rel * rel * (PE.n + PS.n) * T
        ks = rel * nL * PS.n * (T + 1)
        assert L.lolhip_tunnel_hint_work_len(XR._h, XS._h, base) == rel * PS.n * T + max(lin, ks)
    assert L.lolhip_tunnel_hint_work_len(XR._h, XS._h, -3) == -1


def test_host_only_plan_refuses_hints_and_leaves_output(lolhip):
    L = lolhip.lib()
    pq = lolhip.Plan([(2, 4)], [17, 97], host_only=True)
    nL = pq.decomposeLen(0)
    s_crt = np.zeros((pq.n, 2), dtype=np.int64)
    vals = np.zeros((1, pq.n, 2), dtype=np.int64)
    out = np.full((1, nL, 2, pq.n, 2), SENT, dtype=np.int64)
    work = np.zeros(L.lolhip_kshint_work_len(pq._h, 0, 1), dtype=np.int64)
    rc = L.lolhip_kshint_batch(pq._h, None, s_crt.ctypes.data, vals.ctypes.data, 1.0, 0, bytes(32), 0, out.ctypes.data,
                               work.ctypes.data, 1)
    assert rc == lolhip.tensor.ERR_NO_DEVICE
    assert (out == SENT).all()
    with pytest.raises(lolhip.NoDeviceError):
        pq.ksHint(s_crt, vals, 1.0, 0, key=bytes(32))
    with pytest.raises(lolhip.NoDeviceError):
        pq.ksQuadCircHint(s_crt, 1.0, 0)
    qs = [1021, 1201]
    PE, PR, PS = (lolhip.Plan.for_index(m, qs, host_only=True) for m in (4, 12, 20))
    XR, XS = lolhip.Ext(PE, PR), lolhip.Ext(PE, PS)
    rel = PR.n // PE.n
    ys = np.zeros((rel, PS.n, 2), dtype=np.int64)
    hints = np.full((rel, PS.decomposeLen(0), 2, PS.n, 2), SENT, dtype=np.int64)
    work = np.zeros(L.lolhip_tunnel_hint_work_len(XR._h, XS._h, 0), dtype=np.int64)
    s_in, s_out = np.zeros((PR.n, 2), dtype=np.int64), np.zeros((PS.n, 2), dtype=np.int64)
    rc = L.lolhip_tunnel_hint_batch(XR._h, XS._h, None, ys.ctypes.data, s_in.ctypes.data, s_out.ctypes.data, 1.0, 0,
                                    bytes(32), 0, hints.ctypes.data, work.ctypes.data)
    assert rc == lolhip.tensor.ERR_NO_DEVICE
    assert (hints == SENT).all()


@pytest.mark.parametrize("domain", [kr.DOM_HINT_GAUSS, kr.DOM_HINT_UNIFORM])
def test_restated_hint_streams_are_the_block_function(lolhip, domain):
    """item i = ctr + b L + j: nonce (domain, lo32(i), hi32(i)), counter = block"""
    key = bytes(range(7, 39))
    ctr, nL = 2 ** 32 - 5, 3                                            # items carry into the high nonce word
    w = er.stream(key, domain, ctr, 4 * nL, 6)
    for b, j, k in [(0, 0, 0), (0, 2, 5), (1, 1, 3), (3, 2, 1)]:
        i = ctr + b * nL + j
        got = lolhip.chacha20_block(key, k, [domain, i & 0xFFFFFFFF, i >> 32])
        assert np.array_equal(w[b * nL + j, k], got)
    # the residues of kshint_ref.uniform_crt: residue r of a row from block r >> 2, words 4(r & 3) ..
    qs = [97, 2 ** 61 - 1]
    u = kr.uniform_crt(key, domain, ctr, 2, 8, qs)
    blk = lolhip.chacha20_block(key, 1, [domain, (ctr + 1) & 0xFFFFFFFF, (ctr + 1) >> 32])
    for r in range(4, 8):
        v = sum(int(blk[4 * (r & 3) + i]) << (32 * i) for i in range(4))
        assert u[1, r // 2, r % 2] == v % qs[r % 2]
