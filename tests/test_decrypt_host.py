"""Host side of SymmSHE errorTerm / decrypt (include/lolhip.h): no GPU needed.

 - a host-only plan refuses both entries (no CPU fallback);
 - the plan's lift constants (lolhip_plan_table 12: the Garner inverses, q_j mod q_i and the mixed-radix digits
   of floor((Q-1)/2)) equal a Python big-integer derivation;
 - the new declarations are exported (the header-driven export test sees them as well).
"""
import ctypes as C
import os
import re
from math import prod

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lolhip_decrypt_work_len", "lolhip_error_term_batch", "lolhip_decrypt_batch")


def test_host_only_plan_refuses_error_term_and_decrypt(lolhip):
    pq = lolhip.Plan([(2, 4)], [17, 97], host_only=True)
    pp = lolhip.Plan([(2, 4)], [16], host_only=True)
    cs = np.zeros((2, 1, pq.n, 2), dtype=np.int64)
    s_crt = np.zeros((pq.n, 2), dtype=np.int64)
    with pytest.raises(lolhip.NoDeviceError):
        pq.errorTerm(cs, s_crt, 16)
    with pytest.raises(lolhip.NoDeviceError):
        pq.errorTerm(list(cs), s_crt, 16, enc="MSD", cs_crt=True)
    with pytest.raises(lolhip.NoDeviceError):
        pq.decrypt(cs, s_crt, pp)
    with pytest.raises(lolhip.NoDeviceError):
        pq.decrypt(cs, s_crt, pp, ext=lolhip.Ext(lolhip.Plan([(2, 2)], [16], host_only=True), pp), k=1)


def _moduli(m, bits, T):
    """T distinct primes = 1 mod m just above 2^(bits-1)"""
    import lol_amd
    out, lo = [], 2 ** (bits - 1)
    for _ in range(T):
        q = lol_amd.good_q(m, lo)
        out.append(q)
        lo = q
    return out


def _want(qs):
    T, Q = len(qs), prod(qs)
    pinv = [1 % qs[0]] + [pow(prod(qs[:i]) % qs[i], -1, qs[i]) for i in range(1, T)]
    qmod = [[qs[j] % qs[i] for j in range(T)] for i in range(T)]
    h, half = (Q - 1) // 2, []
    for q in qs:
        half.append(h % q)
        h //= q
    assert h == 0
    return pinv, qmod, half


@pytest.mark.parametrize("T", [1, 2, 4, 16])
@pytest.mark.parametrize("bits", [20, 30, 59, 61])
def test_lift_constants_equal_big_integer_derivation(lolhip, T, bits):
    m = 16
    qs = _moduli(m, bits, T)
    P = lolhip.Plan([(2, 4)], qs, host_only=True)
    got = P.liftConsts()
    pinv, qmod, half = _want(qs)
    assert [int(x) for x in got["pinv"]] == pinv
    assert [[int(x) for x in row] for row in got["qmod"]] == qmod
    assert [int(x) for x in got["half"]] == half
    # the digits really are those of (Q-1)/2 in the mixed radix q_0, q_1, ...
    Q = prod(qs)
    assert sum(int(d) * prod(qs[:i]) for i, d in enumerate(got["half"])) == (Q - 1) // 2


def test_lift_constants_of_mixed_sizes(lolhip):
    """moduli of different sizes in one plan, largest first: q_j mod q_i is a real reduction here"""
    qs = _moduli(16, 61, 1) + _moduli(16, 20, 1) + _moduli(16, 59, 1) + _moduli(16, 30, 1)
    got = lolhip.Plan([(2, 4)], qs, host_only=True).liftConsts()
    pinv, qmod, half = _want(qs)
    assert [int(x) for x in got["pinv"]] == pinv
    assert [[int(x) for x in row] for row in got["qmod"]] == qmod
    assert [int(x) for x in got["half"]] == half


def test_decrypt_entries_are_exported_and_declared(lolhip):
    hdr = open(os.path.join(ROOT, "include", "lolhip.h")).read()
    names = set(re.findall(r"LOLHIP_API\s+[\w\s\*]+?\b(\w+)\s*\(", hdr))
    raw = C.CDLL(lolhip.lib_path())
    for nm in NEW:
        assert nm in names, f"include/lolhip.h does not declare {nm}"
        assert hasattr(raw, nm), f"liblolhip.so does not export {nm}"


def test_decrypt_work_len(lolhip):
    L = lolhip.lib()
    pq = lolhip.Plan([(2, 4)], [17, 97], host_only=True)
    n, T = pq.n, pq.T
    for ncs, B in ((1, 3), (2, 3), (3, 5), (4, 1)):
        assert L.lolhip_decrypt_work_len(pq._h, ncs, B) == max(ncs - 1, 1) * B * n * T + B * n
    assert L.lolhip_decrypt_work_len(pq._h, 0, 1) == -1          # LOLHIP_ERR_INVALID
