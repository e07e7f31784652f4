"""Host side of the SymmSHE ciphertext product (*) of any degree (include/lolhip.h lolhip_ct_mul_rule,
lolhip_ct_mul_work_len, lolhip_ct_mul_batch): no GPU needed.

 - the new entries are exported, declared and bound;
 - lolhip_ct_mul_rule equals the restatement of tests/ctmul_ref.py for all four encoding pairs, and refuses what the
   reference has no inverse for;
 - every status of lolhip_ct_mul_batch on host-only plans, in the order the header states, the output untouched;
 - lolhip_ct_mul_work_len equals the restated layout;
 - the kernel's lazy accumulator, replayed in Python integers at the interval lol_amd/csrc/ctmul.h states, stays below
   q 2^64 (what rem128 needs) at the top of every modulus class, and would not with one more term;
 - the restatement itself against decryption in the CPU SHE model: a product of three ciphertexts decrypts to the
   product of the plaintexts.
"""
import ctypes as C
import os
import re
from math import gcd, prod

import numpy as np
import pytest

import ctmul_ref as cm
import public_ref as pr
import saturate as sat
from oracle import lolmath as lm
from oracle import she_model as sm
from oracle.oracle import Params
from test_rns_width_host import mixed16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lolhip_ct_mul_rule", "lolhip_ct_mul_work_len", "lolhip_ct_mul_batch")
INVALID, MODULUS, NO_CRT, NO_DEVICE = -1, -2, -3, -5
SENT = 0x5A5A5A5A
ENC = ("LSD", "MSD")


def test_ctmul_entries_are_exported_declared_and_bound(lolhip):
    hdr = open(os.path.join(ROOT, "include", "lolhip.h")).read()
    names = set(re.findall(r"LOLHIP_API\s+[\w\s\*]+?\b(\w+)\s*\(", hdr))
    raw = C.CDLL(lolhip.lib_path())
    for nm in NEW:
        assert nm in names, f"include/lolhip.h does not declare {nm}"
        assert hasattr(raw, nm), f"liblolhip.so does not export {nm}"
    for nm in ("ctMulRule", "ctMul", "keySwitchLinear", "keySwitchQuadCirc"):
        assert callable(getattr(lolhip.Plan, nm))
    for nm in ("embedCT", "twaceCT"):
        assert callable(getattr(lolhip.Ext, nm))
    assert int(re.search(r"#define\s+LOLHIP_CT_MUL_MAX\s+(\d+)", hdr).group(1)) == cm.MAX == 8


# ---------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------
def _rule_raw(lolhip, P, p, e1, k1, l1, e2, k2, l2):
    """(status, alpha, enc, k, l) of the raw entry over sentinel outputs"""
    al = (C.c_int64 * P.T)(*[SENT] * P.T)
    e, k, l = C.c_int(SENT), C.c_int64(SENT), C.c_int64(SENT)
    rc = lolhip.lib().lolhip_ct_mul_rule(P._h, p, e1, k1, l1, e2, k2, l2, al, C.byref(e), C.byref(k), C.byref(l))
    return rc, list(al), e.value, k.value, l.value


@pytest.mark.parametrize("T", [1, 3])
def test_rule_equals_the_restatement(lolhip, T):
    m = 32
    qs = mixed16(m)[4:4 + T] if T > 1 else [lm.first_good_q(m, 2 ** 30)]
    P = lolhip.Plan(lm.factor_pps(m), qs, host_only=True)
    for p in (3, 5, 16, 257):
        assert gcd(prod(qs), p) == 1
        for e1 in (0, 1):
            for e2 in (0, 1):
                for k1, k2 in ((0, 0), (1, 3), (3, 1), (0, 3)):
                    for l1, l2 in ((1, 1), (p - 1, 2 % p), (2 % p, p - 1), (p - 1, p - 1)):
                        want = cm.rule(qs, p, ENC[e1], k1, l1, ENC[e2], k2, l2)
                        rc, al, e, k, l = _rule_raw(lolhip, P, p, e1, k1, l1, e2, k2, l2)
                        assert rc == 0
                        assert (al, ENC[e], k, l) == ([int(x) for x in want[0]], *want[1:])
                        got = P.ctMulRule(p, ENC[e1], k1, l1, ENC[e2], k2, l2)
                        assert (list(got[0]), *got[1:]) == (al, ENC[e], k, l)
    # the rule in words
    al, e, k, l = P.ctMulRule(5, "MSD", 1, 2, "MSD", 3, 4)
    zp = pow(-prod(qs) % 5, -1, 5)
    assert (list(al), e, k, l) == ([5 % q for q in qs], "MSD", 5, 2 * zp * 4 % 5)
    assert P.ctMulRule(5, "LSD", 0, 1, "LSD", 0, 1)[1:] == ("LSD", 1, 1)
    assert P.ctMulRule(5, "LSD", 0, 1, "MSD", 0, 1)[1] == P.ctMulRule(5, "MSD", 0, 1, "LSD", 0, 1)[1] == "MSD"


def test_rule_refuses_what_has_no_inverse(lolhip):
    qs = [97, 193]                                               # Q = 97 * 193, both 1 mod 32
    P = lolhip.Plan(lm.factor_pps(32), qs, host_only=True)
    untouched = ([SENT] * 2, SENT, SENT, SENT)
    for e1 in (0, 1):
        for e2 in (0, 1):
            rc, *outs = _rule_raw(lolhip, P, 97 * 2, e1, 0, 1, e2, 0, 1)        # gcd(Q, p) = 97
            if e1 == 1 and e2 == 1:
                assert rc == MODULUS and tuple(outs) == untouched
                with pytest.raises(ValueError):
                    cm.rule(qs, 97 * 2, "MSD", 0, 1, "MSD", 0, 1)
            else:                                                # no toLSD: such a p is accepted
                assert rc == 0 and outs[0] == [1, 1]
                assert tuple(outs[1:]) == (e1 | e2, 1, 1)
            for p in (1, 0, -3, 2 ** 62):
                rc, *outs = _rule_raw(lolhip, P, p, e1, 0, 1, e2, 0, 1)
                assert rc == MODULUS and tuple(outs) == untouched
    assert _rule_raw(lolhip, P, 5, 2, 0, 1, 0, 0, 1)[0] == INVALID
    assert _rule_raw(lolhip, P, 5, 0, -1, 1, 0, 0, 1)[0] == INVALID
    L = lolhip.lib()
    e, k, l = C.c_int(0), C.c_int64(0), C.c_int64(0)
    assert L.lolhip_ct_mul_rule(None, 5, 0, 0, 1, 0, 0, 1, (C.c_int64 * 2)(), C.byref(e), C.byref(k), C.byref(l)) == INVALID
    assert L.lolhip_ct_mul_rule(P._h, 5, 0, 0, 1, 0, 0, 1, None, C.byref(e), C.byref(k), C.byref(l)) == INVALID


# ---------------------------------------------------------------------------------------------
# statuses and the work length
# ---------------------------------------------------------------------------------------------
def test_every_status_on_host_only_plans_in_order(lolhip):
    L = lolhip.lib()
    g = lm.good_qs(64, 2 ** 30)
    qs = [next(g), next(g)]
    hi = lolhip.Plan.for_index(64, qs, host_only=True)
    ncrt = lolhip.Plan.for_index(64, [2 ** 20, 2 ** 21 + 1], host_only=True)
    g = lm.good_qs(64, 2 ** 30)
    wide = lolhip.Plan.for_index(64, [next(g) for _ in range(17)], host_only=True)
    B = 2
    a = np.zeros((3, B, hi.n, hi.T), dtype=np.int64)
    b = np.zeros((3, B, hi.n, hi.T), dtype=np.int64)
    out = np.full((5, B, hi.n, hi.T), SENT, dtype=np.int64)
    work = np.zeros(6 * B * hi.n * hi.T, dtype=np.int64)
    al = (C.c_int64 * 17)(*[1] * 17)
    P = lambda x: None if x is None else x.ctypes.data

    def mul(pq=hi, x=a, na=3, y=b, nb=3, crt=0, alpha=al, o=out, ocrt=0, w=work, Bn=B):
        return L.lolhip_ct_mul_batch(pq._h if pq else None, None, P(x), na, P(y), nb, crt, alpha, P(o), ocrt, P(w), Bn)

    # LOLHIP_ERR_INVALID first: it wins over a missing CRT basis and over the missing device
    for pq in (hi, ncrt):
        assert mul(pq=None) == INVALID
        assert mul(pq=pq, na=0) == INVALID and mul(pq=pq, na=9) == INVALID
        assert mul(pq=pq, nb=0) == INVALID and mul(pq=pq, nb=9) == INVALID and mul(pq=pq, nb=-1) == INVALID
        assert mul(pq=pq, Bn=-1) == INVALID
        assert mul(pq=pq, x=None) == INVALID and mul(pq=pq, y=None) == INVALID and mul(pq=pq, o=None) == INVALID
        assert mul(pq=pq, w=None) == INVALID                     # the powerful-basis route needs its work buffer
        assert mul(pq=pq, o=a) == INVALID and mul(pq=pq, o=b) == INVALID     # the output cannot alias an input
        assert mul(pq=pq, x=a, y=a, o=a) == INVALID
    assert mul(pq=wide) == INVALID                               # T > 16
    # then LOLHIP_ERR_NO_CRT, before the device is asked for
    assert mul(pq=ncrt) == NO_CRT and mul(pq=ncrt, crt=1, ocrt=1) == NO_CRT and mul(pq=ncrt, Bn=0) == NO_CRT
    # then LOLHIP_ERR_NO_DEVICE: every argument is fine
    assert mul() == NO_DEVICE and mul(crt=1, w=None) == NO_DEVICE and mul(alpha=None) == NO_DEVICE
    assert mul(y=a) == NO_DEVICE and mul(na=1, nb=8) == NO_DEVICE and mul(na=8, nb=8) == NO_DEVICE
    assert mul(Bn=0, x=None, y=None, o=None, w=None) == NO_DEVICE
    assert (out == SENT).all()
    # the Python layer makes the same checks first
    with pytest.raises(lolhip.NoDeviceError):
        hi.ctMul((a, "LSD", 0, 1), (b, "MSD", 0, 1), p=3)
    with pytest.raises(lolhip.NoDeviceError):
        hi.ctMul((a, "LSD", 0, 1), p=3, cs_crt=True)
    with pytest.raises(lolhip.LolHipError) as e:
        hi.ctMul((a, "MSD", 0, 1), (b, "MSD", 0, 1), p=qs[0])      # the rule's status: gcd(Q, p) != 1
    assert e.value.code == MODULUS
    with pytest.raises(lolhip.LolHipError) as e:
        ncrt.ctMul((a, "LSD", 0, 1), p=3)
    assert e.value.code == NO_CRT


def test_work_len_equals_the_restated_layout(lolhip):
    L = lolhip.lib()
    qs = mixed16(96)[:3]
    P = lolhip.Plan.for_index(96, qs, host_only=True)
    for na, nb in ((1, 1), (2, 2), (3, 2), (8, 8)):
        for crt in (0, 1):
            for sq in ((0, 1) if na == nb else (0,)):
                for B in (0, 1, 5):
                    want = cm.work_len(P.n, P.T, na, nb, crt, sq, B)
                    assert L.lolhip_ct_mul_work_len(P._h, na, nb, crt, sq, B) == want
    assert cm.work_len(P.n, P.T, 3, 2, 0, 0, 5) == 5 * 5 * 32 * 3 and cm.work_len(P.n, P.T, 8, 8, 0, 1, 1) == 8 * 32 * 3
    assert L.lolhip_ct_mul_work_len(None, 2, 2, 0, 0, 1) == INVALID
    assert L.lolhip_ct_mul_work_len(P._h, 0, 2, 0, 0, 1) == INVALID and L.lolhip_ct_mul_work_len(P._h, 2, 9, 0, 0, 1) == INVALID
    assert L.lolhip_ct_mul_work_len(P._h, 2, 2, 0, 0, -1) == INVALID
    assert L.lolhip_ct_mul_work_len(P._h, 3, 2, 0, 1, 1) == INVALID          # a square has na = nb


# ---------------------------------------------------------------------------------------------
# the lazy accumulator
# ---------------------------------------------------------------------------------------------
def test_accumulator_replay_stays_below_the_bound_of_rem128():
    """k_ct_mul adds raw products (each below q^2) into a 128-bit accumulator and reduces it when it holds
    LOLHIP_CT_MUL_LAZY terms and another arrives; rem128 needs its argument below q 2^64.  Replayed for na = nb = 8
    with every residue q - 1: the bound holds at the top of every class, and one more term would break it at 2^62."""
    lazy = cm.lazy_interval()
    src = open(os.path.join(ROOT, "lol_amd", "csrc", "ctmul.hip")).read()
    assert "constexpr int LAZY = LOLHIP_CT_MUL_LAZY;" in src and "cnt == LAZY" in src
    m = 32
    for kind in ("62", "61", "32"):
        q = sat.class_top(m, kind)[0]
        assert lazy * q * q <= q * 2 ** 64                       # the inequality the comment states
        for na, nb in ((8, 8), (4, 5), (1, 8), (3, 3)):
            assert cm.replay(q, na, nb, lazy) < q * 2 ** 64
            if na == nb:
                assert cm.replay(q, na, nb, lazy, square=True) < q * 2 ** 64
        # a product of two 8-component operands does reach the interval: the schedule is exercised, not vacuous
        assert cm.replay(q, 8, 8, lazy) >= lazy * (q - 1) ** 2
    q = sat.class_top(m, "62")[0]
    assert cm.replay(q, 8, 8, lazy + 1) >= q * 2 ** 64
    # without any reduction the 8 terms of the middle coefficient do not fit at 2^62: a fixed "8 terms fit" would be wrong
    assert cm.replay(q, 8, 8, 8) >= q * 2 ** 64


# ---------------------------------------------------------------------------------------------
# the restatement against decryption in the CPU SHE model
# ---------------------------------------------------------------------------------------------
def _stack(ct):
    return dict(ct, c=np.stack(ct["c"]))


@pytest.mark.parametrize("msd", [(False, False, False), (True, True, False), (True, False, True)])
def test_restated_product_of_three_decrypts_to_the_plaintext_product(cpuref, msd):
    m, p = 32, 5
    pps = lm.factor_pps(m)
    g = lm.good_qs(m, 2 ** 30)
    qs = [next(g), next(g)]
    rng = np.random.default_rng(5)
    P = Params(pps, qs)
    she = sm.SHE(sm.CpuEngine(cpuref, P), sm.CpuEngine(cpuref, pr.params(m, [p])), qs, p, rng)
    she.keygen()
    pts = [rng.integers(0, p, size=(2, P.n), dtype=np.int64) for _ in range(3)]
    cts = [she.toMSD(she.encrypt(x)) if f else she.encrypt(x) for x, f in zip(pts, msd)]
    c12 = cm.ct_mul(cpuref, P, _stack(cts[0]), _stack(cts[1]), p)
    assert len(c12["c"]) == 3 and c12["k"] == 1
    lin = she.mul(cts[0], cts[1])                                 # the model's own linear x linear product
    assert np.array_equal(c12["c"], np.stack(lin["c"])) and (c12["enc"], c12["k"], c12["l"]) == (lin["enc"], lin["k"], lin["l"])
    c123 = cm.ct_mul(cpuref, P, c12, _stack(cts[2]), p)
    assert len(c123["c"]) == 4 and c123["k"] == 2
    want = np.stack([pr.negacyclic(pr.negacyclic(pts[0][i], pts[1][i], p), pts[2][i], p) for i in range(2)]).astype(np.int64)
    assert np.array_equal(she.decrypt(dict(c123, c=list(c123["c"]))), want)
