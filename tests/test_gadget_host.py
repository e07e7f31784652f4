"""Host side of gadget error correction (lolhip_gadget_correct_*, lolhip_gadget_encode_batch, Plan.gadgetCorrect /
gadgetEncode): the big-integer restatement (tests/gadget_ref.py) recovers (s, e) from every noisy encoding within the
error cap, so a GPU failure points at the kernel; its intermediates stay inside the bound DESIGN.md 3.4j proves, on
random inputs and on the extremal ones the proof names; the symbols are declared, exported and bound; every status
code.  No GPU: host-only plans."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import gadget_ref as gr
from oracle import lolmath as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, MODULUS, NO_CRT, NO_DEVICE = 0, -1, -2, -3, -5
DEC, POW, CRT = 0, 1, 2
Q60 = 2 ** 60 + 147457
SINGLE = [(257, 2), (257, 3), (12289, 4), (12289, 256), (1073479681, 2), (Q60, 2), (Q60, 256), (7681, 7681), (7681, 10000)]
PAIR = (12289, 7681)


def _plan(lolhip, m, qs):
    return lolhip.Plan(lm.factor_pps(m), list(qs), host_only=True)


def _errors(rng, cap, k):
    return [rng.choice([-cap, cap, rng.randint(-cap, cap)]) for _ in range(k)] if cap > 0 else [0] * k


@pytest.mark.parametrize("q,b", SINGLE)
def test_restatement_round_trip(q, b):
    rng = random.Random(q * 31 + b)
    k, cap = gr.gadlen(b, q), gr.error_cap(b, q)
    g = [row[0] for row in gr.gadget(b, [q])]
    assert len(g) == k and g == [pow(b, i, q) for i in range(k)]
    for _ in range(3000):
        s, e = rng.randrange(q), _errors(rng, cap, k)
        if k == 1:
            e = [0]                                           # one digit carries no redundancy: u = xs_0, e = [0]
        xs = [(g[i] * s + e[i]) % q for i in range(k)]
        assert gr.correct1(b, q, xs) == (s, e)


@pytest.mark.parametrize("base", [0, 2, 16])
def test_restatement_round_trip_pair(base):
    rng = random.Random(base)
    qs = list(PAIR)
    g = gr.gadget(base, qs)
    L = len(g)
    cap = 0 if base == 0 else gr.error_cap(base, min(qs))
    for _ in range(1000):
        s = [rng.randrange(q) for q in qs]
        e = _errors(rng, cap, L)
        xs = gr.encode(base, qs, [s], None if base == 0 else [[v] for v in e])
        u, es = gr.correct(base, qs, xs)
        assert [int(v) for v in u[0]] == s                    # base 0: only u is defined by the encoding
        if base:
            assert [int(es[j, 0]) for j in range(L)] == e


def _extremal(q, b):
    """the inputs the proof names: every v_i at +-floor(q/2), with the signs that push each w_i, and so x and the
    y_i, to one side; the constant vectors; and the alternating ones"""
    k, h = gr.gadlen(b, q), q // 2
    lo = (q + 1) // 2                                         # the residue whose lift is the most negative
    pats = [[h] * k, [lo] * k, [h if i % 2 == 0 else lo for i in range(k)], [lo if i % 2 == 0 else h for i in range(k)],
            [0] * k, [q - 1] * k, [1] * k]
    for cut in range(k):
        pats.append([h] * cut + [lo] * (k - cut))
        pats.append([lo] * cut + [h] * (k - cut))
    return pats


@pytest.mark.parametrize("q,b", SINGLE + [(256, 2), (255, 4), (2 ** 31 - 1, 2), (2 ** 31 - 1, 7)])
def test_intermediates_stay_inside_the_proven_bound(q, b):
    rng = random.Random(q + b)
    k, B = gr.gadlen(b, q), gr.bound(b, q)
    assert B["need"] < 2 ** 63 and gr.in_domain(b, [q])
    worst = 0
    cases = _extremal(q, b) + [[rng.choice([0, q - 1, q // 2, q // 2 + 1, q // 2 - 1, rng.randrange(q)]) for _ in range(k)]
                               for _ in range(2000)]
    for xs in cases:
        tr = {}
        gr.correct1(b, q, xs, tr)
        if k == 1:
            continue
        assert all(abs(w) <= B["W"] for w in tr["w"])
        assert all(abs(y) <= Y for y, Y in zip(tr["y"], B["Y"])) and abs(tr["x"]) <= B["Y"][0]
        assert abs(tr["s"]) <= B["S"]
        assert all(abs(v) <= B["E"] for v in tr["vp"] + tr["e"])
        worst = max(worst, max(abs(v) for v in tr["vp"] + tr["e"] + tr["y"]))
    print(f"q={q} b={b}: k={k} W={B['W']} E={B['E'] / q:.3f} q, largest seen {worst / q:.3f} q")


def test_domain_admits_the_flagship_and_refuses_what_overflows():
    assert gr.in_domain(2, [Q60]) and gr.in_domain(256, [Q60]) and gr.in_domain(0, [Q60])
    assert not gr.in_domain(2, [2 ** 61 - 1])                 # q mod 2^j = 2^j - 1: the y_i reach k q / 2
    assert all(gr.in_domain(b, list(PAIR)) for b in (0, 2, 16))
    assert not gr.in_domain(2, [Q60, 12289])


def test_symbols_are_declared_exported_and_bound(lolhip):
    hdr = open(os.path.join(ROOT, "include", "lolhip.h")).read()
    names = set(re.findall(r"LOLHIP_API\s+[\w\s\*]+?\b(\w+)\s*\(", hdr))
    raw = C.CDLL(lolhip.lib_path())
    for nm in ("lolhip_gadget_correct_work_len", "lolhip_gadget_correct_batch", "lolhip_gadget_encode_batch"):
        assert nm in names
        assert hasattr(raw, nm)
    for nm in ("gadgetEncode", "gadgetCorrect", "gadgetCorrectWorkLen"):
        assert callable(getattr(lolhip.Plan, nm))


def _correct(lolhip, p, base, basis=DEC, B=0, ptr=None):
    return lolhip.lib().lolhip_gadget_correct_batch(p._h if p else None, None, ptr, base, basis, ptr, ptr, ptr, B)


def _encode(lolhip, p, base, B=0, ptr=None):
    return lolhip.lib().lolhip_gadget_encode_batch(p._h if p else None, None, ptr, base, None, ptr, B)


def test_statuses(lolhip):
    L = lolhip.lib()
    p1, p2 = _plan(lolhip, 32, [12289]), _plan(lolhip, 32, PAIR)
    # a valid call on a host-only plan: everything else is decided before the device is asked for
    for p in (p1, p2):
        for base in (0, 2, 16, 256):
            for basis in (DEC, POW, CRT):
                assert _correct(lolhip, p, base, basis) == NO_DEVICE
                assert _correct(lolhip, p, base, basis, B=3, ptr=8) == NO_DEVICE
            assert _encode(lolhip, p, base) == NO_DEVICE
    assert _correct(lolhip, None, 2) == INVALID and _encode(lolhip, None, 2) == INVALID
    for base in (1, -1, -(2 ** 62)):
        assert _correct(lolhip, p1, base) == INVALID
        assert _encode(lolhip, p1, base) == INVALID
        assert L.lolhip_gadget_correct_work_len(p1._h, base, DEC, 1) == INVALID
    assert _correct(lolhip, p1, 2, basis=3) == INVALID and _correct(lolhip, p1, 2, basis=-1) == INVALID
    assert _correct(lolhip, p1, 2, B=-1) == INVALID and _encode(lolhip, p1, 2, B=-1) == INVALID
    # T = 3: the class has instances for fields and pairs only; encode takes any tuple
    p3 = _plan(lolhip, 32, [12289, 7681, 257])
    assert _correct(lolhip, p3, 2) == INVALID and L.lolhip_gadget_correct_work_len(p3._h, 2, DEC, 1) == INVALID
    assert _encode(lolhip, p3, 2) == NO_DEVICE
    # the over-wide pair, a pair that is not coprime, a single modulus outside the domain
    wide = _plan(lolhip, 32, [Q60, 12289])
    assert _correct(lolhip, wide, 2) == MODULUS and L.lolhip_gadget_correct_work_len(wide._h, 2, DEC, 1) == MODULUS
    assert _correct(lolhip, wide, 0) == NO_DEVICE                                  # TrivGad: e' = [0], nothing to overflow
    assert _correct(lolhip, _plan(lolhip, 32, [12289, 12289 * 3]), 2) == MODULUS
    assert _correct(lolhip, _plan(lolhip, 32, [6, 4]), 0) == MODULUS
    assert _correct(lolhip, _plan(lolhip, 32, [2 ** 61 - 1]), 2) == MODULUS
    assert _correct(lolhip, _plan(lolhip, 32, [Q60]), 2) == NO_DEVICE and _correct(lolhip, _plan(lolhip, 32, [Q60]), 256) == NO_DEVICE
    # no CRT basis over q = 256: only the CRT entry refuses
    p256 = _plan(lolhip, 32, [256])
    assert _correct(lolhip, p256, 2, CRT) == NO_CRT and L.lolhip_gadget_correct_work_len(p256._h, 2, CRT, 1) == NO_CRT
    assert _correct(lolhip, p256, 2, POW) == NO_DEVICE and _correct(lolhip, p256, 2, DEC) == NO_DEVICE
    # the Python methods raise the same codes before they stage anything
    for call, code in ((lambda: p3.gadgetCorrect(np.zeros((1, 16, 3), dtype=np.int64), 2), INVALID),
                       (lambda: wide.gadgetCorrect(np.zeros((1, 16, 2), dtype=np.int64), 2), MODULUS),
                       (lambda: p256.gadgetCorrect(np.zeros((9, 1, 16, 1), dtype=np.int64), 2, basis="crt"), NO_CRT),
                       (lambda: p1.gadgetCorrect(np.zeros((14, 1, 16, 1), dtype=np.int64), 2), NO_DEVICE),
                       (lambda: p1.gadgetEncode(np.zeros((1, 16, 1), dtype=np.int64), 1), INVALID),
                       (lambda: p1.gadgetEncode(np.zeros((1, 16, 1), dtype=np.int64), 2), NO_DEVICE)):
        with pytest.raises(lolhip.LolHipError) as e:
            call()
        assert e.value.code == code


@pytest.mark.parametrize("qs", [[12289], list(PAIR), [Q60]])
@pytest.mark.parametrize("base", [0, 2, 256])
def test_work_len(lolhip, qs, base):
    p = _plan(lolhip, 45, qs) if qs != list(PAIR) else _plan(lolhip, 32, qs)
    Lg = p.decomposeLen(base)
    assert Lg == sum(gr.digits(base, q) for q in qs)
    for B in (0, 1, 7):
        assert p.gadgetCorrectWorkLen(base, "dec", B) == 0
        assert p.gadgetCorrectWorkLen(base, "pow", B) == Lg * B * p.n * p.T
        if p.has_crt:
            assert p.gadgetCorrectWorkLen(base, "crt", B) == Lg * B * p.n * p.T
    assert lolhip.lib().lolhip_gadget_correct_work_len(p._h, base, DEC, -1) == INVALID
    assert lolhip.lib().lolhip_gadget_correct_work_len(None, base, DEC, 1) == INVALID
