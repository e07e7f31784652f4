"""Whole RLWE / RLWR challenges without a GPU: the parameter layer of lol_amd/challenges.py against the reference's
parameter list (tests/golden/challenge_params.txt), the work-buffer lengths and host-decided statuses of lolhip_chall_*
and lolhip_chall_ring_* on host-only plans, and the CPU model of tests/challenge_ref.py against itself (honest
instances pass, permuted secrets and one corruption fail, the suppressed instance left out); the messages of RLWE.proto
and Challenges.proto against google.protobuf (both ways, packed and unpacked, both generations, every rejection), their
stand-alone sanitizer driver, and the tree layer (generate -> write -> read -> verify -> suppress -> verify with the
beacon's byte, regen, the reference's error messages) on the CPU model."""
import os
from collections import Counter

import numpy as np
import pytest

import challenge_ref as cf
import rlwe_ref as rr
import rlwe_ring_ref as ring

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = os.path.join(ROOT, "tests", "golden", "challenge_params.txt")
ERR_INVALID, ERR_NO_CRT, ERR_NO_DEVICE = -1, -3, -5
KEY = bytes(range(32))


@pytest.fixture(scope="module")
def ch(lolhip):
    from lol_amd import challenges
    return challenges


@pytest.fixture(scope="module")
def records(ch):
    return ch.parse_params(open(PARAMS).read())


# ---- parameter lines ----------------------------------------------------------------------------------------------------
def test_golden_list_parses_to_516_records(ch, records):
    assert len(records) == 516
    assert Counter(r.kind for r in records) == {"Cont": 228, "Disc": 228, "RLWR": 60}
    assert Counter(r.numSamples for r in records) == {3: 216, 100: 240, 500: 60}
    assert [r.challID for r in records] == list(range(516))
    assert all(r.numInstances == 32 and r.eps == 2.0 ** -25 and r.supported for r in records)
    assert all((r.svar is None) == (r.kind == "RLWR") == (r.p is not None) for r in records)
    assert ch.parse_params(open(PARAMS).read(), num_instances=16)[5].numInstances == 16
    # the list the ring-route tests classify is this list without its comment line
    assert [(r.kind, r.m, r.q, r.p if r.kind == "RLWR" else r.svar) for r in records] == ring.challenge_lines()


def test_challenge_name_is_the_printf_rule(ch, records):
    C = ch.ChallengeParams
    assert ch.challenge_name(records[0]) == "chall-id0000-rlwec-m256-q769-l3-short-toy"
    assert ch.challenge_name(C(7, "Disc", 128, 257, 0.5, None, 100, 32, "x")) == "chall-id0007-rlwed-m128-q257-l100-x"
    assert ch.challenge_name(C(515, "RLWR", 21, 500, None, 32, 500, 32, "toy")) == "chall-id0515-rlwr-m21-q500-p32-l500-toy"
    assert ch.challenge_name(C(12345, "Cont", 8, 17, 1.0, None, 3, 32, "")) == "chall-id12345-rlwec-m8-q17-l3"
    name = ch.challenge_name(records[0])
    assert ch.challenge_path("r", name) == os.path.join("r", name, name + ".challenge")
    assert ch.instance_path("r", name, 10) == os.path.join("r", name, name + "-0A.instance")
    assert ch.secret_path("r", name, 31) == os.path.join("r", name, name + "-1F.secret")
    assert ch.suppressed_secret_id(32, 0xE7) == 7 and ch.suppressed_secret_id(5, 255) == 0


def test_grammar(ch):
    text = '''-- format: challID challType m q v l annotation
      /* a /* nested */ comment */ 3 Cont 8 17 7.8125e-3 3 "a b"   4 RLWR 0x10
      17 16 100 "q\\"uote" -- trailing
      5 Disc 8 17 1e0 3 ""'''
    a, b, c = ch.parse_params(text, num_instances=4)
    assert (a.kind, a.m, a.q, a.svar, a.numSamples, a.annotation, a.numInstances) == ("Cont", 8, 17, 7.8125e-3, 3, "a b", 4)
    assert (b.kind, b.m, b.q, b.p, b.annotation) == ("RLWR", 16, 17, 16, 'q"uote') and c.annotation == "" and c.svar == 1.0
    with pytest.raises(ch.ParamsError, match="Expected p <= q; parsed q=17 and p=18"):
        ch.parse_params('0 RLWR 8 17 18 3 "x"')
    eq = ch.parse_params('0 RLWR 8 17 17 3 "x"')[0]
    assert not eq.supported                                         # p = q parses, as in the reference, and is not run
    with pytest.raises(ch.ParamsError, match="p = q is not supported"):
        ch.generate_arrays(eq, KEY)
    for bad in ('0 Cont 8 17 1 3 "x"', '0 Foo 8 17 1.0 3 "x"', '0 Cont 8 17 1.0 3', '0 Cont 8 17 1.0 3 x', '/* open'):
        with pytest.raises(ch.ParamsError):
            ch.parse_params(bad)


def test_every_line_takes_the_route_has_crt_dictates(ch, records):
    seen = {}
    for r in records:
        if (r.m, r.q) not in seen:
            seen[(r.m, r.q)] = ch.route(r)
        which, plan = seen[(r.m, r.q)]
        assert which == ("plan" if plan.has_crt else "ring")
        assert which == ("plan" if ring.is_prime(r.q) and r.q % r.m == 1 else "ring"), (r.m, r.q)
    assert Counter(w for w, _ in seen.values())["ring"] > 0 and Counter(w for w, _ in seen.values())["plan"] > 0


def test_error_bound_of_a_record(ch, records):
    c, d = records[0], records[1]
    assert ch.error_bound(c) == pytest.approx(rr.error_bound_cont(c.m, c.svar, c.eps), rel=1e-12)
    assert ch.error_bound(d) == rr.error_bound_disc(d.m, d.svar, d.eps)
    assert ch.error_bound(next(r for r in records if r.kind == "RLWR")) is None


# ---- the C entries on host-only plans -------------------------------------------------------------------------------------
def _even(x):
    return (x + 1) & ~1


@pytest.mark.parametrize("m,qs", [(32, [97]), (21, [337]), (32, [97, 193])])
def test_work_len_is_the_stated_layout(lolhip, m, qs):
    L = lolhip.lib()
    P = lolhip.Plan.for_index(m, qs, host_only=True)
    n, T = P.n, P.T
    for kind in (0, 1, 2):
        for I, ell in ((0, 1), (1, 1), (3, 5), (33, 3)):
            B = I * ell
            want = (_even(I * n * T) + _even(B * n * T) + (_even(B * n * T) if kind == 0 else 0)
                    + (0 if kind == 2 else _even(B * n)) + _even(B))
            assert L.lolhip_chall_work_len(P._h, kind, I, ell) == want
    for args in ((3, 1, 1), (-1, 1, 1), (0, -1, 1), (0, 1, 0), (0, 2 ** 31, 1), (0, 2 ** 16, 2 ** 15)):
        assert L.lolhip_chall_work_len(P._h, *args) == ERR_INVALID
    assert L.lolhip_chall_work_len(None, 0, 1, 1) == ERR_INVALID
    assert L.lolhip_chall_work_len(P._h, 0, 2 ** 31 - 1, 1) > 0


@pytest.mark.parametrize("m,q", [(32, 512), (12, 500), (32, 2 ** 61)])
def test_ring_work_len_is_the_stated_layout(lolhip, m, q):
    L = lolhip.lib()
    P = lolhip.Plan.for_index(m, [q], host_only=True)
    r = lolhip.RingRLWE(P)
    n, K = P.n, r.K
    for kind in (0, 1, 2):
        for I, ell in ((0, 1), (1, 1), (3, 5), (33, 3)):
            B = I * ell
            want = (_even(I * n * K) + _even(B * n * K) + _even(B * n) + (0 if kind == 2 else _even(B * n)) + _even(I * n)
                    + _even(B * n) + (_even(B * n) if kind == 0 else 0) + _even(B))
            assert L.lolhip_chall_ring_work_len(r.ring._h, P._h, kind, I, ell) == want
    other = lolhip.Plan.for_index(m, [q + 1], host_only=True)
    assert L.lolhip_chall_ring_work_len(r.ring._h, other._h, 0, 1, 1) == ERR_INVALID
    assert L.lolhip_chall_ring_work_len(None, P._h, 0, 1, 1) == L.lolhip_chall_ring_work_len(r.ring._h, None, 0, 1, 1) == ERR_INVALID
    assert L.lolhip_chall_ring_work_len(r.ring._h, P._h, 3, 1, 1) == L.lolhip_chall_ring_work_len(r.ring._h, P._h, 0, 1, 0) == ERR_INVALID


def test_statuses_are_decided_before_the_device(lolhip):
    L = lolhip.lib()
    P = lolhip.Plan.for_index(32, [97], host_only=True)
    P2 = lolhip.Plan.for_index(32, [97, 193], host_only=True)
    PN = lolhip.Plan.for_index(32, [512], host_only=True)
    gen = lambda pl, kind, p=4, svar=1.0, I=2, ell=2: L.lolhip_chall_generate_batch(pl._h, None, kind, p, svar, KEY, 0, 0, I, ell,
                                                                                  None, None, None, None)
    ver = lambda pl, kind, p=4, I=2, ell=2: L.lolhip_chall_verify_batch(pl._h, None, kind, p, 1, 1.0, I, ell, None, None, None,
                                                                        None, None, None)
    for kind in (0, 1, 2):
        assert gen(P, kind) == ver(P, kind) == ERR_NO_DEVICE           # every host check passed; no CPU fallback
        assert gen(P, kind, I=-1) == ver(P, kind, I=-1) == gen(P, kind, ell=0) == ver(P, kind, ell=0) == ERR_INVALID
        assert gen(PN, kind) == ver(PN, kind) == ERR_NO_CRT
    assert gen(P, 3) == ver(P, -1) == ERR_INVALID
    assert gen(P, 0, svar=0.0) == gen(P, 1, svar=float("nan")) == ERR_INVALID and gen(P, 2, svar=0.0) == ERR_NO_DEVICE
    assert gen(P, 2, p=97) == ver(P, 2, p=1) == ERR_INVALID and gen(P, 2, p=96) == ver(P, 2, p=2) == ERR_NO_DEVICE
    assert gen(P2, 0) == ver(P2, 0) == ERR_NO_DEVICE and gen(P2, 1) == ver(P2, 2) == ERR_INVALID
    # the ring route on the modulus the plan route refuses
    r = lolhip.RingRLWE(PN)
    rgen = lambda kind, p=4, svar=1.0: L.lolhip_chall_ring_generate_batch(r.ring._h, PN._h, None, kind, p, svar, KEY, 0, 0, 2, 2,
                                                                        None, None, None, None)
    rver = lambda kind, p=4: L.lolhip_chall_ring_verify_batch(r.ring._h, PN._h, None, kind, p, 1, 1.0, 2, 2, None, None, None,
                                                              None, None, None)
    for kind in (0, 1, 2):
        assert rgen(kind) == rver(kind) == ERR_NO_DEVICE
    assert rgen(2, p=512) == rver(2, p=0) == rgen(0, svar=-1.0) == ERR_INVALID
    with pytest.raises(lolhip.NoDeviceError):
        lolhip.RLWE(P).instances("disc", 2, 2)
    with pytest.raises(lolhip.NoDeviceError):
        r.validInstances("rlwr", np.zeros((2, P.n), dtype=np.int64), np.zeros((4, P.n), dtype=np.int64),
                         np.zeros((4, P.n), dtype=np.int64), p=4)


# ---- the CPU model against itself: generate -> verify, permuted secrets, one corruption, the suppressed instance ---------
@pytest.mark.parametrize("route,m,q", [("plan", 32, 97), ("plan", 21, 337), ("ring", 32, 512), ("ring", 12, 500)])
def test_model_round_trip(cpuref, ch, route, m, q):
    M = cf.Model(cpuref, m, [q]) if route == "plan" else cf.RingModel(m, q)
    I, ell, svar = 5, 3, 0.5
    for kind, p in ((cf.DISC, 0), (cf.CONT, 0), (cf.RLWR, 2), (cf.RLWR, q - 1)):
        g = cf.generate(M, kind, I, ell, svar, p, KEY, 100, 1000)
        bound = {cf.DISC: rr.error_bound_disc(m, svar, 2.0 ** -25), cf.CONT: rr.error_bound_cont(m, svar, 2.0 ** -25),
                 cf.RLWR: 0}[kind]
        fails, worst = cf.verify(M, kind, ell, g["s"], g["a"], g["b"], bound, p)
        assert not fails.any() and (kind == cf.RLWR or (worst < bound).all())
        fails, _ = cf.verify(M, kind, ell, np.roll(g["s"], 1, axis=0), g["a"], g["b"], bound, p)
        # p = 2 at n = 4: a wrong secret matches a whole sample with probability 2^-4, so only p = q - 1 fails every one
        assert list(fails) == [ell] * I if p != 2 else fails.all()
        b2 = g["b"].copy()
        at = (2 * ell + ell - 1, M.n // 2) + ((0,) if kind == cf.DISC else ())
        b2[at] = (b2[at] + 1) % p if kind == cf.RLWR else (b2[at] + q // 2) % q if kind == cf.DISC else (b2[at] + q / 2) % q
        fails, _ = cf.verify(M, kind, ell, g["s"], g["a"], b2, bound, p)
        assert list(fails) == [0, 0, 1, 0, 0]
        # the suppressed instance (beacon byte 0xE8 -> 232 mod 5 = 2) left out: the other I - 1 verify as before
        sup = ch.suppressed_secret_id(I, 0xE8)
        keep = [i for i in range(I) if i != sup]
        rows = np.concatenate([np.arange(i * ell, (i + 1) * ell) for i in keep])
        fails, _ = cf.verify(M, kind, ell, g["s"][keep], g["a"][rows], b2[rows], bound, p)
        assert sup == 2 and list(fails) == [0] * (I - 1)
        # the strict comparison on the model: a bound equal to the largest norm fails
        if kind == cf.DISC:
            vals = cf.sample_values(M, kind, ell, g["s"], g["a"], g["b"])
            assert cf.verdict(kind, vals, ell, int(vals.max()))[0].any() and not cf.verdict(kind, vals, ell, int(vals.max()) + 1)[0].any()
    assert list(cf.verdict(cf.DISC, [cf.INT64_MAX, 1], 1, cf.INT64_MAX)[0]) == [1, 0]
    f, w = cf.verdict(cf.CONT, [0.0, np.nan, 1.0, 2.0], 2, 1e300)
    assert list(f) == [1, 0] and np.isnan(w[0]) and w[1] == 2.0


# ---- the messages of RLWE.proto / Challenges.proto against google.protobuf ---------------------------------------------
KINDS = ("Cont", "Disc", "RLWR")


@pytest.fixture(scope="module")
def pb():
    """every message of the two .proto files through a dynamic descriptor; a `Pk` suffix: the same with packed xs"""
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    fd = descriptor_pb2.FileDescriptorProto(name="challenge_wire_test.proto", package="c", syntax="proto2")
    F = descriptor_pb2.FieldDescriptorProto
    ty = {"i32": F.TYPE_INT32, "i64": F.TYPE_INT64, "u32": F.TYPE_UINT32, "u64": F.TYPE_UINT64, "s64": F.TYPE_SINT64,
          "f64": F.TYPE_DOUBLE, "bytes": F.TYPE_BYTES}

    def msg(name, *fields):
        d = fd.message_type.add(name=name)
        for fname, num, t, *rest in fields:
            lab = {"req": F.LABEL_REQUIRED, "rep": F.LABEL_REPEATED, "pk": F.LABEL_REPEATED, "opt": F.LABEL_OPTIONAL}[rest[0] if rest else "req"]
            f = d.field.add(name=fname, number=num, label=lab, **({"type": ty[t]} if t in ty else {"type": F.TYPE_MESSAGE, "type_name": ".c." + t}))
            if rest and rest[0] == "pk":
                f.options.packed = True
        return d

    msg("ContParams", ("m", 1, "i32"), ("q", 2, "i64"), ("svar", 3, "f64"), ("bound", 4, "f64"), ("numSamples", 5, "i32"))
    msg("DiscParams", ("m", 1, "i32"), ("q", 2, "i64"), ("svar", 3, "f64"), ("bound", 4, "i64"), ("numSamples", 5, "i32"))
    msg("RLWRParams", ("m", 1, "i32"), ("q", 2, "i64"), ("p", 3, "i64"), ("numSamples", 4, "i32"))
    c = msg("Challenge", ("challengeID", 1, "i32"), ("numInstances", 2, "i32"), ("beaconEpoch", 3, "i64"), ("beaconOffset", 4, "i32"),
            ("cparams", 5, "ContParams", "opt"), ("dparams", 6, "DiscParams", "opt"), ("rparams", 7, "RLWRParams", "opt"))
    c.oneof_decl.add(name="params")
    for f in c.field[4:]:
        f.oneof_index = 0
    for sfx, rep in (("", "rep"), ("Pk", "pk")):
        msg("Rq" + sfx, ("m", 1, "u32"), ("q", 2, "u64"), ("xs", 3, "s64", rep))
        msg("Kq" + sfx, ("m", 1, "u32"), ("q", 2, "u64"), ("xs", 3, "f64", rep))
        msg("RqProduct" + sfx, ("rqlist", 1, "Rq" + sfx, "rep"))
        msg("KqProduct" + sfx, ("kqlist", 1, "Kq" + sfx, "rep"))
        msg("Secret" + sfx, ("challengeID", 1, "i32"), ("instanceID", 2, "i32"), ("m", 3, "i32"), ("q", 4, "i64"), ("seed", 5, "bytes"),
            ("s", 6, "Rq" + sfx))
        msg("SecretProduct" + sfx, ("challengeID", 1, "i32"), ("instanceID", 2, "i32"), ("m", 3, "i32"), ("q", 4, "i64"),
            ("seed", 5, "bytes"), ("s", 6, "RqProduct" + sfx))
        for kind in KINDS:
            bt = "Kq" if kind == "Cont" else "Rq"
            for gen in ("", "Product"):
                msg("Sample" + kind + gen + sfx, ("a", 1, "Rq" + gen + sfx), ("b", 2, bt + gen + sfx))
                msg("Instance" + kind + gen + sfx, ("challengeID", 1, "i32"), ("instanceID", 2, "i32"), ("params", 3, kind + "Params"),
                    ("samples", 4, "Sample" + kind + gen + sfx, "rep"))
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    get = getattr(message_factory, "GetMessageClass", None)
    return (lambda n: get(pool.FindMessageTypeByName("c." + n))) if get else \
        (lambda n: message_factory.MessageFactory(pool).GetPrototype(pool.FindMessageTypeByName("c." + n)))


def _lift(x, q):
    x = int(x) % q
    return x if 2 * x < q else x - q


def _params(kind, m=7, q=97, L=3):
    d = {"kind": kind, "m": m, "q": q, "numSamples": L}
    d.update({"p": 5} if kind == "RLWR" else {"svar": 0.5, "bound": 414 if kind == "Disc" else 112.5})
    return d


def _samples(kind, q=97, p=5, L=3, n=6):
    rng = np.random.default_rng(len(kind))
    a = rng.integers(0, q, size=(L, n), dtype=np.int64)
    b = rng.random((L, n)) * q if kind == "Cont" else rng.integers(0, p if kind == "RLWR" else q, size=(L, n), dtype=np.int64)
    return a, b


def _fill_params(dst, prm):
    for k, v in prm.items():
        if k != "kind":
            setattr(dst, k, v)


def _fill_elem(dst, product, m, q, xs, dbl):
    e = (dst.kqlist if dbl else dst.rqlist).add() if product else dst
    e.m, e.q = m, q
    e.xs.extend([float(x) for x in xs] if dbl else [_lift(x, q) for x in xs])


def _pb_instance(pb, kind, product, packed, prm, a, b, skip=()):
    msg = pb("Instance" + kind + ("Product" if product else "") + ("Pk" if packed else ""))()
    if "challengeID" not in skip:
        msg.challengeID = 515
    if "instanceID" not in skip:
        msg.instanceID = 31
    if "params" not in skip:
        _fill_params(msg.params, {k: v for k, v in prm.items() if k not in skip})
    for ar, br in zip(a, b):
        smp = msg.samples.add()
        _fill_elem(smp.a, product, prm["m"], prm["q"] + (4 if "q_of_a" in skip else 0), ar, False)
        if "b" not in skip:
            _fill_elem(smp.b, product, prm["m"], prm["p"] if kind == "RLWR" else prm["q"], br, kind == "Cont")
    return msg.SerializePartialToString()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("legacy", [False, True])
def test_instance_messages_both_ways(ch, pb, kind, legacy):
    prm = _params(kind)
    a, b = _samples(kind)
    # ours -> protobuf
    data = ch.instance_write(515, 31, prm, a, b, legacy=legacy)
    msg = pb("Instance" + kind + ("" if legacy else "Product"))()
    msg.ParseFromString(data)
    assert (msg.challengeID, msg.instanceID, len(msg.samples)) == (515, 31, 3)
    assert {k: getattr(msg.params, k) for k in prm if k != "kind"} == {k: v for k, v in prm.items() if k != "kind"}
    for smp, ar, br in zip(msg.samples, a, b):
        ea, eb = (smp.a, smp.b) if legacy else (smp.a.rqlist[0], (smp.b.kqlist if kind == "Cont" else smp.b.rqlist)[0])
        assert (ea.m, ea.q, list(ea.xs)) == (7, 97, [_lift(x, 97) for x in ar])
        bq = 5 if kind == "RLWR" else 97
        assert (eb.m, eb.q) == (7, bq) and list(eb.xs) == ([float(x) for x in br] if kind == "Cont" else [_lift(x, bq) for x in br])
    # protobuf -> ours, unpacked and packed; and our own bytes
    for packed in (False, True):
        for blob in (_pb_instance(pb, kind, not legacy, packed, prm, a, b), data):
            got = ch.instance_read(blob, kind)
            assert (got["challengeID"], got["instanceID"], got["params"], got["product"]) == (515, 31, prm, not legacy)
            assert np.array_equal(got["a"], a) and np.array_equal(got["b"], b)


@pytest.mark.parametrize("kind", KINDS)
def test_instance_reader_rejects(lolhip, ch, pb, kind):
    prm = _params(kind)
    a, b = _samples(kind)
    good = _pb_instance(pb, kind, True, False, prm, a, b)
    assert ch.instance_read(good, kind)["a"].shape == (3, 6)
    bad = [good[:-1], good[:-3], good[:len(good) - 9]]                            # truncated inside the last sample
    bad += [_pb_instance(pb, kind, product, False, prm, a, b, skip=(f,)) for product in (True, False)
            for f in ("challengeID", "instanceID", "params", "numSamples", "m", "b")]      # a missing required field
    bad += [_pb_instance(pb, kind, product, False, prm, a, b, skip=("q_of_a",)) for product in (True, False)]   # q of a sample
    # m of the parameters against m of the samples (the first m = 7, q = 97 on the wire are the parameters')
    bad.append(good.replace(b"\x08\x07\x10\x61", b"\x08\x09\x10\x61", 1))
    for blob in bad:
        with pytest.raises(lolhip.LolHipError) as ei:
            ch.instance_read(blob, kind)
        assert ei.value.code == ERR_INVALID
    for cut in range(len(good)):                                                  # any prefix: a status or a shorter instance
        try:
            ch.instance_read(good[:cut], kind)
        except lolhip.LolHipError:
            pass
    # an unknown field is skipped
    assert np.array_equal(ch.instance_read(good + b"\xf8\x07\x05", kind)["a"], a)


def test_challenge_and_secret_messages(lolhip, ch, pb):
    for kind in KINDS:
        prm = _params(kind)
        kw = {k: v for k, v in prm.items() if k not in ("kind", "m", "q", "numSamples")}
        data = ch.challenge_write(515, 32, 1478822400, 63, kind, 7, 97, 3, **kw)
        msg = pb("Challenge")()
        msg.ParseFromString(data)
        arm = {"Cont": "cparams", "Disc": "dparams", "RLWR": "rparams"}[kind]
        assert msg.WhichOneof("params") == arm
        assert (msg.challengeID, msg.numInstances, msg.beaconEpoch, msg.beaconOffset) == (515, 32, 1478822400, 63)
        assert {k: getattr(getattr(msg, arm), k) for k in prm if k != "kind"} == {k: v for k, v in prm.items() if k != "kind"}
        theirs = pb("Challenge")(challengeID=515, numInstances=32, beaconEpoch=1478822400, beaconOffset=63)
        _fill_params(getattr(theirs, arm), prm)
        for blob in (data, theirs.SerializeToString()):
            got = ch.challenge_read(blob)
            assert got == {"challengeID": 515, "numInstances": 32, "beaconEpoch": 1478822400, "beaconOffset": 63, "params": prm}
        no_arm = pb("Challenge")(challengeID=515, numInstances=32, beaconEpoch=1, beaconOffset=63).SerializeToString()
        theirs.ClearField("beaconEpoch")
        for blob in (data[:-1], no_arm, theirs.SerializePartialToString()):
            with pytest.raises(lolhip.LolHipError):
                ch.challenge_read(blob)
    s, seed = np.arange(90, 96, dtype=np.int64), bytes(range(48))
    for legacy in (False, True):
        data = ch.secret_write(515, 31, 7, 97, seed, s, legacy=legacy)
        msg = pb("Secret" if legacy else "SecretProduct")()
        msg.ParseFromString(data)
        e = msg.s if legacy else msg.s.rqlist[0]
        assert (msg.challengeID, msg.instanceID, msg.m, msg.q, msg.seed) == (515, 31, 7, 97, seed)
        assert (e.m, e.q, list(e.xs)) == (7, 97, [_lift(x, 97) for x in s])
        for packed in (False, True):
            theirs = pb(("Secret" if legacy else "SecretProduct") + ("Pk" if packed else ""))(challengeID=515, instanceID=31, m=7, q=97,
                                                                                                seed=seed)
            _fill_elem(theirs.s, not legacy, 7, 97, s, False)
            for blob in (data, theirs.SerializeToString()):
                got = ch.secret_read(blob)
                assert (got["challengeID"], got["instanceID"], got["m"], got["q"], got["seed"], got["product"]) == \
                    (515, 31, 7, 97, seed, not legacy)
                assert np.array_equal(got["s"], s)
            theirs.q = 101                                                        # the message's q against the element's
            theirs2 = type(theirs)()
            theirs2.CopyFrom(theirs)
            theirs2.ClearField("seed")
            for blob in (theirs.SerializeToString(), theirs2.SerializePartialToString(), data[:-2]):
                with pytest.raises(lolhip.LolHipError):
                    ch.secret_read(blob)


def test_wire_code_under_asan_ubsan(tmp_path):
    """the stand-alone driver of tests/native/challenge_wire_sanitize.cpp with wire.cpp, no Python in the process"""
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    assert cxx is not None, "needs g++"
    exe = tmp_path / "challenge_wire_sanitize"
    srcs = [os.path.join(ROOT, "lol_amd", "csrc", "wire.cpp"), os.path.join(ROOT, "tests", "native", "challenge_wire_sanitize.cpp")]
    subprocess.run([cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", f"-I{os.path.join(ROOT, 'include')}", *srcs, "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "challenge wire sanitize ok" in r.stdout


# ---- the tree layer on the CPU model: no device ---------------------------------------------------------------------------
class ModelEngine:
    """the engine interface of lol_amd.challenges over tests/challenge_ref.py"""

    def __init__(self, M):
        self.M = M

    def instances(self, kind, I, L, svar, p, key, ctr_s, ctr):
        g = cf.generate(self.M, ch_kind(kind), I, L, svar, p, key, ctr_s, ctr)
        return tuple(np.asarray(g[k]).reshape(-1, self.M.n) for k in ("s", "a", "b"))

    def valid(self, kind, s, a, b, bound, p):
        return cf.verify(self.M, ch_kind(kind), a.shape[0] // s.shape[0], s, a, b, bound, p)


def ch_kind(kind):
    return {"Disc": cf.DISC, "Cont": cf.CONT, "RLWR": cf.RLWR}[kind]


TREE_LINES = '0 Cont {m} {q} 0.5 3 "toy" 1 Disc {m} {q} 0.5 3 "toy" 2 RLWR {m} {q} {p} 3 "toy"'


@pytest.mark.parametrize("route,m,q", [("plan", 32, 97), ("ring", 12, 500)])
@pytest.mark.parametrize("legacy", [False, True])
def test_tree_round_trip_on_the_model(cpuref, ch, tmp_path, route, m, q, legacy):
    eng = ModelEngine(cf.Model(cpuref, m, [q]) if route == "plan" else cf.RingModel(m, q))
    root = str(tmp_path)
    for cp in ch.parse_params(TREE_LINES.format(m=m, q=q, p=q - 1), num_instances=5):
        # 1 generate -> write
        name = ch.generate(cp, root, KEY, beacon=(1478822400, 63), ctr_s=100, ctr=1000, legacy=legacy, engine=eng)
        assert name == ch.challenge_name(cp) and sorted(os.listdir(os.path.join(root, name))) == sorted(
            [name + ".challenge"] + [f"{name}-0{i}.instance" for i in range(5)] + [f"{name}-0{i}.secret" for i in range(5)])
        c = ch.challenge_read(open(ch.challenge_path(root, name), "rb").read())
        assert (c["challengeID"], c["numInstances"], c["beaconEpoch"], c["beaconOffset"]) == (cp.challID, 5, 1478822400, 63)
        assert c["params"].get("bound") == ch.error_bound(cp)
        sec = ch.secret_read(open(ch.secret_path(root, name, 3), "rb").read())
        assert sec["seed"] == KEY + (103).to_bytes(8, "little") + (1009).to_bytes(8, "little") and sec["product"] == (not legacy)
        # 2 read -> verify, and the regeneration from the seed field
        res = ch.verify(root, name, engine=eng)
        assert sorted(res) == list(range(5)) and all(ok and f == 0 for ok, f, _ in res.values())
        assert ch.regen(root, name, engine=eng)
        # 3 suppress -> verify with the beacon's byte: 0xE8 = 232 -> instance 2
        with pytest.raises(ch.ChallengeError, match="Secret 2 should not exist, but it does! You may need to run the 'suppress' command."):
            ch.verify(root, name, beacon_byte=0xE8, engine=eng)
        assert ch.suppress(root, name, 0xE8) == 2 and not os.path.exists(ch.secret_path(root, name, 2))
        res = ch.verify(root, name, beacon_byte=0xE8, engine=eng)
        assert sorted(res) == [0, 1, 3, 4] and all(ok for ok, _, _ in res.values())
        assert ch.regen(root, name, beacon_byte=0xE8, engine=eng)
        with pytest.raises(ch.ChallengeError, match="file does not exist"):
            ch.verify(root, name, engine=eng)                              # all secrets expected, one is gone
        # a corrupted sample fails its instance only; the structural checks speak the reference's messages
        ipath = ch.instance_path(root, name, 4)
        inst = ch.instance_read(open(ipath, "rb").read(), cp.kind)
        b2 = inst["b"].copy()
        b2[2, 1] = (b2[2, 1] + 1) % cp.p if cp.kind == "RLWR" else (b2[2, 1] + q // 2) % q
        open(ipath, "wb").write(ch.instance_write(cp.challID, 4, inst["params"], inst["a"], b2, legacy=legacy))
        res = ch.verify(root, name, beacon_byte=0xE8, engine=eng)
        assert [i for i, (ok, _, _) in res.items() if not ok] == [4] and res[4][1] == 1
        assert not ch.regen(root, name, beacon_byte=0xE8, engine=eng)
        open(ipath, "wb").write(ch.instance_write(cp.challID, 3, inst["params"], inst["a"], inst["b"], legacy=legacy))
        with pytest.raises(ch.ChallengeError, match="instID mismatch. Expected 4 but got 3"):
            ch.verify(root, name, beacon_byte=0xE8, engine=eng)
        open(ipath, "wb").write(ch.instance_write(cp.challID, 4, dict(inst["params"], numSamples=4), inst["a"], inst["b"]))
        with pytest.raises(ch.ChallengeError, match="params mismatch"):
            ch.verify(root, name, beacon_byte=0xE8, engine=eng)
        open(ipath, "wb").write(ch.instance_write(cp.challID, 4, inst["params"], inst["a"], inst["b"]))
        spath = ch.secret_path(root, name, 0)
        sec = ch.secret_read(open(spath, "rb").read())
        open(spath, "wb").write(ch.secret_write(cp.challID, 0, m, q, sec["seed"][:31], sec["s"]))
        with pytest.raises(ch.ChallengeError, match="Seed length is too short! Expected at least 32 bytes, but only found 31 bytes."):
            ch.verify(root, name, beacon_byte=0xE8, engine=eng)


def test_route_counts_of_the_list(ch, records):
    """the counts README and DESIGN quote"""
    routes = {}
    per_line = Counter(routes.setdefault((r.m, r.q), ch.route(r)[0]) for r in records)
    assert per_line == {"plan": 222, "ring": 294}
    big = [r for r in records if max(p for p, _ in rr.factor_pps(r.m)) > 13]
    assert len(big) == 144 and sorted({r.m for r in big}) == [23, 29, 179, 257, 797]
