"""lol_amd/challenges.py — the parameter layer of rlwe-challenges over the batched challenge calls
(RLWE.instances / RLWE.validInstances and their RingRLWE forms): the parameter-line grammar of Params.hs:107-156, the
challenge names of Generate.hs:91-103, the file names of Common.hs:119-158, suppressedSecretID, the error bound with
eps = 2^-25 and the choice of route by lolhip_plan_has_crt; and one challenge generated or verified on the device from
a parsed record.

The tree layer reads and writes the reference's own messages (RLWE.proto, Challenges.proto, through the readers and
writers of csrc/wire.cpp) in the reference's directory layout: generate, verify, regen and suppress below.  Every
function of that layer takes an `engine`: the device (the default) or any object with the same two methods, which is
how the host tests run the layer on the CPU model.  Beacon XML parsing and its X.509 signature check are host-only
cryptography with no role on the device and are out of scope: the caller passes the beacon's byte.

Regeneration.  The reference's verifier can regenerate an instance from the seed field with its own CTR-DRBG; samples
drawn here come from the library's ChaCha20 stream, which that step cannot reproduce.  The reference itself treats a
failed regeneration as non-fatal.  The seed field of secret i holds key || ctr_s + i || ctr + i L (32 + 8 + 8 = 48 bytes,
little-endian counters; above the 32 bytes validateSecret asks of a CTR-DRBG seed), from which regen() below redraws
the instance with this library and compares."""
from __future__ import annotations

import ctypes as C
import os
import re
import struct
from dataclasses import dataclass

import numpy as np

from ._abi import _i64p, _len, _u8p
from .tensor import RLWE, Plan, RingRLWE, factor_pps, lib

EPS_DEF = 2.0 ** -25
KINDS = ("Cont", "Disc", "RLWR")
_TAG = {"Cont": "rlwec", "Disc": "rlwed", "RLWR": "rlwr"}


class ParamsError(ValueError):
    pass


@dataclass(frozen=True)
class ChallengeParams:
    """one line of a parameter file (Params.hs:33-57): kind "Cont" / "Disc" / "RLWR"; svar for Cont and Disc, p for RLWR"""
    challID: int
    kind: str
    m: int
    q: int
    svar: float | None
    p: int | None
    numSamples: int
    numInstances: int
    annotation: str
    eps: float = EPS_DEF

    @property
    def supported(self):
        """False for an RLWR line with p = q: the reference accepts p <= q, the rounding entries need 2 <= p < q"""
        return self.kind != "RLWR" or 2 <= self.p < self.q


_TOKEN = re.compile(r'\s*(?:(?P<str>"(?:[^"\\\n]|\\.)*")|(?P<float>\d+\.\d+(?:[eE][-+]?\d+)?|\d+[eE][-+]?\d+)'
                    r'|(?P<nat>0[xX][0-9a-fA-F]+|0[oO][0-7]+|\d+)|(?P<word>[A-Za-z]+))')


def _strip_comments(text):
    """`--` to the end of the line and nested /* */, outside string literals"""
    out, i, depth, n = [], 0, 0, len(text)
    while i < n:
        two = text[i:i + 2]
        if depth:
            depth, i = (depth + 1, i + 2) if two == "/*" else (depth - 1, i + 2) if two == "*/" else (depth, i + 1)
        elif two == "/*":
            depth, i = 1, i + 2
        elif two == "--":
            j = text.find("\n", i)
            i = n if j < 0 else j
        elif text[i] == '"':
            mt = re.compile(r'"(?:[^"\\\n]|\\.)*"').match(text, i)
            if not mt:
                raise ParamsError(f"unterminated string literal at offset {i}")
            out.append(mt.group())
            i = mt.end()
        else:
            out.append(text[i])
            i += 1
    if depth:
        raise ParamsError("unterminated comment")
    return "".join(out)


def _tokens(text):
    text, i, out = _strip_comments(text), 0, []
    while text[i:].strip():
        mt = _TOKEN.match(text, i)
        if not mt:
            raise ParamsError(f"unexpected input at {text[i:].strip()[:20]!r}")
        out.append((mt.lastgroup, mt.group(mt.lastgroup)))
        i = mt.end()
    return out


def _nat(tok, what):
    if tok[0] != "nat":
        raise ParamsError(f"expected a natural number for {what}, got {tok[1]!r}")
    v = tok[1].lower()
    return int(v[2:], 16) if v.startswith("0x") else int(v[2:], 8) if v.startswith("0o") else int(v)


def _unescape(lit):
    """the annotation's text: \\" and \\\\ are the escapes taken"""
    body = lit[1:-1]
    if re.search(r'\\[^"\\]', body.replace("\\\\", "")):
        raise ParamsError(f"unsupported escape in {lit}")
    return re.sub(r'\\(["\\])', r"\1", body)


def parse_params(text, num_instances=32):
    """The records of a parameter file, in order (Params.hs:105-156): `challID Cont|Disc m q svar l "annotation"` and
    `challID RLWR m q p l "annotation"`, with `--` and nested /* */ comments.  p > q raises, as in the reference; p = q
    parses and is marked unsupported."""
    toks, out, i = _tokens(text), [], 0
    while i < len(toks):
        rec = toks[i:i + 7]
        if len(rec) < 7:
            raise ParamsError(f"incomplete record after {len(out)} records")
        cid = _nat(rec[0], "challID")
        if rec[1][0] != "word" or rec[1][1] not in KINDS:
            raise ParamsError("""Expected one of '"Cont"', '"Disc"', or '"RLWR"'.""")
        kind = rec[1][1]
        m, q = _nat(rec[2], "m"), _nat(rec[3], "q")
        svar = p = None
        if kind == "RLWR":
            p = _nat(rec[4], "p")
            if p > q:
                raise ParamsError(f"Expected p <= q; parsed q={q} and p={p}")
        else:
            if rec[4][0] != "float":
                raise ParamsError(f"expected a floating-point svar, got {rec[4][1]!r}")
            svar = float(rec[4][1])
        ell = _nat(rec[5], "numSamples")
        if rec[6][0] != "str":
            raise ParamsError(f"expected a quoted annotation, got {rec[6][1]!r}")
        out.append(ChallengeParams(cid, kind, m, q, svar, p, ell, int(num_instances), _unescape(rec[6][1])))
        i += 7
    return out


def challenge_name(cp):
    """challengeName (Generate.hs:91-103), e.g. chall-id0000-rlwec-m256-q769-l3-short-toy"""
    mid = f"-p{cp.p}" if cp.kind == "RLWR" else ""
    ann = f"-{cp.annotation}" if cp.annotation else ""
    return f"chall-id{cp.challID:04d}-{_TAG[cp.kind]}-m{cp.m}-q{cp.q}{mid}-l{cp.numSamples}{ann}"


# ---- the directory layout of Common.hs:125-158 ---------------------------------------------------------------------------
def challenge_dir(root, name):
    return os.path.join(root, name)


def challenge_path(root, name):
    return os.path.join(root, name, name + ".challenge")


def instance_path(root, name, inst_id):
    return os.path.join(root, name, f"{name}-{inst_id:02X}.instance")


def secret_path(root, name, inst_id):
    return os.path.join(root, name, f"{name}-{inst_id:02X}.secret")


def suppressed_secret_id(num_instances, beacon_byte):
    """suppressedSecretID (Common.hs:119-123) of the beacon output's byte at the challenge's offset"""
    return int(beacon_byte) % int(num_instances)


# ---- one challenge on the device ---------------------------------------------------------------------------------------------
def large_prime(m):
    """whether the index has a prime factor above 13: its Z_q transforms then take the dense route (Plan dense_zq)"""
    return any(p > 13 for p, _ in factor_pps(m))


def route(cp, host_only=True, dense_gauss=False):
    """("plan" | "ring", Plan): lolhip_plan_has_crt decides, as for the single-secret entries.  dense_gauss: the plan
    opts in to the dense stage of the Gaussian map, which the error of a Cont or Disc challenge needs at a prime above 13.
    At such an index the plan also routes its Z_q transforms (a s of every kind, RLWR included) to the dense stages and
    its basis changes (L, LInv) to the scan kernel."""
    plan = Plan.for_index(cp.m, [cp.q], host_only=host_only, dense_gauss=dense_gauss, dense_zq=large_prime(cp.m),
                          scan_zq=large_prime(cp.m))
    return ("plan" if plan.has_crt else "ring"), plan


def error_bound(cp):
    """the bound of the challenge file: errorBound svar eps (Continuous.hs:74-84, Discrete.hs:65-76); None for RLWR"""
    return None if cp.kind == "RLWR" else RLWE.errorBound(cp.m, cp.svar, cp.eps, kind=cp.kind.lower())


def _engine(cp):
    if not cp.supported:
        raise ParamsError(f"{challenge_name(cp)}: p = q is not supported (the rounding needs 2 <= p < q)")
    which, plan = route(cp, host_only=False, dense_gauss=cp.kind in ("Cont", "Disc"))
    return RLWE(plan) if which == "plan" else RingRLWE(plan)


def generate_arrays(cp, key, ctr_s=0, ctr=0, stream=None):
    """(s, a, b) of the whole challenge in the decoding basis, the wire basis: numInstances secrets and
    numInstances * numSamples samples in one call; secret i at counter ctr_s + i, sample (i, l) at ctr + i L + l, L = numSamples"""
    return _engine(cp).instances(cp.kind.lower(), cp.numInstances, cp.numSamples, svar=cp.svar or 1.0, p=cp.p or 0, key=key,
                                 ctr_s=ctr_s, ctr=ctr, stream=stream)


def verify_arrays(cp, s, a, b, stream=None):
    """per-instance verdicts [I] (True = every sample of the instance passes) and (fails, worst), for the secrets s [I]
    given: I may be numInstances - 1 with the suppressed instance's samples left out"""
    fails, worst = _engine(cp).validInstances(cp.kind.lower(), s, a, b, bound=error_bound(cp) or 0, p=cp.p or 0, stream=stream)
    f = fails if hasattr(fails, "dtype") and not hasattr(fails, "cpu") else fails.cpu().numpy()
    return f == 0, (fails, worst)


# ---- the messages of RLWE.proto / Challenges.proto (csrc/wire.cpp) -----------------------------------------------------
KIND_ID = {"Disc": 0, "Cont": 1, "RLWR": 2}
KIND_OF = {v: k for k, v in KIND_ID.items()}
MIN_SEED_LEN = 32                                   # genSeedLength of the reference's CTR-DRBG (validateSecret)


class ChallengeError(RuntimeError):
    """a structural error of a challenge tree, with the reference's message"""


def _raw(data):
    return (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data if data else b"\0")


def _two_pass(fn, *args):
    need = _len(fn(*args, None, 0))
    buf = (C.c_uint8 * max(need, 1))()
    return bytes(buf[:_len(fn(*args, buf, need))])


def _i64(vals):
    a = np.ascontiguousarray(vals, dtype=np.int64)
    return a, a.ctypes.data_as(_i64p)


def _f64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _params_out(kind, m, q, svar, bound, p, num_samples):
    """(ip, dp) of include/lolhip.h"""
    x = int(bound) if kind == "Disc" else int(p) if kind == "RLWR" else 0
    return _i64([m, q, x, num_samples]), np.array([svar or 0.0, float(bound) if kind == "Cont" else 0.0])


def _params_in(kind, ip, dp):
    d = {"kind": kind, "m": int(ip[0]), "q": int(ip[1]), "numSamples": int(ip[3])}
    if kind == "RLWR":
        d["p"] = int(ip[2])
    else:
        d["svar"], d["bound"] = float(dp[0]), (int(ip[2]) if kind == "Disc" else float(dp[1]))
    return d


def challenge_write(challenge_id, num_instances, beacon_epoch, beacon_offset, kind, m, q, num_samples, svar=None, bound=0,
                    p=0):
    """a `Challenge` message with the params arm of `kind` ("Cont" / "Disc" / "RLWR")"""
    (_, hp), ((_, ipp), dp) = _i64([challenge_id, num_instances, beacon_epoch, beacon_offset]), \
        _params_out(kind, m, q, svar, bound, p, num_samples)
    return _two_pass(lib().lolhip_challenge_write, hp, KIND_ID[kind], ipp, _f64p(dp))


def challenge_read(data):
    """a `Challenge` message -> dict(challengeID, numInstances, beaconEpoch, beaconOffset, params=dict(kind, m, q, ...))"""
    hdr, ip, dp, kind = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64), np.zeros(2), C.c_int(-1)
    _len(lib().lolhip_challenge_read(_raw(data), len(data), hdr.ctypes.data_as(_i64p), C.byref(kind), ip.ctypes.data_as(_i64p),
                                     _f64p(dp)), "Challenge")
    return {"challengeID": int(hdr[0]), "numInstances": int(hdr[1]), "beaconEpoch": int(hdr[2]), "beaconOffset": int(hdr[3]),
            "params": _params_in(KIND_OF[kind.value], ip, dp)}


def instance_write(challenge_id, instance_id, params, a, b, legacy=False):
    """an `Instance{Cont,Disc,RLWR}Product` message (legacy=True: the forms of the 2016 release) from params (the dict
    of challenge_read) and the samples a [L][n], b [L][n] in the decoding basis"""
    kind = params["kind"]
    (_, idp), ((_, ipp), dp) = _i64([challenge_id, instance_id]), \
        _params_out(kind, params["m"], params["q"], params.get("svar"), params.get("bound", 0), params.get("p", 0),
                    params["numSamples"])
    a = np.ascontiguousarray(a, dtype=np.int64)
    b = np.ascontiguousarray(b, dtype=np.float64 if kind == "Cont" else np.int64)
    L = a.shape[0]
    n = a.size // max(L, 1)
    (_, qp) = _i64([params["q"]])
    return _two_pass(lib().lolhip_instance_write, KIND_ID[kind], int(bool(legacy)), idp, ipp, _f64p(dp), qp, 1, L, n,
                     a.ctypes.data_as(_i64p), b.ctypes.data_as(C.c_void_p))


def instance_read(data, kind):
    """an instance message of either generation -> dict(challengeID, instanceID, params, product (bool), a [L][n], b [L][n])"""
    ids, ip, dp = np.zeros(2, dtype=np.int64), np.zeros(4, dtype=np.int64), np.zeros(2)
    prod, T, cnt, qs = C.c_int(0), C.c_int(0), C.c_int64(0), np.zeros(64, dtype=np.int64)
    head = (_raw(data), len(data), KIND_ID[kind], ids.ctypes.data_as(_i64p), ip.ctypes.data_as(_i64p), _f64p(dp), C.byref(prod),
            C.byref(T), qs.ctypes.data_as(_i64p), 64, C.byref(cnt))
    n = _len(lib().lolhip_instance_read(*head, None, 0, None, 0), "Instance")
    if cnt.value and T.value != 1:
        raise ChallengeError("an instance over more than one modulus")
    a = np.zeros((cnt.value, n), dtype=np.int64)
    b = np.zeros((cnt.value, n), dtype=np.float64 if kind == "Cont" else np.int64)
    _len(lib().lolhip_instance_read(*head, a.ctypes.data_as(_i64p), a.size, b.ctypes.data_as(C.c_void_p), b.size), "Instance")
    return {"challengeID": int(ids[0]), "instanceID": int(ids[1]), "params": _params_in(kind, ip, dp), "product": bool(prod.value),
            "a": a, "b": b}


def secret_write(challenge_id, instance_id, m, q, seed, s, legacy=False):
    """a `SecretProduct` (legacy=True: `Secret`) message; s [n] in the decoding basis"""
    (_, idp), (sa, sp), (_, qp) = _i64([challenge_id, instance_id]), _i64(s), _i64([q])
    return _two_pass(lib().lolhip_secret_write, int(bool(legacy)), idp, int(m), int(q), C.cast(_raw(seed), _u8p), len(seed), qp, 1,
                     sp, sa.size)


def secret_read(data):
    """a secret message of either generation -> dict(challengeID, instanceID, m, q, seed, product, s [n])"""
    ids, m, q, sl = np.zeros(2, dtype=np.int64), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    prod, T, qs = C.c_int(0), C.c_int(0), np.zeros(64, dtype=np.int64)
    call = lambda seed, cap, xs, capx: lib().lolhip_secret_read(
        _raw(data), len(data), ids.ctypes.data_as(_i64p), C.byref(m), C.byref(q), seed, cap, C.byref(sl), C.byref(prod),
        C.byref(T), qs.ctypes.data_as(_i64p), 64, xs, capx)
    n = _len(call(None, 0, None, 0), "Secret")
    if T.value != 1:
        raise ChallengeError("a secret over more than one modulus")
    seed, s = (C.c_uint8 * max(sl.value, 1))(), np.zeros(n, dtype=np.int64)
    _len(call(seed, sl.value, s.ctypes.data_as(_i64p), n), "Secret")
    return {"challengeID": int(ids[0]), "instanceID": int(ids[1]), "m": int(m.value), "q": int(q.value),
            "seed": bytes(seed[:sl.value]), "product": bool(prod.value), "s": s}


# ---- the tree layer: Generate.hs / Verify.hs / Suppress.hs over files ---------------------------------------------------
class DeviceEngine:
    """the two batched calls on the GPU for one (m, q): RLWE or RingRLWE as lolhip_plan_has_crt decides.  The plan opts
    in to the dense stage of the Gaussian map (a Cont or Disc error at a prime above 13; nothing changes elsewhere)"""

    def __init__(self, m, q):
        plan = Plan.for_index(m, [q], dense_gauss=True, dense_zq=large_prime(m), scan_zq=large_prime(m))
        self.r = RLWE(plan) if plan.has_crt else RingRLWE(plan)
        self.n = plan.n

    def instances(self, kind, I, L, svar, p, key, ctr_s, ctr):
        s, a, b = self.r.instances(kind.lower(), I, L, svar=svar or 1.0, p=p or 0, key=key, ctr_s=ctr_s, ctr=ctr)
        return tuple(t.cpu().numpy().reshape(-1, self.n) for t in (s, a, b))

    def valid(self, kind, s, a, b, bound, p):
        return self.r.validInstances(kind.lower(), np.ascontiguousarray(s), np.ascontiguousarray(a), np.ascontiguousarray(b),
                                     bound=bound, p=p or 0)


def _check_eq(where, what, expected, actual):
    """checkParamsEq (Verify.hs:253-258)"""
    if expected != actual:
        raise ChallengeError(f"Error while reading {where}: {what} mismatch. Expected {expected} but got {actual}")


def _read_file(path):
    if not os.path.isfile(path):
        raise ChallengeError(f"Error reading {path}: file does not exist.")
    with open(path, "rb") as f:
        return f.read()


def _seed(key, ctr_s, ctr):
    return bytes(key) + struct.pack("<QQ", ctr_s, ctr)


def generate(cp, root, key, beacon=(0, 0), ctr_s=0, ctr=0, legacy=False, engine=None):
    """Generate.hs:75-88 for one parsed line: draw the whole challenge in one call and write
    <root>/<name>/<name>.challenge, <name>-%02X.instance and <name>-%02X.secret (the Product messages; legacy=True: the
    forms of the 2016 release).  bound = errorBound svar 2^-25; the seed of secret i is key || ctr_s + i || ctr + i L.
    Returns the challenge's name."""
    if not cp.supported:
        raise ParamsError(f"{challenge_name(cp)}: p = q is not supported (the rounding needs 2 <= p < q)")
    key = bytes(key)
    if len(key) != 32:
        raise ValueError("key must be 32 bytes")
    engine = engine or DeviceEngine(cp.m, cp.q)
    name, I, L = challenge_name(cp), cp.numInstances, cp.numSamples
    bound = error_bound(cp) or 0
    s, a, b = engine.instances(cp.kind, I, L, cp.svar, cp.p, key, ctr_s, ctr)
    os.makedirs(challenge_dir(root, name), exist_ok=True)
    with open(challenge_path(root, name), "wb") as f:
        f.write(challenge_write(cp.challID, I, beacon[0], beacon[1], cp.kind, cp.m, cp.q, L, svar=cp.svar, bound=bound, p=cp.p or 0))
    params = challenge_read(_read_file(challenge_path(root, name)))["params"]
    for i in range(I):
        rows = slice(i * L, (i + 1) * L)
        with open(instance_path(root, name, i), "wb") as f:
            f.write(instance_write(cp.challID, i, params, a[rows], b[rows], legacy=legacy))
        with open(secret_path(root, name, i), "wb") as f:
            f.write(secret_write(cp.challID, i, cp.m, cp.q, _seed(key, ctr_s + i, ctr + i * L), s[i], legacy=legacy))
    return name


def read_tree(root, name, beacon_byte=None):
    """readChallenge (Verify.hs:128-172) with validateInstance / validateSecret: (challenge dict, [instance ids], s [I][n],
    a [I L][n], b [I L][n], [seeds]).  beacon_byte given: the suppressed secret must be absent (readSuppChallenge) and
    the other numInstances - 1 are read; otherwise all secrets are expected (readFullChallenge)."""
    ch = challenge_read(_read_file(challenge_path(root, name)))
    prm, cid, I = ch["params"], ch["challengeID"], ch["numInstances"]
    ids = list(range(I))
    if beacon_byte is not None:
        gone = suppressed_secret_id(I, beacon_byte)
        if os.path.isfile(secret_path(root, name, gone)):
            raise ChallengeError(f"Secret {gone} should not exist, but it does! You may need to run the 'suppress' command.")
        ids.remove(gone)
    ss, aa, bb, seeds = [], [], [], []
    for i in ids:
        ifile, sfile = instance_path(root, name, i), secret_path(root, name, i)
        sec = secret_read(_read_file(sfile))
        _check_eq(sfile, "challID", cid, sec["challengeID"])
        _check_eq(sfile, "instID", i, sec["instanceID"])
        _check_eq(sfile, "m", prm["m"], sec["m"])
        _check_eq(sfile, "q", prm["q"], sec["q"])
        if len(sec["seed"]) < MIN_SEED_LEN:
            raise ChallengeError(f"Seed length is too short! Expected at least {MIN_SEED_LEN} bytes, but only found "
                                 f"{len(sec['seed'])} bytes.")
        inst = instance_read(_read_file(ifile), prm["kind"])
        _check_eq(ifile, "challID", cid, inst["challengeID"])
        _check_eq(ifile, "instID", i, inst["instanceID"])
        _check_eq(ifile, "params", prm, inst["params"])
        _check_eq(ifile, "numSamples", prm["numSamples"], inst["a"].shape[0])
        ss.append(sec["s"]); aa.append(inst["a"]); bb.append(inst["b"]); seeds.append(sec["seed"])
    _check_eq(name, "numInstances", I - (beacon_byte is not None), len(ss))
    return ch, ids, np.stack(ss), np.concatenate(aa), np.concatenate(bb), seeds


def verify(root, name, beacon_byte=None, engine=None):
    """Verify.hs:107-115, 346-366 in one call: {instance id: (valid, fails, worst)} for every instance whose secret is
    expected.  Structural errors raise ChallengeError with the reference's messages."""
    ch, ids, s, a, b, _ = read_tree(root, name, beacon_byte)
    prm = ch["params"]
    engine = engine or DeviceEngine(prm["m"], prm["q"])
    fails, worst = engine.valid(prm["kind"], s, a, b, prm.get("bound", 0), prm.get("p", 0))
    return {i: (int(f) == 0, int(f), w.item()) for i, f, w in zip(ids, np.asarray(fails), np.asarray(worst))}


def regen(root, name, beacon_byte=None, engine=None):
    """regenInstance (Verify.hs:260-320) from this library's seed field: True when every instance redrawn from
    key || ctr_s || ctr has the same s, a and discrete b, and a Cont b with max |lift (b - b')| < 2^-20"""
    ch, ids, s, a, b, seeds = read_tree(root, name, beacon_byte)
    prm = ch["params"]
    engine = engine or DeviceEngine(prm["m"], prm["q"])
    L, q, ok = prm["numSamples"], prm["q"], True
    for k, seed in enumerate(seeds):
        if len(seed) != 48:
            return False
        cs, c = struct.unpack("<QQ", seed[32:])
        s1, a1, b1 = engine.instances(prm["kind"], 1, L, prm.get("svar"), prm.get("p", 0), seed[:32], cs, c)
        rows = slice(k * L, (k + 1) * L)
        ok &= np.array_equal(s1[0], s[k]) and np.array_equal(a1, a[rows])
        if prm["kind"] == "Cont":
            d = (b[rows] - b1) % float(q)
            ok &= bool((np.minimum(d, float(q) - d) < 2.0 ** -20).all())
        else:
            ok &= np.array_equal(b1, b[rows])
    return bool(ok)


def suppress(root, name, beacon_byte):
    """Suppress.hs: delete the secret the beacon's byte names; returns its id"""
    ch = challenge_read(_read_file(challenge_path(root, name)))
    gone = suppressed_secret_id(ch["numInstances"], beacon_byte)
    path = secret_path(root, name, gone)
    if os.path.isfile(path):
        os.remove(path)
    return gone
