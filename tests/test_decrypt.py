"""SymmSHE errorTerm / decrypt on the GPU (lolhip_error_term_batch, lolhip_decrypt_batch).

The reference is (a) a big-integer restatement of the pair lift, Prelude.hs:168-180 nested, with decode' of
ZqBasic.hs:92-94 for one modulus: the centred representative mod Q = prod q_t, and (b) the SymmSHE model of
oracle/she_model.py driven by the CPU oracle (CpuEngine): its `decrypt` and the lift inside it.

    lift at its boundaries      ncs = 1, chosen decoding-basis integers: errorTerm returns them (INT64_MIN beyond int64)
    decrypt vs the model        fresh LSD, toMSD, ct x ct, keySwitchQuadCirc, modSwitch: bit for bit, and = plaintext
    m != m'                     the reference's decBenches shapes (16 in 1024 / 2048, p = 8 / 16)
    batch and stream            B = 4096 at m' = 2^14 on a side stream, device tensors, both input bases
    errors                      status codes decided before any launch: the output stays untouched
"""
from math import prod

import numpy as np
import pytest

from oracle import lolmath as lm
from oracle import she_model as sm
from oracle.oracle import Params

INT64_MIN = -(2 ** 63)


def _params(m, qs):
    """oracle Params, also for a modulus without a CRT basis (prime ops only, as tests/test_oracle.py does)"""
    try:
        return Params(lm.factor_pps(m), qs)
    except ValueError:
        P = Params.__new__(Params)
        P.pps = lm.factor_pps(m)
        P.qs, P.T, P.m, P.n = list(qs), len(qs), m, lm.totient_pps(P.pps)
        return P


def _moduli(m, bits, T):
    g = lm.good_qs(m, 2 ** (bits - 1))
    return [next(g) for _ in range(T)]


def _centred(x, Q):
    x %= Q
    return x - Q if 2 * x >= Q else x


# ---------------------------------------------------------------------------------------------
# 1. the lift at its boundaries
# ---------------------------------------------------------------------------------------------
LIFT_CASES = [(2 ** 11, 1, 61), (2 ** 11, 2, 59), (2 ** 12, 4, 59), (64, 16, 61), (45, 3, 30), (45, 16, 20),
              (11648, 2, 30), (15015, 4, 59), (2 ** 10, 3, 20)] + [(45, T, 20) for T in range(5, 16)]


def _boundary_values(Q, rng, count):
    H = (Q - 1) // 2
    vals = [0, 1, -1, 2, -2, H, -H, H - 1, -H + 1, H - 2, -(H - 2)]
    for c in (2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, 2 ** 62, -(2 ** 63) + 1, -(2 ** 63), -(2 ** 63) - 1, -(2 ** 62)):
        if abs(c) <= H:
            vals.append(c)
    while len(vals) < count:
        r, sign, d = int(rng.integers(0, 4)), int(rng.choice([-1, 1])), int(rng.integers(-1000, 1000))
        if r == 0:                                  # small
            vals.append(int(rng.integers(-2 ** 62, 2 ** 62)) % (H + 1) * sign)
        elif r == 1:                                # anywhere in the centred range
            vals.append(_centred(int.from_bytes(rng.bytes((Q.bit_length() + 7) // 8), "little"), Q))
        elif r == 2 and 2 ** 63 + 1000 < H:         # next to +-2^63
            vals.append(sign * (2 ** 63 + d))
        else:                                       # next to +-Q/2
            vals.append(sign * (H - abs(d) % H))
    return vals[:count]


@pytest.mark.gpu
@pytest.mark.parametrize("m,T,bits", LIFT_CASES)
@pytest.mark.parametrize("cs_crt", [False, True])
def test_error_term_lift_boundaries(gpu, m, T, bits, cs_crt):
    qs = _moduli(m, bits, T)
    Q = prod(qs)
    pq = gpu.Plan.for_index(m, qs)
    rng = np.random.default_rng(m + T + bits)
    B = 2
    n = pq.n
    xs = _boundary_values(Q, rng, B * n)
    rng.shuffle(xs)
    x = np.array(xs, dtype=object).reshape(B, n)
    res = np.stack([(x % q).astype(np.int64) for q in qs], axis=-1)         # decoding basis, [0, q)
    c0 = np.ascontiguousarray(pq.l(res))                                    # -> powerful basis
    neg = rng.integers(0, 2, size=c0.shape).astype(bool) & (c0 > 0)          # some representatives in (-q, 0)
    c0 = np.where(neg, c0 - np.array(qs, dtype=np.int64), c0)
    if cs_crt:
        c0 = np.ascontiguousarray(pq.crt(c0))
    s_crt = np.stack([rng.integers(0, q, size=n, dtype=np.int64) for q in qs], axis=-1)
    got = pq.errorTerm([c0], s_crt, 2, cs_crt=cs_crt)
    want = np.array([[v if -(2 ** 63) < v < 2 ** 63 else INT64_MIN for v in row] for row in xs_rows(x)], dtype=np.int64)
    assert np.array_equal(got, want)
    # MSD: the residues are scaled by p first: errorTerm = centred (p x) mod Q
    p = 3
    got = pq.errorTerm([c0], s_crt, p, enc="MSD", cs_crt=cs_crt)
    want = [[_centred(p * v, Q) for v in row] for row in xs_rows(x)]
    want = np.array([[v if -(2 ** 63) < v < 2 ** 63 else INT64_MIN for v in row] for row in want], dtype=np.int64)
    assert np.array_equal(got, want)


def xs_rows(x):
    return [[int(v) for v in row] for row in x]


# ---------------------------------------------------------------------------------------------
# 2. decrypt against the model
# ---------------------------------------------------------------------------------------------
DEC_CASES = [(64, 257, 2 ** 29, 2), (48, 97, 2 ** 29, 2), (45, 181, 2 ** 30, 2),
             (2 ** 15, 65537, 2 ** 58, 3), (2 ** 15, 65537, 2 ** 60, 4)]


def _gpu_checks(she, pq, pp, ct, want_pt):
    """GPU decrypt (both input bases) = the model's decrypt = the plaintext; GPU errorTerm = the model's lift"""
    s_crt = np.ascontiguousarray(she.s_crt[0])
    model = she.decrypt(ct)
    assert np.array_equal(model, want_pt)
    kw = dict(enc=ct["enc"], k=ct["k"], l=ct["l"])
    got = pq.decrypt(ct["c"], s_crt, pp, **kw)
    assert np.array_equal(got, model)
    cs_crt = [np.ascontiguousarray(she.e.crt(c)) for c in ct["c"]]
    assert np.array_equal(pq.decrypt(cs_crt, s_crt, pp, cs_crt=True, **kw), model)
    lsd = she.toLSD(ct)
    e_model = she.lift(she.e.lInv(she.evaluate(lsd["c"])))              # a key-switched error can exceed int64
    e_model = np.array([[int(v) if -(2 ** 63) < v < 2 ** 63 else INT64_MIN for v in row] for row in e_model], dtype=np.int64)
    assert np.array_equal(pq.errorTerm(ct["c"], s_crt, she.p, enc=ct["enc"]), e_model)


@pytest.mark.gpu
@pytest.mark.parametrize("m,p,lower,T", DEC_CASES)
def test_decrypt_matches_model(gpu, cpuref, m, p, lower, T):
    pps = lm.factor_pps(m)
    g = lm.good_qs(m, lower)
    qs = [next(g) for _ in range(T)]
    rng = np.random.default_rng(3000 + m + T)
    eng = lambda qs_: sm.CpuEngine(cpuref, Params(pps, qs_))
    she = sm.SHE(eng(qs), eng([p]), qs, p, rng)
    she.keygen()
    pq, pp = gpu.Plan(pps, qs), gpu.Plan(pps, [p])
    B = 2
    pt1 = rng.integers(0, p, size=(B, she.n), dtype=np.int64)
    pt2 = rng.integers(0, p, size=(B, she.n), dtype=np.int64)
    pt1[0] = 0
    ct1, ct2 = she.encrypt(pt1), she.encrypt(pt2)
    _gpu_checks(she, pq, pp, ct1, pt1)                                       # fresh, LSD
    _gpu_checks(she, pq, pp, she.toMSD(ct1), pt1)                            # MSD
    prod_ = she.mul(ct1, ct2)                                                # ncs = 3, k = 1
    assert len(prod_["c"]) == 3 and prod_["k"] == 1
    want = cpuref.polymul(Params(pps, [p]), pt1[..., None], pt2[..., None]).reshape(pt1.shape)
    _gpu_checks(she, pq, pp, prod_, want)
    lin = she.key_switch_quad(she.ks_quad_hint(0), 0, prod_)                  # MSD, ncs = 2, k = 1
    _gpu_checks(she, pq, pp, lin, want)
    small, she2 = she.mod_switch_drop_first(ct1, eng(qs[1:]))               # T - 1 moduli
    _gpu_checks(she2, gpu.Plan(pps, qs[1:]), pp, small, pt1)
    if T > 2:
        assert prod(qs) > 2 ** 128


# ---------------------------------------------------------------------------------------------
# 3. m != m' at the reference's benchmark shapes (decBenches: lol-apps Benchmarks/Default.hs:43-44)
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m,m2,p", [(16, 1024, 8), (16, 2048, 16)])
def test_decrypt_with_twace(gpu, cpuref, m, m2, p):
    q = 1017857
    pps, pps2 = lm.factor_pps(m), lm.factor_pps(m2)
    rng = np.random.default_rng(m2 + p)
    Pm_p, Pm2_p = _params(m, [p]), _params(m2, [p])
    she = sm.SHE(sm.CpuEngine(cpuref, Params(pps2, [q])), sm.CpuEngine(cpuref, Pm2_p), [q], p, rng)
    she.keygen()
    B = 3
    pt = rng.integers(0, p, size=(B, Pm_p.n), dtype=np.int64)
    pt_hi = cpuref.embed_pow(Pm_p, Pm2_p, pt[..., None])[..., 0]            # embed pt into R_m'
    ct = she.encrypt(pt_hi)
    pq, pp, pm = gpu.Plan(pps2, [q]), gpu.Plan(pps2, [p]), gpu.Plan(pps, [p])
    x_p = gpu.Ext(pm, pp)
    s_crt = np.ascontiguousarray(she.s_crt[0])
    got = pq.decrypt(ct["c"], s_crt, pp, ext=x_p)
    assert got.shape == (B, Pm_p.n)
    assert np.array_equal(got, pt)
    model_hi = she.decrypt(ct)
    assert np.array_equal(got, cpuref.twace_powdec(Pm_p, Pm2_p, model_hi[..., None])[..., 0])
    got_msd = pq.decrypt(she.toMSD(ct)["c"], s_crt, pp, ext=x_p, enc="MSD", l=she.toMSD(ct)["l"])
    assert np.array_equal(got_msd, pt)


# ---------------------------------------------------------------------------------------------
# 4. batch and stream
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_decrypt_batch_on_a_side_stream(gpu, cpuref):
    import torch
    m, T, B, p = 2 ** 14, 2, 4096, 65537
    pps = lm.factor_pps(m)
    qs = _moduli(m, 59, T)
    pq, pp = gpu.Plan(pps, qs), gpu.Plan(pps, [p])
    n = pq.n
    rng = np.random.default_rng(44)
    she = sm.SHE(sm.CpuEngine(cpuref, Params(pps, qs)), sm.CpuEngine(cpuref, Params(pps, [p])), qs, p, rng)
    she.keygen()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    cs = torch.stack([torch.stack([torch.randint(0, q, (B, n), dtype=torch.int64, device="cuda", generator=gen) for q in qs], -1)
                      for _ in range(3)])                                      # [3][B][n][T], arbitrary ciphertexts
    s_crt = torch.from_numpy(np.ascontiguousarray(she.s_crt[0])).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = pq.decrypt(cs, s_crt, pp, k=1, l=7, stream=side.cuda_stream)
        cs_c = cs.clone()
        for i in range(3):
            pq.crt(cs_c[i], stream=side.cuda_stream)
        got_c = pq.decrypt(cs_c, s_crt, pp, k=1, l=7, cs_crt=True, stream=side.cuda_stream)
        e = pq.errorTerm(cs, s_crt, p, enc="MSD", stream=side.cuda_stream)
    torch.cuda.synchronize()
    assert got.is_cuda and got.shape == (B, n)
    assert torch.equal(got, got_c)
    # per-slice decrypts
    for lo in range(0, B, 1024):
        part = pq.decrypt(cs[:, lo:lo + 1024].contiguous(), s_crt, pp, k=1, l=7)
        assert torch.equal(part, got[lo:lo + 1024])
    torch.cuda.synchronize()
    # the model on a sampled subset
    for b in (0, 1777, B - 1):
        ct = {"enc": "LSD", "k": 1, "l": 7, "c": [cs[i, b:b + 1].cpu().numpy() for i in range(3)]}
        assert np.array_equal(got[b:b + 1].cpu().numpy(), she.decrypt(ct)), b
        ctm = {"enc": "MSD", "k": 0, "l": 1, "c": ct["c"]}
        lsd = she.toLSD(ctm)
        want = she.lift(she.e.lInv(she.evaluate(lsd["c"])))           # mostly beyond int64 for arbitrary ciphertexts
        want = np.array([[int(v) if -(2 ** 63) < v < 2 ** 63 else INT64_MIN for v in row] for row in want], dtype=np.int64)
        assert np.array_equal(e[b:b + 1].cpu().numpy(), want), b


# ---------------------------------------------------------------------------------------------
# 5. errors: decided on the host, before any launch
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_decrypt_errors_leave_output_untouched(gpu):
    import torch
    L = gpu.lib()
    SENT = 0x5A5A5A5A
    B = 2

    def run(pq, pp, x_p, ncs, enc=0, k=0, n_out=None, cs_crt=0):
        n_out = n_out or pq.n
        cs = torch.zeros((max(ncs, 1), B, pq.n, pq.T), dtype=torch.int64, device="cuda")
        s_crt = torch.zeros((pq.n, pq.T), dtype=torch.int64, device="cuda")
        work = torch.zeros((max(L.lolhip_decrypt_work_len(pq._h, max(ncs, 1), B), 1),), dtype=torch.int64, device="cuda")
        out = torch.full((B, n_out), SENT, dtype=torch.int64, device="cuda")
        rc = L.lolhip_decrypt_batch(pq._h, pp._h, None if x_p is None else x_p._h, None, cs.data_ptr(), ncs, cs_crt,
                                    s_crt.data_ptr(), enc, k, 1, out.data_ptr(), work.data_ptr(), B)
        torch.cuda.synchronize()
        return rc, bool((out == SENT).all())

    def run_et(pq, ncs, enc, p):
        cs = torch.zeros((max(ncs, 1), B, pq.n, pq.T), dtype=torch.int64, device="cuda")
        s_crt = torch.zeros((pq.n, pq.T), dtype=torch.int64, device="cuda")
        work = torch.zeros((max(L.lolhip_decrypt_work_len(pq._h, max(ncs, 1), B), 1),), dtype=torch.int64, device="cuda")
        out = torch.full((B, pq.n), SENT, dtype=torch.int64, device="cuda")
        rc = L.lolhip_error_term_batch(pq._h, None, cs.data_ptr(), ncs, 0, s_crt.data_ptr(), enc, p, out.data_ptr(),
                                       work.data_ptr(), B)
        torch.cuda.synchronize()
        return rc, bool((out == SENT).all())

    ERR_INVALID, ERR_MODULUS, ERR_NO_CRT, ERR_NOT_DIVISIBLE = -1, -2, -3, -7
    qs = [1017857, 1032193]
    pq = gpu.Plan.for_index(2048, qs)
    pp = gpu.Plan.for_index(2048, [16])
    # a valid call writes
    rc, untouched = run(pq, pp, None, 2)
    assert rc == 0 and not untouched
    # pp of another index / of two moduli
    assert run(pq, gpu.Plan.for_index(1024, [16]), None, 2, n_out=pq.n) == (ERR_INVALID, True)
    assert run(pq, gpu.Plan.for_index(2048, [16, 17]), None, 2) == (ERR_INVALID, True)
    # x_p that does not end in pp's ring and modulus
    pm = gpu.Plan.for_index(16, [16])
    x_other = gpu.Ext(gpu.Plan.for_index(16, [8]), gpu.Plan.for_index(2048, [8]))
    assert run(pq, pp, x_other, 2, n_out=pm.n) == (ERR_INVALID, True)
    x_small = gpu.Ext(pm, gpu.Plan.for_index(1024, [16]))
    assert run(pq, pp, x_small, 2, n_out=pm.n) == (ERR_INVALID, True)
    assert run(pq, pp, gpu.Ext(pm, pp), 2, n_out=pm.n)[0] == 0
    # ncs = 0
    assert run(pq, pp, None, 0) == (ERR_INVALID, True)
    assert run_et(pq, 0, 0, 16) == (ERR_INVALID, True)
    # pq without a CRT basis
    no_crt = [q for q in range(1000003, 1001000, 2) if lm.is_prime(q) and (q - 1) % 2048][:2]
    pnc = gpu.Plan.for_index(2048, no_crt)
    assert not pnc.has_crt
    assert run(pnc, pp, None, 2) == (ERR_NO_CRT, True)
    assert run_et(pnc, 2, 0, 16) == (ERR_NO_CRT, True)
    # MSD with p sharing a factor with Q (LSD with the same p is fine)
    pp_q = gpu.Plan.for_index(2048, [qs[0]])
    assert run(pq, pp_q, None, 2, enc=1) == (ERR_MODULUS, True)
    assert run_et(pq, 2, 1, qs[1] * 3) == (ERR_MODULUS, True)
    assert run(pq, pp_q, None, 2, enc=0)[0] == 0
    # k = 1 where divG is impossible mod p: oddRad(45) = 15 is not invertible mod 5
    g = lm.good_qs(45, 2 ** 29)
    pq45 = gpu.Plan.for_index(45, [next(g), next(g)])
    pp5 = gpu.Plan.for_index(45, [5])
    assert run(pq45, pp5, None, 2, k=1) == (ERR_NOT_DIVISIBLE, True)
    assert run(pq45, pp5, None, 2, k=0)[0] == 0
    # the Python layer raises with the code
    with pytest.raises(gpu.LolHipError) as ei:
        pq45.decrypt(np.zeros((2, 1, pq45.n, 2), dtype=np.int64), np.zeros((pq45.n, 2), dtype=np.int64), pp5, k=1)
    assert ei.value.code == ERR_NOT_DIVISIBLE
