"""tests/ptround_ref.py — a step-by-step restatement of HomomPRF's homomorphic rounding 2^e -> 2 (lol-apps
HomomPRF.hs:232-270) over the SymmSHE model of oracle/she_model.py, tests/modswitch_ref.mod_switch and
tests/public_ref.add_public / mod_switch_pt.  TEST INFRASTRUCTURE: one function per reference line, in the reference's own
structure (the p/4 fanned-out ciphertexts are all formed, then paired, level by level); nothing of the device's fused
algebra.  Every ring operation goes through an engine (CpuEngine or a lol_amd.Plan).

A ciphertext is the model's dict {"enc", "k", "l", "c": [c0, c1, ...]}, components [B][n'][T] in the powerful basis."""
from __future__ import annotations

import numpy as np

import modswitch_ref as mr
import public_ref as pr
from oracle import lolmath as lm
from oracle import she_model as sm
from oracle.oracle import Params


class Ladder:
    """The rings of one ptRound: plaintext modulus p = 2^e over R_m, ciphertexts over R_m' (m | m').  `moduli` is U_0:
    Z_i = moduli[i + 1:] (ZqDown each level) and U_i = moduli[i:] (ZqUp Z_i).  make_engine(pps, qs) supplies the engine
    of index m' over a moduli list; cpu is the CPU oracle (the public constants always go through it, in the reference's
    order: mulGPow mod p, decode', embed, crt)."""

    def __init__(self, make_engine, cpu, m, mp, moduli, p, base, rng):
        self.cpu, self.m, self.mp, self.moduli, self.p, self.base, self.rng = cpu, m, mp, list(moduli), int(p), base, rng
        self.e = self.p.bit_length() - 1
        assert self.p == 1 << self.e and self.e >= 1 and mp % m == 0 and len(self.moduli) >= self.e + 1
        self.pps = lm.factor_pps(mp)
        self.zq = [self.moduli[i + 1:] for i in range(self.e)]
        self.uq = [self.moduli[i:] for i in range(self.e - 1)]
        self.ez = [make_engine(self.pps, q) for q in self.zq]
        self.eu = [make_engine(self.pps, q) for q in self.uq]
        self.P_hi = [Params(self.pps, q) for q in self.zq[:2]]
        self.P_lo = [None if m == mp else Params(lm.factor_pps(m), q) for q in self.zq[:2]]
        self.s_all = None

    def keygen(self):
        """one key, given over U_0 and restricted to every other list (the moduli are suffixes of U_0)"""
        full = sm.SHE(self.eu[0] if self.eu else self.ez[0], None, self.uq[0] if self.uq else self.zq[0], self.p, self.rng)
        full.keygen()
        self.s_all = full.s
        return full.s

    def she(self, qs, eng, p, eng_p=None):
        """the model over one moduli list (a suffix of U_0) and plaintext modulus p, with the ladder's key"""
        out = sm.SHE(eng, eng_p, qs, p, self.rng)
        if self.s_all is not None:
            out.s = np.ascontiguousarray(self.s_all[..., self.s_all.shape[-1] - len(qs):])
            out.s_crt = eng.crt(out.s)
        return out

    def round_hints(self):
        """roundHints (HomomPRF.hs:255-258): ksQuadCircHint over U_i, one per level"""
        return [self.she(self.uq[i], self.eu[i], self.p >> i).ks_quad_hint(self.base) for i in range(self.e - 1)]


def _ct(ct):
    return dict(ct, c=[np.ascontiguousarray(x) for x in ct["c"]])


def add_public(L, i, scalar, ct, p):
    """addPublic (fromInteger scalar) ct over Z_i (SymmSHE.hs:381-390): the scalar as an element of R_m"""
    n_m = L.P_hi[i].n if L.P_lo[i] is None else L.P_lo[i].n
    b = np.zeros((1, n_m), dtype=np.int64)
    b[0, 0] = scalar % p
    B = ct["c"][0].shape[0]
    out = pr.add_public(L.cpu, L.P_hi[i], L.P_lo[i], b, dict(ct, c=np.stack(ct["c"])), p, B)
    return _ct(dict(out, c=list(out["c"])))


def ct_mul(L, i, a, b, p):
    """(*) over Z_i (SymmSHE.hs:444-452)"""
    return _ct(L.she(L.zq[i], L.ez[i], p).mul(a, b))


def mod_switch(eng_from, eng_to, ct, p):
    """modSwitch (SymmSHE.hs:243-246)"""
    c, l = mr.mod_switch(eng_from, eng_to, ct["c"], p, ct["enc"], ct["l"])
    return {"enc": "MSD", "k": ct["k"], "l": l, "c": [np.ascontiguousarray(x) for x in c]}


def key_switch_quad(L, i, hint, ct, p):
    """keySwitchQuadCirc over U_i (SymmSHE.hs:361-371)"""
    return _ct(L.she(L.uq[i], L.eu[i], p).key_switch_quad(hint, L.base, ct))


def mod_switch_pt(L, i, ct, p):
    """modSwitchPT from p to p / 2 over Z_i (SymmSHE.hs:255-258)"""
    out = pr.mod_switch_pt(dict(ct, c=np.stack(ct["c"])), L.zq[i], p, p // 2)
    return _ct(dict(out, c=list(out["c"])))


def switch_level(L, i, hint, prod, p):
    """modSwitch $ keySwitchQuadCirc hint $ modSwitch $ prod: Z_i -> U_i -> Z_(i+1) (HomomPRF.hs:262, 269)"""
    up = mod_switch(L.ez[i], L.eu[i], prod, p)
    lin = key_switch_quad(L, i, hint, up, p)
    return mod_switch(L.eu[i], L.ez[i + 1], lin, p)


def pt_round(L, hints, x):
    """ptRound (HomomPRF.hs:237, 260-265).  x over Z_0, plaintext modulus p -> over Z_(e-1), plaintext modulus 2"""
    if L.e == 1:
        return x                                                 # ptRound RHNil x = x
    p = L.p
    x1 = add_public(L, 0, 1, x, p)                              # x' = addPublic one x
    xprod = switch_level(L, 0, hints[0], ct_mul(L, 0, x, x1, p), p)
    xs = [mod_switch_pt(L, 1, add_public(L, 1, y * (-y + 1), xprod, p), p) for y in range(1, p // 4 + 1)]
    return pt_round_internal(L, 1, hints[1:], xs)


def pt_round_internal(L, i, hints, xs):
    """ptRoundInternal (HomomPRF.hs:239, 267-270): xs over Z_i, plaintext modulus p / 2^i"""
    if not hints:
        (x,) = xs                                                # ptRoundInternal RHNil [x] = x
        return x
    p = L.p >> i
    pairs = [xs[j:j + 2] for j in range(0, len(xs), 2)]
    go = lambda a, b: mod_switch_pt(L, i + 1, switch_level(L, i, hints[0], ct_mul(L, i, a, b, p), p), p)
    return pt_round_internal(L, i + 1, hints[1:], [go(a, b) for a, b in pairs])


def decrypt(L, ct):
    """decrypt of a ptRound output (m = m'): over Z_(e-1), plaintext modulus 2 -> [B][n] residues mod 2"""
    assert L.m == L.mp
    ep = sm.CpuEngine(L.cpu, pr.params(L.mp, [2]))
    return L.she(L.zq[-1], L.ez[-1], 2, ep).decrypt(ct)


def encrypt(L, pt):
    """encrypt over Z_0 (m = m'): pt [B][n] residues mod p"""
    return _ct(L.she(L.zq[0], L.ez[0], L.p).encrypt(pt))


def closed_form(c, p):
    """round(2 c / p) with ties towards infinity = msb(c + p/4) = floor((c + p/4) / (p/2)) mod 2 (HomomPRF.hs:223-224)"""
    return ((c + p // 4) // (p // 2)) % 2


def pt_recursion(x, p, ring_mul):
    """The same tree on plaintexts [n] with exact ring arithmetic: prod = x (x + 1) mod p, xs_y = (prod + y (1 - y)) / 2
    mod p/2, then pair products halved into the halved modulus.  Every halving must be exact (asserted)."""
    def half(v, q):
        v = np.asarray(v, dtype=object) % q
        assert not (v % 2).any(), "modSwitchPT of a plaintext that is not a multiple of 2"
        return (v // 2) % (q // 2)
    if p == 2:
        return np.asarray(x, dtype=object) % 2
    one = np.zeros(len(x), dtype=object)
    one[0] = 1
    prod = ring_mul(x, (np.asarray(x, dtype=object) + one) % p, p)
    xs = [half(prod + one * (y * (1 - y)), p) for y in range(1, p // 4 + 1)]
    q = p // 2
    while len(xs) > 1:
        xs = [half(ring_mul(xs[j], xs[j + 1], q), q) for j in range(0, len(xs), 2)]
        q //= 2
    return xs[0] % 2
