"""tests/modswitch_ref.py — numpy / Python-int restatement of the product-ring rescale (lol Prelude.hs:227-308), of a
ciphertext's modSwitch (lol-apps SymmSHE.hs:236-246) and of tunnelH (HomomPRF.hs:427-431) over the SymmSHE model of
oracle/she_model.py.  TEST INFRASTRUCTURE: every ring operation goes through an engine (CpuEngine or a lol_amd.Plan),
the coefficient-wise rules are written out here in Python integers.

Slabs are [...][T] int64 (component innermost); a ciphertext is the model's dict {"enc", "k", "l", "c": [components]}."""
from __future__ import annotations

import math
from math import prod

import numpy as np

from oracle import lolmath as lm
from oracle import she_model as sm
from oracle import she_ref as sr
from oracle.oracle import Params


def _obj(x):
    return np.asarray(x).astype(object)


def _pack(cols):
    return np.ascontiguousarray(np.stack([c.astype(np.int64) for c in cols], axis=-1))


def lift(a, q):
    """lift (ZqBasic.hs:92-94 with the reference's `2a < q` test): a mod q, then a for 2a < q, else a - q"""
    a = _obj(a) % q
    return np.where(2 * a < q, a, a - q)


def crt_lift(x, qs):
    """residues [...][T] -> centred integers [...] modulo prod qs"""
    x, Q = _obj(x), prod(qs)
    acc = sum(x[..., t] * ((Q // q) * pow(Q // q % q, -1, q)) for t, q in enumerate(qs)) % Q
    return np.where(2 * acc < Q, acc, acc - Q)


# ---- Prelude.hs:227-232: Rescale (a, b) b, one step ----------------------------------------------------------------
def rescale_down1(c, qs):
    """[...][T] over qs -> [...][T-1] over qs[1:]: q_0^-1 (c_s - lift c_0) mod q_s.  Inputs anywhere in (-q, q)."""
    z = lift(np.asarray(c)[..., 0], qs[0])
    return _pack([(_obj(np.asarray(c)[..., s]) - z) * pow(qs[0] % qs[s], -1, qs[s]) % qs[s] for s in range(1, len(qs))])


def rescale_down(c, qs, d):
    """d iterated one-step rescales (NOT one rounding by q_0 ... q_(d-1))"""
    for i in range(d):
        c = rescale_down1(c, qs[i:])
    return c


# ---- Prelude.hs:274-286: Rescale b (a, b), one step ----------------------------------------------------------------
def rescale_up1(c, q_new, qs):
    """[...][T] over qs -> [...][T+1] over [q_new] + qs: (0, q_new c_s)"""
    c = np.asarray(c)
    return _pack([np.zeros(c.shape[:-1], dtype=object)] + [_obj(c[..., s]) * (q_new % qs[s]) % qs[s] for s in range(len(qs))])


def rescale_up(c, qs_new, qs):
    """the moduli qs_new (outermost first) in front of qs, one step each, innermost first"""
    cur = list(qs)
    for qn in reversed(list(qs_new)):
        c = rescale_up1(c, qn, cur)
        cur = [qn] + cur
    return c


def rescale(c, qs_from, qs_to):
    """between suffix-related moduli lists (either direction, or equal: canonical residues)"""
    qs_from, qs_to = list(qs_from), list(qs_to)
    if len(qs_from) >= len(qs_to):
        d = len(qs_from) - len(qs_to)
        assert qs_from[d:] == qs_to
        return rescale_down(c, qs_from, d) if d else _pack([_obj(np.asarray(c)[..., t]) % q for t, q in enumerate(qs_from)])
    u = len(qs_to) - len(qs_from)
    assert qs_to[u:] == qs_from
    return rescale_up(c, qs_to[:u], qs_from)


# ---- SymmSHE.hs:214-246 ---------------------------------------------------------------------------------------------
def to_msd(cs, qs, p, enc, l):
    """toMSD: (components, l') with every residue times p^-1 mod q_t and l times -Q mod p for an LSD input"""
    if enc == "MSD":
        return [_pack([_obj(np.asarray(c)[..., t]) % q for t, q in enumerate(qs)]) for c in cs], int(l) % p
    out = [_pack([_obj(np.asarray(c)[..., t]) * pow(p % q, -1, q) % q for t, q in enumerate(qs)]) for c in cs]
    return out, int(l) * (-prod(qs) % p) % p


def mod_switch(eng_from, eng_to, cs, p, enc="LSD", l=1, cs_crt=False, out_crt=False):
    """modSwitch = modSwitchMSD . toMSD: c_0 rescaled in the decoding basis, the others in the powerful basis.
    cs: a list (or stack) of [B][n][T] components -> ([ncs][B][n][T'] array, l')"""
    qs_f, qs_t = list(eng_from.qs), list(eng_to.qs)
    cs = [np.ascontiguousarray(c) for c in cs]
    cs, l2 = to_msd(cs, qs_f, p, enc, l)
    if cs_crt:
        cs = [eng_from.crtInv(c) for c in cs]
    out = [eng_to.l(rescale(eng_from.lInv(cs[0]), qs_f, qs_t))] + [rescale(c, qs_f, qs_t) for c in cs[1:]]
    out = [np.asarray(c).reshape(cs[0].shape[:-1] + (len(qs_t),)) for c in out]
    if out_crt:
        out = [np.asarray(eng_to.crt(c)).reshape(c.shape) for c in out]
    return np.ascontiguousarray(np.stack(out)), l2


# ---- tunnelH over the model ------------------------------------------------------------------------------------------
class Chain:
    """A tunnelling chain over r_0 -> r_1 -> ... with r' = r (so e' = e = gcd of neighbours), all hops over `up_qs`,
    the input over `in_qs` and the output over `out_qs` (suffixes of up_qs).  make_engine(pps, qs) and
    make_tunnel_engine(pe, pr, ps, qs) supply the engines (the CPU oracle or the GPU)."""

    def __init__(self, make_engine, make_tunnel_engine, ring_ms, up_qs, in_qs, out_qs, p, base, rng):
        self.ms, self.up_qs, self.in_qs, self.out_qs = list(ring_ms), list(up_qs), list(in_qs), list(out_qs)
        self.p, self.base, self.rng, self.mk = int(p), base, rng, make_engine
        assert self.up_qs[len(up_qs) - len(in_qs):] == self.in_qs and self.up_qs[len(up_qs) - len(out_qs):] == self.out_qs
        pps = [lm.factor_pps(m) for m in self.ms]
        # one SHE (and key) per ring over the up list; the end rings also over their own moduli, same keys
        self.she = [sm.SHE(make_engine(pp, self.up_qs), None, self.up_qs, p, rng) for pp in pps]
        for s in self.she:
            s.keygen()
        self.she_in = self._restrict(self.she[0], pps[0], self.in_qs)
        self.she_out = self._restrict(self.she[-1], pps[-1], self.out_qs)
        self.hops = []
        for i in range(len(self.ms) - 1):
            e = math.gcd(self.ms[i], self.ms[i + 1])
            pe = lm.factor_pps(e)
            xeng = make_tunnel_engine(pe, pps[i], pps[i + 1], self.up_qs)
            rel_index = [row[0] for row in lm.ext_indices_coeffs(pe, pps[i])]
            self.hops.append({"pe": pe, "pr": pps[i], "ps": pps[i + 1], "xeng": xeng, "rel_index": rel_index})

    def _restrict(self, she, pps, qs):
        k = len(she.qs) - len(qs)
        out = sm.SHE(self.mk(pps, qs), None, qs, self.p, self.rng)
        out.s = np.ascontiguousarray(she.s[..., k:])
        out.s_crt = out.e.crt(out.s)
        return out

    def gen_hints(self, funcs):
        """funcs[i] [rel_i][n_S_i] residues mod p -> per hop (ys_crt, hints) (she_model.tunnel_hint)"""
        for h, she_r, she_s, f in zip(self.hops, self.she[:-1], self.she[1:], funcs):
            h["ys"], h["hints"] = sm.tunnel_hint(she_r, she_s, h["xeng"], h["rel_index"], f, self.base)

    def tunnel_h(self, ct, steps=None):
        """roundCTDown . roundCTDown . tunnelInternal . roundCTUp on a model ciphertext over in_qs: the hop-by-hop
        composition, every rescale one reference step at a time.  steps (a list) receives every intermediate
        ciphertext.  Returns the model ciphertext over out_qs (powerful basis)."""
        assert len(ct["c"]) == 2 and ct["k"] == 0
        c, l = mod_switch(self.she_in.e, self.she[0].e, ct["c"], self.p, ct["enc"], ct["l"])
        cur = {"enc": "MSD", "k": 0, "l": l, "c": [c[0], c[1]]}
        for h, she_r, she_s in zip(self.hops, self.she[:-1], self.she[1:]):
            if steps is not None:
                steps.append((she_r, cur))
            out = sm.tunnel(she_r, h["xeng"], h["ys"], h["hints"], self.base, cur)
            cur = {"enc": "MSD", "k": 0, "l": out["l"], "c": [she_s.e.crtInv(np.ascontiguousarray(x)) for x in out["c"]]}
        if steps is not None:
            steps.append((self.she[-1], cur))
        qs, pps = list(self.up_qs), lm.factor_pps(self.ms[-1])
        eng = self.she[-1].e
        while len(qs) > len(self.out_qs):                     # one roundCTDown per dropped modulus
            eng2 = self.mk(pps, qs[1:])
            c, l = mod_switch(eng, eng2, cur["c"], self.p, "MSD", cur["l"])
            cur, eng, qs = {"enc": "MSD", "k": 0, "l": l, "c": [c[0], c[1]]}, eng2, qs[1:]
        return cur


def decrypt_lin(she, ct):
    """she_model.SHE.decrypt without the plaintext-ring engine (k = 0): the decoding-basis coefficients of c(s) lifted,
    reduced mod p, scaled by l and taken to the powerful basis by the integer map l.  [B][n] residues mod p."""
    ct = she.toLSD(ct)
    assert ct["k"] == 0
    v_dec = she.lift(she.e.lInv(she.evaluate(ct["c"])))
    x = (v_dec * ct["l"]) % she.p
    x = np.where(2 * x < she.p, x, x - she.p)
    return (she.lift(she.e.l(she.reduce(x))) % she.p).astype(np.int64)


def pt_tunnel(cpuref, ring_ms, big_q, p, x, funcs):
    """evalLin f_k (... evalLin f_1 x) mod p at the plaintext rings (Linear.hs:75-79): every hop over the prime big_q
    (= 1 mod every index) on centred lifts, reduced mod p between hops.  x [B][n_0] mod p, funcs[i] [rel_i][n_(i+1)]."""
    x = np.asarray(x)
    for i, f in enumerate(funcs):
        r, s = ring_ms[i], ring_ms[i + 1]
        PE, PR, PS = (Params(lm.factor_pps(m), [big_q]) for m in (math.gcd(r, s), r, s))
        cen = lambda v: np.where(2 * (_obj(v) % p) < p, _obj(v) % p, _obj(v) % p - p)
        xq = (cen(x) % big_q).astype(np.int64)[..., None]
        fq = (cen(f) % big_q).astype(np.int64)[..., None]
        x_dec = np.asarray(cpuref.linv(PR, np.ascontiguousarray(xq))).reshape(x.shape[0], PR.n, 1)
        f_crt = np.asarray(cpuref.crt(PS, np.ascontiguousarray(fq))).reshape(len(f), PS.n, 1)
        y = np.asarray(cpuref.crtinv(PS, sr.evallin(cpuref, PE, PR, PS, x_dec, f_crt))).reshape(x.shape[0], PS.n)
        x = (lift(y, big_q) % p).astype(np.int64)
    return x


# ---- the chain of the tests: r = 8 -> 12 -> 30 with r' = r over the first three good primes above 2^29 that are
# 1 mod 120 (the up list); the input over the last two, the output over the last one ---------------------------------
CHAIN_MS = (8, 12, 30)
CHAIN_CASES = [(241, 0), (8, 2)]                             # (p, gadget base; 0 = TrivGad)


def chain_moduli():
    g = lm.good_qs(120, 2 ** 29)
    return [next(g) for _ in range(3)]


def run_chain(make_engine, make_tunnel_engine, cpuref, p, base, seed, B=2):
    """the chain property on a model; returns (chain, ct, funcs, x, want) for the callers that go on"""
    up = chain_moduli()
    rng = np.random.default_rng(seed)
    ch = Chain(make_engine, make_tunnel_engine, CHAIN_MS, up, up[1:], up[2:], p, base, rng)
    funcs = []
    for h, she_s in zip(ch.hops, ch.she[1:]):
        funcs.append(rng.integers(0, p, size=(len(h["rel_index"]), she_s.n), dtype=np.int64))
    ch.gen_hints(funcs)
    x = rng.integers(0, p, size=(B, ch.she_in.n), dtype=np.int64)
    x[0] = 0
    x[0, 1] = 1
    ct = ch.she_in.encrypt(x)
    assert np.array_equal(decrypt_lin(ch.she_in, ct), x)
    want = pt_tunnel(cpuref, CHAIN_MS, up[0], p, x, funcs)
    assert want.any()
    return ch, ct, funcs, x, want
