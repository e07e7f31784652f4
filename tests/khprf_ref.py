"""CPU restatement of the key-homomorphic ring PRF of lol-apps KeyHomomorphicPRF.hs for the tests: buildDecTree's
buildSubtree and ringPRF', one input at a time, with no sharing between inputs.  Every transform and product goes
through the CPU oracle (CpuRef.crt / crtinv / linv / mul), the gadget decomposition through oracle.she_ref.decompose and
the rounding through oracle.she_ref.div_mod_cent / lift_centered.  Test infrastructure only.

Trees are preorder lists of leaf counts (1 = L, [c, left..., right...] = I c left right); a0, a1 are [L][n] int64 in
the CRT basis of a one-modulus plan."""
import numpy as np

from oracle import she_ref as sr


def parse(tree):
    """preorder leaf counts -> nested ('L',) / ('I', c, left, right)"""
    pos = 0

    def rec():
        nonlocal pos
        c = tree[pos]
        pos += 1
        if c == 1:
            return ("L",)
        left = rec()
        right = rec()
        assert leaves(left) + leaves(right) == c
        return ("I", c, left, right)

    t = rec()
    assert pos == len(tree)
    return t


def leaves(t):
    return 1 if t[0] == "L" else t[1]


def decompose_matrix(cpu, P, row_crt, base):
    """fmap reduce (decomposeMatrix row): [L][n] CRT entries -> [L (digit i)][L (entry j)][n] CRT digits"""
    nL = row_crt.shape[0]
    pow_ = cpu.crtinv(P, row_crt.reshape(nL, P.n, 1))
    digits = sr.decompose(P, pow_, base)                               # [L digits][L entries][n][1]
    return cpu.crt(P, digits.reshape(-1, P.n, 1)).reshape(nL, nL, P.n)


def row_times(cpu, P, lval, dec):
    """the 1 x L row lval times the L x L matrix dec (column j = dec[:, j]): [L][n]"""
    nL = lval.shape[0]
    q = P.qs[0]
    out = np.zeros((nL, P.n), dtype=object)
    for j in range(nL):
        for i in range(nL):
            out[j] += cpu.mul(P, lval[i].reshape(1, P.n, 1), dec[i, j].reshape(1, P.n, 1)).reshape(P.n).astype(object)
    return (out % q).astype(np.int64)


def eval_tree(cpu, P, base, tree, a0, a1, x):
    """A_T(x): buildSubtree x T of buildDecTree (rbits = x & (2^c_r - 1), lbits = x >> c_r), [L][n] CRT basis"""
    def sub(x, t):
        if t[0] == "L":
            return np.asarray(a1 if x else a0, dtype=np.int64)
        _, _, lt, rt = t
        cr = leaves(rt)
        lval = sub(x >> cr, lt)
        rval = sub(x & ((1 << cr) - 1), rt)
        return row_times(cpu, P, lval, decompose_matrix(cpu, P, rval, base))

    t = parse(tree)
    assert 0 <= x < (1 << leaves(t))
    return sub(x, t)


def rescale_dec(cpu, P, y_crt, p):
    """rescaleDec to Z_p of CRT-basis polynomials [.][n]: crtInv, lInv, then rescaleMod per coefficient
    (fst (divModCent (p lift z) q), Prelude.hs:144-153) -> int64 in [0, p)"""
    q = P.qs[0]
    shape = y_crt.shape
    dec = cpu.linv(P, cpu.crtinv(P, y_crt.reshape(-1, P.n, 1))).reshape(shape)
    quot, _ = sr.div_mod_cent(p * sr.lift_centered(dec, q), q)
    return (quot % p).astype(np.int64)


def ring_prf(cpu, P, base, tree, a0, a1, s_crt, p, x):
    """ringPRF s x = (rescaleDec . (s *)) <$> A_T(x): [L][n] decoding-basis residues mod p"""
    A = eval_tree(cpu, P, base, tree, a0, a1, x)
    nL = A.shape[0]
    sA = cpu.mul(P, A.reshape(nL, P.n, 1), np.broadcast_to(np.asarray(s_crt).reshape(1, P.n, 1), (nL, P.n, 1)).copy())
    return rescale_dec(cpu, P, sA.reshape(nL, P.n), p)
