"""Big-integer restatement of gadget error correction (class Correct), test-only: written from the definitions in
lol/Crypto/Lol/Types/Unsafe/ZqBasic.hs:234-314 (TrivGad, BaseBGad b over one modulus), lol/Crypto/Lol/Gadget.hs:84-134
(pairs) and lol/Crypto/Lol/Cyclotomic/Cyc.hs:615-621 (coefficient-wise in the decoding basis), in Python integers, so
nothing here can overflow.  Also the gadget itself, Gadget.encode plus noise, and the domain bound of DESIGN.md 3.4j.
Nothing from lol_amd is used: the device is compared against this."""
import numpy as np


def gadlen(b, q):
    k = 0
    while q:
        k, q = k + 1, q // b
    return k


def digits(base, q):
    """entries of the gadget over one modulus: 1 for TrivGad (base 0), gadlen(b, q) for BaseBGad b"""
    return 1 if base == 0 else gadlen(base, q)


def gadget(base, qs):
    """[L][T] residues: b^i in its own component, zero elsewhere, first component first"""
    rows = []
    for t, q in enumerate(qs):
        for i in range(digits(base, q)):
            rows.append([(1 if base == 0 else pow(base, i, q)) % q if s == t else 0 for s in range(len(qs))])
    return rows


def lift(x, q):
    """centred representative in [-q/2, q/2)"""
    x %= q
    return x if 2 * x < q else x - q


def div_mod_cent(a, d):
    quo, rem = divmod(a + d // 2, d)
    return quo, rem - d // 2


def correct_z(q, b, v, trace=None):
    """the error vector of v = s g + e over the integers (correctZ); trace: a dict that receives every intermediate"""
    k = gadlen(b, q)
    assert len(v) == k
    w = [div_mod_cent(b * v[i] - v[i + 1], q)[0] for i in range(k - 1)]
    x = sum(w[i] * (q // b ** (i + 1)) for i in range(k - 1))
    y = [x]
    for i in range(k - 1):
        y.append(b * y[i] - q * w[i])
    vp = [a - c for a, c in zip(v, y)]
    s = div_mod_cent(vp[-1], b ** (k - 1))[0]
    e = [vp[i] - s * b ** i for i in range(k)]
    if trace is not None:
        trace.update(w=w, x=x, y=y, vp=vp, s=s, e=e)
    return e


def correct1(base, q, xs, trace=None):
    """one coefficient over one modulus: entries xs (any integers, taken mod q) -> (u, [e_i])"""
    xs = [x % q for x in xs]
    if base == 0:
        assert len(xs) == 1
        return xs[0], [0]
    e = correct_z(q, base, [lift(x, q) for x in xs], trace)
    return (xs[0] - e[0]) % q, e


def correct_pair(base, qa, qb, rows):
    """one coefficient over the pair: rows [(a, beta)] of length k_a + k_b -> ((u_a, u_b), [e_j])"""
    ka = digits(base, qa)
    qb_inv, qa_inv = pow(qb, -1, qa), pow(qa, -1, qb)
    wa, wb = rows[:ka], rows[ka:]
    xb = [lift(beta, qb) for _, beta in wa]
    va = [qb_inv * (a - x) % qa for (a, _), x in zip(wa, xb)]
    xa = [lift(a, qa) for a, _ in wb]
    vb = [qa_inv * (beta - x) % qb for (_, beta), x in zip(wb, xa)]
    sa, ea = correct1(base, qa, va)
    sb, eb = correct1(base, qb, vb)
    es = [x + qb * e for x, e in zip(xb, ea)] + [x + qa * e for x, e in zip(xa, eb)]
    return (qb * sa % qa, qa * sb % qb), es


def correct(base, qs, xs):
    """xs [L][rows][T] (array or nested lists of integers) -> u [rows][T] in [0, q_t), es [L][rows] (object arrays)"""
    xs = np.asarray(xs, dtype=object)
    L, rows, T = xs.shape
    assert T == len(qs) and T in (1, 2) and L == sum(digits(base, q) for q in qs)
    u = np.zeros((rows, T), dtype=object)
    es = np.zeros((L, rows), dtype=object)
    for r in range(rows):
        if T == 1:
            ur, er = correct1(base, qs[0], [int(xs[j, r, 0]) for j in range(L)])
            u[r, 0] = ur
        else:
            ur, er = correct_pair(base, qs[0], qs[1], [(int(xs[j, r, 0]), int(xs[j, r, 1])) for j in range(L)])
            u[r, 0], u[r, 1] = ur
        for j in range(L):
            es[j, r] = er[j]
    return u, es


def encode(base, qs, s, e=None):
    """out_j = g_j s + reduce (e_j): s [rows][T], e [L][rows] or None -> [L][rows][T] object array in [0, q_t)"""
    g = gadget(base, qs)
    s = np.asarray(s, dtype=object)
    rows, T = s.shape
    out = np.zeros((len(g), rows, T), dtype=object)
    for j, gj in enumerate(g):
        for r in range(rows):
            for t, q in enumerate(qs):
                out[j, r, t] = (gj[t] * int(s[r, t]) + (0 if e is None else int(e[j][r]))) % q
    return out


def error_cap(base, q):
    """the largest |e_j| of the round-trip tests: min (floor (q / (2 (b + 1))), floor ((b^(k-1) - 1) / 2)) - 1"""
    k = gadlen(base, q)
    return min(q // (2 * (base + 1)), (base ** (k - 1) - 1) // 2) - 1


# ---- the domain bound -------------------------------------------------------------------------------
def bound(base, q):
    """dict of the proven bounds over ALL inputs for one modulus: W >= |w_i|, Y[i] >= |y_i| (Y[0] >= |x|), S >= |s|,
    E >= |v'_i|, |e_i|, and `need` = E + b^(k-1), what has to stay below 2^63 (k = 1: e = [0], E bounds v' = v only
    and Ee = 0 the error)"""
    if base == 0 or gadlen(base, q) == 1:
        return dict(W=0, Y=[0], S=q // 2, E=q // 2, Ee=0, need=q // 2 + 1)
    b, k, h = base, gadlen(base, q), q // 2
    W = max((b + 2) * h // q, -(-(b * h) // q))
    Y = [W * (sum(b ** (i - 1 - j) * (q % b ** (j + 1)) for j in range(i)) +
              b ** i * sum(q // b ** (j + 1) for j in range(i, k - 1))) for i in range(k)]
    g = b ** (k - 1)
    S = (h + Y[k - 1] + (g + 1) // 2) // g
    E = max(h + Y[i] + S * b ** i for i in range(k))
    return dict(W=W, Y=Y, S=S, E=E, Ee=E, need=E + g)


def in_domain(base, qs):
    """what lolhip_gadget_correct_batch accepts (T = 1 or 2, coprime pair assumed)"""
    lim = 2 ** 63
    bs = [bound(base, q) for q in qs]
    if any(b["need"] >= lim for b in bs):
        return False
    if len(qs) == 2:
        return all(qs[1 - t] // 2 + qs[1 - t] * bs[t]["Ee"] < lim for t in range(2))
    return True
