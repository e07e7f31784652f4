#!/usr/bin/env python3
"""tools/bench_pipelines.py — throughput of the SymmSHE pipeline kernels on one MI355X
(BASELINE configs 3 and 5 shapes), of decrypt (`--decrypt`: that leg alone), of encrypt / errorRounded
(`--encrypt`: that leg alone), of the key-switch / tunnel hints (`--kshint`: that leg alone) and of the key-homomorphic
ring PRF (`--khprf`: that leg alone; `--khprf-lifted`: its lifted family over q = 2^k alone), of ciphertext modSwitch
(`--modswitch`: that leg alone), of multi-hop tunnelling (`--tunnel-chain`: that leg alone), of homomorphic rounding
(`--ptround`: that leg alone, also written to profiles/ptround_pipelines.jsonl) and of RLWE instance
verification and gSqNorm (`--rlwe`: that leg alone, also written to profiles/rlwe_pipelines.jsonl) and of the exact ring
product over moduli without a CRT basis (`--ringmul`: that leg alone, also written to profiles/ringmul_pipelines.jsonl)
and of gadget error correction (`--gadget-correct`: that leg alone, also written to profiles/gadget_correct_pipelines.jsonl)
and of L / divG over int64 and double slabs (`--eltops`: that leg alone, also written to profiles/eltops_bench.jsonl)
and of the ciphertext product of any degree (`--ctmul`: that leg alone, also written to profiles/ctmul_bench.jsonl)
and of the key-homomorphic lattice PRF, matrix-core route against VALU route (`--lprf`: that leg alone, also written to
profiles/lprf_bench.jsonl) and of RLWE / RLWR instances over moduli without a CRT basis, fused tails against the general
composition (`--rlwe-ring`: that leg alone, also written to profiles/rlwe_ring_bench.jsonl) and of whole RLWE challenges,
one grouped call against 32 single-secret calls (`--challenge`: that leg alone, also written to
profiles/challenge_bench.jsonl) and of the Gaussian map at primes above 13, the dense stage against the register stage
(`--gauss-dense`: that leg alone, also written to profiles/gauss_dense_bench.jsonl; `--cplx-dense`: the dense complex
CRT leg alone, written to profiles/cplx_dense_bench.jsonl).
`--zq-dense`: the dense Z_q stages at primes above 13 alone, also written to profiles/zq_dense_bench.jsonl.
`--zq-scan`: the scan route of the prime ops at primes above 13 alone, also written to profiles/zq_scan_bench.jsonl.
Operands resident in HBM, HIP events on the launch stream.  Prints one JSON object per line; `alg_bytes` is the compulsory traffic
of the *fused ideal* (each input slab read once, each output written once)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lol_amd  # noqa: E402


def timeit(fn, iters=10, warm=2):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for s, e in ev:
        s.record(); fn(); e.record()
    torch.cuda.synchronize()
    return sum(s.elapsed_time(e) for s, e in ev) / iters


def rnd(gen, qs, *shape):
    return torch.stack([torch.randint(0, q, shape, dtype=torch.int64, device="cuda", generator=gen) for q in qs], dim=-1)


def report(name, cfg, ms, items, alg_bytes, note=None):
    d = {"op": name, "config": cfg, "ms": round(ms, 4), "items_per_s": round(items / ms * 1e3, 1),
         "alg_GBps": round(alg_bytes / ms / 1e6, 1), "frac_of_8TBps": round(alg_bytes / ms / 1e6 / 8000, 4)}
    if note:
        d["note"] = note
    print(json.dumps(d), flush=True)


def good_qs(m, lower, T):
    out, lo = [], lower
    for _ in range(T):
        q = lol_amd.good_q(m, lo)
        out.append(q); lo = q
    return out


def decrypt_leg(gen):
    """SymmSHE errorTerm / decrypt (lolhip_error_term_batch / lolhip_decrypt_batch).  alg_bytes: the ncs component
    slabs read once and the [B][n_m] output written once (the key, shared by the batch, is not counted)."""
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()
    # (label, m, m', moduli, p, B, ncs, k): config 3's product; the reference's decBenches shape (Default.hs:43-44); the
    # widest lift (k_lift at PIPE_MAX_T moduli)
    for label, m, m2, qs, p, B, ncs, k in (("m'=2^15 T=4 59-bit", 2 ** 15, 2 ** 15, good_qs(2 ** 15, 2 ** 59, 4), 65537, 256, 3, 1),
                                           ("m=16 in m'=2048 q=1017857", 16, 2048, [1017857], 16, 8192, 2, 0),
                                           ("m'=2^13 T=16 30-bit", 2 ** 13, 2 ** 13, good_qs(2 ** 13, 2 ** 29, 16), 65537, 256, 2, 0)):
        pq = lol_amd.Plan.for_index(m2, qs)
        pp = lol_amd.Plan.for_index(m2, [p])
        x_p = None if m == m2 else lol_amd.Ext(lol_amd.Plan.for_index(m, [p]), pp)
        n_out = pp.n if x_p is None else x_p.lo.n
        cs = torch.stack([rnd(gen, qs, B, pq.n) for _ in range(ncs)])
        s_crt = rnd(gen, qs, pq.n)
        work = torch.empty((L.lolhip_decrypt_work_len(pq._h, ncs, B),), dtype=torch.int64, device="cuda")
        out = torch.empty((B, n_out), dtype=torch.int64, device="cuda")
        e_out = torch.empty((B, pq.n), dtype=torch.int64, device="cuda")
        slab = B * pq.n * pq.T * 8
        xh = None if x_p is None else x_p._h
        cfg = f"{label} B={B} ncs={ncs} k={k} p={p}"
        for cs_crt in (0, 1):
            rc = L.lolhip_decrypt_batch(pq._h, pp._h, xh, st, ptr(cs), ncs, cs_crt, ptr(s_crt), 0, k, 1, ptr(out), ptr(work), B)
            assert rc == 0, rc
            ms = timeit(lambda: L.lolhip_decrypt_batch(pq._h, pp._h, xh, st, ptr(cs), ncs, cs_crt, ptr(s_crt), 0, k, 1, ptr(out),
                                                       ptr(work), B))
            report("decrypt" + ("_crt_in" if cs_crt else ""), cfg, ms, B, ncs * slab + B * n_out * 8)
        ms = timeit(lambda: L.lolhip_error_term_batch(pq._h, st, ptr(cs), ncs, 0, ptr(s_crt), 0, p, ptr(e_out), ptr(work), B))
        report("errorTerm", cfg, ms, B, ncs * slab + B * pq.n * 8)
        del cs, work, out, e_out


def encrypt_leg(gen):
    """SymmSHE encrypt (lolhip_encrypt_batch, both output bases) and errorRounded (lolhip_error_rounded_batch).
    alg_bytes: the [B][n_m] plaintext read and the [2][B][n'][T] ciphertext written once (encrypt), the [B][n'] output
    written once (errorRounded); the key, shared by the batch, is not counted."""
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()
    key = bytes(range(32))
    # (label, m, m', moduli, p, B, svar): config 3's ring; the reference's sheBenches encrypt shapes (SHEBenches.hs:82-86,
    # Default.hs:40-41); the reference's key-switch index
    for label, m, m2, qs, p, B, svar in (
            ("m'=2^15 T=4 59-bit", 2 ** 15, 2 ** 15, good_qs(2 ** 15, 2 ** 59, 4), 65537, 256, 1.0),
            ("m=16 in m'=1024 q=1017857", 16, 1024, [1017857], 8, 8192, 1.0),
            ("m=16 in m'=2048 q=1017857", 16, 2048, [1017857], 16, 8192, 1.0),
            ("m'=14400 T=2 30-bit", 14400, 14400, good_qs(14400, 2 ** 29, 2), 11, 1024, 1.0)):
        pq = lol_amd.Plan.for_index(m2, qs)
        pp = lol_amd.Plan.for_index(m2, [p])
        x_p = None if m == m2 else lol_amd.Ext(lol_amd.Plan.for_index(m, [p]), pp)
        n_m = pp.n if x_p is None else x_p.lo.n
        pt = torch.randint(0, p, (B, n_m), dtype=torch.int64, device="cuda", generator=gen)
        s_crt = rnd(gen, qs, pq.n)
        work = torch.empty((L.lolhip_encrypt_work_len(pq._h, B),), dtype=torch.int64, device="cuda")
        out = torch.empty((2, B, pq.n, pq.T), dtype=torch.int64, device="cuda")
        z = torch.empty((B, pq.n), dtype=torch.int64, device="cuda")
        xh = None if x_p is None else x_p._h
        cfg = f"{label} B={B} p={p}"
        for out_crt in (1, 0):
            ctr = [0]

            def enc():
                rc = L.lolhip_encrypt_batch(pq._h, pp._h, xh, st, ptr(pt), ptr(s_crt), svar, key, ctr[0], out_crt, ptr(out),
                                            ptr(work), B)
                assert rc == 0, rc
                ctr[0] += B
            ms = timeit(enc)
            report("encrypt" + ("_crt_out" if out_crt else ""), cfg, ms, B, B * n_m * 8 + 2 * B * pq.n * pq.T * 8)
        ms = timeit(lambda: L.lolhip_error_rounded_batch(pq._h, st, svar, key, 0, ptr(z), None, B))
        report("errorRounded", cfg, ms, B, B * pq.n * 8)
        del pt, s_crt, work, out, z


def kshint_leg(gen):
    """Key-switch hints (lolhip_kshint_batch) and one tunnel hint (lolhip_tunnel_hint_batch).  alg_bytes: the [B][n][T]
    values read and the [B][L][2][n][T] hints written once (the key, shared by the batch, and the linearDec table are not
    counted).  At config 3 encrypt to the CRT basis at B = 256 runs in the same process, as the yardstick of the hint
    (same number of LWE samples as B = 64 TrivGad rows)."""
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()
    key = bytes(range(32))
    q3 = good_qs(2 ** 15, 2 ** 59, 4)
    pq, pp = lol_amd.Plan.for_index(2 ** 15, q3), lol_amd.Plan.for_index(2 ** 15, [65537])
    B = 256
    pt = torch.randint(0, 65537, (B, pq.n), dtype=torch.int64, device="cuda", generator=gen)
    s_crt = rnd(gen, q3, pq.n)
    work = torch.empty((L.lolhip_encrypt_work_len(pq._h, B),), dtype=torch.int64, device="cuda")
    out = torch.empty((2, B, pq.n, pq.T), dtype=torch.int64, device="cuda")
    ms = timeit(lambda: L.lolhip_encrypt_batch(pq._h, pp._h, None, st, ptr(pt), ptr(s_crt), 1.0, key, 0, 1, ptr(out),
                                               ptr(work), B))
    report("encrypt_crt_out", f"m'=2^15 T=4 59-bit B={B} p=65537", ms, B, B * pq.n * 8 + 2 * B * pq.n * pq.T * 8)
    del pt, work, out
    # (label, m', moduli, bases, B): config 3's ring; config 5's ring and moduli; the reference's key-switch index
    for label, m, qs, bases, B in (("m'=2^15 T=4 59-bit", 2 ** 15, q3, (0, 2 ** 16), 64),
                                   ("m'=2048 q=1017857*1032193", 2048, [1017857, 1032193], (256,), 64),
                                   ("m'=14400 T=2 30-bit", 14400, good_qs(14400, 2 ** 29, 2), (0, 256), 16)):
        P = lol_amd.Plan.for_index(m, qs)
        s_crt = rnd(gen, qs, P.n)
        vals = rnd(gen, qs, B, P.n)
        for base in bases:
            nL = P.decomposeLen(base)
            work = torch.empty((L.lolhip_kshint_work_len(P._h, base, B),), dtype=torch.int64, device="cuda")
            out = torch.empty((B, nL, 2, P.n, P.T), dtype=torch.int64, device="cuda")
            ctr = [0]

            def hint():
                rc = L.lolhip_kshint_batch(P._h, st, ptr(s_crt), ptr(vals), 1.0, base, key, ctr[0], ptr(out), ptr(work), B)
                assert rc == 0, rc
                ctr[0] += B * nL
            ms = timeit(hint)
            report("ksHint", f"{label} base={base} B={B} L={nL}", ms, B * nL, B * P.n * P.T * 8 + B * nL * 2 * P.n * P.T * 8)
            del work, out
    # one tunnel hint at the shape of lol-apps' chain hops (e, r, s) = (128, 128*7, 128*13)
    qs = good_qs(128 * 7 * 13, 2 ** 29, 2)
    PE, PR, PS = (lol_amd.Plan.for_index(m, qs) for m in (128, 128 * 7, 128 * 13))
    XR, XS = lol_amd.Ext(PE, PR), lol_amd.Ext(PE, PS)
    rel = PR.n // PE.n
    ys = rnd(gen, qs, rel, PS.n)
    s_in, s_out = rnd(gen, qs, PR.n), rnd(gen, qs, PS.n)
    for base in (0, 16):
        nL = PS.decomposeLen(base)
        work = torch.empty((L.lolhip_tunnel_hint_work_len(XR._h, XS._h, base),), dtype=torch.int64, device="cuda")
        out = torch.empty((rel, nL, 2, PS.n, PS.T), dtype=torch.int64, device="cuda")
        ms = timeit(lambda: L.lolhip_tunnel_hint_batch(XR._h, XS._h, st, ptr(ys), ptr(s_in), ptr(s_out), 1.0, base, key, 0,
                                                       ptr(out), ptr(work)))
        report("tunnelHint", f"e=128 r=896 s=1664 T=2 30-bit base={base} rel={rel} L={nL}", ms, rel * nL,
               rel * nL * 2 * PS.n * PS.T * 8)


def khprf_node_bytes(tree, nL, n, x0, B):
    """compulsory bytes of the k_khprf_node launches of one eval over [x0, x0 + B): per internal node its left values
    [U_l][L][n] and right digits [L][U_r][L][n] read once, its [U_v][L][n] written once (int64)"""
    tot = 0

    def U(c, s, leaf):
        return 2 if leaf else min(2 ** c, ((x0 + B - 1) >> s) - (x0 >> s) + 1)

    def rec(pos, s):                    # -> (next pos, leaves)
        c = tree[pos]
        if c == 1:
            return pos + 1, 1
        nonlocal tot
        lpos = pos + 1
        cr = c - tree[lpos]             # the left child's leaf count is the next entry
        nxt, _ = rec(lpos, s + cr)
        nxt2, _ = rec(nxt, s)
        ul = U(tree[lpos], s + cr, tree[lpos] == 1)
        ur = U(cr, s, tree[nxt] == 1)
        uv = B if pos == 0 else U(c, s, False)
        tot += (ul * nL * n + nL * ur * nL * n + uv * nL * n) * 8
        return nxt2, c

    if len(tree) > 1:
        rec(0, 0)
    return tot


def khprf_leg(gen):
    """The key-homomorphic ring PRF (lolhip_khprf_eval_batch, lolhip_khprf_batch).  The reference's benchmark shape
    (KHPRFBenches.hs: 5 leaves, left / balanced / right trees, all 32 inputs, BaseBGad 2) at m = 128 with q = 257, p = 32
    of Examples/KHPRF.hs, and one throughput shape: m = 2^11, q ~ 2^30, BaseBGad 2 (L = 30), a balanced 12-leaf tree,
    B = 4096.  alg_bytes: what the node kernels must move (khprf_node_bytes) for eval, plus the [nkeys][B][L][n]
    output written and read once more for batch.  The split between digit crt, k_khprf_node and the final passes is
    read from a kernel trace of this leg."""
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()
    q30 = lol_amd.good_q(2 ** 11, 2 ** 29)
    for label, m, q, p, base, trees, B in (
            ("m=128 q=257 p=32 k=5", 128, 257, 32, 2,
             (("left", lol_amd.left_spine_tree(5)), ("balanced", lol_amd.balanced_tree(5)),
              ("right", lol_amd.right_spine_tree(5))), 32),
            (f"m=2^11 q={q30} p=2^10 k=12", 2 ** 11, q30, 2 ** 10, 2, (("balanced", lol_amd.balanced_tree(12)),), 4096)):
        P = lol_amd.Plan.for_index(m, [q])
        nL = P.decomposeLen(base)
        g = np.random.default_rng(0)
        a0, a1 = (g.integers(0, q, size=(nL, P.n), dtype=np.int64) for _ in range(2))
        s = torch.randint(0, q, (1, P.n), dtype=torch.int64, device="cuda", generator=gen)
        for tname, tree in trees:
            f = lol_amd.KHPRF(P, base, tree, a0, a1)
            work = torch.empty((max(f.workLen(0, B), 1),), dtype=torch.int64, device="cuda")
            out = torch.empty((B, nL, P.n), dtype=torch.int64, device="cuda")
            nb = khprf_node_bytes(tree, nL, P.n, 0, B)
            cfg = f"{label} {tname} base={base} L={nL} B={B}"
            ms = timeit(lambda: L.lolhip_khprf_eval_batch(f._h, st, 0, B, ptr(out), ptr(work)))
            report("khprf_eval", cfg, ms, B, nb, note="items = inputs; alg = node kernels' compulsory bytes")
            ms = timeit(lambda: L.lolhip_khprf_batch(f._h, st, ptr(s), 1, p, 0, B, ptr(out), ptr(work)))
            report("khprf_prf", cfg + " nkeys=1", ms, B, nb + B * nL * P.n * 8 * 2)
            del work, out, f


def khprf_lifted_leg(gen):
    """The lifted family (lolhip_khprf_create_lifted) at the reference's own benchmark shape: F128, Zq 8 -> Zq 2,
    BaseBGad 2 (L = 4), 5 leaves (left / balanced / right), all 32 inputs, products at a 30-bit NTT prime Q; and a
    balanced 10-leaf tree over all 1024 inputs.  alg_bytes as for the one-modulus leg (node kernels only)."""
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()
    m, q, p, base = 128, 8, 2, 2
    Q = lol_amd.good_q(m, 2 ** 29)
    Pq, PQ = lol_amd.Plan.for_index(m, [q]), lol_amd.Plan.for_index(m, [Q])
    nL = Pq.decomposeLen(base)
    g = np.random.default_rng(0)
    a0, a1 = (g.integers(0, q, size=(nL, Pq.n), dtype=np.int64) for _ in range(2))
    for tname, tree in (("left", lol_amd.left_spine_tree(5)), ("balanced", lol_amd.balanced_tree(5)),
                        ("right", lol_amd.right_spine_tree(5)), ("balanced", lol_amd.balanced_tree(10))):
        B = 1 << tree[0]
        f = lol_amd.KHPRF.lifted(Pq, PQ, base, tree, a0, a1)
        s = f._key_crt(g.integers(0, q, size=(1, Pq.n), dtype=np.int64), 1)
        work = torch.empty((max(f.workLen(0, B), 1),), dtype=torch.int64, device="cuda")
        out = torch.empty((B, nL, Pq.n), dtype=torch.int64, device="cuda")
        nb = khprf_node_bytes(tree, nL, Pq.n, 0, B)
        cfg = f"m=128 q=8 Q={Q} p=2 k={tree[0]} {tname} base={base} L={nL} B={B}"
        ms = timeit(lambda: L.lolhip_khprf_eval_batch(f._h, st, 0, B, ptr(out), ptr(work)))
        report("khprf_lifted_eval", cfg, ms, B, nb, note="items = inputs; alg = node kernels' compulsory bytes")
        ms = timeit(lambda: L.lolhip_khprf_batch(f._h, st, ptr(s), 1, p, 0, B, ptr(out), ptr(work)))
        report("khprf_lifted_prf", cfg + " nkeys=1", ms, B, nb + B * nL * Pq.n * 8 * 2)
        del work, out, f


def public_leg(gen):
    """The SymmSHE public operations and ciphertext addition (lolhip_mul_public_batch, lolhip_add_public_batch,
    lolhip_ct_lincomb_batch).
      1. HomomPRF's first step: mulPublic of B = 4096 public values of R_128 (stride L n, as lolhip_khprf_eval_batch
         writes them) on one shared 2-component ciphertext over ZQ4 at m' = 128*7*13, p = 8; and on the same box the
         direct composition: embedPow, crt at m', a copy and two lolhip_mul_batch against pre-broadcast components.
         alg_bytes: the 2 output slabs written once (the public values and the shared ciphertext are L2-resident).
      2. addPublic at config 3 (m' = 2^15, T = 4, 59-bit, B = 256, MSD in, k = 1), powerful and CRT basis.
         alg_bytes: 2 component slabs read and written once, the [B][n] public values read once.
      3. ct + ct at config 3: 2 + 2 component slabs read, 2 written."""
    import ctypes
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()
    zq4 = [25159681, 19918081, 19393921, 18869761]
    # ---- 1. HomomPRF mulPublic --------------------------------------------------------------
    m, m2, p, B, nL = 128, 128 * 7 * 13, 8, 4096, 3
    hi, lo = lol_amd.Plan.for_index(m2, zq4), lol_amd.Plan.for_index(m, zq4)
    x = lol_amd.Ext(lo, hi)
    T, n, n_m = hi.T, hi.n, lo.n
    a = torch.randint(0, p, (B, nL, n_m), dtype=torch.int64, device="cuda", generator=gen)
    cs = rnd(gen, zq4, 2, 1, n)
    out = torch.empty((2, B, n, T), dtype=torch.int64, device="cuda")
    work = torch.empty((L.lolhip_public_work_len(hi._h, x._h, B),), dtype=torch.int64, device="cuda")
    cfg = f"m=128 in m'={m2} ZQ4 p=8 B={B} stride=L*n shared 2-comp ct"
    wbytes = 2 * B * n * T * 8
    ms = timeit(lambda: L.lolhip_mul_public_batch(hi._h, x._h, st, ptr(a), nL * n_m, p, ptr(cs), 2, 1, ptr(out),
                                                   ptr(work), B))
    report("mul_public", cfg, ms, B, wbytes, note="gather route: lift, crt at m, k_pub_apply")
    # the direct composition; the lift (the same first step in both routes) is done once outside the timing
    v = a[:, 0, :] % p
    v = torch.where(2 * v < p, v, v - p)
    lifted = torch.stack([v % q for q in zq4], dim=-1).contiguous()
    emb = torch.empty((B, n, T), dtype=torch.int64, device="cuda")
    emb1 = torch.empty_like(emb)
    c0, c1 = (cs[i].expand(B, n, T).contiguous() for i in range(2))

    def direct():
        L.lolhip_embed_pow_batch(x._h, st, ptr(emb), ptr(lifted), B)
        L.lolhip_crt_batch(hi._h, st, ptr(emb), B)
        emb1.copy_(emb)
        L.lolhip_mul_batch(hi._h, st, ptr(emb), ptr(c0), B)
        L.lolhip_mul_batch(hi._h, st, ptr(emb1), ptr(c1), B)
    ms_d = timeit(direct)
    report("mul_public_direct", cfg, ms_d, B, wbytes, note="embedPow, crt at m', copy, 2 mul_batch (lift not timed)")
    del a, cs, out, work, emb, emb1, c0, c1, lifted
    # ---- 2. addPublic at config 3 -------------------------------------------------------------
    qs = good_qs(2 ** 15, 2 ** 59, 4)
    P = lol_amd.Plan([(2, 15)], qs)
    pp = lol_amd.Plan([(2, 15)], [65537])
    B = 256
    slab = B * P.n * P.T * 8
    cs = rnd(gen, qs, 2, B, P.n)
    b = torch.randint(-2 ** 40, 2 ** 40, (B, P.n), dtype=torch.int64, device="cuda", generator=gen)
    out = torch.empty_like(cs)
    work = torch.empty((L.lolhip_public_work_len(P._h, None, B),), dtype=torch.int64, device="cuda")
    lo_out = ctypes.c_int64(0)
    for crt in (0, 1):
        ms = timeit(lambda: L.lolhip_add_public_batch(P._h, None, pp._h, st, ptr(b), P.n, ptr(cs), 2, 0, crt, 1, 1, 3,
                                                      65537, ptr(out), ctypes.byref(lo_out), ptr(work), B))
        report("add_public", f"m'=2^15 T=4 59-bit B={B} MSD k=1 {'CRT' if crt else 'powerful'} basis", ms, B,
               4 * slab + B * P.n * 8)
    # ---- 3. ct + ct at config 3 ---------------------------------------------------------------
    d = rnd(gen, qs, 2, B, P.n)
    one = (ctypes.c_int64 * P.T)(*([1] * P.T))
    ms = timeit(lambda: L.lolhip_ct_lincomb_batch(P._h, st, ptr(cs), 2, one, ptr(d), 2, one, ptr(out), B))
    report("ct_add", f"m'=2^15 T=4 59-bit B={B} 2+2 comps", ms, B, 6 * slab)


ZQ5 = [2149056001, 25159681, 19918081, 19393921, 18869761]      # HomomPRFParams.hs ZQ5; ZQ4 and ZQ3 are its suffixes


def modswitch_leg(gen):
    """Ciphertext modSwitch (lolhip_modswitch_batch) against the composition callers used before: lolhip_ct_lincomb_batch
    for toMSD, then one lolhip_rescale_drop_batch per component per dropped modulus on successive plans (with the same
    crtInv / lInv / l / crt around it where the shape asks for them: no l / lInv at m' = 2^k, whose programs are empty
    and which the one call skips too).  The two routes alternate in one process; the median of three rounds is reported.  alg_bytes: (T + T') 8 bytes per coefficient per component."""
    import ctypes
    import statistics
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()
    lo_out = ctypes.c_int64(0)
    q59 = good_qs(2 ** 15, 2 ** 59, 4)
    # (label, index, moduli, moduli kept, B, CRT basis in and out, p)
    for label, m, qs, keep, B, crt, p in (("m'=2^15 59-bit", 2 ** 15, q59, 3, 256, 0, 65537),
                                           ("m'=2^15 59-bit", 2 ** 15, q59, 2, 256, 0, 65537),
                                           ("m'=9*5*7*13 ZQ5->ZQ3", 9 * 5 * 7 * 13, ZQ5, 3, 4096, 1, 8)):
        T = len(qs)
        plans = [lol_amd.Plan.for_index(m, qs[i:]) for i in range(T - keep + 1)]
        F, G = plans[0], plans[-1]
        n, ncs = F.n, 2
        cs = rnd(gen, qs, ncs, B, n)
        out = torch.empty((ncs, B, n, keep), dtype=torch.int64, device="cuda")
        work = torch.empty((max(L.lolhip_modswitch_work_len(F._h, G._h, ncs, B), 1),), dtype=torch.int64, device="cuda")
        tmp = [torch.empty((ncs, B, n, T - i), dtype=torch.int64, device="cuda") for i in range(T - keep + 1)]
        zq = (ctypes.c_int64 * T)(*F.encodeScales(p, True)[0])
        dec = m & (m - 1) != 0                  # the decoding basis differs from the powerful one

        def fused():
            rc = L.lolhip_modswitch_batch(F._h, G._h, st, ptr(cs), ncs, crt, 0, 1, p, ptr(out), crt, ctypes.byref(lo_out),
                                          ptr(work), B)
            assert rc == 0, rc

        def composed():
            L.lolhip_ct_lincomb_batch(F._h, st, ptr(cs), ncs, zq, None, 0, None, ptr(tmp[0]), B)
            if crt:
                L.lolhip_crtinv_batch(F._h, st, ptr(tmp[0]), ncs * B)
            if dec:
                L.lolhip_linv_batch(F._h, st, ptr(tmp[0]), B)
            for i in range(T - keep):
                for c in range(ncs):
                    L.lolhip_rescale_drop_batch(plans[i]._h, st, ptr(tmp[i][c]), ptr(tmp[i + 1][c]), B)
            if dec:
                L.lolhip_l_batch(G._h, st, ptr(tmp[-1]), B)
            if crt:
                L.lolhip_crt_batch(G._h, st, ptr(tmp[-1]), ncs * B)

        fused(); composed()
        torch.cuda.synchronize()
        assert torch.equal(out, tmp[-1]), "the two routes differ"
        t_f, t_c = [], []
        for _ in range(3):
            t_f.append(timeit(fused))
            t_c.append(timeit(composed))
        alg = (T + keep) * 8 * ncs * B * n
        cfg = f"{label} T={T}->{keep} B={B} ncs={ncs} {'CRT in/out' if crt else 'powerful basis'} LSD p={p}"
        report("modswitch", cfg, statistics.median(t_f), B, alg, note="one lolhip_modswitch_batch call")
        report("modswitch_composed", cfg, statistics.median(t_c), B, alg,
               note="ct_lincomb + one rescale_drop per component per dropped modulus (+ the same transforms)")
        del cs, out, work, tmp
    c = rnd(gen, q59, 256, 2 ** 14)
    o = torch.empty((256, 2 ** 14, 3), dtype=torch.int64, device="cuda")
    P = lol_amd.Plan.for_index(2 ** 15, q59)
    ms = timeit(lambda: L.lolhip_rescale_drop_batch(P._h, st, ptr(c), ptr(o), 256))
    report("rescale_drop", "m=2^15 T=4->3 B=256", ms, 256, 256 * 2 ** 14 * 7 * 8)


def tunnel_chain_leg(gen):
    """tunnelH (lolhip_tunnel_chain_batch) over the reference's five hops (HomomPRFParams.hs RngList, primed rings), up
    list ZQ5, in ZQ4, out ZQ3, base 2, B = 64, random hints (timing only), against the same steps through the Python
    methods one call at a time.  alg_bytes: the input and output ciphertexts (the hops' traffic is not modelled)."""
    st = torch.cuda.current_stream().cuda_stream
    base, B, p = 2, 64, 8
    rs = [128, 64 * 7, 32 * 7 * 13, 8 * 5 * 7 * 13, 4 * 3 * 5 * 7 * 13, 9 * 5 * 7 * 13]
    rps = [128 * 7 * 13, 64 * 7 * 13] + rs[2:]
    import math
    Rp = [lol_amd.Plan.for_index(m, ZQ5) for m in rps]
    exts_er, exts_es, ys, hints = [], [], [], []
    for i in range(5):
        E = lol_amd.Plan.for_index(math.gcd(rs[i], rs[i + 1]) * (rps[i] // rs[i]), ZQ5)
        exts_er.append(lol_amd.Ext(E, Rp[i])); exts_es.append(lol_amd.Ext(E, Rp[i + 1]))
        rel, S = Rp[i].n // E.n, Rp[i + 1]
        ys.append(rnd(gen, ZQ5, rel, S.n))
        hints.append(rnd(gen, ZQ5, rel, S.decomposeLen(base), 2, S.n))
    p_in, p_mid, p_out = lol_amd.Plan.for_index(rps[0], ZQ5[1:]), lol_amd.Plan.for_index(rps[-1], ZQ5[1:]), lol_amd.Plan.for_index(rps[-1], ZQ5[2:])
    chain = lol_amd.TunnelChain(exts_er, exts_es, ys, hints, base, p_in, p_out)
    cs = rnd(gen, ZQ5[1:], 2, B, p_in.n)
    L = lol_amd.lib()
    import ctypes
    work = torch.empty((chain.workLen(B),), dtype=torch.int64, device="cuda")
    out = torch.empty((2, B, p_out.n, p_out.T), dtype=torch.int64, device="cuda")
    lo_out = ctypes.c_int64(0)

    def one_call():
        rc = L.lolhip_tunnel_chain_batch(chain._h, st, cs.data_ptr(), 0, 0, 1, p, out.data_ptr(), 0, ctypes.byref(lo_out),
                                         work.data_ptr(), B)
        assert rc == 0, rc

    res = []

    def hop_by_hop():
        cur, _, l = p_in.modSwitch(Rp[0], cs, p, "LSD", 1)
        for xr, xs, R, S, y, h in zip(exts_er, exts_es, Rp[:-1], Rp[1:], ys, hints):
            c0 = R.lInv(cur[0])
            cur = S.crtInv(xr.tunnel(xs, c0, cur[1], y, h, base))
        cur, _, l = Rp[-1].modSwitch(p_mid, cur, p, "MSD", l)
        cur, _, l = p_mid.modSwitch(p_out, cur, p, "MSD", l)
        res[:] = [cur]

    one_call(); hop_by_hop()
    torch.cuda.synchronize()
    assert torch.equal(out, res[0]), "the two routes differ"
    alg = 8 * 2 * B * (p_in.n * p_in.T + p_out.n * p_out.T)
    cfg = f"RngList 5 hops {rps[0]}->{rps[-1]} ZQ4 -> ZQ5 -> ZQ3 base={base} B={B}"
    report("tunnel_chain", cfg, timeit(one_call, iters=5), B, alg, note="one lolhip_tunnel_chain_batch call")
    report("tunnel_chain_hop_by_hop", cfg, timeit(hop_by_hop, iters=5), B, alg,
           note="Plan.modSwitch up, per hop lInv / Ext.tunnel / crtInv, two Plan.modSwitch down")


def ptround_leg(gen):
    """Homomorphic rounding 2^e -> 2 (lolhip_ptround_batch) at the tail of HomomPRF: index 9*5*7*13 (n' = 1728, m = m'),
    p = 8, ZQ3 -> ZQ1 with the up lists ZQ4 / ZQ3, base 2, B = 512 (the key switch's digit buffer over ZQ4 is then
    L B n' T 8 bytes = 100 * 512 * 1728 * 4 * 8 = 2.8 GB), random hints (timing only).
      (a) k_ct_affine_mul against the same step composed from the entries that were there before it: level 0 as
          lolhip_add_public_batch then lolhip_ctmul_crt_batch; the fan-out + pair step as two lolhip_add_public_batch, two
          toMSD (modSwitchPT) and one toLSD ((*) of two MSD operands) through lolhip_ct_lincomb_batch, then
          lolhip_ctmul_crt_batch.  The routes alternate in one process, five rounds of ten calls; median, min and max.
      (b) the whole chain and every pass of it alone at the chain's shapes.
      (c) the achieved bytes/s of (a) against lolhip_copy_slab on a slab of the product's size.
    alg_bytes of the products: 2 component slabs read and 3 written (gCRT and the constants are cache-resident).
    Also written to profiles/ptround_pipelines.jsonl."""
    import ctypes
    import statistics
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()
    m, p, base, B = 9 * 5 * 7 * 13, 8, 2, 512
    lv = [lol_amd.Plan.for_index(m, ZQ5[2 + i:]) for i in range(3)]
    up = [lol_amd.Plan.for_index(m, ZQ5[1 + i:]) for i in range(2)]
    pp = lol_amd.Plan.for_index(m, [p])
    n = lv[0].n
    lines = []

    def rep(name, cfg, times, items, alg, note=None):
        ms = statistics.median(times)
        d = {"op": name, "config": cfg, "ms": round(ms, 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4),
             "rounds": len(times), "items_per_s": round(items / ms * 1e3, 1), "alg_GBps": round(alg / ms / 1e6, 1),
             "frac_of_8TBps": round(alg / ms / 1e6 / 8000, 4)}
        if note:
            d["note"] = note
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def alternate(f, g, rounds=5):
        tf, tg = [], []
        for _ in range(rounds):
            tf.append(timeit(f)); tg.append(timeit(g))
        return tf, tg

    arr = lambda P, v: (ctypes.c_int64 * P.T)(*[int(x) for x in v])
    lo_out = ctypes.c_int64(0)
    one_src = torch.zeros((1, n), dtype=torch.int64, device="cuda"); one_src[0, 0] = 1
    # ---- (a) level 0: x (p x + 1), MSD input, k = 0 -------------------------------------------------------------------
    Z = lv[0]
    slab = B * n * Z.T * 8
    x = rnd(gen, Z.qs, 2, B, n)
    v1 = rnd(gen, Z.qs, 1, n)
    prod = torch.empty((1, 3, B, n, Z.T), dtype=torch.int64, device="cuda")
    xp = torch.empty_like(x)
    e = [torch.empty((B, n, Z.T), dtype=torch.int64, device="cuda") for _ in range(3)]
    wpub = torch.empty((max(L.lolhip_public_work_len(Z._h, None, B), 1),), dtype=torch.int64, device="cuda")
    ones, ps = arr(Z, [1] * Z.T), arr(Z, [p] * Z.T)

    def fused0():
        rc = L.lolhip_ct_affine_mul_batch(Z._h, st, ptr(x), ones, None, ptr(x), ps, ptr(v1), 1, ptr(prod), B)
        assert rc == 0, rc

    def composed0():
        rc = L.lolhip_add_public_batch(Z._h, None, pp._h, st, ptr(one_src), 0, ptr(x), 2, 0, 1, 1, 0, 1, p, ptr(xp),
                                       ctypes.byref(lo_out), ptr(wpub), B)
        assert rc == 0, rc
        L.lolhip_ctmul_crt_batch(Z._h, st, ptr(x[0]), ptr(x[1]), ptr(xp[0]), ptr(xp[1]), ptr(e[0]), ptr(e[1]), ptr(e[2]), B)

    # the same words: the fused pass given the constant the composed route adds, decode'(l^-1) with l = 1 through toLSD
    # (a scalar with k = 0 is a constant vector in the CRT basis)
    dec = lambda v: v % p - p if 2 * (v % p) >= p else v % p
    v1[:] = torch.tensor([dec(pow(Z.encodeScales(p, False)[1], -1, p)) % q for q in Z.qs], dtype=torch.int64, device="cuda")
    fused0(); composed0()
    torch.cuda.synchronize()
    assert all(torch.equal(prod[0, i], e[i]) for i in range(3)), "level 0: the two routes differ"
    cfg = f"m'={m} ZQ3 p={p} B={B} MSD k=0"
    tf, tc = alternate(fused0, composed0)
    rep("ptround_level0_fused", cfg, tf, B, 5 * slab, note="one k_ct_affine_mul pass")
    rep("ptround_level0_composed", cfg, tc, B, 5 * slab, note="lolhip_add_public_batch then lolhip_ctmul_crt_batch")
    # ---- (a) fan-out + pair over Z_1: (p_1 (xprod + v_1)) (xprod + v_2) ---------------------------------------------------
    Z = lv[1]
    slab = B * n * Z.T * 8
    x = rnd(gen, Z.qs, 2, B, n)
    prod = torch.empty((1, 3, B, n, Z.T), dtype=torch.int64, device="cuda")
    xs = [torch.empty_like(x) for _ in range(2)]
    e = [torch.empty((B, n, Z.T), dtype=torch.int64, device="cuda") for _ in range(3)]
    wpub = torch.empty((max(L.lolhip_public_work_len(Z._h, None, B), 1),), dtype=torch.int64, device="cuda")
    ys = [torch.zeros((1, n), dtype=torch.int64, device="cuda") for _ in range(2)]
    ys[1][0, 0] = -2                                                 # y (1 - y) for y = 1, 2
    zq_m = arr(Z, Z.encodeScales(p, True)[0])                       # toMSD over plaintext modulus p
    zq_l = arr(Z, Z.encodeScales(p // 2, False)[0])                 # toLSD over p / 2
    inv_p = [pow(p, -1, q) for q in Z.qs]
    # the constants as the fused pass takes them: addPublic's polynomial through toMSD's p^-1 (and toLSD's p_1 on the a side);
    # a scalar with l = 1 and k = 0 is a constant vector in the CRT basis
    va = torch.tensor([[0] * Z.T] * n, dtype=torch.int64, device="cuda").reshape(1, n, Z.T)
    c2 = dec(-2 * pow(Z.encodeScales(p, False)[1], -1, p))
    vb = torch.tensor([[(c2 * w) % q for w, q in zip(inv_p, Z.qs)]] * n, dtype=torch.int64, device="cuda").reshape(1, n, Z.T)
    ones = arr(Z, [1] * Z.T)

    def fused1():
        rc = L.lolhip_ct_affine_mul_batch(Z._h, st, ptr(x), zq_l, ptr(va), ptr(x), ones, ptr(vb), 1, ptr(prod), B)
        assert rc == 0, rc

    def composed1():
        for y, o in zip(ys, xs):
            rc = L.lolhip_add_public_batch(Z._h, None, pp._h, st, ptr(y), 0, ptr(x), 2, 0, 1, 1, 0, 1, p, ptr(o),
                                           ctypes.byref(lo_out), ptr(wpub), B)
            assert rc == 0, rc
            L.lolhip_ct_lincomb_batch(Z._h, st, ptr(o), 2, zq_m, None, 0, None, ptr(o), B)       # modSwitchPT: toMSD
        L.lolhip_ct_lincomb_batch(Z._h, st, ptr(xs[0]), 2, zq_l, None, 0, None, ptr(xs[0]), B)   # (*): toLSD of the first
        L.lolhip_ctmul_crt_batch(Z._h, st, ptr(xs[0][0]), ptr(xs[0][1]), ptr(xs[1][0]), ptr(xs[1][1]), ptr(e[0]), ptr(e[1]),
                                 ptr(e[2]), B)

    fused1(); composed1()
    torch.cuda.synchronize()
    assert all(torch.equal(prod[0, i], e[i]) for i in range(3)), "fan-out: the two routes differ"
    cfg = f"m'={m} ZQ2 p={p} B={B} one pair"
    tf, tc = alternate(fused1, composed1)
    rep("ptround_fanout_pair_fused", cfg, tf, B, 5 * slab, note="one k_ct_affine_mul pass")
    rep("ptround_fanout_pair_composed", cfg, tc, B, 5 * slab,
        note="2 lolhip_add_public_batch, 3 lolhip_ct_lincomb_batch (2 toMSD, 1 toLSD), lolhip_ctmul_crt_batch")
    # ---- (c) the copy yardstick on a slab of the level-0 product's traffic ----------------------------------------------
    words = 5 * B * n * lv[0].T // 2
    src = torch.empty((words,), dtype=torch.int64, device="cuda"); dst = torch.empty_like(src)
    tcopy = [timeit(lambda: L.lolhip_copy_slab(st, ptr(dst), ptr(src), words * 8, 0)) for _ in range(5)]
    rep("copy_slab", f"{words * 8 >> 20} MiB read + written", tcopy, B, 2 * words * 8, note="lolhip_copy_slab, the HBM yardstick")
    del x, prod, xs, e, src, dst, xp
    # ---- (b) the whole chain and its passes ------------------------------------------------------------------------------
    hints = [rnd(gen, U.qs, U.decomposeLen(base), 2, n) for U in up]
    chain = lol_amd.PTRound(lv, up, hints, base, p, pp_m=pp)
    cs = rnd(gen, lv[0].qs, 2, B, n)
    work = torch.empty((chain.workLen(B),), dtype=torch.int64, device="cuda")
    out = torch.empty((2, B, n, lv[2].T), dtype=torch.int64, device="cuda")
    ko = ctypes.c_int64(0)

    def whole():
        rc = L.lolhip_ptround_batch(chain._h, st, ptr(cs), 1, 1, 0, 1, ptr(out), 1, ctypes.byref(ko), ctypes.byref(lo_out),
                                    ptr(work), B)
        assert rc == 0, rc

    cfg = f"m'={m} p={p} ZQ3 -> ZQ1 up ZQ4 / ZQ3 base={base} B={B} CRT in/out"
    alg = 8 * 2 * B * n * (lv[0].T + lv[2].T)
    rep("ptround", cfg, [timeit(whole, iters=5) for _ in range(3)], B, alg,
        note=f"one lolhip_ptround_batch call; work {work.numel() * 8 >> 20} MiB; alg_bytes: the input and output ciphertexts")
    del work
    for i in range(2):
        Zi, U, Zn = lv[i], up[i], lv[i + 1]
        pi = p >> i
        p3 = rnd(gen, Zi.qs, 3, B, n)
        u3 = torch.empty((3, B, n, U.T), dtype=torch.int64, device="cuda")
        k2 = torch.empty((2, B, n, U.T), dtype=torch.int64, device="cuda")
        o2 = torch.empty((2, B, n, Zn.T), dtype=torch.int64, device="cuda")
        Ld = U.decomposeLen(base)
        dig = torch.empty((Ld, B, n, U.T), dtype=torch.int64, device="cuda")
        sub = torch.empty((max(3 * B * n * Zi.T, 2 * B * n * U.T),), dtype=torch.int64, device="cuda")
        x2 = rnd(gen, Zi.qs, 2, B, n)
        one_i = arr(Zi, [1] * Zi.T)
        w = 8 * B * n
        steps = (
            ("k_ct_affine_mul", lambda: L.lolhip_ct_affine_mul_batch(Zi._h, st, ptr(x2), one_i, None, ptr(x2), one_i, None, 1, ptr(p3), B), 5 * w * Zi.T),
            ("modswitch up (3 comps, CRT -> powerful)", lambda: L.lolhip_modswitch_batch(Zi._h, U._h, st, ptr(p3), 3, 1, 1, 1, pi, ptr(u3), 0, ctypes.byref(lo_out), ptr(sub), B), 3 * w * (Zi.T + U.T)),
            ("crt c0, c1", lambda: L.lolhip_crt_batch(U._h, st, ptr(u3), 2 * B), 4 * w * U.T),
            ("keyswitch", lambda: L.lolhip_keyswitch_batch(U._h, st, ptr(u3[2]), base, ptr(hints[i]), 2, ptr(u3), ptr(k2), ptr(dig), B), 5 * w * U.T),
            ("modswitch down (2 comps, CRT -> CRT)", lambda: L.lolhip_modswitch_batch(U._h, Zn._h, st, ptr(k2), 2, 1, 1, 1, pi, ptr(o2), 1, ctypes.byref(lo_out), ptr(sub), B), 2 * w * (U.T + Zn.T)),
        )
        for name, fn, ab in steps:
            assert fn() == 0
            rep(f"  level {i}: {name}", f"T={Zi.T} up {U.T} L={Ld}", [timeit(fn, iters=5) for _ in range(3)], B, ab)
        del p3, u3, k2, o2, dig, sub, x2
    os.makedirs(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"), exist_ok=True)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ptround_pipelines.jsonl")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def rlwe_leg(gen):
    """RLWE instance verification norm-only (lolhip_rlwe_error_batch with e_out = NULL) and gSqNorm alone
    (lolhip_gsqnorm_batch), at the challenge shape and at m = 2^14.  alg_bytes: a and b read once and the [B] norms
    written (verify; the secret, shared by the batch, is not counted); e read once and the norms written (gsqnorm)."""
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()
    key = bytes(range(32))
    lines = []

    def rep(name, cfg, ms, items, alg):
        d = {"op": name, "config": cfg, "ms": round(ms, 4), "items_per_s": round(items / ms * 1e3, 1),
             "alg_GBps": round(alg / ms / 1e6, 1)}
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    for label, m, q, B, svar in (("m=256 q=7681", 256, 7681, 65536, 0.28125),
                                 ("m=2^14 30-bit", 2 ** 14, lol_amd.good_q(2 ** 14, 2 ** 29), 4096, 0.28125)):
        P = lol_amd.Plan.for_index(m, [q])
        n = P.n
        s_crt = torch.empty((n, 1), dtype=torch.int64, device="cuda")
        assert L.lolhip_rlwe_secret(P._h, st, key, 0, ptr(s_crt)) == 0
        a = torch.empty((B, n, 1), dtype=torch.int64, device="cuda")
        nm = torch.empty((B,), dtype=torch.int64, device="cuda")
        cfg = f"{label} T=1 B={B}"
        for kind, name in ((0, "rlwe_verify_disc"), (1, "rlwe_verify_cont")):
            work = torch.empty((L.lolhip_rlwe_work_len(P._h, kind, B),), dtype=torch.int64, device="cuda")
            b = torch.empty((B, n), dtype=torch.int64, device="cuda")           # 8-byte words of either kind
            assert L.lolhip_rlwe_sample_batch(P._h, st, kind, 0, ptr(s_crt), svar, key, 0, ptr(a), ptr(b), ptr(work), B) == 0
            call = lambda: L.lolhip_rlwe_error_batch(P._h, st, kind, ptr(a), ptr(b), ptr(s_crt), None, ptr(nm), ptr(work), B)
            assert call() == 0
            rep(name, cfg, timeit(call), B, 2 * B * n * 8 + B * 8)
            del work, b
        e = torch.randint(-2 ** 20, 2 ** 20, (B, n), dtype=torch.int64, device="cuda", generator=gen)
        rep("gsqnorm_i64", cfg, timeit(lambda: L.lolhip_gsqnorm_batch(P._h, st, ptr(e), ptr(nm), B)), B, B * n * 8 + B * 8)
        del a, e, nm
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rlwe_pipelines.jsonl")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def ringmul_leg(gen):
    """The exact ring product over q = 2^8 (one NTT prime, a 32-bit class) and q = 2^32 (two primes) at m = 16384,
    B = 4096: lolhip_ringmul_batch beside lolhip_polymul_batch on the same plan_Q and batch in the same process, so the
    difference is the two passes (k_ring_lift twice, k_ring_fold once: (3 + 3 K) 8 bytes per word of an operand), against
    lolhip_copy_slab on a slab of the lifted operand's size.  Median of five rounds of ten calls.
    Also written to profiles/ringmul_pipelines.jsonl."""
    import statistics
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()
    lines = []

    def rep(name, cfg, ts, items, alg_bytes, note=None):
        ms = statistics.median(ts)
        d = {"op": name, "config": cfg, "ms": round(ms, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
             "items_per_s": round(items / ms * 1e3, 1), "alg_GBps": round(alg_bytes / ms / 1e6, 1)}
        if note:
            d["note"] = note
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        return ms

    m, B = 16384, 4096
    for q in (2 ** 8, 2 ** 32):
        rm = lol_amd.RingMul(lol_amd.Plan.for_index(m, [q]))
        n, K, PQ = rm.n, rm.K, rm.plan_Q
        words = B * n
        cfg = f"m={m} q=2^{q.bit_length() - 1} Q={PQ.qs} B={B}"
        a, b = (torch.randint(-2 ** 63, 2 ** 63 - 1, (B, n, 1), dtype=torch.int64, device="cuda", generator=gen) for _ in range(2))
        out = torch.empty_like(a)
        work = torch.empty((rm.workLen(B),), dtype=torch.int64, device="cuda")
        la, lb = work[:words * K], work[words * K:2 * words * K]
        bhat = rm.prepare(b)
        rounds = lambda fn: [timeit(fn) for _ in range(5)]
        t_ring = rep("ringmul", cfg, rounds(lambda: L.lolhip_ringmul_batch(rm._h, st, ptr(out), ptr(a), ptr(b), ptr(work), B)),
                     B, 3 * words * 8, note="alg = a, b read and out written once")
        t_pm = rep("  polymul(plan_Q)", cfg, rounds(lambda: L.lolhip_polymul_batch(PQ._h, st, ptr(la), ptr(la), ptr(lb), B)),
                   B, 3 * words * K * 8, note="the lifted slabs of the call above, c = a as inside it")
        t_copy = rep("  copy_slab", f"{words * K * 8 >> 20} MiB read + written",
                     rounds(lambda: L.lolhip_copy_slab(st, ptr(lb), ptr(la), words * K * 8, 0)), B, 2 * words * K * 8,
                     note="lolhip_copy_slab, the HBM yardstick")
        pass_bytes = (3 + 3 * K) * words * 8
        d = {"op": "  lift + lift + fold", "config": cfg, "ms": round(t_ring - t_pm, 4),
             "alg_GBps": round(pass_bytes / (t_ring - t_pm) / 1e6, 1),
             "copy_GBps": round(2 * words * K * 8 / t_copy / 1e6, 1), "note": "ringmul - polymul, medians; (3 + 3 K) 8 bytes per word"}
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        rep("ringmul_prepared", cfg + " Bb=B", rounds(lambda: L.lolhip_ringmul_prepared_batch(rm._h, st, ptr(out), ptr(a), ptr(bhat), B, ptr(work), B)),
            B, (2 + K) * words * 8, note="lift, crt, pointwise product, crtInv, fold")
        del a, b, out, work, bhat, la, lb, rm
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    with open(os.path.join(root, "profiles", "ringmul_pipelines.jsonl"), "w") as f:
        f.write("\n".join(lines) + "\n")


def rlwe_ring_leg(gen):
    """RLWE / RLWR instances over moduli without a CRT basis (lolhip_rlwe_ring_*) at (m, q) = (256, 512), (512, 2^17),
    (1155, 2^18) and (2^14, 2^17), one slab of a of at least 1 GiB: RLWR sample, Disc sample and Disc error + norm, on the
    route the library picks and, at the 2-power indices, on the general composition (debug switch RLWE_RING_UNFUSED),
    beside lolhip_ringmul_prepared_batch (Bb = 1) on the same (m, q, B) and lolhip_copy_slab on a slab of a's size, all in
    the same process.  yard_ms = the prepared product's time + `extra_words` slab words (read or written beyond the
    prepared product's own traffic, counted from the launch plan) at the copy's measured rate; over_yard = ms / yard_ms.
    Median of five rounds of ten calls.  Also written to profiles/rlwe_ring_bench.jsonl."""
    import statistics
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()
    lines = []
    rounds = lambda fn: [timeit(fn) for _ in range(5)]

    def rep(name, cfg, ts, items, **more):
        ms = statistics.median(ts)
        d = {"op": name, "config": cfg, "ms": round(ms, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
             "items_per_s": round(items / ms * 1e3, 1)}
        d.update(more)
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        return ms

    # slab words moved beyond lolhip_ringmul_prepared_batch's own (lift: 1 + K, the transforms and the product: 6 K,
    # fold: K + 1), by the launch plans of include/lolhip.h: (fused, general at a 2-power, general elsewhere)
    EXTRA = {"rlwr_sample": (0, 2, 4), "disc_sample": (0, 2, 8), "disc_error_norm": (2, 4, 6)}
    key, svar = bytes(range(32)), 7.8125e-3
    for m, q in ((256, 512), (512, 2 ** 17), (1155, 2 ** 18), (2 ** 14, 2 ** 17)):
        P = lol_amd.Plan.for_index(m, [q])
        r = lol_amd.RingRLWE(P)
        n, K, h = P.n, r.K, r.ring._h
        two_power = m & (m - 1) == 0
        B = -(-2 ** 30 // (n * 8))
        words, slab = B * n, B * n * 8
        cfg = f"m={m} n={n} q={q} K={K} B={B} ({slab >> 20} MiB)"
        _, shat = r.secret(key=key, ctr=0)
        a, b = (torch.empty((B, n), dtype=torch.int64, device="cuda") for _ in range(2))
        e = torch.empty((B, n), dtype=torch.int64, device="cuda")
        nm = torch.empty((B,), dtype=torch.int64, device="cuda")
        work = torch.empty((max(L.lolhip_rlwe_ring_work_len(h, P._h, 0, B), r.ring.workLen(B)),), dtype=torch.int64, device="cuda")
        t_copy = rep("  copy_slab", cfg, rounds(lambda: L.lolhip_copy_slab(st, ptr(e), ptr(b), slab, 0)), B,
                     note="lolhip_copy_slab, the HBM yardstick: one slab word read and one written")
        word_ms = t_copy / (2 * words)
        assert L.lolhip_rlwe_ring_sample_batch(h, P._h, st, 0, 0, ptr(shat), svar, key, 0, ptr(a), ptr(b), ptr(work), B) == 0
        t_prep = rep("  ringmul_prepared", cfg + " Bb=1",
                     rounds(lambda: L.lolhip_ringmul_prepared_batch(h, st, ptr(e), ptr(a), ptr(shat), 1, ptr(work), B)), B,
                     note="lift, crt, pointwise product, crtInv, fold")
        calls = {
            "rlwr_sample": lambda: L.lolhip_rlwe_ring_sample_batch(h, P._h, st, 2, 2, ptr(shat), 1.0, key, 0, ptr(a), ptr(b), ptr(work), B),
            "disc_sample": lambda: L.lolhip_rlwe_ring_sample_batch(h, P._h, st, 0, 0, ptr(shat), svar, key, 0, ptr(a), ptr(b), ptr(work), B),
            "disc_error_norm": lambda: L.lolhip_rlwe_ring_error_batch(h, P._h, st, 0, ptr(a), ptr(b), ptr(shat), ptr(e), ptr(nm), ptr(work), B),
        }
        for unfused in ((False, True) if two_power else (True,)):
            lol_amd.debug_set("RLWE_RING_UNFUSED", unfused)
            try:
                for name in ("rlwr_sample", "disc_sample", "disc_error_norm"):    # the Disc sample leaves (a, b) for the error call
                    extra = EXTRA[name][0 if not unfused else 1 if two_power else 2]
                    assert calls[name]() == 0
                    ts = rounds(calls[name])
                    yard = t_prep + extra * words * word_ms
                    rep(f"rlwe_ring_{name}" + ("(unfused)" if unfused and two_power else ""), cfg, ts, B,
                        route="unfused" if unfused else "fused", extra_words=extra, yard_ms=round(yard, 4),
                        over_yard=round(statistics.median(ts) / yard, 4))
            finally:
                lol_amd.debug_set("RLWE_RING_UNFUSED", False)
        torch.cuda.synchronize()
        del a, b, e, nm, work, shat, r, P
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    with open(os.path.join(root, "profiles", "rlwe_ring_bench.jsonl"), "w") as f:
        f.write("\n".join(lines) + "\n")


def challenge_leg(gen):
    """One whole challenge of I = 32 instances, generate and verify (Disc and RLWR), at L = 3 and L = 100 on m = 256 /
    q = 769 (lolhip_chall_*, a CRT basis) and m = 256 / q = 512 (lolhip_chall_ring_*): the grouped call against the same
    work as 32 single-secret calls in the same process.  The single-secret generate is secret + sample per instance and
    then the three basis changes over the whole arrays (the grouped call returns the decoding basis); the single-secret
    verify is the basis changes, prepare (ring) and error + norm / check per instance.  Both verifies end with the copy of
    their verdicts to the host (32 counts, or 32 L norms).  Times include the launch path: at L = 3 that is the point.
    Median of five rounds of ten calls, HIP events.  Also written to profiles/challenge_bench.jsonl."""
    import statistics
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()
    lines = []
    key, svar, I, m, p = bytes(range(32)), 7.8125e-3, 32, 256, 2
    i64 = lambda *sh: torch.empty(sh, dtype=torch.int64, device="cuda")

    def rep(name, cfg, ts, **more):
        d = {"op": name, "config": cfg, "ms": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4),
             "ms_max": round(max(ts), 4)}
        d.update(more)
        lines.append(d)
        print(json.dumps(d), flush=True)
        return d["ms"]

    def ok(rc):
        assert rc == 0, rc

    for q in (769, 512):
        P = lol_amd.Plan.for_index(m, [q])
        ring = not P.has_crt
        r = lol_amd.RingRLWE(P) if ring else lol_amd.RLWE(P)
        n, K = P.n, (r.K if ring else 1)
        hp = (r.ring._h, P._h) if ring else (P._h,)
        pre = "lolhip_chall_ring_" if ring else "lolhip_chall_"
        one = "lolhip_rlwe_ring_" if ring else "lolhip_rlwe_"
        for ell in (3, 100):
            B = I * ell
            for kind, kname in ((0, "disc"), (2, "rlwr")):
                cfg = f"m={m} n={n} q={q} route={'ring' if ring else 'plan'} kind={kname} I={I} L={ell}"
                bound = lol_amd.RLWE.errorBound(m, svar, kind="disc") if kind == 0 else 0
                s, a, b = i64(I, n), i64(B, n), i64(B, n)
                fails, worst = torch.empty((I,), dtype=torch.int32, device="cuda"), i64(I)
                work = i64(max(getattr(L, pre + "work_len")(*hp, kind, I, ell), 2))
                g_gen = lambda: ok(getattr(L, pre + "generate_batch")(*hp, st, kind, p, svar, key, 0, 0, I, ell, ptr(s), ptr(a),
                                                                      ptr(b), ptr(work)))

                def g_ver():
                    ok(getattr(L, pre + "verify_batch")(*hp, st, kind, p, bound, 0.0, I, ell, ptr(s), ptr(a), ptr(b), ptr(fails),
                                                        ptr(worst), ptr(work)))
                    return fails.cpu()

                # the single-secret calls: per-instance slabs of the same arrays
                s1, a1, b1 = i64(I, n), i64(B, n), i64(B, n)
                shat = i64(I, n, K)
                nm, mm = i64(B), torch.empty((B,), dtype=torch.int32, device="cuda")
                w1 = i64(max(getattr(L, one + "work_len")(*hp, kind, ell), 2))
                row = lambda t, i, per: t.data_ptr() + 8 * i * per * n
                to_dec = ((L.lolhip_linv_batch,) if ring else (L.lolhip_crtinv_batch, L.lolhip_linv_batch))
                to_in = ((L.lolhip_l_batch,) if ring else (L.lolhip_l_batch, L.lolhip_crt_batch))

                def s_gen():
                    for i in range(I):
                        if ring:
                            ok(L.lolhip_rlwe_ring_secret(*hp, st, key, i, row(s1, i, 1), row(shat, i, K)))
                            sec = row(shat, i, K)
                        else:
                            ok(L.lolhip_rlwe_secret(*hp, st, key, i, row(s1, i, 1)))
                            sec = row(s1, i, 1)
                        ok(getattr(L, one + "sample_batch")(*hp, st, kind, p, sec, svar, key, i * ell, row(a1, i, ell),
                                                            row(b1, i, ell), ptr(w1), ell))
                    for f in to_dec:
                        ok(f(P._h, st, ptr(s1), I)); ok(f(P._h, st, ptr(a1), B))
                        if kind == 0:
                            ok(f(P._h, st, ptr(b1), B))

                sc, ac, bc = i64(I, n), i64(B, n), i64(B, n)

                def s_ver():
                    sc.copy_(s1); ac.copy_(a1); bc.copy_(b1)
                    for f in to_in:
                        ok(f(P._h, st, ptr(sc), I)); ok(f(P._h, st, ptr(ac), B))
                        if kind == 0:
                            ok(f(P._h, st, ptr(bc), B))
                    for i in range(I):
                        sec = row(sc, i, 1)
                        if ring:
                            ok(L.lolhip_ringmul_prepare(r.ring._h, st, row(shat, i, K), sec, None, 1))
                            sec = row(shat, i, K)
                        if kind == 0:
                            ok(getattr(L, one + "error_batch")(*hp, st, 0, row(ac, i, ell), row(bc, i, ell), sec, None,
                                                               nm.data_ptr() + 8 * i * ell, ptr(w1), ell))
                        else:
                            chk = L.lolhip_rlwr_ring_check_batch if ring else L.lolhip_rlwr_check_batch
                            ok(chk(*hp, p, st, row(ac, i, ell), row(bc, i, ell), sec, mm.data_ptr() + 4 * i * ell, ptr(w1), ell))
                    return (nm if kind == 0 else mm).cpu()

                g_gen(); s_gen()
                torch.cuda.synchronize()
                assert torch.equal(s, s1) and torch.equal(a, a1) and torch.equal(b, b1), cfg
                f_g, v_s = g_ver(), s_ver()
                assert not f_g.any() and ((v_s < bound).all() if kind == 0 else not v_s.any()), cfg
                rounds = lambda fn: [timeit(fn) for _ in range(5)]
                for what, gfn, sfn in (("generate", g_gen, s_gen), ("verify", g_ver, s_ver)):
                    tg = rep(f"chall_{what}(grouped)", cfg, rounds(gfn))
                    ts = rep(f"chall_{what}(32 single-secret calls)", cfg, rounds(sfn))
                    rep(f"chall_{what} speedup", cfg, [ts / tg])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    with open(os.path.join(root, "profiles", "challenge_bench.jsonl"), "w") as f:
        f.write("\n".join(json.dumps(d) for d in lines) + "\n")


def gadget_correct_leg(gen):
    """Gadget error correction (lolhip_gadget_correct_batch, decoding basis) at config 5's shape (m = 2048, q = (1017857,
    1032193), B = 8192) with base 256 and over one 61-bit modulus (q = 2^60 + 147457, m = 2^14, B = 64) with base 2: with
    and without the error polynomials, beside lolhip_gadget_encode_batch and lolhip_decompose_batch at the same shape and
    lolhip_copy_slab on a slab of the input's size, all in the same process.  alg_bytes = (L T + T + L) 8 per row (L T + T
    without errors); frac_of_copy = alg_GBps over the copy's.  Median of five rounds of ten calls.
    Also written to profiles/gadget_correct_pipelines.jsonl."""
    import statistics
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()
    lines = []
    rounds = lambda fn: [timeit(fn) for _ in range(5)]

    def rep(name, cfg, ts, items, alg_bytes, copy_gbps=None, note=None):
        ms = statistics.median(ts)
        d = {"op": name, "config": cfg, "ms": round(ms, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
             "items_per_s": round(items / ms * 1e3, 1), "alg_bytes": alg_bytes, "alg_GBps": round(alg_bytes / ms / 1e6, 1)}
        if copy_gbps:
            d["frac_of_copy"] = round(alg_bytes / ms / 1e6 / copy_gbps, 4)
        if note:
            d["note"] = note
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        return alg_bytes / ms / 1e6

    for pps, qs, B, base in (([(2, 11)], [1017857, 1032193], 8192, 256), ([(2, 14)], [2 ** 60 + 147457], 64, 2)):
        P = lol_amd.Plan(pps, qs)
        n, T, Ld = P.n, P.T, P.decomposeLen(base)
        rows = B * n
        cfg = f"m={P.m} T={T} q={qs} base={base} L={Ld} B={B}"
        s = rnd(gen, qs, B, n)
        cap = min(min(qs) // (2 * (base + 1)), (base ** (Ld // T - 1) - 1) // 2) - 1
        e = torch.randint(-cap, cap + 1, (Ld, B, n), dtype=torch.int64, device="cuda", generator=gen)
        xs = torch.empty((Ld, B, n, T), dtype=torch.int64, device="cuda")
        u, es = torch.empty_like(s), torch.empty_like(e)
        dst = torch.empty_like(xs)
        copy = rep("  copy_slab", f"{xs.numel() * 8 >> 20} MiB read + written",
                   rounds(lambda: L.lolhip_copy_slab(st, ptr(dst), ptr(xs), xs.numel() * 8, 0)), B, 2 * xs.numel() * 8,
                   note="lolhip_copy_slab, the HBM yardstick")
        del dst
        rep("gadget_encode", cfg, rounds(lambda: L.lolhip_gadget_encode_batch(P._h, st, ptr(s), base, ptr(e), ptr(xs), B)),
            B, (T + Ld + Ld * T) * rows * 8, copy)
        rep("gadget_correct", cfg, rounds(lambda: L.lolhip_gadget_correct_batch(P._h, st, ptr(xs), base, 0, ptr(u), ptr(es), None, B)),
            B, (Ld * T + T + Ld) * rows * 8, copy, note="u and the L error polynomials")
        torch.cuda.synchronize()
        assert torch.equal(u, s) and torch.equal(es, e), "gadget_correct did not recover (s, e)"
        rep("gadget_correct(es=NULL)", cfg, rounds(lambda: L.lolhip_gadget_correct_batch(P._h, st, ptr(xs), base, 0, ptr(u), None, None, B)),
            B, (Ld * T + T) * rows * 8, copy, note="u alone: one sweep")
        rep("  decompose", cfg, rounds(lambda: L.lolhip_decompose_batch(P._h, st, ptr(s), base, ptr(xs), B)),
            B, (T + Ld * T) * rows * 8, copy, note="k_decompose at the same shape, the mirror pass")
        del s, e, xs, u, es
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    with open(os.path.join(root, "profiles", "gadget_correct_pipelines.jsonl"), "w") as f:
        f.write("\n".join(lines) + "\n")


def eltops_leg(gen):
    """L and divGPow over int64 and float64 slabs (lolhip_elt_op_batch, T = 1) at the tunnelling index m = 128 * 7 * 13
    (n = 4608) and at m = 3 * 2^13 (n = 8192), batches of at least 1 GiB, on the route the library picks (LDS-resident
    items) and, for L over int64, on the forced global route (one pass per odd prime); beside lolhip_copy_slab on a slab
    of the same size (`hbm_copy`) and lolhip_l_batch (Z_q, one 31-bit modulus) at the same index and batch, all in the
    same process.  alg_bytes = 2 x slab; frac_of_copy = alg_GBps over the copy's.  The ops work in place, so the operand
    changes from call to call (the int64 slab of divGPow is indivisible after the first: the flags say 0 and the
    numerators are stored, the same traffic).  Median of five rounds of ten calls.
    Also written to profiles/eltops_bench.jsonl."""
    import statistics
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    lines = []
    rounds = lambda fn: [timeit(fn) for _ in range(5)]

    def rep(name, cfg, ts, items, alg_bytes, copy_gbps=None, note=None):
        ms = statistics.median(ts)
        d = {"op": name, "config": cfg, "ms": round(ms, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
             "items_per_s": round(items / ms * 1e3, 1), "alg_bytes": alg_bytes, "alg_GBps": round(alg_bytes / ms / 1e6, 1)}
        if copy_gbps:
            d["frac_of_copy"] = round(alg_bytes / ms / 1e6 / copy_gbps, 4)
        if note:
            d["note"] = note
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        return alg_bytes / ms / 1e6

    OP_L, OP_DIVGPOW, I64, F64 = 4, 8, 0, 1
    q31 = 2 ** 31 - 1
    for m in (128 * 7 * 13, 3 * 2 ** 13):
        P = lol_amd.Plan(lol_amd.factor_pps(m), [q31])
        n = P.n
        B = -(-2 ** 30 // (n * 8))
        slab = B * n * 8
        cfg = f"m={m} n={n} T=1 B={B} ({slab >> 20} MiB)"
        yi = torch.randint(-2 ** 62, 2 ** 62, (B, n, 1), dtype=torch.int64, device="cuda", generator=gen)
        yf = torch.randn((B, n, 1), dtype=torch.float64, device="cuda", generator=gen)
        ok = torch.empty((B,), dtype=torch.int32, device="cuda")
        dst = torch.empty_like(yi)
        copy = rep("  hbm_copy", cfg, rounds(lambda: L.lolhip_copy_slab(st, dst.data_ptr(), yi.data_ptr(), slab, 0)), B, 2 * slab,
                   note="lolhip_copy_slab, the HBM yardstick")
        del dst
        for name, op in (("L", OP_L), ("divGPow", OP_DIVGPOW)):
            for ename, elt, y in (("i64", I64, yi), ("f64", F64, yf)):
                call = lambda: L.lolhip_elt_op_batch(P._h, st, op, elt, 1, y.data_ptr(), ok.data_ptr(), B)
                assert call() == 0
                rep(f"elt_{name}_{ename}", cfg, rounds(call), B, 2 * slab, copy, note="on-chip route, one launch")
        lol_amd.debug_set("ELT_GLOBAL", True)
        try:
            for name, op in (("L", OP_L), ("divGPow", OP_DIVGPOW)):
                call = lambda: L.lolhip_elt_op_batch(P._h, st, op, I64, 1, yi.data_ptr(), ok.data_ptr(), B)
                assert call() == 0
                rep(f"elt_{name}_i64(global)", cfg, rounds(call), B, 2 * slab, copy, note="forced global route: one pass per odd prime"
                    + (", then the flag and division passes" if op == OP_DIVGPOW else ""))
        finally:
            lol_amd.debug_set("ELT_GLOBAL", False)
        yq = torch.randint(0, q31, (B, n, 1), dtype=torch.int64, device="cuda", generator=gen)
        call = lambda: L.lolhip_l_batch(P._h, st, yq.data_ptr(), B)
        assert call() == 0
        rep("  l_batch(Zq)", cfg + f" q={q31}", rounds(call), B, 2 * slab, copy, note="lolhip_l_batch over Z_q, one 31-bit modulus")
        torch.cuda.synchronize()
        del yi, yf, yq, ok
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    with open(os.path.join(root, "profiles", "eltops_bench.jsonl"), "w") as f:
        f.write("\n".join(lines) + "\n")


def lprf_leg(gen):
    """The key-homomorphic lattice PRF (lolhip_lprf_batch): the route the host rule picks (the matrix cores from K = 56 on:
    `route` says which) against the VALU route (debug switch LPRF_VALU) in the same process, alternately, three rounds each (median; min and max beside it).  Shapes: n = 256,
    q = 12289, base 2 (ell = 14, K = 3584), p = 64, a balanced 10-leaf tree, all of B = 1024 inputs, 1 and 16 keys; the same
    at n = 64, 16, 8 and 4 (K = 896 ... 56: where the routes cross); the reference's toy shapes (Zq 8 -> Zq 2, n = 3, 5 leaves, three trees;
    Zq 257 -> Zq 32, n = 3, 10 leaves); a 62-bit modulus (W = 8 limbs) at K = 62 and 248.  macs = the multiply-adds of the node products and of s A_l as the host plans
    them; the matrix route runs W limb products per multiply-add and is rated against the i8 MFMA peak (2 x the 2.5 PF
    BF16 peak = 2.5e15 multiply-adds/s), the VALU route against 256 CUs x 64 lanes x 2.4 GHz / 3 (a 64 x 64 -> 64
    product is at least three 32-bit multiplier instructions).  Also written to profiles/lprf_bench.jsonl."""
    import statistics
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import khprf_cases as kc
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    lines = []
    MFMA_PEAK, VALU_PEAK = 2.5e15, 256 * 64 * 2.4e9 / 3

    def macs(tree, n, K, nkeys, B):
        nodes = kc.parse(tree)
        tot = sum(kc.view(v, 0, B)[0] * n * K * K for i, v in enumerate(nodes) if i and not v.leaf)
        return tot + kc.view(nodes[nodes[0].l], 0, B)[0] * nkeys * n * K + B * nkeys * K * K

    def limbs(q):
        W = 1
        while q - 1 > 127 * ((256 ** W - 1) // 255):
            W += 1
        return W

    shapes = [(12289, 64, 2, n, lol_amd.balanced_tree(10), nk, "balanced10") for n in (256, 64, 16, 8, 4) for nk in (1, 16)]
    shapes += [(8, 2, 2, 3, t(5), 1, nm) for t, nm in ((lol_amd.left_spine_tree, "left5"), (lol_amd.balanced_tree, "balanced5"),
                                                      (lol_amd.right_spine_tree, "right5"))]
    shapes += [(257, 32, 2, 3, lol_amd.balanced_tree(10), 1, "balanced10")]
    shapes += [(2 ** 62 - 57, 2, 2, n, lol_amd.balanced_tree(10), 1, "balanced10") for n in (1, 4)]      # W = 8, 128-bit VALU sums
    for q, p, base, n, tree, nkeys, tname in shapes:
        ell = len(np.base_repr(q, base))
        K, B = n * ell, 1 << tree[0]
        a = [torch.randint(0, q, (n, K), dtype=torch.int64, generator=gen, device="cuda").cpu().numpy() for _ in range(2)]
        f = lol_amd.LatticePRF(q, base, tree, a[0], a[1])
        s = torch.randint(0, q, (nkeys, n), dtype=torch.int64, device="cuda", generator=gen)
        out = torch.empty((nkeys, B, K), dtype=torch.int64, device="cuda")
        work = torch.empty((max(f.workLen(nkeys, 0, B), 1),), dtype=torch.int64, device="cuda")
        call = lambda: L.lolhip_lprf_batch(f._h, st, s.data_ptr(), nkeys, p, 0, B, out.data_ptr(), work.data_ptr())
        assert call() == 0
        it = 3 if n >= 64 else 10
        m, W = macs(tree, n, K, nkeys, B), limbs(q)
        mfma = K >= 56                                      # the host rule (every shape here passes the certificate)
        ts = {"default": [], "valu": []}
        for _ in range(3):
            for route in ("default", "valu"):
                lol_amd.debug_set("LPRF_VALU", route == "valu")
                try:
                    ts[route].append(timeit(call, iters=it, warm=1))
                finally:
                    lol_amd.debug_set("LPRF_VALU", False)
        cfg = f"q={q} p={p} base={base} n={n} ell={ell} K={K} tree={tname} B={B} nkeys={nkeys}"
        for route in ("default", "valu"):
            ms = statistics.median(ts[route])
            on_mfma = mfma and route == "default"
            rate = m * (W if on_mfma else 1) / ms * 1e3
            d = {"op": f"lprf_prf({route})", "route": "mfma" if on_mfma else "valu", "config": cfg, "ms": round(ms, 4), "ms_min": round(min(ts[route]), 4),
                 "ms_max": round(max(ts[route]), 4), "items_per_s": round(nkeys * B / ms * 1e3, 1), "macs": m,
                 "W": W if on_mfma else 0, "mac_per_s": float(f"{rate:.4g}"),
                 "frac_of_peak": round(rate / (MFMA_PEAK if on_mfma else VALU_PEAK), 5),
                 "valu_over_default": round(statistics.median(ts["valu"]) / statistics.median(ts["default"]), 3)}
            lines.append(json.dumps(d))
            print(lines[-1], flush=True)
        torch.cuda.synchronize()
        del f, out, work
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    with open(os.path.join(root, "profiles", "lprf_bench.jsonl"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


def ctmul_leg(gen):
    """The ciphertext product of any degree (lolhip_ct_mul_batch) at the shape of bench.py's c3_ctmul_pow leg (m = 2^15,
    four ~59-bit moduli, B = 256), against entries whose device code is older than it, in one process:
      (a) linear x linear, CRT -> CRT: against lolhip_ctmul_crt_batch (without a factor the entry launches the same
          kernel, k_ctmul; `_msd`: with the MSD x MSD factor it launches k_ct_mul<2, 2>);
      (b) linear x linear, powerful -> powerful, MSD x MSD: against the composition ctLinComb (toLSD), 4 crt, ctMulCRT,
          3 crtInv (in place on its second operand, as bench.py's leg), and against the same composition with a copy of
          that operand in front (`_keep`): the new entry only reads its operands;
      (c) 3 x 3 components and the square of a quadratic ciphertext, CRT -> CRT: against lolhip_copy_slab moving the same
          number of bytes.
    Every round times the baseline twice (base_a, base_b) and the new entry once, each over a window of about a
    quarter of a second of calls, the order alternating from round to round; a row holds the medians over the rounds, and `spread_ms` = |median base_a - median base_b| is what two runs of
    the baseline alone differ by.  `within_spread`: new <= min(base_a, base_b) + spread.
    Also written to profiles/ctmul_bench.jsonl."""
    import ctypes as C
    import statistics
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()
    lines = []
    m, T, B, p, ROUNDS = 2 ** 15, 4, 256, 5, 6
    qs = good_qs(m, 2 ** 59, T)
    P = lol_amd.Plan([(2, 15)], qs)
    slab = B * P.n * P.T * 8
    cfg = f"m=2^15 T=4 59-bit B={B} ({slab >> 20} MiB per component)"

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def window(fn, iters):
        """ms per call over one window of `iters` calls between two events"""
        s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s_.record()
        for _ in range(iters):
            fn()
        e_.record()
        torch.cuda.synchronize()
        return s_.elapsed_time(e_) / iters

    def versus(name, new, base, alg_bytes, new_note, base_note):
        assert new() == 0
        base()
        # windows of about a quarter of a second each (shorter ones measure the clock ramp), after as much warm-up
        iters = max(10, int(250.0 / max(window(new, 20), window(base, 20))))
        window(new, iters), window(base, iters)
        ts = {"new": [], "base_a": [], "base_b": []}
        for r in range(ROUNDS):
            order = ("base_a", "new", "base_b") if r % 2 == 0 else ("new", "base_b", "base_a")
            for which in order:
                ts[which].append(window(new if which == "new" else base, iters))
        med = {k: statistics.median(v) for k, v in ts.items()}
        spread = abs(med["base_a"] - med["base_b"])
        best = min(med["base_a"], med["base_b"])
        for which, note in (("new", new_note), ("base_a", base_note), ("base_b", base_note)):
            d = {"op": f"{name}:{which}", "config": cfg, "ms": round(med[which], 4), "ms_min": round(min(ts[which]), 4),
                 "ms_max": round(max(ts[which]), 4), "calls_per_window": iters, "alg_bytes": alg_bytes,
                 "alg_GBps": round(alg_bytes / med[which] / 1e6, 1), "note": note}
            if which == "new":
                d.update(spread_ms=round(spread, 4), ratio_to_base=round(med["new"] / best, 4),
                         within_spread=bool(med["new"] <= best + spread))
            emit(d)

    a, b = torch.stack([rnd(gen, qs, B, P.n) for _ in range(2)]), torch.stack([rnd(gen, qs, B, P.n) for _ in range(2)])
    out = torch.empty((3, B, P.n, P.T), dtype=torch.int64, device="cuda")
    # (a)
    versus("ctmul_2x2_crt", lambda: L.lolhip_ct_mul_batch(P._h, st, ptr(a), 2, ptr(b), 2, 1, None, ptr(out), 1, None, B),
           lambda: L.lolhip_ctmul_crt_batch(P._h, st, ptr(a[0]), ptr(a[1]), ptr(b[0]), ptr(b[1]), ptr(out[0]), ptr(out[1]),
                                            ptr(out[2]), B),
           7 * slab, "lolhip_ct_mul_batch, CRT -> CRT, no factor: routed to k_ctmul", "lolhip_ctmul_crt_batch")
    al, e_, k_, l_ = (C.c_int64 * T)(), C.c_int(0), C.c_int64(0), C.c_int64(0)
    assert L.lolhip_ct_mul_rule(P._h, p, 1, 0, 1, 1, 0, 1, al, C.byref(e_), C.byref(k_), C.byref(l_)) == 0
    versus("ctmul_2x2_crt_msd", lambda: L.lolhip_ct_mul_batch(P._h, st, ptr(a), 2, ptr(b), 2, 1, al, ptr(out), 1, None, B),
           lambda: L.lolhip_ctmul_crt_batch(P._h, st, ptr(a[0]), ptr(a[1]), ptr(b[0]), ptr(b[1]), ptr(out[0]), ptr(out[1]),
                                            ptr(out[2]), B),
           7 * slab, "lolhip_ct_mul_batch, CRT -> CRT, MSD x MSD (alpha = p mod q_t): k_ct_mul<2, 2>",
           "lolhip_ctmul_crt_batch (no factor: not the same result, the same traffic)")
    # (b)
    wl = L.lolhip_ct_mul_work_len(P._h, 2, 2, 0, 0, B)
    work = torch.empty((wl,), dtype=torch.int64, device="cuda")
    tmp = torch.empty_like(a)
    zq, _ = P.encodeScales(p, False)
    zq = (C.c_int64 * T)(*zq)

    def composed():
        L.lolhip_ct_lincomb_batch(P._h, st, ptr(a), 2, zq, None, 0, None, ptr(tmp), B)        # toLSD of the first operand
        for x in (tmp[0], tmp[1], b[0], b[1]):
            L.lolhip_crt_batch(P._h, st, ptr(x), B)
        L.lolhip_ctmul_crt_batch(P._h, st, ptr(tmp[0]), ptr(tmp[1]), ptr(b[0]), ptr(b[1]), ptr(out[0]), ptr(out[1]), ptr(out[2]), B)
        for x in out:
            L.lolhip_crtinv_batch(P._h, st, ptr(x), B)

    versus("ctmul_2x2_pow_msd", lambda: L.lolhip_ct_mul_batch(P._h, st, ptr(a), 2, ptr(b), 2, 0, al, ptr(out), 0, ptr(work), B),
           composed, 7 * slab, "lolhip_ct_mul_batch, powerful -> powerful, MSD x MSD: 2 copies, crt over 4 B, product, crtInv over 3 B",
           "ctLinComb (toLSD), 4 crt, ctMulCRT, 3 crtInv (9 launches), in place on its operands")
    tmpb = torch.empty_like(b)

    def composed_keep():
        """the same composition leaving its operands as it found them, as the new entry does: b is copied first"""
        L.lolhip_copy_slab(st, ptr(tmpb), ptr(b), 2 * slab, 0)
        L.lolhip_ct_lincomb_batch(P._h, st, ptr(a), 2, zq, None, 0, None, ptr(tmp), B)
        for x in (tmp[0], tmp[1], tmpb[0], tmpb[1]):
            L.lolhip_crt_batch(P._h, st, ptr(x), B)
        L.lolhip_ctmul_crt_batch(P._h, st, ptr(tmp[0]), ptr(tmp[1]), ptr(tmpb[0]), ptr(tmpb[1]), ptr(out[0]), ptr(out[1]), ptr(out[2]), B)
        for x in out:
            L.lolhip_crtinv_batch(P._h, st, ptr(x), B)

    versus("ctmul_2x2_pow_msd_keep", lambda: L.lolhip_ct_mul_batch(P._h, st, ptr(a), 2, ptr(b), 2, 0, al, ptr(out), 0, ptr(work), B),
           composed_keep, 7 * slab, "lolhip_ct_mul_batch, powerful -> powerful, MSD x MSD (the same call as above)",
           "copy of b, ctLinComb (toLSD), 4 crt, ctMulCRT, 3 crtInv (10 launches): the composition with its operands left intact")
    del work, tmp, tmpb, a, b, out
    # (c)
    a3, b3 = (torch.stack([rnd(gen, qs, B, P.n) for _ in range(3)]) for _ in range(2))
    out5 = torch.empty((5, B, P.n, P.T), dtype=torch.int64, device="cuda")
    src = torch.empty((11 * slab // 16,), dtype=torch.int64, device="cuda")
    dst = torch.empty_like(src)
    versus("ctmul_3x3_crt", lambda: L.lolhip_ct_mul_batch(P._h, st, ptr(a3), 3, ptr(b3), 3, 1, None, ptr(out5), 1, None, B),
           lambda: L.lolhip_copy_slab(st, ptr(dst), ptr(src), 11 * slab // 2, 0), 11 * slab,
           "lolhip_ct_mul_batch, 3 x 3 components, CRT -> CRT", "lolhip_copy_slab moving the same 11 slabs (5.5 read, 5.5 written)")
    versus("ctmul_square3_crt", lambda: L.lolhip_ct_mul_batch(P._h, st, ptr(a3), 3, ptr(a3), 3, 1, None, ptr(out5), 1, None, B),
           lambda: L.lolhip_copy_slab(st, ptr(dst), ptr(src), 8 * slab // 2, 0), 8 * slab,
           "lolhip_ct_mul_batch, the square of a quadratic ciphertext, CRT -> CRT", "lolhip_copy_slab moving the same 8 slabs (4 read, 4 written)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    with open(os.path.join(root, "profiles", "ctmul_bench.jsonl"), "w") as f:
        f.write("\n".join(lines) + "\n")


def gauss_dense_leg(gen):
    """The Gaussian map at a prime above 13 (k_gauss_dense, plans created with dense_gauss=True): gaussianDec at m = 179, 257,
    797 and 2^9 17 on a slab of about 2^22 doubles, and RLWE.instances Disc at m = 257.  Two yardsticks from the same run,
    at the index 13 2^k of nearest n: the register route (a default plan) and the dense route forced on that same index
    (debug switch GAUSS_DENSE, read when the plan is built).  Three rounds, the routes alternating, ten timed calls each
    after two warm-up calls; the median round, min and max beside it.  macs = B n sum (p - 1) over the odd primes, the
    multiply-adds of the map; rated against the FP64 vector peak of 78.6 TFLOP/s = 3.93e13 multiply-adds/s.  `tile` is the
    launcher's own line (LOLHIP_GAUSS_INFO).  Also written to profiles/gauss_dense_bench.jsonl."""
    import statistics
    import tempfile
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    FMA_PEAK = 78.6e12 / 2
    lines = []

    def plan(m, dense, forced=False):
        if forced:
            L.lolhip_debug_set(b"GAUSS_DENSE", 1)
        try:
            return lol_amd.Plan.for_index(m, [lol_amd.good_q(m, 2 ** 20)], dense_gauss=dense)
        finally:
            L.lolhip_debug_set(b"GAUSS_DENSE", 0)

    def tile_of(call):
        """the launcher's info line of one call (it goes to the C stderr)"""
        sys.stderr.flush()
        with tempfile.TemporaryFile() as f:
            keep = os.dup(2)
            os.environ["LOLHIP_GAUSS_INFO"] = "1"
            os.dup2(f.fileno(), 2)
            try:
                call()
                torch.cuda.synchronize()
            finally:
                os.dup2(keep, 2); os.close(keep)
                del os.environ["LOLHIP_GAUSS_INFO"]
            f.seek(0)
            got = [ln for ln in f.read().decode().splitlines() if ln.startswith("k_gauss")]
        return got[-1] if got else ""

    def rounds(cases):
        """cases: [(label, m, plan)] timed alternately; one JSON line each"""
        slabs, calls = {}, {}
        for label, m, P in cases:
            B = max(64, 2 ** 22 // P.n)
            src = torch.randn((B, P.n), dtype=torch.float64, device="cuda", generator=gen)
            y = src.clone()
            slabs[label] = (src, y, B)
            calls[label] = (lambda P=P, y=y, B=B: L.lolhip_gaussian_dec_batch(P._h, st, y.data_ptr(), B))
            assert calls[label]() == 0
        ms = {label: [] for label, _, _ in cases}
        for _ in range(3):
            for label, _, _ in cases:
                src, y, _ = slabs[label]
                y.copy_(src)                       # in place: start every round from the same slab
                ms[label].append(timeit(calls[label]))
        for label, m, P in cases:
            src, y, B = slabs[label]
            y.copy_(src)
            tile = tile_of(calls[label])
            macs = B * P.n * sum(p - 1 for p, _ in P.pps if p != 2)
            med = statistics.median(ms[label])
            d = {"op": "gaussianDec", "route": label, "config": f"m={m} n={P.n} B={B}", "ms": round(med, 4),
                 "ms_min": round(min(ms[label]), 4), "ms_max": round(max(ms[label]), 4), "macs": macs,
                 "gmacs_per_s": round(macs / med / 1e6, 1), "frac_of_fp64_peak": round(macs / med * 1e3 / FMA_PEAK, 4),
                 "alg_GBps": round(2 * B * P.n * 8 / med / 1e6, 1), "tile": tile}
            lines.append(d)
            print(json.dumps(d), flush=True)

    # (index with a prime above 13, the index 13 2^k of nearest n)
    for m, m13 in ((179, 13 * 2 ** 5), (257, 13 * 2 ** 6), (797, 13 * 2 ** 7), (2 ** 9 * 17, 13 * 2 ** 9)):
        rounds([("dense", m, plan(m, True)), ("register", m13, plan(m13, False)), ("forced-dense", m13, plan(m13, True, forced=True))])
    # whole Disc instances at m = 257: 32 secrets of 100 samples, as rlwe-challenges' lines ask
    m, I, Ls = 257, 32, 100
    r = lol_amd.RLWE(plan(m, True))
    key = bytes(range(32))
    ms = [timeit(lambda: r.instances("disc", I, Ls, svar=3.90625e-3, key=key, ctr_s=0, ctr=0), iters=5) for _ in range(3)]
    med = statistics.median(ms)
    d = {"op": "RLWE.instances", "route": "dense", "config": f"Disc m={m} q={r.plan.qs[0]} I={I} L={Ls}", "ms": round(med, 4),
         "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "items_per_s": round(I * Ls / med * 1e3, 1)}
    lines.append(d)
    print(json.dumps(d), flush=True)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gauss_dense_bench.jsonl")
    with open(out, "w") as f:
        f.write("".join(json.dumps(x) + "\n" for x in lines))


def cplx_dense_leg(gen):
    """crtC at a prime above 13 (k_cplx_dense, plans created with dense_cplx=True) on slabs of about 2^22 complex doubles:
    m = 179, 257, 797, 17^2, 2^9 17, 2^10 17, the short vectors 17 .. 97 and the long ones 331 .. 509 (12, 10 and 8 columns
    per tile) that decide where the matrix cores start and stop, each
    on the matrix route and on the vector-ALU route (debug switch CPLX_DENSE_VALU, read when the plan is built); the
    indices 13 2^k of nearest n on the register route (k_cplx, a default plan) and with the dense routes forced on them
    (CPLX_DENSE).  Three rounds, the routes alternating, ten timed calls each after two warm-up calls; the median round, min
    and max beside it.  macs = 4 B n sum d over the stages, the real multiply-adds; rated against the FP64 peak of
    78.6 TFLOP/s = 3.93e13 multiply-adds/s (vector and matrix alike on this part).  `tile` is the launcher's own line
    (LOLHIP_CPLX_INFO).  Then the issue rate of v_mfma_f64_16x16x4_f64 from tools/mfma_f64_rate.hip, built on first use.
    Written to profiles/cplx_dense_bench.jsonl."""
    import statistics
    import subprocess
    import tempfile
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    FMA_PEAK = 78.6e12 / 2
    lines = []

    def plan(m, dense, forced=False, valu=False):
        L.lolhip_debug_set(b"CPLX_DENSE", int(forced))
        L.lolhip_debug_set(b"CPLX_DENSE_VALU", int(valu))
        try:
            return lol_amd.Plan.for_index(m, [12289], dense_cplx=dense)
        finally:
            L.lolhip_debug_set(b"CPLX_DENSE", 0)
            L.lolhip_debug_set(b"CPLX_DENSE_VALU", 0)

    def tile_of(call):
        sys.stderr.flush()
        with tempfile.TemporaryFile() as f:
            keep = os.dup(2)
            os.environ["LOLHIP_CPLX_INFO"] = "1"
            os.dup2(f.fileno(), 2)
            try:
                call()
                torch.cuda.synchronize()
            finally:
                os.dup2(keep, 2); os.close(keep)
                del os.environ["LOLHIP_CPLX_INFO"]
            f.seek(0)
            got = [ln for ln in f.read().decode().splitlines() if ln.startswith("k_cplx")]
        return got[-1] if got else ""

    def rounds(cases):
        slabs, calls = {}, {}
        for label, m, P in cases:
            B = max(64, 2 ** 22 // P.n)
            src = torch.randn((B, P.n, 2), dtype=torch.float64, device="cuda", generator=gen)
            y = src.clone()
            slabs[label] = (src, y, B)
            calls[label] = (lambda P=P, y=y, B=B: L.lolhip_crtc_batch(P._h, st, y.data_ptr(), B))
            assert calls[label]() == 0
        ms = {label: [] for label, _, _ in cases}
        for _ in range(3):
            for label, _, _ in cases:
                src, y, _ = slabs[label]
                y.copy_(src)
                ms[label].append(timeit(calls[label]))
        for label, m, P in cases:
            src, y, B = slabs[label]
            y.copy_(src)
            tile = tile_of(calls[label])
            prog = P.cplxProgram()
            sum_d = int(sum(int(r[2]) for r in prog if int(r[0]) in (1, 2, 3)))
            macs = 4 * B * P.n * sum_d
            med = statistics.median(ms[label])
            d = {"op": "crtC", "route": label, "config": f"m={m} n={P.n} B={B}", "ms": round(med, 4),
                 "ms_min": round(min(ms[label]), 4), "ms_max": round(max(ms[label]), 4), "sum_d": sum_d, "macs": macs,
                 "gmacs_per_s": round(macs / med / 1e6, 1), "frac_of_fp64_peak": round(macs / med * 1e3 / FMA_PEAK, 4),
                 "alg_GBps": round(2 * B * P.n * 16 / med / 1e6, 1), "tile": tile}
            lines.append(d)
            print(json.dumps(d), flush=True)

    # (CPLX_DENSE lifts the route rule's conditions, so "dense-mfma" is the matrix route wherever the rule would put the stage)
    for m in (17, 19, 23, 29, 37, 53, 97, 179, 257, 331, 397, 509, 797, 17 ** 2, 2 ** 9 * 17, 2 ** 10 * 17):
        rounds([("dense-mfma", m, plan(m, True, forced=True)), ("dense-valu", m, plan(m, True, valu=True))])
    for m13 in (13 * 2 ** 5, 13 * 2 ** 6, 13 * 2 ** 7, 13 * 2 ** 9):
        rounds([("register", m13, plan(m13, False)), ("forced-mfma", m13, plan(m13, True, forced=True)),
                ("forced-valu", m13, plan(m13, True, forced=True, valu=True))])
    # the issue rate of the f64 MFMA itself: a program of its own, in a process of its own
    here = os.path.dirname(os.path.abspath(__file__))
    exe = os.path.join(here, "_build", "mfma_f64_rate")
    if not os.path.exists(exe):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-o", exe, os.path.join(here, "mfma_f64_rate.hip")])
    for ln in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines():
        if ln.startswith("{"):
            lines.append(json.loads(ln))
            print(ln, flush=True)
    out = os.path.join(os.path.dirname(here), "profiles", "cplx_dense_bench.jsonl")
    with open(out, "w") as f:
        f.write("".join(json.dumps(x) + "\n" for x in lines))


def zq_dense_leg(gen):
    """The dense Z_q stages at a prime above 13 (zqdense.hip, plans created with dense_zq=True): crt, crtInv and the
    poly-mul on slabs of about 2^22 words at m = 179, 257 and 797 (a list modulus with a CRT basis each, and the NTT prime
    RingMul picks for a list modulus without one), at 2^9 17, at the short vectors 17 .. 97 that decide where the matrix
    cores start, and at the index 13 2^k of nearest n for scale.  Per case four routes of the same parameters alternate
    in one process: the opted-in plan as it routes itself (`dense`), the same plan on the vector ALU (switch
    ZQ_DENSE_VALU), on the matrix cores whatever the vector length (ZQ_DENSE_MFMA, where the moduli fit), and a default
    plan (`scalar`: the launches of a plan without the route); where the poly-mul takes one launch, also the same plan
    with the poly-mul composed of its dense transforms (`composed`, switch POLYMUL_UNFUSED).  Three rounds, ten timed calls each after two warm-up
    calls; the median round with min and max beside it.  macs = B n T sum d over the dense stages.  `tile` is the launcher's
    own line (LOLHIP_ZQ_DENSE_INFO).  Then RLWE.instances Disc at m = 257, q = 1056271, 32 x 100, dense against default.
    Also written to profiles/zq_dense_bench.jsonl."""
    import statistics
    import tempfile
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    lines = []

    def tile_of(call):
        sys.stderr.flush()
        with tempfile.TemporaryFile() as f:
            keep = os.dup(2)
            os.environ["LOLHIP_ZQ_DENSE_INFO"] = "1"
            os.dup2(f.fileno(), 2)
            try:
                call()
                torch.cuda.synchronize()
            finally:
                os.dup2(keep, 2); os.close(keep)
                del os.environ["LOLHIP_ZQ_DENSE_INFO"]
            f.seek(0)
            got = [ln for ln in f.read().decode().splitlines() if ln.startswith("k_zq_dense")]
        return got[0] if got else ""

    def case(m, qs, note):
        pps = lol_amd.factor_pps(m)
        P, D = lol_amd.Plan(pps, qs, dense_zq=True), lol_amd.Plan(pps, qs)
        B = max(8, 2 ** 22 // (P.n * P.T))
        a, b = rnd(gen, qs, B, P.n), rnd(gen, qs, B, P.n)
        y, c = a.clone(), torch.empty_like(a)
        ops = {"crt": lambda Q: L.lolhip_crt_batch(Q._h, st, y.data_ptr(), B),
               "crtInv": lambda Q: L.lolhip_crtinv_batch(Q._h, st, y.data_ptr(), B),
               "polymul": lambda Q: L.lolhip_polymul_batch(Q._h, st, c.data_ptr(), a.data_ptr(), b.data_ptr(), B)}
        routes = [("dense", P, None), ("valu", P, b"ZQ_DENSE_VALU"), ("mfma", P, b"ZQ_DENSE_MFMA"), ("scalar", D, None)]
        one_launch = P.zqRoute(2) > 0        # then also the poly-mul composed of the plan's dense transforms (POLYMUL_UNFUSED)
        if P.zqRoute(0) == 0:
            routes = routes[-1:]
        else:
            L.lolhip_debug_set(b"ZQ_DENSE_MFMA", 1)
            can_mfma = P.zqRoute(0) == 2
            L.lolhip_debug_set(b"ZQ_DENSE_MFMA", 0)
            if not can_mfma:
                routes = [r for r in routes if r[0] != "mfma"]
        dsum = sum(int(s[2]) for s in P.program() if s[0] in (1, 2, 3) and s[1] > 13)
        for op, fn in ops.items():
            routes = [r for r in routes if r[0] != "composed"]
            if op == "polymul" and one_launch:
                routes = routes[:1] + [("composed", P, b"POLYMUL_UNFUSED")] + routes[1:]
            ms = {r[0]: [] for r in routes}
            tiles, which = {}, {}

            def run(label, Q, sw):
                if sw:
                    L.lolhip_debug_set(sw, 1)
                try:
                    which[label] = Q.zqRoute(0)
                    assert fn(Q) == 0
                    if label not in tiles:
                        tiles[label] = tile_of(lambda: fn(Q))
                    return timeit(lambda: fn(Q))
                finally:
                    if sw:
                        L.lolhip_debug_set(sw, 0)
            for _ in range(3):
                for label, Q, sw in routes:
                    y.copy_(a)
                    ms[label].append(run(label, Q, sw))
            for label, Q, sw in routes:
                med = statistics.median(ms[label])
                macs = B * P.n * P.T * dsum * (3 if op == "polymul" else 1)
                d = {"op": op, "route": label, "zq_route": which[label], "one_launch": bool(op == "polymul" and one_launch and label not in ("composed", "scalar")), "config": f"m={m} n={P.n} qs={qs} B={B}", "note": note,
                     "ms": round(med, 4), "ms_min": round(min(ms[label]), 4), "ms_max": round(max(ms[label]), 4),
                     "gmacs_per_s": round(macs / med / 1e6, 1), "alg_GBps": round(2 * B * P.n * P.T * 8 / med / 1e6, 1),
                     "tile": tiles[label]}
                lines.append(d)
                print(json.dumps(d), flush=True)

    ntt = lambda m, q: [int(v) for v in lol_amd.RingMul.moduli(lol_amd.factor_pps(m), [q])]
    case(179, [8382929], "list modulus, W = 3")
    case(179, ntt(179, 65536), "NTT primes of RingMul for q = 65536")
    case(257, [15802417], "list modulus, W = 3")
    case(257, ntt(257, 131072), "NTT primes of RingMul for q = 131072")
    case(797, [741587779], "list modulus, W = 4")
    case(797, [44633], "list modulus, W = 2")
    case(797, ntt(797, 65536), "NTT primes of RingMul for q = 65536")
    case(2 ** 9 * 17, [lol_amd.good_q(2 ** 9 * 17, 2 ** 20)], "split route, odd part d = 16 at stride 256")
    for m in (17, 31, 37, 43, 53, 61, 67, 97, 323):
        case(m, [lol_amd.good_q(m, 2 ** 20)], "short vectors: where the matrix cores start")
    for m13 in (13 * 2 ** 5, 13 * 2 ** 6, 13 * 2 ** 7):
        case(m13, [lol_amd.good_q(m13, 2 ** 20)], "scale: the vector interpreter at the nearest n")
    # whole Disc instances at m = 257: 32 secrets of 100 samples, as rlwe-challenges' lines ask
    m, q, I, Ls = 257, 1056271, 32, 100
    key = bytes(range(32))
    rs = {"dense": lol_amd.RLWE(lol_amd.Plan.for_index(m, [q], dense_gauss=True, dense_zq=True)),
          "scalar": lol_amd.RLWE(lol_amd.Plan.for_index(m, [q], dense_gauss=True))}
    ms = {k: [] for k in rs}
    for _ in range(3):
        for k, r in rs.items():
            ms[k].append(timeit(lambda: r.instances("disc", I, Ls, svar=3.90625e-3, key=key, ctr_s=0, ctr=0), iters=5))
    for k, r in rs.items():
        med = statistics.median(ms[k])
        d = {"op": "RLWE.instances", "route": k, "zq_route": r.plan.zqRoute(0), "config": f"Disc m={m} q={q} I={I} L={Ls}",
             "ms": round(med, 4), "ms_min": round(min(ms[k]), 4), "ms_max": round(max(ms[k]), 4),
             "items_per_s": round(I * Ls / med * 1e3, 1)}
        lines.append(d)
        print(json.dumps(d), flush=True)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "zq_dense_bench.jsonl")
    with open(out, "w") as f:
        f.write("".join(json.dumps(x) + "\n" for x in lines))


def zq_scan_leg(gen):
    """The scan route of the prime ops at a prime above 13 (zqscan.hip, plans created with scan_zq=True): L, divGPow and
    divGDec on slabs of about 2^22 words at m = 17, 67, 179, 257, 797 and 2176 (128 * 17: the column layout), each over a
    modulus below 2^32 and over a 61-bit one.  Per line three things alternate in one process: the opted-in plan
    (`scan`), a default plan of the same parameters (`scalar`: exactly the launches of a plan without the route) and
    lolhip_copy_slab of the same bytes (`copy`: the floor of a read-once / write-once kernel).  Three rounds, ten timed
    calls each after two warm-up calls, HIP events; the median round with min and max beside it.  `tile` is the
    launcher's own line (LOLHIP_ZQ_SCAN_INFO).  Then one whole Disc challenge of I = 32 instances of L = 3 samples,
    generate and verify, at m = 257 and m = 797: the plan lol_amd.challenges builds and the same plan without the bit.
    Also written to profiles/zq_scan_bench.jsonl."""
    import statistics
    import tempfile
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    lines = []

    def tile_of(call):
        sys.stderr.flush()
        with tempfile.TemporaryFile() as f:
            keep = os.dup(2)
            os.environ["LOLHIP_ZQ_SCAN_INFO"] = "1"
            os.dup2(f.fileno(), 2)
            try:
                call()
                torch.cuda.synchronize()
            finally:
                os.dup2(keep, 2); os.close(keep)
                del os.environ["LOLHIP_ZQ_SCAN_INFO"]
            f.seek(0)
            got = [ln for ln in f.read().decode().splitlines() if ln.startswith("k_zq_scan")]
        return got[0] if got else ""

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    def case(m, qs):
        pps = lol_amd.factor_pps(m)
        P, D = lol_amd.Plan(pps, qs, scan_zq=True), lol_amd.Plan(pps, qs)
        B = max(8, 2 ** 22 // (P.n * P.T))
        a = rnd(gen, qs, B, P.n)
        y = a.clone()
        nbytes = a.numel() * 8
        ops = {"L": (4, L.lolhip_l_batch), "divGPow": (8, L.lolhip_divgpow_batch), "divGDec": (9, L.lolhip_divgdec_batch)}
        for op, (code, entry) in ops.items():
            assert P.scanRoute(code) == 1 and D.scanRoute(code) == 0
            fns = {"scan": lambda: entry(P._h, st, y.data_ptr(), B), "scalar": lambda: entry(D._h, st, y.data_ptr(), B),
                   "copy": lambda: L.lolhip_copy_slab(st, y.data_ptr(), a.data_ptr(), nbytes, 0)}
            ms = {k: [] for k in fns}
            tile = tile_of(fns["scan"])
            assert tile and not tile_of(fns["scalar"])
            for _ in range(3):
                for label, fn in fns.items():
                    y.copy_(a)
                    assert fn() == 0
                    ms[label].append(timeit(fn))
            for label in fns:
                med = statistics.median(ms[label])
                emit({"op": op, "route": label, "config": f"m={m} n={P.n} qs={qs} B={B}", "word": 4 if max(qs) < 2 ** 32 else 8,
                      "ms": round(med, 4), "ms_min": round(min(ms[label]), 4), "ms_max": round(max(ms[label]), 4),
                      "alg_GBps": round(2 * nbytes / med / 1e6, 1), "tile": tile if label == "scan" else ""})

    for m in (17, 67, 179, 257, 797, 2176):
        case(m, [lol_amd.good_q(m, 2 ** 31)])
        case(m, [lol_amd.good_q(m, 2 ** 60)])
    # one whole Disc challenge, generate and verify, with and without the bit
    key, I, Ls = bytes(range(32)), 32, 3
    for m, q in ((257, 15802417), (797, 741587779)):
        svar = 1.0 / m
        mk = lambda scan: lol_amd.RLWE(lol_amd.Plan.for_index(m, [q], dense_gauss=True, dense_zq=True, scan_zq=scan))
        rs = {"scan": mk(True), "scalar": mk(False)}
        bound = lol_amd.RLWE.errorBound(m, svar, 2.0 ** -25, kind="disc")
        data = {k: r.instances("disc", I, Ls, svar=svar, key=key, ctr_s=0, ctr=0) for k, r in rs.items()}
        calls = {"chall_generate": lambda k: rs[k].instances("disc", I, Ls, svar=svar, key=key, ctr_s=0, ctr=0),
                 "chall_verify": lambda k: rs[k].validInstances("disc", *data[k], bound=bound)}
        for op, fn in calls.items():
            ms = {k: [] for k in rs}
            for _ in range(3):
                for k in rs:
                    ms[k].append(timeit(lambda: fn(k)))
            for k in rs:
                med = statistics.median(ms[k])
                emit({"op": op, "route": k, "config": f"Disc m={m} q={q} I={I} L={Ls}", "ms": round(med, 4),
                      "ms_min": round(min(ms[k]), 4), "ms_max": round(max(ms[k]), 4)})
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "zq_scan_bench.jsonl")
    with open(out, "w") as f:
        f.write("".join(json.dumps(x) + "\n" for x in lines))


def main():
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    if "--zq-scan" in sys.argv:          # the scan route of the prime ops leg alone
        zq_scan_leg(gen)
        return
    if "--zq-dense" in sys.argv:         # the dense Z_q stages leg alone
        zq_dense_leg(gen)
        return
    if "--cplx-dense" in sys.argv:       # the dense complex CRT leg alone
        cplx_dense_leg(gen)
        return
    if "--gauss-dense" in sys.argv:      # the dense Gaussian stage leg alone
        gauss_dense_leg(gen)
        return
    if "--challenge" in sys.argv:        # the whole-challenge leg alone
        challenge_leg(gen)
        return
    if "--lprf" in sys.argv:             # the key-homomorphic lattice PRF leg alone
        lprf_leg(gen)
        return
    if "--ctmul" in sys.argv:            # the ciphertext product of any degree leg alone
        ctmul_leg(gen)
        return
    if "--rlwe-ring" in sys.argv:        # the RLWE / RLWR instances over moduli without a CRT basis leg alone
        rlwe_ring_leg(gen)
        return
    if "--eltops" in sys.argv:           # the L / divG over Z and R leg alone
        eltops_leg(gen)
        return
    if "--gadget-correct" in sys.argv:   # the gadget error correction leg alone
        gadget_correct_leg(gen)
        return
    if "--ringmul" in sys.argv:          # the exact ring product leg alone
        ringmul_leg(gen)
        return
    if "--rlwe" in sys.argv:             # the RLWE verification / gSqNorm leg alone
        rlwe_leg(gen)
        return
    if "--ptround" in sys.argv:          # the homomorphic rounding leg alone
        ptround_leg(gen)
        return
    if "--modswitch" in sys.argv:        # the ciphertext modSwitch leg alone
        modswitch_leg(gen)
        return
    if "--tunnel-chain" in sys.argv:     # the multi-hop tunnelling leg alone
        tunnel_chain_leg(gen)
        return
    if "--public" in sys.argv:           # the public operations / ciphertext addition leg alone
        public_leg(gen)
        return
    if "--khprf-lifted" in sys.argv:     # the lifted key-homomorphic PRF leg alone
        khprf_lifted_leg(gen)
        return
    if "--decrypt" in sys.argv:          # the decrypt leg alone
        decrypt_leg(gen)
        return
    if "--encrypt" in sys.argv:          # the encrypt leg alone
        encrypt_leg(gen)
        return
    if "--kshint" in sys.argv:           # the key-switch / tunnel hint leg alone
        kshint_leg(gen)
        return
    if "--khprf" in sys.argv:            # the key-homomorphic PRF leg alone
        khprf_leg(gen)
        return
    L = lol_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    # ---- config 3: ciphertext product, m = 2^15, T = 4, ~59-bit moduli ------------------
    qs = good_qs(2 ** 15, 2 ** 59, 4)
    P = lol_amd.Plan([(2, 15)], qs)
    B = 256
    ops = [rnd(gen, qs, B, P.n) for _ in range(4)]
    outs = [torch.empty_like(ops[0]) for _ in range(3)]
    slab = B * P.n * P.T * 8
    ptr = lambda t: t.data_ptr()
    ms = timeit(lambda: L.lolhip_ctmul_crt_batch(P._h, st, *map(ptr, ops + outs), B))
    report("ctmul_crt", f"m=2^15 T=4 59-bit B={B}", ms, B, 7 * slab)
    # the same product op by op (what a Tensor-method-at-a-time backend does): 4 mul, 1 add, 3 mulGCRT
    def unfused():
        a, b_, c_, d_ = (o.clone() for o in (ops[0], ops[0], ops[1], ops[1]))
        P.mul(a, ops[2]); P.mul(b_, ops[3]); P.mul(c_, ops[2]); P.mul(d_, ops[3])
        b_ += c_
        P.mulGCRT(a); P.mulGCRT(b_); P.mulGCRT(d_)
    ms_u = timeit(unfused, iters=5)
    report("ctmul_crt_op_by_op", f"m=2^15 T=4 59-bit B={B}", ms_u, B, 7 * slab)
    del ops, outs
    # ---- config 5: key switch, m' = 2048, q = (1017857, 1032193), TrivGad; and at n = 8192 -----
    # (pps, moduli, batch): config 5's ring; the same at n = 8192; the reference's non-2-power key-switch benchmark
    # F64*F9*F25 with Zq (1008001 ** 1065601) (lol-apps Benchmarks/Default.hs:49)
    for pps5, qs5, B in (([(2, 11)], [1017857, 1032193], 8192), ([(2, 14)], good_qs(2 ** 14, 2 ** 20, 2), 1024),
                         ([(2, 6), (3, 2), (5, 2)], [1008001, 1065601], 2048),
                         ([(2, 6), (3, 2), (5, 2)], [1008001, 1065601], 8192)):      # the same with a digit slab beyond the Infinity Cache
        P = lol_amd.Plan(pps5, qs5)
        for base in (0, 256):
            Ld = P.decomposeLen(base)
            c2 = rnd(gen, qs5, B, P.n)
            add = torch.stack([rnd(gen, qs5, B, P.n) for _ in range(2)])
            hint = rnd(gen, qs5, Ld, 2, P.n)
            work = torch.empty((Ld, B, P.n, P.T), dtype=torch.int64, device="cuda")
            out = torch.empty_like(add)
            slab = B * P.n * P.T * 8
            ms = timeit(lambda: L.lolhip_keyswitch_batch(P._h, st, ptr(c2), base, ptr(hint), 2, ptr(add), ptr(out), ptr(work), B))
            report("keyswitch", f"m={P.m} T=2 q~2^20 base={base} L={Ld} B={B}", ms, B, 5 * slab)
            L.lolhip_debug_set(b"KEYSWITCH_UNFUSED", 1)
            ms = timeit(lambda: L.lolhip_keyswitch_batch(P._h, st, ptr(c2), base, ptr(hint), 2, ptr(add), ptr(out), ptr(work), B))
            L.lolhip_debug_set(b"KEYSWITCH_UNFUSED", 0)
            report("keyswitch_three_launches", f"m={P.m} T=2 q~2^20 base={base} L={Ld} B={B}", ms, B, 5 * slab)
            ms = timeit(lambda: L.lolhip_decompose_batch(P._h, st, ptr(c2), base, ptr(work), B))
            report("  decompose", f"L={Ld}", ms, B, (1 + Ld) * slab)
            ms = timeit(lambda: L.lolhip_crt_batch(P._h, st, ptr(work), Ld * B))
            ic = "digit slab %d MiB: re-read from the 256 MiB Infinity Cache when it fits (not an HBM rate)" % (Ld * slab >> 20) if Ld * slab <= (256 << 20) else None
            report("  crt(digits)", f"L={Ld}", ms, B * Ld, 2 * Ld * slab, note=ic)
            ms = timeit(lambda: L.lolhip_knapsack_batch(P._h, st, ptr(work), Ld, ptr(hint), 2, ptr(add), ptr(out), B))
            report("  knapsack", f"L={Ld} K=2", ms, B, (Ld + 4) * slab)
    # ---- rescale: drop the first of four 59-bit moduli at m = 2^15 --------------------------
    qs = good_qs(2 ** 15, 2 ** 59, 4)
    P = lol_amd.Plan([(2, 15)], qs)
    B = 256
    c = rnd(gen, qs, B, P.n)
    out = torch.empty((B, P.n, 3), dtype=torch.int64, device="cuda")
    ms = timeit(lambda: L.lolhip_rescale_drop_batch(P._h, st, ptr(c), ptr(out), B))
    report("rescale_drop", f"m=2^15 T=4->3 B={B}", ms, B, B * P.n * 7 * 8)

    streaming(gen)
    decrypt_leg(gen)
    encrypt_leg(gen)
    rlwe_leg(gen)


def streaming(gen):
    """the HBM-bound Tensor members of SURVEY 8(a) a6, a12-a15: mulRq, mulGCRT, twace*/embed* (config 5's ring pair)"""
    if "--no-streaming" in sys.argv:
        return
    q61 = lol_amd.good_q(2 ** 14, 2 ** 60)
    for cfg, pps, qs, B in (("m=2^14 T=1 61-bit", [(2, 14)], [q61], 4096), ("m=2^11 T=2 q~2^20", [(2, 11)], [1017857, 1032193], 32768)):
        P = lol_amd.Plan(pps, qs)
        a, b = rnd(gen, qs, B, P.n), rnd(gen, qs, B, P.n)
        slab = B * P.n * P.T * 8
        report("mulRq", f"{cfg} B={B}", timeit(lambda: P.mul(a, b)), B, 3 * slab)
        report("mulGCRT", f"{cfg} B={B}", timeit(lambda: P.mulGCRT(a)), B, 2 * slab)
    qs, B = [1017857, 1032193], 8192          # both are 1 mod 14336
    lo, hi = lol_amd.Plan([(2, 11)], qs), lol_amd.Plan([(2, 11), (7, 1)], qs)
    E = lol_amd.Ext(lo, hi)
    x_lo, x_hi = rnd(gen, qs, B, lo.n), rnd(gen, qs, B, hi.n)
    o_lo, o_hi = torch.empty_like(x_lo), torch.empty_like(x_hi)
    byts = B * (lo.n + hi.n) * 2 * 8
    # twacePowDec reads only phi(m) of the phi(m') coefficients (every 6th here, 16 bytes each: whole 64-byte sectors
    # are fetched): compulsory traffic = n coefficients in and out, NOT the (n + n') of the other members
    byts_twpd = B * 2 * lo.n * 2 * 8
    cfg = f"2048 -> 14336 T=2 B={B}"
    for name, fn, bb, note in (("embedPow", lambda: E.embedPow(x_lo, out=o_hi), byts, None), ("embedDec", lambda: E.embedDec(x_lo, out=o_hi), byts, None),
                               ("embedCRT", lambda: E.embedCRT(x_lo, out=o_hi), byts, None),
                               ("twacePowDec", lambda: E.twacePowDec(x_hi, out=o_lo), byts_twpd,
                                "2 n T 8 bytes per item; the gathered 16-byte pairs sit 96 bytes apart, so the sectors fetched are 4x the bytes used"),
                               ("twaceCRT", lambda: E.twaceCRT(x_hi, out=o_lo), byts, None)):
        report(name, cfg, timeit(fn), B, bb, note=note)


if __name__ == "__main__":
    main()
