"""What tests/test_ext_width.py relies on, checked without a GPU.

  routes            launch_gather's and launch_twace_crt's choices (kernels.hip) restated as functions of (n_in, n_out, T,
                    alignment, replicating), and the case table of the GPU module run through them: every route, chunk
                    width, chunks-per-coefficient count, split and tile count the table is there for is asserted, so
                    the coverage cannot rot when a shape is edited
  magic division    floor(c (floor(2^32 / cpt) + 1) / 2^32) = c div cpt for every chunk index a launch can form
  moduli / inputs   the helper's widths; the rows that reach the x = 0 branch of a negated embedDec entry
  oracle            the Python twace_crt against crt . twace_powdec . crtinv through the compiled CPU restatement, and the
                    embed / twace identities on the oracle alone, at the wide and mixed tuples
"""
import numpy as np
import pytest

from oracle import lolmath as lm

import test_ext_width as tw

GA_K, TC_K = 4, 2                     # chunks per thread of k_gather / k_gather_lds and of k_twace_crt
LDS_LIMIT = 64 * 1024                 # the largest source polynomial launch_gather stages in LDS
COEFFS_TILE = 512                     # outputs per workgroup of k_coeffs


def _ceil(a, b):
    return (a + b - 1) // b


def gather_route(n_in, n_out, T, aligned, replicating):
    """launch_gather: kernel, TW (components per access), cpt (chunks per coefficient), tiles of 256 GA_K chunks, whether
    the last one is partial, and for the LDS route split (workgroups per polynomial), cps (chunks each) and LDS bytes"""
    TW = 2 if T % 2 == 0 and aligned else 1
    cpt = T // TW
    chunks = n_out * cpt
    tile = 256 * GA_K
    src_bytes = n_in * T * 8
    r = dict(TW=TW, cpt=cpt, chunks=chunks, src_bytes=src_bytes)
    if replicating and src_bytes <= LDS_LIMIT and n_out >= 2 * n_in:
        cps = _ceil(4 * n_in * cpt, tile) * tile
        if cps > chunks:
            cps = _ceil(chunks, tile) * tile
        split = _ceil(chunks, cps)
        last = chunks - (split - 1) * cps                               # chunks of the last workgroup
        r.update(kernel="k_gather_lds", split=split, cps=cps, lds=src_bytes, tiles=(split - 1) * (cps // tile) + _ceil(last, tile),
                 partial=last % tile != 0)
    else:
        r.update(kernel="k_gather", split=1, cps=chunks, lds=0, tiles=_ceil(chunks, tile), partial=chunks % tile != 0)
    r["max_chunk"] = r["tiles"] * tile - 1 if r["kernel"] == "k_gather" else (r["split"] - 1) * r["cps"] + _ceil(
        chunks - (r["split"] - 1) * r["cps"], tile) * tile - 1         # the largest c a thread forms, padding included
    return r


def twace_crt_route(n_in, n_out, T, aligned):
    """launch_twace_crt (the tweak table is a fresh allocation: always aligned)"""
    TW = 2 if T % 2 == 0 and aligned else 1
    cpt = T // TW
    chunks = n_out * cpt
    tile = 256 * TC_K
    return dict(kernel="k_twace_crt", TW=TW, cpt=cpt, chunks=chunks, tiles=_ceil(chunks, tile), partial=chunks % tile != 0,
                rel=n_in // n_out, max_chunk=_ceil(chunks, tile) * tile - 1)


def _n(m):
    return lm.totient_pps(lm.factor_pps(m))


def _routes(cases, offsets_of):
    """every launch the GPU module makes for `cases`: (case, op, aligned, route)"""
    out = []
    for c in cases:
        m, m2, T, _ = c
        n, n2 = _n(m), _n(m2)
        for off_in, off_out in offsets_of(T):
            al = off_in % 2 == 0 and off_out % 2 == 0
            for op in ("embedPow", "embedDec"):
                out.append((c, op, al, gather_route(n, n2, T, al, False)))
            out.append((c, "embedCRT", al, gather_route(n, n2, T, al, True)))
            out.append((c, "twacePowDec", al, gather_route(n2, n, T, al, False)))
            out.append((c, "twaceCRT", al, twace_crt_route(n2, n, T, al)))
    return out


@pytest.fixture(scope="module")
def routes():
    return _routes(tw.CASES, tw._offsets)


def _pick(routes, op=None, shape=None, **want):
    return [(c, o, al, r) for c, o, al, r in routes if (op is None or o == op) and (shape is None or c[:2] == shape) and
            all(r.get(k) == v for k, v in want.items())]


def test_small_shapes_reach_every_chunk_layout_in_one_partial_tile(routes):
    small = [x for x in routes if x[0][:2] in tw.SMALL]
    assert {c[:2] for c, *_ in small} == set(tw.SMALL)
    for c, op, al, r in small:
        assert _n(c[0]) <= 6 and _n(c[1]) <= 24
        assert r["tiles"] == 1 and r["partial"], (c, op)
    for kernel, ops in (("k_gather", ("embedPow", "embedDec", "twacePowDec")), ("k_gather_lds", ("embedCRT",)),
                        ("k_twace_crt", ("twaceCRT",))):
        for shape in tw.SMALL:
            got = {(r["TW"], r["cpt"]) for c, op, al, r in small if op in ops and c[:2] == shape and r["kernel"] == kernel}
            assert {cpt for tw_, cpt in got if tw_ == 2} == {1, 2, 3, 4, 8}, (kernel, shape)       # T = 2, 4, 6, 8, 16
            assert {cpt for tw_, cpt in got if tw_ == 1} == {1, 2, 4, 5, 6, 7, 8, 16}, (kernel, shape)
    # both chunk widths for every even T, one for every odd T
    for T in tw.SMALL_T:
        assert {r["TW"] for c, op, al, r in small if c[2] == T} == ({1, 2} if T % 2 == 0 else {1})


def test_small_shapes_run_a_coeffs_tile_across_output_vectors():
    for m, m2 in tw.SMALL:
        for T in tw.SMALL_T:
            slab, total = tw.B_OPS * _n(m) * T, tw.B_OPS * _n(m2) * T         # one output vector; all of them
            assert total > slab and slab < COEFFS_TILE, (m, m2, T)           # tile 0 starts in vector 0 and runs past it


def test_rel_one_takes_the_plain_gather_for_embed_crt(routes):
    got = _pick(routes, op="embedCRT", shape=(8, 8))
    assert {c[2] for c, *_ in got} == {2, 4}
    assert all(r["kernel"] == "k_gather" for *_, r in got) and {r["TW"] for *_, r in got} == {1, 2}
    assert all(r["rel"] == 1 for *_, r in _pick(routes, op="twaceCRT", shape=(8, 8)))


def test_56_2912_reaches_several_tiles_and_a_split_lds_gather(routes):
    assert (_n(56), _n(2912)) == (24, 1152)
    al = [x for x in _pick(routes, shape=(56, 2912)) if x[2] and x[0][3] == "mixed"]
    up = [r for c, op, a, r in al if op in ("embedPow", "embedDec")]
    assert {r["kernel"] for r in up} == {"k_gather"}
    assert {r["tiles"] for r in up} == {3, 4, 6, 8} and all(r["partial"] for r in up)
    lds = {c[2]: r for c, op, a, r in al if op == "embedCRT"}
    assert all(r["kernel"] == "k_gather_lds" and r["split"] > 1 for r in lds.values())
    assert {T: (r["TW"], r["cpt"], r["split"]) for T, r in lds.items()} == {4: (2, 2, 3), 5: (1, 5, 6), 6: (2, 3, 4), 7: (1, 7, 8)}
    assert all(r["partial"] for r in lds.values())
    assert all(r["rel"] == 48 for *_, r in _pick(routes, op="twaceCRT", shape=(56, 2912)))
    # the unaligned calls of the even T: split > 1 with cpt = 4 and 6 at one word per chunk
    assert {(r["TW"], r["cpt"]) for c, op, a, r in _pick(routes, op="embedCRT", shape=(56, 2912)) if not a and r["split"] > 1} \
        == {(1, 4), (1, 6)}


def test_728_2912_reaches_two_twace_crt_tiles_with_a_partial_last_one(routes):
    got = {c[2]: r for c, op, a, r in _pick(routes, op="twaceCRT", shape=(728, 2912)) if a}
    assert {T: (r["chunks"], r["tiles"], r["partial"]) for T, r in got.items()} == {4: (576, 2, True), 3: (864, 2, True)}
    assert got[4]["TW"] == 2 and got[3]["TW"] == 1


def test_4096_12288_sits_on_the_lds_admission_limit(routes):
    assert (_n(4096), _n(12288)) == (2048, 4096)
    cases = [c for c in tw.CASES if c[:2] == (4096, 12288)]
    assert [c[2] for c in cases] == [4, 5]                                 # the limit, then the first size above it
    at, above = (next(r for c, op, a, r in routes if c == case and op == "embedCRT" and a) for case in cases)
    assert (at["kernel"], at["src_bytes"], at["lds"], at["split"], at["TW"], at["cpt"]) == ("k_gather_lds", 65536, 65536, 1, 2, 2)
    assert (above["kernel"], above["src_bytes"], above["lds"]) == ("k_gather", 81920, 0)
    assert [r["tiles"] for c, op, a, r in routes if c in cases and op == "twaceCRT" and a] == [8, 20]
    # one word off, T = 4 still fits: the LDS route at one component per access
    off = next(r for c, op, a, r in routes if c == cases[0] and op == "embedCRT" and not a)
    assert (off["kernel"], off["TW"], off["cpt"], off["lds"]) == ("k_gather_lds", 1, 4, 65536)


def test_alignment_cases_take_the_one_word_route_when_either_slab_is_off():
    assert tw.ALIGN_OFFSETS == [(1, 1), (1, 2), (2, 1)]
    got = _routes(tw.ALIGN_CASES, lambda T: tw.ALIGN_OFFSETS)
    assert len(got) == 2 * 3 * 5 and all(c[2] == 4 and not al and r["TW"] == 1 and r["cpt"] == 4 for c, op, al, r in got)
    assert all(c in tw.CASES for c in tw.ALIGN_CASES)                      # the aligned words are checked against the oracle


def test_largest_slab_and_chunk_index(routes):
    assert max(tw.B_OPS * _n(c[1]) * c[2] for c in tw.CASES) == 4096 * 5 * 3
    for c, op, al, r in routes:
        assert r["max_chunk"] < 16384 * r["cpt"] + 1024, (c, op)


def test_magic_division_is_exact_for_every_chunk_index_a_launch_forms():
    for cpt in range(1, 65):
        magic = 2 ** 32 // cpt + 1
        assert cpt == 1 or magic < 2 ** 32                                  # cpt = 1 bypasses the multiply (kernels.hip)
        c = np.arange(16384 * cpt + 1024, dtype=np.uint64)
        assert int(c[-1]) * magic < 2 ** 64
        assert np.array_equal((c * np.uint64(magic)) >> np.uint64(32), c // np.uint64(cpt)), cpt


def test_moduli_helper_widths():
    for m in (8, 12, 21, 45, 2912, 12288, 60, 84, 80):
        qs = tw.moduli(m, 16, "mixed")
        assert [q.bit_length() for q in qs] == [tw.WIDTHS[t % 4] for t in range(16)]
        assert len(set(qs)) == 16 and all(q % m == 1 and lm.is_prime(q) for q in qs)
        for kind, bits in (("u61", 61), ("u59", 59)):
            qs = tw.moduli(m, 8, kind)
            assert all(q.bit_length() == bits and q % m == 1 for q in qs) and len(set(qs)) == 8


def test_inputs_reach_zero_under_a_negated_embed_dec_entry():
    """row 1 is zero at every odd coefficient: a negated entry of embedDec that reads one takes the x = 0 branch"""
    hit = set()
    for m, m2 in tw.SMALL + [(56, 2912)]:
        ents = lm.base_indices_dec(lm.factor_pps(m), lm.factor_pps(m2))
        negs = [e[0] for e in ents if e is not None and e[1]]
        if any(sh % 2 == 1 for sh in negs):
            hit.add((m, m2))
    assert {(3, 21), (4, 12), (56, 2912)} <= hit
    qs, Rl, Rh, lo, hi = tw.case_inputs(3, 21, 4, "mixed")
    assert (lo[0] == np.array(qs) - 1).all() and (lo[1, 1::2] == 0).all() and (lo[1, ::2] == np.array(qs) - 1).all()
    assert (tw.neg(lo, qs) <= 0).all() and ((tw.neg(lo, qs) % np.array(qs)) == lo).all()


ORACLE_CASES = [(m, m2, T, kind) for m, m2 in tw.SMALL + [(8, 8)] for T, kind in ((4, "mixed"), (7, "mixed"), (2, "u61"), (2, "u59"))]


@pytest.mark.parametrize("m,m2,T,kind", ORACLE_CASES, ids=[tw.case_id(c) for c in ORACLE_CASES])
def test_oracle_identities_at_wide_moduli(cpuref, m, m2, T, kind):
    qs, Rl, Rh, lo, hi = tw.case_inputs(m, m2, T, kind)
    r = lambda R, y: np.asarray(y).reshape(-1, R.n, R.T)
    # the Python twace_crt (tweak table and sums in Python integers) against the compiled transforms
    assert np.array_equal(cpuref.twace_crt(Rl, Rh, hi), r(Rl, cpuref.crt(Rl, cpuref.twace_powdec(Rl, Rh, r(Rh, cpuref.crtinv(Rh, hi))))))
    assert np.array_equal(cpuref.twace_crt(Rl, Rh, cpuref.embed_crt(Rl, Rh, lo)), lo)
    assert np.array_equal(cpuref.twace_powdec(Rl, Rh, cpuref.embed_pow(Rl, Rh, lo)), lo)
    assert np.array_equal(cpuref.embed_crt(Rl, Rh, lo), r(Rh, cpuref.crt(Rh, cpuref.embed_pow(Rl, Rh, r(Rl, cpuref.crtinv(Rl, lo))))))
    assert np.array_equal(cpuref.embed_dec(Rl, Rh, lo), r(Rh, cpuref.linv(Rh, cpuref.embed_pow(Rl, Rh, r(Rl, cpuref.l(Rl, lo))))))
    # negative representatives name the same residues
    assert np.array_equal(cpuref.twace_crt(Rl, Rh, tw.neg(hi, qs) % np.array(qs)), cpuref.twace_crt(Rl, Rh, hi))
