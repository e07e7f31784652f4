"""The dense stages of the CRT over C (k_cplx_dense, floatpath.hip) on the GPU (-m gpu): plans created with
dense_cplx=True (LOLHIP_PLAN_DENSE_CPLX, lolhip_plan_create_opts) at indices with a prime above 13.

Bound everywhere: the float members' contract, max abs error <= 1e-12 max(1, max |expected|) (tests/test_float.py); for
crtInvC also the normwise backward error of oracle/floatref.crtinv_c_residual <= 1e-12.  lol-cpp itself sits at
3e-16 .. 2e-15 against the same long-double oracle on these indices.

  1 accuracy     every index of cplx_dense_cases.DENSE_INDICES: crtC, crtInvC and the round trip against the long-double
                 oracle and against lol-cpp's own outputs (golden_cplx_dense.npz); the launcher's line names the route
                 of every stage
  2 routes       in fresh child processes under CPLX_DENSE / CPLX_DENSE_VALU: register, vector-ALU and matrix outputs
                 agree pairwise within the bound
  3 lane maps    unit vectors e_j at m = 19 and m = 289: the output is column j of the matrix, for every j
  4 batches      B = 0, 1, one short of and one past a tile; beyond one sweep of the grid; in place on a view under a
                 side stream with guard rows
  5 mulC         round(crtInvC(mulC(crtC a, crtC b))) mod q is RingMul's exact product
  6 refusals     a default plan at m = 17 and an opted-in plan at 3 2^14: LOLHIP_ERR_INVALID, buffer untouched
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from cplx_dense_cases import DENSE_INDICES, LARGE_PARITY, PARITY_INDICES, dense_routes
from float_stages import fixture_columns, stage_inputs
from oracle import floatref as fr
from oracle import lolmath as lm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ERR_INVALID = -1
TOL = 1e-12
ST_DIAG, ST_SCALE = 0, 10
NAMES = {0: "reg", 1: "dense-valu", 2: "dense-mfma"}


def _plan(gpu, m, dense=True):
    return gpu.Plan.for_index(m, [12289], dense_cplx=dense)


def _err(got, want):
    """max abs error over max(1, max |expected|), in the precision of `want`"""
    want = np.asarray(want)
    return float(np.abs(np.asarray(got).astype(want.dtype) - want).max() / max(1.0, float(np.abs(want).max())))


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return np.ascontiguousarray(a).view(np.int64)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "golden_cplx_dense.npz"))


_ORACLE = {}


def oracle(m):
    """(z, crtC z in long double), computed once per index and shared"""
    if m not in _ORACLE:
        z = stage_inputs(m)[0]
        want = fr.crt_c_ext(lm.factor_pps(m), z)
        want.setflags(write=False)
        _ORACLE[m] = (z, want)
    return _ORACLE[m]


@pytest.fixture
def info(monkeypatch, capfd):
    """the launcher's lines since the last read: [(kernel, [route of every stage])]"""
    monkeypatch.setenv("LOLHIP_CPLX_INFO", "1")

    def read():
        return _lines(capfd.readouterr().err)
    return read


def _lines(text):
    return [(ln.split(":")[0], ln.split(" stages ")[1].split()) for ln in text.splitlines() if ln.startswith("k_cplx")]


# ---------------------------------------------------------------------------------------------
# 1. accuracy against the oracle and against lol-cpp's own outputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", DENSE_INDICES)
def test_crtc_and_crtinvc_at_large_primes(gpu, gold, info, m):
    pps = lm.factor_pps(m)
    P = _plan(gpu, m)
    assert P.cplxRoute() == 2 and P.n <= 8192
    z, want = oracle(m)
    info()
    got = P.crtC(z)
    inv = P.crtInvC(z)
    lines = info()
    for (kernel, routes), prog in zip(lines, (P.cplxProgram(), P.cplxProgram(inverse=True))):
        assert kernel == "k_cplx_dense"
        assert routes == [NAMES[r] for r in prog[:, 4].tolist()], (m, routes)
        # the route rule: a stage of a prime above 13 on the matrix cores where an LDS tile holds 16 columns of it, else
        # on the vector ALU (of these indices: m = 797); every other stage in registers
        assert routes == [NAMES[r] for r in dense_routes(prog.tolist(), P.n)]
        assert ("dense-valu" in routes) == (m == 797) and ("dense-mfma" in routes) == (m != 797)
    assert len(lines) == 2
    back = P.crtInvC(got)
    e_f, e_rt = _err(got, want), _err(back, z)
    e_i = float(fr.crtinv_c_residual(pps, inv, z).max())
    cols = fixture_columns(m)
    e_gf, e_gi = _err(got[:, cols], gold[f"m{m}_crtc"]), _err(inv[:, cols], gold[f"m{m}_crtinvc"])
    print(f"cplx-dense-error m={m} crtC={e_f:.3e} crtInvC-residual={e_i:.3e} roundtrip={e_rt:.3e} vs-lol-cpp={e_gf:.3e}/{e_gi:.3e}")
    assert e_f <= TOL and e_i <= TOL and e_rt <= TOL, (m, e_f, e_i, e_rt)
    assert e_gf <= TOL and e_gi <= TOL, (m, e_gf, e_gi)


# ---------------------------------------------------------------------------------------------
# 2. the three routes agree
# ---------------------------------------------------------------------------------------------
def _child(tmp_path, name, indices, **switches):
    out = str(tmp_path / f"{name}.npz")
    env = dict(os.environ, LOLHIP_CPLX_INFO="1", **{f"LOLHIP_{k}": "1" for k in switches})
    r = subprocess.run([sys.executable, os.path.join(HERE, "cplx_dense_child.py"), out, *map(str, indices)], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out), _lines(r.stderr)


def test_register_valu_and_matrix_routes_agree(gpu, info, tmp_path):
    both = PARITY_INDICES + LARGE_PARITY
    mf, mf_lines = _child(tmp_path, "mfma", PARITY_INDICES + [797], CPLX_DENSE=True)
    va, va_lines = _child(tmp_path, "valu", both, CPLX_DENSE=True, CPLX_DENSE_VALU=True)
    assert len(mf_lines) == 2 * len(PARITY_INDICES) + 2 and len(va_lines) == 2 * len(both)
    assert [r for _, r in mf_lines[-2:]] == [["dense-mfma"], ["dense-mfma"]]
    z, want = oracle(797)
    P = _plan(gpu, 797)
    assert P.cplxProgram()[:, 4].tolist() == [1]                   # here the rule's choice is the vector ALU
    assert _err(mf["crtc797"], P.crtC(z)) <= TOL and _err(mf["crtinvc797"], P.crtInvC(z)) <= TOL and _err(mf["crtc797"], want) <= TOL
    for lines, name, ms in ((mf_lines, "dense-mfma", PARITY_INDICES), (va_lines, "dense-valu", both)):
        for i, m in enumerate(ms):
            for kernel, routes in lines[2 * i:2 * i + 2]:
                prog = _plan(gpu, m, dense=False).cplxProgram() if m in PARITY_INDICES else _plan(gpu, m).cplxProgram()
                odd = sum(1 for k, p in prog[:, :2].tolist() if k not in (ST_DIAG, ST_SCALE) and p > 2)
                assert kernel == "k_cplx_dense" and routes.count(name) == odd and set(routes) <= {name, "reg"}, (m, routes)
    for m in both:
        z, want = oracle(m)
        assert int(va[f"route{m}"]) == 2
        P = _plan(gpu, m)
        info()
        here_f, here_i = P.crtC(z), P.crtInvC(z)
        lines = info()
        if m in PARITY_INDICES:
            assert P.cplxRoute() == 1 and [k for k, _ in lines] == ["k_cplx", "k_cplx"]           # no switch here: registers
            assert int(mf[f"route{m}"]) == 2
            triples = [(here_f, va[f"crtc{m}"], mf[f"crtc{m}"]), (here_i, va[f"crtinvc{m}"], mf[f"crtinvc{m}"])]
        else:
            assert P.cplxRoute() == 2 and all("dense-mfma" in r for _, r in lines)                 # no switch here: matrix cores
            triples = [(here_f, va[f"crtc{m}"]), (here_i, va[f"crtinvc{m}"])]
        for outs in triples:
            for a in range(len(outs)):
                for b in range(a + 1, len(outs)):
                    assert _err(outs[a], outs[b]) <= TOL, (m, a, b)
        assert _err(va[f"crtc{m}"], want) <= TOL and _err(here_f, want) <= TOL
        assert float(fr.crtinv_c_residual(lm.factor_pps(m), va[f"crtinvc{m}"], z).max()) <= TOL


# ---------------------------------------------------------------------------------------------
# 3. the lane maps: unit vectors
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [19, 289])
def test_unit_vectors_give_the_columns_of_the_matrix(gpu, m):
    """crtC e_j is column j of the matrix: a swapped pair of lanes, rows or tiles moves whole entries of modulus 1"""
    pps = lm.factor_pps(m)
    P = _plan(gpu, m)
    M = fr.crt_matrix_c(pps)
    got = P.crtC(np.eye(P.n, dtype=np.complex128))
    assert got.shape == (P.n, P.n)
    assert float(np.abs(got - M.T).max()) <= TOL
    inv = P.crtInvC(np.ascontiguousarray(M.T))                  # the inverse takes the columns back to the unit vectors
    assert float(np.abs(inv - np.eye(P.n)).max()) <= TOL


# ---------------------------------------------------------------------------------------------
# 4. batch shapes and calling conventions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [23, 289])
def test_batch_shapes(gpu, m, monkeypatch, capfd):
    """tiles hold ceil(B / 512) items here: B = 1536 fills 512 tiles of 3, B = 1535 leaves the last tile one short,
    B = 1537 makes tiles of 4 with one live item in the last"""
    import torch
    monkeypatch.setenv("LOLHIP_CPLX_INFO", "1")
    pps = lm.factor_pps(m)
    P = _plan(gpu, m)
    n = P.n
    rng = np.random.default_rng(m)
    x = rng.standard_normal((1537, n)) + 1j * rng.standard_normal((1537, n))
    want = fr.crt_c_ext(pps, x[-40:])
    capfd.readouterr()
    whole = {B: P.crtC(x[:B]) for B in (1535, 1536, 1537)}
    items = [int(ln.split(" items ")[1].split(",")[0]) for ln in capfd.readouterr().err.splitlines() if ln.startswith("k_cplx_dense")]
    assert items == [3, 3, 4]
    for B, got in whole.items():
        assert np.array_equal(_bits(got), _bits(whole[1537][:B])), B            # a column's result does not depend on its tile
    assert _err(whole[1537][-40:], want) <= TOL
    assert np.array_equal(_bits(P.crtC(x[1536:1537])), _bits(whole[1537][1536:]))   # B = 1
    assert P.crtC(np.zeros((0, n), dtype=np.complex128)).shape == (0, n)
    assert P.crtInvC(np.zeros((0, n), dtype=np.complex128)).shape == (0, n)
    # in place on a row-offset view under a side stream; the guard rows around the slab stay as they were
    pre, post, K = 2, 3, 5
    sent = torch.from_numpy(rng.standard_normal((pre + K + post, n)) + 1j * rng.standard_normal((pre + K + post, n))).cuda()
    sent[pre:pre + K] = torch.from_numpy(x[:K]).cuda()
    before = sent.clone()
    view = sent[pre:pre + K]
    assert view.is_contiguous() and view.data_ptr() != sent.data_ptr()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = P.crtC(view)
    torch.cuda.synchronize()
    assert out.data_ptr() == view.data_ptr()
    assert torch.equal(sent[:pre], before[:pre]) and torch.equal(sent[pre + K:], before[pre + K:])
    assert np.array_equal(_bits(view), _bits(whole[1537][:K]))
    with torch.cuda.stream(side):
        P.crtInvC(view)
    torch.cuda.synchronize()
    assert torch.equal(sent[:pre], before[:pre]) and torch.equal(sent[pre + K:], before[pre + K:])
    assert _err(view.cpu().numpy(), x[:K]) <= TOL


def test_batch_beyond_one_sweep_of_the_grid(gpu, info):
    """m = 323: two buffers of 288 complex doubles, 7 items fill 64 KiB, so B = 4096 7 + 5 makes 4097 tiles for a grid of
    4096: the first workgroup runs two.  Sampled rows, the first and the last among them, equal their single-row runs."""
    import torch
    m = 323
    P = _plan(gpu, m)
    n, B = P.n, 4096 * 7 + 5
    gen = torch.Generator(device="cuda")
    gen.manual_seed(m)
    x = torch.randn((B, n, 2), dtype=torch.float64, device="cuda", generator=gen)
    keep = torch.view_as_complex(x).cpu().numpy().copy()
    info()
    P.crtC(torch.view_as_complex(x))
    torch.cuda.synchronize()
    lines = info()
    assert lines == [("k_cplx_dense", ["dense-mfma", "dense-mfma"])]
    big = torch.view_as_complex(x).cpu().numpy()
    rng = np.random.default_rng(m)
    rows = np.unique(np.concatenate([[0, 6, 7, B - 1, B - 5, B - 6, 4096 * 7 - 1], rng.choice(B, 25, replace=False)]))
    for i in rows:
        assert np.array_equal(_bits(big[i]), _bits(P.crtC(keep[i:i + 1])[0])), i
    assert _err(big[rows], fr.crt_c_ext(lm.factor_pps(m), keep[rows])) <= TOL


# ---------------------------------------------------------------------------------------------
# 5. end to end through mulC
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,q", [(17, 1024), (257, 2 ** 20)])
def test_ring_product_through_mulc_is_exact(gpu, m, q):
    """n q^2 < 2^53: the product of the centred representatives is an integer float64 holds, and the transforms' error
    stays far below one half, so rounding gives RingMul's product integer for integer"""
    P = gpu.Plan.for_index(m, [q], dense_cplx=True)
    assert P.n * q * q < 2 ** 53 and not P.has_crt
    rng = np.random.default_rng(m)
    B = 3
    a, b = (rng.integers(-q // 2, q // 2, size=(B, P.n), dtype=np.int64) for _ in range(2))
    prod = P.crtInvC(gpu.mulC(P.crtC(a.astype(np.complex128)), P.crtC(b.astype(np.complex128))))
    assert float(np.abs(prod.imag).max()) < 0.25 and float(np.abs(prod.real - np.rint(prod.real)).max()) < 0.25
    got = np.rint(prod.real).astype(np.int64) % q
    want = gpu.RingMul(P)(a.reshape(B, P.n, 1), b.reshape(B, P.n, 1))
    want = want.cpu().numpy() if hasattr(want, "cpu") else want
    assert np.array_equal(got, want.reshape(B, P.n)) and want.any()


# ---------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,dense", [(17, False), (3 * 2 ** 14, True)])
def test_refused_indices_leave_the_buffer_untouched(gpu, m, dense):
    import torch
    L = gpu.lib()
    P = _plan(gpu, m, dense=dense)
    assert P.cplxRoute() == 0
    B = 2
    y = torch.from_numpy(np.random.default_rng(m).standard_normal((B, P.n, 2))).cuda()
    keep = y.clone()
    assert L.lolhip_crtc_batch(P._h, None, y.data_ptr(), B) == ERR_INVALID
    assert L.lolhip_crtinvc_batch(P._h, None, y.data_ptr(), B) == ERR_INVALID
    for fn in (P.crtC, P.crtInvC):
        with pytest.raises(gpu.LolHipError) as ei:
            fn(torch.view_as_complex(y))
        assert ei.value.code == ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(y, keep)
