"""Static checks (-m "not gpu") of the EXEC-predicated lazy-range trims of the 64-bit class (csubx, zq_dev.h;
DESIGN.md 3.1e) on the assembly hipcc produces for gfx950 (compile only, as tools/kreport.sh does).

pow2_ar1.hip and pow2_ar1_t1.hip are compiled with LOLHIP_CSUB_EXEC = 1 (the default) and = 0;
tools/check_csub_exec.py audits the text:

  * every v_cmpx sits between an `s_mov_b64 s[a:b], exec` and, before any branch, barrier, s_endpgm or label, an
    `s_mov_b64 exec, s[a:b]` of that pair, which nothing writes in between (EXEC is never rebuilt from a literal);
  * no v_readlane / v_writelane within 4 wait states and no DPP within 5 of a v_cmpx (the hazard recogniser does not
    look into asm blocks);
  * every k_pow2<*, *, 1, ...>: vgpr_spill_count == 0, no scratch, vgpr_count <= 128;
  * no v_cmpx in a kernel of another arithmetic class, nor in the class-1 kernels whose modulus is per lane
    (n < 1024, T1 = false: they keep the select form);
  * with -DLOLHIP_CSUB_EXEC=0 there is no v_cmpx at all.

The class-1 kernels with a per-lane modulus keep the select form.  Five of them, the fused poly-mul
k_pow2<5..9, 2, 1, false, false>, used to spill 4 to 12 VGPRs to scratch at the 128-VGPR budget; they are now scheduled
register-tight (TIGHT in k_pow2, pow2_impl.h) and test_class1_resources holds for all 74 class-1 kernels.
"""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lol_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNITS = ("pow2_ar1", "pow2_ar1_t1")


def _checker():
    spec = importlib.util.spec_from_file_location("check_csub_exec", os.path.join(ROOT, "tools", "check_csub_exec.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    """{(unit, LOLHIP_CSUB_EXEC): assembly text}; the four compiles run side by side"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail("hipcc not found: the static checks need the gfx950 compiler")
    out = tmp_path_factory.mktemp("csub_exec")
    procs = {}
    for unit in UNITS:
        for flag in (1, 0):
            path = str(out / f"{unit}_{flag}.s")
            cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-I" + os.path.join(ROOT, "include"),
                   f"-DLOLHIP_CSUB_EXEC={flag}", "-S", "--cuda-device-only", os.path.join(CSRC, unit + ".hip"), "-o", path]
            procs[(unit, flag)] = (subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), path)
    texts = {}
    for key, (p, path) in procs.items():
        log, _ = p.communicate(timeout=1800)
        assert p.returncode == 0, f"{key}: hipcc failed\n{log[-2000:]}"
        texts[key] = open(path).read()
    return texts


@pytest.mark.parametrize("unit", UNITS)
def test_exec_save_restore_pairing(asm, unit):
    chk = _checker()
    kernels = chk.kernels(asm[(unit, 1)])
    class1 = [k for k in kernels if (m := chk.KNAME.search(k)) and m.group(3) == "1"]
    assert len(class1) == 37, len(class1)
    total = 0
    for name in class1:
        n, bad = chk.audit_kernel(kernels[name])
        assert not bad, (name, bad[:5])
        total += n
        m = chk.KNAME.search(name)
        uniform = int(m.group(1)) - 4 >= 6 or m.group(4) == "1"
        if uniform:
            assert n > 0, f"{name}: wave-uniform modulus but no predicated trim"
        else:
            assert n == 0, f"{name}: per-lane modulus but {n} v_cmpx"
    assert total > 0
    # the benchmark's kernel: the 348 trims of DESIGN.md 3.1e, all predicated
    bench = [k for k in class1 if "k_pow2ILi13ELi2ELi1ELb1ELb1E" in k]
    if unit == "pow2_ar1_t1":
        assert len(bench) == 1
        lines = kernels[bench[0]]
        assert sum(x.startswith("v_cmpx") for x in lines) == 348
        assert sum(x.startswith("v_cmp_gt_i64") for x in lines) == 0


@pytest.mark.parametrize("unit", UNITS)
def test_class1_resources(asm, unit):
    chk = _checker()
    text = asm[(unit, 1)]
    kernels, md = chk.kernels(text), chk.metadata(text)
    bad = []
    for name, lines in kernels.items():
        m = chk.KNAME.search(name)
        if not m or m.group(3) != "1":
            continue
        d = md[name]
        print(name[:40], {k: d.get(k) for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")})
        if d["vgpr_spill_count"] != 0:
            bad.append((name[:40], "vgpr_spill_count", d["vgpr_spill_count"]))
        if d["private_segment_fixed_size"] != 0 or any(x.startswith("scratch_") for x in lines):
            bad.append((name[:40], "scratch", d["private_segment_fixed_size"]))
        if not d["vgpr_count"] <= 128:
            bad.append((name[:40], "vgpr_count", d["vgpr_count"]))
    assert not bad, bad


@pytest.mark.parametrize("unit", UNITS)
def test_no_cmpx_outside_class1(asm, unit):
    chk = _checker()
    for name, lines in chk.kernels(asm[(unit, 1)]).items():
        m = chk.KNAME.search(name)
        if m and m.group(3) == "1":
            continue
        assert not any(x.startswith("v_cmpx") for x in lines), name


@pytest.mark.parametrize("unit", UNITS)
def test_switch_off_has_no_cmpx(asm, unit):
    text = asm[(unit, 0)]
    assert "v_cmpx" not in text
    chk = _checker()
    bad, counts = chk.audit(text, 1, True)
    assert not any("v_cmpx" in b for b in bad) and sum(counts.values()) == 0


def test_other_classes_have_no_cmpx_source():
    """the other arithmetic classes, mixed_impl.h and the generic kernels never reach csubx: it is only named in
    zq_dev.h (definition), pow2_impl.h (the QKx<true> trims) and nowhere else under csrc"""
    users = []
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".h", ".hip", ".cpp")) and "csubx" in open(os.path.join(CSRC, fn)).read():
            users.append(fn)
    assert users == ["pow2_impl.h", "zq_dev.h"], users
