#!/usr/bin/env python3
"""tools/check_csub_exec.py <file.s> [--class AR] [--expect-none] — static audit of the EXEC-predicated trims
(csubx, zq_dev.h) in gfx950 assembly text (hipcc -S --cuda-device-only).

For every kernel, every v_cmpx_* must
  * come after an `s_mov_b64 s[a:b], exec` whose pair nothing has written since, and
  * be followed, before any branch, barrier, s_endpgm, label or further v_cmpx, by `s_mov_b64 exec, s[a:b]` of such a
    pair, with no write to the pair in between;
  * be at least 4 wait states ahead of any v_readlane / v_readfirstlane / v_writelane and 5 ahead of any DPP
    instruction (the gfx940-class "VALU writes EXEC" rules; the hazard recogniser does not look into asm blocks).
With --class AR (default 1) the kernels k_pow2<*, *, AR, ...> must also have no VGPR spill, no scratch and at most
128 VGPRs, the per-lane-modulus instantiations among them (n < 1024, T1 = false) and every kernel of another
arithmetic class must hold no v_cmpx at all.  --expect-none: no v_cmpx anywhere (LOLHIP_CSUB_EXEC=0 builds).
Exit status 1 on any violation."""
import re
import sys

LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
PAIR = r"s\[(\d+):(\d+)\]"
SAVE = re.compile(r"^s_mov_b64\s+" + PAIR + r",\s*exec\b")
RESTORE = re.compile(r"^s_mov_b64\s+exec,\s*" + PAIR)
SDST = re.compile(r"^s_\w+\s+(?:s(\d+)|" + PAIR + r")")
VSDST = re.compile(r"^v_(?:mad_u64_u32|mad_i64_i32|add_co_u32|sub_co_u32|subrev_co_u32|addc_co_u32|subb_co_u32|subbrev_co_u32|cmp\w*|div_scale\w*)\s+\S+\s+(?:s(\d+)|" + PAIR + r")")
READLANE = re.compile(r"^v_readlane_b32\s+s(\d+)|^v_readfirstlane_b32\s+s(\d+)")
STOP = re.compile(r"^(s_branch|s_cbranch\w*|s_setpc\w*|s_swappc\w*|s_call\w*|s_barrier|s_endpgm)\b")
LANEOP = re.compile(r"^v_(readlane|readfirstlane|writelane)_b32\b")
KNAME = re.compile(r"k_pow2ILi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])E")


def kernels(text):
    """{name: [instruction lines]} for every function that ends in s_endpgm (labels kept as 'name:')"""
    out, cur, name = {}, None, None
    for raw in text.splitlines():
        line = raw.split(";")[0].strip()
        if not line or line.startswith("."):
            continue
        m = LABEL.match(line)
        if m and cur is None:
            if m.group(1).startswith("_Z"):
                name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        cur.append(line)
        if line.startswith("s_endpgm"):
            out[name], cur = cur, None
    return out


def metadata(text):
    """{name: {key: int}} from the amdhsa.kernels notes (one '  - .key:' list item per kernel, keys at 4 spaces)"""
    out, block, inside = {}, None, False
    for raw in text.splitlines():
        if raw.startswith("amdhsa.kernels:"):
            inside = True
        elif inside and raw[:1] not in (" ", ""):
            inside = False
        if not inside:
            continue
        m = re.match(r"^  (- | {2})\.(\w+):\s*(\S*)", raw)
        if not m:
            continue
        if m.group(1) == "- ":
            block = {}
        if m.group(2) == "name":
            out[m.group(3)] = block
        elif m.group(3).isdigit():
            block[m.group(2)] = int(m.group(3))
    return out


def written_sgprs(line):
    regs = set()
    for rx in (SDST, VSDST):
        m = rx.match(line)
        if m:
            if m.group(1) is not None:
                regs.add(int(m.group(1)))
            elif m.group(2) is not None:
                regs.update(range(int(m.group(2)), int(m.group(3)) + 1))
    m = READLANE.match(line)
    if m:
        regs.add(int(m.group(1) or m.group(2)))
    return regs


def wait_states(line):
    m = re.match(r"^s_nop\s+(\d+)", line)
    return int(m.group(1)) + 1 if m else 1


def audit_kernel(lines):
    """(number of v_cmpx, [violations])"""
    bad, saved, n = [], set(), 0
    for i, line in enumerate(lines):
        if LABEL.match(line) or STOP.match(line):
            saved = set()                      # a save does not carry across control flow
            continue
        m = SAVE.match(line)
        if m:
            saved.add((int(m.group(1)), int(m.group(2))))
            continue
        if not line.startswith("v_cmpx"):
            w = written_sgprs(line)
            saved = {p for p in saved if not (w & set(range(p[0], p[1] + 1)))}
            continue
        n += 1
        if not saved:
            bad.append(f"line {i}: {line}: no live EXEC save before it")
            continue
        live, ws, restored = set(saved), 0, False
        for nxt in lines[i + 1:]:
            if LABEL.match(nxt) or STOP.match(nxt) or nxt.startswith("v_cmpx"):
                break
            m = RESTORE.match(nxt)
            if m:
                restored = (int(m.group(1)), int(m.group(2))) in live
                break
            if nxt.startswith("s_") and re.search(r"\bexec\b", nxt.split(None, 1)[1].split(",")[0] if " " in nxt else ""):
                break                          # some other write of EXEC
            w = written_sgprs(nxt)
            live = {p for p in live if not (w & set(range(p[0], p[1] + 1)))}
        if not restored:
            bad.append(f"line {i}: {line}: EXEC not restored from the pair saved before it")
        for nxt in lines[i + 1:]:
            if ws >= 5:
                break
            if (LANEOP.match(nxt) and ws < 4) or (" dpp" in nxt or "_dpp" in nxt or "row_" in nxt or "quad_perm" in nxt):
                bad.append(f"line {i}: {line}: {nxt.split()[0]} only {ws} wait states later")
                break
            ws += wait_states(nxt)
    return n, bad


def audit(text, ar=1, expect_none=False):
    """[violations] over the whole translation unit; also returns {kernel: v_cmpx count}"""
    ks, md, bad, counts = kernels(text), metadata(text), [], {}
    for name, lines in ks.items():
        n, b = audit_kernel(lines)
        counts[name] = n
        bad += [f"{name}: {x}" for x in b]
        m = KNAME.search(name)
        in_class = bool(m) and int(m.group(3)) == ar
        if expect_none or not in_class:
            if n:
                bad.append(f"{name}: {n} v_cmpx where none is expected")
        if in_class:
            d = md.get(name, {})
            if d.get("vgpr_spill_count", -1) != 0:
                bad.append(f"{name}: vgpr_spill_count {d.get('vgpr_spill_count')}")
            if d.get("private_segment_fixed_size", -1) != 0 or any(x.startswith("scratch_") for x in lines):
                bad.append(f"{name}: uses scratch")
            if not 0 < d.get("vgpr_count", 999) <= 128:
                bad.append(f"{name}: vgpr_count {d.get('vgpr_count')}")
            per_lane_modulus = int(m.group(1)) - 4 < 6 and m.group(4) == "0"
            if per_lane_modulus and n:
                bad.append(f"{name}: {n} v_cmpx in a kernel whose modulus is per lane")
    return bad, counts


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    ar = int(argv[argv.index("--class") + 1]) if "--class" in argv else 1
    if "--class" in argv:
        args.remove(str(ar))
    rc = 0
    for path in args:
        bad, counts = audit(open(path).read(), ar, "--expect-none" in argv)
        print(f"{path}: {len(counts)} kernels, {sum(counts.values())} v_cmpx in {sum(1 for c in counts.values() if c)} of them, {len(bad)} violations")
        for b in bad[:50]:
            print("  " + b)
        rc |= bool(bad)
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
