#!/usr/bin/env python3
"""Per-kernel codegen table of two device-assembly files of the same source at two commits.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off --cuda-device-only -S FILE.hip -o X.s     (at each commit)
    tools/codegen_table.py PARENT.s NEW.s > profiles/...txt

For every kernel: registers, LDS, spills, scratch and instruction count on both sides; whether the sub-sequence of matrix, LDS and
global-memory instructions is the same, and whether it still is with waits, barriers and branches counted in; and every
mnemonic-level difference of the whole body.
Kernels are matched by name with enum template arguments read as their integer values.  A kernel of NEW.s whose name is a parent's
with one more trailing `false` template argument (a template flag added with its default) is matched to that parent; kernels that
only NEW.s holds (the flag's `true` instantiations) are listed behind the table with their own figures."""
import difflib
import re
import subprocess
import sys

FIELDS = ["vgpr_count", "sgpr_count", "group_segment_fixed_size", "vgpr_spill_count", "private_segment_fixed_size"]
MEMORY = re.compile(r"^(v_mfma|ds_|global_|buffer_|flat_|scratch_)")
ORDERED = re.compile(MEMORY.pattern + r"|^(s_waitcnt|s_barrier|s_cbranch|s_branch|s_setpc|s_endpgm)")


def canon(sym):
    # (every enum template argument becomes its integer, whatever its type: two kernels that differ only in the TYPE of an enum
    # argument would fall together -- the assertion on the kernel count in main() then fails)
    return re.sub(r"LNS_\d+[A-Za-z_]+E(\d+)E", r"Li\1E", sym)


def parse(path):
    text = open(path).read().splitlines()
    meta, cur = {}, None
    for ln in text:                                   # the kernels' list of .amdgpu_metadata: one "  - ." entry each, keys at indent 4
        if ln.startswith("  - ."):
            cur = {}
            ln = "    " + ln[4:]
        m = re.match(r"^    \.(\w+):\s+(\S+)$", ln)
        if cur is not None and m:
            cur[m.group(1)] = m.group(2)
            if "name" in cur:
                meta[canon(cur["name"])] = cur
    body, name = {}, None
    for ln in text:
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name = canon(m.group(1))
            body[name] = []
            continue
        if ln.startswith(".Lfunc_end"):
            name = None
            continue
        if name is None:
            continue
        m = re.match(r"^\s+([a-z]\w+)", ln)
        if m and not ln.lstrip().startswith((".", ";")):
            body[name].append(m.group(1))
    return meta, body


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
        return {n: re.sub(r"\(anonymous namespace\)::|void |\(DecodeGemmParams\)", "", d) for n, d in zip(names, out)}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    pm, pb = parse(sys.argv[1])
    nm, nb = parse(sys.argv[2])
    names = sorted(pm)
    for k in sorted(nm):                              # a trailing `false` template argument more than the parent's name
        old = re.sub(r"Lb0EEEv", "EEv", k, count=1)
        if k not in pm and old in pm and old not in nm:
            nm[old], nb[old] = nm.pop(k), nb.pop(k)
    added = sorted(set(nm) - set(pm))
    for k in added:
        pm[k], pb[k] = nm[k], nb[k]                   # (no parent: shown against itself)
    names = sorted(pm)
    assert names == sorted(nm), "a kernel of the parent is missing from the new file"
    assert len(names) == len(pb) == len(nb), "kernel names fell together after enum arguments were read as integers"
    pretty = demangle(names)
    print("kernel | vgpr | sgpr | lds | spill | scratch | instructions   (parent -> new where they differ) | MFMA / LDS / global sequence | the same with waits, barriers, branches | mnemonic diff lines")
    notes, bad_mem, bad_ord, bad_spill = [], 0, 0, 0
    for k in names:
        cols = []
        for f in FIELDS:
            a, b = pm[k].get(f, "0"), nm[k].get(f, "0")
            cols.append(a if a == b else f"{a} -> {b}")
        a, b = pb[k], nb[k]
        cols.append(str(len(a)) if len(a) == len(b) else f"{len(a)} -> {len(b)}")
        same_mem = [x for x in a if MEMORY.match(x)] == [x for x in b if MEMORY.match(x)]
        same_ord = [x for x in a if ORDERED.match(x)] == [x for x in b if ORDERED.match(x)]
        ops = [o for o in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes() if o[0] != "equal"]
        nd = sum(max(i2 - i1, j2 - j1) for _, i1, i2, j1, j2 in ops)
        spills = int(nm[k].get("vgpr_spill_count", 0)) + int(nm[k].get("private_segment_fixed_size", 0))
        bad_mem += not same_mem
        bad_ord += not same_ord
        bad_spill += spills != 0
        print(f"{'NEW ' if k in added else ''}{pretty[k]} | " + " | ".join(cols) + f" | {'identical' if same_mem else 'DIFFERENT'} | {'identical' if same_ord else 'DIFFERENT'} | {nd}")
        if ops:
            notes.append(f"\n{pretty[k]}")
            for _, i1, i2, j1, j2 in ops:
                notes.append(f"  @{i1}: - {' '.join(a[i1:i2]) or '(nothing)'}\n  {' ' * len(str(i1))}   + {' '.join(b[j1:j2]) or '(nothing)'}")
    print(f"\n{len(names)} kernels ({len(added)} only in the new file, marked NEW); spills or scratch in {bad_spill}; MFMA / LDS / global sequence different in {bad_mem}; with waits, barriers and branches in {bad_ord}")
    print("\nMnemonic-level differences (parent '-', new '+', @ = instruction index in the parent's body):" + ("" if notes else " none"))
    print("\n".join(notes))


if __name__ == "__main__":
    main()
