#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two builds of one HIP source, kernel by kernel (runs anywhere hipcc does, no GPU needed):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S csrc/X.hip -o before/X.s     (same for after/)
    python tools/asm_compare.py before/X.s after/X.s [--md]

The bar of a refactor that must not move the hot path ("What the f16x3 kernels share"): scratch 0, equal LDS, equal
waves per SIMD, equal counts of every MFMA, ds_*, buffer_*, global_*, s_barrier and s_waitcnt opcode, and the same vmcnt immediates.
Prints one row per kernel and exits 1 if a kernel misses the bar."""
import collections
import re
import subprocess
import sys

COUNTED = re.compile(r"^(v_mfma|v_smfmac|ds_|buffer_|global_|flat_|scratch_|s_barrier|s_waitcnt)")


def kernels(path):
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, cur = m.group(1), {"ins": [], "meta": {}}
            out[name] = cur
            continue
        if cur is None:
            continue
        m = re.match(r";\s*(NumVgprs|NumAgprs|ScratchSize|Occupancy|LDSByteSize):\s*(\d+)", line)
        if m:
            cur["meta"][m.group(1)] = int(m.group(2))
            continue
        m = re.match(r"\t([a-z][a-z0-9_]+)(?:\s+(.*?))?\s*(?:;.*)?$", line)
        if m and "Lfunc_end" not in line and "done" not in cur:
            cur["ins"].append((m.group(1), (m.group(2) or "").strip()))
        if line.startswith(".Lfunc_end"):
            cur["done"] = True
    return out


def summary(k):
    ops = collections.Counter(o for o, _ in k["ins"] if COUNTED.match(o))
    vm = sorted(int(x) for o, a in k["ins"] if o == "s_waitcnt" for x in re.findall(r"vmcnt\((\d+)\)", a))
    return ops, vm


def main():
    md = "--md" in sys.argv
    a, b = (kernels(p) for p in [x for x in sys.argv[1:] if not x.startswith("--")][:2])
    bad = 0
    for name in sorted(set(a) | set(b)):
        short = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().replace("us::", "")
        short = re.sub(r"\(.*\)$", "", re.sub(r"^void ", "", short))
        if name not in a or name not in b:
            print(f"{short}: only in {'before' if name in a else 'after'}")
            bad += 1
            continue
        ka, kb = a[name], b[name]
        (oa, va), (ob, vb) = summary(ka), summary(kb)
        ma, mb = ka["meta"], kb["meta"]
        notes = []
        if ka["ins"] == kb["ins"]:
            verdict = "identical"
        else:
            diff = {o: (oa[o], ob[o]) for o in set(oa) | set(ob) if oa[o] != ob[o]}
            ok = (not diff and va == vb and ma.get("ScratchSize") == 0 and mb.get("ScratchSize") == 0
                  and ma.get("LDSByteSize") == mb.get("LDSByteSize") and ma.get("Occupancy") == mb.get("Occupancy"))
            if [o for o, _ in ka["ins"]] == [o for o, _ in kb["ins"]]:
                verdict = "same opcodes in order, operands differ"
            elif ok:
                verdict = "memory, MFMA, barrier and wait counts equal; integer arithmetic differs"
            else:
                verdict = "DIFFERS"
            if not ok:
                bad += 1
                notes.append(f"counts {diff} vmcnt {va if va != vb else ''} -> {vb if va != vb else ''}")
        res = lambda m: f"{m.get('NumVgprs')} + {m.get('NumAgprs')}, {m.get('LDSByteSize')} B, {m.get('Occupancy')}"
        n = lambda k: len(k["ins"])
        if md:
            print(f"| `{short}` | {res(ma)}, {n(ka)} | {res(mb)}, {n(kb)} | {verdict} |")
        else:
            print(f"{short}\n    before {res(ma)}, {n(ka)} instructions; after {res(mb)}, {n(kb)}: {verdict} {' '.join(notes)}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
