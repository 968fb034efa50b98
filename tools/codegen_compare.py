#!/usr/bin/env python3
"""Per-kernel code-generation figures of two revisions of a .hip file, side by side (markdown).

    hipcc --offload-arch=gfx950 -O3 -std=c++20 --cuda-device-only -S old/mgfn.hip -o old.s      (and the same for the new files)
    python tools/codegen_compare.py --old old.s --new mgfn.s optim.s [--hist KERNEL_SUBSTRING]

Each side may be several assembly files (a revision that moved kernels into a second translation unit).  Per kernel: instruction
count (lines of the kernel's text that are neither label, directive nor comment), VGPR / AGPR / SGPR counts, spill counts, private
segment and LDS bytes from the code object's metadata, and the occupancy the register allocation admits on gfx950: waves per
SIMD (512 registers per lane and SIMD, allocated in granules of 8, at most 8 waves) and, from them, workgroups of the kernel's
block size per CU (a workgroup's waves are dealt over the CU's four SIMDs) -- the step that counts for a kernel is the second.
--hist prints the opcode histogram difference of the kernels whose demangled name contains the string.  The tool reads
opcodes as words: it knows no instruction by name.
"""
import argparse
import collections
import re
import subprocess

META = {
    "vgpr": ".vgpr_count", "agpr": ".agpr_count", "sgpr": ".sgpr_count", "vspill": ".vgpr_spill_count", "sspill": ".sgpr_spill_count",
    "private": ".private_segment_fixed_size", "lds": ".group_segment_fixed_size", "wg": ".max_flat_workgroup_size",
}


def parse(path):
    """{symbol: {"insts": n, "hist": Counter, metadata...}} of one assembly file"""
    kernels, cur, in_meta, entry = {}, None, False, None
    for line in open(path):
        s = line.strip()
        if s == ".amdgpu_metadata":
            in_meta = True
        elif s == ".end_amdgpu_metadata":
            in_meta = False
        elif in_meta:
            # a kernel's record: "  - .key: value" opens it, "    .key: value" continues it (its .args sit deeper and are skipped)
            m = re.match(r"^  (?:- |  )(\.[a-z_]+):\s*(\S+)\s*$", line)
            if not m:
                continue
            if line.startswith("  - "):
                entry = {}
            k, v = m.groups()
            if k == ".name":
                kernels.setdefault(v, {}).update(entry)
                entry = kernels[v]
            for name, mk in META.items():
                if k == mk:
                    entry[name] = int(v)
        else:
            m = re.match(r"^([A-Za-z_][\w$.]*):", line)
            if m and not m.group(1).startswith(".L"):
                cur = kernels.setdefault(m.group(1), {})
                cur.setdefault("insts", 0)
                cur.setdefault("hist", collections.Counter())
            elif s.startswith(".Lfunc_end") or s.startswith(".section") or s.startswith(".text"):
                if s.startswith(".Lfunc_end"):
                    cur = None
            elif cur is not None and s and s[0] not in ".;" and not s.endswith(":") and line[0] in " \t":
                op = s.split()[0]
                cur["insts"] += 1
                cur["hist"][op] += 1
    return {k: v for k, v in kernels.items() if "vgpr" in v and "insts" in v}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    short = {}
    for n, d in zip(names, out):
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"\(.*\)$", "", d)  # drop the parameter list, keep template arguments
        short[n] = d.replace("advhip::", "").replace("(anonymous namespace)::", "")
    return short


def waves(k):
    alloc = -(-max(k["vgpr"] + k.get("agpr", 0), 1) // 8) * 8
    return min(8, 512 // alloc)


def groups(k):
    return waves(k) // max(1, -(-k["wg"] // 256))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--hist", default=None)
    a = ap.parse_args()
    old, new = {}, {}
    for p in a.old:
        old.update(parse(p))
    for p in a.new:
        new.update(parse(p))
    names = demangle(sorted(set(old) | set(new)))
    print(f"{len(old)} kernels old, {len(new)} new; only old: {sorted(names[n] for n in set(old) - set(new))}; "
          f"only new: {sorted(names[n] for n in set(new) - set(old))}\n")
    print("| kernel | block | insts old | new | VGPR old | new | waves/SIMD (groups/CU) old | new | SGPR old | new | spills (v+s) old | new | private old | new | LDS old | new |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    flags = []
    for n in sorted(set(old) & set(new), key=lambda n: names[n]):
        o, w = old[n], new[n]
        sp = lambda k: k["vspill"] + k["sspill"]
        vg = lambda k: f"{k['vgpr']}" + (f"+{k['agpr']}a" if k.get("agpr") else "")
        print(f"| `{names[n]}` | {w['wg']} | {o['insts']} | {w['insts']} | {vg(o)} | {vg(w)} | {waves(o)} ({groups(o)}) | {waves(w)} ({groups(w)}) | {o['sgpr']} | {w['sgpr']} | "
              f"{sp(o)} | {sp(w)} | {o['private']} | {w['private']} | {o['lds']} | {w['lds']} |")
        why = []
        if w["insts"] > o["insts"]:
            why.append(f"instructions {o['insts']} -> {w['insts']}")
        if groups(w) < groups(o):
            why.append(f"workgroups per CU {groups(o)} -> {groups(w)}")
        if w["lds"] != o["lds"]:
            why.append(f"LDS {o['lds']} -> {w['lds']}")
        if sp(w) or w["private"]:
            why.append(f"spills {sp(w)}, private segment {w['private']} (old: {sp(o)}, {o['private']})")
        if why:
            flags.append(f"- `{names[n]}`: " + "; ".join(why))
    print("\n" + ("\n".join(flags) if flags else "No kernel has more instructions, fewer workgroups per CU, another LDS size, a spill or a private segment."))
    if a.hist:
        for n in sorted(set(old) & set(new)):
            if a.hist in names[n]:
                print(f"\n`{names[n]}` opcode histogram (old -> new, differing rows):")
                for op in sorted(set(old[n]["hist"]) | set(new[n]["hist"])):
                    if old[n]["hist"][op] != new[n]["hist"][op]:
                        print(f"  {op:28s} {old[n]['hist'][op]:5d} -> {new[n]['hist'][op]:5d}")


if __name__ == "__main__":
    main()
