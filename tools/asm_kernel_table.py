"""Static table of a device assembly file (hipcc ... --cuda-device-only -S), and a function-by-function diff of two of them.
    python tools/asm_kernel_table.py NEW.s [--match SUBSTRING]        counts per kernel whose demangled name contains SUBSTRING
    python tools/asm_kernel_table.py NEW.s --against PARENT.s         which function bodies differ (labels and debug lines normalised)
The profiles/README of a round that changes a kernel's text quotes both (lessons: 'the other kernels' assembly is the proof')."""
import argparse
import re
import subprocess
import sys


def functions(path):
    """{mangled name: [instruction lines]} and {mangled name: {metadata key: value}}"""
    body, meta, cur = {}, {}, None
    for line in open(path, errors="replace"):
        s = line.strip()
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", line)
        if m and not m.group(1).startswith(".L") and m.group(1).startswith("_Z"):
            cur = m.group(1)
            body[cur] = []
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is not None and s and not s.startswith((";", ".")):
            body[cur].append(re.sub(r"\s*;.*$", "", s))
        m = re.match(r"^;\s*(ScratchSize|NumVgprs|NumAgprs|SGPRBlocks|NumSgprs|codeLenInByte|Occupancy):\s*(\d+)", s)
        if m and body:
            meta.setdefault(list(body)[-1], {})[m.group(1)] = int(m.group(2))
    spills = {}
    txt = open(path, errors="replace").read()
    # the metadata block lists the kernels in order, each with its spill counts
    for blk in txt.split("  - .agpr_count:")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        sg, vg = re.search(r"\.sgpr_spill_count:\s+(\d+)", blk), re.search(r"\.vgpr_spill_count:\s+(\d+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if nm:
            spills[nm.group(1)] = (int(sg.group(1)) if sg else 0, int(vg.group(1)) if vg else 0, int(ps.group(1)) if ps else 0)
    return body, meta, spills


def demangle(names):
    out = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out))


def normal(lines):
    """labels renumber when an unrelated function changes: compare with them blanked"""
    return [re.sub(r"\.L[\w$]+", ".L", x) for x in lines]


def counts(lines):
    c = {"instructions": len(lines)}
    c["v_* (without v_mfma)"] = sum(1 for x in lines if x.startswith("v_") and not x.startswith("v_mfma"))
    c["v_cmp + v_cndmask"] = sum(1 for x in lines if x.startswith(("v_cmp", "v_cndmask")))
    c["branches"] = sum(1 for x in lines if x.startswith(("s_cbranch", "s_branch")))
    c["s_waitcnt"] = sum(1 for x in lines if x.startswith("s_waitcnt"))
    c["v_mfma"] = sum(1 for x in lines if x.startswith("v_mfma"))
    c["v_readlane / v_writelane"] = sum(1 for x in lines if x.startswith(("v_readlane", "v_writelane")))
    c["ds_bpermute"] = sum(1 for x in lines if x.startswith("ds_bpermute"))
    c["s_barrier"] = sum(1 for x in lines if x.startswith("s_barrier"))
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--match", default="k_headsx_gat3x_headsx")
    ap.add_argument("--against")
    a = ap.parse_args()
    body, meta, spills = functions(a.asm)
    names = demangle(list(body))
    if a.against:
        pbody, _, _ = functions(a.against)
        pnames = demangle(list(pbody))
        # a defaulted template parameter changes the mangled name, not the kernel: match on the demangled name without it
        key = lambda d: re.sub(r", H3ShapeAny>", ">", d)
        new = {key(names[k]): normal(v) for k, v in body.items()}
        old = {key(pnames[k]): normal(v) for k, v in pbody.items()}
        same = sorted(k for k in new if k in old and new[k] == old[k])
        diff = sorted(k for k in new if k in old and new[k] != old[k])
        print(f"{len(same)} functions with the parent's assembly, {len(diff)} that differ, {len(set(new) - set(old))} new, {len(set(old) - set(new))} gone")
        for k in diff:
            print("  differs:", k[:140], len(old[k]), "->", len(new[k]))
        for k in sorted(set(new) - set(old)):
            print("  new:", k[:140])
        for k in sorted(set(old) - set(new)):
            print("  gone:", k[:140])
        return 1 if diff else 0
    for k, lines in body.items():
        if a.match not in names[k]:
            continue
        print(names[k][:110])
        for n, v in counts(lines).items():
            print(f"    {n:28s} {v}")
        sg, vg, ps = spills.get(k, (0, 0, 0))
        print(f"    {'scratch per lane (B)':28s} {ps}\n    {'spilled SGPRs / VGPRs':28s} {sg} / {vg}\n    {'VGPRs':28s} {meta.get(k, {}).get('NumVgprs')}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
