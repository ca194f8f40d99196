#!/usr/bin/env python3
"""Instruction counts of the layer boundary of the one-launch chess tower, from the compiler's assembly (no GPU needed).

    tools/layer_boundary_isa.py [--source kz_tower.hip] [--label NAME] [--asm FILE.s]

Runs hipcc -S --cuda-device-only on kzero_amd/csrc/kz_tower.hip with build.sh's flags (or reads FILE.s) and, for every
two-boards-per-workgroup instance of kz_tower_resident, finds the loop over the 3x3 layers — the outermost loop that holds
the 704-MFMA dx loop — and prints, block by block in program order, how many instructions of each class it holds: the head
of a layer (before the dx loop), the dx loop, and every block of the tail up to the barrier.  Blocks are basic-block runs
between two labels; a block that is one arm of a branch (one epilogue variant, one special super-step) shows as its own
line.  Registers, scratch and spill counts come from the kernel's metadata comment.

With --source another copy of the file (the parent commit's, for instance) is compiled with the headers of this tree's
directory.  profiles/boundary/isa_counts.txt holds the output for the parent and for this tree."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "kzero_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

CLASSES = [  # first match wins
    ("mfma", r"v_mfma_"),
    ("accvgpr_mov", r"v_accvgpr_mov_b32"),
    ("accvgpr_write", r"v_accvgpr_write_b32"),
    ("accvgpr_read", r"v_accvgpr_read_b32"),
    ("max_i32", r"v_max_i32"),
    ("pk_max_i16", r"v_pk_max_i16"),
    ("cvt_pk_f16", r"v_cvt_pk(rtz)?_f16_f32"),
    ("cvt_f32_f16", r"v_cvt_f32_f16"),
    ("pk_add_f32", r"v_pk_(add|fma|mul)_f32"),
    ("ds_read_b128", r"ds_read_b128"),
    ("ds_read_other", r"ds_read"),
    ("ds_write", r"ds_write"),
    ("global_load", r"global_load"),
    ("scratch", r"scratch_"),
    ("waitcnt", r"s_waitcnt"),
    ("s_nop", r"s_nop"),
    ("barrier", r"s_barrier"),
    ("branch", r"s_c?branch"),
    ("other_valu", r"v_"),
    ("salu", r"s_"),
]


def build_flags():
    """FLAGS of kzero_amd/csrc/build.sh, the product build"""
    text = open(os.path.join(CSRC, "build.sh")).read()
    m = re.search(r'^FLAGS="([^"]*)"', text, re.M)
    flags = m.group(1).replace("$DEFS", "").replace("${KZ_EXTRA_FLAGS:-}", "")
    return flags.split()


def compile_asm(source):
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    cmd = [HIPCC, *build_flags(), "-I", CSRC, "-x", "hip", "-S", "--cuda-device-only", source, "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    text = open(out).read()
    os.unlink(out)
    return text


def classify(ins):
    for name, pat in CLASSES:
        if re.match(pat, ins):
            return name
    return "other"


def kernels(text):
    """(demangled-ish name, [(label or None, instruction)], metadata dict) per kz_tower_resident<2, ...> instance"""
    lines = text.split("\n")
    for i, line in enumerate(lines):
        m = re.match(r"(_ZN2kz\S*kz_tower_residentILi2E(\S*?)EEv\S*):", line)
        if not m:
            continue
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        items = []
        for l in lines[i + 1:end]:
            s = l.strip()
            if s.startswith(".LBB"):
                items.append((s.split(":")[0], None))
            elif s and not s.startswith((";", ".")):
                items.append((None, s.split(";")[0].strip()))
        meta = {}
        for l in lines[end:end + 80]:
            mm = re.match(r"; (NumVgprs|NumAgprs|ScratchSize|TotalNumSgprs|Occupancy): (\d+)", l)
            if mm:
                meta[mm.group(1)] = int(mm.group(2))
            if l.startswith(".Lfunc_begin") or re.match(r"_ZN", l):
                break
        for l in lines[i:end]:  # the remarks clang leaves in the body, if any
            mm = re.search(r"; (\d+)-byte Folded (Spill|Reload)|vgpr_spill_count", l)
            if mm:
                meta["spill_remarks"] = meta.get("spill_remarks", 0) + 1
        flags = m.group(2).replace("Lb1", "true").replace("Lb0", "false").replace("Li", "").split("E")
        yield "kz_tower_resident<2, " + ", ".join(f for f in flags if f) + ">", items, meta


def blocks_of(items):
    """[(label, [instructions])] in program order"""
    out = [("entry", [])]
    for label, ins in items:
        if label:
            out.append((label, []))
        else:
            out[-1][1].append(ins)
            if re.match(r"s_c?branch", ins):  # what follows a branch is a block of its own
                out.append((out[-1][0].rstrip("'") + "'", []))
    return out


def hist(instrs):
    c = collections.Counter(classify(i) for i in instrs)
    return ", ".join(f"{c[n]} {n}" for n, _ in CLASSES + [("other", "")] if c[n])


def report(name, items, meta):
    blocks = blocks_of(items)
    index = {label: k for k, (label, _) in enumerate(blocks)}
    # loops: a branch to a label at or before its own block
    loops = []
    for k, (label, instrs) in enumerate(blocks):
        for ins in instrs:
            m = re.match(r"s_c?branch\S*\s+(\.LBB\S+)", ins)
            if m and index.get(m.group(1), 1 << 30) <= k:
                loops.append((index[m.group(1)], k))

    # (a loop with several latches — one per epilogue variant — is one loop: header to last latch)
    loops = sorted({lo: (lo, max(h for l, h in loops if l == lo)) for lo, _ in loops}.values())

    def mfmas(lo, hi):
        return sum(classify(i) == "mfma" for _, b in blocks[lo:hi + 1] for i in b)

    # the dx loop of the 3x3 layers: the innermost loop with at least 704 MFMAs; the layer loop: the smallest loop around it.
    # Where the dx loop is unrolled the innermost such loop IS the layer loop, and the k-loop is what lies between its
    # first and its last MFMA.
    inner = min((l for l in loops if mfmas(*l) >= 704), key=lambda l: l[1] - l[0])
    around = [l for l in loops if l[0] <= inner[0] and l[1] >= inner[1] and l != inner and mfmas(*l) < 3 * 2112]
    layer = min(around, key=lambda l: l[1] - l[0]) if around else inner
    flat = [(label, ins) for label, instrs in blocks[layer[0]:layer[1] + 1] for ins in instrs]
    if around:
        first = sum(len(b) for _, b in blocks[layer[0]:inner[0]])
        last = first + sum(len(b) for _, b in blocks[inner[0]:inner[1] + 1]) - 1
        kname = "dx loop (3 trips per layer)"
    else:
        at = [k for k, (_, ins) in enumerate(flat) if classify(ins) == "mfma"]
        first, last = at[0], at[-1]
        kname = "k-loop, dx unrolled (first to last MFMA of a layer)"
    print(f"== {name}")
    print(f"   registers: {meta.get('NumVgprs')} VGPR + {meta.get('NumAgprs')} AGPR, {meta.get('TotalNumSgprs')} SGPR; "
          f"scratch {meta.get('ScratchSize')} bytes; scratch instructions in the kernel: "
          f"{sum(classify(i) == 'scratch' for _, i in items if i)}")
    for part, seg in (("head of a layer", flat[:first]), (kname, flat[first:last + 1]), ("tail of a layer", flat[last + 1:])):
        runs = []
        for label, ins in seg:
            if not runs or runs[-1][0] != label:
                runs.append((label, []))
            runs[-1][1].append(ins)
        print(f"   {part}: {len(seg)} instructions in {len(runs)} blocks")
        small = [i for _, instrs in runs if len(instrs) < 30 for i in instrs]
        for label, instrs in runs:
            if len(instrs) >= 30:
                print(f"      {label:<12} {len(instrs):5d}: {hist(instrs)}")
        if small:
            n_small = sum(len(instrs) < 30 for _, instrs in runs)
            print(f"      {str(n_small) + ' short':<12} {len(small):5d}: {hist(small)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", default=os.path.join(CSRC, "kz_tower.hip"))
    ap.add_argument("--asm")
    ap.add_argument("--label", default="this tree")
    args = ap.parse_args()
    text = open(args.asm).read() if args.asm else compile_asm(args.source)
    print(f"# {args.label}: kz_tower.hip, flags {' '.join(build_flags())}")
    for name, items, meta in kernels(text):
        try:
            report(name, items, meta)
        except ValueError:
            print(f"== {name}: no 3x3 layer loop found")
    return 0


if __name__ == "__main__":
    sys.exit(main())
