#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, kernel by kernel.  CPU only: it reads object files.

    python tools/device_code_diff.py OLD NEW        # two build trees (every *.o below them, paired by name) or two .o files

Per object file: the `.hip_fatbin` section is dumped with llvm-objcopy, the gfx950 code object unbundled from it with
clang-offload-bundler, disassembled with llvm-objdump and its kernel metadata read with llvm-readelf --notes.  Reported:
functions present on one side only, and functions whose instruction text or metadata record (VGPR / AGPR / SGPR counts,
LDS, scratch, kernarg size, ...) differs.  The raw code objects differ between builds in their symbol hash tables even
when no instruction moved, hence the comparison per function and not by file hash.  Exit status 0: nothing differs and
nothing is new; 1 otherwise (functions that only disappeared are listed but do not fail the run).
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
RECORD_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
               ".kernarg_segment_size")


def find_tool(name):
    for d in (os.environ.get("ROCM_LLVM_BIN"), "/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin"):
        if d and os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    path = shutil.which(name)
    if not path:
        sys.exit(f"{name} not found (set ROCM_LLVM_BIN)")
    return path


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """The gfx950 code object inside a host object file, or None (a host-only file)."""
    fat = os.path.join(tmp, "fatbin")
    co = os.path.join(tmp, "gfx950.co")
    for f in (fat, co):
        if os.path.exists(f):
            os.remove(f)
    subprocess.run([find_tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o")],
                   capture_output=True)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    run(find_tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}")
    return co


def functions(co):
    """symbol -> instruction text."""
    text = run(find_tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co)
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:\s*$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None and line.strip() and line.strip() != "...":   # ("...": zero padding up to the next function)
            out[name].append(re.sub(r"\s*//.*$", "", line).strip())   # (trailing comments carry addresses)
    # A PC-relative address (s_getpc_b64, then s_add_u32 / s_addc_u32 of a displacement) changes whenever anything between
    # the instruction and its target changes size, e.g. a kernel that left the file: the displacement is not compared.
    for lines in out.values():
        for i, ins in enumerate(lines):
            if ins.startswith("s_getpc_b64"):
                for j in range(i + 1, min(i + 3, len(lines))):
                    lines[j] = re.sub(r"^(s_addc?_u32 \S+ \S+) \S+$", r"\1 <pc-relative>", lines[j])
    return {k: "\n".join(v) for k, v in out.items()}


def metadata(co):
    """kernel name -> its record of the amdhsa.kernels note, as text."""
    text = run(find_tool("llvm-readelf"), "--notes", co)
    start = text.find("amdhsa.kernels:")
    if start < 0:
        return {}
    body = text[start:].split("\n", 1)[1]
    end = re.search(r"^\S", body, re.M)   # the next top-level key
    if end:
        body = body[:end.start()]
    out = {}
    for block in re.split(r"^  - ", body, flags=re.M)[1:]:
        m = re.search(r"^\s*\.name:\s*(\S+)", block, re.M)
        if m:
            out[m.group(1).strip("'\"")] = block.rstrip()
    return out


def record(block):
    return {k: v for k, v in re.findall(r"^\s*(\.\w+):\s*(\S+)\s*$", block, re.M) if k in RECORD_KEYS}


def objects(path):
    if os.path.isfile(path):
        return {os.path.basename(path): path}
    found = {}
    for root, _, files in os.walk(path):
        for f in files:
            if f.endswith(".o"):
                found[os.path.relpath(os.path.join(root, f), path)] = os.path.join(root, f)
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--list", action="store_true", help="name every function that disappeared, not only their number")
    args = ap.parse_args()
    old, new = objects(args.old), objects(args.new)
    if os.path.isfile(args.old) and os.path.isfile(args.new):
        new = {next(iter(old)): next(iter(new.values()))}
    total = dict(units=0, same=0, differ=0, gone=0, added=0)
    with tempfile.TemporaryDirectory() as tmp:
        for unit in sorted(set(old) | set(new)):
            if unit not in old or unit not in new:
                print(f"{unit}: only in {'OLD' if unit in old else 'NEW'}")
                total["added" if unit in new else "gone"] += 1
                continue
            sides = []
            for i, obj in enumerate((old[unit], new[unit])):
                sub = os.path.join(tmp, str(i))
                os.makedirs(sub, exist_ok=True)
                co = code_object(obj, sub)
                sides.append(None if co is None else (functions(co), metadata(co)))
            if sides[0] is None and sides[1] is None:
                print(f"{unit}: no device code on either side")
                continue
            if sides[0] is None or sides[1] is None:
                print(f"{unit}: device code only in {'NEW' if sides[0] is None else 'OLD'}")
                total["differ"] += 1
                continue
            (f0, m0), (f1, m1) = sides
            total["units"] += 1
            gone, added = sorted(set(f0) - set(f1)), sorted(set(f1) - set(f0))
            differ = []
            for name in sorted(set(f0) & set(f1)):
                what = []
                if f0[name] != f1[name]:
                    what.append("instructions")
                if m0.get(name) != m1.get(name):
                    r0, r1 = record(m0.get(name, "")), record(m1.get(name, ""))
                    what.append("metadata " + (", ".join(f"{k} {r0.get(k)} -> {r1.get(k)}" for k in RECORD_KEYS if r0.get(k) != r1.get(k))
                                               or "(outside the resource record)"))
                if what:
                    differ.append(f"{name}: {'; '.join(what)}")
            n_same = len(set(f0) & set(f1)) - len(differ)
            total["same"] += n_same
            total["differ"] += len(differ)
            total["gone"] += len(gone)
            total["added"] += len(added)
            kernels = f"{len(m0)} -> {len(m1)} kernels"
            print(f"{unit}: {kernels}; {n_same} functions identical, {len(differ)} differ, {len(gone)} only in OLD, {len(added)} only in NEW")
            for d in differ:
                print(f"    DIFFERS  {d}")
            for name in added:
                print(f"    NEW      {name}")
            if args.list:
                for name in gone:
                    print(f"    GONE     {name}")
    print(f"summary: {total['units']} translation units with device code; {total['same']} functions identical, "
          f"{total['differ']} differ, {total['gone']} only in OLD, {total['added']} only in NEW")
    return 1 if total["differ"] or total["added"] else 0


if __name__ == "__main__":
    sys.exit(main())
