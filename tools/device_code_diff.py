#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libndp_hip.so, kernel by kernel.

    python tools/device_code_diff.py OLD.so NEW.so [--labels OLD_NAME NEW_NAME] [--out FILE]

The code object is taken out of each library's .hip_fatbin section (objcopy, clang-offload-bundler) and disassembled
(llvm-objdump -d).  A function's text is its instructions WITH their encodings and without the addresses they stand at, so a
function that merely moved compares equal; one whose instructions, registers, immediates or branch distances changed does not.
(The one literal that moves with a function, the pc-relative distance to a data symbol behind s_getpc_b64, is left out too.)
Prints the two function counts, the names present on one side only and the names whose text differs; exit status 1 if any differs.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def functions(lib):
    """{name: [instruction + encoding, ...]} of the gfx950 code object in `lib`."""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                               f"--targets={TARGET}", f"--output={co}"])
        text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", co], text=True)
    out, cur, pcrel = {}, None, 0
    for line in text.splitlines():
        head = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if head:
            cur, pcrel = out.setdefault(head.group(1), []), 0
        elif cur is not None and line.startswith("\t"):
            ins, _, enc = line.partition("//")
            ins, enc = ins.strip(), enc.partition(":")[2].strip()           # "// 000000114D00: C0060100 ..." -> the encoding alone
            # the two adds behind s_getpc_b64 carry the DISTANCE to a symbol of the data section: an address, not code
            if pcrel and re.match(r"s_addc?_u32 s\d+, s\d+, (0x[0-9a-f]+|-?\d+)$", ins):
                ins, enc = ins.rsplit(",", 1)[0] + ", <pc-relative>", enc.split()[0]
            pcrel = 2 if ins.startswith("s_getpc_b64") else max(pcrel - 1, 0)
            cur.append((ins, enc))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--labels", nargs=2, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    la, lb = args.labels or (args.old, args.new)
    a, b = functions(args.old), functions(args.new)
    differ = sorted(k for k in a.keys() & b.keys() if a[k] != b[k])
    lines = [f"# gfx950 device code of libndp_hip.so, function by function (tools/device_code_diff.py): instructions and encodings, addresses left out",
             f"old: {la}: {len(a)} functions, {sum(map(len, a.values()))} instructions",
             f"new: {lb}: {len(b)} functions, {sum(map(len, b.values()))} instructions",
             f"only in old: {', '.join(sorted(a.keys() - b.keys())) or 'none'}",
             f"only in new: {', '.join(sorted(b.keys() - a.keys())) or 'none'}",
             f"in both and identical: {len(a.keys() & b.keys()) - len(differ)}",
             f"in both and different: {', '.join(differ) or 'none'}"]
    for k in differ:
        n = next((i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y), min(len(a[k]), len(b[k])))
        lines.append(f"  {k}: {len(a[k])} -> {len(b[k])} instructions, first difference at instruction {n}")
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    if args.out:
        with open(args.out, "w") as f:
            f.write(report)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
