#!/usr/bin/env python3
"""isa_digest.py [--root TREE] [src.hip ...] -- one line per kernel: name, sha256 of its instruction text, instruction count.

Compiles the kernel sources of csrc/ for gfx950 exactly as tools/isa_lines.py does (device only, no GPU needed) and digests
the disassembly of every kernel symbol.  Two trees whose outputs are equal generate the same device code: run it on a
checkout of the base revision (--root) and on the working tree and diff the two outputs.  What depends on a kernel's PLACE
in the code object, not on its code, is left out of the digest: the address comments, the literal of the s_add_u32 that
follows an s_getpc_b64 (the distance from the instruction to a constant table), and the s_nop padding behind the kernel's
last instruction (alignment of the next kernel; the last kernel of the object carries the prefetch guard's 256 more).
"""
import hashlib
import re
import sys

from isa_lines import ROOT, build

SRCS = ["mbx_stream.hip", "mbx_fec.hip", "mbx_expand.hip", "mbx_api.hip"]


def kernels(text):
    out, cur, pcrel = {}, None, False
    for ln in text.splitlines():
        m = re.match(r"^<(\S+)>:", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        ins = ln.split("//")[0].strip()
        if cur is None or not ins:
            continue
        if pcrel:
            ins = re.sub(r"0x[0-9a-f]+$", "<pcrel>", ins)
        pcrel = ins.startswith("s_getpc_b64")
        cur.append(ins)
    for ins in out.values():
        while ins and ins[-1] == "s_nop 0":
            ins.pop()
    return out


def main():
    args = sys.argv[1:]
    root = args[1] if args[:1] == ["--root"] else ROOT
    for src in (args[2:] if args[:1] == ["--root"] else args) or SRCS:
        for name, ins in sorted(kernels(build(src, line_info=False, root=root)).items()):
            print(name, hashlib.sha256("\n".join(ins).encode()).hexdigest(), len(ins))


if __name__ == "__main__":
    main()
