#!/usr/bin/env python3
"""Instruction mix of the K loop of every gemm_pp_kernel instantiation in an assembly listing
(hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -S --cuda-device-only FILE.hip -o FILE.s).

The K loop is taken as the stretch between the first and the last MFMA of a kernel.  Columns: all instructions, MFMAs, other
vector ALU, lane reads / writes (SGPR spill traffic), scratch accesses (VGPR spill traffic), scalar instructions
(waits, barriers and nops included), branches, LDS-DMA, plus the spill counts of the kernel's metadata.

usage: conv_stage_isa.py FILE.s [FILE.s ...]"""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(path):
    """name -> list of instruction lines of the function body"""
    out, cur = {}, None
    for line in open(path):
        s = line.strip()
        m = re.match(r"^(_Z\w*gemm_pp_kernel\w*):", s)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if s.startswith(".end_amdhsa_kernel") or s.startswith("s_endpgm"):
            cur = None
            continue
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        cur.append(s.split(";")[0].strip())
    return out


def spills(path):
    """kernel name -> (sgpr_spill_count, vgpr_spill_count) from the metadata"""
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"\.name:\s+(_Z\w*gemm_pp_kernel\w*)\n(.*?)\.wavefront_size", txt, re.S):
        s = re.search(r"\.sgpr_spill_count:\s+(\d+)", m.group(2))
        v = re.search(r"\.vgpr_spill_count:\s+(\d+)", m.group(2))
        out[m.group(1)] = (int(s.group(1)) if s else -1, int(v.group(1)) if v else -1)
    return out


def count(body):
    idx = [i for i, s in enumerate(body) if s.startswith("v_mfma")]
    loop = body[idx[0]:idx[-1] + 1]
    c = dict(instr=len(loop), mfma=0, valu=0, lane=0, scratch=0, salu=0, branch=0, dma=0)
    for s in loop:
        op = s.split()[0]
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op in ("v_readlane_b32", "v_writelane_b32"):
            c["lane"] += 1
        elif op.startswith("scratch_"):
            c["scratch"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
        elif op.startswith(("s_cbranch", "s_branch")):
            c["branch"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        elif op.startswith("global_load_lds") or (op.startswith("buffer_load") and " lds" in s):
            c["dma"] += 1
    return c


def main(paths):
    print("%-64s %6s %5s %5s %5s %7s %5s %6s %4s %11s %11s" % ("kernel", "instr", "MFMA", "VALU", "lane", "scratch", "SALU", "branch", "DMA",
                                                        "sgpr_spill", "vgpr_spill"))
    for path in paths:
        ks, sp = kernels(path), spills(path)
        names = demangle(list(ks))
        for k, body in ks.items():
            c = count(body)
            short = re.sub(r"^void ss::gemm_pp_kernel|\(.*$", "", names[k])
            print("%-64s %6d %5d %5d %5d %7d %5d %6d %4d %11d %11d" % (short, c["instr"], c["mfma"], c["valu"], c["lane"], c["scratch"], c["salu"],
                                                               c["branch"], c["dma"], *sp.get(k, (-1, -1))))


if __name__ == "__main__":
    main(sys.argv[1:])
