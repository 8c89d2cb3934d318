"""Compiler record of the kernels of ss_gemv.hip (no GPU needed): per kernel symbol the registers, scratch, spills, occupancy and
static LDS that hipcc reports (-Rpass-analysis=kernel-resource-usage) and the md5 of the function's body in the device assembly
(label to .Lfunc_end; lines naming __hip_cuid_ dropped, comments dropped, the function index taken out of the block labels).
  python tools/gemv_isa.py --record SRC.hip OUT.json      (SRC: an ss_gemv.hip; headers it does not sit beside come from csrc)
  python tools/gemv_isa.py --compare PARENT.json CHANGE.json OUT.txt
--compare exits 1 when a kernel of the change has more scratch, more spills or a lower occupancy than its twin."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "seed-story_amd", "csrc")
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -DSS_EXPERIMENTAL=0".split()       # the Makefile's
FIELDS = [("sgpr", r"TotalSGPRs"), ("vgpr", r"VGPRs"), ("agpr", r"AGPRs"), ("scratch", r"ScratchSize \[bytes/lane\]"),
          ("occupancy", r"Occupancy \[waves/SIMD\]"), ("sgpr_spill", r"SGPRs Spill"), ("vgpr_spill", r"VGPRs Spill"),
          ("lds", r"LDS Size \[bytes/block\]")]


def pretty(mangled):
    s = subprocess.check_output(["c++filt", mangled], text=True).strip()
    s = re.sub(r"\(bool\)(1|true)", "true", re.sub(r"\(bool\)(0|false)", "false", s)).replace("(int)", "")
    if s.endswith(")"):
        s = s[:s.rindex("(")]
    return s.replace("void ", "").replace("ss::", "").replace(" ", "")


def record(src, out_path):
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "gemv.s")
        cmd = ["/opt/rocm/bin/hipcc"] + FLAGS + ["-I", CSRC, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", src, "-o", asm]
        remarks = subprocess.run(cmd, check=True, text=True, stderr=subprocess.PIPE).stderr
        text = open(asm).read()
    kernels, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        for key, pat in FIELDS:
            m = re.search(r"remark: .*\s%s: (\d+)" % pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    out = {}
    for sym, res in kernels.items():
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(sym), text, re.S | re.M)
        if not m or ".amdhsa_kernel %s\n" % sym not in text:
            continue                                        # a device function, not a kernel
        body = [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s*;.*$", "", l)) for l in m.group(1).splitlines() if "__hip_cuid_" not in l]
        res["md5"] = hashlib.md5("\n".join(l for l in body if l.strip()).encode()).hexdigest()
        out[pretty(sym)] = res
    json.dump(out, open(out_path, "w"), indent=0, sort_keys=True)
    print("%d kernel symbols -> %s" % (len(out), out_path))


def compare(pa, pb, out_path):
    a, b = json.load(open(pa)), json.load(open(pb))
    fmt = lambda r: "/".join(str(r[k]) for k, _ in FIELDS)      # noqa: E731
    lines, worse, same = [], [], 0
    for name in sorted(set(a) | set(b)):
        ra, rb = a.get(name), b.get(name)
        if ra is None or rb is None:
            lines.append("%-58s %s" % (name, "ONLY IN THE %s" % ("CHANGE" if ra is None else "PARENT")))
            worse.append(name)
            continue
        if rb["scratch"] > ra["scratch"] or rb["vgpr_spill"] > ra["vgpr_spill"] or rb["sgpr_spill"] > ra["sgpr_spill"] or rb["occupancy"] < ra["occupancy"]:
            worse.append(name)
        same += ra["md5"] == rb["md5"]
        lines.append("%-58s %-28s %-28s %s  %s  %s" % (name, fmt(ra), fmt(rb), ra["md5"], rb["md5"], "same" if ra["md5"] == rb["md5"] else "DIFFERENT"))
    with open(out_path, "w") as f:
        f.write("# kernel  parent SGPRs/VGPRs/AGPRs/scratch B per lane/occupancy/SGPR spills/VGPR spills/static LDS B  change (same fields)  "
                "md5(parent body)  md5(change body)\n")
        f.write("\n".join(lines))
        f.write("\n# %d / %d kernel symbols (parent / change); %d bodies identical, %d differ; more scratch, more spills or lower occupancy in: %s\n"
                % (len(a), len(b), same, len(set(a) & set(b)) - same, ", ".join(worse) or "none"))
    print(open(out_path).read().splitlines()[-1])
    return 1 if worse else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--record":
        record(*sys.argv[2:])
    elif len(sys.argv) == 5 and sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
