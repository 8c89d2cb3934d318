"""Which kernels serve ss_gemv / ss_gemv_batched: one call per case over a fixed grid of dtypes, sequence counts, shapes,
prologues / epilogues and tuning knobs, with a non-GEMV kernel between cases so a kernel trace can be cut per case.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o trace -- python tools/gemv_launch_table.py --cases DIR/cases.json
  python tools/gemv_launch_table.py --reduce DIR/cases.json TRACE.csv OUT.json

The first command runs the grid (no other tracing, no counters); the second joins the case list with the trace and writes per
case the kernels' names, workgroups, workgroup size and LDS bytes as the trace reports them (static LDS only).
tests/golden/gemv_launches.json is that output for the library BEFORE the launch-plan refactor of ss_gemv.hip;
test_gemv_plan_matches_recorded_launches holds ss_gemv_plan to it on a CPU machine.  tools/gemv_hash.py walks the same grid
and hashes the outputs.  quant_grid() is the grid of the quantised calls (ss_gemv_w8 / ss_gemv_mx4, cases with a "fmt" key):
run() feeds them codes and scales from seeded CPU generators, never from the library's own quantisers."""
import csv
import json
import os
import re
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in ("seed-story_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

DTYPES = ["bf16", "fp16", "fp32"]
NBS = [1, 2, 3, 4, 5, 8, 16]
# W rows x K: the five LLaMA-7B projections of tools/gemv_bench.py (gate|up as its 22016 stacked rows), then the odd ones
SHAPES = [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008), (32066, 4096), (1000, 1664), (100, 512), (33, 8), (37, 4104)]
VARIANTS = ["plain", "norm", "bias+res", "silu", "norm+silu"]          # SiLU pairs: rows [gate; up], legal when the row count is even
KNOB_SETS = [{}, {"gemv_mfma_min_nb": 1}, {"gemv_mfma_generic": 1}, {"gemv_mfma_long": 0}, {"gemv_force_lds": 1}, {"gemm_f32_split": 1}]
# the shapes of test_gemv_multi_tile_bound (tests/test_kernel_edges_gpu.py): every workgroup / wave walks several tiles or groups
EDGE_KNOBS = {"gemv_mfma_blocks": 2, "gemv_max_blocks": 1}
EDGE_SHAPES = [(100, 256), (37, 4096), (40, 11008)]
EDGE_NBS = [1, 4, 8]
EDGE_SILU_ROWS = [48, 80]                               # I = 24: one tile per workgroup; I = 40: two on the first


def grid():
    """-> dicts {dtype, nb, rows, K, variant, knobs}; `rows` = rows of W (SiLU: 2 I)"""
    for dtype in DTYPES:
        for knobs in KNOB_SETS:
            for rows, K in SHAPES:
                for nb in NBS:
                    for v in VARIANTS:
                        if "silu" in v and rows % 2:
                            continue
                        yield dict(dtype=dtype, nb=nb, rows=rows, K=K, variant=v, knobs=knobs)


def edge_grid():
    for dtype in DTYPES:
        for rows, K in EDGE_SHAPES:
            for nb in EDGE_NBS:
                for v in ("plain", "bias+res", "norm"):
                    yield dict(dtype=dtype, nb=nb, rows=rows, K=K, variant=v, knobs=EDGE_KNOBS)
                for rows_silu in EDGE_SILU_ROWS:
                    yield dict(dtype=dtype, nb=nb, rows=rows_silu, K=K, variant="silu", knobs=EDGE_KNOBS)
    for v in ("plain", "bias+res"):
        yield dict(dtype="fp32", nb=8, rows=37, K=4104, variant=v, knobs=dict(EDGE_KNOBS, gemm_f32_split=1))


# kernels no knob set of the grid above reaches: the dot-product kernels at 3 / 4 sequences and every NIT of the 16-bit types
# (the MFMA forms switched off), the non-temporal instantiations of the exact MFMA kernels
COVER_SHAPES = [(100, 512), (100, 1000), (1000, 1664), (64, 4096), (48, 11008)]
COVER_KNOBS = [{"gemv_mfma_min_nb": 17, "gemv_x_reg_packs": 32}, {"gemv_mfma_nt": 1}]


def coverage_grid():
    for dtype in DTYPES:
        for knobs in COVER_KNOBS:
            for rows, K in COVER_SHAPES:
                for nb in (1, 2, 3, 4, 8):
                    for v in ("plain", "norm", "silu"):
                        yield dict(dtype=dtype, nb=nb, rows=rows, K=K, variant=v, knobs=knobs)


# the quantised calls: the five LLaMA-7B projections + the four small shapes of tests/test_gemv_w8_gpu.py / test_gemv_mx4_gpu.py
# (the partial last load, a partial wave slice, the 16-step loop with a partial row tile, the packed loop with fp8's tail and
# MXFP4's dead slot); an odd row count gains a row for the SiLU pair; no RMSNorm prologue at K = 11008 (the call refuses it)
Q_SMALL = {"fp8": [(33, 16), (100, 272), (37, 4096), (40, 11008)], "mxfp4": [(33, 32), (100, 288), (37, 4096), (40, 11008)]}
Q_NBS = [1, 2, 3, 8, 16]
Q_KNOB_SETS = [{}, {"gemv_mfma_generic": 1}, EDGE_KNOBS]


def quant_grid():
    """-> dicts {fmt, dtype, nb, rows, K, variant, knobs}"""
    for fmt, small in Q_SMALL.items():
        for dtype in DTYPES[:2]:
            for knobs in Q_KNOB_SETS:
                for rows, K in SHAPES[:5] + small:
                    for nb in Q_NBS:
                        for v in VARIANTS:
                            if "norm" in v and K == 11008:
                                continue
                            yield dict(fmt=fmt, dtype=dtype, nb=nb, rows=rows + rows % 2 if "silu" in v else rows, K=K, variant=v, knobs=knobs)


def seeded_bytes(seed, n):
    """n bytes, each a pure function of (seed, index) (oracle/synth.py's generator), filled chunk by chunk"""
    import numpy as np
    import synth
    out = np.empty(n, dtype=np.uint8)
    for s in range(0, n, 1 << 23):
        m = min(1 << 23, n - s)
        out[s:s + m] = np.floor(synth.uniform01(seed, m, start=s) * 256.0)
    return out


def quant_planes(nel, nrows):
    """CPU planes the quantised cases cut their weights from: every e4m3 code but the two NaNs (0x7f, 0xff -> 0x7e, 0xfe) with
    fp32 row scales in [0.001, 0.004); e2m1 code pairs with e8m0 scale bytes 127 + X, X in [-13, 7] (triangular around -6: the
    range of the contract skewed low, so that fp16 outputs stay finite)"""
    import numpy as np
    import torch
    import synth
    q8 = seeded_bytes(201, nel)
    q8[(q8 & 0x7f) == 0x7f] ^= 1
    sb = seeded_bytes(203, nel // 32).astype(np.int64)
    X = np.clip(((sb & 15) + (sb >> 4) - 15) * 13 // 15 - 6, -13, 13)
    return {"q8": torch.from_numpy(q8), "s8": synth.uniform(202, (nrows,), 0.001, 0.004),
            "q4": torch.from_numpy(seeded_bytes(204, nel // 2)), "s4": torch.from_numpy((127 + X).astype(np.uint8))}


def run(cases, on_case):
    """one ops.gemv (nb 1) / ops.gemv_batched call per case into a guarded output; on_case(index, case, guarded output) follows,
    then a non-GEMV kernel"""
    import torch
    import kernel_check as KC
    import synth
    from seedstory import _lib, ops
    dev = "cuda:0"
    TD = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
    cases = list(cases)
    nel = max(c["rows"] * c["K"] for c in cases)
    kmax = max(c["K"] for c in cases)
    nmax = max(c["rows"] for c in cases)
    base = {"w": synth.normal_like(101, (nel,), std=0.02), "x": synth.normal_like(102, (16, kmax), std=1.0),
            "g": synth.normal_like(103, (kmax,), std=0.1, mean=1.0), "b": synth.normal_like(104, (nmax,), std=0.5),
            "r": synth.normal_like(105, (16, nmax), std=1.0)}
    qp = {}
    if any("fmt" in c for c in cases):
        qp = {k: v.to(dev) for k, v in quant_planes(max(c["rows"] * c["K"] for c in cases if "fmt" in c), nmax).items()}
    marker = torch.zeros(64, device=dev)
    cur = None
    for idx, c in enumerate(cases):
        if cur != c["dtype"]:
            cur = c["dtype"]
            t = {k: v.to(TD[cur]).to(dev) for k, v in base.items()}
        rows, K, nb, v = c["rows"], c["K"], c["nb"], c["variant"]
        silu = "silu" in v
        N = rows // 2 if silu else rows
        fmt = c.get("fmt")
        if fmt == "fp8":
            w = (qp["q8"][:rows * K].view(rows, K), qp["s8"][:rows])
        elif fmt == "mxfp4":
            w = (qp["q4"][:rows * K // 2].view(rows, K // 2), qp["s4"][:rows * K // 32].view(rows, K // 32))
        else:
            w = t["w"][:rows * K].view(rows, K)
        x = t["x"][:nb, :K].contiguous()
        kw = dict(norm_w=t["g"][:K].contiguous() if "norm" in v else None, eps=1e-5, silu_mul=silu)
        if v == "bias+res":
            kw.update(bias=t["b"][:N].contiguous(), residual=t["r"][:nb, :N].contiguous())
        g = KC.GuardedOut(nb, N, TD[cur], device=dev)
        old = {k: _lib.get_tuning(k) for k in c["knobs"]}
        for k, val in c["knobs"].items():
            _lib.set_tuning(k, val)
        torch.cuda.synchronize()
        marker.add_(1.0)                                   # the cut between two cases' GEMV kernels
        try:
            if fmt:
                (ops.gemv_w8 if fmt == "fp8" else ops.gemv_mx4)(*w, x, out=g.out, **kw)
            elif nb == 1:
                ops.gemv(w, x[0], out=g.view(N), **kw)
            else:
                ops.gemv_batched(w, x, out=g.out, **kw)
        finally:
            for k, val in old.items():
                _lib.set_tuning(k, val)
        on_case(idx, c, g)
    marker.add_(1.0)
    torch.cuda.synchronize()


def kernel_name(raw):
    """'void ss::gemv_kernel<ss::bf16_t, 8, 2, 1>(ss::GemvArgs)' -> 'gemv_kernel<bf16_t,8,2,1>'"""
    s = re.sub(r"\s*\[clone.*\]$", "", raw.strip()).replace(".kd", "")
    s = re.sub(r"\(bool\)(1|true)", "true", re.sub(r"\(bool\)(0|false)", "false", s)).replace("(int)", "")
    if s.endswith(")"):
        s = s[:s.rindex("(")]                              # the argument list (no nested parentheses)
    return s.replace("void ", "").replace("ss::", "").replace(" ", "")


def reduce(cases_path, trace_path, out_path):
    cases = json.load(open(cases_path))
    rows = list(csv.DictReader(open(trace_path, newline="")))
    col = lambda *names: next(n for n in names if n in rows[0])       # noqa: E731
    c_name, c_start = col("Kernel_Name"), col("Start_Timestamp")
    c_lds = col("LDS_Block_Size", "Group_Segment_Size", "LDS_Block_Size_v")
    c_wg, c_grid = col("Workgroup_Size_X", "Workgroup_Size"), col("Grid_Size_X", "Grid_Size")
    rows.sort(key=lambda r: int(r[c_start]))
    runs, inside = [], False
    for r in rows:
        if "gemv" not in r[c_name]:
            inside = False
            continue
        if not inside:
            runs.append([])
            inside = True
        wg = int(r[c_wg])
        runs[-1].append({"kernel": kernel_name(r[c_name]), "workgroups": int(r[c_grid]) // wg, "threads": wg, "lds": int(r[c_lds])})
    assert len(runs) == len(cases), "the trace has %d runs of GEMV kernels for %d cases" % (len(runs), len(cases))
    # compact (the file is a committed fixture): one line per (dtypes, rows, K, variant) holding, per sequence count of NBS,
    # [launches under knob set 0, {knob set: launches where they differ}]; bf16 and fp16 share a line where their records
    # differ only in the kernels' type argument (written T16)
    t16 = lambda name: name.replace("bf16_t", "T16").replace("f16_t", "T16")       # noqa: E731
    kernels = sorted({t16(l["kernel"]) for r in runs for l in r})
    knobsets = []
    for c in cases:
        if c["knobs"] not in knobsets:
            knobsets.append(c["knobs"])
    table = {}
    for c, launches in zip(cases, runs):
        per_nb = table.setdefault((c["rows"], c["K"], c["variant"]), {}).setdefault(c["dtype"], {})
        per_nb.setdefault(c["nb"], {})[knobsets.index(c["knobs"])] = [[kernels.index(t16(l["kernel"])), l["workgroups"], l["threads"], l["lds"]]
                                                                      for l in launches]
    lines = []
    for (rows_w, K, variant), by_dtype in table.items():
        groups = []
        for dtype, per_nb in by_dtype.items():
            entry = [[per_nb[nb][0], {str(ks): l for ks, l in per_nb[nb].items() if ks and l != per_nb[nb][0]}] for nb in NBS]
            same = [g for g in groups if g[1] == entry]
            if same:
                same[0][0].append(dtype)
            else:
                groups.append(([dtype], entry))
        for dtypes, entry in groups:
            lines.append("  %s: %s" % (json.dumps("%s %d %d %s" % ("|".join(dtypes), rows_w, K, variant)), json.dumps(entry, separators=(",", ":"))))
    head = {"lds": "the trace's %s column: the kernel's STATIC LDS in 512-byte granules; the dynamic request of a launch is not "
                   "in the trace" % c_lds, "kernels": kernels, "knob_sets": knobsets, "nbs": NBS,
            "cases": "'dtypes rows-of-W K variant' -> per entry of nbs [launches under knob set 0, {knob set: launches where they "
                     "differ}]; a launch is [kernel, workgroups, threads, lds]; T16 in a kernel's name is the line's dtype"}
    with open(out_path, "w") as f:
        f.write("{" + ",\n ".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in head.items()))
        f.write(',\n "table": {\n' + ",\n".join(lines) + "\n }}\n")
    print("%d cases, %d launches -> %s" % (len(cases), sum(len(r) for r in runs), out_path))


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--reduce":
        reduce(*sys.argv[2:])
    elif len(sys.argv) == 3 and sys.argv[1] == "--cases":
        cs = list(grid())
        run(cs, lambda i, c, g: None)
        json.dump(cs, open(sys.argv[2], "w"))
        print("%d cases" % len(cs))
    else:
        sys.exit(__doc__)
