"""Bit-for-bit record of ss_gemv / ss_gemv_batched / ss_gemv_w8 / ss_gemv_mx4: the case grid of tools/gemv_launch_table.py, the
multi-tile shapes of test_gemv_multi_tile_bound, a few cases under knobs that reach the remaining kernel instantiations
(together: every kernel of ss_gemv.hip) and the grid of the quantised calls (quant_grid: codes and scales from seeded CPU
generators); inputs from the seeded generators of oracle/synth.py, every output written into a guarded buffer
(tests/kernel_check.py) whose guards must stay untouched; one sha1 per case over the whole buffer, guards included.
  python tools/gemv_hash.py OUT.json          run with two libraries (SEEDSTORY_HIP_LIB), then
  python tools/gemv_hash.py --compare A.json B.json
The kernels have no atomics and a fixed reduction order, so two libraries that compute the same thing give equal files."""
import hashlib
import json
import sys

import gemv_launch_table as G


def main(out_path):
    hashes = []

    def on_case(i, c, g):
        msgs, _ = g.problems()
        assert not msgs, (c, msgs)
        hashes.append(hashlib.sha1(g.flat.cpu().numpy().tobytes()).hexdigest())
        if len(hashes) % 1000 == 0:
            print("%d cases" % len(hashes), flush=True)

    cases = list(G.grid()) + list(G.edge_grid()) + list(G.coverage_grid()) + list(G.quant_grid())
    G.run(cases, on_case)
    json.dump({"cases": cases, "sha1": hashes}, open(out_path, "w"))
    print("%d cases hashed -> %s" % (len(cases), out_path))


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    assert a["cases"] == b["cases"], "different case lists"
    bad = [c for c, ha, hb in zip(a["cases"], a["sha1"], b["sha1"]) if ha != hb]
    for c in bad[:20]:
        print("DIFFERENT:", json.dumps(c))
    print("%d cases, %d differ" % (len(a["cases"]), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
