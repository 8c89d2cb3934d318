"""Golden picture for a CPU test that used to read the reference tree at test time, produced by the REAL reference.

    python oracle/make_golden_host_refs.py       (build container only: reads the reference tree, SEEDSTORY_REFERENCE_ROOT)

``tests/golden/add_subtitle_ref.npy`` — the picture the reference's ``add_subtitle`` (``src/inference/gen_george.py``,
lifted out of its script: its module-level code loads models) draws for the image and caption of
``tests/test_story_cpu.py::test_add_subtitle_matches_reference_rendering``; uint8 [200, 200, 3].  Only the output is stored.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from ref_shims import REFERENCE_ROOT  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def subtitle_case():
    """The image and caption of tests/test_story_cpu.py::test_add_subtitle_matches_reference_rendering."""
    from PIL import Image
    img = Image.fromarray((np.arange(120 * 200 * 3) % 251).astype(np.uint8).reshape(120, 200, 3))
    return img, "George climbed the tree and waved at the man with the yellow hat."


def main():
    src = open(os.path.join(REFERENCE_ROOT, "src", "inference", "gen_george.py")).read()
    start = src.index("def add_subtitle(")
    end = src.index("\nfor j in range(len(image_paths))", start)
    ns = {}
    exec("from PIL import Image, ImageDraw, ImageFont\n" + src[start:end], ns)
    img, text = subtitle_case()
    out = np.asarray(ns["add_subtitle"](img, text))
    assert out.shape == (200, 200, 3) and out.dtype == np.uint8
    np.save(os.path.join(GOLDEN, "add_subtitle_ref.npy"), out)
    print("wrote tests/golden/add_subtitle_ref.npy")


if __name__ == "__main__":
    main()
