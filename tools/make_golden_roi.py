"""Writes tests/golden/roi/nms3d_ref.npz: the outputs of the REFERENCE's own nms_3d (models/model_rpointnet.py:436-466) on the seeded cases of
tests/roi_ref.py: NMS_CASES.

    python tools/make_golden_roi.py --reference /path/to/the/reference/checkout

Lines 436-466 are cut out of the reference at generation time (checked to begin with the function's signature and to end with its return),
exec'd with numpy, and only inputs and outputs are stored -- nothing of the source, as with oracle/Makefile: slices.  The generator asserts
what the cases are there for: pairwise distinct scores per scene, float32 throughout, int32 out, and that both exits of the loop occur
(output full; candidates exhausted)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import roi_ref as RR  # noqa: E402

FIRST, LAST = 436, 466


def reference_nms_3d(ref_root):
    lines = open(os.path.join(ref_root, "models", "model_rpointnet.py")).read().split("\n")[FIRST - 1:LAST]
    assert lines[0].startswith("def nms_3d(boxes, scores, pre_nms_limit, max_output_size"), lines[0]
    assert lines[-1].strip() == "return selected_indices", lines[-1]
    scope = {"np": np}
    exec("\n".join(lines), scope)
    return scope["nms_3d"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GSPN_REFERENCE"), help="checkout of the reference (or GSPN_REFERENCE)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "roi", "nms3d_ref.npz"))
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or GSPN_REFERENCE) is required")
    nms = reference_nms_3d(a.reference)
    store, full, exhausted = {}, 0, 0
    for name in RR.NMS_CASES:
        boxes, scores, pre, m, thr, sthr = RR.nms_case(name)
        bx, sc = boxes.numpy(), scores.numpy()
        assert bx.dtype == np.float32 and sc.dtype == np.float32
        for row in sc:
            assert len(np.unique(row)) == len(row), "scores of a scene must be pairwise distinct (the reference's argsort is not stable)"
        sel = nms(bx, sc, pre, m, thr, sthr)
        assert sel.dtype == np.int32 and sel.shape == (bx.shape[0], m)
        picks = (sel >= 0).sum(1)
        full += int((picks == m).sum())
        exhausted += int((picks < m).sum())
        print("%-26s picks per scene %s of %d, distinct %s" % (name, picks.tolist(), m, [len(np.unique(r[r >= 0])) for r in sel]))
        store[name + "/boxes"], store[name + "/scores"], store[name + "/selected"] = bx, sc, sel
        store[name + "/args"] = np.array([pre, m, thr, sthr], dtype=np.float64)
    assert full > 0 and exhausted > 0, "both exits of the reference's loop must occur"
    np.savez_compressed(a.out, **store)
    print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
