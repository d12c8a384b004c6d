"""Writes tests/golden/detect/class_nms_ref.npz: the per-class NMS of refine_detections (models/model_rpointnet.py:855-901) with the
REFERENCE's own nms_3d (:436-466) run once per class, on the seeded cases of tests/detect_ref.py: CLASS_NMS_CASES.

    python tools/make_golden_detect.py --reference /path/to/the/reference/checkout

As tools/make_golden_roi.py: lines 436-466 are cut out of the reference at generation time, exec'd with numpy, and only inputs and outputs
are stored -- boxes, scores, class ids, the arguments and the selected rows after the intersection of :893 and the top_k of :900 -- nothing
of the source.  Here the loop over the classes, the index sets and the top_k around the reference's function are the restatement of
tests/detect_ref.py; refine_detections and unmold_segmentation themselves, TensorFlow graph code, are executed by
tools/make_golden_graph.py over the numpy stand-in tools/tf_numpy.py, which pins that loop to the reference's own lines too
(tests/golden/graph/refine_detections.npz).  The generator asserts what the cases are there for: pairwise distinct scores per scene, a scene with more
survivors than max_output_size, a class that reaches max_per_class, a zero-volume candidate that is picked again, a scene without any
candidate."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden_roi import reference_nms_3d  # noqa: E402
from tests import detect_ref as DR  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GSPN_REFERENCE"), help="checkout of the reference (or GSPN_REFERENCE)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "detect", "class_nms_ref.npz"))
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or GSPN_REFERENCE) is required")
    nms = reference_nms_3d(a.reference)
    seen = {"more_than_outputs": 0, "class_full": 0, "repicked_zero_volume": 0, "no_candidate": 0}

    def watched(boxes, scores, pre, m, thr, sthr):
        """the reference's function, looking at what it returns for one class"""
        sel = nms(boxes, scores, pre, m, thr, sthr)
        assert sel.dtype == np.int32 and sel.shape == (1, m)
        picks = sel[0][sel[0] >= 0]
        seen["class_full"] += int(len(picks) == m)
        for k in np.unique(picks):
            if (picks == k).sum() > 1:
                assert boxes[0, k, 3:].prod() < 1.2e-9
                seen["repicked_zero_volume"] += int(boxes[0, k, 3:].prod() == 0)
        return sel

    store = {}
    for name in DR.CLASS_NMS_CASES:
        boxes, scores, class_ids, per_class, m, thr = DR.class_nms_case(name)
        assert boxes.numpy().dtype == np.float32 and scores.numpy().dtype == np.float32 and class_ids.numpy().dtype == np.int32
        for row in scores.numpy():
            assert len(np.unique(row)) == len(row), "scores of a scene must be pairwise distinct (the reference's argsort is not stable)"
        sel = DR.class_nms(boxes, scores, class_ids, per_class, m, thr, nms=watched)
        survivors = [len(DR.class_nms_scene(boxes[i], scores[i], class_ids[i], per_class, boxes.shape[1], thr, nms)) for i in range(len(boxes))]
        seen["more_than_outputs"] += sum(s > m for s in survivors)
        seen["no_candidate"] += int(((class_ids > 0).sum(1) == 0).sum())
        print("%-22s survivors per scene %s, max_output_size %d" % (name, survivors, m))
        store[name + "/boxes"], store[name + "/scores"], store[name + "/class_ids"] = boxes.numpy(), scores.numpy(), class_ids.numpy()
        store[name + "/selected"] = sel.numpy()
        store[name + "/args"] = np.array([per_class, m, thr], dtype=np.float64)
    print(seen)
    assert all(v > 0 for v in seen.values()), seen
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez_compressed(a.out, **store)
    print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
