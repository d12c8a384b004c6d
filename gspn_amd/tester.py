"""The reference's test.py on the device: from a checkpoint and a validation cache to the benchmark's prediction and ground-truth files and
an AP figure -- the loop of test.py:116-206 over a train.DeviceDataset, chained from rpointnet_inference, predict.scene_predictions,
write_predictions / write_ground_truth and evaluate.InstanceAP.

The reference tests one scene at a time (test.py:213).  Here a scene alone leaves most of the card idle (FPS runs one workgroup per scene,
DESIGN.md 8), so Tester runs batch_size scenes per step.  Nothing of a scene's result may then depend on the batch it sits in: the proposal
net runs with z = cmean, batch norm uses the moving statistics, NMS is per scene, and the two crop draws take a seed per scene --
seed + 2 * scene number for the first crop, + 1 for the second (rpointnet_inference's scene_seeds, gspn_sample_points_in_boxes_seeds).
Given the same values in its boxes a scene draws the same crops in every batch and slot.  The network's outputs themselves are not
promised bit-equal across batch sizes: the GEMM launch plans differ with the row count.

Nothing reads a value back to the host between the batch assembly and the cloned outputs; the host IO of run() works on the clones.
No CPU fallback."""
import os

import torch

from . import tf_util
from .evaluate import _FIELDS, InstanceAP, classes_from_label_ids, instance_match, instance_overlaps, write_result_file
from .predict import (SCANNET_LABEL_MAP, mean_iou, scene_predictions, semantic_iou_counts, write_ground_truth, write_predictions)
from .train import DeviceDataset, restore_variables

__all__ = ["Tester", "RESULT_FILE"]

RESULT_FILE = "semantic_instance_evaluation.txt"          # test.py:222
_LIFT_KEYS = ("detections", "rpointnet_mask_selected", "pc_coord_cropped_final_unnormalized", "pc_seed", "fb_prob", "sem_class_logits")


class _Capture:
    """one captured step: the graph, the valid-instance index it reads and the tensors it leaves"""
    __slots__ = ("graph", "valid", "out")


class Tester:
    """test.py's loop.  config: an rpointnet.Config whose NUM_SAMPLE, NUM_CATEGORY, SPN_* and DETECTION_* are the run's; NUM_GROUP,
    NUM_POINT and NUM_POINT_INS are set here from the data (test.py:45) and BATCH_SIZE to batch_size.  data: a train.DeviceDataset built
    with is_augment=False, permute_points=False (test.py:44).  scans: one name per scene (default scene_%04d), the stems of the files.
    seed: seeds the variables' initial values (a restore overwrites them) and the crops: scene k draws with seed + 2 * k and
    seed + 2 * k + 1.  fused_crop as in rpointnet_inference; sem_conf_th, fb_conf_th, mask_th, label_map as in scene_predictions
    (test.py:137-139, :136), label_map with one entry per category; vote_th: the segment vote's threshold in [0, 1), read by run_vertices for
    a scan that brings 'segments' and by nothing else; mask_nms_th: None, or the IoU in [0, 1) above which run_vertices suppresses a
    per-vertex mask that copies an earlier one of its label; run() and the captured predict step never read it.
    min_component (an int >= 1, or None) and min_component_share (in [0, 1]): run_vertices drops the components of a mask that are smaller
    than that many vertices or than that share of the mask's largest, for a scan that brings 'faces' (DESIGN.md 4.25); nothing else reads them.
    max_hole (an int >= 0, or None) and max_hole_share (in [0, 1]): run_vertices fills the gaps of at most that many vertices, and at most
    that share of the mask's set vertices, that a mask encloses on the mesh, for a scan that brings 'faces' (DESIGN.md 4.26); nothing else reads them.

    The variables are created by one rpointnet_inference pass over the first batch, in the reference's order.
    captured=True: rpointnet_inference, scene_predictions, the AP counts and the semantic IoU counts replay from one graph.CapturedStep.
    The batch, the geometry, the scene seeds and the valid-instance index are prepared outside it into buffers it reads; it is captured
    once per number of valid instances of a batch (the instance encoder's shapes depend on it; at most max_captures graphs are kept).
    Every variable, the moving statistics included, is left as it was: nothing here runs in training mode."""

    def __init__(self, config, data, scans=None, batch_size=1, seed=0, captured=True, fused_crop=False, sem_conf_th=0.01, fb_conf_th=0.01,
                 mask_th=0.4, label_map=SCANNET_LABEL_MAP, max_captures=8, vote_th=0.5, mask_nms_th=None, min_component=None,
                 min_component_share=0.0, max_hole=None, max_hole_share=1.0):
        if not isinstance(data, DeviceDataset):
            raise TypeError("Tester: data must be a train.DeviceDataset")
        if data.is_augment or data.permute_points:
            raise ValueError("Tester: the dataset must be built with is_augment=False, permute_points=False (test.py:44)")
        self.b = int(batch_size)
        if self.b < 1:
            raise ValueError("Tester: batch_size must be positive, got %d" % self.b)
        self.scans = ["scene_%04d" % k for k in range(len(data))] if scans is None else [str(s) for s in scans]
        if len(self.scans) != len(data) or len(set(self.scans)) != len(self.scans):
            raise ValueError("Tester: scans must hold one name per scene, %d different ones, got %d" % (len(data), len(self.scans)))
        self.label_map = tuple(int(v) for v in (label_map.tolist() if hasattr(label_map, "tolist") else label_map))
        if len(self.label_map) != int(config.NUM_CATEGORY):
            raise ValueError("Tester: label_map must have one entry per category, %d, got %d" % (config.NUM_CATEGORY, len(self.label_map)))
        self.cfg, self.data = config, data
        config.NUM_GROUP, config.NUM_POINT, config.NUM_POINT_INS = data.ngroup, data.pc.shape[1], data.pc_ins.shape[2]          # test.py:45
        config.BATCH_SIZE = self.b
        self.seed, self.captured, self.fused_crop, self.max_captures = int(seed), bool(captured), bool(fused_crop), int(max_captures)
        self.thresholds = dict(sem_conf_th=float(sem_conf_th), fb_conf_th=float(fb_conf_th), mask_th=float(mask_th))
        self.vote_th = float(vote_th)                # run_vertices alone: the segment vote of a scan that brings 'segments' 
        if not 0.0 <= self.vote_th < 1.0:
            raise ValueError("Tester: vote_th must lie in [0, 1), got %r" % self.vote_th)
        self.mask_nms_th = None if mask_nms_th is None else float(mask_nms_th)      # run_vertices alone: mask NMS on every scan
        if self.mask_nms_th is not None and not 0.0 <= self.mask_nms_th < 1.0:
            raise ValueError("Tester: mask_nms_th must lie in [0, 1), got %r" % self.mask_nms_th)
        self.min_component, self.min_component_share = None, 0.0                   # run_vertices alone: a scan that brings 'faces' 
        if min_component is not None:
            from ._args import _parameters
            self.min_component, self.min_component_share = _parameters(min_component, min_component_share, "Tester")
        self.max_hole, self.max_hole_share = None, 1.0                             # run_vertices alone: a scan that brings 'faces' 
        if max_hole is not None:
            from ._args import _hole_parameters
            self.max_hole, self.max_hole_share = _hole_parameters(max_hole, max_hole_share, "Tester")
        self.dev = data.pc.device
        self.store = tf_util.set_variable_store(tf_util.VariableStore(device=self.dev, seed=self.seed))

        # persistent inputs of the step
        self.buf = data.empty_batch(self.b)
        self.scene_idx = torch.zeros(self.b, dtype=torch.int32, device=self.dev)
        self.scene_seeds = torch.zeros(self.b, dtype=torch.int64, device=self.dev)
        self._batch_seed = torch.zeros(1, dtype=torch.int64, device=self.dev)       # gspn_batch_assemble's: not read without permutation and augmentation
        self.geo = None
        self._captures = {}
        self._metric = InstanceAP(int(config.NUM_CATEGORY), label_map=self.label_map)          # its thresholds and minimum region size

        slots = self._assemble(list(range(min(self.b, len(data)))))
        self._step(self._geometry(), self._valid_index(slots))

    # ---- the parts of a step ----
    def _assemble(self, idx):
        """get_batch (test.py:75-94) into the persistent buffers, a short batch filled by repeating its last scene -> the scene of each slot"""
        idx = [int(k) for k in idx]
        if not 1 <= len(idx) <= self.b or min(idx) < 0 or max(idx) >= len(self.data):
            raise ValueError("Tester: 1 to %d scene numbers in [0, %d) expected, got %r" % (self.b, len(self.data), idx))
        slots = idx + [idx[-1]] * (self.b - len(idx))
        self.scene_idx.copy_(torch.tensor(slots, dtype=torch.int32))
        self.scene_seeds.copy_(torch.tensor([self.seed + 2 * k for k in slots], dtype=torch.int64))
        self.data.batch(self.scene_idx, self._batch_seed, out=self.buf)
        return slots

    def _valid_index(self, slots):
        """shape_proposal.valid_instances(group_indicator) from the host's copy of the group counts: no read-back"""
        rows = [(s, j) for s, k in enumerate(slots) for j in range(min(self.data.counts_host[k], self.data.ngroup))]
        return torch.tensor(rows, dtype=torch.int64).reshape(-1, 2).to(self.dev)

    def _geometry(self):
        from .shape_proposal import SPN_SEM_POINTS
        from .spn_trunks import spn_geometry
        return spn_geometry(self.buf["pc"], int(self.cfg.NUM_SAMPLE), SPN_SEM_POINTS, True, points=self.buf["color"])

    def _step(self, geo, valid):
        """the buffers -> {'pred': scene_predictions', 'ap_counts': instance_match's with the rows' classes and confidences,
        'iou_inter', 'iou_union' (B, C - 1) int64: the semantic IoU counts of each slot, 'lift': the six tensors of the batch that
        lift.scan_predictions reads}"""
        from .inference import rpointnet_inference
        u, cfg = self.buf, self.cfg
        tf_util.set_variable_store(self.store)
        with torch.no_grad():
            ep = rpointnet_inference(u["pc"], u["color"], u["pc_ins"], u["group_label"], u["group_indicator"], u["seg_label"], u["bbox_ins"], cfg,
                                     False, None, geometry=geo, valid_idx=valid, scene_seeds=self.scene_seeds, fused_crop=self.fused_crop)
            pred = scene_predictions(ep, u["pc"], label_map=self.label_map, **self.thresholds)
            pred_class = classes_from_label_ids(pred["label_ids"], self.label_map)
            inter, void_count, pred_count, gt_count = instance_overlaps(pred["masks"], pred_class, u["seg_label"], u["group_label"],
                                                                        int(cfg.NUM_CATEGORY), int(cfg.NUM_GROUP))
            n_true, n_false, hard_fn, n_gt, n_pred = instance_match(inter, void_count, pred_count, pred_class, pred["confidence"], pred["count"],
                                                                    gt_count, self._metric.overlaps, self._metric.min_region_size)
            counts = {"n_true": n_true, "n_false": n_false, "hard_fn": hard_fn, "n_gt": n_gt, "n_pred": n_pred, "pred_class": pred_class,
                      "confidence": pred["confidence"]}
            # per slot, so that the filled slots of a short batch can be left out (train.py:365-368 on the whole scene's points)
            logits = ep["sem_class_logits"]
            per_slot = [semantic_iou_counts(logits[s], u["seg_label"][s]) for s in range(self.b)]
            # what lift.scan_predictions reads of a batch, as the step leaves it: run_vertices lifts each scene behind the step
            lift = {k: ep[k] for k in _LIFT_KEYS}
            return {"pred": pred, "ap_counts": counts, "iou_inter": torch.stack([p[0] for p in per_slot]),
                    "iou_union": torch.stack([p[1] for p in per_slot]), "lift": lift}

    def _capture(self, valid):
        from .graph import CapturedStep
        cap = _Capture()
        cap.valid = valid.clone()
        st = {}

        def step():
            st["out"] = self._step(self.geo, cap.valid)

        cap.graph = CapturedStep(step)
        cap.out = st["out"]
        self._captures[valid.shape[0]] = cap
        while len(self._captures) > self.max_captures:
            self._captures.pop(next(iter(self._captures)))
        return cap

    # ---- the public calls ----
    def restore(self, path, scope=None):
        """test.py:62 through train.restore_variables: reads a file of Trainer.save (or save_variables) as it is, the optimiser's and the
        generators' entries ignored.  scope=None: every variable of the inference graph; one that the checkpoint lacks raises KeyError
        naming it -- for a checkpoint of SPN training alone, a head variable -- and nothing is written.  scope='shape_proposal_net'
        restores that part alone.  Variables are written in place, so captured graphs stay valid."""
        ckpt = restore_variables(path, self.store, scope)
        print('RESTORE MODEL FROM ' + str(path), flush=True)
        return ckpt

    def _outputs(self, idx):
        """the step on the scenes idx -> _step's dict itself, not cloned: it holds until the next step"""
        from .graph import copy_into
        slots = self._assemble(idx)
        geo, valid = self._geometry(), self._valid_index(slots)
        if self.captured:
            self.geo = geo if self.geo is None else copy_into(self.geo, geo)
            cap = self._captures.get(valid.shape[0])
            if cap is None:
                cap = self._capture(valid)
            else:
                cap.valid.copy_(valid)
            cap.graph.replay()
            out = cap.out
        else:
            out = self._step(geo, valid)
        return out

    def predict(self, idx):
        """idx: 1 to batch_size scene numbers -> (pred, batch), clones cut to len(idx) scenes.  pred: scene_predictions' dict.  batch: the
        ten tensors of DeviceDataset.batch plus 'ap_counts' (what InstanceAP.add_counts takes) and 'iou_inter', 'iou_union'
        (len(idx), C - 1) int64, the semantic IoU counts of each scene."""
        out = self._outputs(idx)
        k = len(idx)
        cut = lambda t: t[:k].clone()
        batch = {name: cut(t) for name, t in self.buf.items()}
        batch["ap_counts"] = {name: cut(out["ap_counts"][name]) for name in _FIELDS}
        batch["iou_inter"], batch["iou_union"] = cut(out["iou_inter"]), cut(out["iou_union"])
        return {name: cut(t) for name, t in out["pred"].items()}, batch

    def run(self, out_dir=None, evaluate=True):
        """test.py:209-222 over every scene once, in order.  out_dir: <out_dir>/gt/<scan>.txt (gen_gt, :116-129) and
        <out_dir>/pred/<scan>.txt with pred_mask/ (output_prediction, :131-206) are written.  evaluate: the AP counts and the semantic IoU
        counts of the real scenes are accumulated on the device -> InstanceAP.compute()'s dict plus 'iou' (train.py:385-386), also written
        to <out_dir>/pred/semantic_instance_evaluation.txt (test.py:222) when there is an out_dir.  evaluate=False -> None."""
        metric = InstanceAP(int(self.cfg.NUM_CATEGORY), label_map=self.label_map) if evaluate else None
        c = int(self.cfg.NUM_CATEGORY)
        inter = torch.zeros(c - 1, dtype=torch.int64, device=self.dev)
        union = torch.zeros(c - 1, dtype=torch.int64, device=self.dev)
        if out_dir is not None:
            gt_dir, pred_dir = os.path.join(out_dir, "gt"), os.path.join(out_dir, "pred")
            os.makedirs(gt_dir, exist_ok=True)
            os.makedirs(pred_dir, exist_ok=True)
        for lo in range(0, len(self.data), self.b):
            idx = list(range(lo, min(lo + self.b, len(self.data))))
            pred, batch = self.predict(idx)
            if evaluate:
                metric.add_counts(batch["ap_counts"])
                inter += batch["iou_inter"].sum(0)
                union += batch["iou_union"].sum(0)
            if out_dir is not None:
                for s, k in enumerate(idx):
                    write_ground_truth(gt_dir, self.scans[k], batch["seg_label"][s], batch["group_label"][s], self.label_map)
                    write_predictions(pred_dir, self.scans[k], pred, s)
        if not evaluate:
            return None
        result = metric.compute()
        result["iou"] = float(mean_iou(inter, union))
        if out_dir is not None:
            write_result_file(os.path.join(pred_dir, RESULT_FILE), result)
        return result

    def run_vertices(self, out_dir, vertices, evaluate=True):
        """run() at the resolution of each scan's own mesh.  vertices(k) -> {'xyz': (V, 3) float32} for scene k, the scan's
        vertices in the coordinates of the scene's points, and, for the ground truth and the evaluation, 'seg_label' and 'group_label'
        (V,) int32 in the cache's numbering (classes 0..C-1, groups from 0); numpy arrays or tensors.  A scan that also brings 'segments'
        ((V,) integers: the raw ids of its mesh's over-segmentation, data_prep.read_segments) has its masks and its semantic labels
        snapped to them at the tester's vote_th: the ids are compacted, scan_predictions votes, the files and the AP come
        from the voted masks and the IoU counts from the voted labels; a scan without goes the way it always went.  With the tester's
        mask_nms_th every scan's masks then pass mask NMS: a suppressed mask is empty, so it is not written and not counted.
        With the tester's min_component a scan that brings 'faces' ((F, 3) integers: its mesh's triangles, io_util.read_ply_faces) has the
        small components of its masks dropped behind the vote and before mask NMS; a scan without goes as it went.
        With the tester's max_hole such a scan has the gaps its masks enclose on the mesh filled behind that and before mask NMS.
        The scenes run batched through the same step as run(); behind it lift.scan_predictions runs eagerly once per scan, V differing from scan to scan.  out_dir:
        <out_dir>/pred_vertices/<scan>.txt with pred_mask/, one line per vertex in every mask, and, where vertices(k) has labels,
        <out_dir>/gt_vertices/<scan>.txt.  evaluate: AP per scan through InstanceAP at B = 1 and the semantic IoU counts of
        sem_class_logits[src] against the vertices' labels -> run()'s dict, also written to <out_dir>/pred_vertices/
        semantic_instance_evaluation.txt; evaluate=False -> None.  run()'s own outputs and every variable are left as they are."""
        from .lift import scan_predictions
        from .components import mesh_faces
        from .segments import compact_segments
        metric = InstanceAP(int(self.cfg.NUM_CATEGORY), label_map=self.label_map) if evaluate else None
        c = int(self.cfg.NUM_CATEGORY)
        inter = torch.zeros(c - 1, dtype=torch.int64, device=self.dev)
        union = torch.zeros(c - 1, dtype=torch.int64, device=self.dev)
        if out_dir is not None:
            gt_dir, pred_dir = os.path.join(out_dir, "gt_vertices"), os.path.join(out_dir, "pred_vertices")
            os.makedirs(gt_dir, exist_ok=True)
            os.makedirs(pred_dir, exist_ok=True)
        for lo in range(0, len(self.data), self.b):
            idx = list(range(lo, min(lo + self.b, len(self.data))))
            out = self._outputs(idx)
            for s, k in enumerate(idx):
                scan = vertices(k)
                xyz = torch.as_tensor(scan["xyz"]).to(self.dev)
                voted = {}
                if "segments" in scan:
                    raw = torch.as_tensor(scan["segments"]).to(self.dev)
                    if tuple(raw.shape) != (xyz.shape[0],):
                        raise ValueError("Tester.run_vertices: vertices(%d) must name the segment of each of its %d vertices, got %s"
                                         % (k, xyz.shape[0], tuple(raw.shape)))
                    compact, nseg = compact_segments(raw)
                    voted = dict(segments=compact, num_segments=nseg, vote_th=self.vote_th)
                cleaned = {}
                if (self.min_component is not None or self.max_hole is not None) and "faces" in scan:
                    cleaned = dict(faces=mesh_faces(scan["faces"], xyz.shape[0]))
                    if self.min_component is not None:                              # 4.25: behind the vote, before the order and mask NMS
                        cleaned.update(min_component=self.min_component, min_component_share=self.min_component_share)
                    if self.max_hole is not None:                                   # 4.26: behind the filter, before the order and mask NMS
                        cleaned.update(max_hole=self.max_hole, max_hole_share=self.max_hole_share)
                pred = scan_predictions(out["lift"], s, xyz, pc=self.buf["pc"], label_map=self.label_map, **self.thresholds, **voted,
                                        mask_nms_th=self.mask_nms_th, **cleaned)        # 4.24: behind the vote, on the rows in output order
                labelled = "seg_label" in scan and "group_label" in scan
                if evaluate and not labelled:
                    raise ValueError("Tester.run_vertices: vertices(%d) has no 'seg_label' and 'group_label' to evaluate against" % k)
                if labelled:
                    seg = torch.as_tensor(scan["seg_label"]).to(self.dev).int().contiguous()
                    group = torch.as_tensor(scan["group_label"]).to(self.dev).int().contiguous()
                    if tuple(seg.shape) != (xyz.shape[0],) or tuple(group.shape) != (xyz.shape[0],):
                        raise ValueError("Tester.run_vertices: vertices(%d) must label each of its %d vertices, got %s and %s"
                                         % (k, xyz.shape[0], tuple(seg.shape), tuple(group.shape)))
                if evaluate:
                    metric.add_predictions(pred, seg.unsqueeze(0), group.unsqueeze(0), max(int(group.max()), 0) + 1)
                    if voted:                        # a one-hot row's first maximum is the label: the same counts entry
                        semantic_iou_counts(torch.nn.functional.one_hot(pred["sem_label"].long(), c).float(), seg, inter, union)
                    else:
                        semantic_iou_counts(out["lift"]["sem_class_logits"][s][pred["src"].long()], seg, inter, union)
                if out_dir is not None:
                    if labelled:
                        write_ground_truth(gt_dir, self.scans[k], seg, group, self.label_map)
                    write_predictions(pred_dir, self.scans[k], pred, 0)
        if not evaluate:
            return None
        result = metric.compute()
        result["iou"] = float(mean_iou(inter, union))
        if out_dir is not None:
            write_result_file(os.path.join(pred_dir, RESULT_FILE), result)
        return result
