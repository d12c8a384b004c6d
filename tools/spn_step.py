"""Times shape_proposal_net's two trunks (gspn_amd/spn_trunks.py) and the whole SPN training step (gspn_amd/rpointnet.py) on one GPU.

  step      one training step of shift_pred_net + sem_net (forward + backward), (a) each trunk building its own geometry inline, as
            code written against the reference's modules does, and (b) with one spn_geometry shared by both (computed inside the step)
  full_fwd  the full-feature forward (return_fullfea=True, eval, mode='inference') with the dense 3-NN of spn_geometry by one three_nn per
            level vs one three_nn_nested scan
  nn        the dense 3-NN alone: three_nn onto l1, l2, l3, l4 (four launches) vs three_nn_nested (one launch)
  spn       one full SPN training step -- rpointnet + get_loss + backward, eager, geometry computed inside the step -- at the reference's
            configuration (256 seeds, 100 groups of 512 points, 19 categories, SHRINK_BOX on), and box_shrink on its HIP kernel against the
            reference's broadcast formulation written in torch, alternating in one process, at 256 and 2048 boxes per scene
  roi       the ROI stage (gspn_amd/roi.py) per op, at the training shape (256 -> 192 -> 128 proposals, 64 ROIs x 256 points) and the inference
            shape (2048 -> 1536 -> 384, 1024 points per ROI): nms_3d on the device against the host formulation the reference runs (copy to
            the host, a numpy loop, copy back) alternating in one process, box_point_count, detection_target_gen_batch,
            mask_selection_gen_batch, and points_cropping forward + backward with --crop-channels feature channels (forward only at the
            inference shape, which has no backward)
  detect    the detection output stage (gspn_amd/detect.py) at the inference shape: refine_detections_batch on 384 ROIs per scene,
            nearest_in_sets with and without the box gate and unmold_segmentation on 100 detections x 1024 crop points, and
            unmold_segmentation as the reference states it -- the broadcast distance tensor, written in torch and chunked over the ROIs so
            that it fits -- alternating in one process; median / min / max, the inside share and the distance evaluations per launch
  heads     the two heads (gspn_amd/heads.py) with the reference's widths over --crop-channels feature channels, their first layer fused
            with the crop (crop=, the T GEMM included) against points_cropping + the materialised heads, alternating in one process: both
            heads forward + backward at the training shape (64 ROIs x 256 points), forward only at the inference shapes (classification
            head 384 x 1024, segmentation head 100 x 1024); median / min / max and the largest relative difference between the two forms
  infer     rpointnet_inference (gspn_amd/inference.py) with Config(istrain=False) -- 2048 seeds -> 1536 -> 384 ROIs x 1024 points, 100
            detections -- on freshly initialised variables (DETECTION_MIN_CONFIDENCE 0, which they never reach): the whole call and its
            stages (the same parts chained by hand with an event between them) with fused_crop off and on, alternating in one process; the
            detections per scene; and crop_mean against the reference's own form of the per-ROI probabilities (concatenate the 20 columns
            to the 1024 features, points_cropping at width 1044, split, mean), alternating, with their largest relative difference
  dataset   the instance resampling of dataset.py:107-118 (gspn_amd/dataset.py) on scenes whose instance sizes are the mix of
            tests/test_gpu_dataset.py scaled to the shape, --points-per-instance picks per instance: fps_segments (one call for the batch)
            against the loop the library offered before -- a boolean compaction and a b = 1 farthest_point_sample per instance -- and
            against instance_point_sets replayed from a captured graph, alternating in one process; the loop's FPS calls and host
            compactions, and whether the sampled rows of the two forms are equal
  predict   the prediction export stage (gspn_amd/predict.py) with Config(istrain=False)'s widths -- 100 detections x 1024 crop points, 19
            categories, 2048 seeds -- on synthetic head outputs: scene_predictions against the same arithmetic written in torch on the
            device (unmold_segmentation's (B, R, N) float tensor, a float64 matmul with the softmax table, two argsorts, the threshold),
            alternating in one process, and the stage replayed from a captured graph; whether the two orders and masks are equal and the
            largest relative difference of the confidences
  lift      predictions on a scan's own vertices (gspn_amd/lift.py) on the synthetic head outputs of `predict` -- 75 valid detections of
            100, 1024 crop points --, scene 0 of the batch: scan_predictions against scene_predictions on the scene's own points, then on
            synthetic scans of --lift-vertices vertices around the scene, with vertex_tables and gspn_lift_masks timed alone beside it,
            alternating in one process; and the same arithmetic in torch on the device in chunks of vertices (up to --lift-torch-max
            vertices, at most 5 repeats).  Call times: device events around the calls as a user makes them
  segments  the segment vote (gspn_amd/segments.py) on the masks of `lift`'s inputs -- 100 rows -- at the scene's own points and at
            --lift-vertices vertices, the segments synth.scan_segments' 0.25 m cubes: segment_vote (its own workspace, and one the caller
            holds) and segment_label_vote against the same arithmetic in torch on the device (index_add_ per row), compact_segments, and
            scan_predictions with and without segments beside lift_masks and vertex_tables, alternating in one process
  mask_nms  mask NMS (gspn_amd/mask_nms.py) on the rows scan_predictions leaves behind the segment vote for `segments`' inputs -- 100 rows
            -- at the scene's own points and at --lift-vertices vertices, as they are and with every row doubled: mask_overlaps against
            masks.float() @ masks.float().T on the device, mask_nms whole (its own workspace, and one the caller holds), and
            scan_predictions with segments with and without mask_nms_th, alternating in one process
  components  mask components (gspn_amd/components.py) on the same rows, synth.scan_faces over `segments`' instances as the mesh (a bridge
            per 1000 vertices): mask_components and component_filter (their own workspace, and one the caller holds) against iterated
            scatter_reduce(amin) over the set edges in torch on the device, and scan_predictions with segments with and without the stage
  holes     mask holes (gspn_amd/holes.py) on `components`' rows and mesh with gaps punched into the rows: hole_fill (its own workspace, and
            one the caller holds with out) beside component_filter on the same rows, and scan_predictions with segments with and without
            the stage
  evaluate the instance AP counts of one batch (gspn_amd/evaluate.py) on synthetic masks at Config(istrain=False)'s widths -- 100 rows, 100
            groups, 19 categories, the benchmark's 10 thresholds: instance_overlaps against the same counts written in torch on the device
            (masks.float() against a one-hot of seg * G + group), each alone and in front of instance_match, alternating in one process,
            and the two kernels replayed from a captured graph; whether the counts are equal
  data_prep the two computations of data_prep.py (gspn_amd/data_prep.py) at the reference's sizes, whatever --shapes says: segment_labels on
            150000 vertices against the reference's host loop (wall clock), and downsample_scans at batch 1, 2, 4, 8 over eight synthetic
            scans of 100000-200000 points down to 30000 against eight single farthest_point_sample calls, alternating in one process;
            whether the labels and the picks are equal

Prints one JSON line per (shape, measurement): median / min milliseconds over --iters timed runs after --warmup runs.
    python tools/spn_step.py --shapes 2x18000,8x32768
    python tools/spn_step.py --shapes 2x18000 --measures spn
    python tools/spn_step.py --shapes 2x18000 --measures roi
    python tools/spn_step.py --shapes 2x18000 --measures detect
    python tools/spn_step.py --shapes 2x18000 --measures heads --iters 30
    python tools/spn_step.py --shapes 2x18000 --measures infer --iters 5
    python tools/spn_step.py --shapes 2x18000 --measures train_heads --iters 10
    python tools/spn_step.py --shapes 2x18000,2x30000 --measures dataset --iters 30
    python tools/spn_step.py --shapes 2x18000 --measures predict --iters 30
    python tools/spn_step.py --shapes 1x18000 --measures lift --iters 30
    python tools/spn_step.py --shapes 1x18000 --measures segments --warmup 5 --iters 30
    python tools/spn_step.py --shapes 1x18000 --measures mask_nms --warmup 5 --iters 30
    python tools/spn_step.py --shapes 1x18000 --measures components --warmup 5 --iters 30
    python tools/spn_step.py --shapes 1x18000 --measures holes --warmup 5 --iters 30
    python tools/spn_step.py --shapes 2x18000,8x32768 --measures train --iters 20
    python tools/spn_step.py --shapes 2x18000 --measures evaluate --iters 30
    python tools/spn_step.py --shapes 1x150000 --measures data_prep --iters 9
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gspn_amd import synth, tf_util  # noqa: E402
from gspn_amd import spn_trunks as S  # noqa: E402
from gspn_amd.tf_interpolate import nested_local_maps, three_nn, three_nn_nested  # noqa: E402
from gspn_amd.tf_sampling import farthest_point_sample, gather_point  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4)}


def trunks(xyz, col, ns, nm, ncat, training, full, mode, geo):
    ep = S.shift_pred_net(xyz, col, ns, {}, 'shift_predictor', training, 0.5, return_fullfea=full, geometry=geo)
    return S.sem_net(xyz, col, nm, ncat, ep['ind_seed'], ep, 'sem_predictor', training, 0.5, return_fullfea=full, mode=mode, geometry=geo)


def box_shrink_torch(box, pc):
    """box_shrink as models/model_rpointnet.py:529-551 writes it: boxes broadcast against points, (B, S, N, 3) temporaries"""
    pc_aug, box_aug = pc.unsqueeze(1), box.unsqueeze(2)
    masks = (pc_aug >= box_aug[..., :3] - box_aug[..., 3:] / 2) & (pc_aug <= box_aug[..., :3] + box_aug[..., 3:] / 2)
    out = 1 - (masks[..., 0] & masks[..., 1] & masks[..., 2]).float().unsqueeze(-1)
    gamma = 1e4
    box_max, box_min = (pc_aug - gamma * out).amax(2), (pc_aug + gamma * out).amin(2)
    keep = (box_max - box_min > 0).all(-1, keepdim=True).float()
    return torch.cat(((box_max + box_min) / 2, box_max - box_min + 1e-3), 2) * keep


def timed_alternating(fns, warmup, iters):
    """median / min / max of each of several callables, run in turn (a, b, a, b, ...) so that clocks and neighbours hit them alike; the
    spread of the repeats is what a difference between two of them is judged against"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: {"median_ms": round(sorted(v)[len(v) // 2], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in ts.items()}


def measure_spn(a, shape, b, n, dev):
    from gspn_amd import rpointnet as RP
    from gspn_amd.spn_boxes import box_shrink
    cfg = RP.Config()
    cfg.BATCH_SIZE, cfg.NUM_POINT, cfg.SHRINK_BOX = b, n, True
    sc = {k: torch.from_numpy(v).to(dev) for k, v in
          synth.spn_batch(a.kind, b, n, cfg.NUM_GROUP, cfg.NUM_POINT_INS, cfg.NUM_CATEGORY, seed0=7).items()}
    store = tf_util.set_variable_store(tf_util.VariableStore(device=dev, seed=1))

    def step():
        for p in store.parameters():
            p.grad = None
        ep = RP.rpointnet(sc["pc"], sc["color"], sc["pc_ins"], sc["group_label"], sc["group_indicator"], sc["seg_label"], sc["bbox_ins"], cfg,
                          True, bn_decay=0.5)
        loss, _ = RP.get_loss(ep, cfg, 1.0, sc["smpw"])
        loss.backward()

    res = timed(step, a.warmup, a.iters)
    # get_loss alone (forward + gradients with respect to the network's outputs) on the detached end_points of one forward pass
    ep = RP.rpointnet(sc["pc"], sc["color"], sc["pc_ins"], sc["group_label"], sc["group_indicator"], sc["seg_label"], sc["bbox_ins"], cfg, True,
                      bn_decay=0.5)
    ep = {k: v.detach() for k, v in ep.items()}
    outs = ('fb_logits', 'pc_ins_pred', 'shift_pred_seed_4d', 'sem_class_logits', 'mean', 'log_var', 'cmean', 'clog_var')
    for k in outs:
        ep[k].requires_grad_(True)

    def loss_only():
        loss, _ = RP.get_loss(dict(ep), cfg, 1.0, sc["smpw"])
        torch.autograd.grad(loss, [ep[k] for k in outs])

    print(json.dumps({"shape": shape, "kind": a.kind, "measure": "spn", "seeds": cfg.NUM_SAMPLE, "groups": cfg.NUM_GROUP,
                      "points_per_instance": cfg.NUM_POINT_INS, "step": res, "get_loss_fwd_bwd": timed(loss_only, a.warmup, a.iters)}), flush=True)
    for s in (256, 2048):
        g = torch.Generator().manual_seed(s)
        ext = sc["pc"].amax((0, 1)).cpu()
        box = torch.cat((torch.rand(b, s, 3, generator=g) * ext, torch.rand(b, s, 3, generator=g) * 1.5 + 0.05), -1).to(dev)
        same = bool(torch.equal(box_shrink(box, sc["pc"]), box_shrink_torch(box, sc["pc"])))
        res = timed_alternating({"hip": lambda: box_shrink(box, sc["pc"]), "torch_broadcast": lambda: box_shrink_torch(box, sc["pc"])},
                                a.warmup, a.iters)
        print(json.dumps({"shape": "%dx%dx%d" % (b, s, n), "kind": a.kind, "measure": "box_shrink", "equal": same, **res}), flush=True)


def nms_3d_host(boxes, scores, pre_nms_limit, max_output_size, iou_threshold, score_threshold=float("-inf")):
    """nms_3d the way the reference runs it: device tensors to the host, greedy suppression per scene in numpy, the indices back"""
    bx, sc = boxes.cpu().numpy(), scores.cpu().numpy()
    out = np.full((bx.shape[0], max_output_size), -1, dtype=np.int32)
    for i in range(bx.shape[0]):
        lo, hi = bx[i, :, :3] - bx[i, :, 3:] / 2, bx[i, :, :3] + bx[i, :, 3:] / 2
        vol = bx[i, :, 3] * bx[i, :, 4] * bx[i, :, 5]
        cand = np.argsort(-sc[i])
        if pre_nms_limit > 0:
            cand = cand[:pre_nms_limit]
        cand = cand[sc[i][cand] > score_threshold]
        for k in range(max_output_size):
            if len(cand) == 0:
                break
            top = cand[0]
            out[i, k] = top
            inter = np.prod(np.maximum(np.minimum(hi[top], hi[cand]) - np.maximum(lo[top], lo[cand]), 0), axis=1)
            cand = cand[~(inter / (vol[cand] + vol[top] - inter + 1e-8) > iou_threshold)]
    return torch.from_numpy(out).to(boxes.device)


def roi_proposals(gt_boxes, ext, s, gen):
    """s boxes per scene as SPN hands them on: three quarters jittered copies of ground-truth boxes, the rest random in the room, sizes
    + 1e-3 like box_shrink's; scores from a permutation (pairwise distinct)"""
    b, g, _ = gt_boxes.shape
    nj = (3 * s) // 4
    src = torch.gather(gt_boxes, 1, torch.randint(0, g, (b, nj), generator=gen).unsqueeze(-1).expand(-1, -1, 6))
    jit = torch.cat((src[..., :3] + 0.12 * src[..., 3:] * torch.randn(b, nj, 3, generator=gen),
                     src[..., 3:] * (1 + 0.15 * torch.randn(b, nj, 3, generator=gen)).clamp(min=0.3)), -1)
    rnd = torch.cat((torch.rand(b, s - nj, 3, generator=gen) * ext, torch.rand(b, s - nj, 3, generator=gen) * 0.9 + 0.6), -1)
    boxes = torch.cat((jit, rnd), 1)
    boxes[..., 3:] += 1e-3
    scores = torch.stack([(torch.randperm(s, generator=gen).float() + 0.5) / s for _ in range(b)])
    return boxes.contiguous(), scores.contiguous()


def measure_roi(a, shape, b, n, dev):
    from gspn_amd import rpointnet as RP
    sc = {k: torch.from_numpy(v) for k, v in synth.spn_batch(a.kind, b, n, 100, 512, 19, seed0=7).items()}
    ext = sc["pc"].amax((0, 1))
    pc, gt_boxes, group_label = sc["pc"].to(dev), sc["bbox_ins"].to(dev), sc["group_label"].to(dev)
    gt_cls = RP.seg_label_per_group(sc["seg_label"].to(dev), group_label, 100)
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    for name, cfg in (("training", RP.Config()), ("inference", RP.Config(istrain=False))):
        train = name == "training"
        m = cfg.SPN_NMS_MAX_SIZE_TRAINING if train else cfg.SPN_NMS_MAX_SIZE_INFERENCE
        r, p = (cfg.TRAIN_ROIS_PER_IMAGE, cfg.NUM_POINT_INS_MASK) if train else (m, cfg.NUM_POINT_INS_MASK)
        boxes, scores = roi_proposals(sc["bbox_ins"], ext, cfg.NUM_SAMPLE, torch.Generator().manual_seed(cfg.NUM_SAMPLE))
        boxes, scores = boxes.to(dev), scores.to(dev)
        nms_args = (cfg.SPN_PRE_NMS_LIMIT, m, cfg.SPN_IOU_THRESHOLD)
        sel = RP.nms_3d(boxes, scores, *nms_args)
        res = {"nms_equal_to_host": bool(torch.equal(sel, nms_3d_host(boxes, scores, *nms_args))), "nms_picks": (sel >= 0).sum(1).tolist()}
        res.update(timed_alternating({"nms_3d": lambda: RP.nms_3d(boxes, scores, *nms_args),
                                      "nms_3d_host_round_trip": lambda: nms_3d_host(boxes, scores, *nms_args)}, a.warmup, a.iters))
        spn_rois = RP.gather_selection(boxes, sel, m)
        res["box_point_count"] = timed(lambda: RP.box_point_count(spn_rois, pc), a.warmup, a.iters)
        fea = torch.randn(b, n, a.crop_channels, device=dev).requires_grad_(train)
        cen = (pc + 0.1 * torch.randn(b, n, 3, device=dev)).requires_grad_(train)
        if train:
            targets = lambda: RP.detection_target_gen_batch(spn_rois, gt_cls, gt_boxes, group_label, pc, cfg, seed)
            res["detection_target_gen_batch"] = timed(targets, a.warmup, a.iters)
            rois, _, _, idx, _ = targets()
        selection = lambda: RP.mask_selection_gen_batch(spn_rois, pc, m, cfg, True, seed)
        res["mask_selection_gen_batch"] = timed(selection, a.warmup, a.iters)
        if not train:
            rois, idx = selection()

        def crop():
            fea.grad = cen.grad = None
            out = RP.points_cropping(pc, fea, cen, rois, idx, r, p, cfg.NORMALIZE_CROP_REGION)
            if train:
                (out[0].sum() + out[1].sum()).backward()

        res["points_cropping_fwd_bwd" if train else "points_cropping_fwd"] = timed(crop, a.warmup, a.iters)
        print(json.dumps({"shape": shape, "kind": a.kind, "measure": "roi", "config": name, "proposals": [cfg.NUM_SAMPLE, cfg.SPN_PRE_NMS_LIMIT, m],
                          "rois": r, "points_per_roi": p, "crop_channels": a.crop_channels, **res}), flush=True)


def unmold_segmentation_torch(masks, rois, class_ids, crop, pc, chunk):
    """unmold_segmentation as models/model_rpointnet.py:1008-1048 writes it -- the (B, R, N, P) distances, argmin, gather, times the box
    mask -- `chunk` ROIs at a time (the whole tensor is 3.7 G floats at 2 x 100 x 18000 x 1024)"""
    b, r, p, _ = masks.shape
    sel = torch.gather(masks, 3, class_ids.long().reshape(b, r, 1, 1).expand(b, r, p, 1)).squeeze(3)
    out = torch.empty((b, r, pc.shape[1]), dtype=masks.dtype, device=masks.device)
    pc_aug = pc.unsqueeze(1)
    for k in range(0, r, chunk):
        dist = (pc_aug.unsqueeze(3) - crop[:, k:k + chunk].unsqueeze(2)).square().sum(-1)
        val = torch.gather(sel[:, k:k + chunk], 2, dist.argmin(3))
        box = rois[:, k:k + chunk].unsqueeze(2)
        inside = ((pc_aug >= box[..., :3] - box[..., 3:] / 2) & (pc_aug <= box[..., :3] + box[..., 3:] / 2)).all(-1)
        out[:, k:k + chunk] = val * inside.float()
    return out


def measure_detect(a, shape, b, n, dev):
    from gspn_amd import rpointnet as RP
    cfg = RP.Config(istrain=False)
    sc = {k: torch.from_numpy(v) for k, v in synth.spn_batch(a.kind, b, n, 100, 512, 19, seed0=7).items()}
    ext = sc["pc"].amax((0, 1))
    pc = sc["pc"].to(dev)
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    gen = torch.Generator().manual_seed(384)
    r, c = cfg.SPN_NMS_MAX_SIZE_INFERENCE, cfg.NUM_CATEGORY
    rois = roi_proposals(sc["bbox_ins"], ext, r, gen)[0].to(dev)
    probs = torch.softmax(torch.randn(b, r, c, generator=gen) * 2.5, -1).to(dev)
    deltas = (torch.randn(b, r, c, 6, generator=gen) * 0.3).to(dev)
    fb, sem = torch.rand(b, r, generator=gen).to(dev), torch.rand(b, r, generator=gen).to(dev)
    det = RP.refine_detections_batch(rois, probs, deltas, pc, fb, sem, cfg)
    res = {"detections": (det[..., 6] > 0).sum(1).tolist()}
    res.update(timed_alternating({"refine_detections_batch": lambda: RP.refine_detections_batch(rois, probs, deltas, pc, fb, sem, cfg)}, a.warmup, a.iters))
    # 100 detections per scene: boxes around the instances, 1024 crop points drawn inside each
    m, p = cfg.DETECTION_MAX_INSTANCES, cfg.NUM_POINT_INS_MASK
    boxes = roi_proposals(sc["bbox_ins"], ext, m, gen)[0].to(dev)
    det_rois, idx = RP.mask_selection_gen_batch(boxes, pc, m, cfg, False, seed)
    crop = RP.points_cropping(pc, pc, pc, det_rois, idx, m, p, cfg.NORMALIZE_CROP_REGION)[3].contiguous()
    masks = torch.sigmoid(torch.randn(b, m, p, c, generator=gen) * 3.0).to(dev)
    ids = torch.randint(1, c, (b, m), generator=gen).int().to(dev)
    gated = RP.nearest_in_sets(pc, crop, det_rois)
    inside = int((gated >= 0).sum())
    ours = RP.unmold_segmentation(masks, det_rois, ids, crop, pc)
    theirs = unmold_segmentation_torch(masks, det_rois, ids, crop, pc, a.unmold_chunk)
    res.update({"inside_share": round(inside / gated.numel(), 5), "distance_evals_gated": inside * p, "distance_evals_ungated": gated.numel() * p,
                "unmold_values_differing_from_torch": int((ours != theirs).sum())})       # torch's argmin leaves the choice among equals open
    res.update(timed_alternating({"nearest_in_sets_gated": lambda: RP.nearest_in_sets(pc, crop, det_rois),
                             "nearest_in_sets_ungated": lambda: RP.nearest_in_sets(pc, crop),
                             "unmold_segmentation": lambda: RP.unmold_segmentation(masks, det_rois, ids, crop, pc),
                             "unmold_segmentation_torch_broadcast": lambda: unmold_segmentation_torch(masks, det_rois, ids, crop, pc, a.unmold_chunk)},
                            a.warmup, a.iters))
    print(json.dumps({"shape": shape, "kind": a.kind, "measure": "detect", "rois": r, "detections_per_scene": m, "points_per_roi": p,
                      "unmold_chunk": a.unmold_chunk, **res}), flush=True)


def measure_heads(a, shape, b, n, dev):
    from gspn_amd import rpointnet as RP
    sc = {k: torch.from_numpy(v) for k, v in synth.spn_batch(a.kind, b, n, 100, 512, 19, seed0=7).items()}
    ext = sc["pc"].amax((0, 1))
    pc = sc["pc"].to(dev)
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    gen = torch.Generator().manual_seed(64)
    ncat = RP.Config.NUM_CATEGORY
    cases = (("training_both_heads_fwd_bwd", True, 64, 256, True, True), ("inference_classification_head_fwd", False, 384, 1024, True, False),
             ("inference_segmentation_head_fwd", False, 100, 1024, False, True))
    for name, train, r, p, with_cls, with_seg in cases:
        cfg = RP.Config(istrain=train)
        cfg.NUM_POINT_INS_MASK = p
        boxes = roi_proposals(sc["bbox_ins"], ext, r, gen)[0].to(dev)
        rois, idx = RP.mask_selection_gen_batch(boxes, pc, r, cfg, False, seed)
        fea = torch.randn(b, n, a.crop_channels, device=dev).requires_grad_(train)
        cen = (pc + 0.1 * torch.randn(b, n, 3, device=dev)).requires_grad_(train)
        store = tf_util.set_variable_store(tf_util.VariableStore(device=dev, seed=1))
        last = {}

        def run(fused):
            def fn():
                fea.grad = cen.grad = None
                for v in store.parameters():
                    v.grad = None
                if fused:
                    crop, coord, feat = dict(pc=pc, pc_fea=fea, pc_center=cen, rois=rois, idx=idx, normalize=cfg.NORMALIZE_CROP_REGION), None, None
                else:
                    f, c, coord, _ = RP.points_cropping(pc, fea, cen, rois, idx, r, p, cfg.NORMALIZE_CROP_REGION)
                    crop, feat = None, torch.cat((f, c), -1)
                outs = []
                if with_cls:
                    logits, _, deltas = RP.classification_head(coord, feat, ncat, [128, 256, 512], [256, 256], train, 0.5, 'classification_head',
                                                               crop=crop)
                    outs += [logits, deltas]
                if with_seg:
                    outs.append(RP.segmentation_head(coord, feat, ncat, [64, 64], [64, 128, 512], [256, 256], train, 0.5, 'segmentation_head',
                                                     crop=crop))
                if train:
                    sum(o.square().mean() for o in outs).backward()
                last[fused] = [o.detach() for o in outs]
            return fn

        fns = {"materialised": run(False), "fused": run(True)}
        for fn in fns.values():
            fn()
        diff = max(float((x - y).abs().max() / (y.abs().max() + 1e-30)) for x, y in zip(last[True], last[False]))
        res = timed_alternating(fns, a.warmup, a.iters)
        print(json.dumps({"shape": shape, "kind": a.kind, "measure": "heads", "config": name, "rois": r, "points_per_roi": p,
                          "crop_channels": a.crop_channels, "iters": a.iters, "max_relative_difference_fused_vs_materialised": diff, **res}),
              flush=True)


def measure_infer(a, shape, b, n, dev):
    from gspn_amd import rpointnet as RP
    from gspn_amd.inference import _point_probabilities
    from gspn_amd.shape_proposal import valid_instances
    cfg = RP.Config(istrain=False)
    cfg.BATCH_SIZE, cfg.NUM_POINT, cfg.DETECTION_MIN_CONFIDENCE = b, n, 0
    sc = {k: torch.from_numpy(v).to(dev) for k, v in
          synth.spn_batch(a.kind, b, n, cfg.NUM_GROUP, cfg.NUM_POINT_INS, cfg.NUM_CATEGORY, seed0=7).items()}
    args = (sc["pc"], sc["color"], sc["pc_ins"], sc["group_label"], sc["group_indicator"], sc["seg_label"], sc["bbox_ins"])
    pc = sc["pc"]
    valid = valid_instances(sc["group_indicator"])
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    m, p, d = cfg.SPN_NMS_MAX_SIZE_INFERENCE, cfg.NUM_POINT_INS_MASK, cfg.DETECTION_MAX_INSTANCES
    tf_util.set_variable_store(tf_util.VariableStore(device=dev, seed=1))
    whole = lambda fused: (lambda: RP.rpointnet_inference(*args, cfg, valid_idx=valid, seed=seed, fused_crop=fused))
    ep = whole(False)()
    found = (ep['detections'].abs().sum(-1) != 0).sum(1).tolist()
    fused_ep = whole(True)()
    diff = {k: float((fused_ep[k] - ep[k]).abs().max() / (ep[k].abs().max() + 1e-30)) for k in ('rpointnet_class_logits', 'rpointnet_bbox')}
    res = timed_alternating({"materialised": whole(False), "fused": whole(True)}, a.warmup, a.iters)
    print(json.dumps({"shape": shape, "kind": a.kind, "measure": "infer", "what": "rpointnet_inference", "seeds": cfg.NUM_SAMPLE, "rois": m,
                      "points_per_roi": p, "detections_per_scene": found, "detections_per_scene_fused": (fused_ep['detections'].abs().sum(-1) != 0)
                      .sum(1).tolist(), "max_relative_difference_fused_vs_materialised": diff, "iters": a.iters, **res}), flush=True)

    def stages(fused, times):
        """the driver's chain with an event behind every stage"""
        marks = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e))

        def heads_input(rois, idx, r):
            if fused:
                return None, None, dict(pc=pc, pc_fea=fea, pc_center=e_p['center_pos'], rois=rois, idx=idx, normalize=cfg.NORMALIZE_CROP_REGION)
            f, c, coord, _ = RP.points_cropping(pc, fea, e_p['center_pos'], rois, idx, r, p, cfg.NORMALIZE_CROP_REGION)
            return coord, torch.cat((f, c), -1), None

        with torch.no_grad():
            mark("start")
            e_p = RP.shape_proposal_net(pc, sc["color"], sc["pc_ins"], sc["group_label"], sc["group_indicator"], cfg.NUM_CATEGORY,
                                        'shape_proposal_net', False, bn_decay=None, nsmp=cfg.NUM_SAMPLE, return_fullfea=True, mode='inference',
                                        valid_idx=valid)
            mark("shape_proposal_net")
            sel = RP.nms_3d(e_p['bbox_ins_pred'], e_p['fb_prob'][:, :, 1], cfg.SPN_PRE_NMS_LIMIT, m, cfg.SPN_IOU_THRESHOLD, cfg.SPN_SCORE_THRESHOLD)
            rois, idx = RP.mask_selection_gen_batch(RP.gather_selection(e_p['bbox_ins_pred'], sel, m), pc, m, cfg, True, seed)
            mark("nms_and_mask_selection")
            fea = RP.fpn_features(e_p, False, None)
            mark("fpn_features")
            means = RP.crop_mean(_point_probabilities(pc, e_p), idx)
            mark("point_probabilities_and_crop_mean")
            coord, feat, crop = heads_input(rois, idx, m)
            logits, probs, deltas = RP.classification_head(coord, feat, cfg.NUM_CATEGORY, [128, 256, 512], [256, 256], False, None,
                                                           'classification_head', crop=crop)
            del coord, feat
            mark("crop_and_classification_head")
            sem = torch.gather(means[:, :, 1:], 2, logits.argmax(-1, keepdim=True)).squeeze(-1)
            det = RP.refine_detections_batch(rois, probs, deltas, pc, means[:, :, 0].contiguous(), sem, cfg)
            rois_f, idx_f = RP.mask_selection_gen_batch(det[:, :, :6], pc, d, cfg, False, seed + 1)
            mark("refine_detections_and_mask_selection")
            coord, feat, crop = heads_input(rois_f, idx_f, d)
            mask = RP.segmentation_head(coord, feat, cfg.NUM_CATEGORY, [64, 64], [64, 128, 512], [256, 256], False, None, 'segmentation_head',
                                        crop=crop)
            RP.select_segmentation(torch.sigmoid(mask), det[:, :, 6])
            mark("crop_and_segmentation_head")
        marks[-1][1].synchronize()
        for (_, e0), (name, e1) in zip(marks, marks[1:]):
            times.setdefault(name, []).append(e0.elapsed_time(e1))

    per_stage = {}
    for fused in (False, True):
        times = {}
        for i in range(a.warmup + a.iters):
            stages(fused, times if i >= a.warmup else {})
        per_stage["fused" if fused else "materialised"] = {k: {"median_ms": round(sorted(v)[len(v) // 2], 4), "min_ms": round(min(v), 4),
                                                                "max_ms": round(max(v), 4)} for k, v in times.items()}
    print(json.dumps({"shape": shape, "kind": a.kind, "measure": "infer", "what": "stages", "iters": a.iters, **per_stage}), flush=True)

    # crop_mean on the 1024-wide path against the reference's form at width 1044
    with torch.no_grad():
        fea = RP.fpn_features(ep, False, None)
    table = _point_probabilities(pc, ep)
    rois, idx = ep['rois'], ep['mask_selection_idx']

    def reference_form():
        wide = torch.cat((fea, table), -1)
        cropped = RP.points_cropping(pc, wide, ep['center_pos'], rois, idx, m, p, cfg.NORMALIZE_CROP_REGION)[0]
        return cropped[..., fea.shape[2]:].mean(2)

    ours, theirs = RP.crop_mean(table, idx), reference_form()
    res = timed_alternating({"crop_mean": lambda: RP.crop_mean(table, idx), "concat_crop_split_mean": reference_form}, a.warmup, a.iters)
    print(json.dumps({"shape": shape, "kind": a.kind, "measure": "infer", "what": "crop_mean", "table": list(table.shape), "idx": list(idx.shape),
                      "feature_channels": fea.shape[2], "iters": a.iters,
                      "max_relative_difference": float((ours - theirs).abs().max() / (theirs.abs().max() + 1e-30)), **res}), flush=True)


def measure_train_heads(a, shape, b, n, dev):
    """one head-training step -- the frozen proposal net, rpointnet_heads_from_proposals, get_head_training_loss, backward -- in the four
    forms, alternating; and segmentation_head's forward alone at the inference shape with and without split_post.  A freshly initialised
    proposal net matches no ground truth and the step would train on padding alone, so the proposals are planted as in
    tests/test_gpu_head_training.py: the first NUM_GROUP seeds carry the foreground ground-truth boxes of non-zero size, the others small cubes about points
    of the scene (a few device operations inside the timed step, the same for every form)."""
    from gspn_amd import rpointnet as RP
    from gspn_amd.shape_proposal import valid_instances
    cfg = RP.Config()
    cfg.BATCH_SIZE, cfg.NUM_POINT, cfg.TRAIN_MODULE = b, n, ['RPOINTNET']
    sc = {k: torch.from_numpy(v).to(dev) for k, v in
          synth.spn_batch(a.kind, b, n, cfg.NUM_GROUP, cfg.NUM_POINT_INS, cfg.NUM_CATEGORY, seed0=7).items()}
    pc = sc["pc"]
    valid = valid_instances(sc["group_indicator"])
    noise = torch.randn(b, cfg.NUM_SAMPLE, 256, device=dev)
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    store = tf_util.set_variable_store(tf_util.VariableStore(device=dev, seed=1))
    heads_of = ("fpn", "classification_head/", "segmentation_head/")
    per_group = RP.seg_label_per_group(sc["seg_label"], sc["group_label"], cfg.NUM_GROUP)
    # (a group of one point has a box of size 0: as an ROI it would divide its crop by 0, here as in the reference -- not planted)
    fg = ((per_group > 0) & (sc["bbox_ins"][:, :, 3:].amin(-1) > 0)).unsqueeze(-1)
    at = (torch.arange(cfg.NUM_SAMPLE, device=dev) * 61 + 7) % n
    score = torch.linspace(0.99, 0.01, cfg.NUM_SAMPLE, device=dev).expand(b, -1)
    last = {}

    def run(name, **switches):
        def fn():
            for v in store.parameters():
                v.grad = None
            with torch.no_grad():
                ep = RP.shape_proposal_net(pc, sc["color"], sc["pc_ins"], sc["group_label"], sc["group_indicator"], cfg.NUM_CATEGORY,
                                           'shape_proposal_net', False, bn_decay=None, nsmp=cfg.NUM_SAMPLE, return_fullfea=True, mode='training',
                                           noise=noise, valid_idx=valid)
            cubes = torch.cat((pc[:, at], torch.full((b, cfg.NUM_SAMPLE, 3), 0.3, device=dev)), -1)
            ep['bbox_ins_pred'] = torch.cat((torch.where(fg, sc["bbox_ins"], cubes[:, :cfg.NUM_GROUP]), cubes[:, cfg.NUM_GROUP:]), 1)
            ep['fb_prob'] = torch.stack((1 - score, score), -1)
            ep = RP.rpointnet_heads_from_proposals(ep, pc, sc["group_label"], sc["seg_label"], sc["bbox_ins"], cfg, True, 0.5, seed=seed,
                                                   **switches)
            loss, ep = RP.get_head_training_loss(ep, cfg, 1.0, sc["smpw"])
            loss.backward()
            last[name] = (loss.detach(), {k: v.grad for k, v in store.named_parameters() if k.startswith(heads_of)}, ep)
        return fn

    fns = {"materialised": run("materialised"), "fused_crop": run("fused_crop", fused_crop=True),
           "shared_first": run("shared_first", fused_crop=True, shared_first=True),
           "split_post": run("split_post", fused_crop=True, shared_first=True, split_post=True)}
    for fn in fns.values():
        fn()
    loss0, grads0, ep0 = last["materialised"]
    for name, (loss, grads, _) in last.items():              # a difference of NaNs would read as 0
        if not (bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) for g in grads.values())):
            raise RuntimeError("train_heads: the %s form returned a loss or a gradient that is not finite" % name)
    valid_rois = ep0['rois'].abs().sum(-1) != 0
    diffs = {}
    for name in list(fns)[1:]:
        loss, grads, _ = last[name]
        worst = 0.0
        for k, g0 in grads0.items():
            beta = k.rsplit("/", 1)[0] + "/bn/beta"              # biases in front of a batch norm: true gradient 0, judged on beta's scale
            scale = grads0[beta] if k.endswith("/biases") and beta in grads0 else g0
            worst = max(worst, float((grads[k] - g0).abs().max() / (scale.abs().max() + 1e-30)))
        diffs[name] = {"loss": float((loss - loss0).abs() / loss0.abs()), "parameter_gradients": worst}
    res = timed_alternating(fns, a.warmup, a.iters)
    print(json.dumps({"shape": shape, "kind": a.kind, "measure": "train_heads", "what": "step: proposal net (frozen) + heads + loss + backward",
                      "seeds": cfg.NUM_SAMPLE, "rois": cfg.TRAIN_ROIS_PER_IMAGE, "points_per_roi": cfg.NUM_POINT_INS_MASK,
                      "positive_rois_per_scene": (valid_rois & (ep0['target_class_ids'] > 0)).sum(1).tolist(),
                      "negative_rois_per_scene": (valid_rois & (ep0['target_class_ids'] == 0)).sum(1).tolist(), "loss": float(loss0),
                      "max_relative_difference_vs_materialised": diffs, "iters": a.iters, **res}), flush=True)
    del last, fns
    for v in store.parameters():
        v.grad = None

    # segmentation_head forward alone at the inference shape, on materialised inputs built outside the timed region
    r, p, c = 100, 1024, a.crop_channels
    gen = torch.Generator().manual_seed(65)
    coord = (torch.rand(b, r, p, 3, generator=gen) - 0.5).to(dev)
    feat = torch.randn(b, r, p, c + 3, generator=gen).to(dev)
    tf_util.set_variable_store(tf_util.VariableStore(device=dev, seed=1))
    out = {}

    def seg(split):
        def fn():
            with torch.no_grad():
                out[split] = RP.segmentation_head(coord, feat, cfg.NUM_CATEGORY, [64, 64], [64, 128, 512], [256, 256], False, None,
                                                  'segmentation_head', split_post=split)
        return fn

    fns = {"materialised_concat": seg(False), "split_post": seg(True)}
    for fn in fns.values():
        fn()
    diff = float((out[True] - out[False]).abs().max() / (out[False].abs().max() + 1e-30))
    res = timed_alternating(fns, a.warmup, a.iters)
    print(json.dumps({"shape": shape, "kind": a.kind, "measure": "train_heads", "what": "segmentation_head forward alone", "rois": r,
                      "points_per_roi": p, "input_channels": c + 6, "max_relative_difference": diff, "iters": a.iters, **res}), flush=True)


DATASET_MIX = ([300, 17000, 9000, 4500, 1300, 600, 68], [20000, 1800, 400, 64, 10, 0, 2500, 7994])      # of 32768 points: tests/test_gpu_dataset.py


def measure_dataset(a, shape, b, n, dev):
    from gspn_amd import dataset, graph
    m, g = a.points_per_instance, max(len(s) for s in DATASET_MIX)
    pcs, labels, sizes_used = [], [], []
    for s in range(b):
        rng = np.random.default_rng(90 + s)
        mix = DATASET_MIX[s % len(DATASET_MIX)]
        sizes = [c * n // 32768 for c in mix] + [0] * (g - len(mix))
        sizes[1] += n - sum(sizes)
        sizes_used.append(sizes)
        pcs.append(synth.cloud_d(n, 90 + s))
        labels.append(np.repeat(np.arange(g), sizes)[rng.permutation(n)])
    pc, label = torch.from_numpy(np.stack(pcs)).to(dev), torch.from_numpy(np.stack(labels)).to(dev)
    seed = torch.tensor([7], dtype=torch.int64, device=dev)
    calls = {"fps": 0, "compactions": 0}

    def loop():
        """what the library offered before: one boolean compaction (a host synchronisation) and one b = 1 FPS call per instance"""
        out = torch.zeros((b, g, m, 3), device=dev)
        calls["fps"] = calls["compactions"] = 0
        for s in range(b):
            for j in range(1, g):
                pts = pc[s][label[s] == j]
                calls["compactions"] += 1
                c = pts.shape[0]
                if c > m:
                    out[s, j] = pts[farthest_point_sample(m, pts[None])[0].long()]
                    calls["fps"] += 1
                elif c > 0:
                    out[s, j] = torch.cat((pts, pts[torch.randint(0, c, (m - c,), device=dev)]))
        return out

    want, got = loop(), dataset.instance_point_sets(pc, label, g, m, seed)
    sampled = [(s, j) for s in range(b) for j in range(1, g) if sizes_used[s][j] > m]
    same = all(bool(torch.equal(want[s, j], got[s, j])) for s, j in sampled)
    step = graph.CapturedStep(lambda: dataset.instance_point_sets(pc, label, g, m, seed))
    res = timed_alternating({"fps_segments": lambda: dataset.fps_segments(pc, label, g, m, seed), "per_instance_loop": loop,
                             "instance_point_sets_captured": step.replay}, a.warmup, a.iters)
    print(json.dumps({"shape": shape, "measure": "dataset", "points_per_instance": m, "groups": g, "instance_sizes": sizes_used,
                      "sampled_rows_equal_the_loop": same, "loop_fps_calls": calls["fps"], "loop_host_compactions": calls["compactions"],
                      "iters": a.iters, **res}), flush=True)


def scene_predictions_torch(RP, masks, ep, pc, label_map, sem_th=0.01, fb_th=0.01, mask_th=0.4):
    """test.py:163-205 in torch on the device: the unmolded (B, R, N) float tensor, float64 products with the tables, two argsorts"""
    from gspn_amd.inference import _point_probabilities
    det = ep["detections"]
    cls = det[:, :, 6].long()
    valid = cls > 0
    table = _point_probabilities(pc, ep).double()
    g = RP.unmold_segmentation(masks, det[:, :, :6].contiguous(), det[:, :, 6], ep["pc_coord_cropped_final_unnormalized"], pc).double()
    g = g * valid.unsqueeze(-1)
    total = 1e-8 + g.sum(-1)
    sem_conf = torch.gather(torch.matmul(g, table[:, :, 1:]), 2, cls.unsqueeze(-1)).squeeze(-1) / total
    fb_conf = torch.matmul(g, table[:, :, :1]).squeeze(-1) / total
    score = (det[:, :, 7].double() * sem_conf * fb_conf) * valid
    group = torch.where(valid, torch.where((sem_conf > sem_th) & (fb_conf > fb_th), 0, 1), 2)
    by_score = torch.argsort(-score, dim=1, stable=True)
    order = torch.gather(by_score, 1, torch.argsort(torch.gather(group, 1, by_score), dim=1, stable=True))
    mask = (g > mask_th).to(torch.uint8)
    rows = order.unsqueeze(-1).expand(-1, -1, pc.shape[1])
    return {"order": order.int(), "count": valid.sum(1).int(), "label_ids": torch.gather(label_map[cls] * valid, 1, order).int(),
            "confidence": torch.gather(torch.where(group == 0, 1.0, 0.97) * valid, 1, order).float(), "sem_conf": torch.gather(sem_conf, 1, order),
            "fb_conf": torch.gather(fb_conf, 1, order), "score": torch.gather(score, 1, order), "masks": torch.gather(mask, 1, rows),
            "mask_points": torch.gather(mask.sum(-1), 1, order).int()}


def predict_inputs(a, b, n, dev):
    """synthetic head outputs with Config(istrain=False)'s widths -> RP, pc, masks, ep, the detection boxes, (m, p, c, ns)"""
    from gspn_amd import rpointnet as RP
    cfg = RP.Config(istrain=False)
    sc = {k: torch.from_numpy(v) for k, v in synth.spn_batch(a.kind, b, n, 100, 512, 19, seed0=7).items()}
    ext = sc["pc"].amax((0, 1))
    pc = sc["pc"].to(dev)
    gen = torch.Generator().manual_seed(19)
    m, p, c, ns = cfg.DETECTION_MAX_INSTANCES, cfg.NUM_POINT_INS_MASK, cfg.NUM_CATEGORY, cfg.NUM_SAMPLE
    boxes = roi_proposals(sc["bbox_ins"], ext, m, gen)[0].to(dev)
    det_rois, idx = RP.mask_selection_gen_batch(boxes, pc, m, cfg, False, torch.zeros(1, dtype=torch.int64, device=dev))
    crop = RP.points_cropping(pc, pc, pc, det_rois, idx, m, p, cfg.NORMALIZE_CROP_REGION)[3].contiguous()
    masks = torch.sigmoid(torch.randn(b, m, p, c, generator=gen) * 3.0).to(dev)
    ids = torch.randint(1, c, (b, m), generator=gen)
    ids[:, 3 * m // 4:] = 0                                          # the padding rows behind the last detection
    det = torch.cat((det_rois, ids.float().unsqueeze(-1).to(dev), torch.rand(b, m, 1, generator=gen).to(dev)), -1).contiguous()
    seeds = torch.stack([torch.randperm(n, generator=gen)[:ns] for _ in range(b)]).to(dev)
    ep = {"detections": det, "rpointnet_mask_selected": RP.select_segmentation(masks, det[:, :, 6]).contiguous(),
          "pc_coord_cropped_final_unnormalized": crop, "pc_seed": torch.gather(pc, 1, seeds.unsqueeze(-1).expand(-1, -1, 3)).contiguous(),
          "fb_prob": torch.softmax(torch.randn(b, ns, 2, generator=gen), -1).to(dev), "sem_class_logits": (torch.randn(b, n, c, generator=gen) * 2).to(dev)}
    return RP, pc, masks, ep, det_rois, (m, p, c, ns)


def measure_predict(a, shape, b, n, dev):
    from gspn_amd import graph
    RP, pc, masks, ep, det_rois, (m, p, c, ns) = predict_inputs(a, b, n, dev)
    crop = ep["pc_coord_cropped_final_unnormalized"]
    label_map = torch.tensor(RP.SCANNET_LABEL_MAP, device=dev)
    ours, theirs = RP.scene_predictions(ep, pc), scene_predictions_torch(RP, masks, ep, pc, label_map)
    live = theirs["sem_conf"] > 0
    res = {"predictions": ours["count"].tolist(), "inside_share": round(float((RP.nearest_in_sets(pc, crop, det_rois) >= 0).float().mean()), 5),
           "order_equal": bool(torch.equal(ours["order"], theirs["order"])), "masks_equal": bool(torch.equal(ours["masks"], theirs["masks"])),
           "labels_equal": bool(torch.equal(ours["label_ids"], theirs["label_ids"])),
           "confidence_rel_diff": float(max(((ours[k] - theirs[k]).abs()[live] / theirs[k][live]).max() for k in ("sem_conf", "fb_conf")))}
    st = {}
    step = graph.CapturedStep(lambda: st.update(pred=RP.scene_predictions(ep, pc)))
    res.update(timed_alternating({"scene_predictions": lambda: RP.scene_predictions(ep, pc),
                                  "torch_on_device": lambda: scene_predictions_torch(RP, masks, ep, pc, label_map),
                                  "scene_predictions_captured": step.replay}, a.warmup, a.iters))
    print(json.dumps({"shape": shape, "kind": a.kind, "measure": "predict", "detections_per_scene": m, "points_per_roi": p, "categories": c,
                      "seeds": ns, "iters": a.iters, **res}), flush=True)


def scan_predictions_torch(ep, s, verts, pc, chunk=1024):
    """lift.vertex_tables and gspn_lift_masks in torch on the device, a chunk of vertices at a time: (chunk, N) and (R, chunk, P) distance
    tensors, the first minimum of each, the sums in float64 -> sem_conf, fb_conf (R,), mask (R, V) uint8"""
    det, crops, masks = ep["detections"][s], ep["pc_coord_cropped_final_unnormalized"][s], ep["rpointnet_mask_selected"][s]
    cls = det[:, 6].long()
    valid = (cls > 0).unsqueeze(-1)
    sem_prob = torch.softmax(ep["sem_class_logits"][s], -1).double()
    fb1 = ep["fb_prob"][s][:, 1].double()
    lo, hi = (det[:, :3] - det[:, 3:6] / 2).unsqueeze(1), (det[:, :3] + det[:, 3:6] / 2).unsqueeze(1)
    r, v = det.shape[0], verts.shape[0]
    sums = torch.zeros((3, r), dtype=torch.float64, device=verts.device)
    mask = torch.empty((r, v), dtype=torch.uint8, device=verts.device)

    def first_min(q, pts):                                            # q (..., C, 3), pts (..., P, 3) -> (..., C)
        d = q.unsqueeze(-2) - pts.unsqueeze(-3)
        return torch.argmin((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], -1)

    for at in range(0, v, chunk):
        q = verts[at:at + chunk]
        src, seed = first_min(q, pc[s]), first_min(q, ep["pc_seed"][s])
        inside = ((q.unsqueeze(0) >= lo) & (q.unsqueeze(0) <= hi)).all(-1) & valid
        g = torch.gather(masks, 1, first_min(q.unsqueeze(0).expand(r, -1, -1), crops)).double() * inside
        sums[0] += g.sum(1)
        sums[1] += (g * sem_prob[src][:, cls].t()).sum(1)
        sums[2] += (g * fb1[seed].unsqueeze(0)).sum(1)
        mask[:, at:at + chunk] = g > 0.4
    return sums[1] / (1e-8 + sums[0]), sums[2] / (1e-8 + sums[0]), mask


def measure_lift(a, shape, b, n, dev):
    """--measures lift: scan_predictions against scene_predictions on the scene's own points, then on synthetic scans of
    150 000 and 500 000 vertices around the scene with the share of vertex_tables and of gspn_lift_masks alone, vertex_tables by three_nn
    and by nearest_point with the build alone and both searches by the size of the known set, and the same arithmetic
    in torch on the device.  Call times: device events around the calls as a user makes them, allocations and torch's own kernels included."""
    from gspn_amd import lift
    from gspn_amd.nearest import nearest_point
    from gspn_amd.tf_interpolate import three_nn
    RP, pc, masks, ep, det_rois, (m, p, c, ns) = predict_inputs(a, b, n, dev)
    own = pc[0].contiguous()
    ours, whole = lift.scan_predictions(ep, 0, own, pc=pc), RP.scene_predictions(ep, pc)
    res = {"inside_share": round(float((RP.nearest_in_sets(pc, ep["pc_coord_cropped_final_unnormalized"], det_rois) >= 0).float().mean()), 5),
           "valid_detections": int(whole["count"][0]),
           "equal_to_scene_predictions": all(bool(torch.equal(ours[k][0], whole[k][0])) for k in ("masks", "mask_points", "order", "count", "label_ids", "confidence")),
           "src_is_identity": bool(torch.equal(ours["src"], torch.arange(n, dtype=torch.int32, device=dev)))}
    res["at_%d" % n] = timed_alternating({"scene_predictions": lambda: RP.scene_predictions(ep, pc),
                                          "scan_predictions": lambda: lift.scan_predictions(ep, 0, own, pc=pc)}, a.warmup, a.iters)
    for v in [n] + [int(t) for t in a.lift_vertices.split(",") if t]:
        verts = torch.from_numpy(synth.scan_vertices(own.cpu().numpy(), np.zeros(n, np.int32), np.zeros(n, np.int32), v, 3)[0]).to(dev)
        src, vert_fb = lift.vertex_tables(verts, own, ep["pc_seed"][0], ep["fb_prob"][0])
        sem_prob = torch.softmax(ep["sem_class_logits"][0:1], -1)[0]
        det = ep["detections"][0]
        args = (verts, ep["pc_coord_cropped_final_unnormalized"][0], det[:, :6].contiguous(), ep["rpointnet_mask_selected"][0], det[:, 6].int(), src,
                sem_prob, vert_fb)
        pred = lift.scan_predictions(ep, 0, verts, pc=pc)
        entry = res.setdefault("at_%d" % v, {})
        entry.update({"set_share": round(float(lift.lift_masks(*args)[3].sum()) / (max(int(whole["count"][0]), 1) * v), 5), "mask_bytes": m * v})
        entry.update(timed_alternating({"scan_predictions_and_parts": lambda: lift.scan_predictions(ep, 0, verts, pc=pc),
                                        "vertex_tables": lambda: lift.vertex_tables(verts, own, ep["pc_seed"][0], ep["fb_prob"][0]),
                                        "lift_masks": lambda: lift.lift_masks(*args)}, a.warmup, a.iters))
        # vertex_tables by the parent's route (three_nn twice) and with both searches through nearest_point, the build alone
        # (a call with one query: six build launches and one query workgroup), and the two searches by the size of the known set
        tables = {k: lift.vertex_tables(verts, own, ep["pc_seed"][0], ep["fb_prob"][0], search=k) for k in ("three_nn", "nearest_point")}
        entry["routes_equal"] = bool(torch.equal(tables["three_nn"][0], tables["nearest_point"][0])
                                     and torch.equal(tables["three_nn"][1].view(torch.int32), tables["nearest_point"][1].view(torch.int32)))
        q1, k1 = verts.unsqueeze(0), own.unsqueeze(0)
        entry.update(timed_alternating({
            "vertex_tables_three_nn": lambda: lift.vertex_tables(verts, own, ep["pc_seed"][0], ep["fb_prob"][0], search="three_nn"),
            "vertex_tables_nearest_point": lambda: lift.vertex_tables(verts, own, ep["pc_seed"][0], ep["fb_prob"][0], search="nearest_point"),
            "nearest_point_build_alone": lambda: nearest_point(q1[:, :1], k1)}, a.warmup, a.iters))
        by_size = entry.setdefault("by_known_size", {})
        for size in (256, 512, 1024, 2048, 4096, 8192, n):
            known = k1[:, torch.randperm(n, generator=torch.Generator().manual_seed(size))[:size].to(dev)].contiguous()
            by_size[str(size)] = timed_alternating({"three_nn": lambda: three_nn(q1, known)[1][0, :, 0].contiguous(),
                                                    "nearest_point": lambda: nearest_point(q1, known)[1][0]}, a.warmup, a.iters)
        if v <= a.lift_torch_max:
            sem_conf, fb_conf, mask = scan_predictions_torch(ep, 0, verts, pc)
            at = pred["order"][0].long()
            entry["torch_masks_equal"] = bool(torch.equal(mask[at], pred["masks"][0]))
            entry.update(timed_alternating({"torch_on_device": lambda: scan_predictions_torch(ep, 0, verts, pc)}, 1, min(a.iters, 5)))
    print(json.dumps({"shape": shape, "kind": a.kind, "measure": "lift", "detections": m, "points_per_roi": p, "categories": c, "seeds": ns,
                      "iters": a.iters, **res}), flush=True)


def segment_vote_torch(masks, seg, s, vote_th):
    """segments.segment_vote in torch on the device: the sizes once, then an index_add_ of the set vertices, the double compare and a gather
    per row -> out (R, V) uint8, mask_points (R,) int32"""
    inside = (seg >= 0) & (seg < s)
    ids = seg.long().clamp(0, max(s - 1, 0))
    size = torch.zeros(s, dtype=torch.int32, device=seg.device).index_add_(0, ids, inside.int()).double()
    out = torch.empty_like(masks)
    for k in range(masks.shape[0]):
        own = masks[k] != 0
        cnt = torch.zeros(s, dtype=torch.int32, device=seg.device).index_add_(0, ids, (inside & own).int()).double()
        out[k] = torch.where(inside, (cnt > vote_th * size)[ids], own)
    return out, out.sum(1, dtype=torch.int32)


def segment_label_vote_torch(labels, seg, s, c):
    """segments.segment_label_vote in torch on the device: one index_add_ into the (S, C) table, its first maxima, a gather"""
    inside = (seg >= 0) & (seg < s)
    votes = inside & (labels >= 0) & (labels < c)
    ids = seg.long().clamp(0, max(s - 1, 0))
    cnt = torch.zeros(s * c, dtype=torch.int32, device=seg.device).index_add_(0, ids * c + labels.long().clamp(0, c - 1), votes.int()).view(s, c)
    best, arg = cnt.max(1)
    return torch.where(inside & (best > 0)[ids], arg.int()[ids], labels)


def measure_segments(a, shape, b, n, dev):
    """--measures segments: segment_vote on the masks gspn_lift_masks leaves for the synthetic head outputs of `lift` -- 100
    rows -- on the scene's own points and on synthetic scans of --lift-vertices vertices, with synth.scan_segments' cubes of 0.25 m inside
    instances of 1 m cubes as the segments; with a workspace it allocates and with one the caller holds; against the same arithmetic in torch
    on the device; segment_label_vote at the `lift` inputs' categories and its torch form; compact_segments; and scan_predictions with
    and without segments beside lift_masks and vertex_tables, alternating in one process.  Call times by device events."""
    from gspn_amd import _lib, lift
    from gspn_amd import segments as SG
    RP, pc, masks, ep, det_rois, (m, p, c, ns) = predict_inputs(a, b, n, dev)
    own = pc[0].contiguous()
    res = {}
    for v in [n] + [int(t) for t in a.lift_vertices.split(",") if t]:
        xyz = synth.scan_vertices(own.cpu().numpy(), np.zeros(n, np.int32), np.zeros(n, np.int32), v, 3)[0]
        cube = np.floor(xyz.astype(np.float64)).astype(np.int64)
        group = ((cube[:, 0] * 7 + cube[:, 1]) * 5 + cube[:, 2]).astype(np.int32)                    # instances: the 1 m cubes of the room
        raw = torch.from_numpy(synth.scan_segments(xyz, group % c, group, 0.25, 5)).to(dev)
        verts = torch.from_numpy(xyz).to(dev)
        seg, s = SG.compact_segments(raw)
        src, vert_fb = lift.vertex_tables(verts, own, ep["pc_seed"][0], ep["fb_prob"][0])
        sem_prob = torch.softmax(ep["sem_class_logits"][0:1], -1)[0]
        det = ep["detections"][0]
        args = (verts, ep["pc_coord_cropped_final_unnormalized"][0], det[:, :6].contiguous(), ep["rpointnet_mask_selected"][0], det[:, 6].int(), src,
                sem_prob, vert_fb)
        mask = lift.lift_masks(*args)[2]
        labels = ep["sem_class_logits"][0].max(-1).indices.int().index_select(0, src.long())
        ws = torch.empty((int(_lib.lib().gspn_segment_vote_ws_bytes(m, v, s)),), dtype=torch.uint8, device=dev)
        held = torch.empty_like(mask)
        ours, theirs = SG.segment_vote(mask, seg, s), segment_vote_torch(mask, seg, s, 0.5)
        entry = res.setdefault("at_%d" % v, {})
        entry.update({"segments": s, "mask_bytes": m * v, "set_share_in": round(float((mask != 0).float().mean()), 5),
                      "set_share_out": round(float(ours[0].float().mean()), 5), "bytes_changed": int((ours[0] != mask).sum()),
                      "vote_equals_torch": bool(torch.equal(ours[0], theirs[0]) and torch.equal(ours[1], theirs[1])),
                      "labels_equal_torch": bool(torch.equal(SG.segment_label_vote(labels, seg, s, c), segment_label_vote_torch(labels, seg, s, c)))})
        entry.update(timed_alternating({
            "segment_vote": lambda: SG.segment_vote(mask, seg, s),
            "segment_vote_held_ws_and_out": lambda: SG.segment_vote(mask, seg, s, out=held, ws=ws),
            "segment_vote_torch": lambda: segment_vote_torch(mask, seg, s, 0.5),
            "segment_label_vote": lambda: SG.segment_label_vote(labels, seg, s, c),
            "segment_label_vote_torch": lambda: segment_label_vote_torch(labels, seg, s, c),
            "compact_segments": lambda: SG.compact_segments(raw),
            "lift_masks": lambda: lift.lift_masks(*args),
            "vertex_tables": lambda: lift.vertex_tables(verts, own, ep["pc_seed"][0], ep["fb_prob"][0]),
            "scan_predictions": lambda: lift.scan_predictions(ep, 0, verts, pc=pc),
            "scan_predictions_segments": lambda: lift.scan_predictions(ep, 0, verts, pc=pc, segments=seg, num_segments=s)}, a.warmup, a.iters))
    print(json.dumps({"shape": shape, "kind": a.kind, "measure": "segments", "rows": m, "categories": c, "iters": a.iters, **res}), flush=True)


def mask_overlaps_torch(masks):
    """mask_nms.mask_overlaps in torch on the device: the masks as floats (a copy four times their size) and one fp32 GEMM; exact while a
    count stays below 2^24 -> sizes (R,) int32, inter (R, R) int32"""
    f = (masks != 0).float()
    inter = (f @ f.T).int()
    return inter.diagonal().contiguous(), inter


def measure_mask_nms(a, shape, b, n, dev):
    """--measures mask_nms: the rows scan_predictions leaves in output order behind the segment vote, for `segments`' inputs
    -- 100 rows -- on the scene's own points and on synthetic scans of --lift-vertices vertices, and the same rows with every even row
    copied onto the odd row behind it (duplicates for the stage to find): mask_overlaps against masks.float() @ masks.float().T on the
    device, mask_nms whole with a workspace it allocates and with one the caller holds, and scan_predictions with segments with and
    without mask_nms_th, alternating in one process.  Call times by device events."""
    from gspn_amd import _lib, lift
    from gspn_amd import mask_nms as MN
    from gspn_amd import segments as SG
    RP, pc, masks, ep, det_rois, (m, p, c, ns) = predict_inputs(a, b, n, dev)
    own = pc[0].contiguous()
    res = {}
    for v in [n] + [int(t) for t in a.lift_vertices.split(",") if t]:
        xyz = synth.scan_vertices(own.cpu().numpy(), np.zeros(n, np.int32), np.zeros(n, np.int32), v, 3)[0]
        cube = np.floor(xyz.astype(np.float64)).astype(np.int64)
        group = ((cube[:, 0] * 7 + cube[:, 1]) * 5 + cube[:, 2]).astype(np.int32)                    # instances: the 1 m cubes of the room
        seg, s = SG.compact_segments(torch.from_numpy(synth.scan_segments(xyz, group % c, group, 0.25, 5)).to(dev))
        verts = torch.from_numpy(xyz).to(dev)
        pred = lift.scan_predictions(ep, 0, verts, pc=pc, segments=seg, num_segments=s)
        rows, count, labels = pred["masks"][0].contiguous(), pred["count"][0], pred["label_ids"][0].contiguous()
        twice = rows.clone()
        twice[1::2] = twice[0:2 * (m // 2):2]
        labels2 = labels.clone()
        labels2[1::2] = labels2[0:2 * (m // 2):2]
        ws = torch.empty((int(_lib.lib().gspn_mask_nms_ws_bytes(1, m, v)),), dtype=torch.uint8, device=dev)
        held = torch.empty_like(rows)
        ours, theirs = MN.mask_overlaps(rows), mask_overlaps_torch(rows)
        kept, kept2 = MN.mask_nms(rows, count, labels, iou_th=0.5)[1], MN.mask_nms(twice, count, labels2, iou_th=0.5)[1]
        entry = res.setdefault("at_%d" % v, {})
        entry.update({"mask_bytes": m * v, "live_rows": int(count), "set_share": round(float((rows != 0).float().mean()), 5),
                      "overlaps_equal_torch": bool(torch.equal(ours[0], theirs[0]) and torch.equal(ours[1], theirs[1])),
                      "nonzero_pairs": int((ours[1] != 0).sum()), "suppressed": int(count) - int(kept.sum()),
                      "suppressed_doubled_rows": int(count) - int(kept2.sum())})
        entry.update(timed_alternating({
            "mask_overlaps": lambda: MN.mask_overlaps(rows),
            "mask_overlaps_held_ws": lambda: MN.mask_overlaps(rows, ws=ws),
            "mask_overlaps_torch": lambda: mask_overlaps_torch(rows),
            "mask_overlaps_doubled_rows": lambda: MN.mask_overlaps(twice, ws=ws),
            "mask_nms": lambda: MN.mask_nms(rows, count, labels, iou_th=0.5),
            "mask_nms_held_ws_and_out": lambda: MN.mask_nms(rows, count, labels, iou_th=0.5, out=held, ws=ws),
            "mask_nms_doubled_rows": lambda: MN.mask_nms(twice, count, labels2, iou_th=0.5, out=held, ws=ws),
            "scan_predictions_segments": lambda: lift.scan_predictions(ep, 0, verts, pc=pc, segments=seg, num_segments=s),
            "scan_predictions_segments_mask_nms": lambda: lift.scan_predictions(ep, 0, verts, pc=pc, segments=seg, num_segments=s, mask_nms_th=0.5)},
            a.warmup, a.iters))
    print(json.dumps({"shape": shape, "kind": a.kind, "measure": "mask_nms", "rows": m, "iters": a.iters, **res}), flush=True)


def mask_components_torch(masks, faces):
    """components.mask_components' comp in torch on the device, what a user would write: the labels start as the vertex's own index, every
    edge whose two ends are set in a row passes the smaller label of its ends to both with scatter_reduce(amin), over all rows at once,
    until nothing changes (one read-back per round) -> comp (R, V) int32"""
    r, v = masks.shape
    f = faces.long()
    e = torch.cat((f[:, [0, 1]], f[:, [1, 2]], f[:, [0, 2]]))
    e = e[((e >= 0) & (e < v)).all(1)]
    on = masks != 0
    k, j = torch.nonzero(on[:, e[:, 0]] & on[:, e[:, 1]], as_tuple=True)               # (row, edge) pairs with both ends set
    a, b = k * v + e[j, 0], k * v + e[j, 1]
    label = torch.arange(v, device=masks.device).repeat(r)
    base = torch.arange(r, device=masks.device).repeat_interleave(v) * v
    while True:
        low = torch.minimum(label[a], label[b])
        new = label.scatter_reduce(0, a, low, "amin").scatter_reduce(0, b, low, "amin")
        new = new[base + new]                                                          # one pointer jump: a label's own label
        if torch.equal(new, label):
            break
        label = new
    return torch.where(on, label.view(r, v), -1).int()


def measure_components(a, shape, b, n, dev):
    """--measures components: the rows scan_predictions leaves in output order behind the segment vote, for `segments`'
    inputs -- 100 rows -- on the scene's own points and on synthetic scans of --lift-vertices vertices, with synth.scan_faces over
    `segments`' instances as the mesh: mask_components and component_filter with a workspace they allocate and with one the caller holds,
    the same labelling in torch on the device (iterated scatter_reduce(amin) to a fixed point), and scan_predictions with segments with
    and without the stage, alternating in one process.  Call times by device events."""
    from gspn_amd import _lib, lift
    from gspn_amd import components as MC
    from gspn_amd import segments as SG
    RP, pc, masks, ep, det_rois, (m, p, c, ns) = predict_inputs(a, b, n, dev)
    own = pc[0].contiguous()
    res = {}
    for v in [n] + [int(t) for t in a.lift_vertices.split(",") if t]:
        xyz = synth.scan_vertices(own.cpu().numpy(), np.zeros(n, np.int32), np.zeros(n, np.int32), v, 3)[0]
        cube = np.floor(xyz.astype(np.float64)).astype(np.int64)
        group = ((cube[:, 0] * 7 + cube[:, 1]) * 5 + cube[:, 2]).astype(np.int32)                    # instances: the 1 m cubes of the room
        seg, s = SG.compact_segments(torch.from_numpy(synth.scan_segments(xyz, group % c, group, 0.25, 5)).to(dev))
        faces = MC.mesh_faces(synth.scan_faces(xyz, group % c, group, 0.25, 5, bridges=v // 1000), v)
        verts = torch.from_numpy(xyz).to(dev)
        pred = lift.scan_predictions(ep, 0, verts, pc=pc, segments=seg, num_segments=s)
        rows = pred["masks"][0].contiguous()
        nf = int(faces.shape[0])
        ws_c = torch.empty((int(_lib.lib().gspn_mask_components_ws_bytes(m, v, nf)),), dtype=torch.uint8, device=dev)
        ws_f = torch.empty((int(_lib.lib().gspn_mask_component_filter_ws_bytes(m, v, nf)),), dtype=torch.uint8, device=dev)
        held = torch.empty_like(rows)
        comp, ncomp, largest = MC.mask_components(rows, faces)
        out, points, _, nkept = MC.component_filter(rows, faces, min_vertices=100, min_share=0.1)
        entry = res.setdefault("at_%d" % v, {})
        entry.update({"mask_bytes": m * v, "faces": nf, "set_share": round(float((rows != 0).float().mean()), 5),
                      "components": int(ncomp.sum()), "largest": int(largest.max()), "kept": int(nkept.sum()),
                      "vertices_dropped": int((rows != 0).sum()) - int(points.sum()), "bound_never_reached": bool((ncomp >= 0).all()),
                      "comp_equals_torch": bool(torch.equal(comp, mask_components_torch(rows, faces)))})
        stage = dict(faces=faces, min_component=100, min_component_share=0.1)
        entry.update(timed_alternating({
            "mask_components": lambda: MC.mask_components(rows, faces),
            "mask_components_held_ws": lambda: MC.mask_components(rows, faces, ws=ws_c),
            "mask_components_torch": lambda: mask_components_torch(rows, faces),
            "component_filter": lambda: MC.component_filter(rows, faces, min_vertices=100, min_share=0.1),
            "component_filter_held_ws_and_out": lambda: MC.component_filter(rows, faces, min_vertices=100, min_share=0.1, out=held, ws=ws_f),
            "scan_predictions_segments": lambda: lift.scan_predictions(ep, 0, verts, pc=pc, segments=seg, num_segments=s),
            "scan_predictions_segments_components": lambda: lift.scan_predictions(ep, 0, verts, pc=pc, segments=seg, num_segments=s, **stage)},
            a.warmup, a.iters))
    print(json.dumps({"shape": shape, "kind": a.kind, "measure": "components", "rows": m, "iters": a.iters, **res}), flush=True)


def measure_holes(a, shape, b, n, dev):
    """--measures holes: `components`' rows and mesh -- 100 rows in output order behind the segment vote, synth.scan_faces
    over `segments`' instances -- on the scene's own points and on synthetic scans of --lift-vertices vertices, with gaps punched into the
    rows (every set vertex whose cube of 0.1 m falls on one residue in eleven is unset): hole_fill with a workspace it allocates and with
    one the caller holds, beside component_filter on the same rows, and scan_predictions with segments with and without the stage,
    alternating in one process.  Call times by device events."""
    from gspn_amd import _lib, lift
    from gspn_amd import components as MC
    from gspn_amd import holes as MH
    from gspn_amd import segments as SG
    RP, pc, masks, ep, det_rois, (m, p, c, ns) = predict_inputs(a, b, n, dev)
    own = pc[0].contiguous()
    res = {}
    for v in [n] + [int(t) for t in a.lift_vertices.split(",") if t]:
        xyz = synth.scan_vertices(own.cpu().numpy(), np.zeros(n, np.int32), np.zeros(n, np.int32), v, 3)[0]
        cube = np.floor(xyz.astype(np.float64)).astype(np.int64)
        group = ((cube[:, 0] * 7 + cube[:, 1]) * 5 + cube[:, 2]).astype(np.int32)                    # instances: the 1 m cubes of the room
        seg, s = SG.compact_segments(torch.from_numpy(synth.scan_segments(xyz, group % c, group, 0.25, 5)).to(dev))
        faces = MC.mesh_faces(synth.scan_faces(xyz, group % c, group, 0.25, 5, bridges=v // 1000), v)
        verts = torch.from_numpy(xyz).to(dev)
        pred = lift.scan_predictions(ep, 0, verts, pc=pc, segments=seg, num_segments=s)
        small = np.floor(xyz.astype(np.float64) / 0.1).astype(np.int64)
        punched = torch.from_numpy(((small[:, 0] * 7 + small[:, 1] * 5 + small[:, 2] * 3) % 11) == 0).to(dev)
        whole = pred["masks"][0].contiguous()
        rows = (whole * ~punched).contiguous()
        nf = int(faces.shape[0])
        ws = torch.empty((int(_lib.lib().gspn_mask_hole_fill_ws_bytes(m, v, nf)),), dtype=torch.uint8, device=dev)
        ws_f = torch.empty((int(_lib.lib().gspn_mask_component_filter_ws_bytes(m, v, nf)),), dtype=torch.uint8, device=dev)
        held = torch.empty_like(rows)
        limit = 200
        out, points, nholes, nfilled, label = MH.hole_fill(rows, faces, verts, max_vertices=limit, label=True)
        entry = res.setdefault("at_%d" % v, {})
        entry.update({"mask_bytes": m * v, "faces": nf, "set_share": round(float((rows != 0).float().mean()), 5),
                      "vertices_punched": int((whole != 0).sum()) - int((rows != 0).sum()), "candidates": int((label >= 0).sum()),
                      "candidate_components": int((label == torch.arange(v, device=dev, dtype=torch.int32)).sum()), "holes": int(nholes.sum()),
                      "vertices_filled": int(nfilled.sum()), "filled_were_set": int(((out != 0) & (rows == 0) & (whole != 0)).sum()),
                      "bound_never_reached": bool((nholes >= 0).all()), "workspace_bytes": int(ws.numel())})
        stage = dict(faces=faces, max_hole=limit)
        entry.update(timed_alternating({
            "hole_fill": lambda: MH.hole_fill(rows, faces, verts, max_vertices=limit),
            "hole_fill_held_ws_and_out": lambda: MH.hole_fill(rows, faces, verts, max_vertices=limit, out=held, ws=ws),
            "component_filter": lambda: MC.component_filter(rows, faces, min_vertices=100, min_share=0.1),
            "component_filter_held_ws_and_out": lambda: MC.component_filter(rows, faces, min_vertices=100, min_share=0.1, out=held, ws=ws_f),
            "scan_predictions_segments": lambda: lift.scan_predictions(ep, 0, verts, pc=pc, segments=seg, num_segments=s),
            "scan_predictions_segments_holes": lambda: lift.scan_predictions(ep, 0, verts, pc=pc, segments=seg, num_segments=s, **stage)},
            a.warmup, a.iters))
    print(json.dumps({"shape": shape, "kind": a.kind, "measure": "holes", "rows": m, "iters": a.iters, **res}), flush=True)


def instance_counts_torch(masks, pred_class, seg, group, c, g):
    """instance_overlaps' four outputs in torch on the device: masks.float() against a one-hot of seg * G + group, a (B, N, C * G) float tensor"""
    live = (seg > 0) & (seg < c) & (group >= 0) & (group < g)
    onehot = torch.nn.functional.one_hot(torch.where(live, seg * g + group, 0).long(), c * g).float() * live.unsqueeze(-1)
    m = (masks != 0).float()
    valid = (pred_class > 0) & (pred_class < c)
    per_pair = torch.bmm(m, onehot).view(masks.shape[0], masks.shape[1], c, g)      # exact: counts below 2^24
    at = pred_class.clamp(0, c - 1).long().view(masks.shape[0], masks.shape[1], 1, 1).expand(-1, -1, 1, g)
    inter = (torch.gather(per_pair, 2, at).squeeze(2) * valid.unsqueeze(-1)).int()
    void = (torch.bmm(m, (~live).float().unsqueeze(-1)).squeeze(-1) * valid).int()
    return inter, void, (m.sum(-1) * valid).int(), onehot.sum(1).view(-1, c, g).int()


def measure_evaluate(a, shape, b, n, dev):
    """the instance AP counts of one batch (gspn_amd/evaluate.py) at Config(istrain=False)'s widths on synthetic masks: the two kernels, the
    same counts in torch on the device in front of the same matching kernel, and the two kernels replayed from a captured graph"""
    from gspn_amd import evaluate as EV
    from gspn_amd import graph
    from gspn_amd import rpointnet as RP
    cfg = RP.Config(istrain=False)
    r, c, g = cfg.DETECTION_MAX_INSTANCES, cfg.NUM_CATEGORY, 100
    gen = torch.Generator().manual_seed(23)
    cuts = torch.sort(torch.randint(0, n, (b, g - 1), generator=gen), 1)[0]
    group = torch.searchsorted(cuts, torch.arange(n).expand(b, n).contiguous()).int()          # g runs of points, about 1 % of the scene each
    seg_of = torch.randint(0, c, (b, g), generator=gen).int()
    seg = torch.gather(seg_of, 1, group.long())
    rows = torch.randint(0, g, (b, r), generator=gen)
    masks = ((group.unsqueeze(1) == rows.unsqueeze(-1)) & (torch.rand(b, r, n, generator=gen) < 0.85)) | (torch.rand(b, r, n, generator=gen) < 0.001)
    pred_class = torch.gather(seg_of, 1, rows)
    confidence = torch.where(torch.rand(b, r, generator=gen) < 0.5, 1.0, 0.97).float()
    count = torch.full((b,), 3 * r // 4, dtype=torch.int32)
    masks, pred_class, seg, group, confidence, count = (t.to(dev).contiguous() for t in (masks.to(torch.uint8), pred_class, seg, group, confidence, count))
    ours = EV.instance_overlaps(masks, pred_class, seg, group, c, g)
    theirs = instance_counts_torch(masks, pred_class, seg, group, c, g)

    def kernels():
        return EV.instance_match(*EV.instance_overlaps(masks, pred_class, seg, group, c, g)[:3], pred_class, confidence, count, ours[3])

    def torch_form():
        inter, void, size, gt = instance_counts_torch(masks, pred_class, seg, group, c, g)
        return EV.instance_match(inter, void, size, pred_class, confidence, count, gt)

    res = {"mask_density": round(float((masks != 0).float().mean()), 5), "counts_equal": all(bool(torch.equal(x, y)) for x, y in zip(ours, theirs)),
           "records": [int(v.sum()) for v in kernels()[:2]]}
    st = {}
    step = graph.CapturedStep(lambda: st.update(out=kernels()))
    res.update(timed_alternating({"instance_overlaps": lambda: EV.instance_overlaps(masks, pred_class, seg, group, c, g),
                                  "counts_torch_on_device": lambda: instance_counts_torch(masks, pred_class, seg, group, c, g),
                                  "overlaps_and_match": kernels, "torch_counts_and_match": torch_form,
                                  "overlaps_and_match_captured": step.replay}, a.warmup, a.iters))
    print(json.dumps({"shape": shape, "measure": "evaluate", "rows": r, "groups": g, "categories": c, "thresholds": len(EV.DEFAULT_OVERLAPS),
                      "iters": a.iters, **res}), flush=True)


def measure_train(a, shape, b, n, dev):
    """train.py's per-step work around the network: DeviceDataset.batch (one gspn_batch_assemble call) against the same batch made with
    index_select + dataset.augment_and_box (given the same R and t on the device: its best case; it has no permutation, so the
    like-for-like pair is permute=0), and a captured SPN training step that accumulates its loss terms on the device against the same
    step with a per-step host read of them (train.py:283-285)."""
    import time
    from gspn_amd import dataset
    from gspn_amd import rpointnet as RP
    from gspn_amd import train as T
    cfg = RP.Config()
    cfg.BATCH_SIZE = b
    scenes = 2 * b
    d = {k: torch.from_numpy(v).to(dev) for k, v in
         synth.spn_batch(a.kind, scenes, n, cfg.NUM_GROUP, cfg.NUM_POINT_INS, cfg.NUM_CATEGORY, seed0=7).items()}
    ngroup = torch.full((scenes,), cfg.NUM_GROUP, dtype=torch.int32, device=dev)
    make = lambda **kw: T.DeviceDataset(d["pc"], d["color"], d["group_label"], d["seg_label"], d["pc_ins"], ngroup, **kw)
    idx = torch.arange(b - 1, 2 * b - 1, dtype=torch.int32, device=dev)
    seed = torch.tensor([7], dtype=torch.int64, device=dev)
    plain, full = make(is_augment=True, permute_points=False), make(is_augment=True, permute_points=True)
    out_plain, out_full = plain.batch(idx, seed), full.batch(idx, seed)
    rot, tr, idx_long = out_plain["rotation"], out_plain["translation"], idx.long()
    group, seg = d["group_label"].int(), d["seg_label"].int()

    def chain():
        pc, color = d["pc"].index_select(0, idx_long), d["color"].index_select(0, idx_long)
        g, s = group.index_select(0, idx_long), seg.index_select(0, idx_long)
        pc, pc_ins, indicator, bbox = dataset.augment_and_box(pc, d["pc_ins"].index_select(0, idx_long), ngroup.index_select(0, idx_long), rot, tr)
        return pc, color, pc_ins, g, indicator, s, bbox, torch.ones((b, n), device=dev)

    want = chain()
    same = all(bool(torch.equal(out_plain[k], w)) for k, w in
               zip(("pc", "color", "pc_ins", "group_label", "group_indicator", "seg_label", "bbox_ins", "smpw"), want))
    res = timed_alternating({"batch_assemble": lambda: plain.batch(idx, seed, out=out_plain),
                             "batch_assemble_with_permutation": lambda: full.batch(idx, seed, out=out_full),
                             "index_select_augment_and_box": chain}, a.warmup, a.iters)
    print(json.dumps({"shape": shape, "kind": a.kind, "measure": "train_batch", "groups": cfg.NUM_GROUP, "points_per_instance": cfg.NUM_POINT_INS,
                      "equal_to_the_chain": same, "iters": a.iters, **res}), flush=True)

    # the captured step, the loss terms summed on the device or read per step
    trainer = T.Trainer(cfg, make(is_augment=True, permute_points=True), make(is_augment=False, permute_points=False), seed=1, captured=True)
    batches = [list(range(k, k + b)) for k in range(0, scenes, b)]
    read = lambda info: [float(v) for v in info["terms"].values()]

    def steps(hook, count):
        trainer.on_step = hook
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(count):
            trainer.train_step(batches[k % len(batches)])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / count

    steps(None, a.warmup + 2)
    ts = {"device_sums": [], "host_read_per_step": []}
    for _ in range(5):
        ts["device_sums"].append(steps(None, a.iters))
        ts["host_read_per_step"].append(steps(read, a.iters))
    trainer.sums.read()
    print(json.dumps({"shape": shape, "kind": a.kind, "measure": "train_step", "terms": len(trainer.terms), "steps_per_block": a.iters,
                      "includes": "batch assembly, geometry, graph replay, optimiser",
                      **{k: {"median_ms": round(sorted(v)[len(v) // 2], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
                         for k, v in ts.items()}}), flush=True)


DATA_PREP_SCANS = 8
DATA_PREP_NSAMPLE = 30000           # data_prep.py:65


def measure_data_prep(a, shape, b, n, dev):
    """data_prep.py's two computations (gspn_amd/data_prep.py); the shape is not used: the inputs have the reference's sizes.
    segment_labels at one scan-sized input (150000 vertices, 3000 segments, 40 groups) against the reference's host loop restated in numpy
    (wall clock, it runs on the host), and downsample_scans at batch 1, 2, 4, 8 over eight synthetic scans of 100000-200000 points against
    eight single farthest_point_sample calls with their gathers -- the form the library offered before -- alternating in one process."""
    import time
    from gspn_amd import data_prep
    rng = np.random.default_rng(17)
    nv, nseg, ngroup = 150000, 3000, 40
    seg = rng.integers(0, nseg, nv)
    owner = rng.integers(0, ngroup + 4, nseg)                                     # >= ngroup: in no group
    groups = [(g, np.nonzero(owner == g)[0]) for g in range(ngroup)]

    def host_loop():
        out = np.zeros(seg.shape) - 1
        errors = 0
        for object_id, segments in groups:
            for segment in segments:
                at = np.where(seg == segment)
                if not all(out[at] == -1):
                    errors += 1
                out[at] = object_id
        return out.astype(np.int64), errors

    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        want, errors = host_loop()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    d_seg = torch.from_numpy(seg.astype(np.int32)).to(dev)
    d_ps = torch.from_numpy(np.concatenate([s for _, s in groups]).astype(np.int32)).to(dev)
    d_po = torch.from_numpy(np.concatenate([np.full(len(s), g) for g, s in groups]).astype(np.int32)).to(dev)
    label, conflicts = data_prep.segment_labels(d_seg, d_ps, d_po, nseg)
    labels_equal = bool(np.array_equal(label.cpu().numpy(), want)) and int(conflicts.item()) == errors
    res = timed_alternating({"segment_labels": lambda: data_prep.segment_labels(d_seg, d_ps, d_po, nseg)}, a.warmup, a.iters)
    res["host_loop"] = {"median_ms": round(sorted(host_ms)[1], 2), "min_ms": round(min(host_ms), 2), "max_ms": round(max(host_ms), 2)}

    sizes = [100000 + (100000 * i) // (DATA_PREP_SCANS - 1) for i in range(DATA_PREP_SCANS)]
    order = np.random.default_rng(3).permutation(DATA_PREP_SCANS)                  # the caller's order is not the order of size
    scans = []
    for i in order:
        xyz = synth.cloud_d(sizes[i], 50 + int(i)) * np.array([8.0, 6.0, 3.0], np.float32)          # a metre-scale room
        r = np.random.default_rng(60 + int(i))
        scans.append(tuple(torch.from_numpy(v).to(dev) for v in (xyz, r.integers(0, 256, (sizes[i], 3)).astype(np.uint8),
                                                                  r.integers(0, 40, sizes[i]).astype(np.int32), r.integers(-1, 30, sizes[i]).astype(np.int32))))

    def single_calls():
        out = []
        for scan in scans:
            pick = farthest_point_sample(DATA_PREP_NSAMPLE, scan[0][None])[0].long()
            out.append(tuple(t[pick] for t in scan))
        return out

    base = single_calls()
    torch.cuda.synchronize()
    fns, same = {"eight_single_calls": single_calls}, {}
    for batch in (1, 2, 4, 8):
        got = data_prep.downsample_scans(scans, DATA_PREP_NSAMPLE, batch)
        same["batch_%d" % batch] = all(bool(torch.equal(x, y)) for p, q in zip(base, got) for x, y in zip(p, q))
        fns["downsample_scans_batch_%d" % batch] = (lambda k: lambda: data_prep.downsample_scans(scans, DATA_PREP_NSAMPLE, k))(batch)
    res.update(timed_alternating(fns, a.warmup, a.iters))
    print(json.dumps({"measure": "data_prep", "vertices": nv, "segments": nseg, "pairs": int(d_ps.shape[0]), "conflicts": errors,
                      "labels_equal_the_host_loop": labels_equal, "scan_sizes": [sizes[i] for i in order], "nsample": DATA_PREP_NSAMPLE,
                      "picks_equal_the_single_calls": same, "iters": a.iters, **res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points-per-instance", type=int, default=512)  # npoint_ins of --measures dataset (dataset.py:14)
    ap.add_argument("--measures", default="step,full_fwd,nn,spn")
    ap.add_argument("--shapes", default="2x18000,8x32768")
    ap.add_argument("--kind", default="S")
    ap.add_argument("--seed-points", type=int, default=128)          # shape_proposal_net's nsmp
    ap.add_argument("--sem-points", type=int, default=1024)          # model_rpointnet.py:345
    ap.add_argument("--categories", type=int, default=20)
    ap.add_argument("--crop-channels", type=int, default=1024)       # feature channels of points_cropping in --measures roi
    ap.add_argument("--lift-vertices", default="150000,500000")     # scan sizes of --measures lift, beside the scene's own points
    ap.add_argument("--lift-torch-max", type=int, default=150000)   # the largest scan the torch formulation of --measures lift is run on
    ap.add_argument("--unmold-chunk", type=int, default=4)          # ROIs per slice of the torch formulation in --measures detect
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ns, nm, ncat = a.seed_points, a.sem_points, a.categories
    measures = a.measures.split(",")
    for shape in a.shapes.split(","):
        b, n = (int(v) for v in shape.split("x"))
        if "spn" in measures:
            measure_spn(a, shape, b, n, dev)
        if "roi" in measures:
            measure_roi(a, shape, b, n, dev)
        if "detect" in measures:
            measure_detect(a, shape, b, n, dev)
        if "heads" in measures:
            measure_heads(a, shape, b, n, dev)
        if "infer" in measures:
            measure_infer(a, shape, b, n, dev)
        if "train_heads" in measures:
            measure_train_heads(a, shape, b, n, dev)
        if "dataset" in measures:
            measure_dataset(a, shape, b, n, dev)
        if "predict" in measures:
            measure_predict(a, shape, b, n, dev)
        if "lift" in measures:
            measure_lift(a, shape, b, n, dev)
        if "segments" in measures:
            measure_segments(a, shape, b, n, dev)
        if "mask_nms" in measures:
            measure_mask_nms(a, shape, b, n, dev)
        if "components" in measures:
            measure_components(a, shape, b, n, dev)
        if "holes" in measures:
            measure_holes(a, shape, b, n, dev)
        if "train" in measures:
            measure_train(a, shape, b, n, dev)
        if "evaluate" in measures:
            measure_evaluate(a, shape, b, n, dev)
        if "data_prep" in measures:
            measure_data_prep(a, shape, b, n, dev)
        if not set(measures) & {"step", "full_fwd", "nn"}:
            continue
        xyz = torch.from_numpy(synth.batch(a.kind, b, n)).to(dev)
        col = torch.rand(b, n, 3, device=dev)
        tf_util.set_variable_store(tf_util.VariableStore(device=dev, seed=1))
        params = []

        def step(shared):
            def run():
                for p in params:
                    p.grad = None
                geo = S.spn_geometry(xyz, ns, nm, points=col) if shared else None
                ep = trunks(xyz, col, ns, nm, ncat, True, False, 'training', geo)
                (ep['shift_pred_seed_4d'].square().mean() + ep['sem_class_logits'].square().mean()).backward()
            return run

        step(False)()
        params[:] = tf_util.get_variable_store().parameters()
        if "step" in measures:
            res = {"inline_geometry": timed(step(False), a.warmup, a.iters), "shared_geometry": timed(step(True), a.warmup, a.iters)}
            print(json.dumps({"shape": shape, "kind": a.kind, "measure": "step", **res}), flush=True)

        def full(nested):
            def run():
                with torch.no_grad():
                    trunks(xyz, col, ns, nm, ncat, False, True, 'inference', S.spn_geometry(xyz, ns, nm, True, points=col, nested=nested))
            return run

        if "full_fwd" in measures:
            res = {"per_level_three_nn": timed(full(False), a.warmup, a.iters), "three_nn_nested": timed(full(True), a.warmup, a.iters)}
            print(json.dumps({"shape": shape, "kind": a.kind, "measure": "full_fwd", **res}), flush=True)
        if "nn" not in measures:
            continue

        # the dense 3-NN alone, on the geometry spn_geometry builds
        fps, order, cur, lv = [], None, xyz, []
        for npoint, _, _, _ in S.SPN_SA_SPEC:
            f, o = farthest_point_sample(npoint, cur, return_order=True)
            order = o if order is None else order
            fps.append(f)
            cur = gather_point(cur, f)
            lv.append(cur)
        local = nested_local_maps(lv[0].shape[1], fps[1:])
        res = {"per_level_three_nn": timed(lambda: [three_nn(xyz, lk, order=order) for lk in lv], a.warmup, a.iters),
               "three_nn_nested": timed(lambda: three_nn_nested(xyz, lv[0], local, order=order), a.warmup, a.iters)}
        print(json.dumps({"shape": shape, "kind": a.kind, "measure": "nn", **res}), flush=True)


if __name__ == "__main__":
    main()
