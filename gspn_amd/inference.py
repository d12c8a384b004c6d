"""R-PointNet inference as its users call it: rpointnet_inference is models/model_rpointnet.py:1064-1221 for mode='inference', from a scene
batch to `detections` and `rpointnet_mask_selected`, chained from the parts of rpointnet.py (shape_proposal_net, nms_3d, gather_selection,
mask_selection_gen_batch, fpn_features, the two heads, refine_detections_batch, select_segmentation) in the reference's order, with its
scopes, variable creation order and end_points keys.

One step has a form of its own.  The reference appends fb_prob (1 column) and sem_prob (NUM_CATEGORY columns) to the feature tensor before
points_cropping (:1144), splits them off again and only averages them over each ROI's points (:1146-1150).  crop_mean (gspn_crop_mean of
csrc/crop_mean.hip) takes that average from the narrow table directly, so the cropped tensor stays as wide as the features (1024 at the
reference's widths, which crop_linear still takes) and the twenty extra columns are never cropped.

Everything runs under torch.no_grad(); every shape is static and, with the geometry, the valid-instance index and a device seed prepared
outside, nothing reads a value back to the host: the whole call captures in a graph.CapturedStep.  No CPU fallback."""
import torch

from . import _lib as L
from .detect import first_max_column, nearest_in_sets, refine_detections_batch, select_segmentation
from .heads import classification_head, fpn_features, segmentation_head
from .roi import mask_selection_gen_batch, nms_3d, points_cropping, scene_seed_tensor, seed_tensor
from .shape_proposal import shape_proposal_net
from .spn_boxes import box_shrink
from .tf_grouping import group_point

__all__ = ["crop_mean", "rpointnet_inference", "CROP_MEAN_MAX_C"]

CROP_MEAN_MAX_C = 64          # CM_MAX_C of csrc/crop_mean.hip: one lane per column, at most a wave per gathered row


def crop_mean(table, masks_selection_idx):
    """The mean of table's rows over each ROI's points (:1146-1150 without the crop).  table (B, N, C), masks_selection_idx (B, R, P) int32,
    scene-local, a value outside [0, N) clamped -> (B, R, C): out[b, r] = mean_j table[b, idx[b, r, j]].  The all-zero index rows of padding
    ROIs average point 0, as in the reference.  Summed in double in a fixed order and rounded once: the same bits on every call.
    No gradient (inputs are detached).  Raises NotImplementedError for C > 64, before anything has run."""
    idx = L.need(masks_selection_idx.detach(), torch.int32, 3, "masks_selection_idx")
    table = L.need(table.detach(), torch.float32, 3, "table")
    b, n, c = table.shape
    r, p = idx.shape[1:]
    if idx.shape[0] != b:
        raise ValueError("crop_mean: table (B, N, C) and masks_selection_idx (B, R, P) must share B, got %s and %s"
                         % (tuple(table.shape), tuple(idx.shape)))
    if min(b, n, c, r, p) <= 0:
        raise ValueError("crop_mean: empty table %s or index tensor %s" % (tuple(table.shape), tuple(idx.shape)))
    if c > CROP_MEAN_MAX_C:
        raise NotImplementedError("crop_mean: C <= %d (got %d)" % (CROP_MEAN_MAX_C, c))
    out = torch.empty((b, r, c), dtype=torch.float32, device=table.device)
    with torch.cuda.device(table.device):
        L.check(L.lib().gspn_crop_mean(b, n, r, p, c, L.ptr(table), L.ptr(idx), L.ptr(out), L.stream()), "crop_mean")
    return out


def _point_probabilities(pc, end_points):
    """:1136-1141.  (B, N, 1 + NUM_CATEGORY): the foreground probability of each point's nearest seed (tf.argmin's first minimum of
    (dx*dx + dy*dy) + dz*dz: nearest_in_sets with one set per scene) and the softmax of its semantic logits"""
    midx = nearest_in_sets(pc, end_points['pc_seed'])[:, 0].long()                                      # (B, N)
    fb_prob = torch.gather(end_points['fb_prob'][:, :, 1], 1, midx)
    sem_prob = torch.softmax(end_points['sem_class_logits'], -1)
    return torch.cat((fb_prob.unsqueeze(-1), sem_prob), -1)


def rpointnet_inference(pc, color, pc_ins, group_label, group_indicator, seg_label, bbox_ins, config, is_training=False, bn_decay=None, *,
                        geometry=None, valid_idx=None, seed=0, fused_crop=False, scene_seeds=None):
    """:1064-1221 for mode='inference'.  pc, color (B, N, 3), pc_ins (B, NUM_GROUP, NUM_POINT_INS, 3), group_label, seg_label (B, N),
    group_indicator (B, NUM_GROUP), bbox_ins (B, NUM_GROUP, 6) -> end_points: shape_proposal_net's (with return_fullfea) plus
      group_label, seg_label, seg_label_per_group, bbox_ins                                                       (:1194-1197)
      selected_indices (B, M) int32, spn_rois, rois (B, M, 6), rpointnet_class_logits, rpointnet_class (B, M, NUM_CATEGORY),
      rpointnet_bbox (B, M, NUM_CATEGORY, 6), detections (B, D, 8), rpointnet_mask (B, D, P, NUM_CATEGORY), rpointnet_mask_selected (B, D, P),
      pc_coord_cropped_final_unnormalized (B, D, P, 3)                                                            (:1211-1220)
      fb_prob_cropped, sem_prob_cropped (B, M)                                                                    (:1149, :1163)
    with M = SPN_NMS_MAX_SIZE_INFERENCE, D = DETECTION_MAX_INSTANCES, P = NUM_POINT_INS_MASK, and, as extensions, mask_selection_idx
    (B, M, P) int32, rois_final (B, D, 6) and mask_selection_idx_final (B, D, P) int32: the crops behind the two heads.
    The proposal net runs with is_training=False and bn_decay=None whatever is passed (:1070); is_training / bn_decay reach the FPN layers
    and the heads, as in the reference.  Extensions: geometry -- spn_geometry(pc, NUM_SAMPLE, 1024, True, points=color) -- and valid_idx
    -- valid_instances(group_indicator) -- as in shape_proposal_net; seed -- a Python int or a one-element int64 device tensor, the first
    crop draws with seed, the second with seed + 1 (added on the device); fused_crop -- the heads' first layer as crop_linear instead of
    over the materialised crop (off until it is measured); scene_seeds -- a contiguous (B,) int64 device tensor, a seed per
    scene: the first crop draws with scene_seeds, the second with scene_seeds + 1 (added on the device), seed is ignored, and a scene's
    crops no longer depend on the batch it is run in or on its slot there (tester.py batches test scenes on this).
    Variables are created in the reference's order: shape_proposal_net/..., fpn1..fpn4, classification_head/..., segmentation_head/...."""
    from .rpointnet import gather_selection, seg_label_per_group
    if scene_seeds is not None:
        scene_seeds = scene_seed_tensor(scene_seeds, pc, "rpointnet_inference")
    with torch.no_grad():
        if not config.USE_COLOR:
            color = None
        end_points = shape_proposal_net(pc, color, pc_ins, group_label, group_indicator, config.NUM_CATEGORY, scope='shape_proposal_net',
                                        is_training=False, bn_decay=None, nsmp=config.NUM_SAMPLE, return_fullfea=True, mode='inference',
                                        geometry=geometry, valid_idx=valid_idx)
        end_points = {k: v.detach() for k, v in end_points.items()}                                     # dict_stop_gradient, :1071
        if config.SHRINK_BOX:
            end_points['bbox_ins_pred'] = box_shrink(end_points['bbox_ins_pred'], pc)
        per_group = seg_label_per_group(seg_label, group_label, config.NUM_GROUP)

        # proposals -> ROIs (:1079-1083, :1117-1123)
        m = int(config.SPN_NMS_MAX_SIZE_INFERENCE)
        nroi_final = int(config.DETECTION_MAX_INSTANCES)
        npoint = int(config.NUM_POINT_INS_MASK)
        normalize = bool(config.NORMALIZE_CROP_REGION)
        if scene_seeds is None:
            seed = seed_tensor(seed, pc.device)
            seed_final, scene_seeds_final = seed + 1, None
        else:
            seed_final, scene_seeds_final = seed, scene_seeds + 1
        selected_indices = nms_3d(end_points['bbox_ins_pred'], end_points['fb_prob'][:, :, 1], config.SPN_PRE_NMS_LIMIT, m,
                                  config.SPN_IOU_THRESHOLD, config.SPN_SCORE_THRESHOLD)
        spn_rois = gather_selection(end_points['bbox_ins_pred'], selected_indices, m)
        rois, mask_selection_idx = mask_selection_gen_batch(spn_rois, pc, m, config, True, seed, scene_seeds)

        # features (:1129-1132) and the per-ROI probabilities (:1136-1150)
        fea = fpn_features(end_points, is_training, bn_decay)
        center_pos = end_points['center_pos']
        prob_cropped = crop_mean(_point_probabilities(pc, end_points), mask_selection_idx)             # (B, M, 1 + NUM_CATEGORY)
        fb_prob_cropped = prob_cropped[:, :, 0].contiguous()
        sem_prob_cropped = prob_cropped[:, :, 1:]

        # classification and box refinement head (:1155-1157)
        if fused_crop:
            crop = dict(pc=pc, pc_fea=fea, pc_center=center_pos, rois=rois, idx=mask_selection_idx, normalize=normalize)
            coord, head_fea = None, None
        else:
            crop = None
            fea_cropped, center_cropped, coord, _ = points_cropping(pc, fea, center_pos, rois, mask_selection_idx, m, npoint, normalize)
            head_fea = torch.cat((fea_cropped, center_cropped), -1)
            del fea_cropped
        rpointnet_class_logits, rpointnet_class, rpointnet_bbox = classification_head(
            coord, head_fea, config.NUM_CATEGORY, [128, 256, 512], [256, 256], is_training, bn_decay, 'classification_head', crop=crop)
        del coord, head_fea

        # the semantic probability of each ROI's own class (:1159-1162)
        midx = first_max_column(rpointnet_class_logits)
        sem_prob_cropped = torch.gather(sem_prob_cropped, 2, midx.unsqueeze(-1)).squeeze(-1)

        detections = refine_detections_batch(rois, rpointnet_class, rpointnet_bbox, pc, fb_prob_cropped, sem_prob_cropped, config)

        # the second crop (:1172-1183) and the mask head (:1186-1191)
        rois_final, mask_selection_idx_final = mask_selection_gen_batch(detections[:, :, :6], pc, nroi_final, config, False, seed_final,
                                                                        scene_seeds_final)
        if fused_crop:
            crop = dict(pc=pc, pc_fea=fea, pc_center=center_pos, rois=rois_final, idx=mask_selection_idx_final, normalize=normalize)
            coord, head_fea = None, None
            coord_unnormalized = group_point(pc, mask_selection_idx_final)
        else:
            fea_cropped, center_cropped, coord, coord_unnormalized = points_cropping(pc, fea, center_pos, rois_final, mask_selection_idx_final,
                                                                                     nroi_final, npoint, normalize)
            head_fea = torch.cat((fea_cropped, center_cropped), -1)
            del fea_cropped
        rpointnet_mask = segmentation_head(coord, head_fea, config.NUM_CATEGORY, [64, 64], [64, 128, 512], [256, 256], is_training, bn_decay,
                                           'segmentation_head', crop=crop)
        rpointnet_mask_selected = select_segmentation(torch.sigmoid(rpointnet_mask), detections[:, :, 6])

        end_points['group_label'] = group_label
        end_points['seg_label'] = seg_label
        end_points['seg_label_per_group'] = per_group
        end_points['bbox_ins'] = bbox_ins
        end_points['fb_prob_cropped'] = fb_prob_cropped
        end_points['sem_prob_cropped'] = sem_prob_cropped
        end_points['selected_indices'] = selected_indices
        end_points['spn_rois'] = spn_rois
        end_points['rois'] = rois
        end_points['rpointnet_class_logits'] = rpointnet_class_logits
        end_points['rpointnet_class'] = rpointnet_class
        end_points['rpointnet_bbox'] = rpointnet_bbox
        end_points['detections'] = detections
        end_points['rpointnet_mask'] = rpointnet_mask
        end_points['rpointnet_mask_selected'] = rpointnet_mask_selected
        end_points['pc_coord_cropped_final_unnormalized'] = coord_unnormalized
        end_points['mask_selection_idx'] = mask_selection_idx
        end_points['rois_final'] = rois_final
        end_points['mask_selection_idx_final'] = mask_selection_idx_final
        return end_points
