"""The SPN stage of models/model_rpointnet.py as its users call it: rpointnet (:1051) for TRAIN_MODULE == ['SPN'], mode='training', and the
SPN terms of get_loss (:1325), with the helpers they use (box_shrink :529, spn_target_gen :599, gather_selection :468, smooth_l1_loss
:1223, get_spn_class_loss :1232).  Same names, argument order and end_points keys as the reference.

Every shape here is static and nothing reads a value back to the host, so with the geometry, the valid-instance index and the noise
prepared outside, rpointnet + get_loss + backward capture in a graph.CapturedStep.  The ROI stage behind it -- nms_3d (:436),
detection_target_gen (:647), mask_selection_gen (:749), points_cropping (:785), box_refinement (:553), apply_box_delta (:570) -- lives in
roi.py and is re-exported here under the reference's names, and so is the detection output stage behind the heads -- refine_detections
(:818), select_segmentation (:986), unmold_segmentation (:1008), with the extensions class_nms_3d and nearest_in_sets -- which lives in
detect.py.  The heads between the two -- the FPN layers (fpn_features, :1100-1104), classification_head (:915), segmentation_head (:946),
crop_linear (their first layer fused with the crop) and the R-PointNet losses (:1251-1323, get_rpointnet_loss) -- live in heads.py and are
re-exported here as callable parts.  Inference is its own driver, rpointnet_inference (:1064-1221 for mode='inference', with crop_mean for
the per-ROI probabilities of :1146-1150), which lives in inference.py and is re-exported here.  Head training is its own driver too:
rpointnet_head_training / rpointnet_heads_from_proposals (:1070-1115, :1198-1209 for TRAIN_MODULE == ['RPOINTNET']) and
get_head_training_loss (:1325-1416 for it), which live in training.py and are re-exported here.  The prediction export stage behind
inference -- scene_predictions, write_predictions, write_ground_truth (test.py:96-129, :155-206) and semantic_iou_counts / mean_iou
(train.py:365-368, 385-386) -- lives in predict.py and is re-exported here.  rpointnet itself does not chain the
parts: with mode='inference' or 'RPOINTNET' in TRAIN_MODULE, and get_loss with 'RPOINTNET' in TRAIN_MODULE, it raises NotImplementedError
and names the function to call."""
import torch

from . import _lib as L
from .detect import (class_nms_3d, nearest_in_sets, refine_detections, refine_detections_batch, select_segmentation,
                     unmold_segmentation)
from .inference import crop_mean, rpointnet_inference
from .predict import (SCANNET_LABEL_MAP, mean_iou, scene_confidence, scene_predictions, scene_rank, semantic_iou_counts, write_ground_truth,
                      write_predictions)
from .heads import (classification_head, crop_linear, fpn_features, get_rpointnet_bbox_loss, get_rpointnet_class_loss, get_rpointnet_loss,
                    get_rpointnet_mask_loss, segmentation_head, shared_first_layers, tile_linear)
from .proposal_head import chamfer_recons_loss
from .roi import (apply_box_delta, box_point_count, box_refinement, detection_target_gen, detection_target_gen_batch, mask_selection_gen,
                  mask_selection_gen_batch, nms_3d, points_cropping, sample_points_in_boxes)
from .shape_proposal import shape_proposal_net
from .spn_boxes import box_shrink, points_bbox, spn_target_gen_batch
from .training import get_head_training_loss, rpointnet_head_training, rpointnet_heads_from_proposals

__all__ = ["Config", "box_shrink", "spn_target_gen", "spn_target_gen_batch", "gather_selection", "smooth_l1_loss", "get_spn_class_loss",
           "seg_label_per_group", "rpointnet", "get_loss", "nms_3d", "box_point_count", "sample_points_in_boxes", "detection_target_gen",
           "detection_target_gen_batch", "mask_selection_gen", "mask_selection_gen_batch", "points_cropping", "box_refinement", "apply_box_delta",
           "class_nms_3d", "refine_detections", "refine_detections_batch", "select_segmentation", "nearest_in_sets", "unmold_segmentation",
           "crop_linear", "classification_head", "segmentation_head", "fpn_features", "get_rpointnet_class_loss", "get_rpointnet_bbox_loss",
           "get_rpointnet_mask_loss", "get_rpointnet_loss", "crop_mean", "rpointnet_inference", "tile_linear", "shared_first_layers",
           "rpointnet_heads_from_proposals", "rpointnet_head_training", "get_head_training_loss", "SCANNET_LABEL_MAP", "scene_confidence",
           "scene_rank", "scene_predictions", "semantic_iou_counts", "mean_iou", "write_predictions", "write_ground_truth"]


class Config(object):
    """models/config.py's attributes with the reference's default values (training: istrain=True; the reference's constructor assigns
    the test values to locals and so changes nothing -- here istrain=False really sets them)."""
    NUM_CATEGORY = 1 + 18
    NUM_GROUP = 100
    NUM_POINT = 18000
    NUM_POINT_INS = 512
    BATCH_SIZE = 2
    NUM_SAMPLE = 256
    SPN_PRE_NMS_LIMIT = 192
    SPN_NMS_MAX_SIZE_TRAINING = 128
    SPN_NMS_MAX_SIZE_INFERENCE = 96
    SPN_IOU_THRESHOLD = 0.5
    SPN_SCORE_THRESHOLD = float('-inf')
    NUM_POINT_INS_MASK = 256
    TRAIN_ROIS_PER_IMAGE = 64
    ROI_POSITIVE_RATIO = 0.33
    BBOX_STD_DEV = (0.1, 0.1, 0.1, 0.2, 0.2, 0.2)
    NORMALIZE_CROP_REGION = True
    SHRINK_BOX = False
    USE_COLOR = True
    TRAIN_MODULE = ['SPN']
    DETECTION_MIN_CONFIDENCE = 0.7
    DETECTION_NMS_THRESHOLD = 0.1
    DETECTION_MAX_INSTANCES = 100

    def __init__(self, istrain=True):
        if not istrain:
            self.NUM_SAMPLE = 2048
            self.SPN_PRE_NMS_LIMIT = 1536
            self.SPN_NMS_MAX_SIZE_TRAINING = 512
            self.SPN_NMS_MAX_SIZE_INFERENCE = 384
            self.NUM_POINT_INS_MASK = 1024
            self.TRAIN_ROIS_PER_IMAGE = 512


def spn_target_gen(proposals, proposal_seed_class_ids, gt_class_ids, gt_boxes):
    """:599-644 with the reference's per-scene signature: proposals (S, 6), proposal_seed_class_ids (S,), gt_class_ids (G,), gt_boxes
    (G, 6) -> spn_match (S,) float32 like the reference's.  A thin wrapper of spn_target_gen_batch, which takes the whole batch in one
    launch."""
    return spn_target_gen_batch(proposals.unsqueeze(0), proposal_seed_class_ids.unsqueeze(0), gt_class_ids.unsqueeze(0),
                                gt_boxes.unsqueeze(0))[0].float()


def gather_selection(source, selected_idx, max_selected_size):
    """:468-482.  source (B, N, C), selected_idx (B, M) with -1 for "nothing" -> (B, M, C), zero rows where nothing is selected.  Static
    shapes: a gather on the clamped index and a mask instead of tf.where / scatter_nd."""
    if selected_idx.shape[1] != max_selected_size:
        raise ValueError("gather_selection: selected_idx has %d columns, max_selected_size is %d" % (selected_idx.shape[1], max_selected_size))
    idx = selected_idx.long()
    picked = torch.gather(source, 1, idx.clamp(0, source.shape[1] - 1).unsqueeze(-1).expand(-1, -1, source.shape[2]))
    return picked * (idx >= 0).unsqueeze(-1).to(source.dtype)


def smooth_l1_loss(y_true, y_pred):
    """:1223-1230"""
    diff = torch.abs(y_true - y_pred)
    less_than_one = (diff < 1.0).to(diff.dtype)
    return (less_than_one * 0.5 * diff ** 2) + (1 - less_than_one) * (diff - 0.5)


def get_spn_class_loss(fb_logits, spn_match):
    """:1232-1249.  fb_logits (B, nsmp, 2), spn_match (B, nsmp): mean cross-entropy over the proposals with spn_match != 0 (label 1 for the
    positive ones), as a masked mean with static shapes; 0 when no proposal is matched."""
    fb_logits = fb_logits.reshape(-1, 2)
    spn_match = spn_match.reshape(-1)
    valid = (spn_match != 0).to(fb_logits.dtype)
    label = (spn_match == 1).long()
    ce = torch.logsumexp(fb_logits, dim=1) - torch.gather(fb_logits, 1, label.unsqueeze(1)).squeeze(1)
    return (ce * valid).sum() / valid.sum().clamp(min=1.0)


def seg_label_per_group(seg_label, group_label, num_group):
    """:1074-1076: the mean semantic label of each group's points, rounded half to even (tf.round), (B, NUM_GROUP) int32; 0 for a group
    without points.  Labels outside [0, num_group) fall in no group, as with tf.one_hot."""
    onehot = (group_label.long().unsqueeze(-1) == torch.arange(num_group, device=group_label.device)).float()      # (B, N, G)
    total = (seg_label.float().unsqueeze(-1) * onehot).sum(1)
    return torch.round(total / (onehot.sum(1) + 1e-8)).int()


def rpointnet(pc, color, pc_ins, group_label, group_indicator, seg_label, bbox_ins, config, is_training, mode='training', bn_decay=None,
              geometry=None, noise=None, valid_idx=None):
    """:1051.  pc, color (B, N, 3), pc_ins (B, NUM_GROUP, NUM_POINT_INS, 3), group_label, seg_label (B, N), group_indicator (B, NUM_GROUP),
    bbox_ins (B, NUM_GROUP, 6) -> end_points of shape_proposal_net plus group_label, seg_label, seg_label_per_group, bbox_ins.
    geometry / noise / valid_idx (extensions) are handed on to shape_proposal_net.
    mode='inference' and 'RPOINTNET' in TRAIN_MODULE raise NotImplementedError: inference is rpointnet_inference and head training is
    rpointnet_head_training, functions of their own."""
    assert mode in ['training', 'inference']
    if mode == 'inference':
        raise NotImplementedError("rpointnet: mode='inference' is not wired into this driver: call rpointnet_inference, which chains "
                                  "fpn_features, classification_head, segmentation_head and refine_detections")
    if 'RPOINTNET' in config.TRAIN_MODULE:
        raise NotImplementedError("rpointnet: 'RPOINTNET' in TRAIN_MODULE is not wired into this driver: call rpointnet_head_training (or "
                                  "rpointnet_heads_from_proposals) with TRAIN_MODULE == ['RPOINTNET'], and get_head_training_loss")
    if 'SPN' not in config.TRAIN_MODULE:
        raise NotImplementedError("rpointnet: TRAIN_MODULE must be ['SPN']")
    if not config.USE_COLOR:
        color = None
    end_points = shape_proposal_net(pc, color, pc_ins, group_label, group_indicator, config.NUM_CATEGORY, scope='shape_proposal_net',
                                    is_training=is_training, bn_decay=bn_decay, nsmp=config.NUM_SAMPLE, return_fullfea=False, mode=mode,
                                    geometry=geometry, noise=noise, valid_idx=valid_idx)
    if config.SHRINK_BOX:
        end_points['bbox_ins_pred'] = box_shrink(end_points['bbox_ins_pred'], pc)
    end_points['group_label'] = group_label
    end_points['seg_label'] = seg_label
    end_points['seg_label_per_group'] = seg_label_per_group(seg_label, group_label, config.NUM_GROUP)
    end_points['bbox_ins'] = bbox_ins
    return end_points


def get_loss(end_points, config, alpha, smpw, mode='training'):
    """:1325, the five SPN terms (:1328-1381, :1395).  smpw (B, N): per-point weights of the semantic loss.  Returns (loss, end_points);
    end_points gains spn_match, sem_labels, spn_class_loss, recons_loss, shift_loss, sem_loss, kl_loss, loss.
    The R-PointNet terms (:1383-1392) are get_rpointnet_loss, which get_head_training_loss adds for TRAIN_MODULE == ['RPOINTNET']; here
    'RPOINTNET' in TRAIN_MODULE raises."""
    if 'RPOINTNET' in config.TRAIN_MODULE or 'SPN' not in config.TRAIN_MODULE:
        raise NotImplementedError("get_loss: only TRAIN_MODULE == ['SPN'] is implemented (for ['RPOINTNET'] call get_head_training_loss, "
                                  "which adds the R-PointNet terms of get_rpointnet_loss)")
    return _spn_loss_terms(end_points, config, alpha, smpw)


def _spn_loss_terms(end_points, config, alpha, smpw):
    """the body get_loss and get_head_training_loss share: the five SPN terms (:1328-1381), their sum (:1395) and the keys of :1405-1414"""
    nsmp_ins = config.NUM_POINT_INS
    pc_ins_centered_seed = L.need(end_points['pc_ins_centered_seed'], torch.float32, 4, "pc_ins_centered_seed")
    bbox_size = points_bbox(pc_ins_centered_seed)[:, :, 3:].unsqueeze(2)                                  # (B, nsmp, 1, 3)
    radius = 1e-8 + torch.sqrt(torch.sum(torch.square(bbox_size / 2), dim=-1, keepdim=True))              # (B, nsmp, 1, 1)
    shift_gt_seed = end_points['pc_ins_center_seed'] - end_points['pc_seed'].unsqueeze(2)                 # (B, nsmp, 1, 3)
    shift_dist = torch.sqrt(torch.sum(torch.square(shift_gt_seed), 3, keepdim=True) + 1e-8)
    shift_gt_seed_normalized_4d = torch.cat((shift_gt_seed / shift_dist, shift_dist / radius), -1)
    shift_pred_4d = end_points['shift_pred_seed_4d'].unsqueeze(2)
    shift_pred_seed_normalized_4d = torch.cat((shift_pred_4d[:, :, :, :3], shift_pred_4d[:, :, :, 3:] / radius), -1)

    # foreground / background loss (:1336-1344)
    seg_label = end_points['seg_label']
    ind_seed = end_points['ind_seed']
    fb_score_gt = (gather_selection(seg_label.unsqueeze(-1), ind_seed, ind_seed.shape[1]).squeeze(-1) > 0).float()      # (B, nsmp)
    spn_match = spn_target_gen_batch(end_points['bbox_ins_pred'], fb_score_gt, (end_points['seg_label_per_group'] > 0).float(),
                                     end_points['bbox_ins'])
    end_points['spn_match'] = spn_match
    spn_class_loss = get_spn_class_loss(end_points['fb_logits'], spn_match)

    # reconstruction loss (:1347-1355)
    pc_ins_pred_normalized = (end_points['pc_ins_pred'] / radius).reshape(-1, nsmp_ins, 3)
    pc_ins_gt_normalized = ((pc_ins_centered_seed + shift_gt_seed) / radius).reshape(-1, nsmp_ins, 3)
    recon_valid_mask = fb_score_gt.reshape(-1).detach()
    recons_loss = chamfer_recons_loss(pc_ins_pred_normalized, pc_ins_gt_normalized, recon_valid_mask)
    denom = recon_valid_mask.sum() + 1e-8

    # shift loss (:1358-1360)
    shift_loss = smooth_l1_loss(shift_gt_seed_normalized_4d, shift_pred_seed_normalized_4d).sum(-1)
    shift_loss = (shift_loss.reshape(-1) * recon_valid_mask).sum() / denom

    # semantic loss (:1363-1372): tf.losses' default reduction, the weighted sum over the number of non-zero weights
    ind_sem = end_points['ind_sem'].long()
    logits = end_points['sem_class_logits']
    sem_labels = torch.gather(seg_label, 1, ind_sem).int()
    weights = torch.gather(smpw, 1, ind_sem).to(logits.dtype)
    label = sem_labels.long().clamp(0, logits.shape[-1] - 1)
    ce = torch.logsumexp(logits, dim=-1) - torch.gather(logits, 2, label.unsqueeze(-1)).squeeze(-1)
    sem_loss = (ce * weights).sum() / (weights != 0).sum().to(logits.dtype).clamp(min=1.0)
    end_points['sem_labels'] = sem_labels

    # KL loss (:1375-1381)
    mean, log_var, cmean, clog_var = end_points['mean'], end_points['log_var'], end_points['cmean'], end_points['clog_var']
    kl_loss = 0.5 * torch.mean(log_var - clog_var + (torch.exp(clog_var) + (mean - cmean) ** 2) / torch.exp(log_var) - 1.0, 2)
    kl_loss = (kl_loss.reshape(-1) * recon_valid_mask).sum() / denom

    loss = kl_loss * alpha + recons_loss + shift_loss + spn_class_loss + sem_loss                         # :1395
    end_points['spn_class_loss'] = spn_class_loss
    end_points['recons_loss'] = recons_loss
    end_points['shift_loss'] = shift_loss
    end_points['sem_loss'] = sem_loss
    end_points['kl_loss'] = kl_loss
    end_points['loss'] = loss
    return loss, end_points
