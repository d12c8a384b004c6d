"""R-PointNet head training as its users call it: models/model_rpointnet.py with TRAIN_MODULE == ['RPOINTNET'], mode='training'.

rpointnet_head_training is :1064-1115 and :1194-1209 for that configuration: the proposal net frozen in evaluation mode behind
dict_stop_gradient (:1070-1071), then rpointnet_heads_from_proposals -- seg_label_per_group, nms_3d, gather_selection,
detection_target_gen_batch, fpn_features, the crop and the two heads, in the reference's order with its scopes, variable creation order and
end_points keys.  get_head_training_loss is :1325-1416 for it: the five SPN terms are computed and stored as the reference does, and the
loss is the sum of the three R-PointNet terms (:1399).

Three switches, all off by default, pick other forms of the same arithmetic on the same variables (heads.py): fused_crop -- the heads' first
layer as crop_linear instead of over the materialised crop; shared_first -- both heads' first layers as one crop_linear over the common
crop (implies fused_crop); split_post -- the mask head's conv_post_0 as tile_linear, without concat(tile(global), local).

Every shape is static and, with the geometry, the valid-instance index, the noise and a device seed prepared outside, nothing reads a value
back to the host: forward + loss + backward capture in a graph.CapturedStep.  No CPU fallback."""
import torch

from . import tf_util
from .heads import (classification_head, declare_classification_head, fpn_features, get_rpointnet_loss, segmentation_head,
                    shared_first_layers)
from .pointnet_util import _mlp_layers
from .roi import detection_target_gen_batch, nms_3d, points_cropping, seed_tensor
from .shape_proposal import shape_proposal_net
from .spn_boxes import box_shrink

__all__ = ["rpointnet_heads_from_proposals", "rpointnet_head_training", "get_head_training_loss"]

_CLS_MLPS = ([128, 256, 512], [256, 256])                          # :1110
_SEG_MLPS = ([64, 64], [64, 128, 512], [256, 256])                 # :1115


def _require_heads_only(config, what):
    modules = list(config.TRAIN_MODULE)
    if 'RPOINTNET' not in modules:
        raise NotImplementedError("%s: TRAIN_MODULE must be ['RPOINTNET'], got %s (for ['SPN'] call rpointnet and get_loss)" % (what, modules))
    if 'SPN' in modules:
        raise NotImplementedError("%s: TRAIN_MODULE must be ['RPOINTNET'], got %s -- with 'SPN' in it the reference calls the proposal net "
                                  "with return_fullfea=False (:1068) and then reads sem_fea_full_l1..l4 (:1100-1103), which that call does "
                                  "not return: the combination cannot run there either" % (what, modules))


def rpointnet_heads_from_proposals(end_points, pc, group_label, seg_label, bbox_ins, config, is_training, bn_decay=None, *, seed=0,
                                   fused_crop=False, shared_first=False, split_post=False):
    """:1074-1115 and :1194-1209 for mode='training', TRAIN_MODULE == ['RPOINTNET'], from the end_points of a shape_proposal_net call made
    with return_fullfea=True (detached here: dict_stop_gradient, :1071).  pc (B, N, 3), group_label, seg_label (B, N), bbox_ins
    (B, NUM_GROUP, 6) -> end_points plus
      group_label, seg_label, seg_label_per_group, bbox_ins                                                       (:1194-1197)
      selected_indices (B, M) int32, spn_rois (B, M, 6), rois (B, R, 6), target_class_ids (B, R), target_bbox (B, R, 6),
      target_mask_selection_idx (B, R, P) int32, target_mask (B, R, P) bool, rpointnet_class_logits, rpointnet_class (B, R, NUM_CATEGORY),
      rpointnet_bbox (B, R, NUM_CATEGORY, 6), rpointnet_mask (B, R, P, NUM_CATEGORY)                              (:1199-1209)
    with M = SPN_NMS_MAX_SIZE_TRAINING, R = TRAIN_ROIS_PER_IMAGE, P = NUM_POINT_INS_MASK.
    Variables are created in the reference's order: fpn1..fpn4, classification_head/..., segmentation_head/....
    Extensions: seed -- a Python int or a one-element int64 device tensor, read by detection_target_gen_batch on the device; fused_crop,
    shared_first (implies fused_crop; a shape crop_linear declines at 192 columns runs the two first layers separately), split_post --
    the module's three forms, off until they are measured."""
    from .rpointnet import gather_selection, seg_label_per_group
    _require_heads_only(config, "rpointnet_heads_from_proposals")
    end_points = {k: v.detach() for k, v in end_points.items()}                                         # dict_stop_gradient, :1071
    if config.SHRINK_BOX:
        end_points['bbox_ins_pred'] = box_shrink(end_points['bbox_ins_pred'], pc)
    per_group = seg_label_per_group(seg_label, group_label, config.NUM_GROUP)

    # proposals -> ROIs and their targets (:1079-1094)
    m = int(config.SPN_NMS_MAX_SIZE_TRAINING)
    nroi = int(config.TRAIN_ROIS_PER_IMAGE)
    npoint = int(config.NUM_POINT_INS_MASK)
    normalize = bool(config.NORMALIZE_CROP_REGION)
    seed = seed_tensor(seed, pc.device)
    selected_indices = nms_3d(end_points['bbox_ins_pred'], end_points['fb_prob'][:, :, 1], config.SPN_PRE_NMS_LIMIT, m,
                              config.SPN_IOU_THRESHOLD, config.SPN_SCORE_THRESHOLD)
    spn_rois = gather_selection(end_points['bbox_ins_pred'], selected_indices, m)
    rois, target_class_ids, target_bbox, target_mask_selection_idx, target_mask = detection_target_gen_batch(
        spn_rois, per_group, bbox_ins, group_label, pc, config, seed)

    # features and the crop (:1100-1105)
    fea = fpn_features(end_points, is_training, bn_decay)
    center_pos = end_points['center_pos']
    cls_first = seg_first = None
    if fused_crop or shared_first:
        crop = dict(pc=pc, pc_fea=fea, pc_center=center_pos, rois=rois, idx=target_mask_selection_idx, normalize=normalize)
        coord, head_fea = None, None
        if shared_first:
            # every variable of the classification head first, so that segmentation_head/conv_prev_0 comes behind them as in the reference
            cin = fea.shape[2] + 6
            cls_layer = declare_classification_head(cin, config.NUM_CATEGORY, _CLS_MLPS[0], _CLS_MLPS[1], 'classification_head')
            with tf_util.variable_scope('segmentation_head'):
                seg_layer = _mlp_layers(_SEG_MLPS[0][:1], cin, 'conv_prev_', True)[0]
            try:
                cls_first, seg_first = shared_first_layers(crop, cls_layer, seg_layer, is_training, bn_decay)
            except NotImplementedError:                  # a shape crop_linear declines at the joint width: one first layer per head
                pass
    else:
        crop = None
        fea_cropped, center_cropped, coord, _ = points_cropping(pc, fea, center_pos, rois, target_mask_selection_idx, nroi, npoint, normalize)
        head_fea = torch.cat((fea_cropped, center_cropped), -1)
        del fea_cropped

    # the two heads (:1108-1115)
    rpointnet_class_logits, rpointnet_class, rpointnet_bbox = classification_head(
        coord, head_fea, config.NUM_CATEGORY, _CLS_MLPS[0], _CLS_MLPS[1], is_training, bn_decay, 'classification_head',
        crop=crop if cls_first is None else dict(crop, first=cls_first))
    rpointnet_mask = segmentation_head(
        coord, head_fea, config.NUM_CATEGORY, _SEG_MLPS[0], _SEG_MLPS[1], _SEG_MLPS[2], is_training, bn_decay, 'segmentation_head',
        crop=crop if seg_first is None else dict(crop, first=seg_first), split_post=split_post)

    end_points['group_label'] = group_label
    end_points['seg_label'] = seg_label
    end_points['seg_label_per_group'] = per_group
    end_points['bbox_ins'] = bbox_ins
    end_points['selected_indices'] = selected_indices
    end_points['spn_rois'] = spn_rois
    end_points['rois'] = rois
    end_points['target_class_ids'] = target_class_ids
    end_points['target_bbox'] = target_bbox
    end_points['target_mask_selection_idx'] = target_mask_selection_idx
    end_points['target_mask'] = target_mask
    end_points['rpointnet_class_logits'] = rpointnet_class_logits
    end_points['rpointnet_class'] = rpointnet_class
    end_points['rpointnet_bbox'] = rpointnet_bbox
    end_points['rpointnet_mask'] = rpointnet_mask
    return end_points


def rpointnet_head_training(pc, color, pc_ins, group_label, group_indicator, seg_label, bbox_ins, config, is_training, bn_decay=None, *,
                            geometry=None, valid_idx=None, noise=None, seed=0, fused_crop=False, shared_first=False, split_post=False):
    """:1064-1115, :1194-1209 for mode='training', TRAIN_MODULE == ['RPOINTNET'].  pc, color (B, N, 3), pc_ins
    (B, NUM_GROUP, NUM_POINT_INS, 3), group_label, seg_label (B, N), group_indicator (B, NUM_GROUP), bbox_ins (B, NUM_GROUP, 6) ->
    end_points: shape_proposal_net's (with return_fullfea, mode='training': the pc_ins-dependent keys get_head_training_loss reads are
    there) plus the keys of rpointnet_heads_from_proposals.
    The proposal net runs under no_grad with is_training=False and bn_decay=None whatever is passed (:1070-1071): none of its variables
    gets a gradient and its moving statistics do not move.  is_training / bn_decay reach the FPN layers and the heads.
    Extensions: geometry -- spn_geometry(pc, NUM_SAMPLE, 1024, True, points=color) --, valid_idx -- valid_instances(group_indicator) --
    and noise as in shape_proposal_net; seed, fused_crop, shared_first, split_post as in rpointnet_heads_from_proposals.
    Variables are created in the reference's order: shape_proposal_net/..., fpn1..fpn4, classification_head/..., segmentation_head/....
    Raises NotImplementedError unless 'RPOINTNET' is in TRAIN_MODULE and 'SPN' is not."""
    _require_heads_only(config, "rpointnet_head_training")
    if not config.USE_COLOR:
        color = None
    with torch.no_grad():
        end_points = shape_proposal_net(pc, color, pc_ins, group_label, group_indicator, config.NUM_CATEGORY, scope='shape_proposal_net',
                                        is_training=False, bn_decay=None, nsmp=config.NUM_SAMPLE, return_fullfea=True, mode='training',
                                        geometry=geometry, noise=noise, valid_idx=valid_idx)
    return rpointnet_heads_from_proposals(end_points, pc, group_label, seg_label, bbox_ins, config, is_training, bn_decay, seed=seed,
                                          fused_crop=fused_crop, shared_first=shared_first, split_post=split_post)


def get_head_training_loss(end_points, config, alpha, smpw):
    """:1325-1416 for TRAIN_MODULE == ['RPOINTNET'], mode='training'.  The five SPN terms are computed (without a graph: their inputs are
    detached) and stored as the reference does (:1405-1409) -- the values get_loss gives on the same end_points --, the three R-PointNet
    terms are get_rpointnet_loss's (:1383-1392, :1411-1413) and loss = class + bbox + mask (:1399).  Returns (loss, end_points)."""
    from .rpointnet import _spn_loss_terms
    _require_heads_only(config, "get_head_training_loss")
    with torch.no_grad():
        _spn_loss_terms(end_points, config, alpha, smpw)
    loss, end_points = get_rpointnet_loss(end_points, config)
    end_points['loss'] = loss
    return loss, end_points
