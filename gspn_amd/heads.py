"""The two heads of R-PointNet and what feeds and scores them, same names, argument order and scopes as models/model_rpointnet.py:
classification_head (:915), segmentation_head (:946), the FPN conv1d layers (:1100-1104) as fpn_features, and the three R-PointNet losses
(:1251, :1264, :1293) with get_rpointnet_loss for :1383-1392 and the sum of :1397.

The heads' input is the crop concat(pc_fea_cropped (C), pc_center_cropped (3), pc_coord_cropped (3)) of roi.points_cropping.  Their first
layer is linear and per point, so it commutes with the gather (crop_linear, on csrc/heads.hip):
    y[b, r, p, :] = T[b, idx[b, r, p], :] + center_n[b, r, p] . W[C:C+3] + coord_n[b, r, p] . W[C+3:C+6] + bias,     T = pc_fea . W[:C]
T is one GEMM over the B*N points instead of the B*R*P crop rows, the gathered rows are cout floats wide and the (B, R, P, C + 6) tensor
is never written.  A head given crop=dict(...) runs its first layer that way, on the same variables as the materialised form.

Two more opt-in forms, both on the variables of the plain ones.  The segmentation head's conv_post_0 reads concat(tile(global), local); it
is linear, so tile_linear runs it as a product over the B*R*P local rows, a product over the B*R global rows and a broadcast add
(gspn_tile_add / gspn_tile_sum of csrc/tile_linear.hip): segmentation_head(split_post=True) never builds the concatenation.  And both
heads read the same crop, so shared_first_layers runs their two conv_prev_0 layers as ONE crop_linear on the weights concatenated along
the output axis -- one T, one gather, one set of inverse lists -- and a head given crop=dict(..., first=rows) starts behind it.

Static shapes, nothing reads a value back to the host: heads + get_rpointnet_loss + backward capture in a graph.CapturedStep.  No CPU
fallback."""
import torch

from . import _lib as L
from . import tf_util
from .mlp import LayerParams, layer_typed, mlp_linear, mlp_stack
from .pointnet_util import _mlp_layers
from .roi import _crop_gather_grad, _Lists, points_cropping

__all__ = ["crop_linear", "tile_linear", "shared_first_layers", "declare_classification_head", "classification_head", "segmentation_head",
           "fpn_features", "get_rpointnet_class_loss", "get_rpointnet_bbox_loss", "get_rpointnet_mask_loss", "get_rpointnet_loss"]

CROP_LINEAR_MAX_COUT = 256          # CL_MAX_COUT of csrc/heads.hip: one float4 of the output row per lane, at most a wave per row


# --------------------------------------------------------------------------- the crop-fused first layer
class _CropLinearSide(torch.autograd.Function):
    """T (B*N, cout), pc_center (B, N, 3), wside (6, cout), bias (cout) -> Y (B, R, P, cout) = T[idx] + side . wside + bias
    (gspn_crop_linear_fwd).  Backward: dwside, dbias and the per-row centre gradient from gspn_crop_linear_bwd_side, dT and dcenter as the
    transposes of the gather through ONE set of inverse lists.  pc and rois get no gradient."""

    @staticmethod
    def forward(ctx, T, pc_center, wside, bias, pc, rois, idx, normalize, lists):
        b, r, p = idx.shape
        n, cout = pc.shape[1], wside.shape[1]
        y = torch.empty((b, r, p, cout), dtype=torch.float32, device=T.device)
        with torch.cuda.device(T.device):
            L.check(L.lib().gspn_crop_linear_fwd(b, n, r, p, cout, L.ptr(T), T.shape[1], L.ptr(idx), L.ptr(pc), L.ptr(pc_center), L.ptr(rois),
                                                 int(normalize), L.ptr(wside), L.ptr(bias), L.ptr(y), L.stream()), "crop_linear")
        ctx.save_for_backward(pc_center, wside, pc, rois, idx)
        ctx.normalize, ctx.lists = int(normalize), lists
        return y

    @staticmethod
    def backward(ctx, dy):
        pc_center, wside, pc, rois, idx = ctx.saved_tensors
        b, r, p = idx.shape
        n, cout = pc.shape[1], wside.shape[1]
        dy = dy.contiguous()
        dev = dy.device
        lib = L.lib()
        dwside = torch.empty_like(wside)
        dbias = torch.empty(cout, dtype=torch.float32, device=dev)
        dcenter_rows = torch.empty((b, r, p, 4), dtype=torch.float32, device=dev)
        part = torch.empty(int(lib.gspn_crop_linear_part_floats(b, r, p, cout)), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            L.check(lib.gspn_crop_linear_bwd_side(b, n, r, p, cout, L.ptr(dy), L.ptr(idx), L.ptr(pc), L.ptr(pc_center), L.ptr(rois), ctx.normalize,
                                                  L.ptr(wside), L.ptr(part), L.ptr(dwside), L.ptr(dbias), L.ptr(dcenter_rows), L.stream()),
                    "crop_linear(grad)")
        dT = _crop_gather_grad(ctx.lists, dy).reshape(b * n, cout) if ctx.needs_input_grad[0] else None
        dcenter = _crop_gather_grad(ctx.lists, dcenter_rows)[:, :, :3].contiguous() if ctx.needs_input_grad[1] else None
        return dT, dcenter, dwside, dbias, None, None, None, None, None


def _aligned16(t):
    return t.data_ptr() % 16 == 0


def crop_linear(pc, pc_fea, pc_center, rois, masks_selection_idx, lp, normalize_crop_region=True):
    """The first layer of a head over the crop of points_cropping, without the crop.  pc (B, N, 3), pc_fea (B, N, C), pc_center (B, N, 3),
    rois (B, R, 6) zero padded, masks_selection_idx (B, R, P) int32, lp: the layer's LayerParams with weights (C + 6, cout) in the order
    [features, centre xyz, coordinate xyz] -> (B, R, P, cout), before batch norm and activation.  Gradients flow to pc_fea, pc_center,
    the weights and the biases; rois is detached, as in points_cropping.
    Raises NotImplementedError, before anything has run, for C > 1024, cout not a multiple of 4 or > 256, weights that are not contiguous,
    or weights / biases / pc_fea that are not 16-byte aligned (the side kernels read them through bare pointers; a strided bias is copied)."""
    idx = L.need(masks_selection_idx, torch.int32, 3, "masks_selection_idx")
    pc = L.need(pc.detach(), torch.float32, 3, "pc")
    pc_fea = L.need(pc_fea, torch.float32, 3, "pc_fea")
    pc_center = L.need(pc_center, torch.float32, 3, "pc_center")
    rois = L.need(rois.detach(), torch.float32, 3, "rois")
    b, n, _ = pc.shape
    c = pc_fea.shape[2]
    r, p = idx.shape[1:]
    if pc.shape[2] != 3 or tuple(pc_center.shape) != (b, n, 3) or tuple(pc_fea.shape[:2]) != (b, n) or idx.shape[0] != b \
            or tuple(rois.shape) != (b, r, 6):
        raise ValueError("crop_linear: expected pc, pc_center (B, N, 3), pc_fea (B, N, C), rois (B, R, 6), masks_selection_idx (B, R, P), got "
                         "%s, %s, %s, %s, %s" % (tuple(pc.shape), tuple(pc_center.shape), tuple(pc_fea.shape), tuple(rois.shape), tuple(idx.shape)))
    cout = layer_typed(lp, c + 6, "crop_linear")            # weights (C + 6, cout), biases (cout): dtype, rank, size
    biases = lp.biases.contiguous()                         # (a strided bias is copied, under autograd; the weights are sliced below and must be in place)
    if c > tf_util._MLP_MAX_CHANNELS or cout % 4 or cout > CROP_LINEAR_MAX_COUT:
        raise NotImplementedError("crop_linear: C <= %d and cout a multiple of 4, <= %d (got C %d, cout %d)"
                                  % (tf_util._MLP_MAX_CHANNELS, CROP_LINEAR_MAX_COUT, c, cout))
    w_fea, w_side = lp.weights[:c], lp.weights[c:]
    if not (lp.weights.is_contiguous() and _aligned16(w_fea) and _aligned16(w_side) and _aligned16(biases) and _aligned16(pc_fea)):
        raise NotImplementedError("crop_linear: the weights (contiguous, and their rows C..C+5), the biases and pc_fea must be 16-byte aligned")
    T = mlp_linear(pc_fea.reshape(b * n, c), c, LayerParams(w_fea, torch.zeros_like(biases), False))
    return _CropLinearSide.apply(T, pc_center, w_side, biases, pc, rois, idx, bool(normalize_crop_region), _Lists(idx, n))


# --------------------------------------------------------------------------- the layer behind concat(tile(global), local), split
class _TileAdd(torch.autograd.Function):
    """a (G*P, c), g (G, c) -> a[k*P + j] + g[k] (gspn_tile_add).  Backward: da = dy itself, dg = the per-group sum of dy in a fixed order
    (gspn_tile_sum)."""

    @staticmethod
    def forward(ctx, a, g, p):
        groups, c = g.shape
        y = torch.empty_like(a)
        with torch.cuda.device(a.device):
            L.check(L.lib().gspn_tile_add(groups, p, c, L.ptr(a), L.ptr(g), L.ptr(y), L.stream()), "tile_add")
        ctx.p = p
        ctx.groups = groups
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        groups, p, c = ctx.groups, ctx.p, dy.shape[1]
        dg = None
        if ctx.needs_input_grad[1]:
            lib = L.lib()
            dg = torch.empty((groups, c), dtype=torch.float32, device=dy.device)
            nfloats = int(lib.gspn_tile_sum_part_floats(groups, p, c))
            part = torch.empty(nfloats, dtype=torch.float32, device=dy.device) if nfloats else None
            with torch.cuda.device(dy.device):
                L.check(lib.gspn_tile_sum(groups, p, c, L.ptr(dy), L.ptr(part), L.ptr(dg), L.stream()), "tile_sum")
        return dy, dg, None


def tile_linear(local_rows, global_rows, lp, p):
    """The linear layer over concat(tile(global, p), local) without the concatenation.  local_rows (G*P, cl), global_rows (G, cg), lp: the
    layer's LayerParams with weights (cg + cl, cout) in the reference's [global, local] order -> (G*P, cout), before batch norm and
    activation:  y[g*P + j] = local[g*P + j] . W[cg:] + (global[g] . W[:cg] + bias).
    Two mlp_linear products -- over the rows with zero bias, over the groups with the bias -- and gspn_tile_add; backward hands dY to the
    local product as it is, its per-group sum (gspn_tile_sum, fixed order) to the global one, and mlp_linear's backward does the rest.
    Raises NotImplementedError, before anything has run, for cout not a multiple of 4, cg, cl or cout > 1024, G*P >= 2^31 or weights that
    are not contiguous and 16-byte aligned."""
    local_rows = L.need(local_rows, torch.float32, 2, "local_rows")
    global_rows = L.need(global_rows, torch.float32, 2, "global_rows")
    p = int(p)
    groups, cg = global_rows.shape
    rows, cl = local_rows.shape
    if p <= 0 or groups <= 0 or rows != groups * p:
        raise ValueError("tile_linear: local_rows (G*P, cl) and global_rows (G, cg) with P = %d, got %s and %s"
                         % (p, tuple(local_rows.shape), tuple(global_rows.shape)))
    cout = layer_typed(lp, cg + cl, "tile_linear")          # weights (cg + cl, cout), biases (cout): dtype, rank, size
    biases = lp.biases.contiguous()                         # (a strided bias is copied, under autograd)
    most = tf_util._MLP_MAX_CHANNELS
    if cout % 4 or cout > most or cg > most or cl > most or rows >= 2 ** 31:
        raise NotImplementedError("tile_linear: cout a multiple of 4, cg, cl, cout <= %d, G*P < 2^31 (got cg %d, cl %d, cout %d, G*P %d)"
                                  % (most, cg, cl, cout, rows))
    if not (lp.weights.is_contiguous() and _aligned16(lp.weights) and _aligned16(biases)):
        raise NotImplementedError("tile_linear: the weights and the biases must be contiguous and 16-byte aligned")
    y_local = mlp_linear(local_rows, cl, LayerParams(lp.weights[cg:], torch.zeros_like(biases), False))
    y_global = mlp_linear(global_rows, cg, LayerParams(lp.weights[:cg], biases, False))
    return _TileAdd.apply(y_local, y_global, p)


# --------------------------------------------------------------------------- the heads
def _pad4(rows):
    """(rows, c) with the row pitch the MLP kernels stage 16 bytes at a time (pad columns zero)"""
    c = rows.shape[1]
    return torch.nn.functional.pad(rows, (0, 4 - c % 4)) if c % 4 else rows


def _stack(rows, cin, layers, is_training, bn_decay, pool_ns=None):
    """mlp_stack over materialised rows of any width: a first layer with more input channels than one launch takes runs as
    tf_util's wide-input layer (column blocks of the same weights), the rest as one stack"""
    if not layers:
        return rows if not pool_ns else rows.view(-1, pool_ns, rows.shape[1]).max(dim=1).values
    if cin > tf_util._MLP_MAX_CHANNELS:
        rows = tf_util._apply_layer(rows, cin, layers[0], torch.relu, bool(is_training), bn_decay)
        return _stack(rows, rows.shape[1], layers[1:], is_training, bn_decay, pool_ns)
    return mlp_stack(_pad4(rows), cin, layers, bool(is_training), bn_decay, pool_ns=pool_ns)


def _bn_relu_rows(y, lp, is_training, bn_decay):
    """the stand-alone batch norm (statistics about a pivot row) and ReLU behind a linear layer, on the layer's own bn variables"""
    if lp.bn:
        y = tf_util._BatchNormRows.apply(y, lp.gamma, lp.beta, lp.moving_mean, lp.moving_variance, bool(is_training),
                                         0.9 if bn_decay is None else float(bn_decay))
    return torch.relu(y)


def _first_layers(pc, pc_fea, mlp_list, is_training, bn_decay, bn, crop, pool_ns_of_stack):
    """the conv_prev_%d layers of either head: -> (rows (B*R*P, mlp_list[-1]) or pooled (B*R, ...), B, R, P).  pool_ns_of_stack: whether the
    stack ends in the max over the P points (classification head) or returns the rows (segmentation head)."""
    if crop is not None:
        b, r, p = L.need(crop["idx"], torch.int32, 3, "crop['idx']").shape
        cin = L.need(crop["pc_fea"], torch.float32, 3, "crop['pc_fea']").shape[2] + 6
    else:
        b, r, p, _ = L.need(pc, torch.float32, 4, "pc").shape
        cin = L.need(pc_fea, torch.float32, 4, "pc_fea").shape[3] + 3
    layers = _mlp_layers(mlp_list, cin, 'conv_prev_', bn)
    rows = None
    if crop is not None and crop.get("first") is not None:          # conv_prev_0 has run outside (shared_first_layers), on these variables
        rows = L.need(crop["first"], torch.float32, 2, "crop['first']")
        if tuple(rows.shape) != (b * r * p, mlp_list[0]):
            raise ValueError("crop['first'] must be (B*R*P, %d) = (%d, %d), got %s" % (mlp_list[0], b * r * p, mlp_list[0], tuple(rows.shape)))
        layers, cin = layers[1:], rows.shape[1]
    elif crop is not None:
        normalize = crop.get("normalize", True)
        try:
            y = crop_linear(crop["pc"], crop["pc_fea"], crop["pc_center"], crop["rois"], crop["idx"], layers[0], normalize)
        except NotImplementedError:                      # a shape the kernels decline: the materialised crop, same variables
            fea, cen, coord, _ = points_cropping(crop["pc"], crop["pc_fea"], crop["pc_center"], crop["rois"], crop["idx"], r, p, normalize)
            pc, pc_fea = coord, torch.cat((fea, cen), -1)
        else:
            rows = _bn_relu_rows(y.reshape(b * r * p, y.shape[3]), layers[0], is_training, bn_decay)
            layers, cin = layers[1:], y.shape[3]
    if rows is None:
        rows = torch.cat((pc_fea, pc), -1).reshape(b * r * p, cin)
    return _stack(rows, cin, layers, is_training, bn_decay, p if pool_ns_of_stack else None), b, r, p


def _conv1d_bn_relu(inputs, num_outputs, scope, is_training, bn_decay, bn):
    """tf_util.conv1d(..., bn=bn) with the same variables in the same order, as a linear layer, then the stand-alone batch norm, then ReLU:
    the form of shape_proposal._fc_bn_relu, for the same reason -- these layers normalise max-pooled, non-negative features, whose mean is
    large against their spread."""
    cin = inputs.shape[-1]
    lp = tf_util._layer_params(scope, cin, num_outputs, [1, cin, num_outputs], True, 1e-3, None, False)
    with tf_util.variable_scope(scope):
        y = tf_util._apply_layer(inputs.reshape(-1, cin), cin, lp, None, bool(is_training), bn_decay).view(*inputs.shape[:-1], num_outputs)
        if bn:
            y = tf_util.batch_norm_for_conv1d(y, is_training, bn_decay, 'bn')
    return torch.relu(y)


def declare_classification_head(cin, num_category, mlp_list, mlp_list2, scope, bn=True):
    """Creates (or finds) every variable of classification_head in the reference's order without running it and returns conv_prev_0's
    LayerParams.  cin = C + 6, the width of the head's input rows.  What shared_first_layers needs of the segmentation head --
    segmentation_head/conv_prev_0 -- can then be created before the classification head has run and still comes behind all of its
    variables."""
    with tf_util.variable_scope(scope):
        first = _mlp_layers(mlp_list, cin, 'conv_prev_', bn)[0]
        c = mlp_list[-1]
        for i, num_out_channel in enumerate(mlp_list2):
            tf_util._layer_params('conv_post_%d' % i, c, num_out_channel, [1, c, num_out_channel], True, 1e-3, None, False)
            if bn:
                with tf_util.variable_scope('conv_post_%d' % i), tf_util.variable_scope('bn'):
                    tf_util._bn_variables(num_out_channel)
            c = num_out_channel
        tf_util._layer_params('conv_classify', c, num_category, [1, c, num_category], True, 1e-3, None, False)
        tf_util._layer_params('conv_bbox_regress', c, num_category * 6, [1, c, num_category * 6], True, 1e-3, None, False)
    return first


def shared_first_layers(crop, cls_layer, seg_layer, is_training, bn_decay):
    """conv_prev_0 of both heads over one crop as ONE crop_linear: the two layers' weights (C + 6, 128) and (C + 6, 64) and their biases are
    concatenated along the output axis for the call (the variables stay two and get their gradients through the concatenation), the
    (B, R, P, 192) result is split and each part goes through its own layer's batch norm and ReLU.  One T product, one gather, one side
    backward and one set of inverse lists instead of two of each.  crop: the dict the heads take; cls_layer, seg_layer: the LayerParams of
    classification_head/conv_prev_0 and segmentation_head/conv_prev_0 -> (cls_rows (B*R*P, 128), seg_rows (B*R*P, 64)), what
    crop=dict(..., first=rows) takes.  Raises NotImplementedError, before anything has run, where crop_linear does."""
    c_cls = cls_layer.weights.shape[1]
    both = LayerParams(torch.cat((cls_layer.weights, seg_layer.weights), 1), torch.cat((cls_layer.biases, seg_layer.biases)), False)
    y = crop_linear(crop["pc"], crop["pc_fea"], crop["pc_center"], crop["rois"], crop["idx"], both, crop.get("normalize", True))
    y = y.reshape(-1, y.shape[3])
    return (_bn_relu_rows(y[:, :c_cls].contiguous(), cls_layer, is_training, bn_decay),
            _bn_relu_rows(y[:, c_cls:].contiguous(), seg_layer, is_training, bn_decay))


def classification_head(pc, pc_fea, num_category, mlp_list, mlp_list2, is_training, bn_decay, scope, bn=True, crop=None):
    """:915-944.  pc (B, R, P, 3) = pc_coord_cropped, pc_fea (B, R, P, NFEA) = concat(pc_fea_cropped, pc_center_cropped) ->
    logits (B, R, num_category), probs (B, R, num_category), bbox_deltas (B, R, num_category, 6).
    Variables in the reference's order: conv_prev_%d, conv_post_%d, conv_classify, conv_bbox_regress.
    crop (extension) = dict(pc=(B, N, 3), pc_fea=(B, N, C), pc_center=(B, N, 3), rois=(B, R, 6), idx=(B, R, P) int32, normalize=bool): the
    inputs of points_cropping instead of its outputs; the first layer then runs as crop_linear -> stand-alone batch norm -> ReLU on the
    same variables and pc / pc_fea may be None.  A shape crop_linear declines is cropped and takes the materialised path.
    With crop['first'] = rows (B*R*P, mlp_list[0]) -- shared_first_layers' -- conv_prev_0 has run outside: its variables are still created
    here, in their place, and the head starts at conv_prev_1."""
    with tf_util.variable_scope(scope):
        new_points, b, r, _ = _first_layers(pc, pc_fea, mlp_list, is_training, bn_decay, bn, crop, True)          # + reduce_max (:933)
        new_points = new_points.view(b, r, -1)
        for i, num_out_channel in enumerate(mlp_list2):
            new_points = _conv1d_bn_relu(new_points, num_out_channel, 'conv_post_%d' % i, is_training, bn_decay, bn)
        logits = tf_util.conv1d(new_points, num_category, 1, padding='VALID', stride=1, scope='conv_classify', activation_fn=None)
        probs = torch.softmax(logits, 2)
        bbox_deltas = tf_util.conv1d(new_points, num_category * 6, 1, padding='VALID', stride=1, scope='conv_bbox_regress', activation_fn=None)
        return logits, probs, bbox_deltas.reshape(-1, r, num_category, 6)


def segmentation_head(pc, pc_fea, num_category, mlp_list, mlp_list2, mlp_list3, is_training, bn_decay, scope, bn=True, crop=None,
                      split_post=False):
    """:946-978.  pc (B, R, P, 3), pc_fea (B, R, P, NFEA) -> masks (B, R, P, num_category).
    Variables in the reference's order: conv_prev_%d, conv_%d, conv_post_%d, conv_seg.  crop: as in classification_head.
    The layer behind concat(tile(global), local), conv_post_0, reads that concatenation materialised; with split_post=True (extension) it
    runs as tile_linear -> stand-alone batch norm -> ReLU on the same variables and the concatenation is never built.  A shape tile_linear
    declines takes the materialised path."""
    with tf_util.variable_scope(scope):
        local_feat, b, r, p = _first_layers(pc, pc_fea, mlp_list, is_training, bn_decay, bn, crop, False)         # (B*R*P, mlp_list[-1])
        c_local = local_feat.shape[1]
        layers = _mlp_layers(mlp_list2, c_local, 'conv_', bn)
        global_feat = _stack(local_feat, c_local, layers, is_training, bn_decay, p)                               # (B*R, mlp_list2[-1])
        c_global = global_feat.shape[1]
        layers = _mlp_layers(mlp_list3, c_global + c_local, 'conv_post_', bn)
        new_points = None
        if split_post and layers:
            try:
                y = tile_linear(local_feat, global_feat, layers[0], p)
            except NotImplementedError:                  # a shape the kernels decline: the materialised concatenation, same variables
                pass
            else:
                new_points = _stack(_bn_relu_rows(y, layers[0], is_training, bn_decay), y.shape[1], layers[1:], is_training, bn_decay)
        if new_points is None:
            new_points = torch.cat((global_feat.view(b * r, 1, c_global).expand(-1, p, -1), local_feat.view(b * r, p, c_local)), -1)
            new_points = _stack(new_points.reshape(b * r * p, c_global + c_local), c_global + c_local, layers, is_training, bn_decay)
        new_points = new_points.view(b, r, p, -1)
        return tf_util.conv2d(new_points, num_category, [1, 1], padding='VALID', stride=[1, 1], scope='conv_seg', activation_fn=None)


def fpn_features(end_points, is_training, bn_decay):
    """:1100-1104.  The four conv1d(64) + BN + ReLU layers fpn1..fpn4 over end_points['sem_fea_full_l1'..'l4'], concatenated behind
    end_points['entity_fea']: the (B, N, C) feature tensor the heads crop."""
    for i in (1, 2, 3, 4):                                # before any variable is created
        L.need(end_points['sem_fea_full_l%d' % i], torch.float32, 3, 'sem_fea_full_l%d' % i)
    levels = [tf_util.conv1d(end_points['sem_fea_full_l%d' % i], 64, 1, padding='VALID', bn=True, is_training=is_training, scope='fpn%d' % i,
                             bn_decay=bn_decay) for i in (1, 2, 3, 4)]
    return torch.cat([end_points['entity_fea']] + levels, -1)


# --------------------------------------------------------------------------- the losses
def _foreground(gt_class_ids, roi_valid_mask):
    """the rows the bbox and mask losses select (:1279, :1310) as a 0/1 mask, and the class index of every row"""
    cls = gt_class_ids.reshape(-1).long()
    return ((roi_valid_mask.reshape(-1) > 0) & (cls > 0)), cls


def get_rpointnet_class_loss(rpointnet_class_logits, gt_class_ids, roi_valid_mask):
    """:1251-1262.  logits (B, R, NUM_CATEGORY), gt_class_ids (B, R) zero padded, roi_valid_mask (B, R): cross-entropy summed over the
    valid ROIs over their number + 1e-8; 0 when there is none."""
    logits = rpointnet_class_logits
    label = gt_class_ids.long().clamp(0, logits.shape[-1] - 1)
    ce = torch.logsumexp(logits, dim=-1) - torch.gather(logits, 2, label.unsqueeze(-1)).squeeze(-1)
    valid = roi_valid_mask.to(logits.dtype)
    return (ce * valid).sum() / (valid.sum() + 1e-8)


def get_rpointnet_bbox_loss(gt_bbox, gt_class_ids, pred_bbox, roi_valid_mask, num_category):
    """:1264-1291.  gt_bbox (B, R, 6), pred_bbox (B, R, NUM_CATEGORY, 6): over the valid ROIs of a foreground class, the mean of the
    smooth-L1 distance (summed over the six) between the target and the deltas of that class -- a masked mean with static shapes instead of
    tf.where / gather_nd; 0 when no ROI qualifies."""
    from .rpointnet import smooth_l1_loss
    sel, cls = _foreground(gt_class_ids, roi_valid_mask)
    pred = pred_bbox.reshape(-1, num_category, 6)
    pred = torch.gather(pred, 1, cls.clamp(0, num_category - 1).view(-1, 1, 1).expand(-1, 1, 6)).squeeze(1)
    per_roi = smooth_l1_loss(gt_bbox.reshape(-1, 6).to(pred.dtype), pred).sum(1)
    sel = sel.to(pred.dtype)
    return (per_roi * sel).sum() / sel.sum().clamp(min=1.0)


def get_rpointnet_mask_loss(gt_masks, gt_class_ids, pred_masks, roi_valid_mask, num_category, num_point_per_roi):
    """:1293-1323.  gt_masks (B, R, P) bool or 0/1, pred_masks (B, R, P, NUM_CATEGORY) logits: over the valid ROIs of a foreground class, the
    mean sigmoid cross-entropy between the target mask and the mask of that class; 0 when no ROI qualifies."""
    sel, cls = _foreground(gt_class_ids, roi_valid_mask)
    pred = pred_masks.reshape(-1, num_point_per_roi, num_category)
    x = torch.gather(pred, 2, cls.clamp(0, num_category - 1).view(-1, 1, 1).expand(-1, num_point_per_roi, 1)).squeeze(2)
    z = gt_masks.reshape(-1, num_point_per_roi).to(x.dtype)
    bce = torch.clamp(x, min=0) - x * z + torch.log1p(torch.exp(-torch.abs(x)))          # tf.nn.sigmoid_cross_entropy_with_logits
    sel = sel.to(x.dtype)
    return (bce.sum(1) * sel).sum() / (sel.sum().clamp(min=1.0) * num_point_per_roi)


def get_rpointnet_loss(end_points, config):
    """:1383-1392 and the R-PointNet sum of :1397, over an end_points with the keys of :1199-1209 (rois, target_class_ids, target_bbox,
    target_mask, rpointnet_class_logits, rpointnet_bbox, rpointnet_mask).  Returns (loss, end_points); end_points gains
    rpointnet_class_loss, rpointnet_bbox_loss and rpointnet_mask_loss (:1411-1413)."""
    roi_valid_mask = (end_points['rois'].abs().sum(-1) != 0).float()
    cls = end_points['target_class_ids']
    class_loss = get_rpointnet_class_loss(end_points['rpointnet_class_logits'], cls, roi_valid_mask)
    bbox_loss = get_rpointnet_bbox_loss(end_points['target_bbox'], cls, end_points['rpointnet_bbox'], roi_valid_mask, config.NUM_CATEGORY)
    mask_loss = get_rpointnet_mask_loss(end_points['target_mask'], cls, end_points['rpointnet_mask'], roi_valid_mask, config.NUM_CATEGORY,
                                        config.NUM_POINT_INS_MASK)
    end_points['rpointnet_class_loss'] = class_loss
    end_points['rpointnet_bbox_loss'] = bbox_loss
    end_points['rpointnet_mask_loss'] = mask_loss
    return class_loss + bbox_loss + mask_loss, end_points
