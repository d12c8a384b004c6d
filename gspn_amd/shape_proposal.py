"""shape_proposal_net (models/model_rpointnet.py:324-434) and its generative parts, same names, argument order and scopes as the reference:
single_encoding_net (:236-255), sample (:269-272) and decoding_net (:274-322).  The decoder's transposed convolutions run on the HIP
kernels of csrc/deconv.hip (tf_util.conv2d_transpose), the rest on the MFMA MLP stack (tf_util.conv2d / fully_connected); the trunks
are spn_trunks.py, the context encoder and the heads proposal_head.py, the bounding boxes csrc/spn_boxes.hip."""
import torch

from . import _lib as L
from . import tf_util
from .deconv import deconv_out_size
from .mlp import mlp_stack
from .pointnet_util import _mlp_layers, pointnet_fp_module
from .proposal_head import fea_trans_net, multi_encoding_net
from .spn_boxes import points_bbox
from .spn_trunks import sem_net, shift_pred_net, spn_geometry

SPN_SEM_POINTS = 1024           # :354

# decoding_net's three up-convolution branches (:284-301): num_point range -> ([(scope, Cout, k, s, bn)], num_point_conv).
# Every layer but the last is batch-normalised and ReLU'd; the last (Cout 3, 1x1) is linear.
DECODER_BRANCHES = (
    ((1536, 3072), ([("upconv1", 512, 2, 1, True), ("upconv2", 256, 3, 1, True), ("upconv3", 256, 4, 2, True),
                     ("upconv4", 128, 5, 3, True), ("upconv5", 3, 1, 1, False)], 1024)),
    ((896, 1536), ([("upconv1", 512, 2, 1, True), ("upconv2", 256, 2, 1, True), ("upconv3", 256, 3, 2, True),
                    ("upconv4", 128, 4, 3, True), ("upconv5", 3, 1, 1, False)], 484)),
    ((384, 896), ([("upconv1", 512, 3, 1, True), ("upconv2", 256, 3, 2, True), ("upconv3", 128, 4, 2, True),
                   ("upconv4", 3, 1, 1, False)], 256)),
)


def decoder_layers(num_point):
    """the up-convolution branch decoding_net takes for num_point: ([(scope, Cout, k, s, bn)], num_point_conv).
    Outside (384, 3072] the reference raises a string (:300-301), a TypeError in Python 3; this raises ValueError."""
    for (lo, hi), branch in DECODER_BRANCHES:
        if lo < num_point <= hi:
            return branch
    raise ValueError("decoding_net: num_point %r outside the three branches (384, 896], (896, 1536], (1536, 3072]" % (num_point,))


def decoder_map_sizes(num_point):
    """spatial side of the feature map after each up-convolution, starting from the 1x1 code"""
    sizes, h = [], 1
    for _, _, k, s, _ in decoder_layers(num_point)[0]:
        h = deconv_out_size(h, s, k)
        sizes.append(h)
    return sizes


def single_encoding_net(pc, mlp_list, mlp_list2, scope, is_training, bn_decay):
    """:236-255.  pc (B, N, 3) -> (B, mlp_list2[-1]): conv2d+BN+ReLU layers over the points, max over N, fully_connected+BN+ReLU."""
    with tf_util.variable_scope(scope):
        b, n, c = pc.shape
        rows = pc.reshape(-1, c)
        if c % 4:
            rows = torch.nn.functional.pad(rows, (0, 4 - c % 4))
        layers = _mlp_layers(mlp_list, c, 'conv', True)                   # scopes conv%d (:247)
        net = mlp_stack(rows, c, layers, bool(is_training), bn_decay, pool_ns=n)     # + reduce_max over the N points (:248-249)
        for i, num_out_channel in enumerate(mlp_list2):
            net = _fc_bn_relu(net, num_out_channel, 'fc%d' % i, is_training, bn_decay)
        return net


def _fc_bn_relu(inputs, num_outputs, scope, is_training, bn_decay):
    """tf_util.fully_connected(..., bn=True) (tf_util.py:330-366) with the same variables in the same order, as a linear layer, then the
    stand-alone batch norm (batch_norm_for_fc), then ReLU.  The stand-alone batch norm takes its statistics about a pivot row; the fused
    MLP launch sums y and y^2 in one pass, which loses digits when |mean| >> std -- the usual case for the max-pooled, non-negative
    instance features fc0 normalises and for de_fc3's ReLU'd input."""
    lp = tf_util._layer_params(scope, inputs.shape[-1], num_outputs, [inputs.shape[-1], num_outputs], True, 1e-3, None, False)
    with tf_util.variable_scope(scope):
        y = tf_util._apply_layer(inputs, inputs.shape[-1], lp, None, bool(is_training), bn_decay)
        y = tf_util.batch_norm_for_fc(y, is_training, bn_decay, 'bn')
    return torch.relu(y)


def sample(mean, log_var, noise=None):
    """:269-272: z = mean + exp(log_var/2) * eps, eps ~ N(0, 1) drawn on the device unless `noise` fixes it"""
    if noise is None:
        noise = torch.randn(mean.shape, dtype=mean.dtype, device=mean.device)
    return mean + torch.exp(log_var / 2.0) * noise


def decoding_net(feat, num_point, scope, is_training, bn_decay):
    """:274-322.  feat (B, nsmp, nfea) -> pc (B, nsmp, num_point, 3): num_point_conv points from the up-convolution branch, the rest
    from three FC layers, concatenated in that order."""
    layers, num_point_conv = decoder_layers(num_point)
    with tf_util.variable_scope(scope):
        b, nsmp, nfea = feat.shape
        feat = feat.reshape(-1, nfea)
        net = feat.reshape(-1, 1, 1, nfea)
        for name, cout, k, s, bn in layers:
            net = tf_util.conv2d_transpose(net, cout, kernel_size=[k, k], stride=[s, s], padding='VALID', scope=name, bn=bn,
                                           bn_decay=bn_decay, is_training=is_training, activation_fn=torch.relu if bn else None)
        pc_upconv = net.reshape(-1, num_point_conv, 3)
        num_point_fc = num_point - num_point_conv
        net = _fc_bn_relu(feat, 512, 'de_fc2', is_training, bn_decay)
        net = _fc_bn_relu(net, 512, 'de_fc3', is_training, bn_decay)
        net = tf_util.fully_connected(net, num_point_fc * 3, activation_fn=None, scope='de_fc4')
        pc_fc = net.reshape(-1, num_point_fc, 3)
        pc = torch.cat([pc_upconv, pc_fc], dim=1)
        return pc.reshape(b, nsmp, num_point, 3)


def check_spn_inputs(pc, pc_ins, group_label, group_indicator):
    """Host-side validation of shape_proposal_net's preconditions, for use OUTSIDE the step (it reads the labels back): shapes, and
    group_label in [0, ngroup) -- the reference's reshape at :369-373 assumes it.  Raises ValueError."""
    if pc.dim() != 3 or pc.shape[2] != 3:
        raise ValueError("pc must be (B, N, 3), got %s" % (tuple(pc.shape),))
    if pc_ins.dim() != 4 or pc_ins.shape[3] != 3 or pc_ins.shape[0] != pc.shape[0]:
        raise ValueError("pc_ins must be (B, ngroup, nsmp_ins, 3), got %s" % (tuple(pc_ins.shape),))
    b, ngroup = pc_ins.shape[:2]
    if tuple(group_label.shape) != (b, pc.shape[1]) or group_label.dtype.is_floating_point:
        raise ValueError("group_label must be integer (B, N), got %s %s" % (group_label.dtype, tuple(group_label.shape)))
    if tuple(group_indicator.shape) != (b, ngroup):
        raise ValueError("group_indicator must be (B, ngroup), got %s" % (tuple(group_indicator.shape),))
    lo, hi = int(group_label.min()), int(group_label.max())
    if lo < 0 or hi >= ngroup:
        raise ValueError("group_label must lie in [0, %d), found values in [%d, %d]" % (ngroup, lo, hi))


def valid_instances(group_indicator):
    """(k, 2) int64 batch / group indices of the instances with group_indicator > 0 (:360), row-major like tf.where.  Reads the
    indicator back to the host: call it ahead of the step and pass the result as valid_idx=."""
    return torch.nonzero(group_indicator > 0)


class _GatherRows(torch.autograd.Function):
    """src (B, G, C) rows at label (B, S) -> (B, S, C).  The gradient adds several seeds into one instance row; it is taken as the product
    with the (S, G) one-hot matrix of the labels -- a fixed summation order, no float atomics."""
    @staticmethod
    def forward(ctx, src, label):
        ctx.save_for_backward(label)
        ctx.g = src.shape[1]
        return torch.gather(src, 1, label.unsqueeze(-1).expand(-1, -1, src.shape[2]))

    @staticmethod
    def backward(ctx, dy):
        label, = ctx.saved_tensors
        onehot = (label.unsqueeze(1) == torch.arange(ctx.g, device=label.device).view(1, -1, 1)).to(dy.dtype)      # (B, G, S)
        return torch.bmm(onehot, dy.contiguous()), None


def shape_proposal_net(pc, color, pc_ins, group_label, group_indicator, num_category, scope, is_training, bn_decay=None, nsmp=128,
                       return_fullfea=False, mode='training', geometry=None, noise=None, valid_idx=None):
    """:324-434.  pc (B, N, 3), color (B, N, 3), pc_ins (B, ngroup, nsmp_ins, 3) in world coordinates, group_label (B, N) integer,
    group_indicator (B, ngroup) -> end_points with the reference's keys (:419-432, plus what the trunks add, plus entity_fea and
    center_pos with return_fullfea).
    Extensions: geometry -- spn_geometry(pc, nsmp, 1024, return_fullfea, points=color); None builds it here, once for both trunks.
    noise -- fixes sample()'s draw, (B, nsmp, 256).  valid_idx -- valid_instances(group_indicator) computed ahead of the step; None
    reads group_indicator back here, before any launch (the instance encoder's batch-norm statistics depend on how many instances it
    sees, so the valid ones are really selected).
    Precondition: group_label in [0, ngroup) (check_spn_inputs raises for it on the host); the index is clamped before every gather, so a
    bad label reads a wrong row, never out of bounds.  bbox_ins_pred carries no gradient (spn_boxes.points_bbox)."""
    pc = L.need(pc, torch.float32, 3, "pc")
    if color is None:
        raise NotImplementedError("shape_proposal_net: sem_net gathers the colours of its samples (:152-153); USE_COLOR=False is not supported")
    color = L.need(color, torch.float32, 3, "color")
    pc_ins = L.need(pc_ins, torch.float32, 4, "pc_ins")
    for name, t in (("group_label", group_label), ("group_indicator", group_indicator)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise L.GspnHipError("%s is not on a ROCm device (no CPU fallback)" % name)
    if valid_idx is None:
        valid_idx = valid_instances(group_indicator)
    with tf_util.variable_scope(scope):
        batch_size, ngroup, nsmp_ins = pc_ins.shape[0], pc_ins.shape[1], pc_ins.shape[2]
        if geometry is None:
            geometry = spn_geometry(pc, nsmp, SPN_SEM_POINTS, return_fullfea, points=color)
        end_points = {}

        # shift prediction (:347-351)
        end_points = shift_pred_net(pc, color, nsmp, end_points, 'shift_predictor', is_training, bn_decay=bn_decay,
                                    return_fullfea=return_fullfea, geometry=geometry)
        pc_seed = end_points['pc_seed']
        shift_pred_seed_4d = end_points['shift_pred_seed_4d']
        ind_seed = end_points['ind_seed']
        shift_pred_seed = shift_pred_seed_4d[:, :, :3] * shift_pred_seed_4d[:, :, 3:]

        # semantic prediction (:354-355)
        end_points = sem_net(pc, color, SPN_SEM_POINTS, num_category, ind_seed, end_points, 'sem_predictor', is_training, bn_decay=bn_decay,
                             return_fullfea=return_fullfea, mode=mode, geometry=geometry)
        sem_fea_seed = end_points['sem_fea_seed']

        # encode the valid instances, scatter back with zeros elsewhere (:358-364)
        pc_ins_center = points_bbox(pc_ins)[:, :, :3].unsqueeze(2)                      # (B, ngroup, 1, 3)
        pc_ins_centered = pc_ins.detach() - pc_ins_center
        vb, vg = valid_idx[:, 0].long(), valid_idx[:, 1].long()
        pc_ins_centered_list = pc_ins_centered[vb, vg]
        pcfea_ins_centered_list = single_encoding_net(pc_ins_centered_list, [64, 256, 512], [256], 'instance_encoder', is_training, bn_decay)
        nfea_ins = pcfea_ins_centered_list.shape[1]
        pcfea_ins_centered = torch.zeros((batch_size, ngroup, nfea_ins), dtype=torch.float32, device=pc.device).index_put(
            (vb, vg), pcfea_ins_centered_list)

        # per-seed instance rows (:367-374)
        group_label_seed = torch.gather(group_label.long(), 1, ind_seed.long()).clamp(0, ngroup - 1)     # (B, nsmp)
        pcfea_ins_seed = _GatherRows.apply(pcfea_ins_centered, group_label_seed)
        rows = torch.arange(batch_size, device=pc.device).unsqueeze(1)
        pc_ins_centered_seed = pc_ins_centered[rows, group_label_seed]                  # (B, nsmp, nsmp_ins, 3)
        pc_ins_center_seed = pc_ins_center[rows, group_label_seed]                      # (B, nsmp, 1, 3)

        # context (:377), foreground / background score (:380-381), mu and sigma (:384-393)
        _, pcfea_seed, _, _ = multi_encoding_net(pc, color, nsmp, [0.5, 1.0, 1.5], [256, 256, 512], [[64, 128, 256], [64, 128, 256], [64, 128, 256]],
                                                 [], is_training, bn_decay, scope='context_encoder', use_xyz=True, output_shift=False,
                                                 shift_pred=shift_pred_seed.detach(), fps_idx=ind_seed)
        fb_logits = fea_trans_net(pcfea_seed, [256, 64, 2], 'fb_logits', is_training, bn_decay)
        fb_prob = torch.softmax(fb_logits, -1)
        mu_sigma_c = fea_trans_net(torch.cat((sem_fea_seed, pcfea_seed), dim=-1), [256, 512, 512], 'mu_sigma_c', is_training, bn_decay)
        mu_sigma_x = fea_trans_net(torch.cat((sem_fea_seed, pcfea_seed, pcfea_ins_seed), dim=-1), [256, 512, 512], 'mu_sigma_x', is_training,
                                   bn_decay)
        mean = mu_sigma_x[:, :, :256]
        log_var = torch.clamp(mu_sigma_x[:, :, 256:], -10.0, 1.0)
        cmean = mu_sigma_c[:, :, :256]
        clog_var = torch.clamp(mu_sigma_c[:, :, 256:], -10.0, 1.0)
        z = sample(mean, log_var, noise) if is_training else cmean                      # :394-396

        # decode (:399-403)
        gcfeat = tf_util.conv1d(pcfea_seed, 256, 1, padding='VALID', bn=True, is_training=is_training, scope='dec_fc', bn_decay=bn_decay)
        feat = torch.cat((z, gcfeat), dim=-1)
        pc_ins_pred = decoding_net(feat, nsmp_ins, 'decoder', is_training=is_training, bn_decay=bn_decay)
        pc_ins_pred = pc_ins_pred + shift_pred_seed.detach().unsqueeze(2)
        bbox_ins_pred = points_bbox(pc_ins_pred, pc_seed)                               # :406-408

        if return_fullfea:                                                              # :411-416
            end_points['entity_fea'] = pointnet_fp_module(pc, pc_seed, None, pcfea_seed, [], is_training=False, bn_decay=None,
                                                          scope='entity_fea_prop', bn=False)
            full = end_points['shift_pred_full_4d']
            end_points['center_pos'] = pc + full[:, :, :3] * full[:, :, 3:]

        end_points['shift_pred_seed'] = shift_pred_seed
        end_points['shift_pred_seed_4d'] = shift_pred_seed_4d
        end_points['pc_seed'] = pc_seed
        end_points['ind_seed'] = ind_seed
        end_points['pc_ins_centered_seed'] = pc_ins_centered_seed
        end_points['pc_ins_center_seed'] = pc_ins_center_seed
        end_points['mean'] = mean
        end_points['log_var'] = log_var
        end_points['cmean'] = cmean
        end_points['clog_var'] = clog_var
        end_points['fb_logits'] = fb_logits
        end_points['fb_prob'] = fb_prob
        end_points['pc_ins_pred'] = pc_ins_pred
        end_points['bbox_ins_pred'] = bbox_ins_pred
        return end_points
