"""The generative parts of shape_proposal_net (models/model_rpointnet.py), same names, argument order and scopes as the reference:
single_encoding_net (:236-255), sample (:269-272) and decoding_net (:274-322).  The decoder's transposed convolutions run on the HIP
kernels of csrc/deconv.hip (tf_util.conv2d_transpose), the rest on the MFMA MLP stack (tf_util.conv2d / fully_connected)."""
import torch

from . import tf_util
from .deconv import deconv_out_size
from .mlp import mlp_stack
from .pointnet_util import _mlp_layers

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
