"""The SA/FP trunks that GSPN's shape_proposal_net runs (models/model_rpointnet.py:324-352, called by rpointnet() in both training
stages, :1067-1071): shift_pred_net (:79-127) and sem_net (:129-206).  Same names, argument order, variable-scope strings and end_points
keys as the reference, so checkpoints' variable names line up.

Both trunks run SA levels 1-4 with identical (npoint, radius, nsample) on the same xyz, and their seed / semantic samples are prefixes of
level 1's FPS (FPS picks index 0 first and no later pick depends on npoint).  spn_geometry(xyz, ...) computes everything the two trunks
derive from coordinates ONCE -- one full-cloud FPS instead of four, one ball query / 3-NN per level instead of two -- and both trunks take it
through geometry=.  In the full-feature mode (return_fullfea=True) every dense point needs its 3 nearest neighbours in l4, l3, l2 and l1:
nested subsets of l1, answered by one scan of l1 (three_nn_nested) or by one three_nn per level (NESTED_NN / NESTED_MIN_POINTS below).

    geo = spn_geometry(xyz, nsmp, 1024, return_fullfea, points=color)
    end_points = shift_pred_net(xyz, color, nsmp, {}, 'shift_predictor', is_training, bn_decay, return_fullfea, geometry=geo)
    end_points = sem_net(xyz, color, 1024, ncat, end_points['ind_seed'], end_points, 'sem_predictor', is_training, bn_decay,
                         return_fullfea, mode, geometry=geo)
"""
import os

import torch

from . import tf_util
from .geometry import SAGeometry, fp_geometry, fp_geometry_from_nn, pad_features, sa_geometry
from .pointnet_util import fp_concat, pointnet_fp_module, pointnet_sa_module
from .tf_interpolate import nested_local_maps, three_nn, three_nn_nested
from .tf_sampling import farthest_point_sample, gather_point

# (npoint, radius, nsample, mlp) of the four SA levels, model_rpointnet.py:103-106 and :170-173 (identical in both trunks)
SPN_SA_SPEC = ((2048, 0.2, 32, [32, 32, 64]), (512, 0.4, 32, [64, 64, 128]), (128, 0.8, 32, [128, 128, 256]), (32, 1.6, 32, [256, 256, 512]))
# mlp of fa_layer1..4, :109-112 and :183-186
SPN_FP_MLP = ([256, 256], [256, 256], [256, 128], [128, 128, 128])

# full-feature dense 3-NN: one scan of l1 for all four levels (three_nn_nested) instead of one three_nn per level -- identical results.
# Measured on MI355X (tools/spn_step.py, S clouds): 8 x 32768 -> 193 us of kernel time instead of 346 us for the four launches; 2 x 18000 ->
# 0.178 ms instead of 0.145 ms (141 workgroups of 256 queries leave most of the chip idle, the per-level wave kernels do not).  So the
# nested scan is taken from NESTED_MIN_POINTS dense points per batch on; GSPN_SPN_NESTED_NN=1 / 0 forces either path.
NESTED_NN = {"1": True, "0": False}.get(os.environ.get("GSPN_SPN_NESTED_NN", ""), None)
NESTED_MIN_POINTS = 1 << 17


def _prefix_or_fps(fps1, k, xyz):
    """the first k picks of level 1's FPS; a separate FPS when k exceeds level 1's npoint (the prefix argument needs k <= 2048)"""
    if k <= fps1.shape[1]:
        return fps1[:, :k].contiguous()
    return farthest_point_sample(k, xyz)


def _rows(t, ind):
    """t (b, n, 3) rows at ind (b, k) -> (b, k, 3)"""
    return torch.gather(t, 1, ind.long().unsqueeze(-1).expand(-1, -1, t.shape[2]))


def spn_geometry(xyz, npoint_seed, npoint_sem, return_fullfea=False, points=None, nested=None):
    """Everything shift_pred_net and sem_net derive from coordinates alone, computed once for both (feed it to either through geometry=):
      ind_seed, ind_sem   prefixes of level 1's FPS (separate FPS beyond 2048 points)
      sa_shift, sa_sem    the four SAGeometry of each trunk -- shared objects except level 1, where sa_sem carries the 16-byte-row pad of
                          the colours (feat4, points given) and sa_shift none: the shift trunk groups no features
      fp                  FPGeometry of fa_layer1..3 (shared)
      fa4_shift, fa4_sem  FPGeometry of each trunk's fa_layer4: rows [seed(; cloud)] and [seed; sem(; cloud)] onto l1
      fpn                 (return_fullfea) FPGeometry of fa_layer1_fpn..fa_layer4_fpn: the cloud onto l4, l3, l2, l1
    Bit-identical to what each trunk computes inline.  nested: use three_nn_nested for the dense queries (None: NESTED_NN, or by size)."""
    xyz = xyz.detach()
    if nested is None:
        nested = NESTED_NN if NESTED_NN is not None else xyz.shape[0] * xyz.shape[1] >= NESTED_MIN_POINTS
    sa, fps, cur = [], [], xyz
    for level, (npoint, radius, nsample, _) in enumerate(SPN_SA_SPEC):
        f = farthest_point_sample(npoint, cur, return_order=True)
        g = sa_geometry(cur, npoint, radius, nsample, inverse=level > 0, fps=f)
        sa.append(g)
        fps.append(f[0])
        cur = g.new_xyz
    g1 = sa[0]
    feat4 = pad_features(points) if points is not None else None
    sa_sem0 = SAGeometry(g1.new_xyz, g1.idx, g1.pts_cnt, g1.npoint, g1.nsample, g1.order, g1.offsets, g1.rel, g1.gidx, g1.scan_order, feat4)
    ind_seed = _prefix_or_fps(fps[0], npoint_seed, xyz)
    ind_sem = _prefix_or_fps(fps[0], npoint_sem, xyz)
    l1, l2, l3, l4 = (g.new_xyz for g in sa)
    fp = [fp_geometry(l3, l4, sa[3].scan_order), fp_geometry(l2, l3, sa[2].scan_order), fp_geometry(l1, l2, sa[1].scan_order)]
    m1 = l1.shape[1]
    out = {"ind_seed": ind_seed, "ind_sem": ind_sem, "sa_shift": sa, "sa_sem": [sa_sem0] + sa[1:], "fp": fp}
    if not return_fullfea:
        # training: no dense queries -- the seed and sem rows onto l1 by one three_nn; the shift trunk's rows are its first npoint_seed
        q = torch.cat([gather_point(xyz, ind_seed), gather_point(xyz, ind_sem)], 1)
        dist, idx = three_nn(q, l1)
        out["fa4_sem"] = fp_geometry_from_nn(dist, idx, m1)
        out["fa4_shift"] = fp_geometry_from_nn(dist[:, :npoint_seed], idx[:, :npoint_seed], m1)
        return out
    # full feature: the cloud's 3-NN in l1..l4 -- one nested scan or one three_nn per level
    if nested:
        local = nested_local_maps(m1, fps[1:])
        dist, idx = three_nn_nested(xyz, l1, local, order=g1.scan_order)
    else:
        res = [three_nn(xyz, lk, order=g1.scan_order) for lk in (l1, l2, l3, l4)]
        dist, idx = [r[0] for r in res], [r[1] for r in res]
    sizes = [g.npoint for g in sa]
    out["fpn"] = [fp_geometry_from_nn(dist[k], idx[k], sizes[k]) for k in (3, 2, 1, 0)]
    # fa_layer4: a seed / sem query is the cloud point it was sampled from, bit for bit -- its rows are the cloud's rows in l1
    d1, i1 = dist[0], idx[0]
    ds, is_ = _rows(d1, ind_seed), _rows(i1, ind_seed)
    out["fa4_shift"] = fp_geometry_from_nn(torch.cat([ds, d1], 1), torch.cat([is_, i1], 1), m1)
    out["fa4_sem"] = fp_geometry_from_nn(torch.cat([ds, _rows(d1, ind_sem), d1], 1), torch.cat([is_, _rows(i1, ind_sem), i1], 1), m1)
    return out


def _check_geometry(geometry, npoint_seed, npoint_sem, return_fullfea):
    if geometry is None:
        return
    if geometry["ind_seed"].shape[1] != npoint_seed or (npoint_sem is not None and geometry["ind_sem"].shape[1] != npoint_sem):
        raise ValueError("spn trunk: precomputed geometry was built for other sample counts")
    if bool(return_fullfea) != ("fpn" in geometry):
        raise ValueError("spn trunk: precomputed geometry was built for return_fullfea=%s" % ("fpn" in geometry))


def _sa_stack(xyz, points, is_training, bn_decay, sa):
    outs, cur_xyz, cur_pts = [], xyz, points
    for level, (npoint, radius, nsample, mlp) in enumerate(SPN_SA_SPEC):
        cur_xyz, cur_pts, _ = pointnet_sa_module(cur_xyz, cur_pts, npoint=npoint, radius=radius, nsample=nsample, mlp=mlp, mlp2=None,
                                                 group_all=False, is_training=is_training, bn_decay=bn_decay, scope='layer%d' % (level + 1),
                                                 geometry=sa[level])
        outs.append((cur_xyz, cur_pts))
    return outs


def _fp_stack_123(levels, is_training, bn_decay, fp):
    (l1_xyz, l1_points), (l2_xyz, l2_points), (l3_xyz, l3_points), (l4_xyz, l4_points) = levels
    l3_points = pointnet_fp_module(l3_xyz, l4_xyz, l3_points, l4_points, SPN_FP_MLP[0], is_training, bn_decay, scope='fa_layer1', geometry=fp[0])
    l2_points = pointnet_fp_module(l2_xyz, l3_xyz, l2_points, l3_points, SPN_FP_MLP[1], is_training, bn_decay, scope='fa_layer2', geometry=fp[1])
    l1_points = pointnet_fp_module(l1_xyz, l2_xyz, l1_points, l2_points, SPN_FP_MLP[2], is_training, bn_decay, scope='fa_layer3', geometry=fp[2])
    return l1_points


def shift_pred_net(xyz, points, npoint_seed, end_points, scope, is_training, bn_decay=None, return_fullfea=False, geometry=None):
    """model_rpointnet.py:79-127.  xyz (b,n,3); points is not used (the reference predicts shifts from coordinates alone).
    end_points gains pc_seed (b,npoint_seed,3), shift_pred_seed_4d (b,npoint_seed,4), ind_seed (b,npoint_seed) int32 and, with
    return_fullfea, shift_pred_full_4d (b,n,4).  geometry (extension): spn_geometry(xyz, npoint_seed, ...); None computes it inline."""
    _check_geometry(geometry, npoint_seed, None, return_fullfea)
    with tf_util.variable_scope(scope):
        num_point = xyz.shape[1]
        ind_seed = farthest_point_sample(npoint_seed, xyz) if geometry is None else geometry["ind_seed"]
        pc_seed = gather_point(xyz, ind_seed)
        sa = geometry["sa_shift"] if geometry is not None else (None,) * 4
        fp = geometry["fp"] if geometry is not None else (None,) * 3
        levels = _sa_stack(xyz, None, is_training, bn_decay, sa)           # l0_points = None: no colour for shift prediction
        l1_points = _fp_stack_123(levels, is_training, bn_decay, fp)
        l1_xyz = levels[0][0]
        # the query set [seed(; cloud)] is only needed to compute the 3-NN inline
        new_xyz = None if geometry is not None else (torch.cat([pc_seed, xyz], 1) if return_fullfea else pc_seed)
        l0_points = pointnet_fp_module(new_xyz, l1_xyz, None, l1_points, SPN_FP_MLP[3], is_training, bn_decay, scope='fa_layer4',
                                       geometry=None if geometry is None else geometry["fa4_shift"])
        net = tf_util.conv1d(l0_points, 4, 1, padding='VALID', stride=1, scope='conv_shift_pred', activation_fn=None)
        if return_fullfea:
            shift_pred_seed_4d, shift_pred_full_4d = torch.split(net, [npoint_seed, num_point], dim=1)
            end_points['shift_pred_full_4d'] = shift_pred_full_4d
        else:
            shift_pred_seed_4d = net
        end_points['pc_seed'] = pc_seed
        end_points['shift_pred_seed_4d'] = shift_pred_seed_4d
        end_points['ind_seed'] = ind_seed
        return end_points


def _fpn_rows(xyz, lk_xyz, points, lk_points, g, scope):
    """pointnet_fp_module(xyz, lk_xyz, points, lk_points, [], ...) (:175-179): the N-row [interp, colour] matrix written by the fused
    interpolate + concat kernel (fp_concat) with its 16-byte row pitch, viewed as (b, N, c2 + c1)"""
    with tf_util.variable_scope(scope):
        if g is None:
            g = fp_geometry(xyz, lk_xyz)
        b, n = g.idx.shape[0], g.idx.shape[1]
        c = lk_points.shape[2] + points.shape[2]
        rows = fp_concat(lk_points, g.idx, g.weight, points, g.order, g.offsets)
        return rows.view(b, n, rows.shape[1])[:, :, :c]


def sem_net(xyz, points, npoint_sem, num_category, ind_seed, end_points, scope, is_training, bn_decay=None, return_fullfea=False, mode='training',
            geometry=None):
    """model_rpointnet.py:129-206.  xyz (b,n,3), points (b,n,c) colours, ind_seed (b,npoint_seed) int32.  end_points gains ind_sem,
    sem_fea_seed, sem_fea (and sem_fea_full, sem_fea_full_l1..l4 with return_fullfea) and sem_class_logits -- over the sem points for
    mode='training', over the full cloud for mode='inference' (which needs return_fullfea).  geometry (extension): spn_geometry(...)."""
    if mode not in ('training', 'inference'):
        raise ValueError("sem_net: mode must be 'training' or 'inference'")
    if mode == 'inference' and not return_fullfea:
        raise ValueError("sem_net: mode='inference' classifies sem_fea_full, which needs return_fullfea=True")
    npoint_seed = ind_seed.shape[1]
    _check_geometry(geometry, npoint_seed, npoint_sem, return_fullfea)
    if geometry is not None and ind_seed.data_ptr() != geometry["ind_seed"].data_ptr():
        # fa_layer4's seed rows come from the geometry, their colours from ind_seed: both must be the same sample (no host sync to compare values)
        raise ValueError("sem_net: with geometry=, pass ind_seed = geometry['ind_seed'] (end_points['ind_seed'] of shift_pred_net on that geometry)")
    with tf_util.variable_scope(scope):
        num_point = xyz.shape[1]
        ind_sem = farthest_point_sample(npoint_sem, xyz) if geometry is None else geometry["ind_sem"]
        end_points['ind_sem'] = ind_sem
        new_points_sem = gather_point(points, ind_sem)
        new_points_seed = gather_point(points, ind_seed)
        parts = [new_points_seed, new_points_sem] + ([points] if return_fullfea else [])
        new_points = torch.cat(parts, 1)
        sa = geometry["sa_sem"] if geometry is not None else (None,) * 4
        fp = geometry["fp"] if geometry is not None else (None,) * 3
        levels = _sa_stack(xyz, points, is_training, bn_decay, sa)
        if return_fullfea:
            fpn = geometry["fpn"] if geometry is not None else (None,) * 4
            for k, (lk, key) in enumerate(((3, 'sem_fea_full_l4'), (2, 'sem_fea_full_l3'), (1, 'sem_fea_full_l2'), (0, 'sem_fea_full_l1'))):
                end_points[key] = _fpn_rows(xyz, levels[lk][0], points, levels[lk][1], fpn[k], 'fa_layer%d_fpn' % (k + 1))
        l1_points = _fp_stack_123(levels, is_training, bn_decay, fp)
        new_xyz = None
        if geometry is None:
            qs = [gather_point(xyz, ind_seed), gather_point(xyz, ind_sem)] + ([xyz] if return_fullfea else [])
            new_xyz = torch.cat(qs, 1)
        l0_points = pointnet_fp_module(new_xyz, levels[0][0], new_points, l1_points, SPN_FP_MLP[3], is_training, bn_decay, scope='fa_layer4',
                                       geometry=None if geometry is None else geometry["fa4_sem"])
        net = tf_util.conv1d(l0_points, 128, 1, padding='VALID', bn=True, is_training=is_training, scope='fc1', bn_decay=bn_decay)
        if return_fullfea:
            sem_fea_seed, sem_fea, sem_fea_full = torch.split(net, [npoint_seed, npoint_sem, num_point], dim=1)
            end_points['sem_fea_full'] = sem_fea_full
        else:
            sem_fea_seed, sem_fea = torch.split(net, [npoint_seed, npoint_sem], dim=1)
        end_points['sem_fea_seed'] = sem_fea_seed
        end_points['sem_fea'] = sem_fea
        net = end_points['sem_fea'] if mode == 'training' else end_points['sem_fea_full']
        net = tf_util.dropout(net, keep_prob=0.5, is_training=is_training, scope='dp1')
        end_points['sem_class_logits'] = tf_util.conv1d(net, num_category, 1, padding='VALID', activation_fn=None, scope='fc2')
        return end_points
