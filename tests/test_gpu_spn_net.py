"""GPU tests of shape_proposal_net (gspn_amd/shape_proposal.py) and of rpointnet / get_loss (gspn_amd/rpointnet.py): the dictionary's keys,
shapes and variable names, the glue that can be read off the dictionary against fp32 restatements, the composition against its public
parts called by hand, get_loss against the float64 restatement of tests/spn_ref.py, and one captured step at the reference's operating
point.

Whole-network values or gradients against float64 are deliberately not asked for: the parts are held to float64 where they live, and
test_gpu_spn_trunks.test_trunks_training_match_oracle_composition records why whole-trunk gradients cannot be."""
import pytest
import torch

from gspn_amd import synth
from tests import spn_ref as SR
from tests.test_gpu_modules import fresh_store, rel_err

pytestmark = pytest.mark.gpu

DECAY = 0.5
B, N, NSMP, NGROUP, NINS, NCAT = 2, 4096, 64, 12, 512, 9
INVALID = (2, 5, 11)
SEM = 1024


def scene(seed=5, b=B, n=N, ngroup=NGROUP, nins=NINS, ncat=NCAT, invalid=INVALID, stray=0.05):
    d = synth.spn_batch("S", b, n, ngroup, nins, ncat, seed, invalid=invalid, stray=stray)
    return {k: torch.from_numpy(v).cuda() for k, v in d.items()}


def net(sc, training, full=False, mode='training', noise=None, nsmp=NSMP, ncat=NCAT, **kw):
    from gspn_amd.shape_proposal import shape_proposal_net
    return shape_proposal_net(sc["pc"], sc["color"], sc["pc_ins"], sc["group_label"], sc["group_indicator"], ncat, 'shape_proposal_net',
                              training, bn_decay=DECAY, nsmp=nsmp, return_fullfea=full, mode=mode, noise=noise, **kw)


# ---- 1. structure -------------------------------------------------------------------------------------------------------------------

KEYS = {            # :419-432
    'shift_pred_seed': (B, NSMP, 3), 'shift_pred_seed_4d': (B, NSMP, 4), 'pc_seed': (B, NSMP, 3), 'ind_seed': (B, NSMP),
    'pc_ins_centered_seed': (B, NSMP, NINS, 3), 'pc_ins_center_seed': (B, NSMP, 1, 3), 'mean': (B, NSMP, 256), 'log_var': (B, NSMP, 256),
    'cmean': (B, NSMP, 256), 'clog_var': (B, NSMP, 256), 'fb_logits': (B, NSMP, 2), 'fb_prob': (B, NSMP, 2),
    'pc_ins_pred': (B, NSMP, NINS, 3), 'bbox_ins_pred': (B, NSMP, 6),
}
TRUNK_KEYS = {'ind_sem': (B, SEM), 'sem_fea_seed': (B, NSMP, 128), 'sem_fea': (B, SEM, 128), 'sem_class_logits': (B, SEM, NCAT)}
FULL_KEYS = {'shift_pred_full_4d': (B, N, 4), 'sem_fea_full': (B, N, 128), 'sem_fea_full_l1': (B, N, 64 + 3), 'sem_fea_full_l2': (B, N, 128 + 3),
             'sem_fea_full_l3': (B, N, 256 + 3), 'sem_fea_full_l4': (B, N, 512 + 3), 'entity_fea': (B, N, 768), 'center_pos': (B, N, 3),
             'sem_class_logits': (B, N, NCAT)}

BN = ["bn/beta", "bn/gamma", "bn/moving_mean", "bn/moving_variance"]


def _layer(name, bn=True):
    return [name + "/" + v for v in ["weights", "biases"] + (BN if bn else [])]


def _upconv(name, bn=True):
    return [name + "/" + v for v in ["weights", "conv2d_transpose/kernel", "conv2d_transpose/bias"] + (BN if bn else [])]


def _trunk():
    names = []
    for level in (1, 2, 3, 4):
        for i in range(3):
            names += _layer("layer%d/conv%d" % (level, i))
    for fa, depth in ((1, 2), (2, 2), (3, 2), (4, 3)):
        for i in range(depth):
            names += _layer("fa_layer%d/conv_%d" % (fa, i))
    return names


def expected_variable_names():
    """the reference's creation order under shape_proposal_net/ (:347-402)"""
    names = ["shift_predictor/" + v for v in _trunk() + _layer("conv_shift_pred", False)]
    names += ["sem_predictor/" + v for v in _trunk() + _layer("fc1") + _layer("fc2", False)]
    names += ["instance_encoder/" + v for v in _layer("conv0") + _layer("conv1") + _layer("conv2") + _layer("fc0")]
    for k in range(3):
        for i in range(3):
            names += ["context_encoder/" + v for v in _layer("conv_prev_%d_%d" % (k, i))]
    for head in ("fb_logits", "mu_sigma_c", "mu_sigma_x"):
        names += [head + "/" + v for v in _layer("conv0") + _layer("conv1") + _layer("conv2", False)]
    names += _layer("dec_fc")
    dec = _upconv("upconv1") + _upconv("upconv2") + _upconv("upconv3") + _upconv("upconv4", False)      # 512 points: the third branch, with
    dec += _layer("de_fc2") + _layer("de_fc3") + _layer("de_fc4", False)                                 # each upconv's unused `weights`
    names += ["decoder/" + v for v in dec]
    return ["shape_proposal_net/" + v for v in names]


def test_structure_keys_shapes_and_variable_names():
    sc = scene()
    store = fresh_store(11)
    ep = net(sc, True)
    assert set(ep) == set(KEYS) | set(TRUNK_KEYS)
    for k, shape in {**KEYS, **TRUNK_KEYS}.items():
        assert tuple(ep[k].shape) == shape, k
    assert list(store.vars) == expected_variable_names()
    assert not ep['bbox_ins_pred'].requires_grad and ep['pc_ins_pred'].requires_grad
    ep = net(sc, False, full=True, mode='inference')
    assert set(ep) == set(KEYS) | set(TRUNK_KEYS) | set(FULL_KEYS)
    for k, shape in {**KEYS, **TRUNK_KEYS, **FULL_KEYS}.items():
        assert tuple(ep[k].shape) == shape, k
    assert list(store.vars) == expected_variable_names()          # entity_fea_prop and the fpn layers own no variables


# ---- 2. glue that can be read off the dictionary -----------------------------------------------------------------------------------

def test_glue_against_fp32_restatements():
    sc = scene()
    fresh_store(12)
    ep = {k: v.detach().cpu() for k, v in net(sc, False, full=True, mode='inference').items()}
    pc, pc_ins, label = sc["pc"].cpu(), sc["pc_ins"].cpu(), sc["group_label"].cpu()
    s4 = ep['shift_pred_seed_4d']
    assert torch.equal(ep['shift_pred_seed'], s4[:, :, :3] * s4[:, :, 3:])
    ind = ep['ind_seed'].long()
    assert torch.equal(ep['pc_seed'], torch.gather(pc, 1, ind.unsqueeze(-1).expand(-1, -1, 3)))
    center = (pc_ins.amax(2, keepdim=True) + pc_ins.amin(2, keepdim=True)) / 2                          # :358
    centered = pc_ins - center
    lab_seed = torch.gather(label, 1, ind)
    rows = torch.arange(B).unsqueeze(1)
    assert torch.equal(ep['pc_ins_centered_seed'], centered[rows, lab_seed])
    assert torch.equal(ep['pc_ins_center_seed'], center[rows, lab_seed])
    assert torch.equal(ep['bbox_ins_pred'], SR.points_bbox(ep['pc_ins_pred'], ep['pc_seed']))          # :406-408
    for k in ('log_var', 'clog_var'):
        assert float(ep[k].min()) >= -10.0 and float(ep[k].max()) <= 1.0
    f4 = ep['shift_pred_full_4d']
    assert torch.equal(ep['center_pos'], pc + f4[:, :, :3] * f4[:, :, 3:])
    assert float((ep['fb_prob'] - torch.softmax(ep['fb_logits'].double(), -1)).abs().max()) < 1e-6


# ---- 3. the composition against its public parts called by hand ---------------------------------------------------------------------

def by_hand(sc, training, noise, all_instances=False, full=False, mode='training'):
    """shape_proposal_net restated from the public parts, in the reference's order (:339-432), with plain torch glue"""
    from gspn_amd import tf_util
    from gspn_amd.proposal_head import fea_trans_net, multi_encoding_net
    from gspn_amd.shape_proposal import decoding_net, sample, single_encoding_net
    from gspn_amd.spn_trunks import sem_net, shift_pred_net
    pc, color, pc_ins, label, indicator = sc["pc"], sc["color"], sc["pc_ins"], sc["group_label"], sc["group_indicator"]
    with tf_util.variable_scope('shape_proposal_net'):
        ep = shift_pred_net(pc, color, NSMP, {}, 'shift_predictor', training, bn_decay=DECAY, return_fullfea=full)
        pc_seed, s4, ind_seed = ep['pc_seed'], ep['shift_pred_seed_4d'], ep['ind_seed']
        shift = s4[:, :, :3] * s4[:, :, 3:]
        ep = sem_net(pc, color, SEM, NCAT, ind_seed, ep, 'sem_predictor', training, bn_decay=DECAY, return_fullfea=full, mode=mode)
        sem_fea_seed = ep['sem_fea_seed']
        center = (pc_ins.amax(2, keepdim=True) + pc_ins.amin(2, keepdim=True)) / 2
        centered = pc_ins - center
        idx = torch.nonzero(torch.ones_like(indicator) if all_instances else indicator > 0)
        fea_list = single_encoding_net(centered[idx[:, 0], idx[:, 1]], [64, 256, 512], [256], 'instance_encoder', training, DECAY)
        fea = torch.zeros(pc.shape[0], pc_ins.shape[1], fea_list.shape[1], device=pc.device)
        fea[idx[:, 0], idx[:, 1]] = fea_list
        if all_instances:
            fea = fea * (indicator > 0).unsqueeze(-1)
        lab_seed = torch.gather(label, 1, ind_seed.long())
        rows = torch.arange(pc.shape[0], device=pc.device).unsqueeze(1)
        fea_seed = fea[rows, lab_seed]
        _, ctx, _, _ = multi_encoding_net(pc, color, NSMP, [0.5, 1.0, 1.5], [256, 256, 512], [[64, 128, 256]] * 3, [], training, DECAY,
                                          scope='context_encoder', use_xyz=True, output_shift=False, shift_pred=shift.detach(), fps_idx=ind_seed)
        fb_logits = fea_trans_net(ctx, [256, 64, 2], 'fb_logits', training, DECAY)
        mu_c = fea_trans_net(torch.cat((sem_fea_seed, ctx), -1), [256, 512, 512], 'mu_sigma_c', training, DECAY)
        mu_x = fea_trans_net(torch.cat((sem_fea_seed, ctx, fea_seed), -1), [256, 512, 512], 'mu_sigma_x', training, DECAY)
        mean, log_var = mu_x[:, :, :256], mu_x[:, :, 256:].clamp(-10.0, 1.0)
        cmean, clog_var = mu_c[:, :, :256], mu_c[:, :, 256:].clamp(-10.0, 1.0)
        z = sample(mean, log_var, noise) if training else cmean
        gc = tf_util.conv1d(ctx, 256, 1, padding='VALID', bn=True, is_training=training, scope='dec_fc', bn_decay=DECAY)
        pred = decoding_net(torch.cat((z, gc), -1), pc_ins.shape[2], 'decoder', is_training=training, bn_decay=DECAY)
        pred = pred + shift.detach().unsqueeze(2)
        ep.update(shift_pred_seed=shift, pc_ins_centered_seed=centered[rows, lab_seed], pc_ins_center_seed=center[rows, lab_seed], mean=mean,
                  log_var=log_var, cmean=cmean, clog_var=clog_var, fb_logits=fb_logits, fb_prob=torch.softmax(fb_logits, -1), pc_ins_pred=pred)
        ep['_instance_fea'] = fea
        ep['_lab_seed'] = lab_seed
        return ep


FLOAT_KEYS = [k for k in list(KEYS) + list(TRUNK_KEYS) if k not in ('ind_seed', 'ind_sem', 'bbox_ins_pred')]


def test_composition_eval_bit_equal_to_parts_by_hand():
    sc = scene()
    fresh_store(13)
    got = net(sc, False)
    fresh_store(13)
    want = by_hand(sc, False, None)
    assert torch.equal(got['ind_seed'], want['ind_seed']) and torch.equal(got['ind_sem'], want['ind_sem'])
    for k in FLOAT_KEYS:
        assert torch.equal(got[k], want[k]), k
    # the scene has seeds on stray points of invalid groups: their instance feature row is zero in the scattered tensor
    lab = want['_lab_seed']
    stray = (sc["group_indicator"].gather(1, lab) == 0)
    assert bool(stray.any())
    for g in INVALID:
        assert not want['_instance_fea'][:, g].any()


def test_composition_training_matches_parts_by_hand():
    sc = scene()
    noise = torch.randn(B, NSMP, 256, generator=torch.Generator().manual_seed(3)).cuda()
    fresh_store(14)
    got = net(sc, True, noise=noise)
    fresh_store(14)
    want = by_hand(sc, True, noise)
    for k in FLOAT_KEYS:
        if k == 'sem_class_logits':
            continue                                       # behind dropout: another mask in every call
        assert rel_err(got[k], want[k]) < 1e-5, k
    # valid_idx computed ahead gives the same selection
    from gspn_amd.shape_proposal import valid_instances
    fresh_store(14)
    again = net(sc, True, noise=noise, valid_idx=valid_instances(sc["group_indicator"]))
    assert rel_err(again['mean'], want['mean']) < 1e-5 and rel_err(again['pc_ins_pred'], want['pc_ins_pred']) < 1e-5
    # the instance encoder saw only the valid instances: with all 12 its batch-norm statistics, hence mean / log_var, differ
    fresh_store(14)
    other = by_hand(sc, True, noise, all_instances=True)
    assert rel_err(other['cmean'], want['cmean']) < 1e-5           # (no instance feature in the prior)
    assert rel_err(other['mean'], want['mean']) > 1e-3
    assert rel_err(got['mean'], other['mean']) > 1e-3


def test_instance_feature_gradient_is_a_one_hot_product():
    """several seeds add into one instance row; the gradient equals index_add in float64 and repeats bit for bit"""
    from gspn_amd.shape_proposal import _GatherRows
    g = torch.Generator().manual_seed(9)
    src = torch.randn(2, 100, 256, generator=g).cuda().requires_grad_(True)
    label = torch.randint(0, 100, (2, 256), generator=g).cuda()
    dy = torch.randn(2, 256, 256, generator=g).cuda()
    out = _GatherRows.apply(src, label)
    assert torch.equal(out, src.detach()[torch.arange(2, device="cuda").unsqueeze(1), label])
    g1, = torch.autograd.grad(out, src, dy, retain_graph=True)
    g2, = torch.autograd.grad(out, src, dy)
    assert torch.equal(g1, g2)
    want = torch.zeros(2, 100, 256, dtype=torch.float64)
    for b in range(2):
        want[b].index_add_(0, label[b].cpu(), dy[b].double().cpu())
    assert rel_err(g1, want) < 1e-5


def test_layer_wider_than_one_launch_matches_float64():
    """mu_sigma_x/conv0 has 128 + 768 + 256 = 1152 input channels, more than one MLP launch takes: row blocks of the same variables.
    Against float64: the batch-normalised ReLU layer forward, the linear layer forward and backward (no kink in it)."""
    from gspn_amd import tf_util
    g = torch.Generator().manual_seed(4)
    rows, cin, cout = 128, 1152, 256
    x = torch.randn(2, rows // 2, cin, generator=g).cuda().requires_grad_(True)
    dy = torch.randn(rows, cout, generator=g).cuda()
    store = fresh_store(16)
    y = tf_util.conv1d(x, cout, 1, padding='VALID', bn=True, is_training=True, scope='wide', bn_decay=DECAY)
    w, b = (store.vars['wide/' + k].detach().double().cpu() for k in ('weights', 'biases'))
    assert tuple(store.vars['wide/weights'].shape) == (1, cin, cout) and 'wide/bn/gamma' in store.vars
    lin = x.detach().double().cpu().reshape(rows, cin) @ w.view(cin, cout) + b
    ref = torch.relu((lin - lin.mean(0)) / torch.sqrt(lin.var(0, unbiased=False) + 1e-3))          # gamma 1, beta 0 at creation
    assert rel_err(y.reshape(rows, cout), ref) < 1e-5
    y = tf_util.conv1d(x, cout, 1, padding='VALID', activation_fn=None, scope='wide_linear')
    wp, bp = store.vars['wide_linear/weights'], store.vars['wide_linear/biases']
    with torch.no_grad():
        bp.copy_(torch.randn(cout, generator=g))
    y = tf_util.conv1d(x, cout, 1, padding='VALID', activation_fn=None, scope='wide_linear')
    gx, gw, gb = torch.autograd.grad(y.reshape(rows, cout), (x, wp, bp), dy)
    x64 = x.detach().double().cpu().reshape(rows, cin).requires_grad_(True)
    w64, b64 = wp.detach().double().cpu().view(cin, cout).requires_grad_(True), bp.detach().double().cpu().requires_grad_(True)
    ref = x64 @ w64 + b64
    rx, rw, rb = torch.autograd.grad(ref, (x64, w64, b64), dy.double().cpu())
    assert rel_err(y.reshape(rows, cout), ref) < 1e-5
    assert rel_err(gx.reshape(rows, cin), rx) < 1e-5 and rel_err(gw.view(cin, cout), rw) < 1e-5 and rel_err(gb, rb) < 1e-5


# ---- 4. get_loss against float64 -----------------------------------------------------------------------------------------------------

def loss_inputs(seed, all_background=False):
    """synthetic end_points of the training shapes: 2 x 256 seeds, 512 points, 100 groups, 1024 sem points, 19 categories; scene 1's seeds
    are all background"""
    b, nsmp, nins, ngroup, nsem, ncat, n = 2, 256, 512, 100, 1024, 19, 4096
    g = torch.Generator().manual_seed(seed)
    room = torch.tensor([8.0, 6.0, 3.0])
    prop, _, gt_cls, gt = SR.seeded_target_inputs(seed, b=b, s=nsmp, g=ngroup)
    ind_seed = torch.stack([torch.randperm(n, generator=g)[:nsmp] for _ in range(b)]).int()
    ind_sem = torch.stack([torch.randperm(n, generator=g)[:nsem] for _ in range(b)]).int()
    seg = torch.randint(0, ncat, (b, n), generator=g)
    fg = (torch.rand(nsmp, generator=g) < 0.7).long() * torch.randint(1, ncat, (nsmp,), generator=g)
    seg[0, ind_seed[0].long()] = fg
    seg[1, ind_seed[1].long()] = 0
    if all_background:
        seg[:, :] = 0
    ep = {
        'pc_ins_centered_seed': torch.randn(b, nsmp, nins, 3, generator=g) * 0.5,
        'pc_ins_center_seed': torch.rand(b, nsmp, 1, 3, generator=g) * room,
        'pc_seed': torch.rand(b, nsmp, 3, generator=g) * room,
        'shift_pred_seed_4d': torch.randn(b, nsmp, 4, generator=g),
        'fb_logits': torch.randn(b, nsmp, 2, generator=g),
        'pc_ins_pred': torch.randn(b, nsmp, nins, 3, generator=g) * 0.5,
        'sem_class_logits': torch.randn(b, nsem, ncat, generator=g),
        'mean': torch.randn(b, nsmp, 256, generator=g), 'cmean': torch.randn(b, nsmp, 256, generator=g),
        'log_var': torch.rand(b, nsmp, 256, generator=g) * 4.0 - 3.0, 'clog_var': torch.rand(b, nsmp, 256, generator=g) * 4.0 - 3.0,
        'ind_seed': ind_seed, 'ind_sem': ind_sem, 'seg_label': seg, 'seg_label_per_group': gt_cls.int(), 'bbox_ins': gt, 'bbox_ins_pred': prop,
    }
    smpw = torch.rand(b, n, generator=g) * (torch.rand(b, n, generator=g) >= 0.3)
    return ep, smpw


def run_get_loss(ep, smpw, alpha):
    from gspn_amd.rpointnet import Config, get_loss
    dev = {k: v.cuda() for k, v in ep.items()}
    for k in SR.LOSS_GRAD_KEYS:
        dev[k].requires_grad_(True)
    loss, out = get_loss(dev, Config(), alpha, smpw.cuda())
    grads = torch.autograd.grad(loss, [dev[k] for k in SR.LOSS_GRAD_KEYS])
    return out, dict(zip(SR.LOSS_GRAD_KEYS, grads))


TERMS = ('spn_class_loss', 'recons_loss', 'shift_loss', 'sem_loss', 'kl_loss', 'loss')


def test_get_loss_matches_float64():
    alpha = 0.7
    ep, smpw = loss_inputs(21)
    out, grads = run_get_loss(ep, smpw, alpha)
    # spn_match: exact wherever the largest IoU is clear of the threshold, which must be everywhere
    fb_gt = (torch.gather(ep['seg_label'], 1, ep['ind_seed'].long()) > 0).float()
    want_match, iou = SR.spn_target_gen_batch(ep['bbox_ins_pred'], fb_gt, (ep['seg_label_per_group'] > 0).float(), ep['bbox_ins'])
    assert bool(((iou - 0.5).abs() > 1e-5).all())
    got_match = out['spn_match'].cpu()
    assert got_match.dtype == torch.int32 and torch.equal(got_match, want_match)
    assert all(bool((got_match == v).any()) for v in (1, -1, 0))
    assert not bool(fb_gt[1].any()) and bool((smpw == 0).any())
    ref_ep = {k: (v.double().requires_grad_(True) if k in SR.LOSS_GRAD_KEYS else (v.double() if v.is_floating_point() else v)) for k, v in ep.items()}
    ref = SR.get_loss_ref(ref_ep, alpha, smpw.double(), want_match)
    assert float((ref['smooth_l1_diff'] - 1.0).abs().min()) > 1e-4          # no input on the smooth-L1 kink
    assert torch.equal(out['sem_labels'].cpu(), ref['sem_labels'])
    for k in TERMS:
        err = abs(float(out[k].detach()) - float(ref[k].detach())) / abs(float(ref[k].detach()))
        print("get_loss %s: %.9g vs %.9g, relative error %.3g" % (k, float(out[k].detach()), float(ref[k].detach()), err))
        assert err < 1e-5, k
    ref_grads = torch.autograd.grad(ref['loss'], [ref_ep[k] for k in SR.LOSS_GRAD_KEYS])
    for k, rg in zip(SR.LOSS_GRAD_KEYS, ref_grads):
        err = rel_err(grads[k], rg)
        print("get_loss gradient %s: relative error %.3g" % (k, err))
        assert err < 1e-5, k


def test_get_loss_with_every_seed_background():
    ep, smpw = loss_inputs(22, all_background=True)
    out, grads = run_get_loss(ep, smpw, 1.0)
    for k in ('recons_loss', 'shift_loss', 'kl_loss'):
        assert float(out[k]) == 0.0
    for k in TERMS:
        assert bool(torch.isfinite(out[k]))
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert not bool((out['spn_match'] == 1).any())


# ---- 5. rpointnet + get_loss + backward as one captured step ---------------------------------------------------------------------------

def test_rpointnet_keys_and_seg_label_per_group():
    from gspn_amd.rpointnet import Config, rpointnet
    cfg = Config()
    cfg.NUM_SAMPLE, cfg.NUM_GROUP, cfg.NUM_CATEGORY, cfg.BATCH_SIZE, cfg.NUM_POINT, cfg.SHRINK_BOX = NSMP, NGROUP, NCAT, B, N, True
    sc = scene()
    fresh_store(15)
    ep = rpointnet(sc["pc"], sc["color"], sc["pc_ins"], sc["group_label"], sc["group_indicator"], sc["seg_label"], sc["bbox_ins"], cfg, True,
                   bn_decay=DECAY)
    assert set(ep) == set(KEYS) | set(TRUNK_KEYS) | {'group_label', 'seg_label', 'seg_label_per_group', 'bbox_ins'}
    # every point of a group carries the group's category: the rounded mean is that category, 0 for the groups without points
    seg, lab = sc["seg_label"].cpu(), sc["group_label"].cpu()
    want = torch.zeros(B, NGROUP, dtype=torch.int32)
    for b in range(B):
        for g in range(NGROUP):
            m = lab[b] == g
            want[b, g] = int(seg[b][m][0]) if bool(m.any()) else 0
    assert ep['seg_label_per_group'].dtype == torch.int32 and torch.equal(ep['seg_label_per_group'].cpu(), want)


def test_spn_step_captured_full_size():
    from gspn_amd import parallel
    from gspn_amd.graph import CapturedStep
    from gspn_amd.rpointnet import Config, get_loss, rpointnet
    from gspn_amd.shape_proposal import check_spn_inputs, valid_instances
    from gspn_amd.spn_trunks import spn_geometry
    cfg = Config()                                         # 2 x 18000, 256 seeds, 100 groups of 512 points, 19 categories
    cfg.SHRINK_BOX = True
    sc = scene(seed=50, b=cfg.BATCH_SIZE, n=cfg.NUM_POINT, ngroup=cfg.NUM_GROUP, nins=cfg.NUM_POINT_INS, ncat=cfg.NUM_CATEGORY,
               invalid=(7, 31, 64, 99), stray=0.01)
    check_spn_inputs(sc["pc"], sc["pc_ins"], sc["group_label"], sc["group_indicator"])
    store = fresh_store(48)
    geo = spn_geometry(sc["pc"], cfg.NUM_SAMPLE, SEM, points=sc["color"])
    valid = valid_instances(sc["group_indicator"])
    noise = torch.randn(cfg.BATCH_SIZE, cfg.NUM_SAMPLE, 256, device="cuda")
    st = {}

    def step():
        for p in store.parameters():
            p.grad = None
        ep = rpointnet(sc["pc"], sc["color"], sc["pc_ins"], sc["group_label"], sc["group_indicator"], sc["seg_label"], sc["bbox_ins"], cfg,
                       True, bn_decay=DECAY, geometry=geo, noise=noise, valid_idx=valid)
        _, ep = get_loss(ep, cfg, 1.0, sc["smpw"])
        # sem_loss sits behind dropout, whose mask differs between the eager run and a replay: it enters with weight 0
        loss = ep['kl_loss'] * 1.0 + ep['recons_loss'] + ep['shift_loss'] + ep['spn_class_loss'] + 0.0 * ep['sem_loss']
        loss.backward()
        if "bucket" not in st:
            st["bucket"] = parallel.FlatGradBucket(store.parameters())
        st["bucket"].flatten()
        st["out"] = [ep[k].detach() for k in ('pc_ins_pred', 'bbox_ins_pred', 'spn_match', 'sem_loss')]
        return loss.detach()

    loss0 = step().clone()
    out0 = [o.clone() for o in st["out"]]
    flat0 = st["bucket"].flat.clone()
    cap = CapturedStep(step)
    st["bucket"].flat.zero_()
    loss1 = cap.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(loss0) and torch.isfinite(flat0).all() and all(bool(torch.isfinite(o.float()).all()) for o in out0)
    assert float(flat0.abs().max()) > 0
    assert bool(((out0[2] >= -1) & (out0[2] <= 1)).all())
    assert torch.allclose(loss1, loss0, rtol=1e-6)
    assert torch.allclose(st["out"][0], out0[0], rtol=1e-5, atol=1e-6)
    assert torch.allclose(st["out"][1], out0[1], rtol=1e-5, atol=1e-6)
    assert torch.isfinite(st["out"][3])
    assert torch.allclose(st["bucket"].flat, flat0, rtol=1e-4, atol=1e-7)


def test_spn_step_captured_full_size_with_the_flat_optimiser():
    """the step of test_spn_step_captured_full_size after parallel.FlatAdam has moved every parameter into one flat buffer, with the gradient sinks
    off and on.  sem_net's fc2 has 19 biases, so every parameter stored behind them -- and every gradient slice of the bucket -- starts on a 4-byte
    boundary only: the configuration in which the shared MLP, the transposed convolutions, the stand-alone batch norm and the row-blocked
    1152-channel layer see parameters that no fresh allocation would hand them.  Eager against a replay from CapturedStep and sinks off against
    sinks on at that test's tolerances; the moved step against the unmoved one: loss within rtol 1e-4 (what that test grants two executions of
    one step's gradients; a loss is smoother than a gradient), the bucket difference printed."""
    from gspn_amd import mlp, parallel
    from gspn_amd.graph import CapturedStep
    from gspn_amd.rpointnet import Config, get_loss, rpointnet
    from gspn_amd.shape_proposal import check_spn_inputs, valid_instances
    from gspn_amd.spn_trunks import spn_geometry
    cfg = Config()
    cfg.SHRINK_BOX = True
    sc = scene(seed=50, b=cfg.BATCH_SIZE, n=cfg.NUM_POINT, ngroup=cfg.NUM_GROUP, nins=cfg.NUM_POINT_INS, ncat=cfg.NUM_CATEGORY,
               invalid=(7, 31, 64, 99), stray=0.01)
    check_spn_inputs(sc["pc"], sc["pc_ins"], sc["group_label"], sc["group_indicator"])
    geo = spn_geometry(sc["pc"], cfg.NUM_SAMPLE, SEM, points=sc["color"])
    valid = valid_instances(sc["group_indicator"])
    noise = torch.randn(cfg.BATCH_SIZE, cfg.NUM_SAMPLE, 256, device="cuda")
    runs = {}
    for mode in ("unmoved", "moved", "moved+sinks"):
        store = fresh_store(48)
        st = {}

        def step():
            for p in store.parameters():
                p.grad = None
            ep = rpointnet(sc["pc"], sc["color"], sc["pc_ins"], sc["group_label"], sc["group_indicator"], sc["seg_label"], sc["bbox_ins"], cfg,
                           True, bn_decay=DECAY, geometry=geo, noise=noise, valid_idx=valid)
            _, ep = get_loss(ep, cfg, 1.0, sc["smpw"])
            loss = ep['kl_loss'] * 1.0 + ep['recons_loss'] + ep['shift_loss'] + ep['spn_class_loss'] + 0.0 * ep['sem_loss']
            loss.backward()
            if "bucket" not in st:                          # the first call creates the variables: bucket, optimiser and sinks come after it
                st["bucket"] = parallel.FlatGradBucket(store.parameters())
                if mode != "unmoved":
                    st["opt"] = parallel.FlatAdam(st["bucket"], lr=0.0)          # lr 0: the parameters move, their values stay
                if mode == "moved+sinks":
                    st["bucket"].attach_sinks()
            st["bucket"].flatten()
            st["out"] = [ep[k].detach() for k in ('pc_ins_pred', 'bbox_ins_pred', 'spn_match', 'sem_loss')]
            return loss.detach()

        try:
            step()
            bucket = st["bucket"]
            if mode != "unmoved":
                pres = sorted({p.data_ptr() % 16 for p in store.parameters()})
                gres = sorted({v.data_ptr() % 16 for v in bucket._views})
                print("%s: data-pointer residues of the parameters %s, of the gradient slices %s" % (mode, pres, gres))
                assert any(r != 0 for r in pres) and any(r != 0 for r in gres)
            bucket.flat.fill_(float("nan"))
            loss0 = step().clone()
            out0 = [o.clone() for o in st["out"]]
            flat0 = bucket.flat.clone()
            assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(store.parameters(), bucket._views))
            cap = CapturedStep(step)
            bucket.flat.fill_(float("nan"))
            loss1 = cap.replay()
            torch.cuda.synchronize()
            assert torch.isfinite(loss0) and torch.isfinite(flat0).all() and all(bool(torch.isfinite(o.float()).all()) for o in out0)
            assert torch.isfinite(bucket.flat).all() and float(flat0.abs().max()) > 0
            assert torch.allclose(loss1, loss0, rtol=1e-6)
            assert torch.allclose(st["out"][0], out0[0], rtol=1e-5, atol=1e-6)
            assert torch.allclose(st["out"][1], out0[1], rtol=1e-5, atol=1e-6)
            assert torch.allclose(bucket.flat, flat0, rtol=1e-4, atol=1e-7)
            runs[mode] = (loss0, out0, flat0)
        finally:
            if "bucket" in st:
                for k in [k for k, e in mlp.GRAD_SINKS.items() if e.bucket is st["bucket"]]:
                    del mlp.GRAD_SINKS[k]
    a, b = runs["moved"], runs["moved+sinks"]
    assert torch.allclose(b[0], a[0], rtol=1e-6)
    assert torch.allclose(b[1][0], a[1][0], rtol=1e-5, atol=1e-6) and torch.allclose(b[1][1], a[1][1], rtol=1e-5, atol=1e-6)
    assert torch.allclose(b[2], a[2], rtol=1e-4, atol=1e-7)
    u = runs["unmoved"]
    d = (a[2] - u[2]).abs()
    print("moved against unmoved step: loss %.9g / %.9g; bucket: largest difference %.3g (largest element %.3g), %d of %d elements outside rtol 1e-4, atol 1e-7"
          % (float(a[0]), float(u[0]), float(d.max()), float(u[2].abs().max()), int((d > 1e-7 + 1e-4 * u[2].abs()).sum()), d.numel()))
    assert torch.allclose(a[0], u[0], rtol=1e-4)
