"""GPU tests of gspn_amd/train.py and csrc/train.hip: gspn_batch_assemble's permutation against the int64 restatement train.batch_perm, its
augmentation bit for bit against dataset.augment_and_box fed the call's own draws, the two optimisers against torch.optim.SGD and a float64
restatement of TensorFlow's Adam, gspn_scalars_accumulate against float64 sums, and the driver at the operating point of
tests/test_gpu_spn_net.py: 2 x 4096 points, 64 seeds, 12 groups of 512 points, 9 categories."""
import math

import numpy as np
import pytest
import torch

from gspn_amd import synth, tf_util
from tests.test_gpu_modules import rel_err

pytestmark = pytest.mark.gpu

B, N, NSMP, NGROUP, NINS, NCAT = 2, 4096, 64, 12, 512, 9


def seed_word(v):
    return torch.tensor([v], dtype=torch.int64, device="cuda")


def make_cache(s, n, g, m, counts, seed):
    """a cache of s scenes whose pc rows are unique by construction: pc[k, i, 0] = i, pc[k, i, 1] = k"""
    from gspn_amd.train import DeviceDataset
    gen = torch.Generator().manual_seed(seed)
    pc = torch.rand(s, n, 3, generator=gen) * 4.0
    pc[:, :, 0] = torch.arange(n, dtype=torch.float32)
    pc[:, :, 1] = torch.arange(s, dtype=torch.float32).unsqueeze(1)
    color = torch.rand(s, n, 3, generator=gen)
    group = torch.randint(0, g, (s, n), generator=gen, dtype=torch.int32)
    seg = torch.randint(0, 19, (s, n), generator=gen, dtype=torch.int32)
    pc_ins = torch.randn(s, g, m, 3, generator=gen) * 2.0
    for k, c in enumerate(counts):
        pc_ins[k, c:] = 0.0
        pc_ins[k, 0] = 0.0                                                 # the background's row (dataset.py:148)
    cache = dict(pc=pc.cuda(), color=color.cuda(), group_label=group.cuda(), seg_label=seg.cuda(), pc_ins=pc_ins.cuda(),
                 ngroup=torch.tensor(counts, dtype=torch.int32).cuda())
    return cache, lambda **kw: DeviceDataset(**cache, **kw)


def gathered(cache, idx, perm):
    """the four point arrays of the cache at scenes idx, rows perm (B, n) -- what the permutation must give"""
    k = torch.tensor(idx, device="cuda").unsqueeze(1)
    return {name: cache[name][k, perm] for name in ("pc", "color", "group_label", "seg_label")}


# ---- 1. the permutation ------------------------------------------------------------------------------------------------------------

IDX = [2, 0, 3]


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1000, 4096])
def test_permutation_is_the_restatement_on_all_four_arrays(n):
    from gspn_amd.train import batch_perm
    cache, data = make_cache(4, n, 2, 4, [2, 1, 2, 2], seed=n)
    ds = data(is_augment=False, permute_points=True)
    out = ds.batch(IDX, seed_word(21))
    perm = batch_perm(seed_word(21), len(IDX), n)
    assert torch.equal(out["pc"][:, :, 0].long(), perm)                    # the source row of every output row, read off the unique column
    for name, want in gathered(cache, IDX, perm).items():
        assert out[name].dtype == want.dtype and torch.equal(out[name], want), name
    assert torch.equal(out["smpw"], torch.ones(len(IDX), n, device="cuda"))
    assert torch.equal(out["pc_ins"], cache["pc_ins"][IDX]) and out["group_indicator"].dtype == torch.int32
    if n >= 63:
        assert not torch.equal(perm[0], perm[1]) and not torch.equal(perm[1], perm[2])
        other = ds.batch(IDX, seed_word(22))
        assert not torch.equal(other["pc"], out["pc"])
        assert torch.equal(other["pc"][:, :, 0].long(), batch_perm(seed_word(22), len(IDX), n))
    plain = data(is_augment=False, permute_points=False).batch(IDX, seed_word(21))
    ident = torch.arange(n, device="cuda").expand(len(IDX), n)
    for name, want in gathered(cache, IDX, ident).items():
        assert torch.equal(plain[name], want), name


def test_permutation_spreads_over_seeds_and_has_few_fixed_points():
    n = 4096
    cache, data = make_cache(1, n, 1, 1, [1], seed=1)
    ds = data(is_augment=False, permute_points=True)
    first, worst = set(), 0
    ident = torch.arange(n, device="cuda")
    out = None
    for s in range(64):
        out = ds.batch([0], seed_word(1000 + s), out=out)
        src = out["pc"][0, :, 0].long()
        assert torch.equal(torch.sort(src).values, ident)
        first.add(int(src[0]))
        worst = max(worst, int((src == ident).sum()))
    print("source of position 0 over 64 seeds: %d distinct values; most fixed points of one permutation: %d" % (len(first), worst))
    assert len(first) >= 56 and worst <= 16


def test_seed_is_read_on_the_device_in_a_captured_call():
    from gspn_amd.graph import CapturedStep
    from gspn_amd.train import batch_perm
    n = 1000
    cache, data = make_cache(4, n, 2, 4, [2, 1, 2, 2], seed=5)
    ds = data(is_augment=True, permute_points=True)
    seed, idx = seed_word(40), torch.tensor(IDX, dtype=torch.int32, device="cuda")
    out = ds.empty_batch(len(IDX))
    cap = CapturedStep(lambda: ds.batch(idx, seed, out=out) and None)      # the capture itself proves that nothing is read back
    cap.replay()
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in out.items()}
    eager = ds.batch(idx, seed_word(40))
    for k in first:
        assert torch.equal(first[k], eager[k]), k
    seed.add_(1)
    cap.replay()
    torch.cuda.synchronize()
    assert not torch.equal(out["pc"], first["pc"]) and not torch.equal(out["rotation"], first["rotation"])
    want = ds.batch(idx, seed_word(41))
    for k in first:
        assert torch.equal(out[k], want[k]), k
    assert torch.equal(out["group_label"], gathered(cache, IDX, batch_perm(seed_word(41), len(IDX), n))["group_label"])


# ---- 2. the augmentation -----------------------------------------------------------------------------------------------------------

def draws_numpy(seed, slots):
    """R and t of include/gspn_hip.h in numpy float64"""
    from gspn_amd.train import AUGMENT_STREAM, rand32
    r = rand32(torch.tensor([seed], dtype=torch.int64), slots, AUGMENT_STREAM, 5).numpy().astype(np.float64)
    two_pi, inv = 6.283185307179586, 1.0 / 4294967296.0
    angle = (two_pi * r[:, 0]) * inv
    c, s, zero, one = np.cos(angle), np.sin(angle), np.zeros(slots), np.ones(slots)
    rot = np.stack([c, s, zero, -s, c, zero, zero, zero, one], 1).reshape(slots, 3, 3)
    z = []
    for p in range(2):
        u1, u2 = (r[:, 1 + 2 * p] + 1.0) * inv, r[:, 2 + 2 * p] * inv
        rad = np.sqrt(-2.0 * np.log(u1))
        z += [rad * np.cos(two_pi * u2), rad * np.sin(two_pi * u2)]
    return rot, np.stack(z[:3], 1)


@pytest.mark.parametrize("g", [1, 12])
@pytest.mark.parametrize("m", [1, 64, 512])
def test_augmentation_bit_equal_to_augment_and_box_on_the_calls_own_draws(g, m):
    from gspn_amd import dataset
    from gspn_amd.spn_boxes import points_bbox
    from gspn_amd.train import batch_perm
    n, counts, idx = 1000, [1, max(1, g // 2), g], [2, 0, 1]              # scenes holding 1, some and all G groups
    cache, data = make_cache(3, n, g, m, counts, seed=100 * g + m)
    out = data(is_augment=True, permute_points=True).batch(idx, seed_word(77))
    rot, tr = out["rotation"], out["translation"]
    assert rot.dtype == tr.dtype == torch.float64 and tuple(rot.shape) == (3, 3, 3) and tuple(tr.shape) == (3, 3)
    permuted = gathered(cache, idx, batch_perm(seed_word(77), 3, n))
    ngroup = cache["ngroup"][idx]
    pc, pc_ins, indicator, bbox = dataset.augment_and_box(permuted["pc"], cache["pc_ins"][idx].contiguous(), ngroup, rot, tr)
    assert torch.equal(out["pc"], pc) and torch.equal(out["pc_ins"], pc_ins)           # the operation order, and the zero rows transformed
    assert out["group_indicator"].dtype == indicator.dtype and torch.equal(out["group_indicator"], indicator)
    assert torch.equal(out["bbox_ins"], bbox)
    assert torch.equal(out["group_indicator"].sum(1).cpu(), torch.tensor([counts[k] for k in idx], dtype=torch.int64))
    for name in ("color", "group_label", "seg_label"):
        assert torch.equal(out[name], permuted[name]), name
    # the zero rows went through the transform: they hold t, rounded
    if g > 1:
        assert torch.equal(out["pc_ins"][1, 1:], tr[1].float().expand(g - 1, m, 3))
    # the stated structure, and the draws
    r = rot.cpu()
    assert torch.equal(r[:, 0, 0], r[:, 1, 1]) and torch.equal(r[:, 0, 1], -r[:, 1, 0])
    assert torch.equal(r[:, :, 2], torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand(3, 3))
    assert torch.equal(r[:, 2, :], torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand(3, 3))
    want_rot, want_t = draws_numpy(77, 3)
    err_r, err_t = float(np.abs(r.numpy() - want_rot).max()), float(np.abs(tr.cpu().numpy() - want_t).max())
    print("G %d, M %d: |R - numpy| <= %.3g, |t - numpy| <= %.3g" % (g, m, err_r, err_t))
    assert err_r <= 1e-14 and err_t <= 1e-14
    assert float(tr.abs().max()) > 0 and not torch.equal(r[0], r[1])

    # augment = 0: the coordinates pass through untouched
    plain = data(is_augment=False, permute_points=True).batch(idx, seed_word(77))
    assert torch.equal(plain["pc"], permuted["pc"]) and torch.equal(plain["pc_ins"], cache["pc_ins"][idx])
    assert torch.equal(plain["bbox_ins"], points_bbox(cache["pc_ins"][idx].contiguous()))
    assert torch.equal(plain["rotation"].cpu(), torch.eye(3, dtype=torch.float64).expand(3, 3, 3)) and not bool(plain["translation"].any())
    assert torch.equal(plain["group_indicator"], indicator)


def test_dataset_ngroup_is_settable_and_inputs_are_checked():
    cache, data = make_cache(3, 64, 4, 8, [1, 2, 3], seed=9)
    ds = data()
    assert len(ds) == 3 and ds.ngroup == 4
    ds.ngroup = 6                                                          # train.py:83-85
    out = ds.batch([1, 2], 3)
    assert tuple(out["pc_ins"].shape) == (2, 6, 8, 3) and tuple(out["group_indicator"].shape) == (2, 6) and tuple(out["bbox_ins"].shape) == (2, 6, 6)
    assert out["group_indicator"].cpu().tolist() == [[1, 1, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0]]
    ds.ngroup = 3
    assert ds.ngroup == 3
    with pytest.raises(ValueError):
        ds.ngroup = 2
    with pytest.raises(ValueError):
        ds.batch(torch.zeros(2, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        data(**{}).batch([0], out={k: v[:, :1] for k, v in ds.empty_batch(1).items()})


# ---- 3. the optimisers -------------------------------------------------------------------------------------------------------------

SHAPES = [(6, 32), (32,), (32, 64), (64,), (1, 1, 67, 64), (5,)]            # tests/test_gpu_modules.py::test_flat_adam_matches_torch_adam


def adam_tf_ref(params, grads, t, m, v, lr, b1=0.9, b2=0.999, eps=1e-8):
    """tf.train.AdamOptimizer in float64: lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t);  p -= lr_t * m / (sqrt(v) + eps)"""
    lr_t = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    for i, g in enumerate(grads):
        g = g.double().cpu()
        m[i] = b1 * m[i] + (1.0 - b1) * g
        v[i] = b2 * v[i] + (1.0 - b2) * g * g
        params[i] -= lr_t * m[i] / (v[i].sqrt() + eps)


def run_optimisers(grad_fn, steps):
    """FlatAdamTF, FlatMomentum, torch.optim.SGD(momentum), torch.optim.Adam and the float64 TensorFlow rule on the same fp32 gradients,
    the flat ones behind a bucket summed over 4 ranks and scaled back by grad_scale = 0.25"""
    from gspn_amd.parallel import FlatGradBucket
    from gspn_amd.train import FlatAdamTF, FlatMomentum
    g = torch.Generator().manual_seed(3)
    init = [torch.randn(*s_, generator=g) for s_ in SHAPES]
    make = lambda: [torch.nn.Parameter(t.clone().cuda()) for t in init]
    p_tf, p_mom, p_sgd, p_adam = make(), make(), make(), make()
    sgd, adam = torch.optim.SGD(p_sgd, lr=1e-2, momentum=0.9), torch.optim.Adam(p_adam, lr=1e-2)
    b_tf, b_mom = FlatGradBucket(p_tf), FlatGradBucket(p_mom)
    o_tf, o_mom = FlatAdamTF(b_tf, lr=1e-2), FlatMomentum(b_mom, lr=1e-2, momentum=0.9)
    ref = [t.double().clone() for t in init]
    m, v = [torch.zeros_like(t) for t in ref], [torch.zeros_like(t) for t in ref]
    for step in range(steps):
        grads = [grad_fn(s_, g, step).cuda() for s_ in SHAPES]
        for ps in (p_tf, p_mom, p_sgd, p_adam):
            for p_, gr in zip(ps, grads):
                p_.grad = gr.clone()
        sgd.step()
        adam.step()
        adam_tf_ref(ref, grads, step + 1, m, v, 1e-2)
        for bucket, opt in ((b_tf, o_tf), (b_mom, o_mom)):
            bucket.flatten()
            bucket.flat.mul_(4.0)
            opt.step(grad_scale=0.25)
    torch.cuda.synchronize()
    for ps, opt in ((p_tf, o_tf), (p_mom, o_mom)):
        assert all(opt.flat.data_ptr() <= q.data_ptr() < opt.flat.data_ptr() + opt.flat.numel() * 4 for q in ps)
    assert o_tf.t == o_mom.t == steps
    return p_tf, p_mom, p_sgd, p_adam, ref


def test_flat_momentum_and_flat_adam_tf_follow_their_rules():
    p_tf, p_mom, p_sgd, _, ref = run_optimisers(lambda s_, g, step: torch.randn(*s_, generator=g) * (10.0 ** (step - 3)), 6)
    for i in range(len(SHAPES)):
        e_mom, e_tf = rel_err(p_mom[i], p_sgd[i]), rel_err(p_tf[i], ref[i])
        print("%s: FlatMomentum against torch.optim.SGD %.3g, FlatAdamTF against the float64 TensorFlow rule %.3g" % (SHAPES[i], e_mom, e_tf))
        assert e_mom < 2e-6 and e_tf < 2e-6


def test_flat_adam_tf_is_the_tensorflow_rule_where_the_two_adams_part():
    """gradients of 1e-9: sqrt(v) is comparable to eps, where eps added to the raw root (TensorFlow) and to the bias-corrected root (torch)
    give different steps"""
    p_tf, _, _, p_adam, ref = run_optimisers(lambda s_, g, step: torch.randn(*s_, generator=g) * 1e-9, 3)
    for i in range(len(SHAPES)):
        e_tf, e_torch = rel_err(p_tf[i], ref[i]), rel_err(p_tf[i], p_adam[i])
        print("%s: FlatAdamTF against the float64 TensorFlow rule %.3g, against torch.optim.Adam %.3g" % (SHAPES[i], e_tf, e_torch))
        assert e_tf < 2e-6 and e_torch > 2e-6


# ---- 4. the running sums -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 9, 16])
def test_scalars_accumulate_against_float64_sums_eager_and_replayed(k):
    from gspn_amd.graph import CapturedStep
    from gspn_amd.train import ScalarSums
    gen = torch.Generator().manual_seed(k)
    values = (torch.randn(5, k, generator=gen) * 10.0 ** torch.randint(-6, 7, (5, k), generator=gen).float()).float()
    want = [0.0] * k
    for call in range(5):
        for i in range(k):
            want[i] = want[i] + float(values[call, i])                     # Python floats: float64 adds in the kernel's order
    scalars = [torch.zeros((), device="cuda") for _ in range(k)]            # k separate allocations
    sums = ScalarSums(k, "cuda")

    def fill(call):
        for i, t in enumerate(scalars):
            t.fill_(float(values[call, i]))

    for call in range(5):
        fill(call)
        sums.add(scalars)
    got, count = sums.read()
    assert got == want and count == 5
    assert sums.read() == ([0.0] * k, 0)                                   # read() zeroes
    fill(0)
    cap = CapturedStep(lambda: sums.add(scalars), warmup=1)
    sums.read()
    for call in range(5):
        fill(call)
        cap.replay()
    got, count = sums.read()
    assert got == want and count == 5
    with pytest.raises(ValueError):
        ScalarSums(17, "cuda")
    with pytest.raises(ValueError):
        sums.add(scalars + scalars)


# ---- 5. the driver -----------------------------------------------------------------------------------------------------------------

def datasets():
    """4 training scenes (two of them with 10 of the 12 groups) and 2 validation scenes"""
    from gspn_amd.train import DeviceDataset
    d = {k: torch.from_numpy(v) for k, v in synth.spn_batch("S", 6, N, NGROUP, NINS, NCAT, 70).items()}
    counts = [12, 10, 12, 10, 12, 12]
    for k, c in enumerate(counts):
        lab = d["group_label"][k]
        d["group_label"][k] = torch.where(lab >= c, lab - c, lab)           # the groups past the count have no points and zero rows
        d["pc_ins"][k, c:] = 0.0
    dev = {k: v.cuda() for k, v in d.items()}
    ngroup = torch.tensor(counts, dtype=torch.int32).cuda()
    part = lambda lo, hi, **kw: DeviceDataset(dev["pc"][lo:hi], dev["color"][lo:hi], dev["group_label"][lo:hi], dev["seg_label"][lo:hi],
                                              dev["pc_ins"][lo:hi], ngroup[lo:hi], **kw)
    return part(0, 4, is_augment=True, permute_points=True), part(4, 6, is_augment=False, permute_points=False)


def spn_config():
    from gspn_amd.rpointnet import Config
    cfg = Config()
    cfg.BATCH_SIZE, cfg.NUM_SAMPLE, cfg.NUM_CATEGORY = B, NSMP, NCAT
    return cfg


def heads_config():
    cfg = spn_config()
    cfg.SPN_PRE_NMS_LIMIT, cfg.SPN_NMS_MAX_SIZE_TRAINING, cfg.TRAIN_ROIS_PER_IMAGE, cfg.NUM_POINT_INS_MASK = 48, 32, 16, 64
    return cfg


def trainer(module, captured, log_dir=None, cfg=None):
    from gspn_amd.train import Schedules, Trainer
    train, val = datasets()
    # 2 steps per epoch: step * batch_size reaches decay_step = 6 at step 3, inside the second epoch
    return Trainer(cfg or spn_config(), train, val, train_module=module, schedules=Schedules(B, decay_step=6), log_dir=log_dir, seed=3,
                   captured=captured, log_every=1)


def snapshot(tr):
    return {n: v.detach().clone() for n, v in tr.store.vars.items()}


def watch(tr):
    seen = []
    tr.on_step = lambda info: seen.append(dict(info, terms={k: float(v) for k, v in info["terms"].items()}))
    return seen


class SpnRun:
    """two captured epochs of 'SPN', an evaluation between and after them, a checkpoint"""

    def __init__(self, tmp):
        self.log_dir = str(tmp)
        self.tr = tr = trainer('SPN', True, self.log_dir)
        self.seen = watch(tr)
        self.before = snapshot(tr)
        self.logged = tr.train_one_epoch()
        self.after_train = snapshot(tr)
        self.eval_loss, self.eval_means = tr.eval_one_epoch()
        self.after_eval = snapshot(tr)
        self.logged += tr.train_one_epoch()
        self.ckpt = tr.save(str(tmp / "spn.ckpt"))
        self.saved = snapshot(tr)


@pytest.fixture(scope="module")
def spn_run(tmp_path_factory):
    return SpnRun(tmp_path_factory.mktemp("train_spn"))


def test_spn_two_captured_epochs(spn_run):
    from gspn_amd.train import LOSS_TERMS, Schedules
    run, tr = spn_run, spn_run.tr
    assert tr.step == 4 and tr.opt.t == 4 and len(run.seen) == 4 and len(run.logged) == 4
    for means in run.logged:
        assert set(means) == set(LOSS_TERMS[:6]) and all(math.isfinite(v) for v in means.values()), means
    # with log_every = 1 a logged mean is the step's own value, as the reference's per-step sess.run reads it
    for means, info in zip(run.logged, run.seen):
        for k, v in means.items():
            assert v == info["terms"][k], k
    moving = [n for n in run.before if n not in set(tr.store.trainable)]
    assert len(moving) > 0 and len(tr.store.trainable) > 0
    # the parameters have moved -- all but those whose gradient is identically zero: a bias in front of a batch norm (the mean is
    # subtracted), <upconv>/weights, which the reference creates and never uses (tf_util.conv2d_transpose), and, while alpha is 0 (the
    # first epoch: steps 0 and 1), mu_sigma_c, which only the KL term reaches -- it has moved once the second epoch has weighted that term
    still = [n for n in tr.store.trainable if torch.equal(run.after_train[n], run.before[n])]
    print("%d of %d parameters did not move in the first epoch, %d of them biases"
          % (len(still), len(tr.store.trainable), sum(n.endswith("/biases") for n in still)))

    def zero_gradient(n):
        return (n.endswith("/biases") and n[:-len("biases")] + "bn/beta" in run.before) or "/mu_sigma_c/" in n or \
            ("/decoder/upconv" in n and n.endswith("/weights") and not n.endswith("conv2d_transpose/weights"))
    assert all(zero_gradient(n) for n in still), [n for n in still if not zero_gradient(n)]
    assert len(still) < len(tr.store.trainable) // 2
    assert run.seen[1]["alpha"] == 0.0 and run.seen[3]["alpha"] > 0.0
    assert not torch.equal(run.saved["shape_proposal_net/mu_sigma_c/conv0/weights"], run.before["shape_proposal_net/mu_sigma_c/conv0/weights"])
    assert all(not torch.equal(run.after_train[n], run.before[n]) for n in moving), "a moving statistic did not move in training"
    assert all(torch.equal(run.after_eval[n], run.after_train[n]) for n in run.before), "evaluation changed a variable"
    # the schedules in force, observed through the hook: the staircase moves at step 3, and the step was captured again for its bn_decay
    sch = Schedules(B, decay_step=6)
    for info in run.seen:
        s = info["step"]
        assert info["learning_rate"] == sch.learning_rate(s) and info["bn_decay"] == sch.bn_decay(s) and info["alpha"] == sch.loss_weight(s)
    assert [i["step"] for i in run.seen] == [0, 1, 2, 3]
    assert run.seen[2]["bn_decay"] == 0.5 and run.seen[3]["bn_decay"] == 0.75 and abs(run.seen[3]["learning_rate"] - 7e-4) < 1e-15
    assert run.seen[0]["recaptured"] and run.seen[3]["recaptured"]
    assert all(c.bn_decay == 0.75 for c in tr._captures.values())
    log = open(run.log_dir + "/log_train.txt").read()
    for line in (" -- 002 / 002 --", "mean loss: ", "mean reconstruction loss: ", "mean kl-divergence loss: ", "mean shift loss: ",
                 "mean sem loss: ", "mean spn class loss: ", "---- EPOCH 000 EVALUATION ----", "eval mean iou: "):
        assert line in log, line


def test_spn_evaluation_iou_equals_counts_by_hand(spn_run):
    from gspn_amd.predict import mean_iou
    run, tr = spn_run, spn_run.tr
    loss, means = tr.eval_one_epoch()                                      # the model after the second epoch
    assert 0.0 <= means["iou"] <= 1.0 and all(math.isfinite(v) for v in means.values())
    assert loss == means["recons_loss"]                                    # :403
    assert abs(means["loss"] - sum(means[k] for k in ("recons_loss", "kl_loss", "shift_loss", "spn_class_loss", "sem_loss"))) < 1e-12
    inter, union = torch.zeros(NCAT - 1, dtype=torch.int64), torch.zeros(NCAT - 1, dtype=torch.int64)
    tf_util.set_variable_store(tr.store)
    with torch.no_grad():
        for idx in ([0, 1],):                                              # the one validation batch
            tr._assemble(tr.val_data, idx)
            _, ep = tr._forward(tr._geometry(), tr._valid_index(tr.val_data, idx), False, None)
            pred, lab = ep["sem_class_logits"].argmax(-1).cpu(), ep["sem_labels"].cpu()
            for s in range(1, NCAT):
                inter[s - 1] += int(((pred == s) & (lab == s)).sum())
                union[s - 1] += int(((pred == s) | (lab == s)).sum())
    assert int(union.sum()) > 0
    assert means["iou"] == float(mean_iou(inter.cuda(), union.cuda()))
    assert all(torch.equal(v, run.saved[n]) for n, v in tr.store.vars.items())


@pytest.fixture(scope="module")
def eager_run():
    tr = trainer('SPN', False)
    seen = watch(tr)
    tr.train_one_epoch()
    return tr, seen


def test_eager_epoch_from_the_same_seed_gives_the_same_first_step(spn_run, eager_run):
    tr, seen = eager_run
    assert tr.step == 2 and not seen[0]["recaptured"]
    for k, v in seen[0]["terms"].items():
        print("first step %s: eager %.9g, captured %.9g" % (k, v, spn_run.seen[0]["terms"][k]))
    a, b = seen[0]["terms"]["loss"], spn_run.seen[0]["terms"]["loss"]
    assert abs(a - b) <= 1e-6 * abs(b)


def test_save_restore_then_one_step_is_bit_equal_to_stepping_on(tmp_path, monkeypatch):
    """Run with the library's fixed-order gradients: by default nn_distance's gradient below 4096 points adds in LDS with float atomics
    (tf_nndistance.LDS_GRAD_MAX_POINTS) and the narrow scatter-adds are float atomics too (invlists.DETERMINISTIC), so the last bits of
    everything upstream of the reconstruction loss differ between two runs of one and the same step, restored or not.  With the
    inverse-list forms of both, two runs of a step are bit-equal, and so must be a restored run and the one it was saved from."""
    from gspn_amd import invlists, tf_nndistance
    monkeypatch.setattr(invlists, "DETERMINISTIC", True)
    monkeypatch.setattr(tf_nndistance, "LDS_GRAD_MAX_POINTS", 0)
    tr = trainer('SPN', False)
    tr.train_step([0, 2])
    path = tr.save(str(tmp_path / "model.ckpt"))
    tr.train_step([1, 3])
    other = trainer('SPN', False)
    assert not torch.equal(other.opt.flat, tr.opt.flat)
    other.restore(path)
    assert other.step == 1 and other.opt.t == 1
    other.train_step([1, 3])
    assert other.step == tr.step == 2
    for n, v in tr.store.vars.items():
        assert torch.equal(other.store.vars[n], v), n
    assert torch.equal(other.opt.m, tr.opt.m) and torch.equal(other.opt.v, tr.opt.v)


def test_head_training_from_the_spn_checkpoint(spn_run):
    tr = trainer('RPOINTNET', True, cfg=heads_config())
    spn = [n for n in tr.store.vars if n.startswith("shape_proposal_net/")]
    heads = [n for n in tr.store.trainable if not n.startswith("shape_proposal_net/")]
    assert set(spn) == set(spn_run.saved) and len(heads) > 0 and tr.trained_names == heads
    step_before = tr.step
    tr.restore(spn_run.ckpt, scope='shape_proposal_net')
    assert tr.step == step_before == 0 and tr.opt.t == 0                   # the optimiser state and the step are left alone
    for n in spn:
        assert torch.equal(tr.store.vars[n], spn_run.saved[n]), n
    before = snapshot(tr)
    seen = watch(tr)
    logged = tr.train_one_epoch()
    assert tr.step == 2 and len(logged) == 2
    assert all(math.isfinite(v) for means in logged for v in means.values()) and set(logged[0]) == set(tr.terms) and len(tr.terms) == 9
    assert seen[0]["terms"]["loss"] == pytest.approx(sum(seen[0]["terms"][k] for k in ("rpointnet_class_loss", "rpointnet_bbox_loss",
                                                                                         "rpointnet_mask_loss")), rel=1e-6)
    for n in spn:                                                          # variables and moving statistics of the proposal net
        assert torch.equal(tr.store.vars[n], before[n]), n
    # the heads' variables move: every FPN layer and the classification head always (the class loss counts every ROI); the box and mask
    # branches get a gradient from positive ROIs only, so they are held to it when their loss is not zero
    moved = [n for n in heads if not torch.equal(tr.store.vars[n], before[n])]
    print("%d of %d head variables moved; unmoved: %s" % (len(moved), len(heads), [n for n in heads if n not in moved]))
    for scope in ("fpn1/", "fpn2/", "fpn3/", "fpn4/", "classification_head/"):
        assert any(n.startswith(scope) for n in moved), scope
    if any(info["terms"]["rpointnet_mask_loss"] > 0 for info in seen):
        assert any(n.startswith("segmentation_head/") for n in moved)
