"""The compute of the reference's train.py on the device: what a training run needs besides the networks, their losses (rpointnet.py,
training.py) and the data preparation (dataset.py).

  Schedules            :87-119       learning rate, batch-norm decay and KL weight, staircase exponentials of step * batch_size
  DeviceDataset        :221-240 over dataset.py:143-190: a scene cache on the device; batch() is ONE gspn_batch_assemble call
                       (csrc/train.hip) -- point permutation, padding, rotation about z + translation, bbox_ins -- that reads nothing
                       back, so it captures in a graph
  FlatAdamTF           :156          tf.train.AdamOptimizer's rule over a FlatGradBucket (parallel.FlatAdam is torch.optim.Adam's)
  FlatMomentum         :154          tf.train.MomentumOptimizer's
  ScalarSums                         running sums of device scalars (gspn_scalars_accumulate): a step ends without a host read
  save_variables, restore_variables  :160, :177-184  a checkpoint of a VariableStore, restored whole or under one variable scope
  Trainer              :201-219, :242-403  train_one_epoch, eval_one_epoch, fit, save, restore

Reading PLY / txt / npz files stays with the caller.  No CPU fallback for the kernel-backed parts."""
import ctypes
import os
from collections import OrderedDict
from datetime import datetime

import torch

from . import _lib as L
from . import tf_util
from .parallel import FlatAdam, FlatGradBucket, move_parameters_into_flat
from .roi import seed_tensor

__all__ = ["Schedules", "DeviceDataset", "FlatAdamTF", "FlatMomentum", "ScalarSums", "save_variables", "restore_variables", "Trainer",
           "batch_perm", "rand32", "PERM_STREAM", "AUGMENT_STREAM", "LOSS_TERMS"]

PERM_STREAM = 0xFFFFFFFD           # GSPN_PERM_STREAM of include/gspn_hip.h
AUGMENT_STREAM = 0xFFFFFFFC        # GSPN_AUGMENT_STREAM
SCALARS_MAX = 16                   # GSPN_SCALARS_MAX

# the nine terms train.py sums per step (:253-261), in its order; the last three exist with TRAIN_MODULE == ['RPOINTNET'] only
LOSS_TERMS = ('loss', 'recons_loss', 'kl_loss', 'shift_loss', 'sem_loss', 'spn_class_loss', 'rpointnet_class_loss', 'rpointnet_bbox_loss',
              'rpointnet_mask_loss')
_TERM_WORDING = {'loss': 'loss', 'recons_loss': 'reconstruction loss', 'kl_loss': 'kl-divergence loss', 'shift_loss': 'shift loss',
                 'sem_loss': 'sem loss', 'spn_class_loss': 'spn class loss', 'rpointnet_class_loss': 'rpointnet class loss',
                 'rpointnet_bbox_loss': 'rpointnet bbox loss', 'rpointnet_mask_loss': 'rpointnet mask loss'}


# ---- :87-119 -----------------------------------------------------------------------------------------------------------------------

class Schedules:
    """train.py:87-119.  Every schedule is base * decay_rate ** floor(step * batch_size / decay_step) (tf.train.exponential_decay,
    staircase=True), in plain Python float64.  TensorFlow evaluates the same expressions in float32: a value here differs from the
    reference's by at most one float32 ulp of a hyper-parameter, which is left as it is.  All three move only where
    step * batch_size crosses a multiple of decay_step, and `step` is the host's count of updates: nothing is read from the device."""

    BN_INIT_DECAY, BN_DECAY_DECAY_RATE, BN_DECAY_CLIP = 0.5, 0.5, 0.99          # :67-70
    LEARNING_RATE_FLOOR = 0.00001                                               # :108

    def __init__(self, batch_size, learning_rate=1e-3, decay_step=55000, decay_rate=0.7, kl_weight=1.0):
        self.batch_size, self.base_learning_rate, self.decay_step = int(batch_size), float(learning_rate), int(decay_step)
        self.decay_rate, self.kl_weight = float(decay_rate), float(kl_weight)
        if self.batch_size < 1 or self.decay_step < 1:
            raise ValueError("Schedules: batch_size and decay_step must be positive, got %d and %d" % (self.batch_size, self.decay_step))

    def stair(self, step):
        return (int(step) * self.batch_size) // self.decay_step

    def learning_rate(self, step):
        """:101-109"""
        return max(self.base_learning_rate * self.decay_rate ** self.stair(step), self.LEARNING_RATE_FLOOR)

    def bn_decay(self, step):
        """:111-119"""
        return min(self.BN_DECAY_CLIP, 1.0 - self.BN_INIT_DECAY * self.BN_DECAY_DECAY_RATE ** self.stair(step))

    def loss_weight(self, step):
        """:87-94, alpha of get_loss"""
        return 1.0 * self.kl_weight - 1.0 * self.kl_weight * self.decay_rate ** self.stair(step)


# ---- gspn_batch_perm in torch ---------------------------------------------------------------------------------------------------------

def _fmix32(x):
    m = 0xFFFFFFFF
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & m
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & m
    return x ^ (x >> 16)


def rand32(seed, slots, a, draws):
    """gspn_roi_rand32(seed, s, a, t) for s < slots, t < draws -> (slots, draws) int64 in [0, 2^32), on the seed's device"""
    from .dataset import _GOLD, _mix, _s64, _shr
    dev = seed.device
    st = _mix(seed.reshape(1) + _GOLD * torch.arange(1, slots + 1, dtype=torch.int64, device=dev))
    word = torch.arange(draws, dtype=torch.int64, device=dev) | _s64(int(a) << 32)
    return _shr(_mix(st.unsqueeze(1) ^ word), 32)


def batch_perm(seed, slots, n):
    """gspn_batch_perm of include/gspn_hip.h in int64 torch: (slots, n) int64 with row s the permutation of slot s, so that
    gspn_batch_assemble's out[s, i] = in[scene_idx[s], batch_perm(seed, slots, n)[s, i]].  seed: a one-element int64 tensor; everything
    stays on its device.  The restatement the tests hold the kernel to; the kernel never materialises it."""
    n = int(n)
    if n < 1 or n > (1 << 31):
        raise ValueError("batch_perm: n must be in [1, 2^31], got %d" % n)
    h = 1
    while (1 << (2 * h)) < n:
        h += 1
    mask = (1 << h) - 1
    keys = rand32(seed, slots, PERM_STREAM, 4)

    def encrypt(x):
        left, right = x >> h, x & mask
        for r in range(4):
            left, right = right, left ^ (_fmix32(right ^ keys[:, r:r + 1]) >> (32 - h))
        return (left << h) | right

    x = encrypt(torch.arange(n, dtype=torch.int64, device=seed.device).unsqueeze(0).expand(slots, n))
    while bool((x >= n).any()):
        x = torch.where(x >= n, encrypt(x), x)
    return x


# ---- :221-240 over dataset.py:143-190 --------------------------------------------------------------------------------------------------

_BATCH_KEYS = ("pc", "color", "pc_ins", "group_label", "group_indicator", "seg_label", "bbox_ins", "smpw", "rotation", "translation")


class DeviceDataset:
    """dataset.py's ScanNetDataset after its cache is built, held on the device.  pc, color (S, N, 3) float32; group_label, seg_label
    (S, N) int; pc_ins (S, G, M, 3) float32 with zero rows beyond a scene's groups; ngroup (S,) int, the groups of each scene with the
    background's (dataset.py's curngroup).  is_augment, permute_points as there (:80-81).
    .ngroup is the padded group count G, settable upwards as train.py:83-85 does (pc_ins gains zero rows).
    batch(scene_idx, seed) is get_batch (:221-240): one gspn_batch_assemble call."""

    def __init__(self, pc, color, group_label, seg_label, pc_ins, ngroup, is_augment=True, permute_points=True):
        self.pc = L.need(pc, torch.float32, 3, "pc")
        s, n, _ = self.pc.shape
        self.color = L.need(color, torch.float32, 3, "color")
        self.pc_ins = L.need(pc_ins, torch.float32, 4, "pc_ins")
        if self.pc.shape[2] != 3 or tuple(self.color.shape) != (s, n, 3) or self.pc_ins.shape[0] != s or self.pc_ins.shape[3] != 3:
            raise ValueError("DeviceDataset: pc, color must be (S, N, 3) and pc_ins (S, G, M, 3), got %s, %s and %s"
                             % (tuple(pc.shape), tuple(color.shape), tuple(pc_ins.shape)))
        for name, t in (("group_label", group_label), ("seg_label", seg_label)):
            if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.int64) or tuple(t.shape) != (s, n):
                raise ValueError("DeviceDataset: %s must be an int tensor %s" % (name, (s, n)))
        self.group_label = L.need(group_label.int(), torch.int32, 2, "group_label")
        self.seg_label = L.need(seg_label.int(), torch.int32, 2, "seg_label")
        if not isinstance(ngroup, torch.Tensor) or ngroup.dtype not in (torch.int32, torch.int64) or tuple(ngroup.shape) != (s,):
            raise ValueError("DeviceDataset: ngroup must be an int tensor (S,) = (%d,)" % s)
        self.counts_host = [int(v) for v in ngroup.tolist()]               # read once, here: the driver's valid-instance index needs no read-back
        if min(self.counts_host) < 0 or max(self.counts_host) > self.pc_ins.shape[1]:
            raise ValueError("DeviceDataset: ngroup must lie in [0, G = %d], found [%d, %d]"
                             % (self.pc_ins.shape[1], min(self.counts_host), max(self.counts_host)))
        self.counts = ngroup.to(self.pc.device).int().contiguous()
        self.is_augment, self.permute_points = bool(is_augment), bool(permute_points)

    def __len__(self):
        return self.pc.shape[0]

    @property
    def ngroup(self):
        return self.pc_ins.shape[1]

    @ngroup.setter
    def ngroup(self, value):
        g, have = int(value), self.pc_ins.shape[1]
        if g < max(self.counts_host):
            raise ValueError("DeviceDataset.ngroup: %d is below the %d groups of a scene" % (g, max(self.counts_host)))
        if g > have:
            s, _, m, _ = self.pc_ins.shape
            self.pc_ins = torch.cat((self.pc_ins, torch.zeros((s, g - have, m, 3), dtype=torch.float32, device=self.pc_ins.device)), 1)
        elif g < have:
            self.pc_ins = self.pc_ins[:, :g].contiguous()                   # rows beyond every scene's groups: zeros by the contract

    def empty_batch(self, b):
        """the ten output tensors of batch() for b slots, uninitialised: persistent buffers for a captured step"""
        (_, n, _), (_, g, m, _), dev = self.pc.shape, self.pc_ins.shape, self.pc.device
        f, i, d = torch.float32, torch.int32, torch.float64
        shapes = {"pc": ((b, n, 3), f), "color": ((b, n, 3), f), "pc_ins": ((b, g, m, 3), f), "group_label": ((b, n), i),
                  "group_indicator": ((b, g), i), "seg_label": ((b, n), i), "bbox_ins": ((b, g, 6), f), "smpw": ((b, n), f),
                  "rotation": ((b, 3, 3), d), "translation": ((b, 3), d)}
        return {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in _BATCH_KEYS}

    def batch(self, scene_idx, seed=0, out=None):
        """scene_idx: (B,) int32 device tensor (or a sequence of ints, copied to the device); seed: an int or a one-element int64 device
        tensor, read on the device.  -> dict of pc, color (B, N, 3), pc_ins (B, G, M, 3), group_label (B, N) int32, group_indicator (B, G)
        int32, seg_label (B, N) int32, bbox_ins (B, G, 6), smpw (B, N) ones -- get_batch's eight -- plus rotation (B, 3, 3) and
        translation (B, 3) float64 as drawn (identity and zero without augmentation).  out: the dict of an earlier call or of
        empty_batch(), written in place.  Semantics: include/gspn_hip.h, gspn_batch_assemble."""
        dev = self.pc.device
        if not isinstance(scene_idx, torch.Tensor):
            scene_idx = torch.tensor([int(v) for v in scene_idx], dtype=torch.int32)
        if scene_idx.dtype != torch.int32 or scene_idx.dim() != 1 or scene_idx.numel() < 1:
            raise ValueError("DeviceDataset.batch: scene_idx must be a non-empty (B,) int32 tensor, got %s %s" % (scene_idx.dtype, tuple(scene_idx.shape)))
        scene_idx = scene_idx.to(dev).contiguous()
        b = scene_idx.shape[0]
        seed = seed_tensor(seed, dev)
        if out is None:
            out = self.empty_batch(b)
        else:
            want = self.empty_batch(0)
            for k in _BATCH_KEYS:
                t = out[k]
                if t.dtype != want[k].dtype or tuple(t.shape) != (b,) + tuple(want[k].shape[1:]) or t.device != dev or not t.is_contiguous():
                    raise ValueError("DeviceDataset.batch: out[%r] must be a contiguous %s tensor %s on %s"
                                     % (k, want[k].dtype, (b,) + tuple(want[k].shape[1:]), dev))
        (s, n, _), (_, g, m, _) = self.pc.shape, self.pc_ins.shape
        with torch.cuda.device(dev):
            L.check(L.lib().gspn_batch_assemble(
                s, b, n, g, m, L.ptr(self.pc), L.ptr(self.color), L.ptr(self.group_label), L.ptr(self.seg_label), L.ptr(self.pc_ins),
                L.ptr(self.counts), L.ptr(scene_idx), L.ptr(seed), int(self.permute_points), int(self.is_augment), L.ptr(out["pc"]),
                L.ptr(out["color"]), L.ptr(out["group_label"]), L.ptr(out["seg_label"]), L.ptr(out["pc_ins"]), L.ptr(out["group_indicator"]),
                L.ptr(out["bbox_ins"]), L.ptr(out["smpw"]), L.ptr(out["rotation"]), L.ptr(out["translation"]), L.stream()), "batch_assemble")
        return out


# ---- :153-157 ----------------------------------------------------------------------------------------------------------------------

class _FlatOptimizer:
    """what the flat optimisers share: the parameters moved into one flat buffer (parallel.move_parameters_into_flat), zero_grad, and a
    state that a checkpoint can hold.  `lr` is an attribute: the driver sets the schedule's value before each step."""
    STATE = ()

    def __init__(self, bucket, lr):
        self.bucket, self.lr = bucket, float(lr)
        self.flat = move_parameters_into_flat(bucket)
        self.t = 0

    def zero_grad(self, set_to_none=True):
        self.bucket.discard()
        for p in self.bucket.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def state_dict(self):
        return dict({k: getattr(self, k).detach().cpu().clone() for k in self.STATE}, t=int(self.t))

    def load_state_dict(self, state):
        for k in self.STATE:
            if tuple(state[k].shape) != tuple(getattr(self, k).shape):
                raise ValueError("optimiser state %s has shape %s, this model needs %s" % (k, tuple(state[k].shape), tuple(getattr(self, k).shape)))
            getattr(self, k).copy_(state[k])
        self.t = int(state["t"])


class FlatAdamTF(_FlatOptimizer):
    """tf.train.AdamOptimizer (train.py:156) over the bucket's parameters as one buffer, one gspn_adam_tf_flat launch per step:
    lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t);  p -= lr_t * m / (sqrt(v) + eps).  parallel.FlatAdam applies torch.optim.Adam's rule, with
    eps added to the bias-corrected root; the two part where sqrt(v) is not large against eps, i.e. in the early steps."""
    STATE = ("m", "v")

    def __init__(self, bucket, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(bucket, lr)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.m, self.v = torch.zeros_like(self.flat), torch.zeros_like(self.flat)

    def step(self, grad_scale=1.0):
        self.t += 1
        with torch.cuda.device(self.flat.device):
            L.check(L.lib().gspn_adam_tf_flat(self.flat.numel(), L.ptr(self.flat), L.ptr(self.bucket.flat), L.ptr(self.m), L.ptr(self.v), self.lr,
                                              self.betas[0], self.betas[1], self.eps, float(grad_scale), self.t, L.stream()), "adam_tf_flat")


class FlatMomentum(_FlatOptimizer):
    """tf.train.MomentumOptimizer (train.py:154) -- and torch.optim.SGD(momentum=, dampening=0) -- as one gspn_momentum_flat launch:
    accum = momentum * accum + g;  p -= lr * accum"""
    STATE = ("accum",)

    def __init__(self, bucket, lr=1e-3, momentum=0.9):
        super().__init__(bucket, lr)
        self.momentum = float(momentum)
        self.accum = torch.zeros_like(self.flat)

    def step(self, grad_scale=1.0):
        self.t += 1
        with torch.cuda.device(self.flat.device):
            L.check(L.lib().gspn_momentum_flat(self.flat.numel(), L.ptr(self.flat), L.ptr(self.bucket.flat), L.ptr(self.accum), self.lr,
                                               self.momentum, float(grad_scale), L.stream()), "momentum_flat")


class _TorchRuleAdam(FlatAdam):
    """parallel.FlatAdam with the state interface of the optimisers above (adam_rule='torch')"""

    def state_dict(self):
        return {"m": self.m.detach().cpu().clone(), "v": self.v.detach().cpu().clone(), "t": int(self.t)}

    def load_state_dict(self, state):
        self.m.copy_(state["m"])
        self.v.copy_(state["v"])
        self.t = int(state["t"])


# ---- the running sums of :253-261, :288-297 -----------------------------------------------------------------------------------------

class ScalarSums:
    """sums (k,) float64 and count (1,) int64 on the device.  add(tensors) is one gspn_scalars_accumulate launch: sums[i] += tensors[i],
    count += 1, no host read; read() is the one read of a logging interval (train.py:299) and zeroes both."""

    def __init__(self, k, device):
        if not 1 <= int(k) <= SCALARS_MAX:
            raise ValueError("ScalarSums: 1 <= k <= %d, got %d" % (SCALARS_MAX, k))
        self.k = int(k)
        self.sums = torch.zeros(self.k, dtype=torch.float64, device=device)
        self.count = torch.zeros(1, dtype=torch.int64, device=device)

    def add(self, tensors):
        if len(tensors) != self.k:
            raise ValueError("ScalarSums.add: %d scalars expected, got %d" % (self.k, len(tensors)))
        for t in tensors:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != 1 or t.device != self.sums.device:
                raise ValueError("ScalarSums.add: every scalar must be a one-element float32 tensor on %s" % self.sums.device)
        ptrs = (ctypes.c_void_p * self.k)(*[t.data_ptr() for t in tensors])
        with torch.cuda.device(self.sums.device):
            L.check(L.lib().gspn_scalars_accumulate(self.k, ptrs, L.ptr(self.sums), L.ptr(self.count), L.stream()), "scalars_accumulate")

    def read(self):
        """-> (sums as a list of floats, count); one host read, then both are zeroed"""
        sums, count = self.sums.tolist(), int(self.count.item())
        self.sums.zero_()
        self.count.zero_()
        return sums, count


# ---- :160, :177-184 -----------------------------------------------------------------------------------------------------------------

def _in_scope(name, scope):
    return scope is None or name == scope or name.startswith(scope.rstrip("/") + "/")


def save_variables(path, store, **extra):
    """tf.train.Saver().save (:160, :213, :218): ONE torch.save of {'variables': {full name: CPU tensor}} over every variable of the
    store, the moving statistics included, plus the keyword arguments (the driver adds 'optimizer' and 'step')."""
    ckpt = dict(extra)
    ckpt["variables"] = OrderedDict((n, v.detach().cpu().clone()) for n, v in store.vars.items())
    torch.save(ckpt, path)
    return path


def restore_variables(path, store, scope=None):
    """:177-184.  Loads the checkpoint at `path` into the variables of `store` IN PLACE (their storage -- a flat optimiser's views, the
    addresses a captured step holds -- stays).  scope=None restores every variable of the store; a scope restores only the names under
    it (tf.get_collection(GLOBAL_VARIABLES, scope=...)) and leaves the others alone.  A variable to restore that the checkpoint does
    not hold raises KeyError, one it holds with another shape ValueError; both name the variable, and nothing is written before every
    variable has been checked.  Names of the checkpoint that the store does not have are ignored, as a Saver over a var_list does.
    -> the checkpoint dict."""
    ckpt = torch.load(path, map_location="cpu")
    saved = ckpt["variables"]
    names = [n for n in store.vars if _in_scope(n, scope)]
    if not names:
        raise KeyError("restore_variables: the store has no variable under scope %r" % (scope,))
    for n in names:
        if n not in saved:
            raise KeyError("restore_variables: variable %s is not in the checkpoint %s" % (n, path))
        if tuple(saved[n].shape) != tuple(store.vars[n].shape):
            raise ValueError("restore_variables: variable %s has shape %s in the checkpoint %s, %s in the model"
                             % (n, tuple(saved[n].shape), path, tuple(store.vars[n].shape)))
    with torch.no_grad():
        for n in names:
            store.vars[n].copy_(saved[n])
    return ckpt


# ---- :201-219, :242-403 ------------------------------------------------------------------------------------------------------------

class _Capture:
    """one captured forward + loss + backward: the graph, the valid-instance index it reads and the loss terms it leaves"""
    __slots__ = ("graph", "valid", "terms", "bn_decay")


class Trainer:
    """train.py's loop.  config: an rpointnet.Config whose BATCH_SIZE, NUM_SAMPLE, NUM_CATEGORY, ... are the run's; NUM_POINT,
    NUM_POINT_INS and NUM_GROUP are set here from the data, NUM_GROUP to the larger ngroup of the two datasets (:83-85), and
    TRAIN_MODULE to [train_module].  train_data, val_data: DeviceDataset.  optimizer 'adam' | 'momentum' (:153-157); adam_rule 'tf'
    (FlatAdamTF, the reference's) or 'torch' (parallel.FlatAdam).  schedules: a Schedules (default: Schedules(BATCH_SIZE)).
    log_dir: log_train.txt and the checkpoints of fit() go there (None: no file is written).  seed: seeds the variables' initial
    values, the epoch shuffles, the device seed of the batches and torch's generators (torch.manual_seed: dropout draws from them).

    captured=True: forward + loss + backward replay from a graph.CapturedStep.  The batch, the geometry, the valid-instance index and
    the noise are prepared outside it into buffers it reads; alpha is a 0-d device tensor filled before each replay; bn_decay is a
    float baked into the launches, so the step is captured again when bn_decay(step) changes -- the host knows the step, nothing is
    read back -- and once per number of valid instances of a batch (the instance encoder's shapes depend on it; at most max_captures
    graphs are kept).  The moving statistics and torch's generator state are put back after a capture's warm-up runs, which therefore
    leave no trace: a captured run and an eager one compute the same steps.
    on_step: None or a callable given a dict per training step -- step, learning_rate, bn_decay, alpha (the values IN FORCE: bn_decay is
    the one the executed graph was captured with), recaptured, terms (name -> 0-d device tensor).
    For 'RPOINTNET' the step is training.py's head training: the proposal net frozen in evaluation mode, its variables outside the
    optimiser."""

    def __init__(self, config, train_data, val_data, train_module='SPN', optimizer='adam', momentum=0.9, schedules=None, log_dir=None,
                 seed=0, captured=True, adam_rule='tf', log_every=10, max_captures=8, model_name='model_rpointnet'):
        if train_module not in ('SPN', 'RPOINTNET'):
            raise ValueError("Trainer: train_module must be 'SPN' or 'RPOINTNET', got %r" % (train_module,))
        if optimizer not in ('adam', 'momentum') or adam_rule not in ('tf', 'torch'):
            raise ValueError("Trainer: optimizer must be 'adam' or 'momentum' and adam_rule 'tf' or 'torch', got %r and %r" % (optimizer, adam_rule))
        for d in (train_data, val_data):
            if tuple(d.pc.shape[1:]) != tuple(train_data.pc.shape[1:]) or d.pc_ins.shape[2] != train_data.pc_ins.shape[2]:
                raise ValueError("Trainer: train_data and val_data must agree on the points per scene and per instance")
        self.cfg, self.train_data, self.val_data, self.module = config, train_data, val_data, train_module
        g = max(train_data.ngroup, val_data.ngroup)                                        # :83-85
        train_data.ngroup = val_data.ngroup = g
        config.NUM_GROUP, config.NUM_POINT, config.NUM_POINT_INS = g, train_data.pc.shape[1], train_data.pc_ins.shape[2]
        config.TRAIN_MODULE = [train_module]
        self.b = int(config.BATCH_SIZE)
        if len(train_data) < self.b:
            raise ValueError("Trainer: %d training scenes do not fill a batch of %d" % (len(train_data), self.b))
        self.schedules = schedules if schedules is not None else Schedules(self.b)
        self.captured, self.log_every, self.max_captures, self.model_name = bool(captured), int(log_every), int(max_captures), model_name
        self.log_dir, self._log_file = log_dir, None
        if log_dir is not None:
            os.makedirs(log_dir, exist_ok=True)
            self._log_file = open(os.path.join(log_dir, 'log_train.txt'), 'w')
        self.dev = train_data.pc.device
        self.on_step = None
        self.step, self.epoch_cnt = 0, 0

        torch.manual_seed(int(seed))
        self._shuffle = torch.Generator().manual_seed(int(seed))
        self._noise_gen = torch.Generator(device=self.dev).manual_seed(int(seed))
        self.seed_dev = seed_tensor(int(seed), self.dev).clone()
        self.store = tf_util.set_variable_store(tf_util.VariableStore(device=self.dev, seed=int(seed)))

        # persistent inputs of the step
        self.buf = train_data.empty_batch(self.b)
        self.scene_idx = torch.zeros(self.b, dtype=torch.int32, device=self.dev)
        self.noise = torch.zeros((self.b, int(config.NUM_SAMPLE), 256), dtype=torch.float32, device=self.dev)
        self.alpha = torch.zeros((), dtype=torch.float32, device=self.dev)
        self.geo = None
        self._captures = OrderedDict()
        self.terms = LOSS_TERMS[:6] if train_module == 'SPN' else LOSS_TERMS
        self.sums = ScalarSums(len(self.terms), self.dev)

        # the variables come from one evaluation-mode forward pass (no statistic moves, no generator is consumed), in the reference's order
        idx = list(range(self.b))
        self._assemble(train_data, idx)
        with torch.no_grad():
            self._forward(self._geometry(), self._valid_index(train_data, idx), False, None)
        names = [n for n in self.store.trainable if train_module == 'SPN' or not n.startswith('shape_proposal_net/')]
        self.trained_names = names
        self.bucket = FlatGradBucket([self.store.vars[n] for n in names])
        lr = self.schedules.learning_rate(0)
        if optimizer == 'momentum':
            self.opt = FlatMomentum(self.bucket, lr, momentum)
        elif adam_rule == 'tf':
            self.opt = FlatAdamTF(self.bucket, lr)
        else:
            self.opt = _TorchRuleAdam(self.bucket, lr)
        self.moving = [v for n, v in self.store.vars.items() if n not in set(self.store.trainable)]

    # ---- logging ----
    def log_string(self, out_str):
        """:96-99"""
        if self._log_file is not None:
            self._log_file.write(out_str + '\n')
            self._log_file.flush()
        print(out_str, flush=True)

    def close(self):
        if self._log_file is not None:
            self._log_file.close()
            self._log_file = None

    # ---- the parts of a step ----
    def _assemble(self, data, idx):
        """get_batch (:221-240) into the persistent buffers; the device seed moves on by one, on the device"""
        self.scene_idx.copy_(torch.tensor(idx, dtype=torch.int32))
        self.seed_dev.add_(1)
        data.batch(self.scene_idx, self.seed_dev, out=self.buf)

    def _valid_index(self, data, idx):
        """shape_proposal.valid_instances(group_indicator) from the host's copy of the group counts: no read-back"""
        rows = [(s, j) for s, k in enumerate(idx) for j in range(min(data.counts_host[k], data.ngroup))]
        return torch.tensor(rows, dtype=torch.int64).reshape(-1, 2).to(self.dev)

    def _geometry(self):
        from .shape_proposal import SPN_SEM_POINTS
        from .spn_trunks import spn_geometry
        return spn_geometry(self.buf["pc"], int(self.cfg.NUM_SAMPLE), SPN_SEM_POINTS, self.module == 'RPOINTNET', points=self.buf["color"])

    def _forward(self, geo, valid, is_training, bn_decay):
        """rpointnet + get_loss (:135-136) on the buffers -> (loss, end_points)"""
        from . import rpointnet as RP
        u, cfg = self.buf, self.cfg
        args = (u["pc"], u["color"], u["pc_ins"], u["group_label"], u["group_indicator"], u["seg_label"], u["bbox_ins"], cfg, is_training)
        if self.module == 'SPN':
            ep = RP.rpointnet(*args, mode='training', bn_decay=bn_decay, geometry=geo, noise=self.noise, valid_idx=valid)
            return RP.get_loss(ep, cfg, self.alpha, u["smpw"])
        ep = RP.rpointnet_head_training(*args, bn_decay, geometry=geo, valid_idx=valid, noise=self.noise, seed=self.seed_dev)
        return RP.get_head_training_loss(ep, cfg, self.alpha, u["smpw"])

    def _forward_backward(self, geo, valid, bn_decay, keep):
        for p in self.store.parameters():
            p.grad = None
        loss, ep = self._forward(geo, valid, True, bn_decay)
        loss.backward()
        self.bucket.flatten()
        keep.terms = [ep[k].detach().reshape(()) for k in self.terms]
        return loss.detach()

    def _capture(self, nvalid, valid, bn_decay):
        from .graph import CapturedStep
        cap = _Capture()
        cap.valid, cap.bn_decay = valid.clone(), bn_decay
        moving = [v.clone() for v in self.moving]
        cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(self.dev)
        cap.graph = CapturedStep(lambda: self._forward_backward(self.geo, cap.valid, bn_decay, cap))
        torch.set_rng_state(cpu_state)
        torch.cuda.set_rng_state(dev_state, self.dev)
        with torch.no_grad():
            for v, w in zip(self.moving, moving):
                v.copy_(w)
        self._captures[nvalid] = cap
        while len(self._captures) > self.max_captures:
            self._captures.popitem(last=False)
        return cap

    def train_step(self, idx):
        """one step of :262-297 on the scenes idx of train_data"""
        from .graph import copy_into
        tf_util.set_variable_store(self.store)
        sch, step = self.schedules, self.step
        lr, bn_decay, alpha = sch.learning_rate(step), sch.bn_decay(step), sch.loss_weight(step)
        self._assemble(self.train_data, idx)
        self.noise.copy_(torch.randn(self.noise.shape, generator=self._noise_gen, device=self.dev))
        self.alpha.fill_(alpha)
        geo, valid = self._geometry(), self._valid_index(self.train_data, idx)
        recaptured = False
        if self.captured:
            self.geo = geo if self.geo is None else copy_into(self.geo, geo)
            if self._captures and next(iter(self._captures.values())).bn_decay != bn_decay:
                self._captures.clear()                                # the staircase moved: every graph has the old decay baked in
            cap = self._captures.get(valid.shape[0])
            if cap is None:
                cap, recaptured = self._capture(valid.shape[0], valid, bn_decay), True
            else:
                self._captures.move_to_end(valid.shape[0])
                cap.valid.copy_(valid)
            cap.graph.replay()
        else:
            cap = _Capture()
            cap.bn_decay = bn_decay
            self._forward_backward(geo, valid, bn_decay, cap)
        self.opt.lr = lr
        self.opt.step()
        self.sums.add(cap.terms)
        self.step += 1
        if self.on_step is not None:
            self.on_step({"step": step, "learning_rate": self.opt.lr, "bn_decay": cap.bn_decay, "alpha": alpha, "recaptured": recaptured,
                          "terms": dict(zip(self.terms, cap.terms))})

    def train_one_epoch(self):
        """:242-321 -> the means it logged, one dict per logging interval"""
        tf_util.set_variable_store(self.store)
        order = torch.randperm(len(self.train_data), generator=self._shuffle).tolist()
        num_batches = len(self.train_data) // self.b
        self.log_string(str(datetime.now()))
        self.sums.read()
        logged = []
        for batch_idx in range(num_batches):
            self.train_step(order[batch_idx * self.b:(batch_idx + 1) * self.b])
            if (batch_idx + 1) % self.log_every == 0:
                sums, _ = self.sums.read()                            # the one host read of the interval (:299)
                means = {k: v / self.log_every for k, v in zip(self.terms, sums)}
                self.log_string(' -- %03d / %03d --' % (batch_idx + 1, num_batches))
                self.log_string(' -- Model: ' + self.model_name)
                self.log_string(' -- LOG DIR: ' + str(self.log_dir))
                for k in self.terms:
                    self.log_string('mean %s: %f' % (_TERM_WORDING[k], means[k]))
                logged.append(means)
        return logged

    def eval_one_epoch(self):
        """:324-403: evaluation mode, no permutation, no augmentation (val_data's flags), the 18-class IoU through
        predict.semantic_iou_counts / mean_iou on sem_class_logits and sem_labels -> (the model-selection loss of :400-403, the means it
        logged: the loss terms, 'loss' as :372-374 sums it, and 'iou')"""
        from .predict import mean_iou, semantic_iou_counts
        tf_util.set_variable_store(self.store)
        num_batches = len(self.val_data) // self.b
        self.log_string(str(datetime.now()))
        self.log_string('---- EPOCH %03d EVALUATION ----' % self.epoch_cnt)
        terms = self.terms[1:]
        sums = ScalarSums(len(terms), self.dev)
        inter = union = None
        self.alpha.fill_(self.schedules.loss_weight(self.step))
        with torch.no_grad():
            for batch_idx in range(num_batches):
                idx = list(range(batch_idx * self.b, (batch_idx + 1) * self.b))
                self._assemble(self.val_data, idx)
                _, ep = self._forward(self._geometry(), self._valid_index(self.val_data, idx), False, None)
                inter, union = semantic_iou_counts(ep['sem_class_logits'].contiguous(), ep['sem_labels'].int().contiguous(), inter, union)
                sums.add([ep[k].detach().reshape(()) for k in terms])
        total, _ = sums.read()
        means = {k: v / float(num_batches) for k, v in zip(terms, total)}
        head = ('rpointnet_class_loss', 'rpointnet_bbox_loss', 'rpointnet_mask_loss')
        spn = ('recons_loss', 'kl_loss', 'shift_loss', 'spn_class_loss', 'sem_loss')
        means['loss'] = sum(means[k] for k in (head if self.module == 'RPOINTNET' else spn))                    # :371-374
        means['iou'] = float(mean_iou(inter, union))
        self.log_string('eval mean loss: %f' % means['loss'])
        for k in ('recons_loss', 'kl_loss', 'shift_loss', 'sem_loss'):
            self.log_string('eval mean %s: %f' % (_TERM_WORDING[k], means[k]))
        self.log_string('eval mean iou: %f' % means['iou'])
        for k in ('spn_class_loss',) + (head if self.module == 'RPOINTNET' else ()):
            self.log_string('eval mean %s: %f' % (_TERM_WORDING[k], means[k]))
        self.epoch_cnt += 1
        epoch_loss = sum(means[k] for k in head) if self.module == 'RPOINTNET' else means['recons_loss']       # :400-403
        return epoch_loss, means

    def fit(self, max_epoch):
        """:201-219: keeps the best model by eval_one_epoch's loss and writes model.ckpt every 10 epochs (into log_dir)"""
        best_loss, history = 1e20, []
        for epoch in range(int(max_epoch)):
            self.log_string('************ EPOCH %03d ***********' % epoch)
            self.log_string('Training Model: ' + self.model_name)
            self.log_string('Saving in: ' + str(self.log_dir))
            self.train_one_epoch()
            epoch_loss, means = self.eval_one_epoch()
            history.append(means)
            if epoch_loss < best_loss:
                best_loss = epoch_loss
                if self.log_dir is not None:
                    self.log_string("Model saved in file: %s" % self.save(os.path.join(self.log_dir, "best_model_epoch_%03d.ckpt" % epoch)))
            if epoch % 10 == 0 and self.log_dir is not None:
                self.log_string("Model saved in file: %s" % self.save(os.path.join(self.log_dir, "model.ckpt")))
        return history

    def save(self, path):
        """every variable of the store by full name, the moving statistics included, the optimiser's state and the step count -- and
        the generators' states (the device seed, the noise and shuffle generators, torch's), so that a restored run draws on as the saved
        one would have"""
        rng = {"seed_dev": self.seed_dev.cpu().clone(), "noise": self._noise_gen.get_state(), "shuffle": self._shuffle.get_state(),
               "torch_cpu": torch.get_rng_state(), "torch_cuda": torch.cuda.get_rng_state(self.dev)}
        return save_variables(path, self.store, optimizer=self.opt.state_dict(), optimizer_class=type(self.opt).__name__, step=int(self.step),
                              epoch=int(self.epoch_cnt), rng=rng)

    def restore(self, path, scope=None):
        """:177-184.  scope=None: every variable, the optimiser's state, the step count and the generators' states; a scope (--restore_scope
        shape_proposal_net, the way from SPN training to head training): only the variables under it, the optimiser state and the
        step stay as they are.  Variables are written in place, so captured graphs stay valid."""
        ckpt = restore_variables(path, self.store, scope)
        if scope is None:
            if ckpt.get("optimizer_class") != type(self.opt).__name__:
                raise ValueError("restore: the checkpoint %s holds the state of %s, this run uses %s (pass a scope to restore variables only)"
                                 % (path, ckpt.get("optimizer_class"), type(self.opt).__name__))
            self.opt.load_state_dict(ckpt["optimizer"])
            self.step, self.epoch_cnt, rng = int(ckpt["step"]), int(ckpt.get("epoch", 0)), ckpt["rng"]
            self.seed_dev.copy_(rng["seed_dev"])
            self._noise_gen.set_state(rng["noise"])
            self._shuffle.set_state(rng["shuffle"])
            torch.set_rng_state(rng["torch_cpu"])
            torch.cuda.set_rng_state(rng["torch_cuda"], self.dev)
        print('RESTORE MODEL FROM ' + str(path), flush=True)
        return ckpt
