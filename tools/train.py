"""The reference's train.py on this library: its flags (train.py:18-38), gspn_amd.train.Trainer underneath.

The reference reads ScanNet meshes and labels and builds an .npz cache (dataset.py:28-125); here the cache is a file of its own, made
from a ScanNet download by tools/data_prep.py and then tools/make_cache.py:
  --cache FILE       a torch.save'd dict of the six cache tensors of gspn_amd.train.DeviceDataset -- pc, color (S, N, 3) float32,
                     group_label, seg_label (S, N) int, pc_ins (S, G, M, 3) float32, ngroup (S,) int -- as tools/make_cache.py writes it
                     (gspn_amd.data_prep.build_cache over gspn_amd.dataset; INTEGRATION.md, sections N, O and Q); --val_cache FILE likewise
                     (default: the last tenth of --cache, at least one batch)
  --synthetic S      S scenes from gspn_amd.synth.spn_batch instead, the last tenth (at least one batch) held out for evaluation

    python tools/train.py --synthetic 8 --num_point 4096 --num_sample 64 --num_category 9 --max_epoch 2 --log_dir /tmp/log
    python tools/data_prep.py ./data/scannet ./data/scannet_preprocessed
    python tools/make_cache.py --mesh_path ./data/scannet_preprocessed/mesh/scans --label_path ./data/scannet_preprocessed/label/scans \\
        --list train.txt --out train.pt
    python tools/train.py --cache train.pt --val_cache val.pt --log_dir log_spn
    python tools/train.py --cache train.pt --val_cache val.pt --train_module RPOINTNET --restore_model_path log_spn/model.ckpt \\
        --restore_scope shape_proposal_net --log_dir log_heads
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gspn_amd import synth  # noqa: E402
from gspn_amd.rpointnet import Config  # noqa: E402
from gspn_amd.train import DeviceDataset, Schedules, Trainer  # noqa: E402

CACHE_KEYS = ("pc", "color", "group_label", "seg_label", "pc_ins", "ngroup")


def parse(argv=None):
    cfg = Config()
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--gpu', type=int, default=0, help='GPU to use [default: GPU 0]')
    ap.add_argument('--model', default='model_rpointnet', help='Model name [default: model_rpointnet]')
    ap.add_argument('--log_dir', default='log', help='Log dir [default: log]')
    ap.add_argument('--train_module', default='SPN', help='The module to be trained [options: SPN or RPOINTNET]')
    ap.add_argument('--num_point', type=int, default=cfg.NUM_POINT, help='Point Number in a Scene [default: 18000]')
    ap.add_argument('--num_point_ins', type=int, default=cfg.NUM_POINT_INS, help='Point Number of an Instance [default: 512]')
    ap.add_argument('--num_category', type=int, default=cfg.NUM_CATEGORY, help='Maximum Number of Categories [default: 19]')
    ap.add_argument('--num_sample', type=int, default=cfg.NUM_SAMPLE, help='Number of Sampled Seed Points [default: 256]')
    ap.add_argument('--max_epoch', type=int, default=800, help='Epoch to run [default: 800]')
    ap.add_argument('--batch_size', type=int, default=cfg.BATCH_SIZE, help='Batch Size during training [default: 2]')
    ap.add_argument('--learning_rate', type=float, default=0.001, help='Initial learning rate [default: 0.001]')
    ap.add_argument('--momentum', type=float, default=0.9, help='Initial learning rate [default: 0.9]')
    ap.add_argument('--optimizer', default='adam', help='adam or momentum [default: adam]')
    ap.add_argument('--decay_step', type=int, default=55000, help='Decay step for lr decay [default: 55000]')
    ap.add_argument('--decay_rate', type=float, default=0.7, help='Decay rate for lr decay [default: 0.7]')
    ap.add_argument('--restore_model_path', default=None, help='Restore model path e.g. log/model.ckpt')
    ap.add_argument('--restore_scope', default=None, help='Restore variable scope')
    ap.add_argument('--KL_weight', type=float, default=1, help='Additional weight for KL Loss')
    ap.add_argument('--is_augment', type=int, default=1, help='Whether to augment the training data')
    # not in the reference
    ap.add_argument('--cache', default=None, help='torch.save file of the six training cache tensors')
    ap.add_argument('--val_cache', default=None, help='the same for evaluation [default: the last tenth of --cache]')
    ap.add_argument('--synthetic', type=int, default=0, help='number of synthetic scenes to train on instead of --cache')
    ap.add_argument('--num_group', type=int, default=12, help='groups per synthetic scene [default: 12]')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--eager', action='store_true', help='do not capture the step in a graph')
    ap.add_argument('--adam_rule', default='tf', help="'tf' (the reference's tf.train.AdamOptimizer) or 'torch'")
    return ap.parse_args(argv)


def load_cache(path):
    d = torch.load(path, map_location="cpu")
    missing = [k for k in CACHE_KEYS if k not in d]
    if missing:
        raise KeyError("%s: the cache lacks %s (it must hold %s)" % (path, missing, list(CACHE_KEYS)))
    return {k: d[k] for k in CACHE_KEYS}


def synthetic_cache(a):
    d = synth.spn_batch("S", a.synthetic, a.num_point, a.num_group, a.num_point_ins, a.num_category, a.seed)
    out = {k: torch.from_numpy(d[k]) for k in ("pc", "color", "group_label", "seg_label", "pc_ins")}
    out["ngroup"] = torch.full((a.synthetic,), a.num_group, dtype=torch.int32)
    return out


def split(cache, lo, hi, dev, **flags):
    return DeviceDataset(*[cache[k][lo:hi].to(dev) for k in CACHE_KEYS], **flags)


def main(argv=None):
    a = parse(argv)
    if (a.cache is None) == (a.synthetic <= 0):
        raise SystemExit("give exactly one of --cache FILE and --synthetic S")
    dev = torch.device("cuda", a.gpu)
    torch.cuda.set_device(dev)
    cache = load_cache(a.cache) if a.cache else synthetic_cache(a)
    total = cache["pc"].shape[0]
    if a.val_cache:
        val_cache, ntrain, nval = load_cache(a.val_cache), total, None
    else:
        held = max(a.batch_size, total // 10)
        if total - held < a.batch_size:
            raise SystemExit("%d scenes are too few for a training and an evaluation batch of %d" % (total, a.batch_size))
        val_cache, ntrain, nval = cache, total - held, total
    train = split(cache, 0, ntrain, dev, is_augment=bool(a.is_augment), permute_points=True)                 # train.py:80
    val = split(val_cache, ntrain if nval else 0, nval, dev, is_augment=False, permute_points=False)        # train.py:81
    if train.pc.shape[1] != a.num_point or train.pc_ins.shape[2] != a.num_point_ins:
        raise SystemExit("the cache holds %d points per scene and %d per instance, the flags say %d and %d"
                         % (train.pc.shape[1], train.pc_ins.shape[2], a.num_point, a.num_point_ins))
    cfg = Config()
    cfg.BATCH_SIZE, cfg.NUM_CATEGORY, cfg.NUM_SAMPLE = a.batch_size, a.num_category, a.num_sample
    schedules = Schedules(a.batch_size, a.learning_rate, a.decay_step, a.decay_rate, a.KL_weight)
    trainer = Trainer(cfg, train, val, train_module=a.train_module, optimizer=a.optimizer, momentum=a.momentum, schedules=schedules,
                      log_dir=a.log_dir, seed=a.seed, captured=not a.eager, adam_rule=a.adam_rule, model_name=a.model)
    trainer.log_string(str(a))
    trainer.log_string('pid: %s' % str(os.getpid()))
    if a.restore_model_path is not None:
        trainer.restore(a.restore_model_path, scope=a.restore_scope)
    trainer.fit(a.max_epoch)
    trainer.close()


if __name__ == "__main__":
    main()
