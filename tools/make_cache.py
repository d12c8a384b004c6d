"""The training cache of the reference's dataset.py (:38-125) from the output of tools/data_prep.py, as the file tools/train.py --cache loads:

    python tools/make_cache.py --mesh_path OUT/mesh/scans --label_path OUT/label/scans --list train.txt --out train.pt \\
        [--npoint 18000] [--npoint_ins 512] [--seed 0] [--batch 8]

--list names one scan per line.  The file is a torch.save'd dict of pc, color, group_label, seg_label, pc_ins and ngroup
(gspn_amd.data_prep.build_cache, whose docstring has the seed rule)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mesh_path", required=True, help="the directory of <scan>.ply")
    ap.add_argument("--label_path", required=True, help="the directory of sem_<scan>.txt and group_<scan>.txt")
    ap.add_argument("--list", required=True, help="a file with one scan name per line")
    ap.add_argument("--out", required=True, help="the cache file to write")
    ap.add_argument("--npoint", type=int, default=18000, help="Point Number in a Scene [default: 18000]")
    ap.add_argument("--npoint_ins", type=int, default=512, help="Point Number of an Instance [default: 512]")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=8, help="scenes of equal size per call [default: 8]")
    ap.add_argument("--gpu", type=int, default=0, help="GPU to use [default: GPU 0]")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from gspn_amd.data_prep import build_cache
    dev = torch.device("cuda", a.gpu)
    torch.cuda.set_device(dev)
    cache = build_cache(a.mesh_path, a.label_path, a.list, a.npoint, a.npoint_ins, a.seed, a.batch, dev)
    torch.save(cache, a.out)
    print("%d scenes of %d points, %d groups of %d points -> %s" % (cache["pc"].shape[0], cache["pc"].shape[1], cache["pc_ins"].shape[1],
                                                                    cache["pc_ins"].shape[2], a.out))
    return cache


if __name__ == "__main__":
    main()
