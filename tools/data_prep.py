"""The reference's data_prep.py on this library, with its two positional arguments:

    python tools/data_prep.py DATASET_PATH OUT_PATH [--nsample 30000] [--batch B] [--scans scene0000_00,scene0001_00]

Reads DATASET_PATH/mesh/scans/<scan>/<scan>_vh_clean_2.ply and, under DATASET_PATH/label/scans/<scan>/, <scan>.aggregation.json,
<scan>_vh_clean_2.0.010000.segs.json and <scan>_vh_clean_2.labels.ply; writes OUT_PATH/mesh/scans/<scan>.ply,
OUT_PATH/label/scans/sem_<scan>.txt and group_<scan>.txt.  The labels and the sampling run on the device (gspn_amd/data_prep.py).
--batch: scans per farthest_point_sample call (DESIGN.md 4.19 has the measurement behind the default)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEFAULT_BATCH = 8         # measured fastest of 1, 2, 4, 8 (profiles/data_prep.txt): eight scans share a call in the time of the largest one


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("dataset_path", metavar="DATASET_PATH", help="e.g. ./data/scannet")
    ap.add_argument("out_path", metavar="OUT_PATH", help="e.g. ./data/scannet_preprocessed")
    ap.add_argument("--nsample", type=int, default=30000, help="points kept per scan [default: 30000]")
    ap.add_argument("--batch", type=int, default=DEFAULT_BATCH, help="scans per sampling call [default: %d]" % DEFAULT_BATCH)
    ap.add_argument("--scans", default="", help="comma-separated scan names, default every directory of DATASET_PATH/mesh/scans")
    ap.add_argument("--gpu", type=int, default=0, help="GPU to use [default: GPU 0]")
    a = ap.parse_args(argv)
    a.scans = [name for name in a.scans.split(",") if name] or None
    return a


def main(argv=None):
    a = parse_args(argv)
    import torch
    from gspn_amd.data_prep import prepare_scans
    dev = torch.device("cuda", a.gpu)
    torch.cuda.set_device(dev)
    report = prepare_scans(a.dataset_path, a.out_path, a.nsample, a.batch, a.scans, dev)
    print("%d scans written to %s (%d with label conflicts)" % (len(report), a.out_path, sum(1 for r in report if r[3])))
    return report


if __name__ == "__main__":
    main()
