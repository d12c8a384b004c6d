"""The reference's test.py on this library: its flags (test.py:23-29), gspn_amd.tester.Tester underneath.  From a checkpoint of
tools/train.py and a validation cache to <out>/gt, <out>/pred (the ScanNet benchmark's layout) and the AP figures.

The reference reads ScanNet meshes and labels through dataset.py's cache (test.py:40-44); here, as in tools/train.py:
  --cache FILE       a torch.save'd dict of the six cache tensors of gspn_amd.train.DeviceDataset, as tools/make_cache.py writes it
  --synthetic S      S scenes from gspn_amd.synth.spn_batch instead
and, not in the reference:
  --list FILE        one scan name per line, one per scene of the cache, the stems of the files written (test.py:42; default scene_%04d)
  --out DIR          where gt/ and pred/ go [default: eva, test.py:210]
  --batch_size B     scenes per step [default: 1, test.py:213]; a scene's predictions do not depend on it beyond the GEMMs' rounding
  --test_sizes       the sizes models/config.py names for testing and never sets (its constructor assigns them to locals): NUM_SAMPLE 2048,
                     SPN_PRE_NMS_LIMIT 1536, SPN_NMS_MAX_SIZE_INFERENCE 384, NUM_POINT_INS_MASK 1024.  Without it the run has the sizes the
                     reference's test.py really runs with, the training ones.  --num_sample, when it is not the default, still wins.
  --seed, --eager (no graph capture), --no_files (AP only, nothing written)
and, for predictions at the resolution of each scan's own mesh (Tester.run_vertices, DESIGN.md 4.21: one mask value per vertex, the
ScanNet benchmark's format, into <out>/pred_vertices and <out>/gt_vertices, with AP and mean IoU per vertex):
  --mesh_path DIR    ScanNet's layout as tools/data_prep.py reads it, DIR/<scan>/<scan>_vh_clean_2.ply, the scans named by --list
  --label_path DIR   optional: the vertices' ground truth, DIR/<scan>/ as data_prep.collect_label reads it, through dataset.remap_labels;
                     without it the masks are written and nothing is evaluated
  --synthetic_vertices V   with --synthetic: each scene's scan is its N points followed by V - N jittered copies of seeded scene points
                     that inherit their labels
and, on top of either, the segment vote (masks and semantic labels snapped to the segments of each scan's over-segmentation):
  --segments         with --mesh_path and --label_path: each scan's segIndices, <label_path>/<scan>/<scan>_vh_clean_2.0.010000.segs.json;
                     with --synthetic_vertices: synth.scan_segments, cubes of --segment_cell inside every instance
  --vote_th T        a segment is set where more than T of its vertices are [default: 0.5]; in [0, 1)
and mask NMS (a per-vertex mask that copies an earlier one of its label is emptied before the files and the figures):
  --mask_nms T       with --mesh_path or --synthetic_vertices: suppress a mask whose IoU with an earlier kept one of its label is above T,
                     in [0, 1); behind the segment vote where --segments is given [default: off]
and mask components (the fragments of a per-vertex mask that the mesh's edges do not join to its body are dropped):
  --components N     with --mesh_path (the faces of each scan's <scan>_vh_clean_2.ply) or --synthetic_vertices (synth.scan_faces): drop a
                     component of fewer than N >= 1 vertices; behind the segment vote, before mask NMS [default: off]
  --component_share S   with --components: also drop a component smaller than S of its mask's largest; in [0, 1] [default: 0]
and mask holes (the gaps a per-vertex mask encloses on the mesh are filled):
  --holes N          with --mesh_path or --synthetic_vertices, the faces as for --components: fill an enclosed gap of at most N >= 0
                     vertices; behind --components, before mask NMS [default: off]
  --hole_share S     with --holes: and of at most S of the mask's set vertices; in [0, 1] [default: 1]

    python tools/test.py --synthetic 5 --num_point 4096 --num_sample 64 --num_category 9 --batch_size 2 --model_path log/model.ckpt
    python tools/test.py --cache val.pt --list scannet_val.txt --model_path log_heads/model.ckpt --batch_size 8
    python tools/test.py --cache val.pt --list scannet_val.txt --model_path log_heads/model.ckpt --batch_size 8 \\
        --mesh_path scannet/mesh/scans --label_path scannet/label/scans
    python tools/test.py --cache val.pt --list scannet_val.txt --model_path log_heads/model.ckpt --batch_size 8 \\
        --mesh_path scannet/mesh/scans --label_path scannet/label/scans --segments
    python tools/test.py --cache val.pt --list scannet_val.txt --model_path log_heads/model.ckpt --batch_size 8 \\
        --mesh_path scannet/mesh/scans --label_path scannet/label/scans --segments --mask_nms 0.5
    python tools/test.py --cache val.pt --list scannet_val.txt --model_path log_heads/model.ckpt --batch_size 8 \\
        --mesh_path scannet/mesh/scans --label_path scannet/label/scans --segments --components 100 --component_share 0.1 --mask_nms 0.5
    python tools/test.py --cache val.pt --list scannet_val.txt --model_path log_heads/model.ckpt --batch_size 8 \\
        --mesh_path scannet/mesh/scans --label_path scannet/label/scans --segments --components 100 --holes 200 --hole_share 0.25 --mask_nms 0.5
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gspn_amd import synth  # noqa: E402
from gspn_amd.rpointnet import Config  # noqa: E402

CACHE_KEYS = ("pc", "color", "group_label", "seg_label", "pc_ins", "ngroup")


def parser():
    cfg = Config()
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--gpu', type=int, default=0, help='GPU to use [default: GPU 0]')
    ap.add_argument('--num_point', type=int, default=cfg.NUM_POINT, help='Point Number in a Scene [default: 18000]')
    ap.add_argument('--num_point_ins', type=int, default=cfg.NUM_POINT_INS, help='Point Number of an Instance [default: 512]')
    ap.add_argument('--num_category', type=int, default=cfg.NUM_CATEGORY, help='Maximum Number of Categories [default: 19]')
    ap.add_argument('--num_sample', type=int, default=cfg.NUM_SAMPLE, help='Number of Sampled Seed Points [default: 256]')
    ap.add_argument('--model', default='model_rpointnet', help='Model name [default: model_rpointnet]')
    ap.add_argument('--model_path', default='log/model.ckpt', help='model checkpoint file path [default: log/model.ckpt]')
    # not in the reference
    ap.add_argument('--cache', default=None, help='torch.save file of the six cache tensors of the scenes to test')
    ap.add_argument('--synthetic', type=int, default=0, help='number of synthetic scenes to test on instead of --cache')
    ap.add_argument('--num_group', type=int, default=12, help='groups per synthetic scene [default: 12]')
    ap.add_argument('--list', default=None, help='file of scan names, one per scene [default: scene_%%04d]')
    ap.add_argument('--out', default='eva', help='output directory [default: eva]')
    ap.add_argument('--batch_size', type=int, default=1, help='scenes per step [default: 1]')
    ap.add_argument('--restore_scope', default=None, help='restore only the variables under this scope')
    ap.add_argument('--test_sizes', action='store_true', help="Config(istrain=False): the test sizes models/config.py names")
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--eager', action='store_true', help='do not capture the step in a graph')
    ap.add_argument('--no_files', action='store_true', help='write nothing, print the figures only')
    ap.add_argument('--mesh_path', default=None, help='directory of <scan>/<scan>_vh_clean_2.ply: predict on every vertex of each scan of --list')
    ap.add_argument('--label_path', default=None, help="directory of the scans' label files: the vertices' ground truth (with --mesh_path)")
    ap.add_argument('--synthetic_vertices', type=int, default=0, help='vertices of the synthetic scan around each synthetic scene')
    ap.add_argument('--segments', action='store_true', help="snap the per-vertex masks and labels to each scan's segments (the segment vote)")
    ap.add_argument('--vote_th', type=float, default=0.5, help='the share of a segment above which it is set [default: 0.5]')
    ap.add_argument('--segment_cell', type=float, default=0.25, help='side of a synthetic segment (with --synthetic_vertices) [default: 0.25]')
    ap.add_argument('--mask_nms', type=float, default=None, help='suppress per-vertex masks above this IoU with an earlier one of their label [default: off]')
    ap.add_argument('--components', type=int, default=None, help='drop the components of a per-vertex mask with fewer vertices than this [default: off]')
    ap.add_argument('--component_share', type=float, default=0.0, help="and those smaller than this share of the mask's largest [default: 0]")
    ap.add_argument('--holes', type=int, default=None, help='fill the gaps a per-vertex mask encloses on the mesh of at most this many vertices [default: off]')
    ap.add_argument('--hole_share', type=float, default=1.0, help="and of at most this share of the mask's set vertices [default: 1]")
    return ap


def parse(argv=None):
    return parser().parse_args(argv)


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


def synthetic_vertices(cache, v, seed, segment_cell=None, face_cell=None):
    """vertices(k) of Tester.run_vertices for the scenes of synthetic_cache: synth.scan_vertices around scene k, seeded with seed + k;
    with a segment_cell also 'segments', synth.scan_segments of that scan with the same seed; with a face_cell also 'faces',
    synth.scan_faces of it"""
    def vertices(k):
        xyz, seg, group = synth.scan_vertices(cache["pc"][k].numpy(), cache["seg_label"][k].numpy(), cache["group_label"][k].numpy(), v, seed + k)
        out = {"xyz": xyz, "seg_label": seg, "group_label": group}
        if segment_cell is not None:
            out["segments"] = synth.scan_segments(xyz, seg, group, segment_cell, seed + k)
        if face_cell is not None:
            out["faces"] = synth.scan_faces(xyz, seg, group, face_cell, seed + k)
        return out
    return vertices


def mesh_vertices(mesh_path, label_path, scans, device, segments=False, faces=False):
    """vertices(k) of Tester.run_vertices from ScanNet's files: the vertices of <mesh_path>/<scan>/<scan>_vh_clean_2.ply as
    tools/data_prep.py reads them and, with a label_path, their labels through data_prep.collect_label and dataset.remap_labels;
    segments: also 'segments', data_prep.read_segments of the scan; faces: also 'faces', io_util.read_ply_faces of the same file"""
    import numpy as np
    from gspn_amd import data_prep, dataset, io_util

    def vertices(k):
        scan = scans[k]
        out = {"xyz": np.ascontiguousarray(io_util.read_color_ply(os.path.join(mesh_path, scan, scan + "_vh_clean_2.ply"))[:, :3], np.float32)}
        if faces:
            out["faces"] = io_util.read_ply_faces(os.path.join(mesh_path, scan, scan + "_vh_clean_2.ply"))
        if label_path:
            sem, ins, _ = data_prep.collect_label(label_path, scan, device=device)
            group, seg, _ = dataset.remap_labels(ins.unsqueeze(0), sem.unsqueeze(0), max(int(ins.max()), 0) + 1)
            out["seg_label"], out["group_label"] = seg[0].int(), group[0].int()
        if segments:
            out["segments"] = data_prep.read_segments(label_path, scan)
        return out
    return vertices


def read_list(path):
    with open(path) as f:
        return [line.strip() for line in f if line.strip()]


def config_of(a):
    cfg = Config(istrain=not a.test_sizes)
    if not a.test_sizes or a.num_sample != Config.NUM_SAMPLE:
        cfg.NUM_SAMPLE = a.num_sample
    cfg.NUM_CATEGORY = a.num_category
    return cfg


def main(argv=None):
    a = parse(argv)
    if (a.cache is None) == (a.synthetic <= 0):
        raise SystemExit("give exactly one of --cache FILE and --synthetic S")
    from gspn_amd.predict import SCANNET_LABEL_MAP
    from gspn_amd.tester import Tester
    from gspn_amd.train import DeviceDataset
    if a.mesh_path and a.synthetic_vertices:
        raise SystemExit("give at most one of --mesh_path DIR and --synthetic_vertices V")
    if a.mesh_path and not a.list:
        raise SystemExit("--mesh_path needs --list FILE: the scans whose meshes to read")
    if a.label_path and not a.mesh_path:
        raise SystemExit("--label_path goes with --mesh_path")
    if a.synthetic_vertices and (a.synthetic <= 0 or a.synthetic_vertices < a.num_point):
        raise SystemExit("--synthetic_vertices V goes with --synthetic S and V >= --num_point")
    if a.segments and not (a.synthetic_vertices or (a.mesh_path and a.label_path)):
        raise SystemExit("--segments goes with --mesh_path DIR --label_path DIR (the scans' segs.json) or with --synthetic_vertices V")
    if not 0.0 <= a.vote_th < 1.0:
        raise SystemExit("--vote_th must lie in [0, 1)")
    if not a.segment_cell > 0:
        raise SystemExit("--segment_cell must be positive")
    if a.mask_nms is not None and not (a.synthetic_vertices or a.mesh_path):
        raise SystemExit("--mask_nms goes with the vertex modes: --mesh_path DIR or --synthetic_vertices V")
    if a.mask_nms is not None and not 0.0 <= a.mask_nms < 1.0:
        raise SystemExit("--mask_nms must lie in [0, 1)")
    if a.components is None and a.component_share != 0.0:
        raise SystemExit("--component_share goes with --components N")
    if a.components is not None and not (a.synthetic_vertices or a.mesh_path):
        raise SystemExit("--components goes with the vertex modes: --mesh_path DIR or --synthetic_vertices V")
    if a.components is not None and (a.components < 1 or not 0.0 <= a.component_share <= 1.0):
        raise SystemExit("--components must be at least 1 and --component_share must lie in [0, 1]")
    if a.holes is None and a.hole_share != 1.0:
        raise SystemExit("--hole_share goes with --holes N")
    if a.holes is not None and not (a.synthetic_vertices or a.mesh_path):
        raise SystemExit("--holes goes with the vertex modes: --mesh_path DIR or --synthetic_vertices V")
    if a.holes is not None and (a.holes < 0 or not 0.0 <= a.hole_share <= 1.0):
        raise SystemExit("--holes must not be negative and --hole_share must lie in [0, 1]")
    if not 2 <= a.num_category <= len(SCANNET_LABEL_MAP):
        raise SystemExit("--num_category must lie in [2, %d], the classes of the ScanNet label map" % len(SCANNET_LABEL_MAP))
    dev = torch.device("cuda", a.gpu)
    torch.cuda.set_device(dev)
    cache = load_cache(a.cache) if a.cache else synthetic_cache(a)
    data = DeviceDataset(*[cache[k].to(dev) for k in CACHE_KEYS], is_augment=False, permute_points=False)          # test.py:44
    if data.pc.shape[1] != a.num_point or data.pc_ins.shape[2] != a.num_point_ins:
        raise SystemExit("the cache holds %d points per scene and %d per instance, the flags say %d and %d"
                         % (data.pc.shape[1], data.pc_ins.shape[2], a.num_point, a.num_point_ins))
    scans = read_list(a.list) if a.list else None
    if scans is not None and len(scans) != len(data):
        raise SystemExit("%s names %d scans, the cache holds %d scenes" % (a.list, len(scans), len(data)))
    tester = Tester(config_of(a), data, scans=scans, batch_size=a.batch_size, seed=a.seed, captured=not a.eager,
                    label_map=SCANNET_LABEL_MAP[:a.num_category], vote_th=a.vote_th, mask_nms_th=a.mask_nms,
                    min_component=a.components, min_component_share=a.component_share, max_hole=a.holes, max_hole_share=a.hole_share)
    tester.restore(a.model_path, scope=a.restore_scope)
    if a.mesh_path or a.synthetic_vertices:
        meshed = a.components is not None or a.holes is not None      # the faces are read or drawn for either stage
        vertices = (mesh_vertices(a.mesh_path, a.label_path, scans, dev, a.segments, meshed) if a.mesh_path
                    else synthetic_vertices(cache, a.synthetic_vertices, a.seed, a.segment_cell if a.segments else None,
                                            a.segment_cell if meshed else None))
        result = tester.run_vertices(None if a.no_files else a.out, vertices, evaluate=bool(a.synthetic_vertices or a.label_path))
        if result is None:
            print("per-vertex masks written to %s (no --label_path: nothing to evaluate against)" % os.path.join(a.out, "pred_vertices"))
            return None
    else:
        result = tester.run(out_dir=None if a.no_files else a.out, evaluate=True)
    print("AP: %.3f  AP_50%%: %.3f  AP_25%%: %.3f  mean IoU: %.3f" % (result["all_ap"], result["all_ap_50%"], result["all_ap_25%"], result["iou"]))
    return result


if __name__ == "__main__":
    main()
