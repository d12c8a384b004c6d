"""Instance AP over a directory pair written by gspn_amd.predict.write_predictions / write_ground_truth (the ScanNet benchmark's layout), with
the flags of the benchmark's own evaluation script:

    python tools/evaluate.py --pred_path eva/pred --gt_path eva/gt [--output_file eva/semantic_instance_evaluation.txt] [--scan_list FILE]

Prints the per-class table and the three averages.  The counting and the matching run on the device (gspn_amd/evaluate.py)."""
import argparse
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pred_path", required=True, help="the directory of <scan>.txt and pred_mask/")
    ap.add_argument("--gt_path", required=True, help="the directory of the ground truth <scan>.txt")
    ap.add_argument("--output_file", default="", help="the result file, default <pred_path>/semantic_instance_evaluation.txt")
    ap.add_argument("--scan_list", default="", help="a file with one scan name per line, default every *.txt of gt_path")
    a = ap.parse_args(argv)
    if not a.output_file:
        a.output_file = os.path.join(a.pred_path, "semantic_instance_evaluation.txt")
    return a


def scan_names(a):
    """the scans to evaluate: the lines of --scan_list, or every *.txt of gt_path, sorted"""
    if a.scan_list:
        with open(a.scan_list) as f:
            return [line.strip() for line in f if line.strip()]
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(a.gt_path, "*.txt")))


def format_table(result):
    """the benchmark's printed table -> a list of lines"""
    rule = "#" * 64
    lines = ["", rule, "{:<15}:{:>15}{:>15}{:>15}".format("what", "AP", "AP_50%", "AP_25%"), rule]
    for name in result["class_names"]:
        v = result["classes"][name]
        lines.append("{:<15}:{:>15.3f}{:>15.3f}{:>15.3f}".format(name, v["ap"], v["ap50%"], v["ap25%"]))
    lines += ["-" * 64, "{:<15}:{:>15.3f}{:>15.3f}{:>15.3f}".format("average", result["all_ap"], result["all_ap_50%"], result["all_ap_25%"]), ""]
    return lines


def main(argv=None):
    a = parse_args(argv)
    from gspn_amd.evaluate import evaluate_files, write_result_file
    scans = scan_names(a)
    if not scans:
        raise SystemExit("no scan to evaluate under %s" % a.gt_path)
    print("evaluating %d scans..." % len(scans))
    result = evaluate_files(a.pred_path, a.gt_path, scans)
    print("\n".join(format_table(result)))
    write_result_file(a.output_file, result)
    return result


if __name__ == "__main__":
    main()
