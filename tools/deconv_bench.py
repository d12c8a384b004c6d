"""Times the transposed-convolution kernels (csrc/deconv.hip) on decoding_net's layers at NUM_SAMPLE * B decodes, forward / grad-input /
grad-kernel+bias per layer with device events, and reports achieved FLOP/s against the FP32 MFMA peak (157.3 TF/s).
    python tools/deconv_bench.py [--n 512] [--branch 512] [--iters 20]
FLOPs are counted two ways: 'useful' = 2*n*Hi*Wi*kh*kw*Cin*Cout per pass (every tap product that lands in the output: the issue's table),
'issued' = what the kernels multiply, which for the forward includes the taps of a phase whose input row is masked to zero."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gspn_amd import _lib as L                      # noqa: E402
from gspn_amd.shape_proposal import decoder_layers, decoder_map_sizes   # noqa: E402

PEAK = 157.3e12


def issued_fwd(n, hi, cin, cout, k, s):
    """forward products the phase GEMMs multiply (square maps and kernels): per phase (n * phase pixels) x (phase taps * Cin) x Cout"""
    ho = hi * s + max(k - s, 0)
    if hi == 1:
        s = max(k, s)                              # the launcher's 1-pixel rule
    per_dim = 0
    for p in range(s):
        hq = (ho - p + s - 1) // s
        t = (k - p + s - 1) // s if p < k else 0
        per_dim += hq * t
    return 2.0 * n * cin * cout * per_dim ** 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--branch", type=int, default=512, help="num_point of decoding_net: 512, 1024 or 2048")
    ap.add_argument("--nfea", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = L.lib()
    st = L.stream()
    layers, _ = decoder_layers(args.branch)
    sizes = [1] + decoder_map_sizes(args.branch)
    cin = args.nfea
    rows = []
    for (name, cout, k, s, _), hi, ho in zip(layers, sizes[:-1], sizes[1:]):
        n = args.n
        x = torch.randn(n, hi, hi, cin, device=dev)
        kk = torch.randn(k, k, cout, cin, device=dev) * 0.05
        b = torch.randn(cout, device=dev)
        y = torch.empty(n, ho, ho, cout, device=dev)
        dy = torch.randn_like(y)
        dx = torch.empty_like(x)
        dk = torch.empty_like(kk)
        db = torch.empty_like(b)
        shape = (n, hi, hi, cin, cout, k, k, s, s)
        ws = torch.empty((int(lib.gspn_deconv_bwd_kernel_work_bytes(*shape)) + 3) // 4, device=dev)
        calls = {
            "fwd": lambda: lib.gspn_deconv_fwd(*shape, L.ptr(x), L.ptr(kk), L.ptr(b), L.ptr(y), st),
            "bwd_input": lambda: lib.gspn_deconv_bwd_input(*shape, L.ptr(dy), L.ptr(kk), L.ptr(dx), st),
            "bwd_kernel": lambda: lib.gspn_deconv_bwd_kernel(*shape, L.ptr(dy), L.ptr(x), L.ptr(dk), L.ptr(db), L.ptr(ws), st),
        }
        useful = 2.0 * n * hi * hi * k * k * cin * cout
        for op, fn in calls.items():
            for _ in range(3):
                L.check(fn(), op)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            sec = e0.elapsed_time(e1) / 1e3 / args.iters
            issued = issued_fwd(n, hi, cin, cout, k, s) if op == "fwd" else useful
            rows.append({"layer": name, "op": op, "n": n, "in": hi, "out": ho, "cin": cin, "cout": cout, "k": k, "s": s, "us": round(sec * 1e6, 1),
                         "useful_gflop": round(useful / 1e9, 3), "issued_gflop": round(issued / 1e9, 3),
                         "useful_frac_peak": round(useful / sec / PEAK, 3), "issued_frac_peak": round(issued / sec / PEAK, 3)})
            print(json.dumps(rows[-1]), flush=True)
        cin = cout
    for sel in (("upconv2", "upconv3"), tuple(r["layer"] for r in rows)):
        rs = [r for r in rows if r["layer"] in sel]
        sec = sum(r["us"] for r in rs) / 1e6
        print(json.dumps({"layers": sorted(set(sel)), "us": round(sec * 1e6, 1), "useful_frac_peak": round(sum(r["useful_gflop"] for r in rs) * 1e9 / sec / PEAK, 3),
                          "issued_frac_peak": round(sum(r["issued_gflop"] for r in rs) * 1e9 / sec / PEAK, 3)}), flush=True)


if __name__ == "__main__":
    main()
