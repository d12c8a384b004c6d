"""Times shape_proposal_net's two trunks (gspn_amd/spn_trunks.py) on one GPU.

  step      one training step of shift_pred_net + sem_net (forward + backward), (a) each trunk building its own geometry inline, as
            code written against the reference's modules does, and (b) with one spn_geometry shared by both (computed inside the step)
  full_fwd  the full-feature forward (return_fullfea=True, eval, mode='inference') with the dense 3-NN of spn_geometry by one three_nn per
            level vs one three_nn_nested scan
  nn        the dense 3-NN alone: three_nn onto l1, l2, l3, l4 (four launches) vs three_nn_nested (one launch)

Prints one JSON line per (shape, measurement): median / min milliseconds over --iters timed runs after --warmup runs.
    python tools/spn_step.py --shapes 2x18000,8x32768
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gspn_amd import synth, tf_util  # noqa: E402
from gspn_amd import spn_trunks as S  # noqa: E402
from gspn_amd.tf_interpolate import nested_local_maps, three_nn, three_nn_nested  # noqa: E402
from gspn_amd.tf_sampling import farthest_point_sample, gather_point  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4)}


def trunks(xyz, col, ns, nm, ncat, training, full, mode, geo):
    ep = S.shift_pred_net(xyz, col, ns, {}, 'shift_predictor', training, 0.5, return_fullfea=full, geometry=geo)
    return S.sem_net(xyz, col, nm, ncat, ep['ind_seed'], ep, 'sem_predictor', training, 0.5, return_fullfea=full, mode=mode, geometry=geo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2x18000,8x32768")
    ap.add_argument("--kind", default="S")
    ap.add_argument("--seed-points", type=int, default=128)          # shape_proposal_net's nsmp
    ap.add_argument("--sem-points", type=int, default=1024)          # model_rpointnet.py:345
    ap.add_argument("--categories", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ns, nm, ncat = a.seed_points, a.sem_points, a.categories
    for shape in a.shapes.split(","):
        b, n = (int(v) for v in shape.split("x"))
        xyz = torch.from_numpy(synth.batch(a.kind, b, n)).to(dev)
        col = torch.rand(b, n, 3, device=dev)
        tf_util.set_variable_store(tf_util.VariableStore(device=dev, seed=1))
        params = []

        def step(shared):
            def run():
                for p in params:
                    p.grad = None
                geo = S.spn_geometry(xyz, ns, nm, points=col) if shared else None
                ep = trunks(xyz, col, ns, nm, ncat, True, False, 'training', geo)
                (ep['shift_pred_seed_4d'].square().mean() + ep['sem_class_logits'].square().mean()).backward()
            return run

        step(False)()
        params[:] = tf_util.get_variable_store().parameters()
        res = {"inline_geometry": timed(step(False), a.warmup, a.iters), "shared_geometry": timed(step(True), a.warmup, a.iters)}
        print(json.dumps({"shape": shape, "kind": a.kind, "measure": "step", **res}), flush=True)

        def full(nested):
            def run():
                with torch.no_grad():
                    trunks(xyz, col, ns, nm, ncat, False, True, 'inference', S.spn_geometry(xyz, ns, nm, True, points=col, nested=nested))
            return run

        res = {"per_level_three_nn": timed(full(False), a.warmup, a.iters), "three_nn_nested": timed(full(True), a.warmup, a.iters)}
        print(json.dumps({"shape": shape, "kind": a.kind, "measure": "full_fwd", **res}), flush=True)

        # the dense 3-NN alone, on the geometry spn_geometry builds
        fps, order, cur, lv = [], None, xyz, []
        for npoint, _, _, _ in S.SPN_SA_SPEC:
            f, o = farthest_point_sample(npoint, cur, return_order=True)
            order = o if order is None else order
            fps.append(f)
            cur = gather_point(cur, f)
            lv.append(cur)
        local = nested_local_maps(lv[0].shape[1], fps[1:])
        res = {"per_level_three_nn": timed(lambda: [three_nn(xyz, lk, order=order) for lk in lv], a.warmup, a.iters),
               "three_nn_nested": timed(lambda: three_nn_nested(xyz, lv[0], local, order=order), a.warmup, a.iters)}
        print(json.dumps({"shape": shape, "kind": a.kind, "measure": "nn", **res}), flush=True)


if __name__ == "__main__":
    main()
