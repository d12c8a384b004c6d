"""The split-K kernels of the short layers (csrc/mlp_short.hip, r05): the forward of layers with <= 8192 rows (default path) against an fp64
product -- outputs, the per-workgroup partial column sums the batch norm is finalised from, the 32-row pool epilogue (maximum AND the first
row that reaches it).
utils/pointnet_util.py:109-113,165-169 (the FP1 / SA3 shapes of models/model_rpointnet.py:226-230)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("rows,cin,cout,act,pool", [(4096, 384, 256, False, False), (4096, 256, 128, True, False), (4096, 128, 128, False, False),
                                                    (8192, 64, 64, True, True), (2048, 192, 96, True, True), (1024, 128, 256, True, False),
                                                    (64, 64, 32, False, True), (4032, 256, 64, True, False)])
def test_short_forward_against_fp64(rows, cin, cout, act, pool):
    from tests.test_gpu_mlp_instances import check_forward        # this test's former body, with the shape's alignment and pitches as parameters
    check_forward(rows, cin, cout, act, pool)


def test_short_forward_is_deterministic():
    from gspn_amd import _lib as L
    lib = L.lib()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    rows, cin, cout = 4096, 256, 128
    X = torch.randn(rows, cin, device=dev, generator=gen)
    W = torch.randn(cin, cout, device=dev, generator=gen)
    outs = []
    for _ in range(3):
        Y = torch.empty(rows, cout, device=dev)
        stats = torch.empty(int(lib.gspn_mlp_fwd_stats_bytes(rows, cout)) // 4, device=dev)
        L.check(lib.gspn_mlp_fwd(rows, cin, cout, L.ptr(X), cin, None, None, L.ptr(W), None, L.ptr(Y), cout, L.ptr(stats), L.stream()), "fwd")
        outs.append((Y, stats))
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]) for o in outs[1:])
