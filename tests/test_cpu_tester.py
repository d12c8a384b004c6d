"""CPU checks of the test driver (no GPU needed): tools/test.py's flags against the reference's (test.py:23-29), its exactly-one-of
--cache / --synthetic rule, gspn_sample_points_in_boxes_seeds in the library, the binding and the header at ABI 21 with the argument
checks of gspn_sample_points_in_boxes, and the scene_seeds checks of the three Python calls, which raise before anything runs."""
import ctypes
import importlib.util
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("tools_test", os.path.join(ROOT, "tools", "test.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_flag_defaults_are_the_reference_s():
    """test.py:23-29.  CONFIG there is config.Config(istrain=False), whose constructor assigns the test sizes to locals: the defaults it
    hands to argparse are the class attributes, NUM_SAMPLE = 256 among them (the help text says 2048)."""
    a = _tool().parse([])
    assert (a.gpu, a.num_point, a.num_point_ins, a.num_category, a.num_sample) == (0, 18000, 512, 19, 256)
    assert (a.model, a.model_path) == ('model_rpointnet', 'log/model.ckpt')
    assert (a.cache, a.synthetic, a.list, a.out, a.batch_size, a.seed, a.eager, a.no_files) == (None, 0, None, 'eva', 1, 0, False, False)
    types = {act.dest: act.type for act in _tool().parser()._actions}
    assert all(types[k] is int for k in ('gpu', 'num_point', 'num_point_ins', 'num_category', 'num_sample', 'batch_size', 'seed', 'synthetic'))
    b = _tool().parse(['--num_sample', '2048', '--model_path', 'x.ckpt', '--batch_size', '8', '--eager', '--no_files', '--list', 'val.txt'])
    assert (b.num_sample, b.model_path, b.batch_size, b.eager, b.no_files, b.list) == (2048, 'x.ckpt', 8, True, True, 'val.txt')


def test_config_of_the_flags():
    T = _tool()
    cfg = T.config_of(T.parse(['--num_category', '9', '--num_sample', '64']))
    assert (cfg.NUM_CATEGORY, cfg.NUM_SAMPLE, cfg.SPN_NMS_MAX_SIZE_INFERENCE, cfg.NUM_POINT_INS_MASK) == (9, 64, 96, 256)
    cfg = T.config_of(T.parse(['--test_sizes']))
    assert (cfg.NUM_SAMPLE, cfg.SPN_PRE_NMS_LIMIT, cfg.SPN_NMS_MAX_SIZE_INFERENCE, cfg.NUM_POINT_INS_MASK) == (2048, 1536, 384, 1024)
    assert T.config_of(T.parse(['--test_sizes', '--num_sample', '512'])).NUM_SAMPLE == 512


@pytest.mark.parametrize("argv", [[], ['--cache', 'val.pt', '--synthetic', '3'], ['--synthetic', '0'], ['--synthetic', '-2']])
def test_exactly_one_of_cache_and_synthetic(argv):
    with pytest.raises(SystemExit) as e:
        _tool().main(argv)
    assert "exactly one of --cache FILE and --synthetic S" in str(e.value)


def test_the_seeds_entry_is_exported_bound_and_declared_at_abi_21():
    from gspn_amd import _lib, build
    so = build.build()
    lib = _lib.lib()
    name = "gspn_sample_points_in_boxes_seeds"
    exported = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout.split()
    assert name in exported and "gspn_sample_points_in_boxes" in exported
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES["gspn_sample_points_in_boxes"]
    assert int(lib.gspn_abi_version()) == 21 == _lib.ABI_VERSION
    with open(os.path.join(ROOT, "include", "gspn_hip.h")) as f:
        header = f.read()
    assert "int %s(int b, int r, int n, int nsmp, float margin, const long long* seeds," % name in header
    assert "#define GSPN_ABI_VERSION 21" in header
    # the argument checks and error codes of gspn_sample_points_in_boxes
    null, f0 = ctypes.c_void_p(0), ctypes.c_float(0.0)
    for b, r, n, k in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0), (-1, 4, 4, 4), (4, -1, 4, 4), (4, 4, -1, 4), (4, 4, 4, -1)):
        assert getattr(lib, name)(b, r, n, k, f0, null, null, null, null, null) == -1
    assert getattr(lib, name)(1, 4, 32769, 4, f0, null, null, null, null, null) == -2
    assert getattr(lib, name)(65536, 4, 64, 4, f0, null, null, null, null, null) == -2


def _calls():
    """the three calls that take scene_seeds, on CPU tensors of a batch of 2, as functions of scene_seeds"""
    from gspn_amd import roi
    from gspn_amd.inference import rpointnet_inference
    from gspn_amd.rpointnet import Config
    boxes, pc = torch.ones(2, 3, 6), torch.zeros(2, 8, 3)
    cfg = Config()
    return [
        lambda s: roi.sample_points_in_boxes(boxes, pc, 4, 0, 0.0, scene_seeds=s),
        lambda s: roi.mask_selection_gen_batch(boxes, pc, 3, cfg, True, 0, scene_seeds=s),
        lambda s: rpointnet_inference(pc, pc, torch.zeros(2, 2, 4, 3), torch.zeros(2, 8, dtype=torch.int32), torch.ones(2, 2, dtype=torch.int32),
                                      torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, 2, 6), cfg, scene_seeds=s),
    ]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_scene_seeds_argument_checks(which):
    from gspn_amd import tf_util
    from gspn_amd._lib import GspnHipError
    store = tf_util.set_variable_store(tf_util.VariableStore(device=torch.device("cpu"), seed=0))
    call = _calls()[which]
    good = torch.zeros(2, dtype=torch.int64)
    for bad in (good.int(), good.double(), torch.zeros(3, dtype=torch.int64), torch.zeros(1, dtype=torch.int64),
                torch.zeros(2, 1, dtype=torch.int64), torch.zeros((), dtype=torch.int64)):
        with pytest.raises(ValueError, match="scene_seeds must be a \\(B,\\) = \\(2,\\) int64 tensor"):
            call(bad)
    with pytest.raises(TypeError):
        call([0, 1])
    with pytest.raises(GspnHipError, match="scene_seeds is on cpu"):                # the right dtype and shape on the wrong device
        call(good)
    assert not store.vars                                                          # nothing ran: no variable was created


def test_seed_tensor_keeps_its_one_element_rule():
    from gspn_amd.roi import seed_tensor
    with pytest.raises(ValueError):
        seed_tensor(torch.zeros(2, dtype=torch.int64), "cpu")
    with pytest.raises(ValueError):
        seed_tensor(torch.zeros(1, dtype=torch.int32), "cpu")
