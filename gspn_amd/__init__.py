"""gspn_amd -- MI355X (gfx950) implementation of GSPN's PointNet++ set-abstraction hot path.

Module and function names mirror the reference (tf_ops/*/tf_*.py, utils/pointnet_util.py,
utils/tf_util.py) so model code calls them unchanged, over torch tensors on a ROCm device.
All compute goes through the C ABI of libgspn_hip.so (include/gspn_hip.h); there is no CPU
fallback.
"""
__version__ = "0.1.0"

# gspn_amd.dataset and its functions, resolved on first use: `import gspn_amd` (and `python -m gspn_amd.build`) stays free of torch
_DATASET = ("fps_segments", "instance_point_sets", "resample_scene", "remap_labels", "augment_and_box")
# gspn_amd.data_prep (and gspn_amd.io_util) likewise
_DATA_PREP = ("segment_labels", "collect_label", "downsample_scans", "prepare_scans", "build_cache")
__all__ = ["dataset", "data_prep", "io_util"] + list(_DATASET) + list(_DATA_PREP)


def __getattr__(name):
    if name == "dataset" or name in _DATASET:
        import importlib
        module = importlib.import_module(".dataset", __name__)
        return module if name == "dataset" else getattr(module, name)
    if name in ("data_prep", "io_util") or name in _DATA_PREP:
        import importlib
        module = importlib.import_module("." + (name if name == "io_util" else "data_prep"), __name__)
        return module if name in ("data_prep", "io_util") else getattr(module, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
