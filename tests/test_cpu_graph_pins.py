"""The stages models/model_rpointnet.py writes as TensorFlow graph code, against what the REFERENCE's own lines gave on recorded inputs:
the fixtures tools/make_golden_graph.py writes under tests/golden/graph/ by cutting the line ranges out of a checkout of the reference and
exec'ing them over tools/tf_numpy.py, a numpy stand-in for the TensorFlow 1.x ops they call.  Nothing is rebuilt here: inputs
and outputs are read from the fixtures.  Four parts:

  1. the stand-in's ops, each on a small worked example of the op's documented behaviour, with the dtype rules it promises;
  2. the fixtures' case names against this file's own list;
  3. every restatement in tests/*_ref.py (and the product code that is plain torch and so runs on CPU tensors) against its fixture;
  4. the conditions the generator asserted, re-checked from the stored inputs, so that an edited fixture cannot quietly sit on a threshold.

What "equal" means per stage ("exact": equal integers, equal float32 values -- a zero of either sign is a zero: the reference's
`box * keep` and `mask * roi_mask` give -0.0 where the product writes 0.0):
  box_shrink, gather_selection, points_cropping, segmentation   exact
  spn_target_gen, mask_selection (proposals)                    exact
  box_delta, refined boxes without SHRINK_BOX, the losses       within a bound derived here, against the float64 run of the same lines
  detection_target                                              the tables everything is drawn from: check_detection_targets
  refine_detections                                             the selected rows, class ids and class scores exact; boxes as above"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import detect_ref as DR
from tests import heads_ref as HR
from tests import roi_ref as RR
from tests import spn_ref as SR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "graph")
U = 2.0 ** -24                      # the relative error of one float32 rounding; a float32 step (ulp) is at most 2 U |x|

REQUIRED = {
    "box_shrink": ("no_point_inside", "one_point_inside_zeroed", "flat_in_one_axis_zeroed", "point_on_lower_face", "point_on_upper_face", "holds_every_point",
                   "scene_offset_100"),
    "spn_target_gen": ("class_0_rows_between_valid", "no_valid_ground_truth_all_minus_1", "background_seed_above_0.5_neutral", "argmax_below_0.5_positive",
                       "ground_truth_without_foreground_overlap", "tie_lower_index_wins"),
    "gather_selection": ("minus_1_between_picks", "minus_1_first_and_last", "minus_1_tail", "index_0_and_last", "repeated_index"),
    "box_delta": ("rows", "equal_sizes", "zero_delta"),
    "detection_target": ("zero_row_in_the_middle", "proposal_without_point_dropped", "more_positives_than_cap", "fewer_negatives_than_negative_count",
                         "scene_without_ground_truth", "count_table_rows"),
    "mask_selection": ("point_5e-4_outside_counts", "point_2e-3_outside_does_not", "empty_dropped_under_removal", "empty_kept_without_removal",
                       "more_proposals_than_num_rois"),
    "points_cropping": ("all_zero_roi", "roi_sums_to_0_not_zero", "repeated_indices"),
    "refine_detections": ("more_survivors_than_outputs", "class_full", "repicked_zero_volume", "no_candidate", "equal_top_probabilities_first_column",
                          "class_0_rows", "below_min_confidence"),
    "segmentation": ("duplicated_crop_point_is_nearest", "scene_point_on_roi_face", "all_zero_roi", "roi_without_scene_point"),
    "losses": ("diff_exactly_1", "diff_one_step_below_1", "diff_one_step_above_1", "no_positive_or_negative_spn_match_gives_0", "no_valid_roi_gives_0",
               "valid_roi_of_class_0"),
    "get_loss": ("zero_weights_sampled", "nonzero_count_differs_from_rows_and_sum"),
}
# which of the stand-in's two named stand-ins each fixture's run went through
STAND_INS = {"spn_target_gen": ["scatter_nd_rank1"], "detection_target": ["random_shuffle"], "get_loss": ["scatter_nd_rank1"]}

_loaded = {}


def fixture(stage):
    """the arrays of one fixture, read once and never written"""
    if stage not in _loaded:
        with np.load(os.path.join(GOLDEN, stage + ".npz"), allow_pickle=False) as f:
            _loaded[stage] = {k: f[k] for k in f.files}
        for a in _loaded[stage].values():
            a.setflags(write=False)
    return _loaded[stage]


def t(a, dtype=None):
    x = torch.from_numpy(np.array(a))
    return x if dtype is None else x.to(dtype)


def same_values(got, want):
    """equal shapes, dtypes and values (a zero of either sign is a zero)"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)


def unpack(bits, n):
    return np.unpackbits(bits, axis=-1)[..., :n].astype(bool)


@pytest.fixture(scope="module")
def tfn():
    spec = importlib.util.spec_from_file_location("tf_numpy", os.path.join(os.path.dirname(HERE), "tools", "tf_numpy.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


# ---- 1. the stand-in ---------------------------------------------------------------------------------------------------------------------

def test_stand_in_dtype_rules(tfn):
    tf = tfn.namespace()
    x = tf.constant(np.array([1.5, -2.0, 3.0], np.float32))
    for y in (x * 2.0, 1e4 * x, x / 2, 1 - x, x + 1e-8, x ** 2, x * np.array([0.1, 0.2, 0.3]), tf.multiply(x, 3), tf.divide(x, 1e-8), tf.maximum(x, 0),
              tf.exp(x), tf.reduce_sum(x), tf.reduce_mean(x), tf.to_float(tf.constant([1, 2])), tf.cast(x > 0, tf.float32), tf.constant(0.0), tf.constant([])):
        assert isinstance(y, tfn.Tensor) and y.dtype == np.float32                        # a Python scalar or a float64 array never widens
    assert tf.constant([1, 2]).dtype == np.int32 and tf.range(3).dtype == np.int32 and tf.shape(x).dtype == np.int32 and tf.size(x).dtype == np.int32
    assert tf.where(x > 0).dtype == np.int64 and tf.where(x > 0).shape == (2, 1)
    assert tf.argmax(x).dtype == np.int64 and tf.argmax(x, output_type=tf.int32).dtype == np.int32 and tf.argmin(x, 0, output_type=tf.int32).dtype == np.int32
    assert tf.cast(tf.constant(np.float32(63.99)), tf.int32) == 63 and tf.cast(tf.constant(np.float32(-1.5)), tf.int32) == -1      # toward zero
    assert tf.cast(tf.constant(np.array([0.0, 0.25], np.float32)), tf.bool).tolist() == [False, True]
    with pytest.raises(TypeError):
        tf.constant([1, 2]) + x                                                          # TensorFlow does not convert between tensors
    with pytest.raises(TypeError):
        tf.concat((tf.constant([1]), tf.constant([1.0])), 0)
    with pytest.raises(TypeError):
        tf.constant([1, 2]) * 0.5
    # the precision switch: the same calls mean float64
    tf64 = tfn.namespace("float64")
    x64 = tf64.constant(np.array([1.5, -2.0, 3.0], np.float32))
    assert x64.dtype == np.float64 and tf64.float32 == np.float64 and tf64.cast(tf64.range(3), tf64.float32).dtype == np.float64 and (x64 * 0.1).dtype == np.float64
    assert tf64.constant(0.0).dtype == np.float64 and tf64.to_float(tf64.range(2)).dtype == np.float64
    r = 1.0 / 0.33
    assert float(r * tf.cast(np.int32(33), tf.float32)) == float(np.float32(r) * np.float32(33)) and float(r * tf64.cast(np.int32(33), tf64.float32)) == r * 33
    assert x.get_shape()[0].value == 3 and len(x.get_shape()) == 1
    x.set_shape([3])
    with pytest.raises(ValueError):
        x.set_shape([4])


def test_stand_in_shape_ops(tfn):
    tf = tfn.namespace()
    m = tf.constant(np.arange(6, dtype=np.int32).reshape(2, 3))
    assert tf.reshape(m, [-1]).tolist() == [0, 1, 2, 3, 4, 5] and tf.reshape(m, [3, -1]).shape == (3, 2)
    assert tf.expand_dims(m, 1).shape == (2, 1, 3) and tf.expand_dims(m, -1).shape == (2, 3, 1) and tf.squeeze(tf.expand_dims(m, 0), 0).shape == (2, 3)
    assert tf.tile(tf.constant([[1, 2]]), [2, 2]).tolist() == [[1, 2, 1, 2], [1, 2, 1, 2]]                 # the documented example's pattern
    assert tf.transpose(m).tolist() == [[0, 3], [1, 4], [2, 5]] and tf.transpose(tf.reshape(m, [1, 2, 3]), perm=[0, 2, 1]).shape == (1, 3, 2)
    assert tf.pad(tf.constant([[1, 2, 3], [4, 5, 6]]), [[1, 1], [2, 2]]).tolist() == [[0] * 7, [0, 0, 1, 2, 3, 0, 0], [0, 0, 4, 5, 6, 0, 0], [0] * 7]
    assert tf.pad(tf.constant([5]), [(0, 2)], mode="CONSTANT", constant_values=-1).tolist() == [5, -1, -1]
    assert tf.shape(m).tolist() == [2, 3] and int(tf.size(m)) == 6 and tf.range(2, 5).tolist() == [2, 3, 4]
    assert tf.ones_like(m).tolist() == [[1, 1, 1], [1, 1, 1]] and tf.ones_like(m).dtype == np.int32
    assert tf.concat([m, m], 0).shape == (4, 3) and tf.concat([m, m], 1).shape == (2, 6) and tf.stack([m, m], axis=1).shape == (2, 2, 3)
    assert m[..., tf.newaxis].shape == (2, 3, 1)


def test_stand_in_indexing_ops(tfn):
    tf = tfn.namespace()
    p = tf.constant(np.array([[10, 11], [20, 21], [30, 31]], np.int32))
    assert tf.gather(p, tf.constant([2, 0])).tolist() == [[30, 31], [10, 11]] and tf.gather(p, tf.constant([1, 1]), axis=1).tolist() == [[11, 11], [21, 21], [31, 31]]
    assert tf.gather(p, tf.cast(tf.constant([]), tf.int64)).shape == (0, 2)
    with pytest.raises(IndexError):
        tf.gather(p, tf.constant([-1]))                                                  # numpy would wrap around
    assert tf.gather_nd(p, tf.constant([[0, 0], [1, 1]])).tolist() == [10, 21] and tf.gather_nd(p, tf.constant([[1], [0]])).tolist() == [[20, 21], [10, 11]]   # the documented examples
    cond = tf.constant(np.array([[True, False], [False, True], [True, True]]))
    assert tf.where(cond).tolist() == [[0, 0], [1, 1], [2, 0], [2, 1]]                   # row-major coordinates
    assert tf.where(tf.constant(np.array([True, False])), tf.constant([1, 2]), tf.constant([3, 4])).tolist() == [1, 4]
    assert tf.boolean_mask(tf.constant([0, 1, 2, 3]), tf.constant(np.array([True, False, True, False]))).tolist() == [0, 2]    # the documented example
    assert tf.boolean_mask(p, tf.constant(np.array([True, False, True]))).tolist() == [[10, 11], [30, 31]]
    # scatter_nd, the documented example: indices [[4], [3], [1], [7]], updates [9, 10, 11, 12], shape [8]
    assert tf.scatter_nd(tf.constant([[4], [3], [1], [7]]), tf.constant([9, 10, 11, 12]), tf.constant([8])).tolist() == [0, 11, 0, 10, 9, 0, 0, 12]
    assert tf.scatter_nd(tf.constant([[1], [1]]), tf.constant([2.0, 3.0]), [3]).tolist() == [0.0, 5.0, 0.0]                  # duplicates add
    assert tf.scatter_nd(tf.constant([[0, 1], [1, 0]]), tf.constant([[1, 2], [3, 4]]), tf.constant([2, 2, 2])).tolist() == [[[0, 0], [1, 2]], [[3, 4], [0, 0]]]
    assert not tf.stand_ins
    assert tf.scatter_nd(tf.constant([2, 0]), tf.constant([1.0, 1.0]), (4,)).tolist() == [1.0, 0.0, 1.0, 0.0] and tf.stand_ins == {"scatter_nd_rank1"}
    y, idx = tf.unique(tf.constant([1, 1, 2, 4, 4, 4, 7, 8, 8]))                          # the documented example
    assert y.tolist() == [1, 2, 4, 7, 8] and idx.tolist() == [0, 0, 1, 2, 2, 2, 3, 4, 4]
    assert tf.unique(tf.constant([5, 3, 5, 1, 3]))[0].tolist() == [5, 3, 1]              # first-occurrence order, not sorted


def test_stand_in_elementwise_reductions_and_control(tfn):
    tf = tfn.namespace()
    x = tf.constant(np.array([[1.0, 5.0, 5.0], [-2.0, -2.0, -3.0]], np.float32))
    assert tf.reduce_sum(x, 1).tolist() == [11.0, -7.0] and tf.reduce_sum(x, 1, keep_dims=True).shape == (2, 1) and float(tf.reduce_sum(x)) == 4.0
    assert tf.reduce_max(x, 0).tolist() == [1.0, 5.0, 5.0] and tf.reduce_min(x, axis=1, keep_dims=True).tolist() == [[1.0], [-3.0]] and tf.reduce_mean(x, 0).tolist() == [-0.5, 1.5, 1.0]
    assert tf.reduce_max(tf.constant(np.zeros((3, 0), np.float32)), axis=1).tolist() == [-np.inf] * 3       # the identity of max
    assert tf.argmax(x, axis=1).tolist() == [1, 0] and tf.argmin(x, 1).tolist() == [0, 2] and tf.argmax(x, 0).tolist() == [0, 0, 0]      # the lowest index among equals
    assert tf.argmax(tf.constant(np.zeros((3, 0), np.float32)), 0).shape == (0,)
    top = tf.nn.top_k(tf.constant(np.array([0.2, 0.9, 0.9, 0.1], np.float32)), k=3, sorted=True)
    assert top.indices.tolist() == [1, 2, 0] and top[1].dtype == np.int32 and top.values.tolist() == [np.float32(0.9), np.float32(0.9), np.float32(0.2)]
    assert tf.nn.top_k(tf.constant(np.zeros(0, np.float32)), k=0)[1].shape == (0,)
    assert tf.abs(x)[1].tolist() == [2, 2, 3] and tf.square(x)[0].tolist() == [1, 25, 25] and tf.sqrt(tf.square(x))[1].tolist() == [2, 2, 3]
    assert tf.div(tf.constant([7, -7]), tf.constant([2, 2])).tolist() == [3, -4] and tf.div(x, 2.0)[0].tolist() == [0.5, 2.5, 2.5]
    assert np.allclose(np.asarray(tf.log(tf.exp(x))), np.asarray(x), atol=1e-6) and tf.minimum(x, 0.0)[0].tolist() == [0, 0, 0]
    assert tf.greater_equal(x, 5.0)[0].tolist() == [False, True, True] and tf.less(x, -2.0)[1].tolist() == [False, False, True]
    assert tf.equal(x, 5)[0].tolist() == [False, True, True] and tf.not_equal(x, 5)[0].tolist() == [True, False, False]
    assert tf.logical_and(x > 0, tf.logical_not(x > 2)).tolist() == [[True, False, False], [False] * 3]
    calls = []
    assert float(tf.cond(tf.size(x) > 0, true_fn=lambda: calls.append(1) or tf.constant(1.0), false_fn=lambda: calls.append(2) or tf.constant(0.0))) == 1.0 and calls == [1]
    assert float(tf.cond(tf.size(x) > 9, lambda: tf.constant(1.0), lambda: tf.constant(0.0))) == 0.0
    rows = tf.map_fn(lambda c: tf.pad(tf.where(tf.equal(tf.constant([3, 4, 3]), c))[:, 0], [(0, 1)], constant_values=-1)[:2], tf.constant([3, 4]), dtype=tf.int64)
    assert rows.tolist() == [[0, 2], [1, -1]] and rows.dtype == np.int64
    seen = []
    res = tf.py_func(lambda a, k, thr: seen.append((type(a), a.dtype, k.dtype, thr.dtype)) or (a[:int(k)] * 2).astype(np.int32), [tf.constant([1, 2, 3]), 2, 0.1], tf.int32)
    assert res.tolist() == [2, 4] and seen == [(np.ndarray, np.dtype(np.int32), np.dtype(np.int32), np.dtype(np.float32))]
    assert tf.stop_gradient(x) is x and tf.random_shuffle(tf.range(5)).tolist() == [0, 1, 2, 3, 4] and tf.stand_ins == {"random_shuffle"}
    # the documented example's shape: the intersection of each row pair, ascending, dense with zeros behind
    a = tf.expand_dims(tf.constant(np.array([9, 1, 5, 3], np.int64)), 0)
    b = tf.expand_dims(tf.constant(np.array([3, 9, 4], np.int64)), 0)
    both = tf.sets.set_intersection(a, b)
    assert both.values.tolist() == [3, 9] and both.indices.tolist() == [[0, 0], [0, 1]] and both.dense_shape.tolist() == [1, 2]
    assert tf.sparse_tensor_to_dense(both)[0].tolist() == [3, 9] and tf.sparse_tensor_to_dense(tf.sets.set_intersection(a, a[:, :0]))[0].tolist() == []


def test_stand_in_nn_and_losses(tfn):
    for precision, tol in (("float32", 3e-7), ("float64", 1e-15)):
        tf = tfn.namespace(precision)
        logits = tf.constant(np.array([[2.0, 1.0, 0.1], [0.5, 0.5, 3.0], [-1.0, 0.0, 1.0]], np.float32))
        labels = tf.constant(np.array([0, 2, 1], np.int32))
        x64 = np.asarray(logits, np.float64)
        soft = np.exp(x64) / np.exp(x64).sum(1, keepdims=True)
        ce = -np.log(soft[np.arange(3), [0, 2, 1]])
        assert np.allclose(np.asarray(tf.nn.softmax(logits)), soft, rtol=tol, atol=0) and np.allclose(np.asarray(tf.nn.softmax(tf.expand_dims(logits, 0), 2)[0]), soft, rtol=tol, atol=0)
        got = tf.nn.sparse_softmax_cross_entropy_with_logits(labels=labels, logits=logits)
        assert got.dtype == tf.float32 and np.allclose(np.asarray(got), ce, rtol=4 * tol, atol=0)
        # the TF 1.x default reduction SUM_BY_NONZERO_WEIGHTS: the weighted sum over the NUMBER of non-zero weights
        w = np.array([2.0, 0.0, 0.5], np.float32)
        loss = tf.losses.sparse_softmax_cross_entropy(labels=labels, logits=logits, weights=tf.constant(w))
        assert np.isclose(float(loss), (ce * w).sum() / 2, rtol=4 * tol) and not np.isclose(float(loss), (ce * w).sum() / 3, rtol=1e-3) and not np.isclose(float(loss), (ce * w).sum() / 2.5, rtol=1e-3)
        assert float(tf.losses.sparse_softmax_cross_entropy(labels=labels, logits=logits, weights=tf.constant(np.zeros(3, np.float32)))) == 0.0
        # max(x, 0) - x z + log(1 + exp(-|x|)), the documented stable form: finite at large |x|
        z = tf.constant(np.array([1.0, 0.0, 1.0, 0.0], np.float32))
        big = tf.constant(np.array([200.0, 200.0, -200.0, 0.0], np.float32))
        got = tf.nn.sigmoid_cross_entropy_with_logits(labels=z, logits=big)
        assert got.dtype == tf.float32 and np.allclose(np.asarray(got), [0.0, 200.0, 200.0, np.log(2.0)], rtol=tol, atol=1e-80)


# ---- 2. the fixtures' cases ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stage", sorted(REQUIRED))
def test_every_fixture_holds_its_cases(stage):
    fx = fixture(stage)
    count = dict(zip(fx["cases"].tolist(), fx["case_counts"].tolist()))
    for name in REQUIRED[stage]:
        assert count.get(name, 0) > 0, "%s: case %s is not in the fixture" % (stage, name)
    assert fx["stand_ins"].tolist() == STAND_INS.get(stage, []), "the named stand-ins the run went through"
    assert os.path.getsize(os.path.join(GOLDEN, stage + ".npz")) <= os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "interp_ref_demo.npz"))


# ---- box_shrink ------------------------------------------------------------------------------------------------------------------------------

def test_box_shrink_restatements_equal_the_reference():
    """INTEGRATION.md claims the gamma = 1e4 form and the direct min / max agree below 5e3: both must give the reference's values"""
    fx = fixture("box_shrink")
    box, pc = t(fx["box"]), t(fx["pc"])
    assert same_values(SR.box_shrink_gamma(box, pc).numpy(), fx["out"])
    assert same_values(SR.box_shrink_direct(box, pc).numpy(), fx["out"])
    assert np.abs(fx["pc"]).max() < 5e3


# ---- spn_target_gen ----------------------------------------------------------------------------------------------------------------------------

def iou64(p, g):
    p, g = p.astype(np.float64)[:, None], g.astype(np.float64)[None]
    cube = np.maximum(np.minimum(p[..., :3] + p[..., 3:] / 2, g[..., :3] + g[..., 3:] / 2) - np.maximum(p[..., :3] - p[..., 3:] / 2, g[..., :3] - g[..., 3:] / 2), 0)
    inter = cube.prod(-1)
    return inter / (p[..., 3:].prod(-1) + g[..., 3:].prod(-1) - inter + 1e-8)


def spn_margins(prop, fg, gt_valid, gt):
    """(distance of any roi_iou_max from 0.5, lead of a ground truth's best foreground proposal over the best different one), float64"""
    m05, lead = np.inf, np.inf
    for i in range(len(prop)):
        if gt_valid[i].any():
            ious = iou64(prop[i], gt[i][gt_valid[i]])
            m05 = min(m05, np.abs(ious.max(1) - 0.5).min())
            masked = ious * fg[i][:, None]
            for j in range(masked.shape[1]):
                k = int(np.argmax(masked[:, j]))
                if masked[k, j] > 0:
                    lead = min(lead, masked[k, j] - masked[(prop[i] != prop[i][k]).any(1), j].max())
    return m05, lead


def test_spn_target_gen_restatement_equals_the_reference_and_the_margins_hold():
    fx = fixture("spn_target_gen")
    args = [t(fx[k]) for k in ("proposals", "seed_class_ids", "gt_class_ids", "gt_boxes")]
    for dtype in (torch.float32, torch.float64):
        assert same_values(SR.spn_target_gen_batch(*args, dtype=dtype)[0].numpy(), fx["spn_match"]), dtype
    m05, lead = spn_margins(fx["proposals"], fx["seed_class_ids"] == 1, fx["gt_class_ids"] > 0, fx["gt_boxes"])
    assert m05 > 1e-4 and lead > 1e-5


# ---- gather_selection ----------------------------------------------------------------------------------------------------------------------------

def test_gather_selection_on_cpu_tensors_equals_the_reference():
    from gspn_amd.rpointnet import gather_selection
    fx = fixture("gather_selection")
    got = gather_selection(t(fx["source"]), t(fx["selected_idx"]), fx["selected_idx"].shape[1])
    assert same_values(got.numpy(), fx["out"])


# ---- box_refinement, apply_box_delta -------------------------------------------------------------------------------------------------------------

def refinement_bound(box, gt_box, want):
    """|a float32 evaluation of :560-565 - the float64 run| per element.  Centre terms (g - b) / (s + 1e-8): the subtraction of two float32
    inputs rounds once (U); s + 1e-8 rounds once and holds float32(1e-8) for 1e-8 (2 U together, relative to s >= the constant); the
    division is correctly rounded on the host and within 2.5 steps = 5 U on the device (HIP's documented bound without the correctly-
    rounded switch): 8 U |d|.  Size terms log(g / (s + 1e-8)): the quotient carries 2 U + 5 U = 7 U, which the logarithm turns into an
    absolute 7 U; logf itself is within 1 step on the device (documented) and 2 are allowed: 4 U |log|.  Subnormal results: one 2^-149."""
    want = np.abs(want.astype(np.float64))
    return np.concatenate((8 * U * want[:, :3], 8 * U + 4 * U * want[:, 3:]), 1) + 2.0 ** -149


def applied_bound(box, delta_scale, want, delta_error=0.0):
    """|a float32 evaluation of :578-581 - the float64 run| per element, for deltas that themselves carry a relative error delta_error
    (0 for inputs; 2 U behind `deltas * BBOX_STD_DEV`: the constant's rounding and the product's).  Centres d s + c: the product carries
    delta_error + U, the sum rounds once (an fma rounds only once): (delta_error + U) |d s| + U |result|.  Sizes exp(d) s: expf within
    1 step on the device (documented), 2 allowed = 4 U, the product U, and exp turns the delta's error into delta_error |d|:
    (5 U + delta_error |d|) |result|.  delta_scale: |d s| for the centres, |d| for the sizes, (rows, 6) in the box's order."""
    want = np.abs(want.astype(np.float64))
    return np.concatenate(((delta_error + U) * delta_scale[:, :3] + U * want[:, :3], (5 * U + delta_error * delta_scale[:, 3:]) * want[:, 3:]), 1) + 2.0 ** -149


def delta_scale(box, delta):
    """|d s| (centres) and |d| (sizes) in the order of the box, from deltas in the reference's (dz, dy, dx, dh, dw, dl) order"""
    box, delta = box.astype(np.float64), np.abs(delta.astype(np.float64))
    return np.concatenate((delta[:, 2::-1] * box[:, 3:], delta[:, :2:-1]), 1)


def worst(got, want, bound):
    """the largest |got - want| / bound over the elements, and the largest absolute gap"""
    gap = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    return float((gap / bound).max()) if gap.size else 0.0, float(gap.max()) if gap.size else 0.0


def check_box_delta(refinement, applied, label):
    fx = fixture("box_delta")
    b1 = refinement_bound(fx["box"], fx["gt_box"], fx["refinement_float64"])
    b2 = applied_bound(fx["box"], delta_scale(fx["box"], fx["delta"]), fx["applied_float64"])
    for name, got, want, own, bound in (("box_refinement", refinement, fx["refinement_float64"], fx["refinement_float32"], b1),
                                        ("apply_box_delta", applied, fx["applied_float64"], fx["applied_float32"], b2)):
        ratio, gap = worst(got, want, bound)
        print("%s %s: worst gap from the float64 run %.3g = %.3f of the bound; the float32 run of the reference's lines: %.3g = %.3f of it"
              % (label, name, gap, ratio, worst(own, want, bound)[1], worst(own, want, bound)[0]))
        assert ratio <= 1.0 and worst(own, want, bound)[0] <= 1.0, name


def test_box_delta_restatements_within_the_derived_bound():
    fx = fixture("box_delta")
    box, gt_box, delta = t(fx["box"]), t(fx["gt_box"]), t(fx["delta"])
    check_box_delta(RR.box_refinement(box, gt_box).numpy(), RR.apply_box_delta(box, delta).numpy(), "roi_ref")
    assert np.allclose(RR.box_refinement(box.double(), gt_box.double()).numpy(), fx["refinement_float64"], rtol=1e-13, atol=1e-300)
    assert np.allclose(RR.apply_box_delta(box.double(), delta.double()).numpy(), fx["applied_float64"], rtol=1e-13, atol=1e-300)
    from gspn_amd import roi                                                             # plain torch: the product's own lines on CPU tensors
    check_box_delta(roi.box_refinement(box, gt_box).numpy(), roi.apply_box_delta(box, delta).numpy(), "roi (cpu tensors)")


# ---- detection_target_gen ----------------------------------------------------------------------------------------------------------------------

def target_args():
    rois, ratio, mask_points = fixture("detection_target")["args"]
    return int(rois), float(ratio), int(mask_points)


def target_scenes():
    fx = fixture("detection_target")
    keys = ("proposals", "gt_class_ids", "gt_boxes", "group_label", "pc")
    return [np.stack([fx["s%d/%s" % (i, k)] for i in range(2)]) for k in keys]


def check_detection_targets(roi_src, roi_gt, rois, class_ids, bbox, idx, mask, label):
    """What any draw of detection_target_gen must satisfy, scene by scene, against the tables of the reference's lines: the chosen source
    rows are survivors of trim_zeros and the non-empty filter; rows reported positive are the tables' positives with their assignment and
    class; the counts are the :700-707 table's pair for the scene's number of positives, capped by what exists; positives, then
    negatives, then zero rows; every positive's deltas within refinement_bound (over BBOX_STD_DEV: one more division, 5 U) of the float64
    row; every mask value is masks_full[row, idx]; every index lies inside the row's roi_masks column; negatives and padding carry zeros."""
    fx = fixture("detection_target")
    r, _, _ = target_args()
    std = np.array((0.1, 0.1, 0.1, 0.2, 0.2, 0.2))
    for i in range(2):
        pre = "s%d/" % i
        survivors, positive = fx[pre + "survivors"], fx[pre + "positive"]
        n = fx[pre + "pc"].shape[0]
        masks_full, roi_masks = unpack(fx[pre + "masks_full"], n), unpack(fx[pre + "roi_masks"], n)
        want_pos, want_neg = fx["count_table"][min(int(positive.sum()), r)]
        want_neg = min(int(want_neg), int((~positive).sum()), r - int(want_pos))
        src, gt = np.asarray(roi_src[i]), np.asarray(roi_gt[i])
        npos, nrows = int((gt >= 0).sum()), int((src >= 0).sum())
        assert (npos, nrows - npos) == (int(want_pos), want_neg), "%s scene %d: %d positives and %d negatives, the table says %d and %d" % (
            label, i, npos, nrows - npos, want_pos, want_neg)
        assert (gt[:npos] >= 0).all() and (src[:nrows] >= 0).all() and (src[nrows:] == -1).all() and (gt[npos:] == -1).all(), "positives, negatives, padding"
        assert len(np.unique(src[:nrows])) == nrows and np.isin(src[:nrows], survivors).all(), "distinct survivors"
        at = np.searchsorted(survivors, src[:nrows])                                     # the table row of each chosen proposal
        assert positive[at[:npos]].all() and not positive[at[npos:]].any()
        assert np.array_equal(gt[:npos], fx[pre + "assignment"][at[:npos]]) and np.array_equal(np.asarray(class_ids[i])[:npos], fx[pre + "class_ids"][at[:npos]])
        assert same_values(np.asarray(rois[i])[:nrows], fx[pre + "proposals"][src[:nrows]])
        want = fx[pre + "deltas_float64"][at[:npos]]
        bound = (refinement_bound(None, None, want * std) + 5 * U * np.abs(want * std)) / std
        ratio, gap = worst(np.asarray(bbox[i])[:npos], want, bound)
        own = worst(fx[pre + "deltas_float32"][at[:npos]], want, bound)
        print("%s scene %d: %d positives, %d negatives; deltas %.3g from the float64 rows = %.3f of the bound (the float32 run of the reference's lines: %.3g = %.3f)"
              % (label, i, npos, nrows - npos, gap, ratio, own[1], own[0]))
        assert ratio <= 1.0 and own[0] <= 1.0
        ix, mk = np.asarray(idx[i]).astype(np.int64), np.asarray(mask[i]).astype(bool)
        for k in range(npos):
            assert roi_masks[at[k]][ix[k]].all(), "a sampled point outside its ROI"
            assert np.array_equal(mk[k], masks_full[at[k]][ix[k]])
        assert not np.asarray(class_ids[i])[npos:].any() and not np.asarray(bbox[i])[npos:].any() and not mk[npos:].any() and not ix[npos:].any()
        assert not np.asarray(rois[i])[nrows:].any()


def test_detection_target_restatement_against_the_tables():
    fx = fixture("detection_target")
    r, ratio, p = target_args()
    prop, cls, boxes, label, pc = [t(a) for a in target_scenes()]
    count = RR.box_point_count(prop, pc)
    for seed in (0, 1, 2):
        roi_src, roi_gt, _ = RR.detection_target_select(prop, count, boxes, r, ratio, seed)
        idx = RR.sample_points_in_boxes(RR.take_rows(prop, torch.where(roi_gt >= 0, roi_src, -torch.ones_like(roi_src))), pc, p, seed)
        rois, ids, bbox, mask = RR.detection_targets(prop, cls, boxes, label, pc, roi_src, roi_gt, idx, (0.1, 0.1, 0.1, 0.2, 0.2, 0.2))
        check_detection_targets(roi_src.numpy(), roi_gt.numpy(), rois.numpy(), ids.numpy(), bbox.numpy(), idx.numpy(), mask.numpy(), "roi_ref seed %d" % seed)
    for positives in range(r + 1):                                                       # the reference's own arithmetic of :700-707, number by number
        assert RR.selection_counts(positives, 4 * r, r, ratio) == tuple(fx["count_table"][positives])
    cap = int(r * ratio)
    assert fx["count_table"][:, 0].tolist() == [min(k, cap) for k in range(r + 1)]


def test_detection_target_conditions_hold():
    fx = fixture("detection_target")
    for i in range(2):
        pre = "s%d/" % i
        prop, boxes, survivors = fx[pre + "proposals"], fx[pre + "gt_boxes"], fx[pre + "survivors"]
        valid = np.abs(boxes).sum(1) > 0
        assert np.isin(survivors, np.nonzero(np.abs(prop).sum(1))[0]).all()
        if valid.any():
            ious = iou64(prop[survivors], boxes[valid])
            assert np.abs(ious.max(1) - 0.5).min() > 1e-4
            assert np.array_equal(ious.max(1) >= 0.5, fx[pre + "positive"])
            top2 = np.sort(ious[fx[pre + "positive"]], 1)[:, -2:]
            assert (top2[:, 1] - top2[:, 0]).min() > 1e-5
            assert np.array_equal(np.nonzero(valid)[0][ious.argmax(1)][fx[pre + "positive"]], fx[pre + "assignment"][fx[pre + "positive"]])
        else:
            assert not fx[pre + "positive"].any()
    assert int(fx["count_table_float64_differs"]) == 0       # at 64 ROIs and ratio 0.33 no number of positives tells float32 from float64 in r * P


# ---- mask_selection_gen ------------------------------------------------------------------------------------------------------------------------

def check_mask_selection(rois, idx, i, removal, label):
    """the proposals exact, padding included (the reference returns more rows than num_rois when more are kept: the first num_rois);
    every index inside its ROI's stored mask; the rows of an empty ROI and of the padding all zero"""
    fx = fixture("mask_selection")
    num_rois = int(fx["args"][0])
    key = "s%d/removal_%d/" % (i, removal)
    n = fx["s%d/pc" % i].shape[0]
    assert same_values(np.asarray(rois), fx[key + "proposals"][:num_rois]), label
    masks = unpack(fx[key + "roi_masks"], n)[:num_rois]
    ix = np.asarray(idx).astype(np.int64)
    for k in range(num_rois):
        if k < len(masks) and masks[k].any():
            assert masks[k][ix[k]].all(), "%s: a sampled point outside ROI %d" % (label, k)
        else:
            assert not ix[k].any(), "%s: row %d has no point to draw from" % (label, k)


def test_mask_selection_restatement_equals_the_reference_and_the_margin_holds():
    fx = fixture("mask_selection")
    num_rois, p = int(fx["args"][0]), int(fx["args"][1])
    for i in range(2):
        prop, pc = fx["s%d/proposals" % i], fx["s%d/pc" % i]
        for removal in (True, False):
            key = "s%d/removal_%d/" % (i, removal)
            rows = RR.mask_selection_rows(t(prop)[None], t(pc)[None], num_rois, removal)[0].numpy()
            want = fx[key + "rows"][:num_rois]
            assert np.array_equal(rows[:len(want)], want) and (rows[len(want):] == -1).all()
            rois = RR.take_rows(t(prop)[None], t(rows)[None])
            check_mask_selection(rois[0].numpy(), RR.sample_points_in_boxes(rois, t(pc)[None], p, 3, 1e-3)[0].numpy(), i, removal, "roi_ref")
        live = prop[np.abs(prop).sum(1) > 0].astype(np.float64)
        lo, hi = live[:, None, :3] - live[:, None, 3:] / 2 - 1e-3, live[:, None, :3] + live[:, None, 3:] / 2 + 1e-3
        q = pc.astype(np.float64)[None]
        near = (q >= lo - 1e-3) & (q <= hi + 1e-3)
        dist = np.minimum(np.abs(q - lo), np.abs(q - hi))
        for axis in range(3):
            decides = near[..., (axis + 1) % 3] & near[..., (axis + 2) % 3]
            assert dist[..., axis][decides].min() > 1e-5


# ---- points_cropping ----------------------------------------------------------------------------------------------------------------------------

def check_points_cropping(crop, label):
    fx = fixture("points_cropping")
    for normalize in (True, False):
        got = crop(normalize)
        for name, a in zip(("fea", "center", "coord", "raw"), got):
            assert same_values(np.asarray(a), fx["%s_normalize_%d" % (name, normalize)]), "%s %s normalize %s" % (label, name, normalize)


def test_points_cropping_restatement_equals_the_reference():
    fx = fixture("points_cropping")
    args = [t(fx[k]) for k in ("pc", "pc_fea", "pc_center", "rois", "idx")]
    check_points_cropping(lambda normalize: [a.numpy() for a in RR.points_cropping(*args, normalize_crop_region=normalize)], "roi_ref")
    total = fx["rois"].astype(np.float64).sum(-1)
    assert (np.abs(total[total != 0]) > 0.5).all() and ((total == 0) & fx["rois"].any(-1)).sum() == 1


# ---- refine_detections ----------------------------------------------------------------------------------------------------------------------------

class DetectConfig(object):
    BBOX_STD_DEV = (0.1, 0.1, 0.1, 0.2, 0.2, 0.2)

    def __init__(self, shrink):
        fx = fixture("refine_detections")
        self.SHRINK_BOX = shrink
        self.DETECTION_MIN_CONFIDENCE, self.DETECTION_NMS_THRESHOLD, self.DETECTION_MAX_INSTANCES = float(fx["args"][0]), float(fx["args"][1]), int(fx["args"][2])


def refined_bound(shrink):
    """(B, R, 6): the bound of a float32 evaluation of :841 against the float64 boxes: applied_bound with a 2 U error in the deltas.  With
    SHRINK_BOX the boxes are built from the points inside: exact (the condition below keeps every point 1e-5 clear of the faces)."""
    fx = fixture("refine_detections")
    probs, want = fx["probs"], fx["refined_shrink_%d_float64" % shrink]
    if shrink:
        return np.zeros(want.shape)
    cls = probs.argmax(-1)
    specific = np.take_along_axis(fx["deltas"], cls[..., None, None], 2)[:, :, 0].astype(np.float64) * np.array(DetectConfig.BBOX_STD_DEV)
    return np.stack([applied_bound(fx["rois"][i], delta_scale(fx["rois"][i], specific[i]), want[i], 2 * U) for i in range(len(probs))])


def check_refine_detections(refined, detections, shrink, label):
    """refined (B, R, 6): every ROI's box; detections (B, M, 8).  The rows the reference's lines select, in their order, with their class
    ids and class scores: exact.  The boxes: within refined_bound of the float64 run without SHRINK_BOX; with it, the float32 run's."""
    fx = fixture("refine_detections")
    rows, want32, want64 = fx["rows_shrink_%d" % shrink], fx["detections_shrink_%d_float32" % shrink], fx["detections_shrink_%d_float64" % shrink]
    refined, detections = np.asarray(refined), np.asarray(detections)
    assert detections.dtype == np.float32 and same_values(detections[..., 6:], want32[..., 6:]), "%s: class ids and scores of the selected rows" % label
    for i in range(len(rows)):
        live = rows[i] >= 0
        assert same_values(detections[i][live][:, :6], refined[i][rows[i][live]]) and not detections[i][~live].any(), "%s: the rows selected" % label
    if shrink:
        assert same_values(detections[..., :6], want32[..., :6]), "%s: shrunk boxes are the reference's float32 boxes" % label
        assert np.array_equal(refined.any(-1), fx["refined_shrink_1_float64"].any(-1)), "%s: the same boxes shrink to nothing" % label
        return
    bound = refined_bound(False)
    ratio, gap = worst(refined, fx["refined_shrink_0_float64"], bound + 2.0 ** -149)
    own = [worst(want32[i][rows[i] >= 0][:, :6], want64[i][rows[i] >= 0][:, :6], bound[i][rows[i][rows[i] >= 0]] + 2.0 ** -149) for i in range(len(rows))]
    print("%s: refined boxes %.3g from the float64 run = %.3f of the bound (the float32 run of the reference's lines, detections only: %.3g = %.3f)"
          % (label, gap, ratio, max(o[1] for o in own), max(o[0] for o in own)))
    assert ratio <= 1.0 and max(o[0] for o in own) <= 1.0


def restated_detections(probs, shrink):
    fx = fixture("refine_detections")
    cfg = DetectConfig(shrink)
    rois, probs, deltas, pc = t(fx["rois"]), t(probs), t(fx["deltas"]), t(fx["pc"])
    ids, scores = DR.first_argmax(probs)
    specific = torch.gather(deltas, 2, ids.long().reshape(ids.shape + (1, 1)).expand(ids.shape + (1, 6))).squeeze(2) * torch.tensor(cfg.BBOX_STD_DEV)
    refined = torch.stack([RR.apply_box_delta(rois[i], specific[i]) for i in range(len(rois))])
    if shrink:
        refined = SR.box_shrink_direct(refined, pc)
    det = DR.refine_detections(refined, ids, scores, t(fx["fb_prob"]), t(fx["sem_prob"]), cfg.DETECTION_MIN_CONFIDENCE, cfg.DETECTION_MAX_INSTANCES, cfg.DETECTION_NMS_THRESHOLD)
    return refined.numpy(), det.numpy()


@pytest.mark.parametrize("shrink", [False, True])
def test_refine_detections_restatement_equals_the_reference(shrink):
    fx = fixture("refine_detections")
    check_refine_detections(*restated_detections(fx["probs"], shrink), shrink=shrink, label="detect_ref SHRINK_BOX %s" % shrink)
    if not shrink:
        _, det = restated_detections(fx["probs_no_candidate"], False)
        assert same_values(det[..., 6:], fx["detections_no_candidate"][..., 6:]) and not det[1].any()
        assert np.abs(det[0] - fx["detections_no_candidate"][0]).max() <= refined_bound(False).max() * 2


def test_refine_detections_conditions_hold():
    fx = fixture("refine_detections")
    probs, min_conf, thr = fx["probs"], float(fx["args"][0]), float(fx["args"][1])
    cls, score = probs.argmax(-1), probs.max(-1)
    composite = score.astype(np.float64) * fx["fb_prob"] * fx["sem_prob"]
    composite32 = (score * fx["fb_prob"]) * fx["sem_prob"]
    for i in range(len(probs)):
        assert len(np.unique(composite[i])) == composite.shape[1] and len(np.unique(composite32[i])) == composite.shape[1]
        assert np.abs(score[i].astype(np.float64) - min_conf).min() > 1e-4
        cand = (cls[i] > 0) & (score[i] >= min_conf)
        for shrink in (0, 1):
            boxes = fx["refined_shrink_%d_float64" % shrink][i][cand]
            ious = iou64(boxes, boxes)
            same = (cls[i][cand][:, None] == cls[i][cand][None]) & ~np.eye(len(boxes), dtype=bool)
            assert np.abs(ious[same] - thr).min() > 1e-4
        # SHRINK_BOX: no point within 1e-5 of a face of a refined (not yet shrunk) box, among the points the other axes leave inside
        boxes, q = fx["refined_shrink_0_float64"][i][:, None], fx["pc"][i].astype(np.float64)[None]
        lo, hi = boxes[..., :3] - boxes[..., 3:] / 2, boxes[..., :3] + boxes[..., 3:] / 2
        near = (q >= lo - 1e-3) & (q <= hi + 1e-3)
        dist = np.minimum(np.abs(q - lo), np.abs(q - hi))
        for axis in range(3):
            assert dist[..., axis][near[..., (axis + 1) % 3] & near[..., (axis + 2) % 3]].min() > 1e-5


# ---- select_segmentation, unmold_segmentation ----------------------------------------------------------------------------------------------------

def test_segmentation_restatements_equal_the_reference():
    fx = fixture("segmentation")
    masks, rois, class_ids, crops, pc = [t(fx[k]) for k in ("masks", "rois", "class_ids", "crops", "pc")]
    assert same_values(DR.select_segmentation(masks, class_ids).numpy(), fx["selected"])
    assert same_values(DR.unmold_segmentation(masks, rois, class_ids, crops, pc).numpy(), fx["unmolded"])
    from gspn_amd.detect import select_segmentation                                      # plain torch: the product's own lines on CPU tensors
    assert same_values(select_segmentation(masks, class_ids).numpy(), fx["selected"])
    for a in (fx["pc"], fx["crops"], fx["rois"] * 0.5):                                   # the raster that makes every squared distance exact
        assert np.array_equal(a * 16, np.round(a * 16)) and np.abs(a).max() < 16


# ---- the losses ------------------------------------------------------------------------------------------------------------------------------------

LOSS_KINDS = ("mixed", "no_foreground", "no_valid_roi")


def cross_entropy_bound(value, terms, classes, largest_logit):
    """|a float32 evaluation - the float64 run| of a (weighted) mean of `terms` softmax cross-entropies.  One term logsumexp(x) - x_label:
    `classes` exponentials within 2 steps each (4 U), summed (classes U), a logarithm (absolute 5 U + classes U, and its own 4 U), the
    shift by the maximum and the final subtraction (2 roundings at the size of the logits): an absolute (2 classes + 13) U (1 + largest
    |logit| + ln classes) per term, and the weighted mean of errors is no more than that since the weights over the divisor sum to at most
    about 1 here (asserted by the callers' cases).  The sum of `terms` products then rounds terms + 1 times and the division once, relative
    to the value (all terms are >= 0): (terms + 3) U value."""
    return (2 * classes + 13) * U * (1 + largest_logit + np.log(classes)) + (terms + 3) * U * abs(float(value))


def loss_bounds(kind):
    """name -> bound for the three R-PointNet losses of one input set"""
    fx = fixture("losses")
    cls, valid = fx[kind + "/target_class_ids"], fx[kind + "/roi_valid_mask"]
    sel = int(((valid > 0) & (cls > 0)).sum())
    k, p = fx[kind + "/rpointnet_class_logits"].shape[-1], fx[kind + "/rpointnet_mask"].shape[2]
    want = {name: float(fx["%s/%s_float64" % (kind, name)]) for name in ("class_loss", "bbox_loss", "mask_loss")}
    # smooth-L1 of one element: |a - b| (U), then 0.5 d d or d - 0.5 (3 U): 4 U relative; 6 sel of them summed and divided: (6 sel + 2) U
    # sigmoid cross-entropy of one element max(x, 0) - x z + log1p(exp(-|x|)): expf and log1pf 4 U each on values <= ln 2, two sums at the
    # size of |x| + ln 2: an absolute 10 U (1 + |x|); sel p of them summed and divided: (sel p + 2) U relative
    return {"class_loss": cross_entropy_bound(want["class_loss"], cls.size, k, float(np.abs(fx[kind + "/rpointnet_class_logits"]).max())),
            "bbox_loss": (4 + 6 * sel + 2) * U * want["bbox_loss"],
            "mask_loss": 10 * U * (1 + float(np.abs(fx[kind + "/rpointnet_mask"]).max())) + (sel * p + 2) * U * want["mask_loss"]}, want


def check_losses(smooth_l1, spn_class_loss, class_loss, bbox_loss, mask_loss, label, convert=t):
    fx = fixture("losses")
    got = np.asarray(smooth_l1(convert(fx["y_true"]), convert(fx["y_pred"])))
    want = fx["smooth_l1_float64"]
    bound = 4 * U * np.abs(want) + 2.0 ** -149                                            # |a - b|, its square or the shift, the halving: see loss_bounds
    print("%s smooth_l1: %.3f of the bound (the float32 run of the reference's lines: %.3f)" % (label, worst(got, want, bound)[0], worst(fx["smooth_l1_float32"], want, bound)[0]))
    assert worst(got, want, bound)[0] <= 1.0 and worst(fx["smooth_l1_float32"], want, bound)[0] <= 1.0
    assert got[0] == 0.5 and got[3] == 0.5, "|diff| exactly 1: both branches meet at 0.5"
    logits, match = fx["fb_logits"], fx["spn_match"]
    want = float(fx["spn_class_loss_float64"])
    bound = cross_entropy_bound(want, int((match != 0).sum()), 2, float(np.abs(logits).max()))
    got = float(spn_class_loss(convert(logits), convert(match)))
    print("%s spn_class_loss: %.3g from the float64 run = %.3f of the bound (the float32 run: %.3f)" % (
        label, abs(got - want), abs(got - want) / bound, abs(float(fx["spn_class_loss_float32"]) - want) / bound))
    assert abs(got - want) <= bound and abs(float(fx["spn_class_loss_float32"]) - want) <= bound
    assert float(spn_class_loss(convert(logits), convert(fx["spn_match_neutral"]))) == 0.0 == float(fx["spn_class_loss_neutral_float32"])
    for kind in LOSS_KINDS:
        e = {k: fx["%s/%s" % (kind, k)] for k in ("roi_valid_mask", "target_class_ids", "target_bbox", "rpointnet_class_logits", "rpointnet_bbox", "rpointnet_mask")}
        k, p = e["rpointnet_class_logits"].shape[-1], e["rpointnet_mask"].shape[2]
        e["target_mask"] = unpack(fx[kind + "/target_mask"], p)
        e = {key: convert(a) for key, a in e.items()}
        res = {"class_loss": class_loss(e["rpointnet_class_logits"], e["target_class_ids"], e["roi_valid_mask"]),
               "bbox_loss": bbox_loss(e["target_bbox"], e["target_class_ids"], e["rpointnet_bbox"], e["roi_valid_mask"], k),
               "mask_loss": mask_loss(e["target_mask"], e["target_class_ids"], e["rpointnet_mask"], e["roi_valid_mask"], k, p)}
        bounds, want = loss_bounds(kind)
        for name in res:
            gap, own = abs(float(res[name]) - want[name]), abs(float(fx["%s/%s_float32" % (kind, name)]) - want[name])
            print("%s %s %s: %.6g, %.3g from the float64 run (bound %.3g; the float32 run of the reference's lines: %.3g)" % (label, kind, name, float(res[name]), gap, bounds[name], own))
            assert gap <= bounds[name] and own <= bounds[name], (kind, name)
            if want[name] == 0:
                assert float(res[name]) == 0.0


def test_losses_on_cpu_tensors_and_restatements_against_the_float64_run():
    from gspn_amd import heads, rpointnet
    check_losses(rpointnet.smooth_l1_loss, rpointnet.get_spn_class_loss, heads.get_rpointnet_class_loss, heads.get_rpointnet_bbox_loss,
                 heads.get_rpointnet_mask_loss, "product (cpu tensors)")
    # the float64 restatements against the float64 run of the reference's lines: the same number to the last few bits
    fx = fixture("losses")
    assert np.allclose(HR.smooth_l1(t(fx["y_true"]).double(), t(fx["y_pred"]).double())[0].numpy(), fx["smooth_l1_float64"], rtol=1e-14, atol=0)
    assert np.allclose(SR._smooth_l1(t(fx["y_true"]).double(), t(fx["y_pred"]).double())[0].numpy(), fx["smooth_l1_float64"], rtol=1e-14, atol=0)
    for kind in LOSS_KINDS:
        valid, cls = t(fx[kind + "/roi_valid_mask"]).double(), t(fx[kind + "/target_class_ids"])
        k, p = fx[kind + "/rpointnet_class_logits"].shape[-1], fx[kind + "/rpointnet_mask"].shape[2]
        got = (HR.class_loss(t(fx[kind + "/rpointnet_class_logits"]).double(), cls, valid),
               HR.bbox_loss(t(fx[kind + "/target_bbox"]).double(), cls, t(fx[kind + "/rpointnet_bbox"]).double(), valid, k)[0],
               HR.mask_loss(t(unpack(fx[kind + "/target_mask"], p)), cls, t(fx[kind + "/rpointnet_mask"]).double(), valid, k, p))
        for name, value in zip(("class_loss", "bbox_loss", "mask_loss"), got):
            assert np.isclose(float(value), float(fx["%s/%s_float64" % (kind, name)]), rtol=1e-13, atol=0), (kind, name)


# ---- get_loss, SPN mode ------------------------------------------------------------------------------------------------------------------------------

LOSS_TERMS = ("spn_class_loss", "recons_loss", "shift_loss", "sem_loss", "kl_loss", "loss")


def get_loss_bounds():
    """term -> bound of a float32 evaluation of :1328-1381, :1395 against the float64 run, from the stored inputs.  With n the number of
    seeds B nsmp and every masked mean over them costing (n + 3) U relative to its (non-negative) summands:
      spn_class_loss, sem_loss   cross_entropy_bound (the semantic weights over the number of non-zero weights sum to `wsum`, at most 2 here)
      shift_loss                 radius = 1e-8 + sqrt(sum (size / 2)^2) and shift_dist carry 6 U each, the quotients 5 U more, smooth-L1 4 U
                                 more on an argument whose error the Lipschitz constant 1 passes on: 16 U (|gt4| + |pred4|) per element, summed
      recons_loss                normalised coordinates carry 12 U; a squared distance (a - b)^2 summed over 3 axes 2 (12 U) (|a| + |b|) |a - b|
                                 + 5 U d^2 <= 64 U R^2 with R the largest normalised norm; min is 1-Lipschitz: the mean keeps that bound
      kl_loss                    per latent element log_var - clog_var + (exp(clog_var) + (mean - cmean)^2) / exp(log_var) - 1: every operation
                                 within 5 U of its own result: 12 U of the sum of the absolute values of the parts (`kl_abs`), then the means
      loss                       the sum of the five bounds (alpha times the KL one) plus 5 roundings of the total"""
    fx = fixture("get_loss")
    e = {k[len("end_points/"):]: fx[k].astype(np.float64) if fx[k].dtype == np.float32 else fx[k] for k in fx if k.startswith("end_points/")}
    want = {k: float(fx[k + "_float64"]) for k in LOSS_TERMS}
    n = e["pc_seed"].shape[0] * e["pc_seed"].shape[1]
    fg = (np.take_along_axis(e["seg_label"], e["ind_seed"].astype(np.int64), 1) > 0).astype(np.float64)
    denom = fg.sum() + 1e-8
    size = e["pc_ins_centered_seed"].max(2, keepdims=True) - e["pc_ins_centered_seed"].min(2, keepdims=True)
    radius = 1e-8 + np.sqrt(((size / 2) ** 2).sum(-1, keepdims=True))
    shift = e["pc_ins_center_seed"] - e["pc_seed"][:, :, None]
    dist = np.sqrt((shift ** 2).sum(-1, keepdims=True) + 1e-8)
    gt4 = np.concatenate((shift / dist, dist / radius), -1)
    sp = e["shift_pred_seed_4d"][:, :, None]
    pred4 = np.concatenate((sp[..., :3], sp[..., 3:] / radius), -1)
    big = max(float(np.abs(e["pc_ins_pred"] / radius).max()), float(np.abs((e["pc_ins_centered_seed"] + shift) / radius).max())) * np.sqrt(3.0)
    kl_abs = 0.5 * (np.abs(e["log_var"]) + np.abs(e["clog_var"]) + (np.exp(e["clog_var"]) + (e["mean"] - e["cmean"]) ** 2) / np.exp(e["log_var"]) + 1.0).mean(2)
    w = np.take_along_axis(fx["smpw"].astype(np.float64), e["ind_sem"].astype(np.int64), 1)
    wsum = w.sum() / max((w != 0).sum(), 1)
    assert wsum <= 2.0
    k = e["sem_class_logits"].shape[-1]
    b = {"spn_class_loss": cross_entropy_bound(want["spn_class_loss"], n, 2, float(np.abs(e["fb_logits"]).max())),
         "sem_loss": 2.0 * cross_entropy_bound(want["sem_loss"], w.size, k, float(np.abs(e["sem_class_logits"]).max())),
         "shift_loss": 16 * U * float(((np.abs(gt4) + np.abs(pred4)).sum(-1).reshape(-1) * fg.reshape(-1)).sum() / denom) + (n + 3) * U * want["shift_loss"],
         "recons_loss": 2 * 64 * U * big * big + (n + 3) * U * want["recons_loss"],
         "kl_loss": (12 + e["mean"].shape[2] + n + 3) * U * float((kl_abs.reshape(-1) * fg.reshape(-1)).sum() / denom)}
    alpha = float(fx["alpha"])
    b["loss"] = alpha * b["kl_loss"] + b["spn_class_loss"] + b["sem_loss"] + b["shift_loss"] + b["recons_loss"] + 5 * U * want["loss"]
    return b, want


def check_get_loss(end_points, label):
    fx = fixture("get_loss")
    bounds, want = get_loss_bounds()
    assert same_values(np.asarray(end_points["spn_match"]).astype(np.int32), fx["spn_match"]) and same_values(np.asarray(end_points["sem_labels"]).astype(np.int32), fx["sem_labels"])
    for name in LOSS_TERMS:
        gap, own = abs(float(end_points[name]) - want[name]), abs(float(fx[name + "_float32"]) - want[name])
        print("%s %s: %.7g, %.3g from the float64 run (bound %.3g; the float32 run of the reference's lines: %.3g)" % (label, name, float(end_points[name]), gap, bounds[name], own))
        assert gap <= bounds[name] and own <= bounds[name], name


def get_loss_inputs(convert=t):
    fx = fixture("get_loss")
    return {k[len("end_points/"):]: convert(fx[k]) for k in fx if k.startswith("end_points/")}, convert(fx["smpw"]), float(fx["alpha"])


def test_get_loss_restatement_against_the_float64_run():
    fx = fixture("get_loss")
    ep, smpw, alpha = get_loss_inputs()
    ep = {k: (v.double().requires_grad_(k in SR.LOSS_GRAD_KEYS) if v.dtype == torch.float32 else v) for k, v in ep.items()}
    fg = (torch.gather(ep["seg_label"], 1, ep["ind_seed"].long()) > 0).float()
    match = SR.spn_target_gen_batch(ep["bbox_ins_pred"].detach(), fg, (ep["seg_label_per_group"] > 0).float(), ep["bbox_ins"])[0]
    assert same_values(match.numpy(), fx["spn_match"])
    res = SR.get_loss_ref(ep, alpha, smpw.double(), t(fx["spn_match"]))
    assert same_values(res["sem_labels"].numpy(), fx["sem_labels"])
    for name in LOSS_TERMS:
        assert np.isclose(float(res[name].detach()), float(fx[name + "_float64"]), rtol=1e-12, atol=0), name
    m05, lead = spn_margins(fx["end_points/bbox_ins_pred"], fg.numpy() == 1, fx["end_points/seg_label_per_group"] > 0, fx["end_points/bbox_ins"])
    assert m05 > 1e-4 and lead > 1e-5
    bounds, want = get_loss_bounds()
    for name in LOSS_TERMS:
        assert abs(float(fx[name + "_float32"]) - want[name]) <= bounds[name], name
