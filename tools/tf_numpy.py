"""A numpy stand-in for the TensorFlow 1.x ops that the graph code of models/model_rpointnet.py calls, so that tools/make_golden_graph.py
can exec the reference's own lines where TensorFlow is not installed.  Written from TensorFlow 1.x's documented op semantics (the API
pages of each op), one function per op; nothing of the reference is in here.

    tf = namespace()                 # tf.float32 is float32: the reference's arithmetic
    tf = namespace("float64")        # tf.float32 and cast(.., tf.float32) mean float64: the same lines give the high-precision answer

What a graph hands around is a Tensor, an ndarray subclass with get_shape() / set_shape().  The dtype rules of TensorFlow that numpy does
not share are kept by Tensor.__array_ufunc__: an operand that is not a Tensor (a Python number, a numpy array such as a config constant)
is converted to the Tensor operand's dtype, as tf.convert_to_tensor does with a dtype hint, so it never widens; two Tensors of different
dtypes raise, as in TensorFlow.  where(cond) and argmax give int64 unless output_type says otherwise; argmax, argmin and top_k take the
lowest index among equal values; unique keeps first-occurrence order; set_intersection gives ascending values.

Two ops are NAMED STAND-INS, not semantics; namespace().stand_ins records which of them a run used:
    random_shuffle   the identity (the draws are pinned as tables, not as sequences)
    scatter_nd_rank1 scatter_nd with a rank-1 index into a rank-1 shape is read as an index with a trailing axis of 1 (by the documented
                     rule a rank-1 index is ONE index tuple; INTEGRATION.md "One deviation" states the evident intent)."""
import collections

import numpy as np

__all__ = ["namespace", "Tensor", "SparseTensor"]


class Dimension(object):
    def __init__(self, value):
        self.value = None if value is None else int(value)

    def __int__(self):
        return self.value

    __index__ = __int__

    def __eq__(self, other):
        return self.value == (other.value if isinstance(other, Dimension) else other)

    def __hash__(self):
        return hash(self.value)


class TensorShape(object):
    def __init__(self, dims):
        self.dims = [Dimension(d) for d in dims]

    def __getitem__(self, k):
        return self.dims[k]

    def __len__(self):
        return len(self.dims)

    def __iter__(self):
        return iter(self.dims)

    def as_list(self):
        return [d.value for d in self.dims]

    @property
    def ndims(self):
        return len(self.dims)


_COMPARISONS = (np.greater, np.greater_equal, np.less, np.less_equal, np.equal, np.not_equal)


class Tensor(np.ndarray):
    """an ndarray that follows TensorFlow's dtype rules in arithmetic (see the module's docstring)"""

    def get_shape(self):
        return TensorShape(self.shape)

    def set_shape(self, shape):
        shape = [None if d is None else int(d) for d in shape]
        if len(shape) != self.ndim or any(d is not None and d != s for d, s in zip(shape, self.shape)):
            raise ValueError("set_shape: %s is not compatible with %s" % (shape, self.shape))

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        if method != "__call__":
            raise TypeError("Tensor: ufunc method %s has no TensorFlow meaning here" % method)
        dtypes = {np.asarray(x).dtype for x in inputs if isinstance(x, Tensor)}
        if len(dtypes) != 1:
            raise TypeError("%s: operands of different dtypes %s (TensorFlow does not convert between tensors)" % (ufunc.__name__, sorted(map(str, dtypes))))
        dtype = dtypes.pop()
        plain = []
        for x in inputs:
            if isinstance(x, Tensor):
                plain.append(x.view(np.ndarray))
            else:
                a = np.asarray(x)
                if dtype.kind in "iu" and a.dtype.kind == "f":
                    raise TypeError("%s: a float operand for a tensor of %s" % (ufunc.__name__, dtype))
                if dtype.kind == "b" and a.dtype.kind != "b":
                    raise TypeError("%s: a %s operand for a bool tensor" % (ufunc.__name__, a.dtype))
                plain.append(a.astype(dtype))
        out = kwargs.pop("out", None)
        if out is not None:
            kwargs["out"] = tuple(o.view(np.ndarray) if isinstance(o, Tensor) else o for o in out)
        if ufunc is np.true_divide and dtype.kind in "iu":
            raise TypeError("true_divide of integer tensors is not used by the lines this stands in for")
        res = getattr(ufunc, method)(*plain, **kwargs)
        if ufunc not in _COMPARISONS and ufunc not in (np.logical_and, np.logical_or, np.logical_not, np.isnan, np.isfinite):
            assert res.dtype == dtype, (ufunc.__name__, res.dtype, dtype)
        return np.asarray(res).view(Tensor)


class SparseTensor(object):
    def __init__(self, indices, values, dense_shape):
        self.indices, self.values, self.dense_shape = indices, values, dense_shape


TopK = collections.namedtuple("TopK", ["values", "indices"])
Unique = collections.namedtuple("Unique", ["y", "idx"])


def _t(a, dtype=None):
    return np.ascontiguousarray(np.asarray(a, dtype=dtype)).view(Tensor) if np.asarray(a).ndim else np.asarray(a, dtype=dtype).view(Tensor)


def _plain(x):
    return x.view(np.ndarray) if isinstance(x, Tensor) else np.asarray(x)


def _ints(x):
    """a shape / paddings / multiples argument, possibly a list that holds tensors"""
    if isinstance(x, (list, tuple)):
        return [_ints(v) for v in x]
    return int(x)


class _Namespace(object):
    pass


def namespace(precision="float32"):
    """the `tf` the cut lines see"""
    if precision not in ("float32", "float64"):
        raise ValueError("precision must be 'float32' or 'float64'")
    tf = _Namespace()
    tf.precision = precision
    tf.stand_ins = set()
    tf.float32 = np.dtype(precision)
    tf.float64 = np.dtype(np.float64)
    tf.int32, tf.int64, tf.bool, tf.uint8 = np.dtype(np.int32), np.dtype(np.int64), np.dtype(np.bool_), np.dtype(np.uint8)
    tf.newaxis = None
    tf.Tensor, tf.SparseTensor = Tensor, SparseTensor
    F = tf.float32

    def convert(x, like=None):
        """tf.convert_to_tensor: Tensors as they are; Python ints int32, Python floats float32; numpy arrays keep their dtype except
        float64, which is the dtype numpy gives a list of Python floats (a float64 Tensor is built only through constant(dtype=))"""
        if isinstance(x, Tensor):
            return x
        a = np.asarray(x)
        if like is not None and not isinstance(x, np.ndarray):
            return _t(a.astype(_plain(like).dtype))
        if a.dtype.kind == "f" and not (isinstance(x, np.ndarray) and a.dtype == np.float32 and precision == "float32"):
            a = a.astype(F)
        elif a.dtype.kind in "iu" and not isinstance(x, (np.ndarray, np.generic)):
            a = a.astype(np.int32)
        return _t(a)

    tf.convert_to_tensor = convert

    # ---- shape -----------------------------------------------------------------------------------------------------------------------
    def reshape(tensor, shape, name=None):
        return _t(np.reshape(_plain(convert(tensor)), _ints(list(np.asarray(shape).reshape(-1)) if isinstance(shape, np.ndarray) else shape)))

    def expand_dims(input, axis=None, name=None, dim=None):
        return _t(np.expand_dims(_plain(convert(input)), axis if axis is not None else dim))

    def squeeze(input, axis=None, name=None, squeeze_dims=None):
        axis = axis if axis is not None else squeeze_dims
        return _t(np.squeeze(_plain(input), axis=tuple(axis) if isinstance(axis, (list, tuple)) else axis))

    def tile(input, multiples, name=None):
        multiples = _ints(list(multiples))
        assert len(multiples) == _plain(input).ndim, "tile: one multiple per axis"
        return _t(np.tile(_plain(input), multiples))

    def transpose(a, perm=None, name=None):
        return _t(np.transpose(_plain(a), perm))

    def pad(tensor, paddings, mode="CONSTANT", name=None, constant_values=0):
        if mode.upper() != "CONSTANT":
            raise NotImplementedError("pad: only CONSTANT")
        a = _plain(convert(tensor))
        paddings = [(int(lo), int(hi)) for lo, hi in paddings]
        if len(paddings) != a.ndim or any(lo < 0 or hi < 0 for lo, hi in paddings):
            raise ValueError("pad: paddings %s for a tensor of shape %s" % (paddings, a.shape))
        return _t(np.pad(a, paddings, mode="constant", constant_values=np.asarray(constant_values).astype(a.dtype)))

    def shape(input, name=None, out_type=np.int32):
        return _t(np.array(_plain(input).shape, dtype=out_type))

    def size(input, name=None, out_type=np.int32):
        return _t(np.array(_plain(input).size, dtype=out_type))

    def range_(start, limit=None, delta=1, dtype=None, name=None):
        if limit is None:
            start, limit = 0, start
        return _t(np.arange(int(start), int(limit), int(delta), dtype=dtype or np.int32))

    def ones_like(tensor, dtype=None, name=None):
        return _t(np.ones_like(_plain(tensor), dtype=dtype))

    def zeros_like(tensor, dtype=None, name=None):
        return _t(np.zeros_like(_plain(tensor), dtype=dtype))

    def constant(value, dtype=None, shape=None, name="Const"):
        a = np.asarray(value)
        if dtype is None:
            dtype = F if a.dtype.kind == "f" else np.int32 if a.dtype.kind in "iu" and not isinstance(value, (np.ndarray, np.generic)) else a.dtype
        a = a.astype(dtype)
        return _t(a if shape is None else np.broadcast_to(a, _ints(shape)).copy())

    tf.reshape, tf.expand_dims, tf.squeeze, tf.tile, tf.transpose, tf.pad, tf.shape, tf.size = reshape, expand_dims, squeeze, tile, transpose, pad, shape, size
    tf.range, tf.ones_like, tf.zeros_like, tf.constant = range_, ones_like, zeros_like, constant

    # ---- joining and indexing ----------------------------------------------------------------------------------------------------------
    def _same_dtype(values, what):
        arrays = [_plain(convert(v)) for v in values]
        if len({a.dtype for a in arrays}) > 1:
            raise TypeError("%s: inputs of different dtypes %s" % (what, [str(a.dtype) for a in arrays]))
        return arrays

    def concat(values, axis, name="concat"):
        return _t(np.concatenate(_same_dtype(values, "concat"), axis=int(axis)))

    def stack(values, axis=0, name="stack"):
        return _t(np.stack(_same_dtype(values, "stack"), axis=int(axis)))

    def _index(indices, bound, what):
        idx = _plain(indices)
        if idx.dtype.kind not in "iu":
            raise TypeError("%s: indices must be integers, got %s" % (what, idx.dtype))
        if idx.size and (idx.min() < 0 or idx.max() >= bound):
            raise IndexError("%s: index out of [0, %d)" % (what, bound))
        return idx.astype(np.int64)

    def gather(params, indices, validate_indices=None, name=None, axis=0):
        p = _plain(convert(params))
        return _t(np.take(p, _index(convert(indices), p.shape[axis], "gather"), axis=axis))

    def gather_nd(params, indices, name=None):
        p, idx = _plain(params), _plain(indices)
        k = idx.shape[-1]
        if k > p.ndim:
            raise ValueError("gather_nd: index depth %d for params of rank %d" % (k, p.ndim))
        cols = tuple(_index(idx[..., j], p.shape[j], "gather_nd") for j in range(k))
        return _t(p[cols])

    def where(condition, x=None, y=None, name=None):
        c = _plain(condition)
        if c.dtype != np.bool_:
            raise TypeError("where: the condition must be bool")
        if x is None and y is None:
            return _t(np.argwhere(c).astype(np.int64).reshape(-1, c.ndim))
        xs = _same_dtype([x, y], "where")
        return _t(np.where(c, xs[0], xs[1]))

    def boolean_mask(tensor, mask, name="boolean_mask", axis=None):
        a, m = _plain(tensor), _plain(mask)
        if m.dtype != np.bool_:
            raise TypeError("boolean_mask: the mask must be bool")
        axis = 0 if axis is None else axis
        assert a.shape[axis:axis + m.ndim] == m.shape, "boolean_mask: mask %s does not match %s" % (m.shape, a.shape)
        return _t(a[(slice(None),) * axis + (m,)])

    def scatter_nd(indices, updates, shape, name=None):
        idx, upd = _plain(indices), _plain(updates)
        shape = tuple(int(d) for d in (shape if not isinstance(shape, (Tensor, np.ndarray)) else np.asarray(shape).reshape(-1)))
        if idx.ndim == 1 and len(shape) == 1:
            tf.stand_ins.add("scatter_nd_rank1")
            idx = idx[:, None]
        k = idx.shape[-1]
        if k > len(shape) or upd.shape != idx.shape[:-1] + shape[k:]:
            raise ValueError("scatter_nd: indices %s, updates %s, shape %s" % (idx.shape, upd.shape, shape))
        out = np.zeros(shape, dtype=upd.dtype)
        cols = tuple(_index(idx[..., j], shape[j], "scatter_nd") for j in range(k))
        np.add.at(out, cols, upd)                                                          # duplicate indices add
        return _t(out)

    def unique(x, out_idx=np.int32, name=None):
        a = _plain(x)
        assert a.ndim == 1, "unique: a 1-D tensor"
        vals, first, inverse = np.unique(a, return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")                                           # first-occurrence order
        rank = np.empty(len(order), dtype=np.int64)
        rank[order] = np.arange(len(order))
        return Unique(_t(vals[order]), _t(rank[inverse.reshape(-1)].astype(out_idx)))

    tf.concat, tf.stack, tf.gather, tf.gather_nd, tf.where, tf.boolean_mask, tf.scatter_nd, tf.unique = concat, stack, gather, gather_nd, where, boolean_mask, scatter_nd, unique

    # ---- elementwise and logic -----------------------------------------------------------------------------------------------------------
    def cast(x, dtype, name=None):
        a = _plain(convert(x))
        dtype = np.dtype(dtype)
        if dtype == np.bool_:
            return _t(a != 0)
        return _t(a.astype(dtype))                                                         # float -> int truncates toward zero

    def to_float(x, name="ToFloat"):
        return cast(x, F)

    def _binary(ufunc):
        def op(x, y, name=None):
            x, y = (convert(x), convert(y, like=x)) if isinstance(x, Tensor) or not isinstance(y, Tensor) else (convert(x, like=y), y)
            return ufunc(x, y)
        return op

    def _unary(ufunc, floats_only=False):
        def op(x, name=None):
            x = convert(x)
            if floats_only and _plain(x).dtype.kind != "f":
                raise TypeError("%s: a float tensor" % ufunc.__name__)
            return ufunc(x)
        return op

    def div(x, y, name=None):
        x, y = convert(x), convert(y, like=x)
        return np.floor_divide(x, y) if _plain(x).dtype.kind in "iu" else np.true_divide(x, y)

    tf.cast, tf.to_float = cast, to_float
    tf.add, tf.subtract, tf.multiply, tf.divide, tf.div = _binary(np.add), _binary(np.subtract), _binary(np.multiply), _binary(np.true_divide), div
    tf.maximum, tf.minimum = _binary(np.maximum), _binary(np.minimum)
    tf.abs, tf.square, tf.negative = _unary(np.abs), _unary(np.square), _unary(np.negative)
    tf.sqrt, tf.exp, tf.log = _unary(np.sqrt, True), _unary(np.exp, True), _unary(np.log, True)
    tf.greater, tf.greater_equal, tf.less, tf.less_equal = _binary(np.greater), _binary(np.greater_equal), _binary(np.less), _binary(np.less_equal)
    tf.equal, tf.not_equal = _binary(np.equal), _binary(np.not_equal)

    def logical_and(x, y, name=None):
        x, y = _plain(x), _plain(y)
        if x.dtype != np.bool_ or y.dtype != np.bool_:
            raise TypeError("logical_and: bool tensors")
        return _t(np.logical_and(x, y))

    def logical_not(x, name=None):
        x = _plain(x)
        if x.dtype != np.bool_:
            raise TypeError("logical_not: a bool tensor")
        return _t(np.logical_not(x))

    tf.logical_and, tf.logical_not = logical_and, logical_not

    # ---- reductions --------------------------------------------------------------------------------------------------------------------
    def _reduce(fn, empty):
        def op(input_tensor, axis=None, keepdims=None, name=None, reduction_indices=None, keep_dims=None):
            a = _plain(convert(input_tensor))
            axis = axis if axis is not None else reduction_indices
            keep = bool(keepdims if keepdims is not None else keep_dims)
            if isinstance(axis, (list, np.ndarray)):
                axis = tuple(int(v) for v in axis)
            if a.size == 0 and empty is not None:                                          # the identity of the reduction
                return _t(np.full(np.sum(a, axis=axis, keepdims=keep).shape, empty, dtype=a.dtype))
            return _t(np.asarray(fn(a, axis=axis, keepdims=keep), dtype=a.dtype))
        return op

    tf.reduce_sum, tf.reduce_mean = _reduce(np.sum, None), _reduce(np.mean, None)
    tf.reduce_max, tf.reduce_min = _reduce(np.max, -np.inf), _reduce(np.min, np.inf)

    def _arg(fn):
        def op(input, axis=None, name=None, dimension=None, output_type=np.int64):
            axis = axis if axis is not None else dimension
            return _t(fn(_plain(input), axis=0 if axis is None else int(axis)).astype(output_type))      # numpy: the first among equals
        return op

    tf.argmax, tf.argmin = _arg(np.argmax), _arg(np.argmin)

    # ---- control and sets ----------------------------------------------------------------------------------------------------------------
    def cond(pred, true_fn=None, false_fn=None, strict=False, name=None, fn1=None, fn2=None):
        p = _plain(pred)
        if p.dtype != np.bool_ or p.ndim != 0:
            raise TypeError("cond: a scalar bool predicate")
        return convert((true_fn or fn1)() if bool(p) else (false_fn or fn2)())

    def map_fn(fn, elems, dtype=None, parallel_iterations=10, back_prop=True, swap_memory=False, infer_shape=True, name=None):
        e = convert(elems)
        dtype = np.dtype(dtype) if dtype is not None else _plain(e).dtype
        rows = [_plain(convert(fn(e[k]))) for k in range(e.shape[0])]
        for r in rows:
            if r.dtype != dtype:
                raise TypeError("map_fn: fn returned %s, dtype says %s" % (r.dtype, dtype))
        return _t(np.stack(rows, 0)) if rows else _t(np.zeros((0,), dtype=dtype))

    def py_func(func, inp, Tout, stateful=True, name=None):
        """the inputs reach func as numpy arrays of the dtypes tf.convert_to_tensor gives them; the result must have dtype Tout"""
        res = np.asarray(func(*[np.array(_plain(convert(v))) for v in inp]))
        if res.dtype != np.dtype(Tout):
            raise TypeError("py_func: the function returned %s, Tout is %s" % (res.dtype, np.dtype(Tout)))
        return _t(res)

    def stop_gradient(input, name=None):
        return convert(input)

    def random_shuffle(value, seed=None, name=None):
        tf.stand_ins.add("random_shuffle")
        return convert(value)

    def set_intersection(a, b, validate_indices=True):
        a, b = _plain(a), _plain(b)
        if a.dtype != b.dtype or a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0]:
            raise TypeError("set_intersection: two (rows, n) tensors of one dtype")
        rows = [np.intersect1d(a[i], b[i]) for i in range(a.shape[0])]                    # sorted and unique
        width = max([len(r) for r in rows] + [0])
        indices = np.array([(i, j) for i, r in enumerate(rows) for j in range(len(r))], dtype=np.int64).reshape(-1, 2)
        values = np.concatenate(rows).astype(a.dtype) if rows else np.zeros(0, a.dtype)
        return SparseTensor(_t(indices), _t(values), _t(np.array([a.shape[0], width], dtype=np.int64)))

    def sparse_tensor_to_dense(sp_input, default_value=0, validate_indices=True, name=None):
        out = np.full(tuple(int(d) for d in _plain(sp_input.dense_shape)), default_value, dtype=_plain(sp_input.values).dtype)
        idx = _plain(sp_input.indices)
        out[tuple(idx[:, j] for j in range(idx.shape[1]))] = _plain(sp_input.values)
        return _t(out)

    tf.cond, tf.map_fn, tf.py_func, tf.stop_gradient, tf.random_shuffle = cond, map_fn, py_func, stop_gradient, random_shuffle
    tf.sets = _Namespace()
    tf.sets.set_intersection = set_intersection
    tf.sparse_tensor_to_dense = sparse_tensor_to_dense

    # ---- nn and losses -----------------------------------------------------------------------------------------------------------------
    def top_k(input, k=1, sorted=True, name=None):
        a = _plain(input)
        k = int(k)
        if k > a.shape[-1]:
            raise ValueError("top_k: k = %d for %d columns" % (k, a.shape[-1]))
        order = np.argsort(-a, axis=-1, kind="stable")[..., :k]                            # the lower index first among equals
        return TopK(_t(np.take_along_axis(a, order, -1)), _t(order.astype(np.int32)))

    def _log_softmax(x, axis=-1):
        shifted = x - np.max(x, axis=axis, keepdims=True)
        return shifted - np.log(np.sum(np.exp(shifted), axis=axis, keepdims=True, dtype=x.dtype))

    def softmax(logits, axis=None, name=None, dim=None):
        axis = axis if axis is not None else dim if dim is not None else -1
        return _t(np.exp(_log_softmax(_plain(logits), axis)))

    def sparse_softmax_cross_entropy_with_logits(_sentinel=None, labels=None, logits=None, name=None):
        assert _sentinel is None, "sparse_softmax_cross_entropy_with_logits: named arguments only"
        x, lab = _plain(logits), _plain(labels)
        if lab.dtype not in (np.int32, np.int64) or lab.shape != x.shape[:-1] or x.dtype.kind != "f":
            raise TypeError("sparse_softmax_cross_entropy_with_logits: labels %s %s for logits %s %s" % (lab.dtype, lab.shape, x.dtype, x.shape))
        lab = _index(lab, x.shape[-1], "sparse_softmax_cross_entropy_with_logits")
        return _t(-np.take_along_axis(_log_softmax(x), lab[..., None], -1)[..., 0])

    def sigmoid_cross_entropy_with_logits(_sentinel=None, labels=None, logits=None, name=None):
        assert _sentinel is None, "sigmoid_cross_entropy_with_logits: named arguments only"
        x, z = _plain(logits), _plain(labels)
        if x.dtype != z.dtype or x.shape != z.shape:
            raise TypeError("sigmoid_cross_entropy_with_logits: labels %s %s for logits %s %s" % (z.dtype, z.shape, x.dtype, x.shape))
        return _t(np.maximum(x, 0) - x * z + np.log1p(np.exp(-np.abs(x))))               # the documented stable form

    def losses_sparse_softmax_cross_entropy(labels, logits, weights=1.0, scope=None, loss_collection=None, reduction="SUM_BY_NONZERO_WEIGHTS"):
        """the TF 1.x default reduction: the weighted sum over the number of non-zero weights (0 when there is none)"""
        if reduction != "SUM_BY_NONZERO_WEIGHTS":
            raise NotImplementedError(reduction)
        losses = _plain(sparse_softmax_cross_entropy_with_logits(labels=labels, logits=logits))
        w = np.broadcast_to(_plain(convert(weights, like=_t(losses))), losses.shape)
        present = np.count_nonzero(w)
        total = np.sum(losses * w, dtype=losses.dtype)
        return _t(np.asarray(total / losses.dtype.type(present) if present else 0, dtype=losses.dtype))

    tf.nn = _Namespace()
    tf.nn.top_k, tf.nn.softmax = top_k, softmax
    tf.nn.sparse_softmax_cross_entropy_with_logits = sparse_softmax_cross_entropy_with_logits
    tf.nn.sigmoid_cross_entropy_with_logits = sigmoid_cross_entropy_with_logits
    tf.losses = _Namespace()
    tf.losses.sparse_softmax_cross_entropy = losses_sparse_softmax_cross_entropy
    return tf
