"""conv2d_transpose's arithmetic (tf.layers.conv2d_transpose as utils/tf_util.py:188-267 calls it: VALID, NHWC) as one autograd node
over the three HIP kernels of csrc/deconv.hip.  No CPU fallback."""
import torch

from . import _lib as L


def deconv_out_size(size, stride, kernel):
    """slim's get_deconv_dim for padding='VALID' (tf_util.py:224-230): size*stride + max(kernel - stride, 0)"""
    return size * stride + max(kernel - stride, 0)


class _Deconv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, bias, sh, sw):
        lib = L.lib()
        n, hi, wi, cin = x.shape
        kh, kw, cout, kcin = kernel.shape
        if kcin != cin:
            raise ValueError("kernel (kh, kw, Cout, Cin) has Cin %d, inputs have %d channels" % (kcin, cin))
        y = torch.empty(n, deconv_out_size(hi, sh, kh), deconv_out_size(wi, sw, kw), cout, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            L.check(lib.gspn_deconv_fwd(n, hi, wi, cin, cout, kh, kw, sh, sw, L.ptr(x), L.ptr(kernel), L.ptr(bias), L.ptr(y), L.stream()),
                    "deconv_fwd")
        ctx.save_for_backward(x, kernel)
        ctx.stride = (sh, sw)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = L.lib()
        x, kernel = ctx.saved_tensors
        sh, sw = ctx.stride
        n, hi, wi, cin = x.shape
        kh, kw, cout, _ = kernel.shape
        dy = dy.contiguous()
        shape = (n, hi, wi, cin, cout, kh, kw, sh, sw)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dk = torch.empty_like(kernel) if ctx.needs_input_grad[1] else None
        db = torch.empty(cout, dtype=torch.float32, device=x.device) if ctx.has_bias and ctx.needs_input_grad[2] else None
        with torch.cuda.device(x.device):
            st = L.stream()
            if dx is not None:
                L.check(lib.gspn_deconv_bwd_input(*shape, L.ptr(dy), L.ptr(kernel), L.ptr(dx), st), "deconv_bwd_input")
            if dk is not None or db is not None:
                ws = torch.empty((int(lib.gspn_deconv_bwd_kernel_work_bytes(*shape)) + 3) // 4, dtype=torch.float32, device=x.device)
                L.check(lib.gspn_deconv_bwd_kernel(*shape, L.ptr(dy), L.ptr(x), L.ptr(dk), L.ptr(db), L.ptr(ws), st), "deconv_bwd_kernel")
        return dx, dk, db, None, None


def conv2d_transpose_valid(x, kernel, bias=None, stride=(1, 1)):
    """x (n, hi, wi, cin), kernel (kh, kw, cout, cin), bias (cout) or None -> (n, Ho, Wo, cout), Ho = hi*sh + max(kh - sh, 0)."""
    x = L.need(x, torch.float32, 4, "inputs")
    kernel = L.need(kernel, torch.float32, 4, "kernel")
    if bias is not None:
        bias = L.need(bias, torch.float32, 1, "bias")
    sh, sw = (int(s) for s in stride)
    return _Deconv2d.apply(x, kernel, bias, sh, sw)
