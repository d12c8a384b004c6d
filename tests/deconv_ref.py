"""float64 restatement of conv2d_transpose (VALID, NHWC) by its definition: every tap (ky, kx) adds X . K[ky, kx]^T to the output
pixels (iy*sh + ky, ix*sw + kx).  Runs on whatever device its inputs are on (fast on the GPU for the decoder's n = 512 layers);
tests/test_cpu_deconv.py pins it to torch.nn.functional.conv_transpose2d."""
import torch


def out_size(h, s, k):
    return h * s + max(k - s, 0)


def deconv(x, k, b=None, stride=(1, 1)):
    """x (n, hi, wi, cin), k (kh, kw, cout, cin), b (cout) or None -> (n, Ho, Wo, cout); autograd supplies the backward"""
    n, hi, wi, cin = x.shape
    kh, kw, cout, _ = k.shape
    sh, sw = stride
    ho, wo = out_size(hi, sh, kh), out_size(wi, sw, kw)
    taps = []
    for ky in range(kh):
        for kx in range(kw):
            contrib = (x.reshape(-1, cin) @ k[ky, kx].t()).reshape(n, hi, wi, cout)
            pad = (0, 0, kx, wo - kx - (wi - 1) * sw - 1, ky, ho - ky - (hi - 1) * sh - 1)
            # place contrib at rows ky, ky+sh, ... and columns kx, kx+sw, ...: interleave with zeros, then pad to (ho, wo)
            z = contrib.new_zeros(n, (hi - 1) * sh + 1, (wi - 1) * sw + 1, cout)
            z = z.index_put((torch.arange(n, device=x.device)[:, None, None],
                             (torch.arange(hi, device=x.device) * sh)[None, :, None],
                             (torch.arange(wi, device=x.device) * sw)[None, None, :]), contrib)
            taps.append(torch.nn.functional.pad(z, pad))
    y = torch.stack(taps).sum(0)
    return y + b if b is not None else y


def bn_relu(y, gamma, beta, mm, mv, is_training, decay=0.9, relu=True, eps=1e-3):
    """tf.contrib.layers.batch_norm over every axis but the last (oracle/mlp_ref.py's arithmetic), then ReLU"""
    c = y.shape[-1]
    rows = y.reshape(-1, c)
    if is_training:
        mean = rows.mean(0)
        var = ((rows - mean) ** 2).mean(0)
        mm = mm * decay + mean.detach() * (1 - decay)
        mv = mv * decay + var.detach() * (1 - decay)
    else:
        mean, var = mm, mv
    inv = torch.rsqrt(var + eps) * gamma
    out = (rows * inv + (beta - mean * inv)).reshape(y.shape)
    return (torch.relu(out) if relu else out), mm, mv
