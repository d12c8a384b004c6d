"""Plain torch restatements of the glue of R-PointNet's inference path (models/model_rpointnet.py:1136-1163), written against the
reference's line numbers, for the tests of gspn_amd/inference.py.  CPU tensors, float64 where a value is computed."""
import torch


def crop_mean(table, idx):
    """:1144-1150 for the appended columns: gather each ROI's points, average over them.  table (B, N, C), idx (B, R, P) integer, a value
    outside [0, N) clamped -> (B, R, C) float64"""
    b, n, c = table.shape
    r, p = idx.shape[1:]
    i = idx.long().clamp(0, n - 1).reshape(b, r * p, 1).expand(b, r * p, c)
    return torch.gather(table.double(), 1, i).reshape(b, r, p, c).mean(2)


def crop_mean_naive(table, idx):
    """the same, one ROI and one point at a time"""
    b, n, c = table.shape
    r, p = idx.shape[1:]
    out = torch.zeros(b, r, c, dtype=torch.float64)
    for s in range(b):
        for k in range(r):
            for j in range(p):
                out[s, k] += table[s, min(max(int(idx[s, k, j]), 0), n - 1)].double()
    return out / p


def nearest_seed(pc, pc_seed):
    """:1136.  pc (B, N, 3), pc_seed (B, S, 3) float32 -> (B, N) int64: the first minimum (tf.argmin) of (dx*dx + dy*dy) + dz*dz, the
    distance in float32 as the reference computes it"""
    d = pc.float().unsqueeze(2) - pc_seed.float().unsqueeze(1)
    dist = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    low = dist.min(-1, keepdim=True).values
    cols = torch.arange(dist.shape[-1])
    return torch.where(dist == low, cols, cols.new_full((), dist.shape[-1])).min(-1).values


def point_probabilities(pc, pc_seed, fb_prob, sem_class_logits):
    """:1136-1141.  fb_prob (B, S, 2), sem_class_logits (B, N, C) -> (B, N, 1 + C) float64: column 0 the foreground probability of the
    nearest seed, then softmax(sem_class_logits)"""
    midx = nearest_seed(pc, pc_seed)
    fb = torch.gather(fb_prob[:, :, 1].double(), 1, midx)
    return torch.cat((fb.unsqueeze(-1), torch.softmax(sem_class_logits.double(), -1)), -1)


def first_max_pick(values, logits):
    """:1159-1162.  values, logits (B, R, C) -> (B, R): values at the first maximal column of logits (tf.argmax)"""
    top = logits.max(-1, keepdim=True).values
    cols = torch.arange(logits.shape[-1])
    midx = torch.where(logits == top, cols, cols.new_full((), logits.shape[-1])).min(-1).values
    return torch.gather(values, 2, midx.unsqueeze(-1)).squeeze(-1)
