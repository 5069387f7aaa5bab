"""numpy statement of the class selection of the class-sharded head (fr_class_sample; frhip/sharded_head.py), the numpy
stand-ins of the three ``HipKernels`` methods built on it, and a float64 statement of one sampled step.

All integer arithmetic is mod 2**32 (numpy uint32 wraps):

    fmix32(h)   h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16
    salt        fmix32(seed + 0x9E3779B9 * step)
    key(c)      fmix32((class0 + c) ^ salt),  c = 0 .. n - 1
    pos[c]      some row's local label is c (labels outside [0, n) mark nothing)
    S           the positives + the n_s - P non-positive classes with the smallest keys
    idx         S ascending;  inv[c] = position in idx or -1;  label_s = inv[label] where 0 <= label < n, else -1

Test infrastructure only.  ``select_unforced`` and ``select_local_keys`` are wrong on purpose (negative controls)."""
import numpy as np

M32 = 0xFFFFFFFF


def fmix32(h):
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def salt(seed, step):
    return int(fmix32(np.uint32((int(seed) + 0x9E3779B9 * int(step)) & M32)))


def keys(n, class0, salt_):
    return fmix32((np.arange(n, dtype=np.uint64) + np.uint64(class0)).astype(np.uint32) ^ np.uint32(salt_))


def positives(label_local, n):
    lab = np.asarray(label_local, dtype=np.int64)
    pos = np.zeros(n, dtype=bool)
    pos[lab[(lab >= 0) & (lab < n)]] = True
    return pos


def _finish(sel, label_local, n):
    idx = np.flatnonzero(sel).astype(np.int32)
    inv = np.full(n, -1, dtype=np.int32)
    inv[idx] = np.arange(idx.shape[0], dtype=np.int32)
    lab = np.asarray(label_local, dtype=np.int64)
    own = (lab >= 0) & (lab < n)
    label_s = np.where(own, inv[np.where(own, lab, 0)], -1).astype(np.int64)
    return idx, inv, label_s


def select(label_local, n, n_s, salt_, class0):
    """(idx [n_s] int32 ascending, inv [n] int32, label_s [rows] int64)."""
    lab = np.asarray(label_local, dtype=np.int64)
    assert 1 <= n_s <= n and n_s >= min(n, lab.shape[0]), (n, n_s, lab.shape[0])
    pos = positives(lab, n)
    k = n_s - int(pos.sum())
    key = keys(n, class0, salt_)
    neg = np.flatnonzero(~pos)
    take = neg[np.argsort(key[neg], kind="stable")[:k]]
    sel = pos.copy()
    sel[take] = True
    return _finish(sel, lab, n)


def select_unforced(label_local, n, n_s, salt_, class0):
    """Wrong on purpose: the n_s smallest keys, the positives not forced in."""
    key = keys(n, class0, salt_)
    sel = np.zeros(n, dtype=bool)
    sel[np.argsort(key, kind="stable")[:n_s]] = True
    return _finish(sel, label_local, n)


def select_local_keys(label_local, n, n_s, salt_, class0):
    """Wrong on purpose: the key of the local index, without class0 (every shard would draw the same local set)."""
    return select(label_local, n, n_s, salt_, 0)


def select_dropping_a_positive(label_local, n, n_s, salt_, class0):
    """Wrong on purpose: the first positive gives its place to the unselected class with the smallest key."""
    idx, inv, _ = select(label_local, n, n_s, salt_, class0)
    pos, sel = positives(label_local, n), inv >= 0
    if pos.any() and not sel.all():
        key = keys(n, class0, salt_)
        out = np.flatnonzero(~sel)
        sel[np.flatnonzero(pos)[0]] = False
        sel[out[np.argmin(key[out])]] = True
    return _finish(sel, label_local, n)


# ------------------------------------------------------------------------------------------------ stand-in kernels


def sampling_kernels(base, select_fn=select):
    """``base`` (a stand-in for HipKernels on the CPU) with the three class-sampling methods in numpy / torch indexing.
    The instance keeps every (idx, inv) it drew in ``drawn`` and counts the calls in ``calls``."""
    import torch

    class Sampling(base):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.drawn, self.calls = [], {"sample_classes": 0, "gather_rows": 0, "scatter_rows": 0}

        def sample_classes(self, label_local, n, n_s, salt_, class0):
            self.calls["sample_classes"] += 1
            idx, inv, label_s = select_fn(label_local.numpy(), n, n_s, salt_, class0)
            self.drawn.append((idx, inv))
            return torch.from_numpy(idx), torch.from_numpy(inv), torch.from_numpy(label_s)

        def gather_rows(self, w, idx):
            self.calls["gather_rows"] += 1
            return w[idx.long()].clone()

        def scatter_rows(self, g, inv, n):
            self.calls["scatter_rows"] += 1
            out = torch.zeros((n,) + tuple(g.shape[1:]), dtype=g.dtype)
            hit = inv >= 0
            out[hit] = g[inv[hit].long()]
            return out

    return Sampling()


# ------------------------------------------------------------------------------------------------ one step in float64


def restricted_step(name, full, bias, x, label, cols, step, loss, gamma=2.0):
    """The full head of head/metrics.py in float64 on the whole batch, restricted to the classes ``cols`` (ascending global
    indices, every label among them): (loss, gx, gw [len(cols), D], gb or None).  ``step``: forward calls before this one
    (SphereFace's lambda)."""
    import torch
    import torch.nn.functional as F
    from head import metrics as H
    from oracle import irse_ref as O
    cols_t = torch.as_tensor(np.asarray(cols, dtype=np.int64))
    remap = torch.full((full.shape[0],), -1, dtype=torch.long)
    remap[cols_t] = torch.arange(cols_t.shape[0])
    lab = remap[label]
    assert bool((lab >= 0).all()), "a label is not among the selected classes"
    head = getattr(H, name)(full.shape[1], cols_t.shape[0], None).double()
    with torch.no_grad():
        head.weight.copy_(full.double()[cols_t])
        if name == "Softmax":
            head.bias.copy_(bias.double()[cols_t])
    if name == "SphereFace":
        head.iter = step
    xd = x.double().clone().requires_grad_(True)
    if name == "ArcFace":  # the module has no host path of its own: the oracle's statement of head/metrics.py:66-140
        logits = O.arcface_forward(xd, head.weight, lab, s=head.s, m=head.m, easy_margin=head.easy_margin)
    elif name == "CosFace":
        logits = O.cosface_forward(xd, head.weight, lab, s=head.s, m=head.m)
    else:
        logits = head(xd, lab)
    value = O.focal_loss(logits, lab, gamma) if loss == "Focal" else F.cross_entropy(logits, lab)
    params = [xd, head.weight] + ([head.bias] if name == "Softmax" else [])
    grads = torch.autograd.grad(value, params)
    return value.detach(), grads[0], grads[1], (grads[2] if name == "Softmax" else None)
