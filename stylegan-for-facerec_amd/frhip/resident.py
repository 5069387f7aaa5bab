"""Device-resident training set: decode once, keep the bytes in HBM, pull every batch with one launch.

With ``GPU_INPUT_PIPELINE=True`` the host workers still open and decode every file in every epoch.  The reference's
training sets are small next to the device memory (1.3 M aligned 112x112 crops are 49 GB as uint8 HWC), so the decoded set
can live on the device: ``ResidentStore.build`` makes ONE sequential pass over the dataset, and ``ResidentLoader`` then
yields the batches of an epoch with one ``fr_augment_u8_gather`` launch each -- the host ships an index, a crop and a flip
per image (13 bytes) instead of the image (37 KB), and no worker runs after start-up.

The loader is defined to be, bit for bit, the ``GPU_INPUT_PIPELINE=True`` run it replaces: the same samples in the same
order (``epoch_batches`` instantiates the same ``DistributedSampler`` and ``BatchSampler`` and applies the refill rule of
``util.utils.collate_fn_ignore_none``), the same crop / flip draws from the same generator in the same order
(``GpuTrainTransform.draw``), the same transform (the kernel shares its per-pixel body with ``fr_augment_u8``), and the same
use of the global torch generator (one draw per epoch, the ``DataLoader``'s worker base seed), so the ``State_*`` files
agree too.  Every rank holds the whole set.

With RandAugment on (``gpu_tf.randaug``) the gather moves into ``fr_randaug_u8``, which reads ``store[idx[b]]``, writes the
augmented uint8 batch and the labels, and the unchanged ``fr_augment_u8`` runs on that batch: the loader path's two launches,
with the chain of every image drawn after the batch's crop / flip draws, as there.
"""
import time

import numpy as np
import torch
from torch.utils.data import BatchSampler, DataLoader
from torch.utils.data.distributed import DistributedSampler

from . import ops
from .input_pipeline import MAX_ASPECT

BYTES_PER_IMAGE = 4 + 8 + 1  # what a batch ships per image: int32 index, int32 (x0, y0), uint8 flip
CHUNK = 1024  # images per staging chunk of the build pass (38.5 MB of pinned memory at 112x112, two chunks in flight)


def refill_ignore_none(batch):
    """The list part of ``util.utils.collate_fn_ignore_none``: drop the ``None`` entries, then refill by repeating the
    survivors -- the reference's loop, which appends ``batch[:missing]`` of the GROWING list ``missing`` times and so can
    return more entries than came in."""
    want = len(batch)
    batch = [b for b in batch if b is not None]
    missing = want - len(batch)
    if missing > 0:
        for _ in range(missing):
            batch = batch + batch[:missing]
    return batch


def _samplers(n, world, rank, seed, batch_size, drop_last):
    sampler = DistributedSampler(range(n), world, rank, shuffle=True, seed=seed)
    return sampler, BatchSampler(sampler, batch_size, drop_last)


def epoch_batches(n, valid, world, rank, seed, epoch, batch_size, drop_last):
    """The index lists of one epoch, as ``DataLoader(dataset, batch_size, sampler=DistributedSampler(dataset, world, rank,
    shuffle=True, seed=seed), drop_last=drop_last, collate_fn=collate_fn_ignore_none)`` delivers them after
    ``set_epoch(epoch)`` for a dataset of ``n`` samples of which those with ``valid[i] == False`` return ``None``."""
    sampler, batches = _samplers(n, world, rank, seed, batch_size, drop_last)
    sampler.set_epoch(epoch)
    out = []
    for batch in batches:
        kept = refill_ignore_none([i if valid[i] else None for i in batch])
        if not kept:  # default_collate of an empty list fails in the loader path as well
            raise ValueError("resident: every sample of the batch %r failed to load" % (list(batch),))
        out.append(kept)
    return out


def _chunk_collate(batch):
    """A list collate that keeps every slot: per item ``None`` (failed) or ``(dtype, shape)``, the labels, and the valid
    images stacked into ONE tensor when they are uint8 and share a shape (else ``None``: the caller names the offender).
    One tensor per chunk crosses the worker boundary, not one shared-memory handle per image."""
    good = [it for it in batch if it is not None]
    seen = [None if it is None else (it[0].dtype, tuple(it[0].shape)) for it in batch]
    same = bool(good) and all(torch.is_tensor(it[0]) for it in good) and len(set(s for s in seen if s is not None)) == 1
    stacked = torch.stack([it[0] for it in good]) if same and good[0][0].dtype == torch.uint8 else None
    return seen, [None if it is None else int(it[1]) for it in batch], stacked


class ResidentStore(object):
    """``data`` uint8 [M, H, W, 3] and ``labels`` int64 [M] on the device, ``valid`` bool [M] on the host (a sample that
    failed to load keeps its slot, zero-filled and never drawn)."""

    def __init__(self, data, labels, valid):
        self.data, self.labels, self.valid = data, labels, np.asarray(valid, dtype=bool)

    def __len__(self):
        return len(self.valid)

    @classmethod
    def build(cls, dataset, device, num_workers, max_gb=None):
        """One sequential pass over ``dataset``, whose items are ``(uint8 [H, W, 3] tensor, int label)`` or ``None``
        (``FacesDataset`` with ``StageTransform``, ``SyntheticFaces(staged=True)``).  ``max_gb``: the most the image bytes
        may take, in GB of 1e9 bytes; default half of the device's free memory at this moment."""
        t0 = time.time()
        device = torch.device(device)
        m = len(dataset)
        names = getattr(dataset, "filenames", None)
        # a generator of its own: the pass leaves the global torch generator (initial weights, State_* files) untouched
        loader = DataLoader(dataset, batch_size=CHUNK, shuffle=False, collate_fn=_chunk_collate, num_workers=num_workers,
                            generator=torch.Generator())
        valid = np.zeros(m, dtype=bool)
        host_labels = torch.zeros(m, dtype=torch.int64)
        data, size, stage, done = None, None, None, [None, None]
        at = 0  # the slot of the chunk's first sample
        for k, (seen, chunk_labels, stacked) in enumerate(loader):
            n = len(seen)
            for j, s in enumerate(seen):
                if s is not None:
                    size = cls._check_item(s, size, at + j, names)
                    valid[at + j] = True
                    host_labels[at + j] = chunk_labels[j]
            if data is None and size is not None:
                need = m * size[0] * size[1] * 3
                if max_gb is None:
                    limit, origin = torch.cuda.mem_get_info(device)[0] // 2, "half of the device's free memory"
                else:
                    limit, origin = int(float(max_gb) * 1e9), "max_gb"
                if need > limit:
                    raise ValueError("resident: %d images of %dx%dx3 need %.6f GB, the limit (%s) is %.6f GB"
                                     % (m, size[0], size[1], need / 1e9, origin, limit / 1e9))
                data = torch.empty(m, size[0], size[1], 3, dtype=torch.uint8, device=device)
                if at:
                    data[:at].zero_()  # chunks in which every sample failed
                stage = [torch.empty(CHUNK, size[0], size[1], 3, dtype=torch.uint8).pin_memory() for _ in range(2)]
            if data is not None:
                buf = stage[k % 2]
                if done[k % 2] is not None:
                    done[k % 2].synchronize()  # the copy that last read this staging buffer
                ok = torch.from_numpy(valid[at:at + n])
                buf[:n][~ok] = 0
                if stacked is not None:
                    buf[:n][ok] = stacked
                data[at:at + n].copy_(buf[:n], non_blocking=True)
                done[k % 2] = torch.cuda.Event()
                done[k % 2].record(torch.cuda.current_stream(device))
            at += n
        if size is None:
            raise ValueError("resident: none of the %d samples could be loaded" % m)
        labels = host_labels.pin_memory().to(device, non_blocking=True)
        torch.cuda.synchronize(device)
        print("Resident dataset: {} images, {} failed samples, {:.3f} GB, {:.1f} s".format(
            m, int(m - valid.sum()), data.numel() / 1e9, time.time() - t0))
        return cls(data, labels, valid)

    @staticmethod
    def _check_item(seen, size, index, names):
        """``seen``: (dtype, shape) of sample ``index``; ``size``: the (H, W) of the set, or None before the first sample."""
        where = "sample %d%s" % (index, " (%s)" % names[index] if names is not None else "")
        dtype, shape = seen
        if dtype != torch.uint8 or len(shape) != 3 or shape[2] != 3:
            raise ValueError("resident: %s is %s %s, not a uint8 [H, W, 3] tensor" % (where, dtype, shape))
        h, w = int(shape[0]), int(shape[1])
        if h > MAX_ASPECT * w or w > MAX_ASPECT * h:
            raise ValueError("resident: %s is %dx%d, beyond the supported aspect ratio of %d:1" % (where, h, w, MAX_ASPECT))
        if size is not None and (h, w) != size:
            raise ValueError("resident: %s is %dx%d, the set is %dx%d: all images must share one size"
                             % (where, h, w, size[0], size[1]))
        return h, w


class ResidentLoader(object):
    """Stands where ``DataLoader(dataset, batch_size, sampler=DistributedSampler(...), collate_fn=collate_fn_ignore_none)``
    followed by ``gpu_tf(inputs.to(device), generator=...)`` stood: iterating yields ``(inputs float32 [b, 3, S, S], labels
    int64 [b])`` on the device.  ``generator``: the ``torch.Generator`` of the crop / flip draws, given to ``__iter__`` or
    set on the loader (``loader.generator``); default the global one, as in ``GpuTrainTransform``."""

    def __init__(self, store, gpu_tf, batch_size, drop_last, world=1, rank=0, seed=0, generator=None):
        self.store, self.gpu_tf, self.generator = store, gpu_tf, generator
        self.batch_size, self.drop_last = int(batch_size), bool(drop_last)
        self.world, self.rank, self.seed, self.epoch = int(world), int(rank), int(seed), 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return len(_samplers(len(self.store), self.world, self.rank, self.seed, self.batch_size, self.drop_last)[1])

    def __iter__(self, generator=None):
        generator = self.generator if generator is None else generator
        store, tf = self.store, self.gpu_tf
        m, h, w = int(store.data.shape[0]), int(store.data.shape[1]), int(store.data.shape[2])
        dev = store.data.device
        plan = epoch_batches(len(store), store.valid, self.world, self.rank, self.seed, self.epoch, self.batch_size,
                             self.drop_last)
        # the loader this one replaces draws its workers' base seed from the global generator when an epoch starts; the
        # same draw here keeps the host RNG state (initialisation drawn later, the State_* files) that of the loader run
        torch.empty((), dtype=torch.int64).random_()
        xtab, ytab, lut, kx, ky = tf.tables(dev, h, w)
        for idx in plan:
            b = len(idx)
            idx = np.asarray(idx, dtype=np.int64)
            if idx.min() < 0 or idx.max() >= m:
                raise ValueError("resident: batch index outside [0, %d): %d .. %d" % (m, idx.min(), idx.max()))
            crop, flip = tf.draw(b, generator)
            if getattr(tf, "randaug", None) is not None:
                # RandAugment on: the gather moves into fr_randaug_u8 (idx, labels), and the unchanged fr_augment_u8 runs on
                # the staged result -- the loader path's two launches, draws in the loader path's order.  Still one pinned
                # block and one asynchronous copy, 13 + 5 K bytes per image:
                # [idx int32 b | crop int32 2b | par float32 bK | flip uint8 b | op uint8 bK]
                op, par = tf.randaug.draw(b, generator, (h, w))
                k = int(op.shape[1])
                host = torch.empty((BYTES_PER_IMAGE + 5 * k) * b, dtype=torch.uint8, pin_memory=True)
                host[:4 * b].view(torch.int32).copy_(torch.from_numpy(idx))
                host[4 * b:12 * b].view(torch.int32).copy_(crop.reshape(-1))
                host[12 * b:(12 + 4 * k) * b].view(torch.float32).copy_(par.reshape(-1))
                host[(12 + 4 * k) * b:(13 + 4 * k) * b].copy_(flip)
                host[(13 + 4 * k) * b:].copy_(op.reshape(-1))
                pack = host.to(dev, non_blocking=True)
                labels = torch.empty(b, device=dev, dtype=torch.int64)
                staged = tf.randaug.launch(store.data, pack[(13 + 4 * k) * b:].view(b, k),
                                           pack[12 * b:(12 + 4 * k) * b].view(torch.float32).view(b, k), b, h, w,
                                           pack[:4 * b].view(torch.int32), store.labels, labels)
                out = torch.empty(b, 3, tf.size, tf.size, device=dev, dtype=torch.float32)
                ops.call("fr_augment_u8", staged, xtab, ytab, pack[4 * b:12 * b].view(torch.int32),
                         pack[(12 + 4 * k) * b:(13 + 4 * k) * b], lut, out, b, h, w, tf.big, tf.big, tf.size, kx, ky,
                         ops.current_stream_ptr())()
                yield out, labels
                continue
            # one pinned block, one asynchronous copy: [idx int32 b | crop int32 2b | flip uint8 b]
            host = torch.empty(BYTES_PER_IMAGE * b, dtype=torch.uint8, pin_memory=True)
            host[:4 * b].view(torch.int32).copy_(torch.from_numpy(idx))
            host[4 * b:12 * b].view(torch.int32).copy_(crop.reshape(-1))
            host[12 * b:].copy_(flip)
            pack = host.to(dev, non_blocking=True)
            out = torch.empty(b, 3, tf.size, tf.size, device=dev, dtype=torch.float32)
            labels = torch.empty(b, device=dev, dtype=torch.int64)
            ops.call("fr_augment_u8_gather", store.data, store.labels, pack[:4 * b].view(torch.int32), xtab, ytab,
                     pack[4 * b:12 * b].view(torch.int32), pack[12 * b:], lut, out, labels, m, b, h, w, tf.big, tf.big,
                     tf.size, kx, ky, ops.current_stream_ptr())()
            yield out, labels
