"""Host tests of the device-resident training set (no GPU): ``frhip.resident.epoch_batches`` against the index plan a real
``DataLoader(DistributedSampler, collate_fn_ignore_none)`` delivers, with negative controls the same comparison catches;
``len(ResidentLoader)``; the driver's config keys and the place of their check; the C ABI of ``fr_augment_u8_gather`` and
its argument checks, which run before any launch."""
import ctypes
import inspect
import itertools
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.distributed import DistributedSampler

SEED = 900
BATCH = 5


class _Own(Dataset):
    """A sample is its own index; the indices in ``holes`` fail to load."""

    def __init__(self, n, holes=()):
        self.n, self.holes = n, set(holes)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return None if i in self.holes else i


def _real_loader(n, holes, world, rank, drop_last):
    from util.utils import collate_fn_ignore_none
    ds = _Own(n, holes)
    sampler = DistributedSampler(ds, world, rank, shuffle=True, seed=SEED)
    return sampler, DataLoader(ds, batch_size=BATCH, sampler=sampler, shuffle=False, num_workers=0, drop_last=drop_last,
                               collate_fn=collate_fn_ignore_none)


def _recorded(n, holes, world, rank, drop_last, epoch):
    sampler, loader = _real_loader(n, holes, world, rank, drop_last)
    sampler.set_epoch(epoch)
    return [b.tolist() for b in loader], len(loader)


def _valid(n, holes):
    v = np.ones(n, dtype=bool)
    v[list(holes)] = False
    return v


def _two_of_five(n):
    """Holes that leave one batch of five with three survivors: the first two samples rank 0 of 1 draws in epoch 0."""
    plan, _ = _recorded(n, (), 1, 0, False, 0)
    return tuple(plan[0][:2])


CASES = [(n, holes, world, rank, drop_last, epoch)
         for n in (14, 23) for holes in ((), (0, 6, n - 1), _two_of_five(n))
         for world in (1, 2, 3) for rank in range(world) for drop_last in (False, True) for epoch in (0, 3)]


def test_epoch_batches_is_the_index_plan_of_the_real_loader(capsys):
    from frhip.resident import ResidentLoader, ResidentStore, epoch_batches
    grown = 0
    for n, holes, world, rank, drop_last, epoch in CASES:
        want, want_len = _recorded(n, holes, world, rank, drop_last, epoch)
        valid = _valid(n, holes)
        got = epoch_batches(n, valid, world, rank, SEED, epoch, BATCH, drop_last)
        assert got == want, (n, holes, world, rank, drop_last, epoch, got, want)
        assert all(valid[i] for b in got for i in b)
        loader = ResidentLoader(ResidentStore(None, None, valid), None, BATCH, drop_last, world, rank, SEED)
        assert len(loader) == want_len == len(got), (n, holes, world, rank, drop_last, len(loader), want_len)
        grown += sum(len(b) > BATCH for b in got)
    capsys.readouterr()  # the collate's own prints
    assert grown > 0  # the refill loop's growth is among the cases ...
    n = 14
    got = epoch_batches(n, _valid(n, _two_of_five(n)), 1, 0, SEED, 0, BATCH, False)
    assert len(got[0]) == 7 and got[0][3:5] == got[0][:2] and got[0][5:] == got[0][:2]  # ... 3 survivors -> 5 -> 7


def test_refill_rule_is_the_collate_rule(capsys):
    from frhip.resident import refill_ignore_none
    from util.utils import collate_fn_ignore_none
    for k in range(1, 7):
        for pattern in itertools.product((True, False), repeat=k):
            if not any(pattern):
                continue
            batch = [10 + i if ok else None for i, ok in enumerate(pattern)]
            assert refill_ignore_none(batch) == collate_fn_ignore_none(batch).tolist(), batch
    capsys.readouterr()


def test_negative_controls_differ_from_the_recorded_plan(capsys):
    from frhip.resident import epoch_batches
    n, holes = 23, (0, 6, 22)
    want, _ = _recorded(n, holes, 1, 0, False, 3)
    valid = _valid(n, holes)
    assert epoch_batches(n, valid, 1, 0, SEED, 3, BATCH, False) == want
    # a plan that drops the holes without refilling
    no_refill = [[i for i in b if valid[i]] for b in epoch_batches(n, np.ones(n, dtype=bool), 1, 0, SEED, 3, BATCH, False)]
    assert no_refill != want
    # a plan that ignores set_epoch
    assert epoch_batches(n, valid, 1, 0, SEED, 0, BATCH, False) != want
    capsys.readouterr()


def test_loader_refuses_an_index_outside_the_store():
    """The range check is made on host data before anything touches the device: a store whose ``valid`` is longer than its
    data (a stub here, with an object that only has a shape) raises ValueError, not a device error."""
    from frhip.resident import ResidentLoader, ResidentStore

    class _Shape(object):
        shape, device = (4, 112, 112, 3), torch.device("cpu")

    class _Tf(object):
        size = big = 112

        def tables(self, dev, h, w):
            return None, None, None, 1, 1

    store = ResidentStore(_Shape(), None, np.ones(9, dtype=bool))
    with pytest.raises(ValueError, match=r"outside \[0, 4\)"):
        next(iter(ResidentLoader(store, _Tf(), BATCH, False, 1, 0, SEED)))


def test_config_validation():
    import train
    for ok in ({}, {"GPU_RESIDENT_DATASET": False}, {"GPU_INPUT_PIPELINE": True},
               {"GPU_INPUT_PIPELINE": True, "GPU_RESIDENT_DATASET": True},
               {"GPU_INPUT_PIPELINE": True, "GPU_RESIDENT_DATASET": True, "GPU_RESIDENT_MAX_GB": 60},
               {"GPU_INPUT_PIPELINE": True, "GPU_RESIDENT_DATASET": True, "GPU_RESIDENT_MAX_GB": 0.5}):
        assert train.check_input_config(ok) is None
    with pytest.raises(NotImplementedError, match="GPU_RESIDENT_DATASET=True needs GPU_INPUT_PIPELINE=True: the resident "
                                                  "set feeds the GPU transform"):
        train.check_input_config({"GPU_RESIDENT_DATASET": True})
    with pytest.raises(NotImplementedError, match="feeds the GPU transform"):
        train.check_input_config({"GPU_RESIDENT_DATASET": True, "GPU_INPUT_PIPELINE": False})
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="GPU_RESIDENT_DATASET must be True or False"):
            train.check_input_config({"GPU_INPUT_PIPELINE": True, "GPU_RESIDENT_DATASET": bad})
    for bad in (0, -1, -0.5, True, "8", float("nan")):
        with pytest.raises(ValueError, match="GPU_RESIDENT_MAX_GB must be None or a number greater than 0"):
            train.check_input_config({"GPU_INPUT_PIPELINE": True, "GPU_RESIDENT_DATASET": True,
                                      "GPU_RESIDENT_MAX_GB": bad})
    common = open(os.path.join(os.path.dirname(train.__file__), "configs", "_common.py")).read()
    assert "GPU_RESIDENT_DATASET=False" in common and "GPU_RESIDENT_MAX_GB=None" in common
    from configs._common import stage3
    assert train.check_input_config(stage3("x")) is None  # the shipped defaults are off


def test_main_checks_the_input_config_before_anything_is_built():
    import train
    src = inspect.getsource(train.main)
    assert src.index("check_head_config(cfg)") < src.index("check_input_config(cfg)") < src.index("build_backbone(cfg)")
    assert src.index("check_input_config(cfg)") < src.index("torch.cuda.is_available()")  # before any device work
    assert src.index("num_class = len(dataset.classes)") < src.index("ResidentStore.build(") < src.index("build_backbone(cfg)")
    assert "(loader if resident else sampler).set_epoch(epoch)" in src


def test_c_abi_of_the_gather_entry():
    from frhip import _lib
    lib = _lib.lib
    header = open(_lib.HEADER).read()
    name = "fr_augment_u8_gather"
    assert "int %s(" % name in header and name in _lib.protos and hasattr(lib, name)
    assert _lib.protos[name][2] == ["store", "labels", "idx", "xtab", "ytab", "crop", "flip", "lut", "out", "label_out", "M",
                                    "B", "Hin", "Win", "Hr", "Wr", "S", "kx", "ky", "stream"]
    assert _lib.protos[name][1] == [ctypes.c_void_p] * 10 + [ctypes.c_int] * 9 + [ctypes.c_void_p]
    # the sibling keeps its signature
    assert _lib.protos["fr_augment_u8"][2] == ["src", "xtab", "ytab", "crop", "flip", "lut", "out", "B", "Hin", "Win", "Hr",
                                               "Wr", "S", "kx", "ky", "stream"]
    assert lib.fr_abi_version() == 7 and "#define FR_ABI_VERSION 7" in header


def test_gather_entry_refuses_before_any_launch():
    """Every refusal returns before the launch, so host pointers (never dereferenced) stand in for device ones."""
    from frhip import _lib
    lib = _lib.lib
    mem = ctypes.create_string_buffer(64)
    p = ctypes.cast(mem, ctypes.c_void_p)

    def call(M=13, B=9, Hin=112, Win=112, Hr=128, Wr=128, S=112, kx=3, ky=3, store=p, idx=p, out=p, labels=p, label_out=p):
        return lib.fr_augment_u8_gather(store, labels, idx, p, p, p, p, p, out, label_out, M, B, Hin, Win, Hr, Wr, S, kx, ky,
                                        None)

    def refused(rc):
        assert rc < 0, rc
        assert b"fr_augment_u8_gather" in lib.fr_last_error_string(), lib.fr_last_error_string()

    assert call(B=0) == 0 and call(B=-3) == 0
    assert call(B=0, M=0, store=None, idx=None, out=None) == 0  # the empty batch is served whatever else is passed
    refused(call(M=0))
    refused(call(M=-1))
    refused(call(S=129))  # S > Hr
    refused(call(S=120, Wr=112))  # S > Wr
    for zero in ("Hin", "Win", "S", "kx", "ky"):
        refused(call(**{zero: 0}))
    refused(call(B=65536))
    assert b"65535" in lib.fr_last_error_string()
    for hole in ("store", "idx", "out"):
        refused(call(**{hole: None}))
        assert b"required" in lib.fr_last_error_string()
