"""GPU tests of the device-resident training set (frhip/resident.py, fr_augment_u8_gather in csrc/input_pipeline.hip; config
key GPU_RESIDENT_DATASET).  Every comparison is bit for bit, because the feature is defined as the GPU_INPUT_PIPELINE run:

  kernel            fr_augment_u8 on store[idx], in guarded buffers, repeated / unsorted / end-of-store indices, the labels
  addressing        a 4.3 GB store whose last slots lie beyond a 32-bit byte offset
  store build       the slots are the decoded files, a broken file keeps an invalid zero slot, size and memory refusals
  loader            every batch of two epochs == DataLoader + collate_fn_ignore_none + .to(device) + GpuTrainTransform
  steady state      one launch and one small host-to-device copy per batch, nothing back to the host
  train.py          same loss lines and checkpoints as the loader run, resume at the epoch boundary, two ranks, the refusal
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import head_support as HS

pytestmark = pytest.mark.gpu

SEED = 900


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _draws(tf, b, seed):
    crop, flip = tf.draw(b, torch.Generator().manual_seed(seed))
    span = tf.big - tf.size
    crop[0], crop[1] = torch.tensor([0, 0]), torch.tensor([span, span])  # the corners
    flip[0], flip[1] = 0, 1
    return crop, flip


def _gather(tf, store, labels, idx, crop, flip, out, label_out):
    from frhip import ops
    m, h, w, _ = store.shape
    b = idx.shape[0]
    xtab, ytab, lut, kx, ky = tf.tables(store.device, h, w)
    ops.call("fr_augment_u8_gather", store, labels, idx, xtab, ytab, crop.cuda(), flip.cuda(), lut, out, label_out, m, b, h, w,
             tf.big, tf.big, tf.size, kx, ky, ops.current_stream_ptr())()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the kernel


@pytest.mark.parametrize("h,w,size", [(112, 112, 112), (97, 131, 112), (64, 64, 56)])
def test_gather_is_the_sibling_on_the_gathered_images(h, w, size):
    _need_gpu()
    from frhip.input_pipeline import GpuTrainTransform
    M, idx_list = 13, [12, 0, 5, 5, 12, 3, 1, 0, 7]  # repeats, both ends of the store, unsorted
    B = len(idx_list)
    rng = np.random.default_rng(h * 1000 + w)
    store = torch.from_numpy(rng.integers(0, 256, (M, h, w, 3), dtype=np.uint8)).cuda()
    before = store.clone()
    labels = torch.from_numpy(rng.integers(0, 2 ** 40, M, dtype=np.int64)).cuda()  # values that need all 64 bits
    idx = torch.tensor(idx_list, dtype=torch.int32).cuda()
    tf = GpuTrainTransform(size)
    crop, flip = _draws(tf, B, 3)
    want = tf(store[idx.long()], crop, flip)
    assert want.shape == (B, 3, size, size)

    out, lab = HS.Guarded(B, 3, size, size), HS.Guarded(2 * B)
    label_out = lab.t.view(torch.int64)
    _gather(tf, store, labels, idx, crop, flip, out.t, label_out)
    assert torch.equal(out.t, want), float((out.t - want).abs().max())
    assert torch.equal(label_out, labels[idx.long()])
    out.assert_guards("out")
    lab.assert_guards("label_out")
    assert torch.equal(store, before)

    again = HS.Guarded(B, 3, size, size)
    _gather(tf, store, None, idx, crop, flip, again.t, None)  # no labels at either end
    assert torch.equal(again.t, want)
    again.assert_guards("out, null labels")


def test_gather_addresses_a_store_beyond_4_gib():
    """Slot 114 131 of a 112x112 store is the first whose byte offset (114 131 * 37 632) exceeds 2^32; a 32-bit product would
    read from slots 0 and 8 instead, which hold other bytes."""
    _need_gpu()
    if torch.cuda.mem_get_info()[0] < 6e9:
        pytest.skip("needs 6 GB of free device memory")
    from frhip.input_pipeline import GpuTrainTransform
    M, first_past = 114140, 114131
    per = 112 * 112 * 3
    assert (first_past - 1) * per < 2 ** 32 < first_past * per and M * per > 4.29e9
    store = torch.empty(M, 112, 112, 3, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(7)
    low = list(range(10))  # where the wrapped offsets of the two high slots would land (slots 0 and 8), and around them
    for slot in low + [first_past, M - 1]:
        store[slot] = torch.from_numpy(rng.integers(0, 256, (112, 112, 3), dtype=np.uint8)).cuda()
    labels = torch.arange(M, dtype=torch.int64, device="cuda") * 3 + 1
    idx_list = [M - 1, first_past, 0, M - 1]
    idx = torch.tensor(idx_list, dtype=torch.int32).cuda()
    tf = GpuTrainTransform(112)
    crop, flip = _draws(tf, 4, 11)
    want = tf(torch.stack([store[i] for i in idx_list]), crop, flip)
    assert not torch.equal(want[0], want[2]) and not torch.equal(want[1], want[2])
    out, lab = HS.Guarded(4, 3, 112, 112), HS.Guarded(8)
    _gather(tf, store, labels, idx, crop, flip, out.t, lab.t.view(torch.int64))
    assert torch.equal(out.t, want), float((out.t - want).abs().max())
    assert lab.t.view(torch.int64).tolist() == [3 * i + 1 for i in idx_list]
    out.assert_guards("out")
    lab.assert_guards("label_out")


# ------------------------------------------------------------------------------------------------ store and loader


def _write_faces(root, size=112):
    """3 identities x 4 PNG files plus one broken file: ({path: pixels}, the broken path)."""
    from PIL import Image
    want = {}
    for ident in ("id_b", "id_a", "id_c"):
        os.makedirs(root / ident)
        for k in range(4):
            a = np.random.default_rng(len(want)).integers(0, 256, (size, size, 3), dtype=np.uint8)
            Image.fromarray(a).save(root / ident / ("%d.png" % k))
            want[str(root / ident / ("%d.png" % k))] = a
    broken = root / "id_b" / "1_broken.png"
    broken.write_bytes(b"not an image")
    return want, str(broken)


@pytest.fixture(scope="module")
def faces(tmp_path_factory):
    """(dataset, store, {path: pixels}, the broken path) of the fixture directory, built once with two workers."""
    _need_gpu()
    from dataset import FacesDataset, StageTransform
    from frhip.resident import ResidentStore
    root = tmp_path_factory.mktemp("faces")
    want, broken = _write_faces(root)
    ds = FacesDataset(str(root), StageTransform(), extensions=(".png",))
    state = torch.get_rng_state()
    store = ResidentStore.build(ds, "cuda", 2)
    assert torch.equal(torch.get_rng_state(), state)  # the pass leaves the global generator alone
    return ds, store, want, broken


def test_store_holds_the_decoded_files(faces, tmp_path, capsys):
    from dataset import FacesDataset, StageTransform
    from frhip.resident import ResidentStore
    ds, store, want, broken = faces
    assert len(ds) == 13 and len(store) == 13 and ds.classes == ["id_a", "id_b", "id_c"]
    assert store.data.is_cuda and store.data.dtype == torch.uint8 and tuple(store.data.shape) == (13, 112, 112, 3)
    assert store.labels.is_cuda and store.labels.dtype == torch.int64 and tuple(store.labels.shape) == (13,)
    data, labels = store.data.cpu().numpy(), store.labels.cpu().tolist()
    for i, fn in enumerate(ds.filenames):
        if fn == broken:
            assert not store.valid[i] and not data[i].any()
            continue
        assert store.valid[i] and np.array_equal(data[i], want[fn]), fn
        assert labels[i] == ds.classes.index(fn.split(os.sep)[-2])
    assert int(store.valid.sum()) == 12
    capsys.readouterr()

    ResidentStore.build(ds, "cuda", 0)
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Resident dataset:")]
    assert len(line) == 1 and "13 images, 1 failed samples" in line[0] and " GB, " in line[0] and line[0].endswith(" s")

    with pytest.raises(ValueError, match=r"need 0\.000489 GB, the limit \(max_gb\) is 0\.000001 GB"):
        ResidentStore.build(ds, "cuda", 0, max_gb=1e-6)

    from PIL import Image
    odd_root = tmp_path / "odd"
    _write_faces(odd_root)
    Image.fromarray(np.zeros((96, 96, 3), np.uint8)).save(odd_root / "id_b" / "2_small.png")
    odd = FacesDataset(str(odd_root), StageTransform(), extensions=(".png",))
    at = odd.filenames.index(str(odd_root / "id_b" / "2_small.png"))
    with pytest.raises(ValueError, match=r"sample %d \(.*2_small\.png\) is 96x96, the set is 112x112" % at):
        ResidentStore.build(odd, "cuda", 0)


@pytest.mark.parametrize("world,rank", [(1, 0), (2, 1)])
@pytest.mark.parametrize("drop_last", [False, True])
def test_loader_equals_the_loader_path_bit_for_bit(faces, drop_last, world, rank, capsys):
    from frhip.input_pipeline import GpuTrainTransform
    from frhip.resident import ResidentLoader
    from util.utils import collate_fn_ignore_none
    ds, store, _want, _broken = faces
    dev = store.data.device

    def reseed(gen, epoch):  # train.py's per-epoch re-seeding of aug_rng
        gen.manual_seed(SEED + 7919 * rank + 104729 * (epoch + 1))

    tf_a, rng_a = GpuTrainTransform(112), torch.Generator()
    sampler = torch.utils.data.distributed.DistributedSampler(ds, world, rank, shuffle=True, seed=SEED)
    loader = torch.utils.data.DataLoader(ds, batch_size=5, sampler=sampler, shuffle=False, num_workers=0,
                                         drop_last=drop_last, collate_fn=collate_fn_ignore_none)
    torch.manual_seed(41)
    want = []
    for epoch in range(2):
        sampler.set_epoch(epoch)
        reseed(rng_a, epoch)
        for inputs, labels in loader:
            inputs, labels = inputs.to(dev, non_blocking=True), labels.to(dev, non_blocking=True).long()
            want.append((tf_a(inputs, generator=rng_a), labels))
    state_a = torch.get_rng_state()

    tf_b, rng_b = GpuTrainTransform(112), torch.Generator()
    resident = ResidentLoader(store, tf_b, 5, drop_last, world, rank, SEED, generator=rng_b)
    assert len(resident) == len(loader)
    torch.manual_seed(41)
    got = []
    for epoch in range(2):
        resident.set_epoch(epoch)
        reseed(rng_b, epoch)
        got += list(resident)
    assert torch.equal(torch.get_rng_state(), state_a)  # the global generator moved as under the DataLoader
    capsys.readouterr()

    assert len(got) == len(want) == 2 * len(loader) and len(want) > 0
    for k, ((x, y), (xw, yw)) in enumerate(zip(got, want)):
        assert x.is_cuda and y.is_cuda and x.dtype == torch.float32 and y.dtype == torch.int64
        assert x.shape == xw.shape and torch.equal(y, yw), (k, y.tolist(), yw.tolist())
        assert torch.equal(x, xw), (k, float((x - xw).abs().max()))
    if world == 1:  # the broken file falls into some batch of each epoch: that batch was refilled
        assert sum(x.shape[0] for x, _ in got) == 2 * (13 if not drop_last else 10)


def test_steady_state_is_one_launch_and_one_small_copy_per_batch(monkeypatch):
    _need_gpu()
    from frhip.input_pipeline import GpuTrainTransform
    from frhip.resident import ResidentLoader, ResidentStore
    M, B, N = 240, 20, 10
    rng = np.random.default_rng(5)
    store = ResidentStore(torch.from_numpy(rng.integers(0, 256, (M, 112, 112, 3), dtype=np.uint8)).cuda(),
                          torch.arange(M, dtype=torch.int64).cuda(), np.ones(M, dtype=bool))
    loader = ResidentLoader(store, GpuTrainTransform(112), B, True, 1, 0, SEED, generator=torch.Generator().manual_seed(1))
    assert len(loader) == 12
    it = iter(loader)
    next(it)  # the first batch: tables, allocator, pinned block
    torch.cuda.synchronize()

    # what the profiler calls a copy of either direction, taken from controls: a pageable pair (the names the shared
    # harness looks for) and the loader's own kind, an asynchronous copy out of pinned memory
    one, pinned = torch.ones(1, device="cuda"), torch.ones(260, dtype=torch.uint8).pin_memory()
    control = HS.profiled_names(lambda: (one.cpu(), torch.ones(4).to("cuda")))
    assert any("DtoH" in n for n in control) and any("HtoD" in n for n in control), sorted(set(control))
    idle = HS.profiled_names(lambda: None)

    def copy_names(fn):
        return set(n for n in HS.profiled_names(fn) if n not in idle and not n.startswith("aten::")
                   and ("copy" in n.lower() or "memcpy" in n.lower()))

    up = copy_names(lambda: pinned.to("cuda", non_blocking=True)) | copy_names(lambda: torch.ones(4).to("cuda"))
    down = copy_names(lambda: one.to("cpu", non_blocking=True)) | copy_names(lambda: one.cpu())
    assert up and down - up, (sorted(up), sorted(down))  # each direction shows, and the way back under a name of its own

    shipped = []
    to = torch.Tensor.to

    def counting_to(self, *a, **kw):
        res = to(self, *a, **kw)
        if not self.is_cuda and res.is_cuda:
            shipped.append(self.numel() * self.element_size())
        return res

    monkeypatch.setattr(torch.Tensor, "to", counting_to)
    batches = []
    names = HS.profiled_names(lambda: batches.extend(next(it) for _ in range(N)))
    monkeypatch.undo()
    assert len(batches) == N and all(x.shape == (B, 3, 112, 112) and y.shape == (B,) for x, y in batches)
    assert sum("augment_u8_gather_kernel" in n for n in names) == N, sorted(set(names))
    bad = [n for n in names if "augment_u8_kernel" in n or "DtoH" in n or n in HS.HOST_READS
           or "StreamSynchronize" in n or "EventSynchronize" in n]
    assert not bad, sorted(set(bad))
    # device synchronisations: the harness's own (its torch.cuda.synchronize() and the profiler's), as in an empty run
    assert sum("DeviceSynchronize" in n for n in names) == sum("DeviceSynchronize" in n for n in idle), (names, idle)
    assert not [n for n in names if n in down - up], sorted(set(names))  # nothing goes back to the host
    seen = {n: names.count(n) for n in up if n in names}
    # every host-to-device copy went through the counted call: one per batch, under each name such a copy has
    assert seen and set(seen.values()) == {N} and len(shipped) == N, (seen, shipped, sorted(set(names)))
    assert sum(shipped) <= 32 * B * N, shipped


# ------------------------------------------------------------------------------------------------ train.py

LOADER = dict(HEAD_NAME="ArcFace", GPU_INPUT_PIPELINE=True)
RESIDENT = dict(LOADER, GPU_RESIDENT_DATASET=True)
STATE_KEYS = ("epoch", "batch", "dropout_stream", "epoch_finished", "lr_stage_applied", "torch_rng", "numpy_rng")


def _loss_lines(log):
    return [l for l in log.splitlines() if "Training Loss" in l]


def _assert_same_state_file(a_dir, b_dir, last):
    sa = torch.load(HS.ckpt(a_dir, "State_ArcFace_" + last), map_location="cpu")
    sb = torch.load(HS.ckpt(b_dir, "State_ArcFace_" + last), map_location="cpu")
    assert list(sa.keys()) == list(sb.keys()) and all(k in sa for k in STATE_KEYS), (list(sa.keys()), list(sb.keys()))
    for key in sa:
        same = torch.equal(sa[key], sb[key]) if torch.is_tensor(sa[key]) else sa[key] == sb[key]
        assert same, ("State_", key)


@pytest.fixture(scope="module")
def resident_runs(tmp_path_factory):
    """Two epochs of the resident run straight, and stopped at the epoch boundary and resumed (``HS.resumed`` compares the
    two end states bit for bit)."""
    _need_gpu()
    return HS.resumed(tmp_path_factory.mktemp("resident"), RESIDENT, "ArcFace")


def test_train_resumes_bit_for_bit(resident_runs):
    r = resident_runs  # the body of HS.straight_and_resumed on the shared runs
    losses = [float(m.group(1)) for m in re.finditer(r"Training Loss ([0-9.eE+-]+|nan|inf) \(", r.a_log)]
    assert len(losses) == 12 and all(np.isfinite(losses)), "%s\n%s" % (losses, r.a_log[-2000:])
    assert "Prec@1" in r.a_log and "nan" not in r.a_log.lower(), r.a_log[-2000:]
    assert r.a_log.count("Resident dataset: 120 images, 0 failed samples") == 1
    _assert_same_state_file(r.a_dir, r.b2_dir, "Epoch_2_Batch_12_")


def test_train_equals_the_loader_run(resident_runs, tmp_path):
    r = resident_runs
    l_dir, l_log = HS.run_train(tmp_path, "loader", LOADER)
    assert "Resident dataset" not in l_log
    assert len(_loss_lines(l_log)) == 14 and _loss_lines(l_log) == _loss_lines(r.a_log), (l_log[-1500:], r.a_log[-1500:])
    for last in ("Epoch_1_Batch_6_", "Epoch_2_Batch_12_"):
        HS.assert_same_checkpoints(l_dir, r.a_dir, "ArcFace", last)
        _assert_same_state_file(l_dir, r.a_dir, last)


def _two_ranks(tmp_path, tag, cfg, port):
    env = dict(os.environ, PYTHONPATH=HS.PRODUCT, FRHIP_TRAIN_ONE_DEVICE="1", FRHIP_DIST_BACKEND="gloo",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    model_dir = tmp_path / tag
    script = tmp_path / ("run_%s.py" % tag)
    script.write_text(
        "import sys, runpy\n"
        "import configs.config_synthetic_smoke as c\n"
        "c.configurations[1].update(BATCH_SIZE=10, NUM_EPOCH=1, MODEL_ROOT=r'%s', LOG_ROOT=r'%s', **%r)\n"
        "sys.argv = ['train.py', '--config', 'configs/config_synthetic_smoke.py', '--synthetic', '12x10']\n"
        "runpy.run_path('train.py', run_name='__main__')\n" % (model_dir, tmp_path / "log", cfg))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), str(script)]
    out = HS.child(cmd, HS.PRODUCT, env, 900)
    assert out.returncode == 0, out.stdout[-2500:] + out.stderr[-2500:]
    return model_dir, out.stdout


def test_train_two_ranks_equal_the_loader_run(tmp_path):
    """Both ranks on GPU 0 with gloo, each holding the whole set and drawing its own half of every epoch."""
    _need_gpu()
    l_dir, l_log = _two_ranks(tmp_path, "loader2", LOADER, 29593)
    r_dir, r_log = _two_ranks(tmp_path, "resident2", RESIDENT, 29594)
    assert r_log.count("Resident dataset: 120 images") == 2 and "Resident dataset" not in l_log
    assert len(_loss_lines(l_log)) == 7 and _loss_lines(l_log) == _loss_lines(r_log), (l_log[-1500:], r_log[-1500:])
    HS.assert_same_checkpoints(l_dir, r_dir, "ArcFace", "Epoch_1_Batch_6_")
    _assert_same_state_file(l_dir, r_dir, "Epoch_1_Batch_6_")


def test_train_refuses_the_resident_set_without_the_gpu_transform(tmp_path):
    _need_gpu()
    out = HS.run_train(tmp_path, "refused", dict(HEAD_NAME="ArcFace", GPU_RESIDENT_DATASET=True), max_steps=1, ok=False,
                       limit=120)
    assert out.returncode != 0 and "GPU_RESIDENT_DATASET=True needs GPU_INPUT_PIPELINE=True" in out.stderr, out.stderr[-1500:]
    assert "Number of Training Classes" not in out.stdout and "Resident dataset" not in out.stdout  # before any device work
