"""datasets.py: the device-resident image datasets. CPU: the epoch plan (class segregation, drop_remainder,
labels, shuffles, shards, noise offsets) with device='cpu', where an image's pixels spell its number. GPU:
the batches through the model -- train_step and anneal_and_fit on a dataset against the same batches
assembled by hand with base_functions, bit for bit."""
import numpy as np
import pytest
import torch

from arl_conditional_normalizing_flows_amd.datasets import ClassConditionalDataset, SuperResolutionDataset


def _numbered(n, start=0, H=4, C=1):
    """n images whose every pixel is (start + i) / 64: exact in fp32, so the image can be read back."""
    v = (np.arange(start, start + n, dtype=np.float32) / 64.0)[:, None, None, None]
    return np.broadcast_to(v, (n, H, H, C)).copy()


def _ids(batch):
    return [int(round(float(v) * 64)) for v in batch[:, 0, 0, 0]]


# ---------------------------------------------------------------------------------------------
# CPU: the plan
# ---------------------------------------------------------------------------------------------
CLASSES = [_numbered(7, 0), _numbered(5, 10), _numbered(9, 20)]        # image numbers 0-6, 10-14, 20-28


def _class_ds(**kw):
    kw.setdefault('base_alpha', 1.0)      # noise off: pixels stay readable
    return ClassConditionalDataset(CLASSES, 2, device='cpu', **kw)


def test_class_plan_segregates_drops_and_shuffles_batches():
    ds = _class_ds(seed=3)
    assert len(ds) == 3 + 2 + 4
    epochs = []
    for _ in range(2):
        ep = ds()
        assert len(ep) == 9
        batches = list(ep)
        assert all(b.shape == (2, 4, 4, 2) for b in batches)
        seen = []
        for b in batches:
            ids, lab = _ids(b), b[..., 1]
            k = ids[0] // 10
            assert all(i // 10 == k for i in ids)                              # one class per batch
            assert ids[1] == ids[0] + 1 and (ids[0] % 10) % 2 == 0               # stored order inside a class
            assert bool((lab == [0.0, 0.5, 1.0][k]).all())
            seen += ids
        # the dropped images are the last of each class: 6, 14 and 28
        assert sorted(seen) == list(range(0, 6)) + list(range(10, 14)) + list(range(20, 28))
        epochs.append([tuple(_ids(b)) for b in batches])
    assert epochs[0] != epochs[1]                                              # the batch order is reshuffled
    again = _class_ds(seed=3)
    assert [[tuple(_ids(b)) for b in again()] for _ in range(2)] == epochs     # and repeats for the same seed
    assert [tuple(_ids(b)) for b in _class_ds(seed=4)()] != epochs[0]


def test_class_labels_default_and_given():
    one = ClassConditionalDataset([_numbered(4)], 2, base_alpha=1.0, device='cpu')
    assert all(bool((b[..., 1] == 0.0).all()) for b in one())                  # a single class gets 0
    ds = _class_ds(labels=[0.25, 2.0, -1.0], shuffle=False)
    for b in ds():
        assert bool((b[..., 1] == [0.25, 2.0, -1.0][_ids(b)[0] // 10]).all())


def test_class_logits_match_the_oracle():
    from oracle import transforms_np as T
    x = np.random.default_rng(0).random((4, 4, 4, 3)).astype(np.float32)
    ds = ClassConditionalDataset([x], 4, logits=True, a=0.05, base_alpha=1.0, shuffle=False, device='cpu')
    (b,) = list(ds())
    assert float(np.max(np.abs(b[..., :3].numpy() - T.logit_preprocess(x.astype(np.float64), 0.05)))) < 1e-5


def test_sr_plan_shuffles_examples_and_keeps_a_short_batch():
    from oracle import transforms_np as T
    imgs = _numbered(7)
    ds = SuperResolutionDataset(imgs, 3, residual=False, base_alpha=1.0, seed=1, device='cpu')
    assert len(ds) == 3
    orders = []
    for _ in range(2):
        batches = list(ds())
        assert [b.shape for b in batches] == [(3, 4, 4, 2), (3, 4, 4, 2), (1, 4, 4, 2)]
        orders.append([i for b in batches for i in _ids(b)])
        assert sorted(orders[-1]) == list(range(7))                            # a permutation of all 7
    assert orders[0] != orders[1]
    # the values: preprocess_dataset_SR of the gathered images
    x = np.random.default_rng(5).random((2, 8, 8, 3)).astype(np.float32)
    ds = SuperResolutionDataset(x, 2, model_type='SR4,2', y_levels=1, base_alpha=1.0, shuffle=False, seed=0,
                                device='cpu')
    (b,) = list(ds())
    order = np.random.Generator(np.random.Philox(key=[0, 0])).permutation(2)
    assert float(np.max(np.abs(b.numpy() - T.sr_preprocess(x[order].astype(np.float64), 1, 1, True)))) < 1e-6


@pytest.mark.parametrize('kind', ['class', 'sr'])
def test_shards_interleave_to_the_unsharded_epoch(kind):
    def make(shard):
        if kind == 'class':
            return ClassConditionalDataset(CLASSES, 2, seed=7, shard=shard, device='cpu')       # 9 batches
        return SuperResolutionDataset(_numbered(14, H=4), 3, seed=7, shard=shard, device='cpu')  # 5 batches
    whole, r0, r1 = make(None), make((0, 2)), make((1, 2))
    n = len(whole) // 2
    assert len(r0) == len(r1) == n
    for _ in range(2):                                    # noise on: offsets carry on across epochs on every rank
        w, a, b = list(whole()), list(r0()), list(r1())
        assert len(a) == len(b) == n
        inter = [t for pair in zip(a, b) for t in pair]
        assert all(torch.equal(u, v) for u, v in zip(inter, w[:2 * n]))


def test_renew_noise_restarts_or_carries_the_offsets():
    def two_epochs(**kw):
        ds = ClassConditionalDataset(CLASSES, 2, shuffle=False, device='cpu', **kw)
        return [torch.stack(list(ds())) for _ in range(2)]
    e0, e1 = two_epochs(renew_noise=False)
    assert torch.equal(e0, e1)
    f0, f1 = two_epochs(renew_noise=True)
    assert torch.equal(f0, e0) and not torch.equal(f0, f1)
    assert 0.001 < float((f0 - f1).std()) < 0.1           # two draws of the 2 % noise apart


def test_with_noise_view_restarts_stage_one_and_shares_the_epoch():
    from arl_conditional_normalizing_flows_amd.datasets import _noise_cpu
    ds = ClassConditionalDataset(CLASSES, 2, seed=2, renew_noise=False, device='cpu')
    view = ds.with_noise(0.5, seed=9, offset=40)
    assert len(view) == len(ds)
    a, b = list(view()), list(ds())                        # epochs 0 and 1 of one sequence
    other = ClassConditionalDataset(CLASSES, 2, seed=2, renew_noise=False, device='cpu')
    c, d = list(other()), list(other())
    assert all(torch.equal(u, v) for u, v in zip(b, d))    # the view advanced the shared epoch counter
    # stage 1 is instance_noise of the plain batch, its offset advancing by the batch's element count
    for k, (u, v) in enumerate(zip(a, c)):
        assert torch.equal(u, _noise_cpu(v, 0.5, 9, 40 + k * v.numel()))
    fixed = ClassConditionalDataset(CLASSES, 2, seed=2, shuffle=False, renew_noise=False, device='cpu').with_noise(0.5, 9)
    assert all(torch.equal(u, v) for u, v in zip(fixed(), fixed()))            # and restarts on every call
    with pytest.raises(ValueError):
        ds.with_noise(1.5, seed=0)


def test_bad_arguments_raise_value_error():
    with pytest.raises(ValueError):
        ClassConditionalDataset(CLASSES, 6, device='cpu')                       # a class of 5 < batch_size
    with pytest.raises(ValueError):
        ClassConditionalDataset(CLASSES, 2, shard=(2, 2), device='cpu')
    with pytest.raises(ValueError):
        ClassConditionalDataset(CLASSES, 2, shard=(0, 0), device='cpu')
    with pytest.raises(ValueError):
        ClassConditionalDataset(CLASSES, 0, device='cpu')
    with pytest.raises(ValueError):
        ClassConditionalDataset(CLASSES, 2, labels=[0.0, 1.0], device='cpu')
    with pytest.raises(ValueError):
        ClassConditionalDataset(CLASSES, 2, logits=True, a=0.5, device='cpu')
    with pytest.raises(ValueError):
        ClassConditionalDataset([_numbered(4), _numbered(4, H=8)], 2, device='cpu')
    with pytest.raises(ValueError):
        ClassConditionalDataset(CLASSES, 2, base_alpha=1.5, device='cpu')
    with pytest.raises(ValueError):
        SuperResolutionDataset(_numbered(4, H=6), 2, y_levels=2, device='cpu')  # 6 not divisible by 4
    with pytest.raises(ValueError):
        SuperResolutionDataset(_numbered(4), 2, model_type='SR8,4', device='cpu')
    with pytest.raises(ValueError):
        SuperResolutionDataset(_numbered(4)[0], 2, device='cpu')                # not [N, H, W, C]
    with pytest.raises(ValueError):
        SuperResolutionDataset(_numbered(3), 2, shard=(0, 4), device='cpu')     # 2 batches over 4 ranks


def test_from_tfrecords(tmp_path):
    from arl_conditional_normalizing_flows_amd.tfrecords import make_tfrecord
    paths = []
    for k, x in enumerate(CLASSES):
        paths.append(str(tmp_path / f'class{k}.tfrecord'))
        make_tfrecord(x, np.eye(3, dtype=np.float32)[[k] * len(x)], paths[-1])
    a = ClassConditionalDataset.from_tfrecords(paths, 2, seed=5, device='cpu')
    b = ClassConditionalDataset(CLASSES, 2, seed=5, device='cpu')
    assert all(torch.equal(u, v) for u, v in zip(a(), b()))
    s = SuperResolutionDataset.from_tfrecords(paths[2], 4, seed=5, device='cpu')
    t = SuperResolutionDataset(CLASSES[2], 4, seed=5, device='cpu')
    assert len(s) == 3 and all(torch.equal(u, v) for u, v in zip(s(), t()))


# ---------------------------------------------------------------------------------------------
# GPU: through the model
# ---------------------------------------------------------------------------------------------
SEED, BS = 4, 2


def _tiny_classes():
    rng = np.random.default_rng(8)
    return [rng.random((5, 8, 8, 1)).astype(np.float32) for _ in range(3)]      # 2 batches per class, 1 dropped


class _HandBatches:
    """ClassConditionalDataset(shuffle=False)'s epochs assembled with the existing functions: the fixed batch
    order restated from the rule (Philox key [seed, 0] over the class-major batch list), gather,
    preprocess_dataset_class, the label plane, instance_noise(0.98) with its offsets kept by hand."""

    def __init__(self, classes, gpu, logits, renew_noise=True):
        from arl_conditional_normalizing_flows_amd import base_functions as F
        self.F, self.logits, self.renew = F, logits, renew_noise
        self.x = torch.from_numpy(np.concatenate(classes)).to(gpu)
        starts = np.cumsum([0] + [len(c) for c in classes])
        K = len(classes)
        plan = [(int(starts[k]) + j * BS, k / (K - 1)) for k in range(K) for j in range(len(classes[k]) // BS)]
        order = np.random.Generator(np.random.Philox(key=[SEED, 0])).permutation(len(plan))
        self.plan = [plan[i] for i in order]
        self.off = 0

    def __call__(self):
        out = []
        off = self.off if self.renew else 0
        for lo, lab in self.plan:
            v = self.F.preprocess_dataset_class(self.x[lo:lo + BS], LOGITS=self.logits, a=0.01)
            v = torch.cat([v, torch.full(v.shape[:3] + (1,), lab, device=v.device)], dim=-1)
            out.append(self.F.instance_noise(v, 0.98, seed=SEED, offset=off))
            off += v.numel()
        self.off = off
        return out


def _tiny_flow(gpu):
    from arl_conditional_normalizing_flows_amd.config import PRESETS
    from arl_conditional_normalizing_flows_amd.make_model import cFlow
    from arl_conditional_normalizing_flows_amd.optimizers import Adam
    flow = cFlow(**PRESETS['tiny'].kwargs(), device=gpu)                        # 8x8x2, x_d 1: class-shaped, C = 1
    flow.set_weights(flow.initial_weights(2))
    flow.compile(optimizer=Adam(learning_rate=1e-3))
    return flow


@pytest.mark.gpu
def test_two_train_steps_on_dataset_batches_equal_hand_batches(gpu):
    classes = _tiny_classes()
    ds = ClassConditionalDataset(classes, BS, logits=True, a=0.01, seed=SEED, shuffle=False, device=gpu)
    hand = _HandBatches(classes, gpu, logits=True)
    assert len(ds) == 6
    a, b = _tiny_flow(gpu), _tiny_flow(gpu)
    for _ in range(2):                                     # two epochs: the stage-0 offsets carry on
        got, ref = list(ds()), hand()
        assert len(got) == len(ref) and all(torch.equal(u, v) for u, v in zip(got, ref))
    for u, v in zip(got[:2], ref[:2]):
        a.train_step(u)
        b.train_step(v)
    assert torch.equal(a.params, b.params)
    assert not torch.equal(a.params, _tiny_flow(gpu).params)


@pytest.mark.gpu
def test_anneal_and_fit_fused_route_equals_the_wrapped_route(gpu):
    """anneal_and_fit on the datasets (noise stage 1 inside the batch-assembly launch, through with_noise)
    against hand-assembled batches that go through its instance_noise wrapper, same seeds: histories and
    final parameters bit for bit. shuffle=False is what makes this meaningful: the hand route has no
    dataset to ask for an epoch's order, it restates the one fixed order from the documented rule."""
    from arl_conditional_normalizing_flows_amd.training import Callback, anneal_and_fit
    classes = _tiny_classes()
    val_classes = [c[:2] for c in classes]
    kw = dict(logits=False, seed=SEED, shuffle=False, device=gpu)
    train, val = ClassConditionalDataset(classes, BS, **kw), ClassConditionalDataset(val_classes, BS, renew_noise=False,
                                                                                     **kw)
    assert hasattr(train, 'with_noise')
    hand_train = _HandBatches(classes, gpu, logits=False)
    hand_val = _HandBatches(val_classes, gpu, logits=False, renew_noise=False)
    class Record(Callback):                                # every epoch's logs, over the three fits
        def __init__(self):
            self.rows = []

        def on_epoch_end(self, epoch, logs=None):
            self.rows.append((epoch, dict(logs)))

    a, b, ra, rb = _tiny_flow(gpu), _tiny_flow(gpu), Record(), Record()
    anneal_and_fit(a, train, val, num_annealing_epochs=2, num_epochs=3, seed=5, callbacks=[ra])
    anneal_and_fit(b, lambda: hand_train(), lambda: hand_val(), num_annealing_epochs=2, num_epochs=3, seed=5,
                   callbacks=[rb])
    assert train._state['epoch'] == 3 and val._state['epoch'] == 3
    assert [e for e, _ in ra.rows] == [0, 1, 2] and all('val_loss' in r for _, r in ra.rows)
    assert ra.rows == rb.rows
    assert torch.equal(a.params, b.params)
