"""tools/trainer.py, tools/train.py and tools/summarize_logs.py without a device: triggers and the
lr schedule on a fake loop, extension order, LogReport windows, MaxValueTrigger; the ImageNet
ResNet import and the he_normal mask initialiser on CPU-constructed models."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import trainer as T  # noqa: E402


class _FakeIterator(object):
    def __init__(self, n, batch_size):
        self.dataset = list(range(n))
        self.batch_size = batch_size


class _FakeOptimizer(object):
    def __init__(self, lr):
        self.lr = lr
        self.flushes = 0

    def flush(self):
        self.flushes += 1


class _FakeChain(object):
    def __init__(self):
        self.report = {}


class _FakeLoop(object):
    """TrainLoop's surface: step() reports host numbers (the DictSummary host path)."""

    def __init__(self, n, batch_size, lr=0.01):
        self.iterator = _FakeIterator(n, batch_size)
        self.optimizer = _FakeOptimizer(lr)
        self.chain = _FakeChain()
        self.iteration = 0
        self.lrs = []

    def step(self):
        self.iteration += 1
        self.lrs.append(self.optimizer.lr)
        self.chain.report = {'loss': float(self.iteration), 'roi_cls_loss': 0.5 * self.iteration}


class _Probe(object):
    def __init__(self, name, calls, priority=None):
        self.name, self.calls = name, calls
        if priority is not None:
            self.priority = priority

    def __call__(self, trainer):
        self.calls.append((trainer.iteration, self.name))


def _fired(trigger, n, batch_size, iterations):
    tr = T.Trainer(_FakeLoop(n, batch_size), (iterations, 'iteration'), out='unused')
    out = []
    for _ in range(iterations):
        tr.updater.update()
        if trigger(tr):
            out.append(tr.iteration)
    return out


def test_epoch_detail_and_interval_triggers():
    tr = T.Trainer(_FakeLoop(5, 2), (1, 'epoch'), out='unused')
    details = []
    for _ in range(6):
        tr.updater.update()
        details.append((tr.epoch, tr.epoch_detail))
    assert details == [(0, 0.4), (0, 0.8), (1, 1 + 1 / 5), (1, 1 + 3 / 5), (2, 2.0), (2, 2 + 2 / 5)]
    # epochs of 2.5 iterations: boundaries crossed at iterations 3 and 5
    assert _fired(T.IntervalTrigger(1, 'epoch'), 5, 2, 10) == [3, 5, 8, 10]
    assert _fired(T.IntervalTrigger(0.5, 'epoch'), 5, 2, 5) == [2, 3, 4, 5]
    assert _fired(T.IntervalTrigger(1.5, 'epoch'), 5, 2, 10) == [4, 8]
    assert _fired(T.IntervalTrigger(3, 'iteration'), 5, 2, 10) == [3, 6, 9]


def test_manual_schedule_trigger_and_exponential_shift():
    assert _fired(T.ManualScheduleTrigger([0.5, 1.3], 'epoch'), 5, 2, 6) == [2, 4]
    assert _fired(T.ManualScheduleTrigger(4, 'iteration'), 5, 2, 6) == [4]
    loop = _FakeLoop(5, 2, lr=0.02)
    tr = T.Trainer(loop, (3, 'epoch'), out='unused')
    tr.extend(T.ExponentialShift('lr', 0.1), trigger=T.ManualScheduleTrigger([0.5, 1.3], 'epoch'))
    tr.run()
    # the shift after iteration 2 / 4 applies from the next update on: init * rate ** t
    assert loop.lrs == [0.02] * 2 + [0.02 * 0.1] * 2 + [0.02 * 0.1 ** 2] * 4
    assert tr.iteration == 8 and tr.epoch_detail == 3.2


def test_stop_trigger_fractional_epochs(tmp_path):
    loop = _FakeLoop(10, 2)
    tr = T.Trainer(loop, (1.25, 'epoch'), out=str(tmp_path))
    tr.run()
    assert tr.iteration == 7       # epoch_detail 1.4 is the first >= 1.25


def test_extension_order_priority_then_registration(tmp_path):
    calls = []
    tr = T.Trainer(_FakeLoop(4, 2), (2, 'iteration'), out=str(tmp_path))
    tr.extend(_Probe('reader_a', calls))                            # default: reader 100
    tr.extend(_Probe('snap', calls, T.PRIORITY_SNAPSHOT))
    tr.extend(_Probe('writer', calls, T.PRIORITY_WRITER))
    tr.extend(_Probe('reader_b', calls))
    tr.extend(_Probe('every2', calls, T.PRIORITY_WRITER), trigger=(2, 'iteration'))
    tr.run()
    assert calls == [(1, 'writer'), (1, 'reader_a'), (1, 'reader_b'), (1, 'snap'),
                     (2, 'writer'), (2, 'every2'), (2, 'reader_a'), (2, 'reader_b'), (2, 'snap')]


class _FakeEval(object):
    """Writes validation/main/map from a list, one value per call."""
    priority = T.PRIORITY_WRITER

    def __init__(self, maps):
        self.maps = list(maps)

    def __call__(self, trainer):
        trainer.observation['validation/main/map'] = np.float64(self.maps.pop(0))


def test_log_report_windows_and_validation_keys(tmp_path):
    loop = _FakeLoop(6, 2, lr=0.01)              # 3 iterations per epoch
    tr = T.Trainer(loop, (12, 'iteration'), out=str(tmp_path))
    tr.extend(_FakeEval([0.1, 0.2, 0.3, 0.4]), trigger=(1, 'epoch'))
    tr.extend(T.observe_lr(), trigger=(4, 'iteration'))
    tr.extend(T.LogReport(trigger=(4, 'iteration')))
    tr.run()
    with open(os.path.join(str(tmp_path), 'log')) as f:
        log = json.load(f)
    assert [e['iteration'] for e in log] == [4, 8, 12]
    assert [e['epoch'] for e in log] == [1, 2, 4]
    assert [e['main/loss'] for e in log] == [2.5, 6.5, 10.5]
    assert [e['main/roi_cls_loss'] for e in log] == [1.25, 3.25, 5.25]
    assert [e['lr'] for e in log] == [0.01] * 3
    # evaluations at iterations 3, 6, 9, 12: windows (0,4] (4,8] (8,12] hold 1, 1, 2 of them
    assert [e['validation/main/map'] for e in log] == [0.1, 0.2, (0.3 + 0.4) / 2]
    assert all(e['elapsed_time'] >= 0 for e in log)
    assert tr.get_extension('LogReport').log == log


def test_log_report_omits_validation_in_windows_without_evaluation(tmp_path):
    tr = T.Trainer(_FakeLoop(10, 2), (10, 'iteration'), out=str(tmp_path))
    tr.extend(_FakeEval([0.5, 0.6]), trigger=(1, 'epoch'))      # iterations 5 and 10
    tr.extend(T.LogReport(trigger=(2, 'iteration')))
    tr.run()
    log = tr.get_extension('LogReport').log
    assert [('validation/main/map' in e) for e in log] == [False, False, True, False, True]


def test_max_value_trigger_fires_on_first_and_strictly_greater(tmp_path):
    fired = []

    class _Snap(object):
        priority = T.PRIORITY_SNAPSHOT

        def __call__(self, trainer):
            fired.append(trainer.iteration)

    tr = T.Trainer(_FakeLoop(4, 2), (12, 'iteration'), out=str(tmp_path))
    tr.extend(_FakeEval([0.3, 0.3, 0.2, 0.5, 0.5, 0.7]), trigger=(2, 'iteration'))
    tr.extend(_Snap(), trigger=T.MaxValueTrigger('validation/main/map', (2, 'iteration')))
    tr.run()
    assert fired == [2, 8, 12]


def test_print_and_params_report(tmp_path):
    import io
    import yaml
    buf = io.StringIO()
    tr = T.Trainer(_FakeLoop(4, 2), (4, 'iteration'), out=str(tmp_path))
    tr.extend(T.ParamsReport({'lr': 0.01, 'anchor_scales': (4, 8), 'class_names': ('a', 'b'),
                              'mean': np.float32(1.5)}))
    tr.extend(T.observe_lr(), trigger=(2, 'iteration'))
    tr.extend(T.LogReport(trigger=(2, 'iteration')))
    tr.extend(T.PrintReport(['iteration', 'epoch', 'lr', 'main/loss'], out=buf),
              trigger=(2, 'iteration'))
    tr.run()
    lines = buf.getvalue().splitlines()
    assert lines[0].split() == ['iteration', 'epoch', 'lr', 'main/loss']
    assert [l.split()[0] for l in lines[1:]] == ['2', '4']
    with open(os.path.join(str(tmp_path), 'params.yaml')) as f:
        assert yaml.safe_load(f) == {'lr': 0.01, 'anchor_scales': [4, 8], 'class_names': ['a', 'b'],
                                     'mean': 1.5}


def test_plot_report_writes_png(tmp_path):
    tr = T.Trainer(_FakeLoop(4, 2), (4, 'iteration'), out=str(tmp_path))
    tr.extend(T.PlotReport(['main/loss'], file_name='loss.png', trigger=(2, 'iteration')))
    tr.run()
    with open(os.path.join(str(tmp_path), 'loss.png'), 'rb') as f:
        assert f.read(8) == b'\x89PNG\r\n\x1a\n'


def test_concatenated_and_indexing_dataset():
    import chainer_mask_rcnn_amd as cmr
    cat = T.ConcatenatedDataset([1, 2], [3], [4, 5, 6])
    assert len(cat) == 6 and [cat[i] for i in range(6)] == [1, 2, 3, 4, 5, 6]
    with pytest.raises(IndexError):
        cat[6]
    with pytest.raises(IndexError):
        cat[-1]
    idx = cmr.datasets.IndexingDataset(cat, indices=[5, 0])
    assert len(idx) == 2 and idx[0] == 6 and idx.get_example(1) == 1
    assert len(cmr.datasets.IndexingDataset(cat, 3)) == 1


def test_git_hash():
    import chainer_mask_rcnn_amd as cmr
    h = cmr.utils.git_hash(__file__)
    assert h is None or (isinstance(h, str) and len(h) >= 4)


# ---- ImageNet ResNet import --------------------------------------------------------------------
def _chainer_resnet_npz(path, n_layers, rng):
    """A chainer ResNet{50,101}Layers npz: every key and shape of the real file (random values)."""
    blocks = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}[n_layers]
    d = {}

    def bn(prefix, c):
        d[prefix + '/gamma'] = rng.uniform(0.5, 1.5, c).astype(np.float32)
        d[prefix + '/beta'] = rng.standard_normal(c).astype(np.float32)
        d[prefix + '/avg_mean'] = rng.standard_normal(c).astype(np.float32)
        d[prefix + '/avg_var'] = rng.uniform(0, 2, c).astype(np.float32)
        d[prefix + '/N'] = np.array(100, np.int64)

    d['conv1/W'] = rng.standard_normal((64, 3, 7, 7)).astype(np.float32)
    d['conv1/b'] = rng.standard_normal(64).astype(np.float32)
    bn('bn1', 64)
    in_ch = 64
    for s, (n, mid) in enumerate(zip(blocks, (64, 128, 256, 512))):
        out_ch = mid * 4
        for i in range(n):
            b = 'res%d/%s' % (s + 2, 'a' if i == 0 else 'b%d' % i)
            cin = in_ch if i == 0 else out_ch
            d[b + '/conv1/W'] = rng.standard_normal((mid, cin, 1, 1)).astype(np.float32)
            d[b + '/conv2/W'] = rng.standard_normal((mid, mid, 3, 3)).astype(np.float32)
            d[b + '/conv3/W'] = rng.standard_normal((out_ch, mid, 1, 1)).astype(np.float32)
            bn(b + '/bn1', mid)
            bn(b + '/bn2', mid)
            bn(b + '/bn3', out_ch)
            if i == 0:
                d[b + '/conv4/W'] = rng.standard_normal((out_ch, cin, 1, 1)).astype(np.float32)
                bn(b + '/bn4', out_ch)
        in_ch = out_ch
    d['fc6/W'] = rng.standard_normal((1000, 2048)).astype(np.float32)
    d['fc6/b'] = rng.standard_normal(1000).astype(np.float32)
    np.savez(path, **d)
    return d


def _fold(d, prefix):
    g, b = d[prefix + '/gamma'], d[prefix + '/beta']
    m, v = d[prefix + '/avg_mean'], d[prefix + '/avg_var']
    W = g / np.sqrt(v + np.float32(1e-5))
    return W, b - m * W


@pytest.mark.parametrize('n_layers', [50, 101])
def test_load_imagenet_resnet(tmp_path, n_layers):
    import chainer_mask_rcnn_amd as cmr
    from chainer_mask_rcnn_amd import serializers
    rng = np.random.RandomState(n_layers)
    path = str(tmp_path / ('ResNet-%d-model.npz' % n_layers))
    d = _chainer_resnet_npz(path, n_layers, rng)
    torch.manual_seed(0)
    model = cmr.models.MaskRCNNResNet(n_layers, n_fg_class=3)
    before = serializers.state_arrays(model)
    torch.manual_seed(0)
    model2 = cmr.models.MaskRCNNResNet(n_layers, n_fg_class=3, pretrained_model='imagenet',
                                       imagenet_weights=path)
    serializers.load_imagenet_resnet(path, model)
    for m in (model, model2):
        got = serializers.state_arrays(m)
        assert np.array_equal(got['extractor/conv1/W'], d['conv1/W'][:, ::-1])
        assert np.array_equal(got['extractor/conv1/b'], d['conv1/b'])
        W, b = _fold(d, 'bn1')
        assert np.array_equal(got['extractor/bn1/W'], W) and np.array_equal(got['extractor/bn1/b'], b)
        covered = set()
        for key in d:
            if not key.startswith('res') or key.endswith('/N'):
                continue
            stage, rest = key.split('/', 1)
            owner = 'head' if stage == 'res5' else 'extractor'
            if '/conv' in key:
                assert np.array_equal(got['%s/%s/%s' % (owner, stage, rest)], d[key]), key
                covered.add('%s/%s/%s' % (owner, stage, rest))
            elif key.endswith('/gamma'):
                prefix = key[:-len('/gamma')]
                W, b = _fold(d, prefix)
                dst = '%s/%s' % (owner, prefix)
                assert np.array_equal(got[dst + '/W'], W), dst
                assert np.array_equal(got[dst + '/b'], b), dst
                covered.update((dst + '/W', dst + '/b'))
        assert covered == {k for k in got if '/res' in k}    # every res2..res5 parameter
        # the RPN and the head's own layers keep their initialisers
        for key in got:
            if key.startswith('rpn/') or key.split('/')[1] in ('cls_loc', 'score', 'deconv6', 'mask'):
                assert np.array_equal(got[key], before[key]), key
    assert sum(1 for k in serializers.state_arrays(model) if k.startswith('head/res5/')) > 0


def test_load_imagenet_resnet_errors(tmp_path, monkeypatch):
    import chainer_mask_rcnn_amd as cmr
    from chainer_mask_rcnn_amd import serializers
    monkeypatch.setenv('CHAINER_DATASET_ROOT', str(tmp_path / 'nowhere'))
    want = os.path.join(str(tmp_path / 'nowhere'), 'pfnet', 'chainer', 'models', 'ResNet-50-model.npz')
    assert serializers.default_imagenet_path(50) == want
    with pytest.raises(IOError, match='ResNet-50-model.npz'):
        cmr.models.MaskRCNNResNet(50, n_fg_class=3, pretrained_model='imagenet')
    path = str(tmp_path / 'r50.npz')
    _chainer_resnet_npz(path, 50, np.random.RandomState(0))
    with pytest.raises(KeyError):
        serializers.load_imagenet_resnet(path, cmr.models.MaskRCNNResNet(101, n_fg_class=3))


def test_he_normal_mask_init_uses_chainer_fan_out():
    import chainer_mask_rcnn_amd as cmr
    torch.manual_seed(0)
    n_fg = 80
    m = cmr.models.MaskRCNNResNet(50, n_fg_class=n_fg, mask_initialW='he_normal')
    dw = m.head.deconv6.W.detach().numpy()
    mw = m.head.mask.W.detach().numpy()
    assert dw.shape == (2048, 256, 2, 2) and mw.shape == (n_fg, 256, 1, 1)
    want_d, want_m = np.sqrt(2. / (2048 * 4)), np.sqrt(2. / n_fg)
    assert abs(dw.std() / want_d - 1) < 0.01
    assert abs(mw.std() / want_m - 1) < 0.02
    torch.manual_seed(0)
    m0 = cmr.models.MaskRCNNResNet(50, n_fg_class=n_fg)
    assert abs(m0.head.deconv6.W.detach().numpy().std() / 0.01 - 1) < 0.01
    with pytest.raises(ValueError):
        cmr.models.MaskRCNNResNet(50, n_fg_class=3, mask_initialW='glorot')


# ---- command-line tools --------------------------------------------------------------------------
def test_train_help_and_world_size_refusal():
    train = os.path.join(ROOT, 'tools', 'train.py')
    r = subprocess.run([sys.executable, train, '--help'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ('--model', '--pooling-func', '--roi-size', '--initializer', '--max-epoch',
                 '--batch-size-per-gpu', '--dataset', '--imagenet-weights', '--logs-dir',
                 '--allow-random-init'):
        assert flag in r.stdout, flag
    env = dict(os.environ, WORLD_SIZE='2')
    r = subprocess.run([sys.executable, train, '--dataset', 'synthetic'], capture_output=True,
                       text=True, env=env, timeout=120)
    assert r.returncode != 0 and 'world size 2 is not supported' in r.stderr
    r = subprocess.run([sys.executable, train, '--multi-node'], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and 'not supported' in r.stderr


def test_train_refuses_real_dataset_without_weights(tmp_path):
    env = dict(os.environ, CHAINER_DATASET_ROOT=str(tmp_path))
    env.pop('WORLD_SIZE', None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train.py'), '--dataset', 'voc'],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode != 0 and '--allow-random-init' in r.stderr


def test_summarize_logs(tmp_path):
    import yaml
    logs = tmp_path / 'logs'
    for name, maps in (('20260101_000000', [0.1, 0.3, 0.2]), ('20260102_000000', [0.05])):
        d = logs / name
        d.mkdir(parents=True)
        with open(str(d / 'params.yaml'), 'w') as f:
            yaml.safe_dump({'model': 'resnet50', 'initializer': 'normal', 'lr': 0.0025,
                            'git_hash': 'abc1234', 'hostname': 'h',
                            'timestamp': '2026-01-01T00:00:00'}, f)
        log = []
        for i, m in enumerate(maps):
            log.append({'main/loss': 1.0 / (i + 1), 'epoch': i, 'iteration': 20 * (i + 1),
                        'elapsed_time': 10.0 * (i + 1)})
            log.append({'main/loss': 0.9 / (i + 1), 'validation/main/map': m, 'epoch': i + 1,
                        'iteration': 20 * (i + 1) + 10, 'elapsed_time': 10.0 * (i + 1) + 5})
        with open(str(d / 'log'), 'w') as f:
            json.dump(log, f)
    with open(str(logs / '20260101_000000' / 'snapshot_model.npz.eval_result.yaml'), 'w') as f:
        yaml.safe_dump({'validation/main/map': 0.31}, f)
    (logs / 'not_a_run').mkdir()
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'summarize_logs.py'), str(logs)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    lines = out.splitlines()
    row1 = [l for l in lines if '20260101_000000' in l][0]
    row2 = [l for l in lines if '20260102_000000' in l][0]
    assert lines.index(row2) < lines.index(row1)            # newest first
    assert '0.100< 0.300' in row1 and '50 /70' in row1 and '0.310' in row1 and 'abc1234' in row1
    assert '0.050< 0.050' in row2
    assert 'Ignored logs:' in out and 'not_a_run' in out
