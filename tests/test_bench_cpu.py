"""bench.py pieces that run without a GPU: the power / clock sampler degrades to None fields, a
plain run drops every leg but the headline and --full restores them, the multi-GPU default drops the
auxiliary legs, and a run without a ROCm device fails loudly."""
import os
import subprocess
import sys

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_smi_sampler_without_a_device_reports_none():
    s = bench.SmiSampler(0, period=0.001)
    with s:
        pass
    out = s.summary()
    assert set(out) == {'power_w', 'power_w_max', 'sclk_mhz', 'sclk_mhz_min', 'samples'}
    if s.lib is None or out['samples'] == 0 or out['power_w'] is None:
        assert out['power_w'] is None and out['power_w_max'] is None


def test_bench_refuses_to_run_without_a_rocm_device():
    import torch
    if torch.cuda.is_available():
        return                       # (a GPU box: nothing to refuse, and a full bench run is not a CPU test)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '1', '--warmup', '0',
                        '--no-cpu-baseline'], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and r.stdout.strip() == ''          # no JSON line from a run that measured nothing
    assert 'ROCm device' in r.stderr or 'HIP' in r.stderr or 'hip' in r.stderr


def test_smi_sampler_can_be_disabled_and_survives_a_library_without_the_symbols(monkeypatch):
    s = bench.SmiSampler(0, enabled=False)
    with s:
        pass
    assert s.lib is None and s.summary()['samples'] == 0

    class NoSymbols(object):          # a librocm_smi64 that lacks the two query functions
        def __getattr__(self, name):
            raise AttributeError(name)
    monkeypatch.setattr(bench.ctypes, 'CDLL', lambda name: NoSymbols())
    s = bench.SmiSampler(0)
    with s:
        pass
    assert s.lib is None and s.summary()['power_w'] is None


def _legs(args):
    return dict(rotate=args.rotate_batches, pipeline=args.pipeline_examples, fg_capped=args.fg_capped,
                device_targets=args.device_targets, direct=args.direct_head_forward, fp32=args.fp32_mfma,
                extra=args.extra_workloads, cpu=not args.no_cpu_baseline)


def test_plain_run_is_the_headline_only_and_full_restores_every_leg():
    plain = bench.parse_args(['--steps', '3', '--warmup', '1'])
    assert not plain.full and (plain.steps, plain.warmup) == (3, 1)
    assert not any(_legs(plain).values())
    full = bench.parse_args(['--full'])
    assert full.full and _legs(full) == dict(rotate=4, pipeline=16, fg_capped=True, device_targets=True,
                                             direct=True, fp32=True, extra=True, cpu=True)
    # each leg's own switch still holds under --full
    some = bench.parse_args(['--full', '--no-cpu-baseline', '--rotate-batches', '0', '--no-fp32-mfma'])
    assert _legs(some) == dict(_legs(full), rotate=0, fp32=False, cpu=False)
    # multi-GPU: --full adds no auxiliary leg, --all-legs implies --full and restores them
    multi = bench.parse_args(['--gpus', '2', '--full'])
    assert multi.full and not any(v for k, v in _legs(multi).items() if k not in ('extra', 'cpu'))
    legs = bench.parse_args(['--gpus', '2', '--all-legs'])
    assert legs.full and _legs(legs) == _legs(full)


def test_multi_gpu_request_without_devices_is_refused():
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        return
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1'],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'one process per GPU' in (r.stderr + r.stdout)


def test_write_outputs_dtypes_seeded_sample_and_size_limit(tmp_path, monkeypatch):
    import numpy as np
    import pytest
    monkeypatch.setattr(bench, 'DUMP_SAMPLE', 100)
    big = np.arange(1000, dtype=np.float32)
    arrays = dict(loss=np.float64(1.25), labels=np.array([3, 1], np.int32), big=big)
    n = bench.write_outputs(str(tmp_path / 'a'), arrays)
    bench.write_outputs(str(tmp_path / 'b'), dict(big=big[::-1].copy()))
    got = {k: np.load(str(tmp_path / 'a' / (k + '.npy'))) for k in arrays}
    assert got['loss'].dtype == np.float64 and got['loss'] == 1.25
    assert got['labels'].dtype == np.float32 and got['labels'].tolist() == [3., 1.]
    # a fixed sample: distinct sorted positions, the same ones for every output of that size
    s = got['big']
    assert s.dtype == np.float32 and s.shape == (100,) and np.all(np.diff(s) > 0)
    assert np.array_equal(np.load(str(tmp_path / 'b' / 'big.npy')), 999 - s)
    assert n == 8 + 2 * 4 + 100 * 4
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 64)
    with pytest.raises(ValueError):
        bench.write_outputs(str(tmp_path / 'c'), dict(big=big))
    assert not (tmp_path / 'c').exists()                  # nothing written past the limit


def test_train_step_outputs_concatenate_in_parameter_name_order():
    import torch
    from chainer_mask_rcnn_amd import optimizers

    class Chain(torch.nn.Module):
        def __init__(self):
            super(Chain, self).__init__()
            self.b = torch.nn.Parameter(torch.arange(6, dtype=torch.float32).reshape(2, 3))
            # dense but transposed: the arena keeps its memory order, the dump its logical order
            self.a = torch.nn.Parameter(torch.arange(100, 104, dtype=torch.float32).reshape(2, 2).t())
            self.frozen = torch.nn.Parameter(torch.zeros(5), requires_grad=False)
            self.report = {'loss': torch.tensor(2.5), 'roi_cls_loss': torch.tensor(0.5)}

    chain = Chain()
    opt = optimizers.MomentumSGD(lr=0.1).setup(chain)
    opt._build()
    a = opt.arena
    a.momenta.copy_(-torch.arange(a.size, dtype=torch.float32))
    out = bench.train_step_outputs(chain, opt)
    assert out['loss'] == 2.5 and out['roi_cls_loss'] == 0.5
    assert out['params'].tolist() == [100., 102., 101., 103., 0., 1., 2., 3., 4., 5.]
    off = {n: a.offsets[[id(p) for p in a.params].index(id(getattr(chain, n)))] for n in 'ab'}
    want = [off['a'] + k for k in (0, 2, 1, 3)] + [off['b'] + k for k in range(6)]
    assert out['momenta'].tolist() == [-float(v) for v in want]
