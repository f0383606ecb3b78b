"""The host side of gradient clipping, the non-finite guard and the lr warm-up, without a device:
hook validation, the refusal of deferred weight gradients in both orders, the warm-up sequence and
its composition with ExponentialShift, observe_lr, StopWhenEverythingSkipped, params.yaml of a
default run, and the header / binding tables of the new entry points."""
import os
import re
import sys

import pytest
import torch

from chainer_mask_rcnn_amd import _lib, optimizers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import trainer as T  # noqa: E402


# ---- hooks -------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [0, 0., -1., float('inf'), float('nan')])
def test_gradient_clipping_refuses_a_bad_threshold(bad):
    with pytest.raises(ValueError):
        optimizers.GradientClipping(bad)


def test_hooks_switch_the_optimizer():
    opt = optimizers.MomentumSGD(lr=0.1)
    assert opt.report == {} and opt.lr_scale == 1.0 and not opt.observe_norm
    opt.add_hook(optimizers.WeightDecay(1e-4))
    assert opt.report == {} and not opt.observe_norm and opt.weight_decay == 1e-4
    opt.add_hook(optimizers.ObserveGradientNorm())
    assert opt.observe_norm and opt.grad_clip == 0. and not opt.skip_nonfinite
    opt.add_hook(optimizers.GradientClipping(2.5))
    opt.add_hook(optimizers.SkipNonFiniteUpdate())
    assert opt.grad_clip == 2.5 and opt.skip_nonfinite
    with pytest.raises(TypeError):
        opt.add_hook(object())


def test_report_is_bound_to_the_control_word_once_the_arena_exists():
    lin = torch.nn.Linear(3, 2)
    opt = optimizers.MomentumSGD(lr=0.1).setup(lin)
    opt.add_hook(optimizers.SkipNonFiniteUpdate())
    assert opt.report == {}
    opt._build()
    assert sorted(opt.report) == ['grad_norm', 'skipped']
    for v in opt.report.values():
        assert v.numel() == 1 and v.dtype == torch.float32
        assert v.untyped_storage().data_ptr() == opt._ctl.untyped_storage().data_ptr()
    # installed after the arena was built: bound at once
    opt2 = optimizers.MomentumSGD(lr=0.1).setup(torch.nn.Linear(3, 2))
    opt2._build()
    opt2.add_hook(optimizers.ObserveGradientNorm())
    assert sorted(opt2.report) == ['grad_norm', 'skipped']


@pytest.mark.parametrize('hook', [lambda: optimizers.GradientClipping(1.),
                                  optimizers.SkipNonFiniteUpdate, optimizers.ObserveGradientNorm])
def test_norm_hooks_and_deferred_weight_gradients_refuse_each_other(hook):
    lin = torch.nn.Linear(3, 2)
    opt = optimizers.MomentumSGD(lr=0.1).setup(lin)
    opt.defer_weight_gradients([lin.weight])
    with pytest.raises(ValueError) as e:
        opt.add_hook(hook())
    assert 'defer' in str(e.value) and type(hook()).__name__ in str(e.value)
    assert not opt.observe_norm and opt.deferred_params == [lin.weight]      # nothing un-deferred

    opt = optimizers.MomentumSGD(lr=0.1).setup(lin)
    opt.add_hook(hook())
    with pytest.raises(ValueError) as e:
        opt.defer_weight_gradients([lin.weight])
    assert 'defer_weight_gradients' in str(e.value) and 'GradientClipping' in str(e.value)
    assert opt.deferred_params == [] and opt.observe_norm
    opt.defer_weight_gradients([])            # deferring nothing is no deferral


# ---- warm-up -----------------------------------------------------------------------------------
class _Opt(object):
    def __init__(self, lr):
        self.lr, self.lr_scale = lr, 1.0


class _Loop(object):
    """What Trainer needs of a TrainLoop; ``skipped(i)``: the report of update i."""

    class _It(object):
        batch_size = 1
        dataset = list(range(1000))

    class _Chain(object):
        report = {}

    def __init__(self, lr=0.5, skipped=None):
        self.iterator, self.chain, self.optimizer = self._It(), self._Chain(), _Opt(lr)
        self.iteration = 0
        self.used = []
        self._skipped = skipped

    def step(self):
        opt = self.optimizer
        self.used.append((opt.lr, getattr(opt, 'lr_scale', None)))
        if self._skipped is not None:
            opt.report = {'skipped': self._skipped(self.iteration)}
        self.iteration += 1


def test_linear_warmup_sequence():
    w = T.LinearWarmup(4, 1. / 3.)
    third = 1. / 3.
    assert [w.scale(i) for i in range(7)] == [third, third + (1 - third) * 1 / 4, third + (1 - third) * 2 / 4,
                                              third + (1 - third) * 3 / 4, 1.0, 1.0, 1.0]
    assert [w.scale(i) for i in range(5)] == pytest.approx([1 / 3, 1 / 2, 2 / 3, 5 / 6, 1.0], abs=1e-15)
    assert T.LinearWarmup(0).scale(0) == 1.0
    assert T.LinearWarmup(5).factor == 1. / 3.
    for bad in ((-1, 0.3), (3, -0.1), (3, 1.5)):
        with pytest.raises(ValueError):
            T.LinearWarmup(*bad)
    loop = _Loop()
    tr = T.Trainer(loop, (7, 'iteration'), out=None)
    tr.extend(w)
    tr.run()
    assert [s for _, s in loop.used] == [w.scale(i) for i in range(7)]
    assert loop.used[4][1] == 1.0 and loop.optimizer.lr_scale == 1.0
    assert all(lr == 0.5 for lr, _ in loop.used)                    # lr stays the schedule's


def test_warmup_composes_with_exponential_shift_and_observe_lr_reports_the_product():
    loop = _Loop(lr=0.5)
    tr = T.Trainer(loop, (8, 'iteration'), out=None)
    w = T.LinearWarmup(4, 1. / 3.)
    tr.extend(T.ExponentialShift('lr', 0.1), trigger=T.ManualScheduleTrigger([3, 6], 'iteration'))
    tr.extend(w)
    tr.extend(T.observe_lr())
    log = T.LogReport(trigger=(1, 'iteration'), log_name=None)
    tr.extend(log)
    tr.run()
    lrs = [0.5] * 3 + [0.5 * 0.1] * 3 + [0.5 * 0.1 ** 2] * 2
    assert loop.used == [(lr, w.scale(i)) for i, lr in enumerate(lrs)]
    # the log's lr column: what update i ran at
    assert [e['lr'] for e in log.log] == [lr * w.scale(i) for i, lr in enumerate(lrs)]
    # no warm-up, or an optimizer without lr_scale: the value is lr itself
    plain = _Loop(lr=0.25)
    del plain.optimizer.lr_scale
    tr = T.Trainer(plain, (1, 'iteration'), out=None)
    tr.extend(T.observe_lr())
    tr.extend(T.LogReport(trigger=(1, 'iteration'), log_name=None), name='LogReport')
    tr.run()
    assert tr.get_extension('LogReport').log[0]['lr'] == 0.25


# ---- the trainer's report and the stop ---------------------------------------------------------
def test_trainer_reports_the_optimizers_scalars_and_tolerates_none():
    loop = _Loop(skipped=lambda i: float(i % 2))
    tr = T.Trainer(loop, (4, 'iteration'), out=None)
    log = T.LogReport(trigger=(2, 'iteration'), log_name=None)
    tr.extend(log)
    tr.run()
    assert [e['main/skipped'] for e in log.log] == [0.5, 0.5]
    bare = _Loop()
    del bare.optimizer                       # a loop without an optimizer attribute
    tr = T.Trainer(bare, (2, 'iteration'), out=None)
    bare.step = lambda: setattr(bare, 'iteration', bare.iteration + 1)
    tr.run()
    assert tr.observation == {}


def test_stop_when_everything_skipped():
    # windows of 3: [0 1 1] goes on, [1 1 1] stops at iteration 6
    loop = _Loop(skipped=lambda i: 0. if i == 0 else 1.)
    tr = T.Trainer(loop, (30, 'iteration'), out=None)
    tr.extend(T.LogReport(trigger=(3, 'iteration'), log_name=None))
    tr.extend(T.StopWhenEverythingSkipped(), trigger=(3, 'iteration'))
    with pytest.raises(RuntimeError, match='skipped'):
        tr.run()
    assert loop.iteration == 6
    # nothing skipped, or no such key in the log: runs to the end
    for skipped in (lambda i: 0., None):
        loop = _Loop(skipped=skipped)
        tr = T.Trainer(loop, (6, 'iteration'), out=None)
        tr.extend(T.LogReport(trigger=(3, 'iteration'), log_name=None))
        tr.extend(T.StopWhenEverythingSkipped(), trigger=(3, 'iteration'))
        tr.run()
        assert loop.iteration == 6


def test_extend_reference_set_options(tmp_path):
    import io
    for grad_report in (False, True):
        loop = _Loop(skipped=(lambda i: 0.) if grad_report else None)
        tr = T.Trainer(loop, (4, 'iteration'), out=str(tmp_path / str(grad_report)))
        out = io.StringIO()
        T.extend_reference_set(tr, model=None, plot=False, print_out=out,
                               log_interval=(2, 'iteration'), print_interval=(2, 'iteration'),
                               warmup=T.LinearWarmup(2, 0.5) if grad_report else None,
                               grad_report=grad_report)
        names = [type(e.extension).__name__ for e in tr.ordered_entries()]
        assert ('StopWhenEverythingSkipped' in names) == grad_report
        assert ('LinearWarmup' in names) == grad_report
        if grad_report:
            assert names.index('StopWhenEverythingSkipped') > names.index('LogReport')
        tr.run()
        header = out.getvalue().splitlines()[0].split()
        assert ('main/grad_norm' in header) == grad_report and ('main/skipped' in header) == grad_report
        assert [h for h in header if h not in T.GRAD_KEYS] == \
            ['iteration', 'epoch', 'elapsed_time', 'lr'] + T.LOG_KEYS + ['validation/main/map']
        if grad_report:
            assert [s for _, s in loop.used] == [0.5, 0.75, 1.0, 1.0]
    assert len(T.LOG_KEYS) + len(T.GRAD_KEYS) == 8        # MRCNN_MAX_OBSERVED device scalars


# ---- tools/train.py ----------------------------------------------------------------------------
def test_params_yaml_of_a_default_run_is_unchanged():
    import train
    args = train.parse_args([])
    assert (args.grad_clip, args.skip_nonfinite, args.warmup_iters) == (0., False, 0)
    assert args.warmup_factor == 1. / 3.
    before = {k: v for k, v in vars(args).items()
              if k not in ('grad_clip', 'skip_nonfinite', 'warmup_iters', 'warmup_factor', 'eval_bbox')}
    assert train.recorded_params(args) == before
    args = train.parse_args(['--grad-clip', '10', '--skip-nonfinite', '--warmup-iters', '500',
                             '--warmup-factor', '0.25', '--eval-bbox'])
    rec = train.recorded_params(args)
    assert (rec['grad_clip'], rec['skip_nonfinite'], rec['warmup_iters'], rec['warmup_factor'],
            rec['eval_bbox']) == (10., True, 500, 0.25, True)
    rec = train.recorded_params(train.parse_args(['--skip-nonfinite']))
    assert rec['skip_nonfinite'] is True and 'grad_clip' not in rec and 'warmup_factor' not in rec


def test_norm_hooks_of_the_flags():
    import train_loop
    assert train_loop.norm_hooks() == []
    hooks = train_loop.norm_hooks(5., True)
    assert [type(h) for h in hooks] == [optimizers.GradientClipping, optimizers.SkipNonFiniteUpdate]
    assert hooks[0].threshold == 5.
    import inspect
    sig = inspect.signature(train_loop.setup_training)
    assert sig.parameters['hooks'].default == () and sig.parameters['defer'].default == 5


# ---- C ABI -------------------------------------------------------------------------------------
NEW = ('mrcnn_grad_sumsq', 'mrcnn_grad_control', 'mrcnn_sgd_momentum_wd_ctl')


def test_header_and_binding_tables_hold_the_new_entry_points():
    text = open(os.path.join(ROOT, 'include', 'mrcnn_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NEW:
        assert re.search(r'\bint %s\s*\(' % name, code), name
        assert name in _lib.SIGNATURES
    c = _lib
    assert c.SIGNATURES['mrcnn_grad_sumsq'][1] == [c.c_vp, c.c_i64, c.c_vp, c.c_vp]
    assert c.SIGNATURES['mrcnn_grad_control'][1] == [c.c_vp, c.c_int, c.c_f32, c.c_f32, c.c_int,
                                                     c.c_vp, c.c_vp]
    assert c.SIGNATURES['mrcnn_sgd_momentum_wd_ctl'][1] == \
        [c.c_vp] * 3 + [c.c_i64] + [c.c_f32] * 3 + [c.c_vp, c.c_int, c.c_vp]
    defs = dict(re.findall(r'#define (MRCNN_(?:CTL|SUMSQ)_\w+) (\d+)', text))
    assert int(defs['MRCNN_SUMSQ_PARTIALS']) == optimizers.SUMSQ_PARTIALS
    assert [int(defs['MRCNN_CTL_' + k]) for k in ('NORM', 'FACTOR', 'SKIPPED', 'NORM_REPORTED', 'SIZE')] \
        == [optimizers.CTL_NORM, optimizers.CTL_FACTOR, optimizers.CTL_SKIPPED,
            optimizers.CTL_NORM_REPORTED, optimizers.CTL_SIZE]


def test_new_entry_points_validate_without_a_device():
    import __graft_entry__ as g
    g.build()
    lib = _lib.load()
    assert lib.mrcnn_grad_sumsq(None, -1, None, None) != 0 and b'grad_sumsq' in lib.mrcnn_last_error()
    assert lib.mrcnn_grad_sumsq(None, 0, None, None) != 0 and b'partials' in lib.mrcnn_last_error()
    assert lib.mrcnn_grad_control(None, -1, 1., 0., 0, None, None) != 0
    assert b'grad_control' in lib.mrcnn_last_error()
    assert lib.mrcnn_sgd_momentum_wd_ctl(None, None, None, 4, 0.1, 0.9, 0., None, 0, None) != 0
    assert b'control word' in lib.mrcnn_last_error()
