"""The gradient-norm hooks of optimizers.py on the device, on the small model of
tests/test_gpu_trainer.py (ResNet-50, 144 x 192, 32 RoIs): observing changes nothing, clipping is a
plain step at the device's factor, a non-finite gradient leaves the state alone, a Trainer run with
clip + guard + warm-up across an lr shift is repeatable, and two ranks sharing the GPU clip alike."""
import io
import json
import math
import os
import random
import socket
import sys

import numpy as np
import pytest
import torch

import chainer_mask_rcnn_amd as cmr
import grad_control_ref as R
from chainer_mask_rcnn_amd import optimizers, streams
from chainer_mask_rcnn_amd.functions import conv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

pytestmark = pytest.mark.gpu

H, W = 144, 192
LR, WD = 0.0025, 1e-4


def build_small(dev, hooks=(), seed=4):
    """Model, chain and optimizer of tests/test_gpu_trainer.py:_build without deferred weight
    gradients, with ``hooks`` installed."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    model = cmr.models.MaskRCNNResNet(
        50, n_fg_class=20, anchor_scales=(4, 8, 16, 32), roi_size=14, min_size=H, max_size=W,
        proposal_creator_params=dict(min_size=0, n_train_pre_nms=600, n_train_post_nms=100,
                                     n_test_pre_nms=6000, n_test_post_nms=1000))
    chain = cmr.models.MaskRCNNTrainChain(
        model, proposal_target_creator=cmr.models.utils.ProposalTargetCreator(n_sample=32)).to(dev)
    chain.train()
    opt = optimizers.MomentumSGD(lr=LR, momentum=0.9)
    opt.setup(chain)
    opt.add_hook(optimizers.WeightDecay(WD))
    for hook in hooks:
        opt.add_hook(hook)
    for link in (model.extractor.conv1, model.extractor.bn1, model.extractor.res2):
        optimizers.disable_update(link)
    for m in chain.modules():
        if isinstance(m, cmr.links.AffineChannel2D):
            optimizers.disable_update(m)
    with torch.no_grad():
        model.extractor.bn1.W.fill_(1. / 64.)
        for m in model.modules():
            if isinstance(m, cmr.models.resnet_extractor.Bottleneck):
                m.bn3.W.fill_(0.25)
    return model, chain, opt


def batch(dev, flip=False):
    rng = np.random.RandomState(0)
    imgs = rng.uniform(-120, 130, (2, 3, H, W)).astype(np.float32)
    if flip:
        imgs = imgs[:, :, :, ::-1].copy()
    bboxes = [np.array([[10, 20, 90, 120], [40, 70, 130, 180]], np.float32),
              np.array([[8, 8, 70, 60]], np.float32)]
    labels = [np.array([3, 17], np.int32), np.array([11], np.int32)]
    masks = []
    for b in bboxes:
        m = np.zeros((len(b), H, W), np.int32)
        for g, (y0, x0, y1, x1) in enumerate(b.astype(int)):
            m[g, y0 + 4:y1 - 4, x0 + 4:x1 - 4] = 1
        masks.append(m)
    return torch.tensor(imgs, device=dev), bboxes, labels, masks, [1., 1.]


def backward_by_hand(chain, opt, inputs, seed):
    """Forward + backward into the gradient arena, no step: the arena can be read (or written)
    before ``opt.update()`` without a loss function applies it."""
    if opt.arena is None:
        opt._build()
    np.random.seed(seed)
    loss = chain(*inputs)
    loss.backward()
    streams.join_wgrad_stream()
    torch.cuda.synchronize()
    return loss


def state(opt):
    a = opt.arena
    torch.cuda.synchronize()
    return a.values.clone(), a.momenta.clone(), a.grads.clone()


def rewind(opt, values, momenta, grads, written):
    """Put the arena back to a saved state with ``grads`` as the pending step's gradients."""
    a = opt.arena
    a.values.copy_(values)
    a.momenta.copy_(momenta)
    a.grads.copy_(grads)
    for p, w in zip(a.params, written):
        p._grad_epoch = a.epoch if w else 0


def arena_norm(opt):
    """float64 norm of the gradient arena (tens of millions of elements: the squares are exact in
    float64 and NumPy's pairwise sum is within a few tens of float64 ulps, far below the fp32
    rounding of the reported value; math.fsum over a list of that length would take minutes)."""
    g = opt.arena.grads.cpu().numpy().astype(np.float64)
    return math.sqrt(float(np.sum(g * g)))


def test_observing_the_norm_changes_nothing_and_reports_the_arena_norm(dev):
    inputs = batch(dev)
    out = []
    for hooks in ((), (optimizers.ObserveGradientNorm(),)):
        model, chain, opt = build_small(dev, hooks)
        for k in range(2):
            backward_by_hand(chain, opt, inputs, 11 + k)
            ref = arena_norm(opt)
            opt.update()
            torch.cuda.synchronize()
            if hooks:
                got = float(opt.report['grad_norm'])
                print('step %d: reported %.9g, float64 norm of the arena %.9g' % (k, got, ref))
                assert abs(got - ref) <= 2.0 ** -23 * ref and ref > 0
                assert float(opt.report['skipped']) == 0.
                assert float(opt._ctl[R.CTL_FACTOR]) == 1.0
        assert opt.t == 2 and opt.arena.epoch == 3
        assert (opt.report == {}) == (not hooks)
        out.append(state(opt))
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a, b)
    assert float(out[0][2].abs().max()) == 0.          # gradients cleared on both paths


def test_clipping_is_a_plain_step_at_the_device_factor(dev):
    inputs = batch(dev)
    model, chain, opt = build_small(dev, (optimizers.ObserveGradientNorm(),))
    backward_by_hand(chain, opt, inputs, 21)
    norm = arena_norm(opt)
    v0, m0, g0 = state(opt)
    written = opt.arena.written()
    clip = float(np.float32(0.5 * norm))
    opt.add_hook(optimizers.GradientClipping(clip))
    opt.update()
    torch.cuda.synchronize()
    ctl = opt._ctl.cpu().numpy()
    factor = float(ctl[R.CTL_FACTOR])
    want = np.float32(clip / norm)
    print('norm %.9g (device %.9g), clip %.9g, factor %.9g (reference %.9g)'
          % (norm, ctl[R.CTL_NORM], clip, factor, want))
    assert abs(float(ctl[R.CTL_NORM]) - norm) <= 2.0 ** -23 * norm
    assert abs(factor - float(want)) <= R.ulp32(want) and 0.49 < factor < 0.51
    clipped = state(opt)
    # the same state through the plain path: step(grad_scale=factor) with no norm hook
    rewind(opt, v0, m0, g0, written)
    opt.observe_norm = False
    opt.step(grad_scale=factor, zero_grads=True)
    plain = state(opt)
    for x, y in zip(clipped, plain):
        assert torch.equal(x, y)
    assert not torch.equal(clipped[0], v0)


def test_a_non_finite_gradient_is_skipped_and_the_next_step_is_clean(dev):
    inputs = batch(dev)
    model, chain, opt = build_small(dev, (optimizers.SkipNonFiniteUpdate(),))
    backward_by_hand(chain, opt, inputs, 31)
    opt.update()                                        # one ordinary step: momenta are non-zero
    backward_by_hand(chain, opt, inputs, 32)
    v0, m0, _ = state(opt)
    opt.arena.grads[opt.arena.size // 2] = float('inf')
    t, epoch = opt.t, opt.arena.epoch
    opt.update()
    v1, m1, g1 = state(opt)
    assert torch.equal(v1, v0) and torch.equal(m1, m0)
    assert float(g1.abs().max()) == 0.
    assert float(opt.report['skipped']) == 1. and float(opt.report['grad_norm']) == 0.
    assert (opt.t, opt.arena.epoch) == (t + 1, epoch + 1)
    # the next, clean step equals a plain step from that state
    backward_by_hand(chain, opt, inputs, 33)
    _, _, g2 = state(opt)
    written = opt.arena.written()
    opt.update()
    guarded = state(opt)
    assert float(opt.report['skipped']) == 0. and float(opt.report['grad_norm']) > 0
    rewind(opt, v1, m1, g2, written)
    opt.observe_norm = False
    opt.step(grad_scale=1.0, zero_grads=True)
    for x, y in zip(guarded, state(opt)):
        assert torch.equal(x, y)
    assert not torch.equal(guarded[0], v1)


# ---- Trainer -----------------------------------------------------------------------------------
STEP_POINTS = [1.5]           # inside epoch 2 (3 iterations per epoch): lr x 0.1 from update 5 on
WARMUP = 3


def _trainer_run(dev, root, out):
    import train_loop as TL
    import trainer as T
    data = T.ConcatenatedDataset(T.VOCLikeDataset(root), T.VOCLikeDataset(root))     # 6 examples
    model, chain, opt = build_small(dev)
    norm_probe = []

    class Probe(object):
        priority = 1000

        def __call__(self, trainer):
            o = trainer.loop.optimizer
            norm_probe.append((o.lr, o.lr_scale, o._ctl.clone()))
    opt.add_hook(optimizers.GradientClipping(CLIP))
    opt.add_hook(optimizers.SkipNonFiniteUpdate())
    train = TL.TransformDataset(data, cmr.datasets.MaskRCNNTransform(model))
    loop = TL.TrainLoop(TL.SerialIterator(train, 2), chain, opt, dev, prefetch=True)
    tr = T.Trainer(loop, (8, 'iteration'), out=out)
    tr.extend(Probe())
    printed = io.StringIO()
    T.extend_reference_set(tr, model, step_size=STEP_POINTS, log_interval=(2, 'iteration'),
                           print_interval=(2, 'iteration'), plot=False, print_out=printed,
                           warmup=T.LinearWarmup(WARMUP), grad_report=True)
    tr.run()
    torch.cuda.synchronize()
    loop.close()
    with open(os.path.join(out, 'log')) as f:
        log = json.load(f)
    header = printed.getvalue().splitlines()[0].split()
    assert 'main/grad_norm' in header and 'main/skipped' in header and 'lr' in header
    return state(opt), norm_probe, log, opt


CLIP = 60.            # the run's norms lie between 40 and 90: some steps clip


def test_trainer_with_clip_guard_and_warmup_is_repeatable(tmp_path, dev):
    import trainer as T
    from test_gpu_trainer import _write_voc_like
    root = str(tmp_path / 'custom')
    _write_voc_like(root)
    (sa, pa, log_a, opt), (sb, pb, log_b, _) = (_trainer_run(dev, root, str(tmp_path / k)) for k in 'ab')
    print('norms of the run: %s (threshold %g)' % ([float(c[R.CTL_NORM]) for _, _, c in pa], CLIP))
    for x, y in zip(sa, sb):
        assert torch.equal(x, y)
    for (_, _, ca), (_, _, cb) in zip(pa, pb):
        assert torch.equal(ca, cb)
    for ea, eb in zip(log_a, log_b):
        assert {k: v for k, v in ea.items() if k != 'elapsed_time'} == \
            {k: v for k, v in eb.items() if k != 'elapsed_time'}
    w = T.LinearWarmup(WARMUP)
    lrs = [LR] * 5 + [LR * 0.1] * 3                      # the shift after iteration 5 (epoch 1.67 > 1.5)
    # Probe runs after update i and before the extensions that prepare update i + 1
    assert [(lr, s) for lr, s, _ in pa] == [(lrs[i], w.scale(i)) for i in range(8)]
    assert opt.lr_scale == 1.0 and [s for _, s, _ in pa][WARMUP:] == [1.0] * (8 - WARMUP)
    assert [e['iteration'] for e in log_a] == [2, 4, 6, 8]
    ctl = [c.cpu().numpy() for _, _, c in pa]
    for e in log_a:
        i = e['iteration']
        assert e['lr'] == lrs[i - 1] * w.scale(i - 1)
        window = ctl[i - 2:i]
        for key, slot in (('main/grad_norm', R.CTL_NORM_REPORTED), ('main/skipped', R.CTL_SKIPPED)):
            s = np.float32(0)
            for c in window:
                s = np.float32(s + c[slot])
            assert e[key] == float(s / np.float32(len(window))), (i, key)
        assert e['main/skipped'] == 0. and e['main/grad_norm'] > 0 and 'main/loss' in e
    # the threshold was in play: some step clipped (factor < 1), by chainer's rate
    clipped = [c for c in ctl if c[R.CTL_NORM] > CLIP]
    assert clipped, [float(c[R.CTL_NORM]) for c in ctl]
    for c in ctl:
        if c[R.CTL_NORM] > CLIP:       # the float norm and the float factor: one rounding each
            assert abs(c[R.CTL_FACTOR] - CLIP / c[R.CTL_NORM]) <= 2.0 ** -22 * CLIP / c[R.CTL_NORM]
        elif c[R.CTL_NORM] < CLIP:
            assert c[R.CTL_FACTOR] == 1.0


# ---- two ranks on the one GPU --------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


W2_CLIP = 40.          # the averaged gradient's norm of this batch and these seeds is about 145


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank),
                      WORLD_SIZE=str(world), MRCNN_DP_REHEARSAL='1')
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import torch.distributed as dist
    from chainer_mask_rcnn_amd import parallel
    r, w, local = parallel.init_from_env()
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    conv.WINOGRAD_MIN_WORK = 1 << 24          # as tests/conftest.py
    model, chain, opt = build_small(dev, (optimizers.GradientClipping(W2_CLIP),), seed=10 + rank)
    local_grads = {}

    class Recording(parallel.TorchDistExchange):
        def allreduce_async(self, tensor, bucket_id=0):
            torch.cuda.synchronize()
            local_grads[(tensor.data_ptr(), tensor.numel())] = tensor.detach().cpu().numpy().copy()
            super().allreduce_async(tensor, bucket_id)

    parallel.DataParallelGradSync(opt, exchange=Recording(), bucket_bytes=4 << 20)
    opt._build()
    arena = opt.arena
    w0 = arena.values.detach().cpu().numpy().copy()
    base = arena.grads.data_ptr()
    inputs = batch(dev, flip=bool(rank))
    np.random.seed(5 + rank)
    loss = opt.update(chain, *inputs)
    torch.cuda.synchronize()
    w1 = arena.values.detach().cpu().numpy()
    ctl = opt._ctl.cpu().numpy()
    mine = np.zeros_like(w0)
    covered = np.zeros(w0.shape, bool)
    for (ptr, n), g in local_grads.items():
        off = (ptr - base) // 4
        mine[off:off + n] = g
        covered[off:off + n] = True
    gathered = [None] * world
    dist.all_gather_object(gathered, (mine, covered, float(loss.detach()), w1.copy(), ctl.copy()))
    ok = {}
    ok['covered every trainable slice'] = bool(all(c.all() for _, c, _, _, _ in gathered))
    ok['ranks bit-identical after the step'] = bool(all(np.array_equal(g[3], gathered[0][3]) for g in gathered))
    ok['same control word on every rank'] = bool(all(np.array_equal(g[4], gathered[0][4]) for g in gathered))
    ok['ranks saw different batches'] = gathered[0][2] != gathered[1][2]
    mean_g = sum(g[0].astype(np.float64) for g in gathered) / world
    norm = math.sqrt(float(np.sum(mean_g * mean_g)))
    # the device takes the norm of the fp32 sum over ranks times 1/world: each element one fp32
    # rounding (2^-24) from the exact sum, the float result one more, the factor a third
    ok['norm of the averaged gradient'] = bool(abs(ctl[R.CTL_NORM] - norm) <= 2.0 ** -22 * norm)
    clip = float(np.float32(W2_CLIP))
    ratio = float(ctl[R.CTL_FACTOR]) * world            # factor / (1 / world)
    ok['clipping by threshold / norm'] = bool(
        ctl[R.CTL_SKIPPED] == 0. and abs(ratio - clip / norm) <= 2.0 ** -22 * clip / norm)
    # a ratio that matters in the update below: the threshold sits well inside the gradient's norm
    ok['the factor is in play'] = bool(0.05 < ratio < 0.9)
    step = -LR * (ratio * mean_g + WD * w0.astype(np.float64))
    # tests/test_gpu_parallel_world2.py's bound: one fp32 fma chain per element
    err = np.abs((w1.astype(np.float64) - w0) - step).max() / (1e-4 * np.abs(step).max() + 2e-7 * np.abs(w0).max())
    ok['w1 == w0 - lr (ratio mean gradient + wd w0)'] = bool(err <= 1.0 and np.abs(step).max() > 0)
    ok['finite'] = bool(np.isfinite(w1).all())
    q.put((rank, ok, float(err), float(norm), ctl.tolist()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.is_available() and torch.cuda.device_count() >= 2,
                    reason='the rehearsal mode (two ranks on one device over gloo) refuses to start '
                           'on a node with a GPU per rank')
def test_two_ranks_sharing_the_gpu_clip_alike(dev):
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0
    res = sorted(q.get(timeout=10) for _ in range(2))
    for rank, ok, err, norm, ctl in res:
        print('rank %d: norm %.6g, control word %s, error / bound %.2f' % (rank, norm, ctl, err))
        assert all(ok.values()), (rank, ok, err, norm, ctl)
