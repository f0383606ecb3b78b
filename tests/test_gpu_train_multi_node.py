"""tools/train.py --multi-node at world size 2 on the device: two ranks train a small VOC-like run
through the driver's own assembly (train.assemble) over two epochs, with the lr shift, the sharded
evaluation, the best snapshot and the reports.  The ranks end with bit-identical parameters after
training on their scatter_dataset shards; the lr follows the global batch; the log's losses are
the float32 rank-order means of both ranks' step losses; each sharded evaluation equals a plain
evaluator over the whole test set in the same process; only rank 0 writes, and
tools/evaluate.py --log-dir reproduces its best map.  The driver's command line is run once
under torch.distributed.run.

On a one-GPU box both ranks share device 0 (MRCNN_DP_REHEARSAL=1: gloo moves the gradients
through the host); the RCCL variant, one GPU per rank, needs a node with two or more GPUs."""
import argparse
import glob
import hashlib
import io
import json
import os
import socket
import subprocess
import sys
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, 'tools')
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

pytestmark = pytest.mark.gpu

N_GPU = torch.cuda.device_count() if torch.cuda.is_available() else 0
rehearsal_only = pytest.mark.skipif(
    N_GPU >= 2, reason='a node with a GPU per rank runs the RCCL variant instead: the rehearsal mode '
                       '(two ranks on one device over gloo) refuses to start there')
rccl_only = pytest.mark.skipif(N_GPU < 2, reason='the RCCL variant needs one GPU per rank (>= 2 GPUs)')

WORLD = 2
RANK_TIMEOUT = 900          # seconds, per rank and per queue read: a deadlocked collective fails
KEYS = ['loss', 'rpn_loc_loss', 'rpn_cls_loss', 'roi_loc_loss', 'roi_cls_loss', 'roi_mask_loss']
SETTINGS = dict(min_size=144, max_size=192, anchor_scales=(4, 8, 16, 32))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _write_voc_like(root, n=3, H=96, W=128):
    import PIL.Image
    rng = np.random.RandomState(3)
    for d in ('JPEGImages', 'SegmentationClass', 'SegmentationObject'):
        os.makedirs(os.path.join(root, d))
    for i in range(n):
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        cls = np.zeros((H, W), np.int32)
        ins = np.zeros((H, W), np.int32)
        for g in range(1 + i % 3):
            y0, x0 = rng.randint(0, H // 2), rng.randint(0, W // 2)
            h, w = rng.randint(20, H // 2), rng.randint(20, W // 2)
            cls[y0:y0 + h, x0:x0 + w] = rng.randint(1, 21)
            ins[y0:y0 + h, x0:x0 + w] = g + 1
            img[y0:y0 + h, x0:x0 + w] //= 2
        PIL.Image.fromarray(img).save(os.path.join(root, 'JPEGImages', 'img%02d.jpg' % i), quality=95)
        np.save(os.path.join(root, 'SegmentationClass', 'img%02d.npy' % i), cls)
        np.save(os.path.join(root, 'SegmentationObject', 'img%02d.npy' % i), ins)


class _StepRecorder(object):
    """Per step: the chain's report (host float32) and the lr the step used."""
    priority = 1000

    def __init__(self):
        self.reports, self.lrs = [], []

    def __call__(self, trainer):
        self.reports.append({k: np.float32(v.item()) for k, v in trainer.loop.chain.report.items()})
        self.lrs.append(trainer.loop.optimizer.lr)


class _EvalCheck(object):
    """After each (sharded) evaluation: its observation, and a plain evaluator's over the whole
    test set with the same weights, in this process."""
    priority = 200

    def __init__(self, plain):
        self.plain, self.sharded, self.whole = plain, [], []

    def __call__(self, trainer):
        import trainer as T
        self.sharded.append({k: float(v) for k, v in trainer.observation.items()
                             if k.startswith('validation/')})
        with T.between_steps(trainer):
            self.whole.append({k: float(v) for k, v in self.plain.evaluate().items()})


def _worker(rank, world, port, root, logs, rehearsal, q):
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                          LOCAL_RANK=str(rank), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world))
        if rehearsal:
            os.environ['MRCNN_DP_REHEARSAL'] = '1'
        else:
            os.environ.pop('MRCNN_DP_REHEARSAL', None)
        if TOOLS not in sys.path:
            sys.path.insert(0, TOOLS)
        import chainer_mask_rcnn_amd as cmr
        from chainer_mask_rcnn_amd import serializers
        from chainer_mask_rcnn_amd.functions import conv
        import train
        import train_loop as TL
        import trainer as T
        conv.WINOGRAD_MIN_WORK = 1 << 24       # as tests/conftest.py (and the parent's evaluate.py)

        args = train.parse_args(['--multi-node', '--dataset', 'custom', '--custom-root', root,
                                 '--max-epoch', '2', '--batch-size-per-gpu', '1',
                                 '--logs-dir', logs])
        comm = train.setup_comm(args)
        assert (comm.rank, comm.world) == (rank, world)
        voc = T.VOCLikeDataset(root)
        train_data = T.ConcatenatedDataset(voc, voc)            # 6 examples: 3 per rank
        test_data = T.VOCLikeDataset(root)                      # 3 examples: shards of 1 and 2
        train.configure(args, comm, voc.class_names, SETTINGS)
        model = train.build_model(args, None)
        run = train.assemble(args, comm, model, train_data, test_data, 'voc',
                             synthetic_weights=True, print_out=io.StringIO(),
                             eval_interval=(1, 'epoch'), log_interval=(2, 'iteration'),
                             plot_interval=(0.5, 'epoch'), print_interval=(2, 'iteration'))
        drawn = []
        next_indices = run.loop.iterator.next_indices

        def recording_next_indices():
            idx = next_indices()
            drawn.extend(int(run.train.indices[i]) for i in idx)
            return idx
        run.loop.iterator.next_indices = recording_next_indices

        steps = _StepRecorder()
        run.trainer.extend(steps)
        plain = cmr.extensions.InstanceSegmentationVOCEvaluator(
            TL.SerialIterator(TL.TransformDataset(test_data, cmr.datasets.MaskRCNNTransform(
                model, train=False)), 1, shuffle=False),
            model, use_07_metric=True, label_names=args.class_names)
        check = _EvalCheck(plain)
        run.trainer.extend(check, trigger=(1, 'epoch'))
        try:
            run.trainer.run()
        finally:
            run.loop.close()
        state = serializers.state_arrays(model)              # flushes the deferred updates (all ranks)
        torch.cuda.synchronize()
        digest = hashlib.sha256()
        for k in sorted(state):
            digest.update(k.encode())
            digest.update(np.ascontiguousarray(state[k]).tobytes())
        q.put((rank, dict(out=args.out, lr=args.lr, batch_size=args.batch_size, n_gpu=args.n_gpu,
                          iterations=run.trainer.iteration, shard=[int(i) for i in run.train.indices],
                          drawn=drawn, reports=steps.reports, lrs=steps.lrs,
                          final_lr=run.optimizer.lr, sharded=check.sharded,
                          whole=check.whole, digest=digest.hexdigest(),
                          exchange=run.optimizer.grad_sync.describe())))
        comm.close()
    except BaseException:                                # noqa: BLE001 — reported to the parent
        q.put((rank, 'error: ' + traceback.format_exc()))
        raise


def _spawn(tmp_path, rehearsal):
    root = str(tmp_path / 'custom')
    logs = str(tmp_path / 'logs')
    _write_voc_like(root)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, root, logs, rehearsal, q))
             for r in range(WORLD)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(WORLD):
            rank, out = q.get(timeout=RANK_TIMEOUT)
            assert not isinstance(out, str), 'rank %d: %s' % (rank, out)
            res[rank] = out
    finally:
        for p in procs:
            p.join(RANK_TIMEOUT)
            if p.exitcode is None:
                p.kill()
                p.join(10)
    assert [p.exitcode for p in procs] == [0] * WORLD
    return res, logs


def _check(res, logs):
    import yaml
    import trainer as T
    r0, r1 = res[0], res[1]
    # (1) bit-identical parameters after training
    assert r0['digest'] == r1['digest']
    # (2) the ranks trained on scatter_dataset's shards: 3 examples each of the 6, from seed 0
    order = np.random.RandomState(0).permutation(6)
    assert r0['shard'] == list(order[0:3]) and r1['shard'] == list(order[3:6])
    for r in (r0, r1):
        assert r['iterations'] == 6 and len(r['reports']) == 6
        assert sorted(r['drawn'][:3]) == sorted(r['shard'])          # epoch 1: the shard once
        assert set(r['drawn']) <= set(r['shard'])
    # (3) global batch and lr; the two lr shifts inside epoch 2
    for r in (r0, r1):
        assert r['n_gpu'] == 2 and r['batch_size'] == 2 and r['lr'] == 0.00125 * 2 * 1
        # shifts at epochs 4/3 and 16/9: the first after step 4, the second after the last step
        assert set(r['lrs']) == {0.0025, 0.0025 * 0.1} and r['lrs'] == sorted(r['lrs'], reverse=True)
        assert r['lrs'][0] == 0.0025 and r['lrs'][-1] == 0.0025 * 0.1
        assert r['final_lr'] == 0.0025 * 0.1 ** 2
    assert r0['lrs'] == r1['lrs']
    dirs = os.listdir(logs)
    assert len(dirs) == 1 and os.path.join(logs, dirs[0]) == r0['out'] == r1['out']
    out = r0['out']
    with open(os.path.join(out, 'params.yaml')) as f:
        params = yaml.safe_load(f)
    assert params['n_gpu'] == 2 and params['n_node'] == 1 and params['batch_size'] == 2
    assert params['lr'] == 0.0025 and params['multi_node'] is True
    # (4) the logged losses: float32 rank-order means of both ranks' step losses
    with open(os.path.join(out, 'log')) as f:
        log = json.load(f)
    assert [e['iteration'] for e in log] == [2, 4, 6]
    for e in log:
        it = e['iteration']
        sums = []
        for r in (r0, r1):
            s = np.zeros(len(KEYS), np.float32)
            for rep in r['reports'][it - 2:it]:
                s = np.float32(s + np.array([rep[k] for k in KEYS], np.float32))
            sums.append(s)
        want = T.rank_order_mean(sums, 2)
        for k, w in zip(KEYS, want):
            assert e['main/' + k] == float(w), (it, k)
    # (5) each sharded evaluation == a plain evaluator over the whole test set, same weights
    assert len(r0['sharded']) == len(r1['sharded']) == 2
    for r in (r0, r1):
        for sharded, whole in zip(r['sharded'], r['whole']):
            assert sorted(sharded) == sorted(whole)
            for k in whole:
                assert np.array_equal(sharded[k], whole[k], equal_nan=True), k
    assert r0['sharded'] == r1['sharded'] or all(
        np.array_equal(a[k], b[k], equal_nan=True) for a, b in zip(r0['sharded'], r1['sharded'])
        for k in a)
    # (6) only rank 0's directory, with the run's files
    for f in ('log', 'params.yaml', 'snapshot_model.npz', 'loss.png', 'accuracy.png'):
        assert os.path.exists(os.path.join(out, f)), f
    assert glob.glob(os.path.join(out, 'visualizations', 'iteration=*.jpg'))
    return out, [s['validation/main/map'] for s in r0['sharded']]


def _evaluate_log_dir(out, maps):
    """(7) tools/evaluate.py --log-dir reproduces the best map (first of equals), here: the same
    convolution routes as the workers (conv.WINOGRAD_MIN_WORK of tests/conftest.py)."""
    import evaluate
    import yaml
    best = None
    for m in maps:
        if best is None or m > best:
            best = m
    evaluate.evaluate_log_dir(argparse.Namespace(log_dir=out, limit=0, coco_root=None,
                                                 sbd_root=None, custom_root=None))
    with open(os.path.join(out, 'snapshot_model.npz.eval_result.yaml')) as f:
        got = yaml.safe_load(f)['validation/main/map']
    assert (got == best) or (np.isnan(got) and np.isnan(best)), (got, maps)


@rehearsal_only
def test_train_two_ranks_sharing_the_gpu(tmp_path, dev):
    res, logs = _spawn(tmp_path, rehearsal=True)
    assert 'gloo' in res[0]['exchange']['library'] and res[0]['exchange']['ranks'] == 2
    out, maps = _check(res, logs)
    _evaluate_log_dir(out, maps)


@rccl_only
def test_train_two_ranks_over_rccl(tmp_path, dev):
    res, logs = _spawn(tmp_path, rehearsal=False)
    assert 'RCCL' in res[0]['exchange']['library'] and res[0]['exchange']['ranks'] == 2
    out, maps = _check(res, logs)
    _evaluate_log_dir(out, maps)


@rehearsal_only
def test_train_cli_under_torch_distributed_run(tmp_path, dev):
    logs = str(tmp_path / 'logs')
    env = dict(os.environ, MRCNN_DP_REHEARSAL='1')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE'):
        env.pop(k, None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port()),
           os.path.join(ROOT, 'tools', 'train.py'), '--multi-node', '--dataset', 'synthetic',
           '--synthetic', '4', '--synthetic-epoch', '4', '--max-epoch', '1', '--no-plot',
           '--logs-dir', logs]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=RANK_TIMEOUT)
    assert r.returncode == 0, r.stderr[-3000:]
    dirs = os.listdir(logs)
    assert len(dirs) == 1, dirs
    out = os.path.join(logs, dirs[0])
    assert r.stdout.count('Saved logs: %s' % out) == 1                 # rank 0 prints, once
    for f in ('params.yaml', 'snapshot_model.npz'):
        assert os.path.exists(os.path.join(out, f)), f
