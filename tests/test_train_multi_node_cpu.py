"""Data-parallel pieces of tools/train.py without a device: scatter_dataset's shards, the exact
sharded evaluation's gather-and-merge at world size 2 over gloo (against one process evaluating
the concatenated records), the rank-order float32 mean of the log sums, the Open MPI -> torch
launcher mapping and the launch refusals."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from chainer_mask_rcnn_amd.datasets import scatter_dataset
from chainer_mask_rcnn_amd.extensions import instance_segmentation_evaluators as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import train  # noqa: E402
from chainer_mask_rcnn_amd.utils.evaluations.records import EvalRecords  # noqa: E402
from records_util import ATTRS, same_lists, take  # noqa: E402
import trainer as T  # noqa: E402

TIMEOUT = 120


# ---- scatter_dataset -------------------------------------------------------------------------
@pytest.mark.parametrize('n,world', [(10, 2), (7, 3), (5, 4), (3, 8), (16, 8), (1, 2)])
def test_train_shards_have_equal_lengths_and_cover_the_dataset(n, world):
    data = list(range(100, 100 + n))
    shards = [scatter_dataset(data, r, world, shuffle=True, seed=0) for r in range(world)]
    m = -(-n // world)
    order = np.random.RandomState(0).permutation(n)
    seen = set()
    for r, s in enumerate(shards):
        assert len(s) == m
        got = [s[i] for i in range(len(s))]
        start = n * r // world
        assert got == [data[j] for j in order[start:start + m]]
        assert list(s.indices) == list(order[start:start + m])
        seen.update(got)
        with pytest.raises(IndexError):
            s[len(s)]
    assert seen == set(data)


def test_train_shards_are_reproducible_from_the_seed():
    data = list(range(50))
    a = [list(scatter_dataset(data, r, 4, shuffle=True, seed=3).indices) for r in range(4)]
    b = [list(scatter_dataset(data, r, 4, shuffle=True, seed=3).indices) for r in range(4)]
    c = [list(scatter_dataset(data, r, 4, shuffle=True, seed=4).indices) for r in range(4)]
    assert a == b and a != c
    state = np.random.get_state()
    scatter_dataset(data, 0, 4, shuffle=True, seed=3)
    assert np.array_equal(np.random.get_state()[1], state[1])       # global stream untouched


@pytest.mark.parametrize('n,world', [(10, 2), (7, 3), (3, 2), (2, 4), (9, 8)])
def test_test_shards_are_disjoint_contiguous_and_in_order(n, world):
    data = list(range(n))
    got = []
    for r in range(world):
        s = scatter_dataset(data, r, world, force_equal_length=False)
        idx = [s[i] for i in range(len(s))]
        assert idx == list(range(n * r // world, n * (r + 1) // world))
        got += idx
    assert got == data                       # rank order is the dataset's order, no repeats


def test_world_one_returns_the_dataset():
    data = list(range(5))
    assert scatter_dataset(data, 0, 1, shuffle=True, seed=0) is data
    assert scatter_dataset(data, 0, 1, force_equal_length=False) is data


# ---- exact sharded evaluation ----------------------------------------------------------------
def _records(kind, seed=0, n_img=9):
    """collect()-shaped records: ragged P x G counts, images without predictions or ground truth,
    difficult (VOC) or crowd / area (COCO) flags."""
    rng = np.random.RandomState(seed)
    counts, pls, pss, gls, flags = [], [], [], [], []
    for i in range(n_img):
        G = 0 if i == 2 else rng.randint(1, 5)
        P = 0 if i == 5 else rng.randint(1, 9)
        ga = rng.randint(20, 400, G).astype(np.int64)
        pa = rng.randint(20, 400, P).astype(np.int64)
        inter = np.zeros((P, G), np.int64)
        for p in range(P):
            if G and rng.uniform() < 0.8:
                g = rng.randint(G)
                inter[p, g] = rng.randint(0, min(pa[p], ga[g]) + 1)
        counts.append((inter, pa, ga))
        pls.append(rng.randint(0, 3, P).astype(np.int32))
        ps = rng.uniform(0, 1, P).astype(np.float32)
        if P > 2:
            ps[1] = ps[0]                                       # ties across the ranks' records
        pss.append(ps)
        labels = rng.randint(0, 3, G).astype(np.int32)
        rng.uniform(0, 50, (G, 4)), rng.uniform(size=(G, 8, 8))     # the example's boxes and masks
        gls.append(labels)
        if kind == 'voc':
            flags.append(((rng.uniform(size=G) < 0.3),))
        else:
            flags.append(((rng.uniform(size=G) < 0.25).astype(np.int32),
                          ga.astype(np.float32) * np.float32(rng.uniform(0.8, 1.2))))
    names = ('gt_difficults',) if kind == 'voc' else ('gt_crowdeds', 'gt_areas')
    return EvalRecords(pls, pss, gls, tables={'segm': counts},
                       **{k: [f[i] for f in flags] for i, k in enumerate(names)})


def _evaluator(kind):
    names = ['a', 'b', 'c']
    if kind == 'voc':
        return E.InstanceSegmentationVOCEvaluator(None, None, use_07_metric=True, label_names=names)
    return E.InstanceSegmentationCOCOEvaluator(None, None, label_names=names)


def _shard(records, rank, world):
    n = len(records)
    return take(records, n * rank // world, n * (rank + 1) // world)


class _Collected(object):
    """An evaluator whose device part returns fixed records."""

    def __init__(self, evaluator, records):
        self.evaluator, self.records = evaluator, records

    def collect(self):
        return self.records

    def evaluate_collected(self, records):
        return self.evaluator.evaluate_collected(records)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                      LOCAL_RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from chainer_mask_rcnn_amd import parallel
    parallel.init_from_env(backend='gloo')
    out = {}
    for kind in ('voc', 'coco'):
        records = _shard(_records(kind), rank, world)
        ev = E.create_multi_node_evaluator(_Collected(_evaluator(kind), records))
        out[kind] = ev.evaluate()
        merged = E.gather_records(records)
        out[kind + '/stripped'] = set(vars(merged)) == ATTRS and set(merged.tables) == {'segm'}
        out[kind + '/n'] = len(merged.tables['segm'])
    # the log reduction: every rank's window sums, rank-order float32 mean
    rng = np.random.RandomState(rank)
    sums = (rng.standard_normal(6) * 1e3).astype(np.float32)
    per_rank = parallel.all_gather_object_cpu((('loss',) * 6, sums, 7))
    out['log'] = T.rank_order_mean([s for _, s, _ in per_rank], 7)
    out['run_dir'] = parallel.broadcast_object_cpu(('stamp-of-rank-%d' % rank, rank) if rank == 0
                                                   else None)
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_evaluation_equals_one_process_at_world_2():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=TIMEOUT) for _ in range(2))
    finally:
        for p in procs:
            p.join(TIMEOUT)
            if p.exitcode is None:
                p.kill()
    assert [p.exitcode for p in procs] == [0, 0]
    for kind in ('voc', 'coco'):
        want = _evaluator(kind).evaluate_collected(_records(kind))
        assert 'validation/main/map' in want
        for rank in (0, 1):
            got = res[rank][kind]
            assert sorted(got) == sorted(want)
            for k in want:
                assert np.array_equal(np.asarray(got[k]), np.asarray(want[k]), equal_nan=True), (kind, k)
                assert np.asarray(got[k]).dtype == np.asarray(want[k]).dtype, (kind, k)
            assert res[rank][kind + '/stripped'] and res[rank][kind + '/n'] == 9
    sums = [(np.random.RandomState(r).standard_normal(6) * 1e3).astype(np.float32) for r in (0, 1)]
    want = np.float32(sums[0] + sums[1]) / np.float32(14)
    for rank in (0, 1):
        assert res[rank]['log'].dtype == np.float32
        assert np.array_equal(res[rank]['log'].view(np.uint32), want.view(np.uint32))
        assert res[rank]['run_dir'] == ('stamp-of-rank-0', 0)


def test_rank_order_mean_is_a_float32_sequential_sum():
    rng = np.random.RandomState(0)
    sums = [(rng.standard_normal(6) * np.array([1e7, 1, 1e-3, 3e4, 1, 1])).astype(np.float32)
            for _ in range(5)]
    got = T.rank_order_mean(sums, 3)
    acc = sums[0].copy()
    for s in sums[1:]:
        acc = np.float32(acc + s)
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), (acc / np.float32(15)).view(np.uint32))
    # world size 1: the single-rank float32 _x / _n
    one = T.rank_order_mean(sums[:1], 3)
    assert np.array_equal(one, sums[0] / np.float32(3))


def test_records_keep_what_matching_reads():
    """The record never holds an example's boxes or masks: its attributes are the labels, the
    scores, the flags and the tables, and a pickle round trip (how it travels) keeps them."""
    import pickle
    rec = _records('coco', n_img=3)
    assert set(vars(rec)) == ATTRS == {'pred_labels', 'pred_scores', 'gt_labels', 'gt_difficults',
                                       'gt_crowdeds', 'gt_areas', 'tables'}
    assert rec.gt_difficults is None and len(rec.gt_crowdeds) == len(rec.gt_areas) == 3
    back = pickle.loads(pickle.dumps(rec))
    for h, g in zip(back.gt_labels + back.gt_crowdeds + back.gt_areas,
                    rec.gt_labels + rec.gt_crowdeds + rec.gt_areas):
        assert h.dtype == g.dtype and np.array_equal(h, g)
    m = EvalRecords.merge([rec, rec])
    assert same_lists(m.tables['segm'], rec.tables['segm'] * 2)
    assert same_lists(m.gt_labels, rec.gt_labels * 2)
    assert same_lists(m.gt_crowdeds, rec.gt_crowdeds * 2)
    assert same_lists(m.gt_areas, rec.gt_areas * 2)


# ---- launch ----------------------------------------------------------------------------------
def test_ompi_variables_map_onto_torch_names():
    ompi = dict(OMPI_COMM_WORLD_RANK='3', OMPI_COMM_WORLD_SIZE='4', OMPI_COMM_WORLD_LOCAL_RANK='3',
                OMPI_COMM_WORLD_LOCAL_SIZE='4')
    assert train.torch_env_from_ompi(ompi) == dict(
        RANK='3', WORLD_SIZE='4', LOCAL_RANK='3', LOCAL_WORLD_SIZE='4', MASTER_ADDR='127.0.0.1',
        MASTER_PORT='29500')
    kept = dict(ompi, MASTER_ADDR='10.0.0.1', MASTER_PORT='1234')
    env = train.torch_env_from_ompi(kept)
    assert 'MASTER_ADDR' not in env and 'MASTER_PORT' not in env and env['RANK'] == '3'
    assert train.torch_env_from_ompi(dict(ompi, RANK='0')) == {}       # torchrun's names win
    assert train.torch_env_from_ompi({}) == {}


def test_launch_checks():
    args = train.parse_args(['--dataset', 'synthetic'])
    assert train.launch_error(args, {}) is None
    assert train.launch_error(args, dict(WORLD_SIZE='1')) is None
    assert 'world size 2 is not supported' in train.launch_error(args, dict(WORLD_SIZE='2'))
    args = train.parse_args(['--multi-node'])
    assert 'not supported' in train.launch_error(args, {})
    assert train.launch_error(args, dict(RANK='0', WORLD_SIZE='2')) is None
    assert train.launch_error(args, dict(RANK='0', WORLD_SIZE='1')) is None


def test_multi_node_at_world_one_is_a_plain_run():
    args = train.parse_args(['--multi-node'])
    env = dict(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', LOCAL_WORLD_SIZE='1')
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        import torch.distributed as dist
        comm = train.setup_comm(args)
        assert (comm.rank, comm.world, comm.local, comm.n_node) == (0, 1, 0, 1)
        assert not comm.parallel and str(comm.device) == 'cuda:0'
        assert not dist.is_initialized()
        assert comm.broadcast(('a', 1)) == ('a', 1)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _launch(argv, env):
    base = {k: v for k, v in os.environ.items()
            if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK') and not k.startswith('OMPI_')}
    base.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train.py')] + argv,
                          capture_output=True, text=True, env=base, timeout=TIMEOUT)


def test_refusals():
    r = _launch(['--dataset', 'synthetic'], dict(WORLD_SIZE='2'))
    assert r.returncode != 0 and 'world size 2 is not supported without --multi-node' in r.stderr
    r = _launch(['--multi-node'], {})
    assert r.returncode != 0 and ('--multi-node is not supported without a launcher'
                                  in r.stderr)
    # mpirun -n 2 without --multi-node: two independent runs would race for one directory
    r = _launch(['--dataset', 'synthetic'], dict(OMPI_COMM_WORLD_RANK='0', OMPI_COMM_WORLD_SIZE='2',
                                                 OMPI_COMM_WORLD_LOCAL_RANK='0',
                                                 OMPI_COMM_WORLD_LOCAL_SIZE='2'))
    assert r.returncode != 0 and 'world size 2 is not supported' in r.stderr


# ---- rank-0-only extensions ------------------------------------------------------------------
class _Opt(object):
    lr = 0.01
    pending = False

    def has_pending(self):
        return self.pending


class _Loop(object):
    def __init__(self):
        self.iterator = type('It', (), dict(dataset=list(range(4)), batch_size=1))()
        self.optimizer = _Opt()
        self.iteration = 0


def test_rank_zero_only_refuses_pending_deferred_work():
    calls = []

    class Ext(object):
        priority = -100
        trigger = (1, 'epoch')

        def __call__(self, trainer):
            calls.append(trainer.iteration)
    tr = T.Trainer(_Loop(), (1, 'iteration'), out=None)
    ext = T.RankZeroOnly(Ext())
    assert ext.priority == -100 and ext.trigger == (1, 'epoch') and ext.name == 'Ext'
    ext(tr)
    assert calls == [0]
    tr.loop.optimizer.pending = True
    with pytest.raises(RuntimeError, match='rank 0 alone'):
        ext(tr)
    assert calls == [0]


def test_reference_set_per_rank():
    def names(rank, gather):
        tr = T.Trainer(_Loop(), (1, 'iteration'), out=None)
        T.extend_reference_set(tr, model=None, evaluator=object(), vis_iterator=[], class_names=['a'],
                               step_size=[0.5], params={}, rank=rank, gather=gather)
        return [(type(e.extension).__name__, getattr(e.extension, 'extension', None).__class__.__name__
                 if isinstance(e.extension, T.RankZeroOnly) else None) for e in tr._entries]
    plain = names(0, None)
    assert not any(w for _, w in plain)
    lead = names(0, lambda obj: [obj])
    assert [n for n, _ in lead] == [n if n not in ('snapshot_object', 'VisReport') else 'RankZeroOnly'
                                    for n, _ in plain]
    assert sorted(w for _, w in lead if w) == ['VisReport', 'snapshot_object']
    other = names(1, lambda obj: [obj, obj])
    assert [n for n, _ in other] == ['ExponentialShift', 'Evaluator', 'observe_lr', 'LogReport',
                                     'PlotReport']
