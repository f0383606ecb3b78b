"""chainermn.scatter_dataset without a communicator: every rank builds the whole dataset and keeps
an index view of its shard, so nothing travels between ranks."""
import numpy as np


class SubDataset(object):
    """chainer.datasets.SubDataset(dataset, start, finish, order): examples ``order[start:finish]``
    of ``dataset`` (``start:finish`` itself without an order)."""

    def __init__(self, dataset, start, finish, order=None):
        if not 0 <= start <= finish <= len(dataset):
            raise ValueError('shard [%d, %d) outside a dataset of %d examples'
                             % (start, finish, len(dataset)))
        self._dataset, self._start, self._finish = dataset, int(start), int(finish)
        self._order = order

    def __len__(self):
        return self._finish - self._start

    @property
    def indices(self):
        """The dataset indices of this shard's examples, in order."""
        idx = np.arange(self._start, self._finish)
        return idx if self._order is None else np.asarray(self._order)[idx]

    def __getitem__(self, i):
        if not 0 <= i < len(self):
            raise IndexError('index %d out of a shard of %d examples' % (i, len(self)))
        j = i + self._start
        return self._dataset[int(j if self._order is None else self._order[j])]

    get_example = __getitem__


def scatter_dataset(dataset, rank, world, shuffle=False, seed=None, force_equal_length=True):
    """Rank ``rank``'s shard of ``dataset`` as chainermn.scatter_dataset cuts it: the order is
    ``RandomState(seed).permutation(n)`` with ``shuffle`` (a private stream: the global
    ``np.random`` is untouched), else ``arange(n)``; shard i starts at ``n * i // world`` and holds
    ``ceil(n / world)`` examples with ``force_equal_length`` (every rank the same iterations per
    epoch; the last ones overlap their neighbours), else it ends at ``n * (i + 1) // world``
    (disjoint contiguous shards: the test split).  World size 1 returns ``dataset`` itself."""
    if world == 1:
        return dataset
    if not 0 <= rank < world:
        raise ValueError('rank %d outside world size %d' % (rank, world))
    n = len(dataset)
    order = np.random.RandomState(seed).permutation(n) if shuffle else None
    start = n * rank // world
    if force_equal_length:
        finish = start + (n + world - 1) // world
    else:
        finish = n * (rank + 1) // world
    return SubDataset(dataset, start, finish, order)
