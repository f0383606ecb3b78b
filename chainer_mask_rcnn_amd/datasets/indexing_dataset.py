"""IndexingDataset — the reference's chainer_mask_rcnn/datasets/indexing_dataset.py: the
examples of ``dataset`` at ``indices`` (an int is a one-element list)."""


class IndexingDataset(object):

    def __init__(self, dataset, indices=0):
        self._dataset = dataset
        if isinstance(indices, int):
            indices = [indices]
        self._indices = indices
        self._size = len(indices)

    def __len__(self):
        return self._size

    def get_example(self, i):
        index = self._indices[i]
        ds = self._dataset
        return ds.get_example(index) if hasattr(ds, 'get_example') else ds[index]

    def __getitem__(self, i):
        return self.get_example(i)
