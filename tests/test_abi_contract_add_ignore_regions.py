"""Rows of the ABI contract's probe table (tests/abi_contract.py ``PROBES``) for
functions/ignore_regions.py, so that the sweeps of test_abi_contract_cpu.py and
test_gpu_abi_contract.py cover ``mrcnn_mask_union_pack`` and ``mrcnn_box_coverage`` like every other
entry point.

The rows are appended when this module is imported.  Both sweep modules build their parameter
lists from ``PROBES`` when THEY are imported, and pytest imports the modules of a directory in name
order — hence this file's name, which sorts before ``test_abi_contract_cpu``.  The sweeps see the
rows in any run that collects this directory (the whole suite, ``-m gpu``); a run of
test_abi_contract_cpu.py by itself does not, and its completeness test then names the two entry
points as uncovered.  The tests below run the same sweep on the rows directly, so the rows are
checked wherever this file is."""
import numpy as np
import pytest
import torch

import abi_contract as A

NAMES = ('ignore_regions.union_plane', 'ignore_regions.box_coverage')


def _register():
    if any(p.name in NAMES for p in A.PROBES):
        return

    @A.probe(NAMES[0], ('masks_u8', 'base'))
    def _p(dev):
        from chainer_mask_rcnn_amd.functions import ignore_regions as IR
        a = dict(masks_u8=A._masks(dev, 3, 5, 70), base=A._words(dev, 1, 5, 70, seed=2)[0])
        return a, lambda a: IR.union_plane(a['masks_u8'], a['base'])

    @A.probe(NAMES[1], ('plane', 'boxes'))
    def _p(dev):
        from chainer_mask_rcnn_amd.functions import ignore_regions as IR
        boxes = np.array([[0, 0, 5, 70], [1.5, 2.5, 4.5, 66], [-3, 60, 9, 200], [4, 4, 2, 2]], np.float32)
        a = dict(plane=A._words(dev, 1, 5, 70, seed=1)[0], boxes=A._f(boxes, dev))
        return a, lambda a: IR.box_coverage(a['plane'], 70, a['boxes'])


_register()
ROWS = [p for p in A.PROBES if p.name in NAMES]


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from chainer_mask_rcnn_amd import _lib
    _lib.load()
    return _lib


@pytest.mark.parametrize('p', ROWS, ids=[p.name for p in ROWS])
def test_dry_sweep_of_the_ignore_region_rows(lib, p):
    fails, entries = A.dry_sweep(p, torch.device('cpu'))
    assert not fails, '\n'.join(fails)
    assert set(entries) == {'mrcnn_mask_union_pack' if p.name == NAMES[0] else 'mrcnn_box_coverage'}


def test_rows_are_in_the_table_the_sweeps_read():
    import sys
    assert len(ROWS) == 2
    mod = sys.modules.get('test_abi_contract_cpu')
    if mod is not None:     # collected in the same run: it must have seen the rows
        assert {p.name for p in mod.CPU_PROBES} >= set(NAMES)
