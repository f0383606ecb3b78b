"""Rows of the ABI contract's probe table (tests/abi_contract.py ``PROBES``) for
functions/polygons.py and the two hand-offs that reach it — ``functions.upload_packed_masks`` and
``utils.evaluations.masks.pack_masks`` given a ``datasets.PolygonMasks`` — so that the sweeps of
test_abi_contract_cpu.py and test_gpu_abi_contract.py cover ``mrcnn_polygon_rasterize`` like every
other entry point.

The rows are appended when this module is imported.  Both sweep modules build their parameter
lists from ``PROBES`` when THEY are imported, and pytest imports the modules of a directory in name
order — hence this file's name, which sorts before ``test_abi_contract_cpu``.  The sweeps see the
rows in any run that collects this directory (the whole suite, ``-m gpu``); a run of
test_abi_contract_cpu.py by itself does not, and its completeness test then names the entry point
as uncovered.  The tests below run the same sweep on the rows directly, so the rows are checked
wherever this file is.

The functions take host data (vertices, packed rows) and build every tensor they hand over
themselves, so the rows name no tensor to perturb: the sweep checks what the unperturbed call hands
to the library."""
import numpy as np
import pytest
import torch

import abi_contract as A

NAMES = ('polygons.rasterize_polygons', 'gt_masks.upload_packed_masks of PolygonMasks',
         'evaluations.masks.pack_masks of PolygonMasks')


def _polys(mixed):
    """Two polygon instances on a 5 x 70 image (one of two rings), with a packed row between them
    when ``mixed``."""
    from chainer_mask_rcnn_amd.datasets import PolygonMasks
    row = np.zeros((5, 2), np.uint64)
    row[1:3, 1] = 7
    insts = [[[1., 1., 60.5, 1., 66., 4.5, 2., 4.]]] + ([row] if mixed else []) + \
            [[[3., 0., 9., 0., 9., 5.], [62., 1., 69., 1., 69., 4., 62., 4.]]]
    return PolygonMasks(5, 70, insts)


def test_a_host_packed_masks_is_uploaded_without_a_launch(lib):
    from chainer_mask_rcnn_amd.utils.evaluations import masks as M
    with A.Recorder(dry=True) as rec:
        packed, area, extent = M.pack_masks(_polys(True).to_packed(), device=torch.device('cpu'))
    assert not rec.entries and packed.dtype == torch.int64 and tuple(packed.shape) == (3, 5, 2)
    assert area.tolist() == [int(a) for a in _polys(True).unpack().reshape(3, -1).sum(1)]
    assert extent.dtype == torch.int32 and extent[1].tolist() == [1, 3, 1, 2]


def _register():
    if any(p.name in NAMES for p in A.PROBES):
        return

    @A.probe(NAMES[0], ())
    def _p(dev):
        from chainer_mask_rcnn_amd.functions import polygons
        return dict(polys=_polys(False)), lambda a: polygons.rasterize_polygons(a['polys'], dev)

    @A.probe(NAMES[1], ())
    def _p(dev):
        from chainer_mask_rcnn_amd.functions import gt_masks
        return dict(polys=_polys(True)), lambda a: gt_masks.upload_packed_masks(a['polys'], dev)[0]

    @A.probe(NAMES[2], ())
    def _p(dev):
        from chainer_mask_rcnn_amd.utils.evaluations import masks as M
        return dict(polys=_polys(True)), lambda a: M.pack_masks(a['polys'], device=dev)


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
def test_dry_sweep_of_the_polygon_rows(lib, p):
    fails, entries = A.dry_sweep(p, torch.device('cpu'))
    assert not fails, '\n'.join(fails)
    assert set(entries) == {'mrcnn_polygon_rasterize'}


def test_what_crosses_is_the_vertex_tables_and_the_outputs(lib):
    """One int32 upload holds xy5, ring_off and inst_off; the outputs are int64 words and int32
    area / extent / box; the workspace is as large as the library asks."""
    with A.Recorder(dry=True) as rec:
        ROWS[0].run(torch.device('cpu'))
    assert not rec.violations()
    got = {c.param: (c.dtype, c.shape) for c in rec.crossings}
    assert got['xy5'] == (torch.int32, (2 * 11,)) and got['ring_off'] == (torch.int32, (4,))
    assert got['inst_off'] == (torch.int32, (3,))
    assert got['packed'] == (torch.int64, (2, 5, 2)) and got['area'] == (torch.int32, (2,))
    assert got['extent'] == (torch.int32, (2, 4)) and got['box'] == (torch.int32, (2, 4))
    assert got['ws'][0] == torch.uint8
    assert got['ws'][1][0] >= lib.load().mrcnn_polygon_rasterize_workspace_bytes(2, 5, 70) == 2 * 2 * 5 * 4


def test_entry_refuses_bad_shapes_without_a_launch(lib):
    L = lib.load()
    assert L.mrcnn_polygon_rasterize_workspace_bytes(0, 5, 70) == 0
    assert L.mrcnn_polygon_rasterize(None, None, None, 0, 5, 70, None, None, None, None, None, None) == 0
    for G, H, W in ((1, 0, 7), (1, 7, 0), (-1, 5, 5), (1, 4001, 5), (1, 1 << 11, 1 << 20)):
        assert L.mrcnn_polygon_rasterize(None, None, None, G, H, W, None, None, None, None, None, None) != 0
        assert b'polygon_rasterize' in L.mrcnn_last_error()
    assert L.mrcnn_polygon_rasterize(None, None, None, 1, 5, 5, None, None, None, None, None, None) != 0
    assert b'null pointer' in L.mrcnn_last_error()
    assert L.mrcnn_abi_version() == 1


def test_rows_are_in_the_table_the_sweeps_read():
    import sys
    assert len(ROWS) == len(NAMES)
    mod = sys.modules.get('test_abi_contract_cpu')
    if mod is not None:     # collected in the same run: it must have seen the rows
        assert {p.name for p in mod.CPU_PROBES} >= set(NAMES)
