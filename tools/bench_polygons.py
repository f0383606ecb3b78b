"""Times of ground-truth polygons -> packed masks on the device, two routes
for the same image in the same run: an 800 x 1333 image with 8 instances, and one with 100.

  a. device route     — ``functions.rasterize_polygons`` of a ``datasets.PolygonMasks``: the vertex
                        tables are upsampled on the host and uploaded (a few KB), then
                        ``mrcnn_polygon_rasterize`` draws COCO's rule.
       a_total_ms        host clock around the call, ending in a device synchronise
       a_host_ms         of that, the host part (``upsample_vertices``), timed by itself
       a_kernel_ms       device events around back-to-back ``mrcnn_polygon_rasterize`` calls on
                         tables already on the device
  b. the route it replaces — ``PIL.ImageDraw.polygon`` per instance on the host, the dense
                        (G, H, W) int32 stack uploaded, ``mrcnn_mask_pack`` (``pack_masks``).
       b_total_ms        host clock around all of it, ending in a device synchronise
       b_host_draw_ms    the PIL drawing and the stacking, by itself
       b_device_ms       host clock around upload + pack of a stack already drawn, synchronised
       b_kernel_ms       device events around back-to-back ``mrcnn_mask_pack`` calls on a stack
                         already on the device

The two routes draw by different rules (PIL's masks are about a pixel fatter), so their words are
not compared; route a's words are checked against the host rule before anything is timed.  The
alternated medians over ``--reps`` rounds are what DESIGN.md quotes.  Writes
profiles/polygons.json.  Nothing is gated on these numbers.

    python tools/bench_polygons.py [--reps 30] [--out profiles/polygons.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chainer_mask_rcnn_amd import _lib  # noqa: E402
from chainer_mask_rcnn_amd import functions as F  # noqa: E402
from chainer_mask_rcnn_amd.datasets import PolygonMasks  # noqa: E402
from chainer_mask_rcnn_amd.functions import polygons as P  # noqa: E402
from chainer_mask_rcnn_amd.utils.evaluations import masks as M  # noqa: E402

from bench_scale_jitter import back_to_back_ms  # noqa: E402

H, W = 800, 1333


def instances(rng, G):
    """G star-shaped polygons of 8..60 vertices, 40..500 pixels across, as COCO objects are."""
    out = []
    for _ in range(G):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        ry, rx = rng.uniform(20, 250, 2)
        k = int(rng.randint(8, 61))
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        rad = rng.uniform(0.6, 1.0, k)
        ring = np.stack([cx + rx * rad * np.cos(ang), cy + ry * rad * np.sin(ang)], 1).round(2)
        out.append([ring.reshape(-1).tolist()])
    return out


def pil_stack(insts):
    import PIL.Image
    import PIL.ImageDraw
    out = np.empty((len(insts), H, W), np.int32)
    for g, rings in enumerate(insts):
        canvas = PIL.Image.new('L', (W, H), 0)
        pen = PIL.ImageDraw.Draw(canvas)
        for ring in rings:
            pen.polygon(xy=list(map(tuple, np.asarray(ring).reshape(-1, 2))), outline=1, fill=1)
        out[g] = np.asarray(canvas) == 1
    return out


def host_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def case(G, reps, dev, rng):
    insts = instances(rng, G)
    polys = PolygonMasks(H, W, insts)
    sync = torch.cuda.synchronize

    def route_a():
        F.rasterize_polygons(polys, dev)
        sync()

    def route_b():
        M.pack_masks(pil_stack(insts), device=dev)
        sync()

    stack = pil_stack(insts)

    def b_device():
        M.pack_masks(stack, device=dev)
        sync()

    got = F.rasterize_polygons(polys, dev)[0].cpu().numpy()
    assert np.array_equal(got, polys.to_packed().words.view(np.int64)), 'device words differ from the host rule'
    for fn in (route_a, route_b, b_device):
        fn()
    times = {k: [] for k in ('a_total_ms', 'a_host_ms', 'b_total_ms', 'b_host_draw_ms', 'b_device_ms')}
    for _ in range(reps):                                # alternated: both routes see the same machine
        times['a_total_ms'].append(host_ms(route_a))
        times['b_total_ms'].append(host_ms(route_b))
        times['a_host_ms'].append(host_ms(lambda: P.upsample_vertices(insts)))
        times['b_host_draw_ms'].append(host_ms(lambda: pil_stack(insts)))
        times['b_device_ms'].append(host_ms(b_device))
    tables = P.upsample_vertices(insts)
    t = [torch.from_numpy(a.reshape(-1)).to(dev) for a in tables]
    Wq = (W + 63) // 64
    packed = torch.empty((G, H, Wq), dtype=torch.int64, device=dev)
    area, extent, box = (torch.empty(s, dtype=torch.int32, device=dev) for s in ((G,), (G, 4), (G, 4)))
    ws = torch.empty((_lib.load().mrcnn_polygon_rasterize_workspace_bytes(G, H, W),), dtype=torch.uint8, device=dev)
    stack_d = torch.from_numpy(stack).to(dev)

    def a_kernel():
        _lib.call('mrcnn_polygon_rasterize', _lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), G, H, W,
                  _lib.ptr(packed), _lib.ptr(area), _lib.ptr(extent), _lib.ptr(box), _lib.ptr(ws),
                  _lib.stream_ptr())

    def b_kernel():
        _lib.call('mrcnn_mask_pack', _lib.ptr(stack_d), 4, G, H, W, _lib.ptr(packed), _lib.ptr(area),
                  _lib.ptr(extent), _lib.stream_ptr())

    res = {'instances': G, 'vertices': int(len(tables[0])),
           'a_upload_bytes': int(sum(a.nbytes for a in tables)), 'b_upload_bytes': int(stack.nbytes),
           'packed_bytes': int(G * H * Wq * 8)}
    for k, v in times.items():
        res[k + '_median'], res[k + '_min'] = float(np.median(v)), float(np.min(v))
    res['a_kernel_ms'] = back_to_back_ms(a_kernel, 10 * reps)
    res['b_kernel_ms'] = back_to_back_ms(b_kernel, 10 * reps)
    res['a_over_b_total'] = res['a_total_ms_median'] / res['b_total_ms_median']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'polygons.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_polygons.py: no ROCm device')
    rng = np.random.RandomState(0)
    dev = torch.device('cuda:0')
    res = {'image': [H, W], 'reps': args.reps, 'device': torch.cuda.get_device_name(0),
           # (the 100-instance stack is 427 MB of int32: fewer rounds of it)
           'cases': [case(G, max(3, args.reps // (1 + G // 25)), dev, rng) for G in (8, 100)]}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
