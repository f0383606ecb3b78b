"""COCO's polygon rule, restated literally in pure Python from pycocotools' maskApi.c rleFrPoly
(cocoapi common/maskApi.c): upsample by 5, walk every edge point by point, collect the crossings
of pixel-column centres, sort ``x * h + y``, turn the differences into run lengths, decode them
column-major; an instance is the union of its rings (frPyObjects + rleMerge).

Kept independent of the package: no NumPy arithmetic in the rule (Python floats are IEEE doubles,
never fused), the sort-and-difference form of the fill and not the XOR form the package and the
kernel use.  pycocotools itself is not available to these tests, so this restatement is — like the
RLE codec of oracle/np_data.py — unpinned against the real library.

Also the cases the CPU and GPU tests share."""
import math

import numpy as np

SCALE = 5.0


def walk(ring):
    """The dense walk of one ring ``[x0, y0, x1, y1, ...]``: the lists u, v of rleFrPoly."""
    xy = [float(c) for c in ring]
    k = len(xy) // 2
    x = [int(SCALE * xy[2 * j] + .5) for j in range(k)]
    y = [int(SCALE * xy[2 * j + 1] + .5) for j in range(k)]
    x.append(x[0])
    y.append(y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe = xe, xs
            ys, ye = ye, ys
        if dx >= dy:
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                # dx == 0: C computes (int)NaN here and never reads it
                v.append(int(ys + ((ye - ys) / dx) * t + .5) if dx else ys)
        else:
            s = (xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + .5))
    return u, v


def crossings(ring, h, w):
    """[(x, y)] in walking order: 0 <= x < w, 0 <= y <= h."""
    if len(ring) // 2 < 3:
        return []
    u, v = walk(ring)
    out = []
    for j in range(1, len(u)):
        if u[j] != u[j - 1]:
            xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
            xd = (xd + .5) / SCALE - .5
            if math.floor(xd) != xd or xd < 0 or xd > w - 1:
                continue
            yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
            yd = (yd + .5) / SCALE - .5
            if yd < 0:
                yd = 0.
            elif yd > h:
                yd = float(h)
            out.append((int(xd), int(math.ceil(yd))))
    return out


def ring_mask(ring, h, w):
    """One ring -> (h, w) uint8: sorted positions, differences, zero runs merged, column-major
    decode — the tail of rleFrPoly followed by rleDecode."""
    a = sorted(x * h + y for x, y in crossings(ring, h, w)) + [h * w]
    d, p = [], 0
    for t in a:
        d.append(t - p)
        p = t
    b, j = [d[0]], 1
    while j < len(d):
        if d[j] > 0:
            b.append(d[j])
            j += 1
        else:
            j += 1
            if j < len(d):
                b[-1] += d[j]
                j += 1
    flat, pos, val = np.zeros(h * w, np.uint8), 0, 0
    for c in b:
        flat[pos:pos + c] = val
        pos += c
        val ^= 1
    assert pos == h * w
    return flat.reshape(w, h).T


def mask(rings, h, w):
    """An instance: the union of its rings."""
    out = np.zeros((h, w), np.uint8)
    for ring in rings:
        out |= ring_mask(ring, h, w)
    return out


def tight_box(m):
    """(y1, x1, y2, x2), zeros for an empty mask."""
    ys, xs = np.nonzero(m)
    return (int(ys.min()), int(xs.min()), int(ys.max()) + 1, int(xs.max()) + 1) if ys.size else (0, 0, 0, 0)


def packbits(masks):
    """(G, H, W) {0,1} -> (G, H, Wq) int64 bit pattern of the packed format."""
    masks = np.asarray(masks)
    G, H, W = masks.shape
    Wq = (W + 63) // 64
    padded = np.zeros((G, H, Wq * 64), np.uint8)
    padded[:, :, :W] = masks != 0
    return np.packbits(padded, axis=-1, bitorder='little').view(np.uint64).view(np.int64).reshape(G, H, Wq)


# ------------------------------------------------------------------------------------ the cases
SQUARE = [1, 1, 4, 1, 4, 4, 1, 4]
TRIANGLE = [0, 0, 3, 0, 3, 3]
COVER = [-5, -5, 100, -5, 100, 100, -5, 100]
STRADDLE = [63.4, 0.2, 64.6, 0.2, 64.6, 4.7, 63.4, 4.7]
BOWTIE = [1, 1, 8, 8, 8, 1, 1, 8]
FMA_TRIANGLE = [24.0, 15.6, 20.0, 3.8, 5.6, 14.0]

# (name, rings, h, w)
KNOWN = [
    ('square', [SQUARE], 6, 6),
    ('triangle', [TRIANGLE], 5, 5),
    ('cover', [COVER], 7, 70),
    ('straddle', [STRADDLE], 5, 130),
    ('bowtie', [BOWTIE], 10, 10),
    ('one_vertex', [[2, 2]], 5, 5),
    ('two_vertices', [[1, 1, 3, 3]], 5, 5),
    ('fma_triangle', [FMA_TRIANGLE], 40, 40),
]


def random_ring(rng, trial, h, w, k=None):
    """1..8 vertices from -10 to size + 10; thirds of the trials rounded to halves, integers, fifths."""
    k = int(rng.randint(1, 9)) if k is None else k
    xy = np.stack([rng.uniform(-10, w + 10, k), rng.uniform(-10, h + 10, k)], 1)
    if trial % 3 == 0:
        xy = np.round(xy * 2) / 2
    elif trial % 3 == 1:
        xy = np.round(xy)
    else:
        xy = np.round(xy * 5) / 5
    return xy.reshape(-1).tolist()


def random_rings(n=320, seed=7):
    """[(ring, h, w)]: sizes 1..80 x 1..150."""
    rng = np.random.RandomState(seed)
    out = []
    for trial in range(n):
        h, w = int(rng.randint(1, 81)), int(rng.randint(1, 151))
        out.append((random_ring(rng, trial, h, w), h, w))
    return out


def random_instances(n, h, w, seed, min_vertices=1):
    """n instances of 1..3 rings on one h x w image."""
    rng = np.random.RandomState(seed)
    return [[random_ring(rng, int(rng.randint(0, 3)), h, w, int(rng.randint(min_vertices, 9)))
             for _ in range(int(rng.randint(1, 4)))] for _ in range(n)]


# ------------------------------------------------------------------ a synthetic annotation file
def rle_counts(m):
    """(H, W) mask -> COCO's uncompressed counts (column-major runs, zeros first)."""
    flat = (np.asarray(m) != 0).astype(np.int8).T.reshape(-1)
    change = np.flatnonzero(np.diff(np.concatenate([[0], flat])))
    return np.diff(np.concatenate([[0], change, [flat.size]])).astype(int).tolist()


RLE_BLOB = np.zeros((12, 70), np.uint8)
RLE_BLOB[2:9, 60:68] = 1
RLE_CROWD = np.zeros((12, 70), np.uint8)
RLE_CROWD[0:5, 3:40] = 1
TWO_RINGS = [[5.5, 1.0, 30.0, 1.5, 28.0, 10.5, 4.0, 9.0], [20.0, 4.0, 66.5, 5.0, 50.0, 11.5]]


def write_coco(root):
    """instances_minival2014.json under ``root``: image 21 (6 x 6) the square; image 22 (12 x 70)
    a two-ring polygon, a run-length instance and a run-length crowd; image 23 (9 x 8) a
    run-length annotation of the wrong size (dropped) and the triangle."""
    import json
    import os
    os.makedirs(os.path.join(root, 'annotations'), exist_ok=True)
    images = [dict(id=21, height=6, width=6), dict(id=22, height=12, width=70),
              dict(id=23, height=9, width=8)]
    cats = [dict(id=c, name='cat%d' % c) for c in (1, 3, 18)]
    anns = [
        dict(id=1, image_id=21, category_id=1, iscrowd=0, area=9., segmentation=[SQUARE]),
        dict(id=2, image_id=22, category_id=3, iscrowd=0, area=300., segmentation=TWO_RINGS),
        dict(id=3, image_id=22, category_id=18, iscrowd=0, area=56.,
             segmentation={'size': [12, 70], 'counts': rle_counts(RLE_BLOB)}),
        dict(id=4, image_id=22, category_id=1, iscrowd=1, area=185.,
             segmentation={'size': [12, 70], 'counts': rle_counts(RLE_CROWD)}),
        dict(id=5, image_id=23, category_id=3, iscrowd=0, area=4.,
             segmentation={'size': [5, 4], 'counts': [0, 4, 16]}),
        dict(id=6, image_id=23, category_id=18, iscrowd=0, area=3., segmentation=[TRIANGLE]),
    ]
    with open(os.path.join(root, 'annotations', 'instances_minival2014.json'), 'w') as f:
        json.dump(dict(images=images, annotations=anns, categories=cats), f)
    return images, anns
