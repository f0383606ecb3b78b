"""chainer_mask_rcnn_amd.streams: three getters, one stream each per device for the whole process,
every one created at its own first use (the order of creation decides which streams share a
hardware queue, so no getter may create another's stream)."""
import os
import subprocess
import sys

import pytest
import torch

from chainer_mask_rcnn_amd import streams
from chainer_mask_rcnn_amd.models import mask_rcnn_train_chain

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_three_distinct_streams_each_created_once(dev):
    getters = (streams.copy_stream, streams.wgrad_stream, streams.defer_stream)
    got = [g(dev) for g in getters]
    current = torch.cuda.current_stream(dev)
    assert len(set(s.cuda_stream for s in got + [current])) == 4
    assert all(s.device == dev for s in got)
    for g, s in zip(getters, got):
        assert g(dev) is s
    assert streams.wgrad_stream_if_used(dev) is got[1]
    assert mask_rcnn_train_chain.copy_stream(dev) is got[0]
    assert mask_rcnn_train_chain.copy_stream is streams.copy_stream


_CHILD = '''
import torch
from chainer_mask_rcnn_amd import streams
dev = torch.device('cuda:0')
assert streams.wgrad_stream_if_used(dev) is None
copy, defer = streams.copy_stream(dev), streams.defer_stream(dev)
assert copy is not defer
assert streams.wgrad_stream_if_used(dev) is None, 'another getter created the weight-gradient stream'
streams.join_wgrad_stream()                     # nothing to join, nothing created
assert streams.wgrad_stream_if_used(dev) is None
side = streams.wgrad_stream(dev)
assert streams.wgrad_stream_if_used(dev) is side and side not in (copy, defer)
print('lazy ok')
'''


def test_weight_gradient_stream_exists_only_once_it_was_asked_for(dev):
    """In a fresh process: no earlier test can have created the stream."""
    r = subprocess.run([sys.executable, '-c', _CHILD], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and 'lazy ok' in r.stdout, r.stderr[-2000:]
