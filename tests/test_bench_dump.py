"""bench.py --dump-outputs (CPU part): the writer of the last timed step's outputs -- losses as float64 scalars, gradients (and
updated parameters) as float32, tensors above the per-tensor share of the budget as a fixed seeded sample, the same files from run
to run, within the size budget."""
import os

import numpy as np
import torch

import bench


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.big = torch.nn.Parameter(torch.randn(4096, 2048))
        self.small = torch.nn.Parameter(torch.randn(7))
        self.unused = torch.nn.Parameter(torch.zeros(3))


def _dump(tmp_path, tag, m, with_params):
    d = tmp_path / tag
    bench.dump_outputs(str(d), {'loss_total': torch.tensor(1.25), 'EgoNCE': torch.tensor(0.5)}, m, with_params)
    return {f: np.load(d / f) for f in sorted(os.listdir(d))}, sum(os.path.getsize(d / f) for f in os.listdir(d))


def test_dump_outputs_is_seeded_typed_and_bounded(tmp_path):
    torch.manual_seed(0)
    m = _Net()
    m.big.grad = torch.randn(4096, 2048)
    m.small.grad = torch.randn(7)
    a, size = _dump(tmp_path, 'a', m, True)
    b, _ = _dump(tmp_path, 'b', m, True)
    assert sorted(a) == ['EgoNCE.npy', 'grad.big.npy', 'grad.small.npy', 'loss_total.npy',
                         'param.big.npy', 'param.small.npy', 'param.unused.npy']           # no file for a None gradient
    assert size <= 64 << 20
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a['loss_total.npy'].dtype == np.float64 and float(a['loss_total.npy']) == 1.25
    assert np.array_equal(a['grad.small.npy'], m.small.grad.numpy())                       # small tensors whole
    per_tensor = bench.DUMP_BUDGET_BYTES // 4 // (2 * 3)
    g = a['grad.big.npy']
    assert per_tensor < m.big.numel() and g.dtype == np.float32 and g.shape == (per_tensor,)
    assert np.isin(g, m.big.grad.numpy().reshape(-1)).all()                               # a sample of the tensor's own elements
