"""`autograd.LinearFn` with act=1 (the FFN's first linear, ReLU derivative taken from the output) against torch's CPU autograd in fp64.
Bound per tensor as in tests/test_rnn_train_gpu.py: err = max|g - g64| / max|g64| <= max(8 err_torch32, n 2^-24), n = max(M, K, N)."""
import numpy as np
import pytest
import torch

from tests.helpers_reg_train import U, rel_err
from video2music_amd.autograd import LinearFn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def torch_cpu(x, w, b, dy, dtype):
    t = [torch.from_numpy(v).to(dtype).requires_grad_(True) for v in (x, w, b)]
    y = torch.relu(torch.nn.functional.linear(*t))
    y.backward(torch.from_numpy(dy).to(dtype))
    return [y.detach().numpy()] + [v.grad.numpy() for v in t]


@pytest.mark.parametrize("M,K,N", [(2, 32, 3), (37, 64, 100), (300, 128, 256)])
def test_relu_linear_gradients(M, K, N):
    rng = np.random.default_rng(M + K + N)
    x, w = rng.standard_normal((M, K)).astype(np.float32), (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b, dy = (0.1 * rng.standard_normal(N)).astype(np.float32), rng.standard_normal((M, N)).astype(np.float32)
    g64, g32 = torch_cpu(x, w, b, dy, torch.float64), torch_cpu(x, w, b, dy, torch.float32)
    t = [torch.from_numpy(v).to(DEV).requires_grad_(True) for v in (x, w, b)]
    y = LinearFn.apply(t[0], t[1], t[2], 1)
    y.backward(torch.from_numpy(dy).to(DEV))
    got = [y.detach().cpu().numpy()] + [v.grad.cpu().numpy() for v in t]
    for name, a, w64, w32 in zip(("y", "dx", "dw", "db"), got, g64, g32):
        err, e32 = rel_err(a, w64), rel_err(w32, w64)
        assert err <= max(8 * e32, max(M, K, N) * U), (name, err, e32)
