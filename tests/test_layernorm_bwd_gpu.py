"""amt_layernorm_bwd (csrc/layernorm_bwd.hip) through `autograd.LayerNormFn` against torch's CPU autograd in fp64 on
F.layer_norm(x (+ resid), w, b): the gradients of x, resid, w and b.

Bound per tensor, the one tests/test_rnn_train_gpu.py established: err = max|g - g64| / max|g64| <= max(8 err_torch32, n 2^-24), with
err_torch32 torch's own fp32 CPU autograd on the same inputs and n the longest sum's length: `dim` values inside a row (the statistics
and the two means of dx), `rows` terms of a column of dw / db -- n = max(rows, dim)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers_reg_train import U, rel_err
from video2music_amd import _lib, ops
from video2music_amd.autograd import LayerNormFn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
CASES = [(rows, dim, resid) for rows in (1, 37, 600) for dim in (32, 100, 512, 1024) for resid in (False, True)]


def inputs(rows, dim, resid):
    rng = np.random.default_rng(1000 * rows + dim + int(resid))
    a = {"x": rng.standard_normal((rows, dim)), "w": 1.0 + 0.3 * rng.standard_normal(dim), "b": 0.1 * rng.standard_normal(dim),
         "dy": rng.standard_normal((rows, dim))}
    if resid:
        a["resid"] = 0.5 * rng.standard_normal((rows, dim))
    return {k: v.astype(np.float32) for k, v in a.items()}


def torch_cpu(a, dtype):
    t = {k: torch.from_numpy(v).to(dtype).requires_grad_(k != "dy") for k, v in a.items()}
    u = t["x"] + t["resid"] if "resid" in t else t["x"]
    y = F.layer_norm(u, (u.shape[1],), t["w"], t["b"], EPS)
    y.backward(t["dy"])
    out = {k: t[k].grad.numpy() for k in t if k != "dy"}
    out["y"] = y.detach().numpy()
    return out


def device(a):
    t = {k: torch.from_numpy(v).to(DEV).requires_grad_(k != "dy") for k, v in a.items()}
    y = LayerNormFn.apply(t["x"], t.get("resid"), t["w"], t["b"], EPS)
    y.backward(t["dy"])
    torch.cuda.synchronize()
    out = {k: t[k].grad.cpu().numpy() for k in t if k != "dy"}
    out["y"] = y.detach().cpu().numpy()
    return out


@pytest.mark.parametrize("rows,dim,resid", CASES)
def test_gradients_against_fp64(rows, dim, resid):
    a = inputs(rows, dim, resid)
    g64, g32, got = torch_cpu(a, torch.float64), torch_cpu(a, torch.float32), device(a)
    again = device(a)
    for k in g64:
        assert np.array_equal(got[k], again[k]), k                       # fixed summation order: equal bits on repeat
        err, e32 = rel_err(got[k], g64[k]), rel_err(g32[k], g64[k])
        bound = max(8 * e32, max(rows, dim) * U)
        print(f"rows {rows} dim {dim} resid {resid} {k}: err {err:.3e} torch32 {e32:.3e} bound {bound:.3e}")
        assert err <= bound, (k, err, e32, bound)
    if resid:
        assert np.array_equal(got["x"], got["resid"])                    # one gradient for both addends


def test_more_rows_than_the_workgroup_cap_spreads():
    """rows = 2049 > 128 workgroups x 16 rows: the rows are spread evenly (17 per workgroup) and the last workgroups get none."""
    a = inputs(2049, 64, True)
    g64, g32, got = torch_cpu(a, torch.float64), torch_cpu(a, torch.float32), device(a)
    for k in g64:
        err, e32 = rel_err(got[k], g64[k]), rel_err(g32[k], g64[k])
        assert err <= max(8 * e32, 2049 * U), (k, err, e32)


def test_bad_arguments():
    t = torch.zeros(4, 32, device=DEV)
    w = torch.zeros(32, device=DEV)
    ws = torch.zeros(4 + 256 * 32, device=DEV)
    P = _lib.ptr
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_layernorm_bwd", P(t), P(t), None, P(w), P(t), P(w), P(w), None, 4, 32, EPS, None)
    with pytest.raises(_lib.AmtError, match="dim=30"):
        _lib.call("amt_layernorm_bwd", P(t), P(t), None, P(w), P(t), P(w), P(w), P(ws), 4, 30, EPS, None)
    with pytest.raises(_lib.AmtError, match="dim=1028"):
        _lib.call("amt_layernorm_bwd", P(t), P(t), None, P(w), P(t), P(w), P(w), P(ws), 4, 1028, EPS, None)
    with pytest.raises(_lib.AmtError, match="rows=0"):
        _lib.call("amt_layernorm_bwd", P(t), P(t), None, P(w), P(t), P(w), P(w), P(ws), 0, 32, EPS, None)
