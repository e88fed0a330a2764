"""amt_layernorm_bwd (csrc/norm_bwd.hip, norm_bwd_kernel<false>) through `autograd.LayerNormFn` against torch's CPU autograd in fp64 on
F.layer_norm(x (+ resid), w, b): the gradients of x, resid, w and b.

Bound per tensor, the one tests/test_rnn_train_gpu.py established: err = max|g - g64| / max|g64| <= max(8 err_torch32, n 2^-24), with
err_torch32 torch's own fp32 CPU autograd on the same inputs and n the longest sum's length: `dim` values inside a row (the statistics
and the two means of dx), `rows` terms of a column of dw / db -- n = max(rows, dim).

Every third row of x (and resid) is scaled by SMALL = 3e-3, so that its variance is near eps: on rows of unit variance no epsilon shows
(test_a_wrong_epsilon_shows_on_the_small_variance_rows_only).

EDGE_CASES: the row counts at which the launcher's plan changes (one workgroup to several, 16 rows per workgroup to the even spread), asked
from its own rule, at dim 4 (one lane of a wave has a column) and dim 260 (one lane in the second float4 chunk)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers_family_train import norm_bwd_plan_boundaries
from tests.helpers_reg_train import U, rel_err
from video2music_amd import _lib, ops
from video2music_amd.autograd import LayerNormFn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
SMALL = 3e-3                            # rows 1, 4, 7, ... of x and resid: variance about 1e-5, the epsilon itself
CASES = [(rows, dim, resid) for rows in (1, 37, 600) for dim in (32, 100, 512, 1024) for resid in (False, True)]
EDGE_ROWS = (16, 17, 2048, 2049)
EDGE_CASES = [(rows, dim, resid) for rows in EDGE_ROWS for dim in (4, 260) for resid in (False, True)]


def inputs(rows, dim, resid):
    rng = np.random.default_rng(1000 * rows + dim + int(resid))
    a = {"x": rng.standard_normal((rows, dim)), "w": 1.0 + 0.3 * rng.standard_normal(dim), "b": 0.1 * rng.standard_normal(dim),
         "dy": rng.standard_normal((rows, dim))}
    if resid:
        a["resid"] = 0.5 * rng.standard_normal((rows, dim))
        a["resid"][1::3] *= SMALL
    a["x"][1::3] *= SMALL
    return {k: v.astype(np.float32) for k, v in a.items()}


def torch_cpu(a, dtype, eps=EPS):
    t = {k: torch.from_numpy(v).to(dtype).requires_grad_(k != "dy") for k, v in a.items()}
    u = t["x"] + t["resid"] if "resid" in t else t["x"]
    y = F.layer_norm(u, (u.shape[1],), t["w"], t["b"], eps)
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


def test_edge_rows_are_the_plan_rules_boundaries():
    assert norm_bwd_plan_boundaries() == list(EDGE_ROWS)


@pytest.mark.parametrize("rows,dim,resid", CASES + EDGE_CASES)
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


@pytest.mark.parametrize("rows,dim,resid", [(37, 100, True), (600, 512, False), (600, 1024, True)])
def test_a_wrong_epsilon_shows_on_the_small_variance_rows_only(rows, dim, resid):
    """Host side, fp64: eps = 1e-6 in place of 1e-5 misses the bound of test_gradients_against_fp64 by over 10 times on the rows scaled
    by SMALL, in y and in dx alike, and stays inside it on the rows of unit variance -- the rows these cases had before."""
    a = inputs(rows, dim, resid)
    g64, g32, wrong = torch_cpu(a, torch.float64), torch_cpu(a, torch.float32), torch_cpu(a, torch.float64, eps=1e-6)
    small = np.zeros(rows, dtype=bool)
    small[1::3] = True
    for k in ("y", "x"):
        bound = max(8 * rel_err(g32[k], g64[k]), max(rows, dim) * U)
        d = np.abs(wrong[k] - g64[k]).max(axis=1) / np.abs(g64[k]).max()
        assert d[small].max() >= 10 * bound and d[~small].max() <= bound, (k, d[small].max(), d[~small].max(), bound)


def test_more_rows_than_the_workgroup_cap_spreads():
    """The first row count past the rule's cap of workgroups times 16 rows: the rows are spread evenly (17 per workgroup) and the last
    workgroups get none."""
    rows = norm_bwd_plan_boundaries()[-1]
    blocks = ops.norm_bwd_blocks(rows)
    per = -(-rows // blocks)
    assert blocks == ops.norm_bwd_blocks(10 * rows) and per == 17 and (blocks - 1) * per >= rows
    a = inputs(rows, 64, True)
    g64, g32, got = torch_cpu(a, torch.float64), torch_cpu(a, torch.float32), device(a)
    for k in g64:
        err, e32 = rel_err(got[k], g64[k]), rel_err(g32[k], g64[k])
        assert err <= max(8 * e32, rows * U), (k, err, e32)


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
