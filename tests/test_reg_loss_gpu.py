"""amt_reg_loss_fwd_bwd (csrc/reg_loss.hip) against the fp64 restatement `helpers_reg_train.loss64`.

The kernel is fed as training feeds it: ln_nd and the probabilities come from the device's own head GEMMs over the inputs of
`helpers_reg_eval.make_case`; the restatement forms both heads in fp64 from the same fp32 inputs.  Bounds, with delta the head-value
bound of `helpers_reg_eval.heads64` ((W + 2) 2^-24 (sum |x w| + |b|)) and U = 2^-24:

  d_ln_nd      4 U |g| + delta_y / (2 rows)                       |d SmoothL1' / de| <= 1
  d_logit      4 U |g| + (delta_z / 4 + 4 U) / (40 rows)          g = (p - t) / N, |dp / dz| <= 1/4, the fp32 sigmoid a few ulps of p
  loss         SmoothL1: sum (min(|e|, 1) delta_y + delta_y^2 / 2 + 4 U term) + n U sum, over 2 rows
               BCE: the form of `helpers_reg_eval.restate`: sum (delta_z + 4 U / min(p, 1 - p) + 4 U |term|) + n U sum, over 40 rows
               n = the longest chain of additions a value goes through: its thread's values (the count over 1024 threads of each of the
               min(256, ceil(40 rows / 4096)) workgroups), 6 in the wave, 16 over the waves, then one per workgroup
               and 4 U |loss| for the two divisions and the final add."""
import numpy as np
import pytest
import torch

from tests import helpers_reg_eval as H
from tests.helpers_reg_train import U, loss64
from video2music_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = 40
CASES = [(1, 1), (1, 5), (1, 63), (1, 64), (1, 65), (3, 300)]           # rows = B S: 1, 5, 63, 64, 65, 900


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def heads_on_device(c):
    rows = c["feat"].shape[0] * c["feat"].shape[1]
    x = dev(c["feat"].reshape(rows, -1))
    Kp = (x.shape[1] + 31) // 32 * 32
    pad = lambda t: torch.nn.functional.pad(t, (0, Kp - t.shape[1])).contiguous()
    ln_nd = ops.linear_ex(pad(x), pad(dev(c["reg_w"])), dev(c["reg_b"]))
    p = ops.linear_ex(pad(x), pad(dev(c["cls_w"])), dev(c["cls_b"]), act=2)
    return ln_nd, p


def targets(c):
    rows = c["feat"].shape[0] * c["feat"].shape[1]
    return dev(c["note_density"].reshape(rows)), dev(c["loudness"].reshape(rows)), dev(c["instrument"].reshape(rows, 40))


def chain_length(count, rows):
    nb = min(256, -(-40 * rows // 4096))
    return -(-count // (1024 * nb)) + 1 + 6 + 16 + nb


def bounds(c, want, h):
    rows = want["sl1"].shape[0]
    dy, dz = h["d_ln_nd"].reshape(rows, 2), h["d_z"].reshape(rows, 40)
    e = np.abs(h["ln_nd"].reshape(rows, 2) - np.stack([c["note_density"].reshape(-1), c["loudness"].reshape(-1)], 1).astype(np.float64))
    p = 1.0 / (1.0 + np.exp(-h["z"].reshape(rows, 40)))
    chain = lambda count: chain_length(count, rows)
    sl1 = (np.minimum(e, 1.0) * dy + dy * dy / 2 + 4 * U * want["sl1"]).sum() + chain(2 * rows) * U * want["sl1"].sum()
    bce = (dz + 4 * U / np.minimum(p, 1 - p) + 4 * U * np.abs(want["bce"])).sum() + chain(40 * rows) * U * want["bce"].sum()
    return {"loss": sl1 / (2 * rows) + bce / (40 * rows) + 4 * U * abs(want["loss"]),
            "d_ln_nd": 4 * U * np.abs(want["d_ln_nd"]) + dy / (2 * rows),
            "d_logit": 4 * U * np.abs(want["d_logit"]) + (dz / 4 + 4 * U) / (40 * rows)}


@pytest.mark.parametrize("B,S", CASES)
def test_kernel_equals_fp64_restatement_and_torch_on_the_device(B, S):
    c = H.make_case(B, S, W)
    h = H.heads64(c["feat"], c["reg_w"], c["reg_b"], c["cls_w"], c["cls_b"])
    want = loss64(h["ln_nd"], 1.0 / (1.0 + np.exp(-h["z"])), c["note_density"], c["loudness"], c["instrument"])
    bd = bounds(c, want, h)
    ln_nd, p = heads_on_device(c)
    nd, lo, inst = targets(c)
    loss, d_ln_nd, d_logit = ops.reg_loss(ln_nd, p, nd, lo, inst)
    loss2, d2, d3 = ops.reg_loss(ln_nd, p, nd, lo, inst)
    assert torch.equal(loss, loss2) and torch.equal(d_ln_nd, d2) and torch.equal(d_logit, d3)     # fixed summation order
    got = {"loss": float(loss[0]), "d_ln_nd": d_ln_nd.cpu().numpy().astype(np.float64), "d_logit": d_logit.cpu().numpy().astype(np.float64)}
    for k in ("loss", "d_ln_nd", "d_logit"):
        ratio = np.max(np.abs(got[k] - want[k]) / bd[k])
        print(f"rows {B * S} {k}: max error / bound = {ratio:.3f}")
        assert ratio <= 1.0, k
    assert abs(float(loss[1]) + float(loss[2]) - float(loss[0])) <= 2 * U * float(loss[0])
    # the torch expressions of train_epoch on the same device tensors, their gradients taken through the sigmoid by hand
    y, q = ln_nd.clone().requires_grad_(True), p.clone().requires_grad_(True)
    tl = torch.nn.SmoothL1Loss()(y, torch.stack([nd, lo], dim=1)) + torch.nn.functional.binary_cross_entropy(q, inst)
    tl.backward()
    assert abs(float(tl) - want["loss"]) <= bd["loss"] and abs(float(tl) - got["loss"]) <= bd["loss"]
    assert (np.abs(y.grad.cpu().numpy() - got["d_ln_nd"]) <= bd["d_ln_nd"]).all()
    assert (np.abs((q.grad * q.detach() * (1 - q.detach())).cpu().numpy() - got["d_logit"]) <= bd["d_logit"]).all()


def test_both_sides_of_the_smooth_l1_knee_and_at_it():
    """|e| = 0.5, 1 - 2^-24, 1, 1 + 2^-23, 1.5 with either sign: exact inputs, so 4 U relative on every value."""
    e = np.array([0.5, 1 - 2.0 ** -24, 1.0, 1 + 2.0 ** -23, 1.5, -0.5, -(1 - 2.0 ** -24), -1.0, -(1 + 2.0 ** -23), -1.5], dtype=np.float32)
    rows = e.size // 2
    ln_nd = dev(e.reshape(rows, 2))
    zero = torch.zeros(rows, device=DEV)
    p, t = torch.full((rows, 40), 0.5, device=DEV), torch.zeros(rows, 40, device=DEV)
    loss, d_ln_nd, d_logit = ops.reg_loss(ln_nd, p, zero, zero, t)
    want = loss64(e.reshape(rows, 2), np.full((rows, 40), 0.5), np.zeros(rows), np.zeros(rows), np.zeros((rows, 40)))
    assert (np.abs(d_ln_nd.cpu().numpy() - want["d_ln_nd"]) <= 4 * U * np.abs(want["d_ln_nd"])).all()
    one = float(np.float32(1.0) / np.float32(2 * rows))
    assert float(d_ln_nd[1, 0]) == one and float(d_ln_nd[3, 1]) == -one      # |e| = 1: sign(e), which equals e
    assert abs(float(loss[1]) - want["sl1"].mean()) <= 16 * U * want["sl1"].mean()
    assert abs(float(loss[2]) - np.log(2.0)) <= 16 * U and (d_logit.cpu().numpy() == np.float32(0.5) / np.float32(40 * rows)).all()


def test_saturated_probabilities():
    """p rounded to 0 or 1: the wrong side's term is exactly 100 (the clamp), the right side's exactly 0, the logit gradient exactly 0."""
    rows = 3
    p = torch.zeros(rows, 40, device=DEV)
    p[:, ::2] = 1.0
    t = 1.0 - p                                         # every probability on the wrong side
    t[2] = p[2]                                         # but the last row's
    y = torch.zeros(rows, 2, device=DEV)
    zero = torch.zeros(rows, device=DEV)
    loss, _, d_logit = ops.reg_loss(y, p, zero, zero, t)
    assert not d_logit.any()
    assert float(loss[1]) == 0.0 and float(loss[2]) == np.float32(8000.0) / np.float32(120.0) and float(loss[0]) == float(loss[2])
    p[1, 0], t[1, 0] = 1.0e-20, 0.0                     # below the 1e-12 floor of p (1 - p): torch's own quotient, not (p - t) / N
    _, _, d_logit = ops.reg_loss(y, p, zero, zero, t)
    want = loss64(np.zeros((rows, 2)), p.cpu().numpy(), np.zeros(rows), np.zeros(rows), t.cpu().numpy())
    assert abs(float(d_logit[1, 0]) - want["d_logit"][1, 0]) <= 8 * U * want["d_logit"][1, 0] and float(d_logit[1, 0]) < 1e-20


def test_more_values_than_256_workgroups_of_4096():
    """rows = 27000: 1.08 M instrument values, the workgroup count capped at 256, five values per thread.  Exact inputs, so the gradients
    are held to 4 U relative (8 U for the logit's: torch's own order of operations has seven roundings) and the loss to its chain."""
    rows = 27000
    rng = np.random.default_rng(8)
    y = rng.uniform(-3, 3, (rows, 2)).astype(np.float32)
    p = rng.uniform(0.01, 0.99, (rows, 40)).astype(np.float32)
    t = (rng.random((rows, 40)) < 0.3).astype(np.float32)
    nd, lo = rng.uniform(0, 2, rows).astype(np.float32), rng.uniform(0, 2, rows).astype(np.float32)
    want = loss64(y, p, nd, lo, t)
    a, b = ops.reg_loss(dev(y), dev(p), dev(nd), dev(lo), dev(t)), ops.reg_loss(dev(y), dev(p), dev(nd), dev(lo), dev(t))
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    loss, d_ln_nd, d_logit = a
    assert (np.abs(d_ln_nd.cpu().numpy() - want["d_ln_nd"]) <= 4 * U * np.abs(want["d_ln_nd"]) + U / (2 * rows)).all()      # e = y - t rounds once
    assert (np.abs(d_logit.cpu().numpy() - want["d_logit"]) <= 8 * U * np.abs(want["d_logit"])).all()
    p64 = p.astype(np.float64)
    sl1 = (4 * U * (want["sl1"] + np.abs(y))).sum() + chain_length(2 * rows, rows) * U * want["sl1"].sum()
    bce = (4 * U / np.minimum(p64, 1 - p64) + 4 * U * want["bce"]).sum() + chain_length(40 * rows, rows) * U * want["bce"].sum()
    bound = sl1 / (2 * rows) + bce / (40 * rows) + 4 * U * want["loss"]
    print("rows 27000 loss error / bound", abs(float(loss[0]) - want["loss"]) / bound)
    assert abs(float(loss[0]) - want["loss"]) <= bound


def test_bad_arguments():
    t = torch.zeros(4, 40, device=DEV)
    ws = torch.zeros(ops.REG_LOSS_WS_FLOATS, device=DEV)
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_reg_loss_fwd_bwd", _lib.ptr(t), None, _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), 1, _lib.ptr(t), _lib.ptr(t), _lib.ptr(t),
                  _lib.ptr(ws), None)
    with pytest.raises(_lib.AmtError, match="null pointer"):
        _lib.call("amt_reg_loss_fwd_bwd", *([_lib.ptr(t)] * 5), 1, _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), None, None)
    with pytest.raises(_lib.AmtError, match="rows=0"):
        _lib.call("amt_reg_loss_fwd_bwd", *([_lib.ptr(t)] * 5), 0, _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(ws), None)
